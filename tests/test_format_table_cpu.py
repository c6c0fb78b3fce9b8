"""The storage-format table of ``index.py`` (``_FORMATS``) without a device: every record agrees with the module
dicts the other tests pin and with what libsss.so serves for its code."""
import pytest

PINNED_CODE = {"f32": 0, "bf16": 1, "f16": 4, "i8": 6}          # include/sss.h: dtype
PINNED_ALIGN = {"f32": 4, "bf16": 8, "f16": 8, "i8": 16}        # elements per 16-byte piece of a stored row


@pytest.fixture(scope="module")
def L():
    import sessionsimilaritysearch_amd as pkg
    return pkg.lib()


def test_table_order_and_derived_dicts():
    import torch
    from sessionsimilaritysearch_amd import index as ix
    assert list(ix._FORMATS) == ["f32", "bf16", "f16", "i8"]
    assert ix._CODE == PINNED_CODE
    assert ix.DTYPE_CODE == {"f32": 0, "bf16": 1, "f16": 4} and ix.INT_DTYPE_CODE == {"i8": 6}
    assert ix._TORCH_DTYPE == {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16, "i8": torch.int8}
    assert ix.FUSED_DIMS == {"f32": (64, 128, 256), "bf16": (128, 256, 512), "f16": (128, 256, 512), "i8": (256, 512, 1024)}
    assert ix._EXHAUSTIVE_WS_BYTES == 1 << 30


@pytest.mark.parametrize("name", ["f32", "bf16", "f16", "i8"])
def test_record_agrees_with_the_pinned_dicts(name):
    from sessionsimilaritysearch_amd import _lib, index as ix
    fmt = ix._FORMATS[name]
    assert fmt.name == name and fmt.code == PINNED_CODE[name] == ix._CODE[name]
    assert fmt.torch_dtype == ix._TORCH_DTYPE[name] and fmt.torch_dtype.itemsize == fmt.elem_bytes
    assert 16 // fmt.elem_bytes == fmt.align == PINNED_ALIGN[name]
    assert fmt.fused_dims == ix.FUSED_DIMS[name] == tuple(rb // fmt.elem_bytes for rb in (256, 512, 1024))
    assert fmt.long_rows == (name != "i8") and fmt.checks_finite == (name == "f16")
    assert (fmt.numpy_dtype is None) == (name == "bf16")
    try:                                                    # construction validates before it asks for a device
        idx = ix.FlatIndex(fmt.align, "ip", dtype=name)
        assert idx._fmt is fmt and idx.dtype == name and idx._tdtype == fmt.torch_dtype
    except _lib.SssError as e:
        assert "no HIP device" in str(e)
    if name != "f32":
        with pytest.raises(ValueError):
            ix.FlatIndex(fmt.align + 1, "ip", dtype=name)


@pytest.mark.parametrize("name", ["f32", "bf16", "f16", "i8"])
def test_library_serves_exactly_the_fused_dims(L, name):
    from sessionsimilaritysearch_amd import index as ix
    fmt = ix._FORMATS[name]
    for d in (fmt.align, 64, 128, 256, 512, 1024, 2048):
        nbytes = L.sss_ip_topk_workspace_bytes(32, 1024, d, 10, fmt.code)
        assert (nbytes != 0) == (d in fmt.fused_dims), (name, d, nbytes)
        assert L.sss_ip_topk_workspace_bytes(32, 1024, d, 10, 5) == 0       # 5 stays unassigned
