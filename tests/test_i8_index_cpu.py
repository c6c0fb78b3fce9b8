"""The int8 corpus dtype (``FlatIndex(d, dtype="i8")``) without a device: its C ABI ``dtype`` code, the shapes its fused
scan serves, ``quantize_i8`` against a numpy restatement, the integer-valued check on float input, the scan policy, the
argument checks of every C entry point that takes ``dtype``, and the canonical score at the 2^24 edge.

The code is 6, not 5: tests/test_f16_index_cpu.py passes 5 to every entry point as a value that must stay invalid (and
pins ``index.DTYPE_CODE`` to the three float formats, so the int8 code lives in ``index.INT_DTYPE_CODE``)."""
import functools
import os
import re
import sys

import numpy as np
import pytest

P = 1 << 20                     # a 256-byte aligned stand-in for device pointers: never dereferenced
I8 = 6
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))


@pytest.fixture(scope="module")
def L():
    import sessionsimilaritysearch_amd as pkg
    return pkg.lib()


def test_dtype_code_and_fused_dims():
    import torch
    from sessionsimilaritysearch_amd import _lib, index as ix
    assert ix.INT_DTYPE_CODE == {"i8": I8}
    assert ix._CODE == {"f32": 0, "bf16": 1, "f16": 4, "i8": I8}
    assert ix.FUSED_DIMS["i8"] == (256, 512, 1024)          # row bytes 256 / 512 / 1024 at one byte per element
    assert ix._TORCH_DTYPE["i8"] == torch.int8
    try:                                                    # construction validates before it asks for a device
        idx = ix.FlatIndex(256, "ip", dtype="i8")
        assert idx._tdtype == torch.int8 and idx.scan == "native"
    except _lib.SssError as e:
        assert "no HIP device" in str(e)
    for d in (8, 24, 250, 1608):                            # 16-byte row pieces hold 16 elements
        with pytest.raises(ValueError):
            ix.FlatIndex(d, "ip", dtype="i8")
    with pytest.raises(ValueError):
        ix.FlatIndex(256, "ip", dtype="i8", scan="f16")     # the derived images belong to a float32 index
    with pytest.raises(ValueError):
        ix.FlatIndex(256, "cos", dtype="i8")


def test_header_documents_the_code_and_declares_what_the_binding_declares():
    from sessionsimilaritysearch_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "sss.h")).read()
    assert f"dtype {I8}" in hdr and "int8" in hdr and "v_mfma_i32_32x32x32_i8" in hdr
    assert "5 is unassigned" in hdr
    declared = set(re.findall(r"\b(sss_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)))
    assert declared == set(_lib.exported_symbols())         # no new C symbol, none lost


def _np_quantize(x, scale=None):
    x = np.asarray(x, np.float32)
    if scale is None:
        amax = float(np.abs(x).max()) if x.size else 0.0
        scale = 127.0 / amax if amax > 0 else 1.0
    y = np.rint(x * np.float32(scale))                      # float32 product, round half to even
    return np.clip(y, -127, 127).astype(np.int8), float(scale)


def test_quantize_i8_against_numpy():
    import torch
    from sessionsimilaritysearch_amd.index import quantize_i8
    rng = np.random.default_rng(0)
    x = rng.standard_normal((37, 48)).astype(np.float32)
    codes, scale = quantize_i8(x)
    ec, es = _np_quantize(x)
    assert codes.dtype == np.int8 and isinstance(scale, float) and scale == es
    assert np.array_equal(codes, ec) and np.abs(codes).max() == 127 and codes.min() >= -127
    # round half to even, and the clip at +-127 (never -128)
    h = np.array([[0.5, 1.5, 2.5, -0.5, -1.5, -2.5, 126.5, 127.5, -127.5, -128.0, 300.0, -300.0, 1e9, -1e9, 0.49, -0.51]], np.float32)
    codes, scale = quantize_i8(h, 1.0)
    assert scale == 1.0
    assert codes.tolist() == [[0, 2, 2, 0, -2, -2, 126, 127, -127, -127, 127, -127, 127, -127, 0, -1]]
    assert np.array_equal(codes, _np_quantize(h, 1.0)[0])
    codes, _ = quantize_i8(x, 10.0)
    assert np.array_equal(codes, _np_quantize(x, 10.0)[0])
    # an all-zero input: scale 1, all-zero codes
    z, zs = quantize_i8(np.zeros((3, 16), np.float32))
    assert zs == 1.0 and z.dtype == np.int8 and not z.any()
    # a tensor in -> a tensor out, the same codes
    t, ts = quantize_i8(torch.from_numpy(x))
    assert isinstance(t, torch.Tensor) and t.dtype == torch.int8 and ts == es and np.array_equal(t.numpy(), ec)


def test_integer_valued_check_on_host_tensors():
    import torch
    from sessionsimilaritysearch_amd.index import integer_valued_i8
    ok = torch.tensor([[-128.0, -1.0, 0.0, -0.0, 1.0, 127.0]])
    assert bool(integer_valued_i8(ok))
    assert bool(integer_valued_i8(torch.zeros((0, 16))))                       # nothing to refuse
    for bad in (0.5, -0.25, 127.0001, 128.0, -129.0, 1e9, float("inf"), float("-inf"), float("nan"), 1e-30):
        x = ok.clone()
        x[0, 3] = bad
        assert not bool(integer_valued_i8(x)), bad


def test_scan_policy_is_host_logic():
    """scan_for / rung_scan of an i8 index: the fused scan at d = 256 / 512 / 1024 up to k = 500, nothing else -- no
    long-row scan (d = 1600 and every other d go to the exhaustive kernels), no L2."""
    from routing_stub import make_routing
    Stub = functools.partial(make_routing, dtype="i8")      # no device: only the policy

    for d in (256, 512, 1024):
        assert [Stub(d).scan_for(k) for k in (1, 10, 100, 500, 501, 600)] == ["native"] * 4 + ["", ""]
        assert Stub(d).rung_scan() == "native"
    for d in (16, 48, 128, 1600, 2048, 8192):
        assert Stub(d).scan_for(10) == "" and Stub(d).rung_scan() == "" and Stub(d)._long_or_none(10) == ""
    assert Stub(1600, dtype="f16").scan_for(10) == "long"    # (the 16-bit formats keep theirs)
    assert Stub(256, "l2").scan_for(10) == "" and Stub(256, "l2").rung_scan() == "" and Stub(256, n=0).scan_for(10) == ""
    assert Stub(256).next_scan("native") == ""


def test_workspace_sizes_of_the_int8_code_equal_those_of_bf16_at_the_same_row_bytes(L):
    for d in (256, 512, 1024):
        for nq, n, k in ((1, 1000, 1), (33, 200_000, 10), (1024, 1_000_000, 10), (1024, 200_000, 500)):
            assert L.sss_ip_topk_workspace_bytes(nq, n, d, k, I8) == L.sss_ip_topk_workspace_bytes(nq, n, d // 2, k, 1) > 0
            assert L.sss_ip_topk_threshold_workspace_bytes(nq, n, d, I8) == L.sss_ip_topk_threshold_workspace_bytes(nq, n, d // 2, 1) > 0
            assert L.sss_range_search_workspace_bytes(nq, n, d, I8) == L.sss_range_search_workspace_bytes(nq, n, d // 2, 1) > 0
    for d in (16, 64, 128, 384, 1600, 2048):                # no fused scan of that row size (128-byte rows included)
        assert L.sss_ip_topk_workspace_bytes(16, 1000, d, 10, I8) == 0
        assert L.sss_ip_topk_threshold_workspace_bytes(16, 1000, d, I8) == 0
        assert L.sss_range_search_workspace_bytes(16, 1000, d, I8) == 0
    for d in (1600, 1024, 4096):                            # no long-row scan at all
        assert L.sss_ip_topk_long_workspace_bytes(16, 1000, d, I8) == 0
    assert L.sss_ip_topk_exhaustive_workspace_bytes(4, 1000) > 0


def _guards(L):
    """name -> call(dtype, d): each entry point that takes `dtype`, with arguments that are valid but for a workspace (or
    state) too small -- a call that passes every argument check returns -2 and never launches."""
    def topk(dt, d=256):
        return L.sss_ip_topk(P, 4, P, 1000, d, 10, dt, 0, 1.0, P, P, P, 0, P, 16, P, 1 << 30, 0)

    def threshold(dt, d=256, scan=None):
        return L.sss_ip_topk_threshold(P, P, 4, P, dt, P, dt if scan is None else scan, 0, 0.0, 1000, d, 10, 0, 1.0, P, P, P, P, 256, 0)

    def exhaustive(dt, d=48):
        return L.sss_ip_topk_exhaustive(P, P, 4, P, 1000, d, 10, dt, 0, 0, P, P, P, 256, 0)

    def exhaustive_lb(dt, d=48):
        return L.sss_ip_topk_exhaustive_lb(P, P, 4, P, 1000, d, 10, dt, 0, P, P, P, P, 256, 0)

    def range_count(dt, d=256, scan=None):
        return L.sss_range_search_count(P, 4, P, dt, P, dt if scan is None else scan, 0, 0.0, 1000, d, P, 1.0, P, P, P, 256, 0)

    def range_ex_count(dt, d=48):
        return L.sss_range_search_exhaustive_count(P, P, 4, P, 1000, d, dt, 1, P, P, P, 256, 0)

    return {"sss_ip_topk": topk, "sss_ip_topk_threshold": threshold, "sss_ip_topk_exhaustive": exhaustive,
            "sss_ip_topk_exhaustive_lb": exhaustive_lb, "sss_range_search_count": range_count,
            "sss_range_search_exhaustive_count": range_ex_count}


@pytest.mark.parametrize("entry", ["sss_ip_topk", "sss_ip_topk_threshold", "sss_ip_topk_exhaustive", "sss_ip_topk_exhaustive_lb",
                                   "sss_range_search_count", "sss_range_search_exhaustive_count"])
def test_the_int8_code_passes_the_argument_checks(L, entry):
    call = _guards(L)[entry]
    assert call(I8) == -2, L.sss_last_error()               # valid but for the workspace / state
    assert call(I8, d=1600 if "exhaustive" in entry else 512) == -2, L.sss_last_error()
    assert call(I8, d=24) == -1                             # 16-byte row pieces: d % 16 == 0
    assert call(I8, d=8) == -1
    if "exhaustive" not in entry:
        assert call(I8, d=128) == -1 and call(I8, d=1600) == -1      # no fused scan of those rows
    assert call(5) == -1                                    # still unassigned


def test_scan_code_goes_with_the_dtype(L):
    g = _guards(L)
    for entry in ("sss_ip_topk_threshold", "sss_range_search_count"):
        for scan in (0, 1, 2, 3, 4, 5):
            assert g[entry](I8, scan=scan) == -1, (entry, scan)
        for dt in (0, 1, 4):
            assert g[entry](dt, scan=I8) == -1, (entry, dt)


def test_long_rows_refuse_int8_with_a_message(L):
    rc = L.sss_ip_topk_long(P, 4, P, I8, P, 0, 0.0, 1000, 1600, 100, 0, 1.0, P, P, P, P, 1 << 30, 0)
    assert rc == -1
    msg = L.sss_last_error().decode()
    assert "int8" in msg and "long" in msg, msg


def test_row_norm_max_takes_the_int8_code(L):
    assert L.sss_row_norm_max(P, 0, 256, I8, P, 0) == 0     # n = 0: nothing to do, after the argument checks
    assert L.sss_row_norm_max(P, 0, 48, I8, P, 0) == 0
    assert L.sss_row_norm_max(P, 0, 24, I8, P, 0) == -1 and L.sss_row_norm_max(P, 0, 8, I8, P, 0) == -1
    assert L.sss_row_norm_max(P, 0, 256, 5, P, 0) == -1


def test_canonical_score_at_the_magnitude_edge_is_exact_in_float32():
    """d = 1024, every element -128: the score is 1024 * 2^14 = 2^24, the largest an int8 fused shape can produce -- an
    integer float32 still holds (as it holds every integer below it), so the oracle's float64 chain rounds nowhere."""
    from oracle import search_ref as sr
    q = np.full((2, 1024), -128, np.int8)
    c = np.full((3, 1024), -128, np.int8)
    c[1] = 127
    c[2, ::2] = 127
    s = sr.canonical_scores(q.astype(np.float32), c.astype(np.float32))
    assert s.dtype == np.float32
    assert s[0, 0] == np.float32(2.0 ** 24) and float(s[0, 0]) == 16777216.0
    exact = q.astype(np.int64) @ c.astype(np.int64).T
    assert np.array_equal(s.astype(np.int64), exact) and exact[0, 1] == -1024 * 128 * 127
    D, I = sr.search_exact(q, c, 3)
    assert np.array_equal(I, np.tile(np.array([0, 2, 1]), (2, 1))) and np.array_equal(D.astype(np.int64), np.sort(exact, axis=1)[:, ::-1])
    l2 = sr.canonical_l2(q.astype(np.float32), c.astype(np.float32))
    assert np.array_equal(l2.astype(np.int64), ((q[:, None, :].astype(np.int64) - c[None].astype(np.int64)) ** 2).sum(-1))
