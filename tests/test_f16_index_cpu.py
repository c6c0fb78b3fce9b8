"""The float16 corpus dtype (``FlatIndex(d, dtype="f16")``, C ABI ``dtype = 4``) without a device: the dtype is accepted,
its scan policy is the bf16 index's, and every C entry point that takes ``dtype`` lets 4 through its host-side argument
checks exactly where it lets 1 through -- while 2 and 3 (scan images of a float32 corpus) and 5 stay rejected."""
import functools
import os
import sys

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))

P = 1 << 20                     # a 256-byte aligned stand-in for device pointers: never dereferenced


@pytest.fixture(scope="module")
def L():
    import sessionsimilaritysearch_amd as pkg
    return pkg.lib()


def test_f16_dtype_is_accepted_as_far_as_the_others():
    """Construction validates (metric, dtype, d, scan) before it asks for a device: with none present an f16 index gets
    as far as an f32 or bf16 one (the no-device error), and is not turned away as an unknown dtype."""
    import torch
    from sessionsimilaritysearch_amd import _lib, index as ix
    assert ix.DTYPE_CODE == {"f32": 0, "bf16": 1, "f16": 4}
    assert ix.FUSED_DIMS["f16"] == (128, 256, 512)
    outcome = {}
    for dtype in ("f32", "bf16", "f16"):
        try:
            idx = ix.FlatIndex(128, "ip", dtype=dtype)
            outcome[dtype] = ("built", idx._tdtype)
        except _lib.SssError as e:
            assert "no HIP device" in str(e)
            outcome[dtype] = ("no device", None)
    assert len({o[0] for o in outcome.values()}) == 1, outcome
    if outcome["f16"][0] == "built":
        assert outcome["f16"][1] == torch.float16
    with pytest.raises(ValueError):
        ix.FlatIndex(128, "ip", dtype="f8")
    with pytest.raises(ValueError):
        ix.FlatIndex(132, "ip", dtype="f16")                # 16-byte row pieces: d % 8 == 0, as bf16
    with pytest.raises(ValueError):
        ix.FlatIndex(128, "ip", dtype="f16", scan="f16")    # the derived images belong to a float32 index
    assert callable(ix.to_f16)


def test_f16_scan_policy_is_host_logic():
    """scan_for / rung_scan of an f16 index: the bf16 index's policy (stored rows are the only scan source)."""
    from routing_stub import make_routing
    Stub = functools.partial(make_routing, dtype="f16")     # no device: only the policy

    for d in (128, 256, 512):
        assert [Stub(d).scan_for(k) for k in (1, 10, 100, 500, 501, 600)] == ["native"] * 4 + ["", ""]
        assert Stub(d).rung_scan() == "native"
    assert [Stub(1600).scan_for(k) for k in (1, 100, 1024, 1025)] == ["long", "long", "long", ""]
    assert Stub(1600).rung_scan() == "" and Stub(8192).scan_for(10) == "long" and Stub(8256).scan_for(10) == ""
    assert Stub(96).scan_for(10) == "" and Stub(96).rung_scan() == ""
    assert Stub(128, "l2").scan_for(10) == "" and Stub(128, "l2").rung_scan() == "" and Stub(128, n=0).scan_for(10) == ""
    assert Stub(128).next_scan("native") == ""
    for d, k in ((128, 10), (256, 500), (512, 1), (1600, 100), (96, 10), (128, 501), (64, 10)):   # the same answers as bf16
        assert Stub(d).scan_for(k) == Stub(d, dtype="bf16").scan_for(k)
    a = Stub(128)
    a.last_scan = "native"
    a._note_fallbacks(10, 1024, 500)                        # no ladder to climb
    assert a.scan_for(10) == "native"


def test_workspace_sizes_of_dtype_4_equal_those_of_bf16(L):
    for d in (128, 256, 512):
        for nq, n, k in ((1, 1000, 1), (33, 200_000, 10), (1024, 1_000_000, 10), (1024, 200_000, 500)):
            assert L.sss_ip_topk_workspace_bytes(nq, n, d, k, 4) == L.sss_ip_topk_workspace_bytes(nq, n, d, k, 1) > 0
            assert L.sss_ip_topk_threshold_workspace_bytes(nq, n, d, 4) == L.sss_ip_topk_threshold_workspace_bytes(nq, n, d, 1) > 0
            assert L.sss_range_search_workspace_bytes(nq, n, d, 4) == L.sss_range_search_workspace_bytes(nq, n, d, 1) > 0
    assert L.sss_ip_topk_long_workspace_bytes(16, 100_000, 1600, 4) == L.sss_ip_topk_long_workspace_bytes(16, 100_000, 1600, 1) > 0
    for d in (64, 96, 12, 1600):
        assert L.sss_ip_topk_workspace_bytes(16, 1000, d, 10, 4) == 0
        assert L.sss_ip_topk_threshold_workspace_bytes(16, 1000, d, 4) == 0
    assert L.sss_ip_topk_long_workspace_bytes(16, 1000, 1616, 4) == 0 and L.sss_ip_topk_long_workspace_bytes(16, 1000, 8256, 4) == 0
    for code in (2, 3, 5, -1):                              # never a corpus dtype
        assert L.sss_ip_topk_workspace_bytes(16, 1000, 128, 10, code) == 0
        assert L.sss_ip_topk_long_workspace_bytes(16, 1000, 1600, code) == 0
    assert L.sss_ip_topk_threshold_workspace_bytes(16, 1000, 128, 5) == 0 and L.sss_range_search_workspace_bytes(16, 1000, 128, 5) == 0


def _guards(L):
    """name -> call(dtype, d=None): each entry point that takes `dtype`, with arguments that are valid but for a workspace
    (or state) one byte class too small -- a call that passes every argument check returns -2 and never launches.  Where
    a `scan` code goes with the dtype it is the dtype's own ("the index's own rows")."""
    def topk(dt, d=128):
        return L.sss_ip_topk(P, 4, P, 1000, d, 10, dt, 0, 1.0, P, P, P, 0, P, 16, P, 1 << 30, 0)

    def threshold(dt, d=128, scan=None):
        return L.sss_ip_topk_threshold(P, P, 4, P, dt, P, dt if scan is None else scan, 0, 0.0, 1000, d, 10, 0, 1.0, P, P, P, P, 256, 0)

    def long_rows(dt, d=1600):
        return L.sss_ip_topk_long(P, 4, P, dt, P, 0, 0.0, 1000, d, 100, 0, 1.0, P, P, P, P, 256, 0)

    def exhaustive(dt, d=96):
        return L.sss_ip_topk_exhaustive(P, P, 4, P, 1000, d, 10, dt, 0, 0, P, P, P, 256, 0)

    def exhaustive_lb(dt, d=96):
        return L.sss_ip_topk_exhaustive_lb(P, P, 4, P, 1000, d, 10, dt, 0, P, P, P, P, 256, 0)

    def range_count(dt, d=128, scan=None):
        return L.sss_range_search_count(P, 4, P, dt, P, dt if scan is None else scan, 0, 0.0, 1000, d, P, 1.0, P, P, P, 256, 0)

    def range_ex_count(dt, d=96):
        return L.sss_range_search_exhaustive_count(P, P, 4, P, 1000, d, dt, 1, P, P, P, 256, 0)

    return {"sss_ip_topk": topk, "sss_ip_topk_threshold": threshold, "sss_ip_topk_long": long_rows,
            "sss_ip_topk_exhaustive": exhaustive, "sss_ip_topk_exhaustive_lb": exhaustive_lb,
            "sss_range_search_count": range_count, "sss_range_search_exhaustive_count": range_ex_count}


@pytest.mark.parametrize("entry", ["sss_ip_topk", "sss_ip_topk_threshold", "sss_ip_topk_long", "sss_ip_topk_exhaustive",
                                   "sss_ip_topk_exhaustive_lb", "sss_range_search_count", "sss_range_search_exhaustive_count"])
def test_dtype_4_passes_the_argument_checks_where_dtype_1_does(L, entry):
    call = _guards(L)[entry]
    assert call(1) == -2, L.sss_last_error()                # bf16: valid but for the workspace / state
    assert call(4) == -2, L.sss_last_error()                # float16: the same
    assert call(4, d=12) == -1                              # 16-byte row pieces (and no scan of that row size)
    assert call(1, d=12) == -1
    for code in (2, 3, 5):                                  # scan-image codes and the next free value: not a corpus dtype
        assert call(code) == -1, (entry, code)


def test_scan_code_goes_with_the_dtype(L):
    """An f16 index scans its own rows (scan = 4); the derived images of a float32 corpus (2, 3) and the other dtypes' own
    codes do not pair with it, as they do not pair with a bf16 index."""
    g = _guards(L)
    for entry in ("sss_ip_topk_threshold", "sss_range_search_count"):
        for scan in (0, 1, 2, 3, 5):
            assert g[entry](4, scan=scan) == -1, (entry, scan)
        assert g[entry](1, scan=4) == -1 and g[entry](0, scan=4) == -1
        assert g[entry](0, scan=3) == -2                    # (the f16 IMAGE of a float32 corpus is still code 3)


def test_row_norm_max_takes_dtype_4(L):
    assert L.sss_row_norm_max(P, 0, 128, 4, P, 0) == 0      # n = 0: nothing to do, after the argument checks
    assert L.sss_row_norm_max(P, 0, 128, 1, P, 0) == 0
    assert L.sss_row_norm_max(P, 0, 12, 4, P, 0) == -1 and L.sss_row_norm_max(P, 0, 12, 1, P, 0) == -1
    for code in (2, 3, 5):
        assert L.sss_row_norm_max(P, 0, 128, code, P, 0) == -1


def test_header_documents_code_4():
    import os
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "sss.h")).read()
    assert "dtype 4" in hdr and "float16" in hdr
