"""L2 on the matrix-core scans without a device: the new header and its ctypes table agree, include/sss.h keeps its
entry points, and the routing policy of ``FlatIndex.l2_scan_for`` is host logic."""
import os
import sys

import pytest

from sessionsimilaritysearch_amd import _lib, index as ix

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
from abi import declared  # noqa: E402
from routing_stub import make_routing  # noqa: E402


def test_l2_header_and_ctypes_binding_declare_the_same_entry_points():
    names = declared("sss_l2.h")
    assert names == _lib.symbols("sss_l2.h")
    assert names == ["sss_l2_row_bias", "sss_l2_topk", "sss_l2_topk_threshold", "sss_l2_topk_threshold_workspace_bytes",
                     "sss_l2_topk_workspace_bytes"]
    L = _lib.lib()
    for n in names:
        assert getattr(L, n).argtypes == _lib.HEADERS["sss_l2.h"][n][1]


def test_main_header_keeps_its_entry_points():
    """The L2 entry points live in their own header: include/sss.h declares what it declared (its coverage table is in a
    test file of its own) and none of the new names."""
    main = declared("sss.h")
    assert main == _lib.exported_symbols() and len(main) == 60
    assert not [n for n in main if n.startswith("sss_l2_")]


def test_l2_sizing_queries_are_host_arithmetic():
    L = _lib.lib()
    assert L.sss_l2_topk_workspace_bytes(8, 20000, 128, 10, 0) == L.sss_ip_topk_workspace_bytes(8, 20000, 128, 10, 0) > 0
    assert L.sss_l2_topk_workspace_bytes(8, 20000, 128, 10, 3) == L.sss_ip_topk_f16_workspace_bytes(8, 20000, 128, 10) > 0
    assert L.sss_l2_topk_workspace_bytes(8, 20000, 128, 10, 1) == 0          # bf16 rows: no L2 scan
    assert L.sss_l2_topk_workspace_bytes(8, 20000, 200, 10, 0) == 0
    assert L.sss_l2_topk_threshold_workspace_bytes(8, 20000, 128, 2) == L.sss_ip_topk_threshold_workspace_bytes(8, 20000, 128, 2) > 0
    assert L.sss_l2_topk_threshold_workspace_bytes(8, 20000, 128, 6) == 0


def Stub(d, metric="l2", **kw):
    """No device: only the policy."""
    return make_routing(d, metric, **kw)


def test_l2_scan_policy():
    assert Stub(200).l2_scan_for(10) == ""                                   # no fused kernel for this d
    assert Stub(128).l2_scan_for(501) == "" and Stub(128).l2_scan_for(500) == "split"
    assert Stub(128, dtype="f16", scan="native").l2_scan_for(10) == ""       # float32 rows only
    assert Stub(128, metric="ip").l2_scan_for(10) == "" and Stub(128, n=0).l2_scan_for(10) == ""
    assert [Stub(128).l2_scan_for(k) for k in (1, 128, 129)] == ["f16", "f16", "split"]
    assert [Stub(128, scan=s).l2_scan_for(10) for s in ("f32", "split", "f16")] == ["f32", "split", "f16"]
    assert Stub(64).l2_scan_for(10) == "split" and Stub(64, scan="f16").l2_scan_for(10) == "split"     # no f16 image at d = 64
    assert Stub(512).l2_scan_for(10) == "f16" and Stub(512, scan="f32").l2_scan_for(10) == ""
    assert Stub(1600).l2_scan_for(10) == ""                                  # long rows: the exhaustive kernels
    # the inner-product views stay what they were for an L2 index
    assert Stub(128).scan_for(10) == "" and Stub(128).fused_ok(10) is False and Stub(128).rung_scan() == ""
    assert Stub(128).l2_rung_scan() == "f16" and Stub(128, scan="f32").l2_rung_scan() == "f32" and Stub(200).l2_rung_scan() == ""


def test_l2_magnitude_guard():
    """The scan route only where cmax^2 / 2 is a normal float32 with room to spare: 2^-60 <= cmax <= 2^60."""
    assert ix.L2_SCAN_MIN_NORM == 2.0 ** -60 and ix.L2_SCAN_MAX_NORM == 2.0 ** 60
    for cmax, want in ((2.0 ** -60, "f16"), (2.0 ** 60, "f16"), (2.0 ** -61, ""), (2.0 ** 61, ""), (0.0, ""),
                       (float("inf"), ""), (float("nan"), "")):
        assert Stub(128, cmax=cmax).l2_scan_for(10) == want, cmax


def test_l2_escalation_state_is_shared_with_the_ladder():
    s = Stub(128, n=20000)
    s.last_scan = "f16"
    s._note_fallbacks(10, 300, 200)                                          # most of a batch unproven
    assert s.l2_scan_for(10) == "split"


def test_l2_index_validates_its_scan_argument():
    with pytest.raises(ValueError):
        ix.FlatIndex(128, "l2", scan="nope")
    try:
        idx = ix.FlatIndex(128, "l2", scan="f32")                            # accepted as for "ip" (then: a device, or the no-device error)
        assert idx.scan == "f32"
    except _lib.SssError as e:
        assert "no HIP device" in str(e)
