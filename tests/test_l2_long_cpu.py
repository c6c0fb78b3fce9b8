"""L2 on the long-row scan without a device: include/sss_l2_long.h and its ctypes table agree and stay out of the other
headers' lists, the workspace size is host arithmetic, and the routing policy of ``FlatIndex.l2_long_for`` is host logic."""
import os
import sys

from sessionsimilaritysearch_amd import _lib, index as ix

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
from abi import declared  # noqa: E402
from routing_stub import make_routing  # noqa: E402
NAMES = ["sss_l2_topk_long", "sss_l2_topk_long_workspace_bytes"]


def test_l2_long_header_and_ctypes_binding_declare_the_same_entry_points():
    names = declared("sss_l2_long.h")
    assert names == _lib.symbols("sss_l2_long.h") == NAMES
    L = _lib.lib()
    for n in names:
        assert getattr(L, n).argtypes == _lib.HEADERS["sss_l2_long.h"][n][1]
        assert getattr(L, n).restype == _lib.HEADERS["sss_l2_long.h"][n][0]


def test_l2_long_names_are_in_no_other_list():
    others = {"sss.h": _lib.exported_symbols(), "sss_sparse.h": _lib.symbols("sss_sparse.h"), "sss_l2.h": _lib.symbols("sss_l2.h"),
              "sss_pad.h": _lib.symbols("sss_pad.h"), "sss_graph.h": _lib.symbols("sss_graph.h"), "sss_eval.h": _lib.symbols("sss_eval.h")}
    for header, listed in others.items():
        assert not set(NAMES) & set(listed), header
        assert not set(NAMES) & set(declared(header)), header


def test_l2_long_workspace_bytes_is_host_arithmetic():
    L = _lib.lib()
    assert L.sss_l2_topk_long_workspace_bytes(8, 20000, 1600) > 0
    assert L.sss_l2_topk_long_workspace_bytes(8, 20000, 200) == 0
    for nq, n, d in ((8, 20000, 1600), (1024, 1_000_000, 1600), (33, 3000, 320), (1, 1, 4096)):
        assert L.sss_l2_topk_long_workspace_bytes(nq, n, d) >= L.sss_ip_topk_long_workspace_bytes(nq, n, d, 0) > 0
    assert L.sss_l2_topk_long_workspace_bytes(0, 20000, 1600) == 0 and L.sss_l2_topk_long_workspace_bytes(8, 0, 1600) == 0
    assert L.sss_l2_topk_long_workspace_bytes(8, 20000, 4160) == 0          # a row over 16 KB


def Stub(d, metric="l2", **kw):
    """No device: only the policy."""
    return make_routing(d, metric, **kw)


def test_l2_long_policy():
    assert Stub(1600).l2_long_for(10) == "long" and Stub(320).l2_long_for(10) == "long"
    assert Stub(128).l2_long_for(10) == ""                                   # a fused scan serves this d
    assert Stub(200).l2_long_for(10) == ""                                   # d % 64
    assert Stub(4160).l2_long_for(10) == ""                                  # a row over 16 KB
    assert Stub(4096).l2_long_for(10) == "long"
    assert Stub(1600).l2_long_for(1024) == "long" and Stub(1600).l2_long_for(1025) == "" and Stub(1600).l2_long_for(0) == ""
    assert Stub(1600, metric="ip").l2_long_for(10) == ""
    assert Stub(1600, dtype="f16", scan="native").l2_long_for(10) == ""      # float32 rows only
    assert Stub(1600, dtype="bf16", scan="native").l2_long_for(10) == ""
    assert Stub(1600, n=0).l2_long_for(10) == ""
    for cmax, want in ((2.0 ** -60, "long"), (2.0 ** 60, "long"), (2.0 ** -61, ""), (2.0 ** 61, ""), (0.0, ""),
                       (float("inf"), ""), (float("nan"), "")):
        assert Stub(1600, cmax=cmax).l2_long_for(10) == want, cmax


def test_l2_route_joins_the_two_policies():
    s = Stub(1600)
    assert s._route(10) == "long" and s.l2_scan_for(10) == ""
    assert Stub(128)._route(10) == "f16" and Stub(128)._route(600) == ""     # fused widths: as before, k > 500 exhaustive
    assert Stub(1600, metric="ip")._route(10) == "long"                      # the inner-product long scan, as before
    assert Stub(1600, dtype="bf16", scan="native")._route(10) == ""
    # the inner-product views stay what they were for an L2 index
    assert s.scan_for(10) == "" and s.fused_ok(10) is False and s.rung_scan() == "" and s.l2_rung_scan() == ""
