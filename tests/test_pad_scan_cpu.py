"""``pad_scan`` without a device: the switch is off by default and changes nothing then; with it the routing policy of a
float32 index of any width d % 4 == 0 up to 512 is host logic; include/sss_pad.h, libsss.so and the ctypes table name the
same entry points; and every argument rule of the new entry points is checked before anything is launched (calls with
null or never-dereferenced pointers, as tests/test_abi_contract_cpu.py makes them)."""
import os
import sys

import pytest

from sessionsimilaritysearch_amd import _lib, index as ix

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
from abi import declared  # noqa: E402
from routing_stub import make_routing as Stub  # noqa: E402    (no device: only the policy)


def _route(d, k, **kw):
    metric = kw.get("metric", "ip")
    s = Stub(d, **kw)
    return s.l2_scan_for(k) if metric == "l2" else s.scan_for(k)


# ------------------------------------------------------------------------------------------- default: nothing changes
@pytest.mark.parametrize("pad_scan", [None, False])
def test_default_routes_are_what_they_were(pad_scan):
    for d in (96, 200, 1616):
        for k in (1, 10, 200, 500, 501):
            assert Stub(d, pad_scan=pad_scan).scan_for(k) == ""
            assert Stub(d, "l2", pad_scan=pad_scan).l2_scan_for(k) == ""
            assert Stub(d, pad_scan=pad_scan).fused_ok(k) is False
        assert Stub(d, pad_scan=pad_scan).rung_scan() == "" and Stub(d, "l2", pad_scan=pad_scan).l2_rung_scan() == ""
        for scan in ("f16", "split", "f32"):
            assert Stub(d, scan=scan, pad_scan=pad_scan).scan_for(10) == ""
            assert Stub(d, pad_scan=pad_scan).scan_width(scan) == 0 and Stub(d, pad_scan=pad_scan).next_scan(scan) == ""
    # the widths with a scan of their own keep it, and their width
    assert Stub(128, pad_scan=pad_scan).scan_for(10) == "f16" and Stub(128, pad_scan=pad_scan).scan_width("f16") == 128
    assert Stub(64, pad_scan=pad_scan).scan_for(10) == "split" and Stub(64, pad_scan=pad_scan).scan_width("f16") == 0
    assert Stub(512, pad_scan=pad_scan).scan_width("f16") == 512 and Stub(512, pad_scan=pad_scan).scan_width("f32") == 0
    assert Stub(1600, pad_scan=pad_scan).scan_for(100) == "long"


def test_the_switch_is_keyword_only_and_off_by_default():
    import inspect
    for fn in (ix.FlatIndex.__init__, ix.build_index):
        p = inspect.signature(fn).parameters["pad_scan"]
        assert p.kind is inspect.Parameter.KEYWORD_ONLY and p.default is False
    assert ix.FlatIndex._pad is False


def test_no_effect_where_d_has_a_scan_or_the_rows_are_not_float32():
    for d in (64, 128, 256, 512):
        a, b = Stub(d, pad_scan=True), Stub(d, pad_scan=False)
        assert a._pad is False
        assert [a.scan_for(k) for k in (10, 200, 501)] == [b.scan_for(k) for k in (10, 200, 501)]
        assert [a.scan_width(s) for s in ("f16", "split", "f32")] == [b.scan_width(s) for s in ("f16", "split", "f32")]
    assert Stub(192, pad_scan=True).scan_for(10) == "long" and Stub(1600, pad_scan=True).scan_for(10) == "long"
    assert Stub(256, dtype="bf16", scan="native", pad_scan=True).scan_for(10) == "native"
    assert Stub(200, dtype="f16", scan="native", pad_scan=True).scan_for(10) == ""
    assert Stub(200, "l2", dtype="f16", scan="native", pad_scan=True).l2_scan_for(10) == ""
    assert Stub(208, dtype="i8", scan="native", pad_scan=True).scan_for(10) == ""


# ------------------------------------------------------------------------------------------- routing with the switch on
@pytest.mark.parametrize("metric", ["ip", "l2"])
def test_padded_routes(metric):
    on = dict(metric=metric, pad_scan=True)
    assert [_route(200, k, **on) for k in (1, 10, 128, 129, 200, 500, 501)] == ["f16", "f16", "f16", "split", "split", "split", ""]
    assert [_route(200, 10, scan=s, **on) for s in ("f32", "split", "f16")] == ["f32", "split", "f16"]
    for scan in ("auto", "f16", "split", "f32"):
        assert [_route(260, k, scan=scan, **on) for k in (10, 200, 500, 501)] == ["f16", "f16", "f16", ""], scan
        assert [_route(508, k, scan=scan, **on) for k in (10, 200)] == ["f16", "f16"], scan
    assert _route(60, 10, scan="f16", **on) == "f16" and Stub(60, scan="f16", pad_scan=True).scan_width("f16") == 128
    assert _route(60, 10, scan="split", **on) == "split" and Stub(60, scan="split", pad_scan=True).scan_width("split") == 64
    assert _route(4, 10, **on) == "f16" and _route(4, 200, **on) == "split"
    for d in (6, 202, 199, 516, 520, 1616, 2):
        assert _route(d, 10, **on) == "", d
    assert _route(200, 10, n=0, **on) == "" and _route(200, 0, **on) == ""


def test_scan_width():
    s = Stub(200, pad_scan=True)
    assert [s.scan_width(x) for x in ("f16", "split", "f32")] == [256, 256, 256]
    assert [Stub(68, pad_scan=True).scan_width(x) for x in ("f16", "split", "f32")] == [128, 128, 128]
    assert [Stub(60, pad_scan=True).scan_width(x) for x in ("f16", "split", "f32")] == [128, 64, 64]
    assert [Stub(4, pad_scan=True).scan_width(x) for x in ("f16", "split", "f32")] == [128, 64, 64]
    assert [Stub(260, pad_scan=True).scan_width(x) for x in ("f16", "split", "f32")] == [512, 0, 0]
    assert [Stub(508, pad_scan=True).scan_width(x) for x in ("f16", "split", "f32")] == [512, 0, 0]


def test_padded_views_report_the_scan_truthfully():
    s = Stub(200, pad_scan=True)
    assert s.fused_ok(10) is True and s.fused_ok(501) is False
    assert s.rung_scan() == "f16" and Stub(200, scan="f32", pad_scan=True).rung_scan() == "f32"
    assert Stub(200, scan="split", pad_scan=True).rung_scan() == "split" and Stub(260, scan="f32", pad_scan=True).rung_scan() == "f16"
    assert s.next_scan("f16") == "split" and s.next_scan("split") == "f32" and s.next_scan("f32") == ""
    assert Stub(260, pad_scan=True).next_scan("f16") == ""
    l2 = Stub(200, "l2", pad_scan=True)
    assert l2.l2_rung_scan() == "f16" and l2.rung_scan() == "" and l2.scan_for(10) == "" and l2.fused_ok(10) is False
    assert Stub(200, "l2", cmax=2.0 ** 61, pad_scan=True).l2_scan_for(10) == ""          # the magnitude guard holds
    r = Stub(200, pad_scan=True)                           # scan="auto": a complete split image beats building an f16 one
    r._complete.add("split")
    assert r.rung_scan() == "split"


@pytest.mark.parametrize("d,native", [(200, 256), (68, 128)])
def test_escalation_and_decay_as_at_a_native_width(d, native):
    """The same sequence of searches moves a padded index and an index of the scan's own width through the same scans."""
    a, b = Stub(d, n=20000, pad_scan=True), Stub(native, n=20000)
    seen = []
    for s in (a, b):
        trace = []
        for bad in [200, 0] + [0] * ix.AUTO_DECAY_SEARCHES + [3, 200, 200, 0]:
            s.last_scan = s.scan_for(10)
            trace.append(s.last_scan)
            s._note_fallbacks(10, 300, bad)
        seen.append(trace)
    assert seen[0] == seen[1]
    # escalated by the first search, back down after AUTO_DECAY_SEARCHES clean ones; 3 unproven of 300 move nothing; a second
    # escalation that proves no more is taken back at once (and pinned)
    n = ix.AUTO_DECAY_SEARCHES
    assert seen[0][:2] == ["f16", "split"] and seen[0][n] == "split" and seen[0][n + 1:n + 4] == ["f16", "f16", "f16"]
    assert seen[0][n + 4:] == ["split", "f16"]
    c = Stub(260, n=20000, pad_scan=True)                  # nothing above f16 at this width: never off the ladder
    c.last_scan = "f16"
    c._note_fallbacks(10, 300, 200)
    assert c.scan_for(10) == "f16"


# ------------------------------------------------------------------------------------------- ABI
PAD_NAMES = ["sss_pad_f16_resid_max", "sss_pad_rows_f32", "sss_pad_scale_f16", "sss_pad_split_bf16", "sss_pad_topk",
             "sss_pad_topk_threshold", "sss_pad_topk_threshold_workspace_bytes", "sss_pad_topk_workspace_bytes"]


def test_pad_header_library_and_ctypes_binding_name_the_same_entry_points():
    names = declared("sss_pad.h")
    assert names == _lib.symbols("sss_pad.h") == PAD_NAMES
    L = _lib.lib()
    for n in names:
        assert getattr(L, n).argtypes == _lib.HEADERS["sss_pad.h"][n][1]
    assert not [n for n in declared("sss.h") if n.startswith("sss_pad_")]
    assert not set(names) & (set(_lib.exported_symbols()) | set(_lib.symbols("sss_l2.h")) | set(_lib.symbols("sss_sparse.h")))


def test_pad_sizing_queries():
    L = _lib.lib()
    nq, n, k = 8, 20000, 10
    for scan in (0, 2, 3):
        assert L.sss_pad_topk_workspace_bytes(nq, n, 200, 256, k, scan) > 0
        assert L.sss_pad_topk_threshold_workspace_bytes(nq, n, 200, 256, scan) > 0
    # what the scan's own width asks: the workspace does not know the rows are narrower
    assert L.sss_pad_topk_workspace_bytes(nq, n, 200, 256, k, 0) == L.sss_ip_topk_workspace_bytes(nq, n, 256, k, 0)
    assert L.sss_pad_topk_workspace_bytes(nq, n, 200, 256, k, 3) == L.sss_ip_topk_f16_workspace_bytes(nq, n, 256, k)
    assert L.sss_pad_topk_threshold_workspace_bytes(nq, n, 200, 256, 2) == L.sss_ip_topk_threshold_workspace_bytes(nq, n, 256, 2)
    assert L.sss_pad_topk_workspace_bytes(nq, n, 260, 512, k, 3) > 0 and L.sss_pad_topk_workspace_bytes(nq, n, 4, 64, k, 0) > 0
    bad = [(202, 256, 0), (0, 256, 0), (-4, 256, 0), (260, 256, 0), (200, 200, 0), (200, 512, 0), (200, 512, 2), (60, 64, 3),
           (200, 256, 1), (200, 256, 4), (200, 256, 6), (200, 256, 7)]
    for d_row, d_scan, scan in bad:
        assert L.sss_pad_topk_workspace_bytes(nq, n, d_row, d_scan, k, scan) == 0, (d_row, d_scan, scan)
        assert L.sss_pad_topk_threshold_workspace_bytes(nq, n, d_row, d_scan, scan) == 0, (d_row, d_scan, scan)
    assert L.sss_pad_topk_workspace_bytes(0, n, 200, 256, k, 0) == 0 and L.sss_pad_topk_workspace_bytes(nq, 0, 200, 256, k, 0) == 0


# Addresses that are never dereferenced: every call below fails a host-side check before anything is launched, and -- as a
# second line -- is handed a workspace of 0 bytes unless the workspace rule itself is the one under test.
A = 1 << 20                             # 256-byte aligned


def _topk(L, q=A, nq=8, c=A, img=A, scan=0, shift=0, resid=0.0, bias=0, n=1000, d_row=200, d_scan=256, k=10, D=A, I=A, status=A,
          state=A, state_bytes=1 << 30, ws=A, ws_bytes=0):
    return L.sss_pad_topk(q, nq, c, img, scan, shift, resid, bias, n, d_row, d_scan, k, 0, 1.0, D, I, status, 0, state, state_bytes, ws,
                          ws_bytes, 0)


def _thr(L, q=A, sel=A, nsel=8, c=A, img=A, scan=0, shift=0, resid=0.0, bias=0, n=1000, d_row=200, d_scan=256, k=10, D=A, I=A,
         status=A, ws=A, ws_bytes=0):
    return L.sss_pad_topk_threshold(q, sel, nsel, c, img, scan, shift, resid, bias, n, d_row, d_scan, k, 0, 1.0, D, I, status, ws,
                                    ws_bytes, 0)


SHARED_RULES = [
    (dict(d_row=202), -1), (dict(d_row=0), -1), (dict(d_row=-4), -1), (dict(d_row=260), -1),            # d_row % 4, 0 < d_row <= d_scan
    (dict(d_scan=200), -1), (dict(d_scan=512), -1), (dict(d_scan=512, scan=2), -1), (dict(d_row=60, d_scan=64, scan=3), -1),   # not a fused shape
    (dict(scan=1), -1), (dict(scan=4), -1), (dict(scan=6), -1),                                          # not a scan of f32 rows
    (dict(img=0), -1), (dict(img=A + 8), -1),                                                            # scan image
    (dict(scan=3, shift=161), -1), (dict(scan=3, resid=-1.0), -1),
    (dict(n=0), -1), (dict(k=0), -1), (dict(n=(1 << 31) - 1024), -1),
    (dict(bias=A + 4), -1),
    (dict(q=0), -1), (dict(c=0), -1), (dict(D=0), -1), (dict(I=0), -1), (dict(status=0), -1), (dict(q=A + 4), -1), (dict(c=A + 8), -1),
    (dict(ws=A + 16), -1),
    (dict(ws=0), -2), (dict(ws_bytes=0), -2),
]


def test_pad_topk_argument_rules():
    L = _lib.lib()
    need = L.sss_pad_topk_workspace_bytes(8, 1000, 200, 256, 10, 0)
    rules = SHARED_RULES + [(dict(nq=0), -1), (dict(k=501), -1), (dict(state=A + 8), -1), (dict(state=0), -2), (dict(state_bytes=16), -2),
                            (dict(ws_bytes=need - 1), -2), (dict(bias=A, ws_bytes=need - 1), -2)]
    for kw, want in rules:
        assert _topk(L, **kw) == want, kw
        assert L.sss_last_error().startswith(b"pad_topk:"), (kw, L.sss_last_error())


def test_pad_topk_threshold_argument_rules():
    L = _lib.lib()
    need = L.sss_pad_topk_threshold_workspace_bytes(8, 1000, 200, 256, 0)
    rules = SHARED_RULES + [(dict(nsel=0), -1), (dict(sel=0), -1), (dict(k=8193), -1), (dict(ws_bytes=need - 1), -2),
                            (dict(bias=A, ws_bytes=need - 1), -2)]
    for kw, want in rules:
        assert _thr(L, **kw) == want, kw
        assert L.sss_last_error().startswith(b"pad_topk_threshold:"), (kw, L.sss_last_error())


def test_pad_builder_argument_rules():
    L = _lib.lib()
    calls = {
        "pad_rows_f32": lambda x=A, n=8, d=200, ds=256, y=A: L.sss_pad_rows_f32(x, n, d, ds, y, 0),
        "pad_scale_f16": lambda x=A, n=8, d=200, ds=256, y=A, shift=0: L.sss_pad_scale_f16(x, n, d, ds, shift, y, 0),
        "pad_split_bf16": lambda x=A, n=8, d=200, ds=256, y=A: L.sss_pad_split_bf16(x, n, d, ds, y, 0),
        "pad_f16_resid_max": lambda x=A, n=8, d=200, ds=256, y=A, shift=0, out=A: L.sss_pad_f16_resid_max(x, y, n, d, ds, shift, out, 0),
    }
    for name, call in calls.items():
        for kw in (dict(d=202), dict(d=0), dict(d=260), dict(ds=252), dict(n=-1), dict(x=0), dict(y=0), dict(x=A + 4), dict(y=A + 8)):
            assert call(**kw) == -1, (name, kw)
            assert L.sss_last_error().startswith(name.encode() + b":"), (name, kw, L.sss_last_error())
        assert call(n=0) == 0 and call(n=0, x=0, y=0) == 0                     # no rows: a no-op
    for name in ("pad_scale_f16", "pad_f16_resid_max"):
        assert calls[name](shift=161) == -1 and L.sss_last_error().startswith(name.encode() + b":")
    assert calls["pad_f16_resid_max"](out=0) == -1
