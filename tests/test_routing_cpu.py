"""``ScanRouting`` on its own -- no device, no tensor, no libsss: the public views are projections of the one decision
``_route(k)``, the corpus norm is read only where it can matter, the module imports neither torch nor the library
binding, and the routing table over a grid of shapes equals the one recorded from ``FlatIndex`` before the policy was
moved out of it (tests/golden/routing_table.json)."""
import itertools
import json
import os
import re
import sys

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
from routing_stub import make_routing  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIMS = (4, 60, 64, 96, 128, 200, 256, 260, 512, 1024, 1600, 4096, 4160)
KS = (0, 1, 128, 129, 500, 501, 1024, 1025)
CORPORA = tuple(itertools.product((0, 1000), (2.0 ** -61, 1.0, 2.0 ** 61)))        # (rows, largest row norm)
SCANS = {"f32": ("auto", "f16", "split", "f32"), "bf16": ("native",), "f16": ("native",), "i8": ("native",)}
SHAPES = [(d, metric, dtype, scan, pad) for dtype in SCANS for scan in SCANS[dtype] for metric in ("ip", "l2")
          for pad in (False, True) for d in DIMS]
LETTER = {"": "-", "native": "n", "f16": "h", "split": "s", "f32": "f", "long": "l"}


def routing_table(make):
    """{shape: "routes rungs"}: per corpus of CORPORA the letter of ``_route(k)`` for every k of KS, then the letters of
    ``rung_scan()`` and ``l2_rung_scan()``.  ``make(d, metric, dtype, scan, n, cmax, pad_scan)`` builds the object asked."""
    table = {}
    for d, metric, dtype, scan, pad in SHAPES:
        routes, rungs = "", ""
        for n, cmax in CORPORA:
            r = make(d, metric, dtype, scan, n, cmax, pad)
            routes += "".join(LETTER[r._route(k)] for k in KS)
            rungs += LETTER[r.rung_scan()] + LETTER[r.l2_rung_scan()]
        table[f"{d} {metric} {dtype} {scan} {'pad' if pad else 'own'}"] = routes + " " + rungs
    return table


def _make(d, metric, dtype, scan, n, cmax, pad):
    return make_routing(d, metric, dtype, scan, n=n, cmax=cmax, pad_scan=pad)


def test_views_are_projections_of_the_route():
    for (d, metric, dtype, scan, pad), (n, cmax), k in itertools.product(SHAPES, CORPORA, KS):
        r = _make(d, metric, dtype, scan, n, cmax, pad)
        route = r._route(k)
        views = [r.scan_for(k), r.l2_scan_for(k), r.l2_long_for(k)]
        where = (d, metric, dtype, scan, pad, n, cmax, k)
        assert route in LETTER and sorted(views) == ["", "", route], where
        if route:
            assert views.index(route) == (0 if metric == "ip" else 2 if route == "long" else 1), where
        assert r.fused_ok(k) is (metric == "ip" and route != ""), where


def test_norm_is_read_only_where_shape_dtype_and_k_allow_a_scan():
    class Counting(type(make_routing(128))):
        reads = 0

        def corpus_max_norm(self):
            self.reads += 1
            return super().corpus_max_norm()

    def reads(d, k, metric="l2", dtype="f32", n=1000, **kw):
        from sessionsimilaritysearch_amd import index as ix
        r = Counting(d, metric, dtype, fmt=ix._FORMATS[dtype], ntotal=n, max_norm=1.0, **kw)
        r._route(k)
        return r.reads

    assert reads(128, 10) == 1 and reads(1600, 10) == 1 and reads(200, 10, pad_scan=True) == 1
    assert reads(96, 10) == 0 and reads(4160, 10) == 0 and reads(1616, 10) == 0          # shape: no scan reads such rows
    assert reads(128, 501) == 0 and reads(1600, 1025) == 0 and reads(128, 0) == 0        # k
    assert reads(128, 10, dtype="f16") == 0 and reads(1600, 10, dtype="bf16") == 0       # dtype: float32 rows only
    assert reads(128, 10, n=0) == 0
    assert reads(128, 10, metric="ip") == 0 and reads(1600, 10, metric="ip") == 0        # inner product: no window at all


def test_routing_module_needs_neither_torch_nor_the_library():
    src = open(os.path.join(ROOT, "sessionsimilaritysearch_amd", "routing.py")).read()
    assert not re.search(r"^\s*(import|from)\s+(torch|numpy|ctypes)\b", src, flags=re.M)
    assert not re.search(r"^\s*from\s+\.(\s+import\s+.*\b_lib\b|_lib\b|index\b|_device\b)", src, flags=re.M)
    assert not re.search(r"^\s*(import|from)\s+sessionsimilaritysearch_amd", src, flags=re.M)


def test_routing_table_is_the_index_s_before_the_split():
    with open(os.path.join(ROOT, "tests", "golden", "routing_table.json")) as f:
        golden = json.load(f)
    table = routing_table(_make)
    assert len(table) == len(SHAPES) == len(golden["table"])
    assert [key for key in table if table[key] != golden["table"][key]] == []
