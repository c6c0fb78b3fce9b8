"""The short-row L2 scans (``k_scan<..., MET = 1>`` at d = 64 / 128 / 256 / 512) where their error bound, its ``+inf`` exits
and the routing guard decide (``select_dev.h: err_bound_l2``, ``routing.py: L2_SCAN_MIN_NORM / L2_SCAN_MAX_NORM``).

A result of this route is wrong without notice in one way: ``B_l2`` too small for some input, the query called proven, and
the float64 re-score ordering the wrong candidates perfectly.  tests/test_l2_scan_gpu.py stays at norms between 1/4 and 13
on well-separated rows, where a missing term costs nothing; here every input makes one term decide, and ids AND distances
are compared with ``array_equal`` against ``sr.topk_from_scores(sr.canonical_l2(q, c), k, largest=False)``.

The inputs come from tests/helpers/l2_scan_ref.py; tests/test_l2_scan_bound_cpu.py proves on the host that they are what
they claim.  "No fallbacks" and the background cap (``fallbacks <= nq // 10``, the cap of tests/test_l2_long_gpu.py) are
conditions, not measurements: the CPU file shows for every such query that the exact-distance gap between rank k and the
first row beyond the select's second chance exceeds four times the documented bound, and every such corpus has more rows
than the threshold rung keeps, so the condition cannot be met by keeping everything.  Every search prints one line --
scan, d, case, unproven, fallbacks; DESIGN 3 has the table measured on an MI355X."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import l2_scan_ref as r  # noqa: E402

pytestmark = pytest.mark.gpu

KERNEL_IDS = [f"{s}{d}" for s, d in r.KERNELS]
SCANS = [s for s, _ in r.KERNELS_128]


def _index(cuda, scan, c):
    from sessionsimilaritysearch_amd.index import FlatIndex
    idx = FlatIndex(c.shape[1], "l2", cuda, scan=scan)
    idx.add(np.array(c))                                               # (a copy: the helper's arrays are read-only)
    return idx


def _search(idx, q, k, want, scan, what):
    """One search on the scan route: the route before, the counts printed, ids and distances against `want`, the route after."""
    assert idx.l2_scan_for(k) == scan
    got = idx.search(np.array(q), k)
    print(f"l2 scan bound: scan={scan} d={idx.d} {what}: nq={q.shape[0]} n={idx.ntotal} k={k}: unproven {idx.last_rescan_queries}, "
          f"fallbacks {idx.last_fallback_queries}")
    r._equal(got, want)
    assert idx.last_scan == scan
    return idx.last_rescan_queries, idx.last_fallback_queries


def _search_outside_the_guard(idx, q, k, want, scan, what):
    """One search beyond the guard: no scan is named, the exhaustive kernels answer every query."""
    assert idx.l2_scan_for(k) == ""
    got = idx.search(np.array(q), k)
    print(f"l2 scan bound: scan={scan} d={idx.d} {what}: nq={q.shape[0]} n={idx.ntotal} k={k}: exhaustive")
    r._equal(got, want)
    assert idx.last_rescan_queries == 0 and idx.last_fallback_queries == q.shape[0]


def _background(idx, q, k, want, scan, what):
    """Background queries: the existing suite's cap -- a condition of the test, not a measurement."""
    _, fallbacks = _search(idx, q, k, want, scan, what + " (background)")
    assert fallbacks <= q.shape[0] // 10, (fallbacks, q.shape[0])


def _rows(want, rows):
    """The oracle scores every query on its own: the result of a subset of the queries is that subset of the rows."""
    return want[0][rows], want[1][rows]


def _first(want, k):
    """... and orders by (distance, id): its first k columns are its answer for k."""
    return np.ascontiguousarray(want[0][:, :k]), np.ascontiguousarray(want[1][:, :k])


# ------------------------------------------------------------------------------- 1. magnitudes: both sides scaled
@pytest.mark.parametrize("corpus", ["gauss", "near"])
@pytest.mark.parametrize("scan,d", r.KERNELS, ids=KERNEL_IDS)
def test_both_sides_scaled(cuda, scan, d, corpus):
    """q and c times 2^s scale every canonical distance by exactly 2^(2 s) inside the normal float32 range: one oracle
    answer serves every scale.  "gauss": no fallbacks wherever the documented bound proves every query -- every scale but
    the two of GAUSS_NO_PROOF at 2^-62: under the split scan's subnormal floors nothing is asserted of the counts, under the
    f16 scan sigma = 2^144 makes B_l2 infinite and every query must come out unproven.  "near": 40 copies straddle rank 10
    inside the window of every query; at s = 0 some query must be unproven."""
    if corpus == "gauss":
        (c, q), scales = r.gauss(d), r.GAUSS_SCALES
        D0, I0 = r.answer(("gauss", d), q, c)
    else:
        (c, q, _), scales = r.near(d, scan == "f16"), r.NEAR_SCALES
        D0, I0 = _first(r.answer(("near", d, scan == "f16"), q, c, 41), r.K)
    for s in scales:
        idx = _index(cuda, scan, r.ldexp32(c, s))
        unproven, fallbacks = _search(idx, r.ldexp32(q, s), r.K, (r.ldexp32(D0, 2 * s), I0), scan, f"{corpus} both x 2^{s}")
        if corpus == "near" and s == 0:
            assert unproven > 0                                        # the corpus really sits inside the window
        if corpus == "gauss":
            why = r.GAUSS_NO_PROOF.get((scan, s))
            if why is None:
                assert fallbacks == 0                                  # an honest bound is scale-free in the normal range
            elif why == "inf":
                assert unproven == q.shape[0]
        del idx


# ------------------------------------------------------------------------------- 2. one side scaled
@pytest.mark.parametrize("side,s", r.ONE_SIDE, ids=[f"{a}{s}" for a, s in r.ONE_SIDE])
@pytest.mark.parametrize("scan", SCANS)
def test_one_side_scaled(cuda, scan, side, s):
    """Unit queries x 2^s against unit rows, unit rows x 2^s against unit queries: no scaling relation holds, every case has
    an oracle answer of its own.  Every distance is the larger side's |x|^2 to within 2^-38: a handful of float32 values,
    the answer exact ties in id order, and the proof must refuse to certify the scan's order.  No cap on unproven queries
    or fallbacks here: they are printed.  A corpus x 2^-70 or 2^-100 lies beyond the guard: the route must say so."""
    c, q = r.one_side(side, s)
    want = r.answer(("one_side", side, s), q, c)
    idx = _index(cuda, scan, c)
    if r.in_guard(c):
        _search(idx, q, r.K, want, scan, f"{side} x 2^{s}")
    else:
        _search_outside_the_guard(idx, q, r.K, want, scan, f"{side} x 2^{s}")


# ------------------------------------------------------------------------------- 3. the +inf exits and the guard
@pytest.mark.parametrize("d", [128, 512])
@pytest.mark.parametrize("name", sorted(r.INF_EXITS))
def test_infinite_bound_leaves_every_query_unproven(cuda, name, d):
    """f16 scan, sigma = 2^(corpus shift + query shift) beyond 2^120 ("sigma": rows x 2^-55, queries x 2^-75) or a scaled
    bias cmax^2 sigma / 2 >= 1e36 ("bias": rows x 2^55, queries x 2^-100): B_l2 = +inf for every query, and the select
    kernels force the status whatever the keys are."""
    c, q = r.unit(d)
    ce, qe = r.INF_EXITS[name]
    cs, qs = r.ldexp32(c, ce), r.ldexp32(q, qe)
    idx = _index(cuda, "f16", cs)
    unproven, _ = _search(idx, qs, r.K, r.answer(("inf", name, d), qs, cs), "f16", f"+inf exit: {name}")
    assert unproven == q.shape[0]


@pytest.mark.parametrize("scan,d", r.KERNELS, ids=KERNEL_IDS)
def test_query_norm_whose_square_overflows_float32(cuda, scan, d):
    """Unit queries x 2^70: every canonical distance rounds to +inf, the oracle answers D = inf, I = 0 .. k-1, and so must
    the device, whichever stage resolves the query."""
    c, q = r.unit(d)
    qs = r.ldexp32(q, 70)
    with np.errstate(over="ignore"):
        want = r.answer(("inf", "qnorm", d), qs, c)
    assert np.isposinf(want[0]).all()
    _search(_index(cuda, scan, c), qs, r.K, want, scan, "queries x 2^70")


@pytest.mark.parametrize("scan,d", r.KERNELS, ids=KERNEL_IDS)
def test_guard_edges(cuda, scan, d):
    """Unit rows (and queries) x 2^59 and 2^-59: the scan; x 2^61 and 2^-61: no scan, the exhaustive kernels.  All exact."""
    c, q = r.unit(d)
    for s in r.GUARD_EDGES:
        cs, qs = r.ldexp32(c, s), r.ldexp32(q, s)
        want = r.answer(("edge", d, s), qs, cs)
        idx = _index(cuda, scan, cs)
        if abs(s) < 60:
            _search(idx, qs, r.K, want, scan, f"guard edge 2^{s}")
        else:
            _search_outside_the_guard(idx, qs, r.K, want, scan, f"guard edge 2^{s}")
        del idx


@pytest.mark.parametrize("scan", SCANS)
def test_route_follows_add_across_the_guard(cuda, scan):
    """One index, inside the guard after the first ``add`` (rows x 2^59), outside after the second (rows x 2^61)."""
    c, q = r.unit(128)
    first, second = r.ldexp32(c[:4000], 59), r.ldexp32(c[4000:], 61)
    qs = r.ldexp32(q, 59)
    idx = _index(cuda, scan, first)
    _search(idx, qs, r.K, r.answer(("cross", 1), qs, first), scan, "first add, x 2^59")
    idx.add(second)
    both = np.concatenate([first, second])
    _search_outside_the_guard(idx, qs, r.K, r.answer(("cross", 2), qs, both), scan, "second add, x 2^61")


# ------------------------------------------------------------------------------- 4. small rows under a large cmax
@pytest.mark.parametrize("scan", SCANS)
def test_small_rows_under_a_large_cmax(cuda, scan):
    """Rows at 2^-70 (subnormal float32 bias), ten zero rows, a zero query, queries at the tiny rows' scale (subnormal
    distances, exact ties in id order), dwarf clusters at 2^-27 and 2^-39 whose f16 image keeps a few bits or none -- under
    giants of norm 8 (largest element 3.0) that set cmax, the corpus shift and c_resid.  A bound that treats a flushed
    image as exact proves a wrong order.  Exactness and the route only."""
    c, q, _ = r.small_rows()
    want = _first(r.answer("small_rows", q, c, 100), r.K)
    _search(_index(cuda, scan, c), q, r.K, want, scan, "small rows under giants")


# ------------------------------------------------------------------------------- 5. rounding aligned against the query
@pytest.mark.parametrize("scan", ["f16", "split"])
def test_rounding_aligned_against_the_query(cuda, scan):
    """The leading input-rounding term: 30 true neighbours of query 0 whose every element the scan image rounds in the
    direction that lowers q.c -- 0.79 of 2^-11 |q||c| for f16, 0.40 of 2^-16 |q||c| for split, measured in
    tests/test_l2_scan_bound_cpu.py -- behind 200 decoys whose image is exact and which tie exactly.  The scan ranks every
    decoy ahead of every neighbour; only the bound keeps the neighbours alive (for f16 their score error is 0.91 of B_l2)."""
    c, q, info = r.worst_f16() if scan == "f16" else r.worst_split()
    want100 = r.answer(("aligned", scan), q, c, 100)
    assert set(want100[1][0, :30].tolist()) == set(info["aligned"].tolist())
    idx = _index(cuda, scan, c)
    for k in (10, 100):
        unproven, _ = _search(idx, q[:1], k, _rows(_first(want100, k), slice(0, 1)), scan, "aligned rounding")
        assert unproven >= 1
    _background(idx, q[1:], r.K, _rows(_first(want100, r.K), slice(1, None)), scan, "aligned rounding")


@pytest.mark.parametrize("norm", r.ULP_NORMS, ids=["norm1/4", "norm4", "norm2^30"])
def test_f32_copies_one_ulp_apart(cuda, norm):
    """The f32 scan rounds no input: 40 copies of query 0's nearest row, one float32 ulp apart in one coordinate, straddle
    rank 10 -- their distances differ by 3e-4 of the bound, the scan cannot order them."""
    c, q, _ = r.ulp_copies(norm)
    want = _first(r.answer(("ulp", norm), q, c, 41), r.K)
    idx = _index(cuda, "f32", c)
    unproven, _ = _search(idx, q[:1], r.K, _rows(want, slice(0, 1)), "f32", f"ulp copies at norm {norm:g}")
    assert unproven >= 1
    _background(idx, q[1:], r.K, _rows(want, slice(1, None)), "f32", f"ulp copies at norm {norm:g}")
