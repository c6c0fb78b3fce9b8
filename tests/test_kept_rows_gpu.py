"""The threshold form (sessionsimilaritysearch_amd/csrc/select_thr.hip) at the edges of its kept-row counts, on the short-row
paths: the rung behind ``search()`` (k_thr_prepare, k_select_all) and the fused route of ``range_search`` (k_range_prepare,
k_range_select, k_range_fill).

Which code a query runs there depends on M, the rows its scan kept.  tests/helpers/kept_rows.py builds corpora in which
M is known per query (tests/test_kept_rows_cpu.py proves it on the host), and the groups put M on both sides of every
switch: the capacity (THR_CAP), the share of the two launches (2048), k_select_all's pruning (2k + 64) and its
selection-or-sort switch (2 Ks), the re-score groups of 128 / 256 rows, and -- by configuration -- the stored row size
from which rows are staged through LDS (1024 bytes).  Queries keep rows AT the radius / the known bound, which do not
pass (range search) or tie across the k-th place (rung).

Every comparison is ``np.array_equal`` on D, I and lims against oracle/search_ref.py; there is no tolerance.  The route
is asserted from both sides: a query that cannot fit must leave the fused route, and no other may (one exactly AT the
capacity may take either; the route it took is printed)."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import kept_rows as kr  # noqa: E402

# (the helper's arrays are read-only and shared between tests; the index only copies them to the device)
pytestmark = [pytest.mark.gpu, pytest.mark.filterwarnings("ignore:The given NumPy array is not writable")]

D_SENTINEL, I_SENTINEL = np.float32(-1234.5), -7


def _index(cuda, cfg, corpus):
    from sessionsimilaritysearch_amd.index import FlatIndex
    _, d, dtype, metric, scan, pad, _ = cfg
    idx = FlatIndex(d, metric, cuda, dtype=dtype, scan=scan, pad_scan=pad)
    idx.add(corpus.c)
    return idx


def _rung_scan(idx):
    return idx.rung_scan() if idx.metric == "ip" else idx.l2_rung_scan()


def _equal(got, want):
    lims, D, I = got
    assert lims.dtype == np.int64 and D.dtype == np.float32 and I.dtype == np.int64
    assert np.array_equal(lims, want[0]), (np.diff(lims), np.diff(want[0]))
    assert np.array_equal(I, want[2])
    assert np.array_equal(D, want[1])


# --------------------------------------------------------------------------------------- (a) range search
@pytest.mark.parametrize("cfg", kr.RANGE_CONFIGS, ids=[c[0] for c in kr.RANGE_CONFIGS])
def test_range_search_at_the_kept_count_edges(cuda, cfg):
    c = kr.corpus(cfg[1], cfg[2], "range")
    idx = _index(cuda, cfg, c)
    want = c.range_expected()
    assert np.array_equal(np.diff(want[0]), c.P)
    must, may = int((c.M > kr.THR_CAP).sum()), int((c.M == kr.THR_CAP).sum())
    assert (must, may) == (3, 2)
    got = idx.range_search(c.q, c.r)
    assert idx.last_range_scan == cfg[6] == idx.rung_scan()
    overflowed = idx.last_range_overflow_queries
    # strict: no row AT a radius is in any result, and query j has exactly its P_j passing rows
    miscounted = [(c.groups[j], int(m)) for j, m in enumerate(np.diff(got[0])) if m != c.P[j]]
    assert (int(c.at_radius[got[2]].sum()), miscounted) == (0, []), "rows AT a radius in the result / (group, count) that differ"
    _equal(got, want)
    # those that cannot fit leave the fused route -- and nobody else, or the exhaustive kernels alone would pass this test
    assert must <= overflowed <= must + may, overflowed
    # the first call's select rewrote every candidate row in place: the same call again, then the queries reversed (the
    # overflowed and the resolved queries interleave differently in the merge)
    again = idx.range_search(c.q, c.r)
    assert idx.last_range_overflow_queries == overflowed
    _equal(again, want)
    order = list(range(c.nq))[::-1]
    back = idx.range_search(np.ascontiguousarray(c.q[order]), np.ascontiguousarray(c.r[order]))
    assert idx.last_range_overflow_queries == overflowed
    _equal(back, c.range_expected(order))
    for j in np.flatnonzero(c.M == kr.THR_CAP):                     # observed, not required: the route AT the capacity
        one = idx.range_search(c.q[j:j + 1], c.r[j:j + 1])
        _equal(one, c.range_expected([j]))
        print(f"kept rows, range {cfg[0]}: group {c.groups[j]} (M = capacity) took the "
              f"{'exhaustive' if idx.last_range_overflow_queries else 'fused'} route")
    print(f"kept rows, range {cfg[0]}: n={c.c.shape[0]} overflowed {overflowed} of {c.nq} (must {must}, may {may})")


# --------------------------------------------------------------------------------------- (b) the rung
def _rung_input(cuda, idx, c, k):
    """(q, D, I, status) on the device as a fused search leaves its unproven queries: column k-1 of D the known bound
    (for L2 the copies' distance, an upper bound of the k-th), status 1 -- and every other entry a sentinel."""
    D = np.full((c.nq, k), D_SENTINEL, np.float32)
    D[:, k - 1] = c.r if idx.metric == "ip" else c.r_l2
    I = np.full((c.nq, k), I_SENTINEL, np.int64)
    return (idx._rows(c.q, "q"), torch.from_numpy(D).to(cuda), torch.from_numpy(I).to(cuda),
            torch.ones(c.nq, dtype=torch.int32, device=cuda), D, I)


def _check_rung(cuda, cfg, c, k):
    """One ``search_threshold`` call on every query of ``c``; returns the rows it left."""
    idx = _index(cuda, cfg, c)
    Dr, Ir = c.topk(k, idx.metric)
    tq, D, I, status, D0, I0 = _rung_input(cuda, idx, c, k)
    left = idx.search_threshold(tq, k, D, I, status, torch.arange(c.nq, device=cuda))
    assert _rung_scan(idx) == cfg[6]
    D, I, status, left = D.cpu().numpy(), I.cpu().numpy(), status.cpu().numpy(), left.cpu().numpy()
    assert set(status.tolist()) <= {0, 1}
    done = status == 0
    wrong = [c.groups[j] for j in np.flatnonzero(done) if not (np.array_equal(I[j], Ir[j]) and np.array_equal(D[j], Dr[j]))]
    assert not wrong, f"resolved queries whose rows differ from the oracle's: groups {wrong}"
    assert np.array_equal(I[~done], I0[~done]) and np.array_equal(D[~done].view(np.uint32), D0[~done].view(np.uint32))
    assert np.array_equal(np.sort(left), np.flatnonzero(~done))
    assert set(np.flatnonzero(c.M > kr.THR_CAP)) <= set(left.tolist()) <= set(np.flatnonzero(c.M >= kr.THR_CAP))
    for j in np.flatnonzero(c.M == kr.THR_CAP):                     # observed, not required
        print(f"kept rows, rung {cfg[0]} k={k}: group {c.groups[j]} (M = capacity) {'stayed unproven' if j in left else 'resolved'}")
    Ds, Is = idx.search(c.q, k)                                     # end to end: what the rung left goes on to the exhaustive kernels
    assert np.array_equal(Is, Ir) and np.array_equal(Ds, Dr)
    return left


@pytest.mark.parametrize("k", (10, 100))
@pytest.mark.parametrize("cfg", kr.RUNG_CONFIGS, ids=[c[0] for c in kr.RUNG_CONFIGS])
def test_rung_at_the_kept_count_edges(cuda, cfg, k):
    c = kr.corpus(cfg[1], cfg[2], ("rung", k))
    assert (c.M >= k).all()                                          # the bound handed in is valid
    left = _check_rung(cuda, cfg, c, k)
    print(f"kept rows, rung {cfg[0]} k={k}: n={c.c.shape[0]} left {sorted(left.tolist())}")


# --------------------------------------------------------------------------------------- (c) next to an overflow
def test_neighbours_of_an_overflowing_query(cuda):
    """The middle query keeps 9100 rows, more than its candidate row holds: the queries whose rows lie before and
    behind it must resolve on the fused route, exactly."""
    cfg = kr.RANGE_CONFIGS[0]
    c = kr.corpus(cfg[1], cfg[2], "neighbours")
    assert c.groups == kr.NEIGHBOUR_GROUPS and c.M[1] > kr.THR_CAP
    idx = _index(cuda, cfg, c)
    want = c.range_expected()
    for _ in range(2):
        got = idx.range_search(c.q, c.r)
        assert idx.last_range_scan == cfg[6] and idx.last_range_overflow_queries == 1
        _equal(got, want)
        assert not c.at_radius[got[2]].any() and np.array_equal(np.diff(got[0]), c.P)
    for k in (10, 100):
        left = _check_rung(cuda, cfg, c, k)
        assert left.tolist() == [1]
