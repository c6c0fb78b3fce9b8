"""The product-type index on the device (include/sss_ptype.h, csrc/ptype.hip, sessionsimilaritysearch_amd/product_types.py).

Fixture parity: on the sessions of tests/golden/eval_metrics.npz with the item -> type table of
tests/golden/type_score_truth.npz, type_bags, search, bands, mine_triples, pair_scores and neighbourhood_recall are
array_equal to the numpy helper of tests/helpers/type_score_ref.py (the score of record: integers, one np.sqrt, one
division), which tests/test_type_score_cpu.py holds to the matrix the reference's own get_score produced, within the
generator's measured tolerance; the pair scores are held to the reference within that tolerance directly as well, and
get_ave_score / get_recall to its recorded values by the bounds of tests/test_eval_metrics_cpu.py.

Kernel edges: every entry point through ctypes on exactly sized, guarded buffers, run twice from two poisons, at the smallest
shapes where the walk of csrc/ptype.hip can go wrong: rows around the DEPTH entries a thread keeps in LDS, every kind of wave,
corpus sizes around the 256-row workgroup, sub-batches of both triples, the largest counts the contract allows."""
import ctypes
import json
import os
import socket
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import type_score_ref as tr  # noqa: E402

from sessionsimilaritysearch_amd import _lib, evaluation, jaccard, product_types as pt, sparse  # noqa: E402
from sessionsimilaritysearch_amd.sessions import ActionTable  # noqa: E402
from test_abi_contract_gpu import OFF, Buf, L, _st, dev_buf, run_twice  # noqa: E402
from test_eval_metrics_cpu import AVE_TOL, GAMMA  # noqa: E402
from test_type_score_cpu import EDGE_SETS, SIM, check_argument_errors, truth  # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEPTH = 16                           # PT_D of csrc/ptype.hip
N_TYPES = 50                         # the type vocabulary of the edge corpus
SEVEN = (0.1, 0.2, 0.25, 1 / 3, 0.5, 0.8, 1.0)
_CACHE = {}


def dev(b, cuda):
    return sparse._device_triple(b[0], b[1], b[2], cuda)


def same(a, b):
    """Bit for bit, a nan equal to a nan."""
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and np.array_equal(a, b, equal_nan=a.dtype.kind == "f")


# ------------------------------------------------------------------------------------------------ fixture parity
def gold(cuda):
    if "gold" not in _CACHE:
        t, g, tab, qb, cb, s = truth()
        seq, tar = tab["query"].split(1, 2)
        n_types = int(t["n_types"])
        bags = pt.type_bags(ActionTable.concat(seq, tar), t["item_type"], n_types, cuda)
        corpus = pt.type_bags(tab["corpus"], t["item_type"], n_types, cuda)
        _CACHE["gold"] = types.SimpleNamespace(t=t, g=g, qb=qb, cb=cb, s=s, bags=bags, corpus=corpus,
                                               index=pt.ProductTypeIndex(n_types, cuda).add(corpus))
    return _CACHE["gold"]


def test_fixture_type_bags_equal_the_helper(cuda):
    G = gold(cuda)
    for got, want in ((G.bags, G.qb), (G.corpus, G.cb)):
        ptr, items, w = got.to_numpy()
        assert same(ptr, want[0]) and same(items, want[1]) and same(w, want[2])
    assert G.index.ntotal == 400 and len(G.bags) == 48 and G.index.n_types == 12
    b = G.index.bags
    assert torch.equal(b.ptr, G.corpus.ptr) and torch.equal(b.items, G.corpus.items) and torch.equal(b.weights, G.corpus.weights)
    # n_types defaults to the largest type + 1; a torch table serves as well
    auto = pt.type_bags(truth()[2]["corpus"], torch.from_numpy(G.t["item_type"]).to(cuda), device=cuda)
    assert torch.equal(auto.ptr, G.corpus.ptr) and torch.equal(auto.items, G.corpus.items) and torch.equal(auto.weights, G.corpus.weights)


def test_fixture_search_equals_the_helper(cuda):
    G = gold(cuda)
    for k in (1, 20, 100, 400, 401, 1024):
        D, I = (x.cpu().numpy() for x in G.index.search(G.bags, k))
        Dr, Ir = tr.topk(G.s, k)
        assert same(I, Ir) and same(D, Dr), k
        assert (I[:, 400:] == -1).all() and (D[:, 400:] == -tr.FLT_MAX).all()
    assert G.index.last_chunks == 1


def test_fixture_bands_equal_the_helper(cuda):
    G = gold(cuda)
    above = [(float(np.nextafter(th, np.inf)),) for th in G.g["thres"]]
    for edges in (*EDGE_SETS, *above, (0.0,), (1.0,), (1.5,), SEVEN):
        counts, first = (x.cpu().numpy() for x in G.index.bands(G.bags, edges))
        cr, fr = tr.bands(G.s, edges)
        assert counts.shape == (48, len(edges) + 1) and same(counts, cr) and same(first, fr), edges
        assert (counts.sum(1) == 400).all()
    assert (tr.bands(G.s, (1.0,))[0][:, 1] > 0).any() and (tr.bands(G.s, (1.5,))[1][:, 1] == -1).all()


def test_fixture_mine_triples_equals_the_restated_loop(cuda):
    G = gold(cuda)
    for lo, hi in EDGE_SETS:
        m = pt.mine_triples(G.index, G.bags, lo, hi)
        ids, sc, keep = tr.mine(G.s, lo, hi)
        assert same(np.stack([m.pos, m.half, m.neg], 1), ids)
        assert same(np.stack([m.pos_score, m.half_score, m.neg_score], 1), sc)
        assert same(m.keep, keep) and int(m.keep.sum()) >= 10 and m.pos_score.dtype == np.float64


def test_fixture_pair_scores_equal_the_helper_and_the_reference(cuda):
    G = gold(cuda)
    I = G.g["I"].copy()
    got = G.index.pair_scores(I, G.bags)
    assert got.dtype == np.float64 and same(got, np.take_along_axis(G.s, I, axis=1))
    ref = np.take_along_axis(G.t["ref_all_product_type_score"], I, axis=1)
    d = tr.ulp_distance(ref, got)
    print("pair scores: largest distance from the reference in ulp:", int(d.max()), "tolerance:", int(G.t["tol_ulp"]))
    assert (d <= int(G.t["tol_ulp"])).all()
    I[3, 5:] = -1                                                    # missing neighbours are nan
    I[7] = -1
    got = G.index.pair_scores(I, G.bags)
    want = np.where(I >= 0, np.take_along_axis(G.s, np.maximum(I, 0), axis=1), np.nan)
    assert same(got, want) and np.isnan(got[7]).all()
    # every pair of the fixture, 400 neighbours a query
    every = np.tile(np.arange(400, dtype=np.int64), (48, 1))
    assert same(G.index.pair_scores(every, G.bags), G.s)
    with pytest.raises(_lib.SssError, match="outside"):
        G.index.pair_scores(np.full((48, 2), 400, np.int64), G.bags)


def test_fixture_neighbourhood_recall_equals_the_helper(cuda):
    G = gold(cuda)
    I = G.g["I"].copy()
    I[3, 5:] = -1
    for thres in (0.0, 0.1, 0.25, 0.5, 0.8):
        got = pt.neighbourhood_recall(I, G.index, G.bags, thres)
        want = tr.recall(I, G.s, thres)
        assert got == want and 0 < got[0] <= 1, (thres, got, want)


def test_fixture_drop_ins_against_the_reference(cuda):
    """The comparison tests/test_eval_metrics_gpu.py applies to ref_ave_all_jaccard and ref_recall_*: get_ave_score is the
    reference's float32 pairwise mean (AVE_TOL), get_recall two float64 means of the same nq integers (GAMMA)."""
    G = gold(cuda)
    I, thres = G.g["I"], G.g["thres"]
    nq, K = I.shape
    v = evaluation.get_ave_score(I, G.bags, G.corpus, SIM)
    print("get_ave_score:", v, "reference:", float(G.t["ref_ave"]), "bound:", AVE_TOL(nq * K))
    assert type(v) is float and abs(v - float(G.t["ref_ave"])) <= AVE_TOL(nq * K)
    s32 = np.take_along_axis(G.s, I, axis=1).astype(np.float32)
    assert abs(v - float(s32.astype(np.float64).sum()) / s32.size) <= GAMMA(I.size)      # the device's own order of the float64 sum
    for th, want in zip(thres, G.t["ref_recall"]):
        r = evaluation.get_recall(G.bags, G.corpus, I, SIM, float(th))
        print(f"get_recall > {th}: {r}, reference {float(want)}, bound {GAMMA(nq)}")
        assert type(r) is float and abs(r - float(want)) <= GAMMA(nq)
        assert r == float(np.mean((s32 > np.float32(th)).sum(1).astype(np.float64))) / K
    miss = I.copy()
    miss[0] = -1                                                     # a missing neighbour scores 0
    s0 = np.where(miss >= 0, s32, np.float32(0))
    assert abs(evaluation.get_ave_score(miss, G.bags, G.corpus, SIM) - float(s0.astype(np.float64).sum()) / s0.size) <= GAMMA(I.size)
    assert evaluation.get_recall(G.bags, G.corpus, miss, SIM, 0.0) == float(np.mean((s0 > 0).sum(1).astype(np.float64))) / K


def test_empty_index_and_empty_batch(cuda):
    G = gold(cuda)
    empty = pt.ProductTypeIndex(12, cuda)
    D, I = empty.search(G.bags, 3)
    counts, first = empty.bands(G.bags, (0.2, 0.8))
    assert (I == -1).all() and (D == -tr.FLT_MAX).all() and (counts == 0).all() and (first == -1).all() and counts.shape == (48, 3)
    m = pt.mine_triples(empty, G.bags)
    assert not m.keep.any() and np.isnan(m.pos_score).all()
    none = sparse.SessionVectors(G.bags.ptr[:1], G.bags.items, G.bags.weights)
    D, I = G.index.search(none, 3)
    counts, first = G.index.bands(none, (0.5,))
    assert tuple(D.shape) == (0, 3) and tuple(I.shape) == (0, 3) and tuple(counts.shape) == (0, 2) and tuple(first.shape) == (0, 2)
    with pytest.raises(ValueError):
        G.index.bands(G.bags, (0.8, 0.2))
    with pytest.raises(ValueError):
        G.index.search(G.bags, 1025)
    with pytest.raises(ValueError):                                  # a type id beyond the index's vocabulary
        pt.ProductTypeIndex(5, cuda).add(G.corpus)


# ------------------------------------------------------------------------------------------------ kernel edges
SHORT, LONG = (0, 1, DEPTH - 1, DEPTH), (DEPTH + 1, 40)


def edge_case():
    """(corpus, queries, float64 scores), made once.  Types come from a vocabulary of 50, so most pairs share a type; counts
    are 1..5.  Rows, 64 to a wave and 4 waves to a workgroup: wave 0 short rows only (0, 1, DEPTH - 1, DEPTH distinct types:
    the LDS form), waves 1 / 2 / 3 short but for ONE long row at lane 0 / lane 63 / lane 30 (the global form beside wave 0's
    LDS form inside one workgroup); wave 4 long rows only (DEPTH + 1 and 40), wave 5 short with DEPTH its longest, wave 6 the
    same but for one row of DEPTH + 1, waves 7 and 8 short, wave 9 the partial last wave of 37 rows whose last row has 40
    types.  n = 613.  Named rows: 1 = {0: 1} (0.8 against query 3 and 0.5 against query 4, exactly), 5 = {7: 64} (a count of
    64), 9 = {0: 8, 1: 6} (parallel to query 3)."""
    if "edge" in _CACHE:
        return _CACHE["edge"]
    rng = np.random.default_rng(20261020)
    draw = lambda m: dict(zip(np.sort(rng.choice(N_TYPES, m, replace=False)).tolist(), rng.integers(1, 6, m).tolist()))
    lengths = []
    for w in range(10):
        ln = [SHORT[(w + i) % 4] for i in range(64 if w < 9 else 37)]
        if w in (1, 2, 3):
            ln[{1: 0, 2: 63, 3: 30}[w]] = LONG[w % 2]
        if w == 4:
            ln = [LONG[i % 2] for i in range(64)]
        if w == 6:
            ln[17] = DEPTH + 1
        if w == 9:
            ln[-1] = 40
        lengths += ln
    rows = [draw(m) for m in lengths]
    rows[1], rows[5], rows[9] = {0: 1}, {7: 64}, {0: 8, 1: 6}
    scaled = lambda r, f: {t: c * f for t, c in r.items()}
    qs = [{}, {7: 1}, draw(40), {0: 4, 1: 3}, {0: 1, 5: 1, 9: 1, 11: 1}, draw(5), draw(DEPTH), draw(DEPTH + 1),
          scaled(rows[64], 2), dict(rows[-1]), scaled(rows[4 * 64 + 3], 3), dict(rows[2]), {7: 64}, {49: 2}, {0: 3}, draw(N_TYPES)]
    c, q = tr.triple(rows), tr.triple(qs)
    _CACHE["edge"] = (c, q, tr.scores(q, c, N_TYPES))
    return _CACHE["edge"]


def test_edge_case_has_every_kind_of_wave_and_pair():
    c, q, s = edge_case()
    ln = np.diff(c[0])
    n = len(ln)
    assert n == 613 and n % 256 and n % 64 == 37 and set(ln.tolist()) >= {0, 1, DEPTH - 1, DEPTH, DEPTH + 1, 40}
    long_lanes = [np.flatnonzero(ln[w * 64:(w + 1) * 64] > DEPTH).tolist() for w in range(10)]
    assert long_lanes[0] == [] and long_lanes[1] == [0] and long_lanes[2] == [63] and long_lanes[3] == [30]       # one workgroup
    assert len(long_lanes[4]) == 64 and long_lanes[5] == [] and ln[5 * 64:6 * 64].max() == DEPTH and long_lanes[6] == [17]
    assert long_lanes[9] == [36] and ln[-1] == 40
    assert np.diff(q[0]).tolist()[:3] == [0, 1, 40] and c[2].max() == 64 and q[2].max() == 64
    assert (s[0] == 0).all() and (ln == 0).sum() > 50                 # the empty query: every pair 0, empty rows included
    assert s[3, 1] == 0.8 and s[4, 1] == 0.5 and s[3, 9] == 1.0       # exactly on the edges; exactly parallel
    assert s[8, 64] == 1.0 and s[9, n - 1] == 1.0 and s[10, 4 * 64 + 3] == 1.0 and s[11, 2] == 1.0 and s[12, 5] == 1.0
    assert ((s > 0) & (s < 1)).mean() > 0.3                           # the walks mostly end with a partial overlap
    assert len(np.unique(s.astype(np.float32))) > 1000 and (np.sort(s, 1)[:, -21] == np.sort(s, 1)[:, -20]).any()


def raw_topk(cb, qb, q_first, nq, c_first, n, k, off, stream=None):
    D, I = Buf((nq, k), torch.float32), Buf((nq, k), torch.int64)
    ws = Buf(int(L().sss_ptype_topk_workspace_bytes(nq, n)), torch.uint8)
    run_twice(lambda: L().sss_ptype_topk(qb[0].ptr + 8 * q_first, qb[1].ptr, qb[2].ptr, nq, cb[0].ptr + 8 * c_first, cb[1].ptr, cb[2].ptr, n, k,
                                         off, D.ptr, I.ptr, ws.ptr, ws.nbytes, _st(stream)), [D, I], [ws])
    return D.t.cpu().numpy(), I.t.cpu().numpy()


def raw_bands(cb, qb, q_first, nq, c_first, n, edges, off, stream=None):
    nb = len(edges) + 1
    counts, first = Buf((nq, nb), torch.int64), Buf((nq, nb), torch.int64)
    e = (ctypes.c_double * len(edges))(*edges)
    run_twice(lambda: L().sss_ptype_bands(qb[0].ptr + 8 * q_first, qb[1].ptr, qb[2].ptr, nq, cb[0].ptr + 8 * c_first, cb[1].ptr, cb[2].ptr, n,
                                          ctypes.addressof(e), len(edges), off, counts.ptr, first.ptr, _st(stream)), [counts, first])
    return counts.t.cpu().numpy(), first.t.cpu().numpy()


def raw_pairs(cb, qb, q_first, nq, c_first, n, I, off, stream=None):
    Ib = dev_buf(I)
    out, err = Buf(I.shape, torch.float64), Buf(1, torch.int32)
    run_twice(lambda: L().sss_ptype_pair_scores(qb[0].ptr + 8 * q_first, qb[1].ptr, qb[2].ptr, nq, cb[0].ptr + 8 * c_first, cb[1].ptr, cb[2].ptr,
                                                n, Ib.ptr, I.shape[1], off, out.ptr, err.ptr, _st(stream)), [out, err])
    assert Ib.guards_ok() and np.array_equal(Ib.t.cpu().numpy(), I)
    return out.t.cpu().numpy(), int(err.t[0])


def pair_ids(nq, n, K, off, seed):
    """I [nq, K]: random rows of the sub-batch + off, its first and last row for every query, a run of -1, one query without
    a neighbour."""
    rng = np.random.default_rng(seed)
    I = rng.integers(0, n, (nq, K)).astype(np.int64)
    I[:, 0], I[:, K - 1] = 0, n - 1
    I += off
    I[1, K // 3:2 * K // 3 + 1] = -1
    I[2] = -1
    return I


def pairs_ref(s, I, off):
    r = I - off
    ok = (I != -1) & (r >= 0) & (r < s.shape[1])
    return np.where(ok, np.take_along_axis(s, np.clip(r, 0, s.shape[1] - 1), axis=1), np.nan)


def edge_bufs(cuda):
    if "bufs" not in _CACHE:
        c, q, _ = edge_case()
        _CACHE["bufs"] = ([dev_buf(x) for x in c], [dev_buf(x) for x in q])
    return _CACHE["bufs"]


@pytest.mark.parametrize("c_first,n", [(0, 613), (0, 1), (64, 1), (0, 255), (0, 256), (0, 257), (5, 300), (612, 1), (357, 256)])
def test_raw_calls_on_guarded_buffers(cuda, c_first, n):
    """Sub-batches `ptr + first_row` of both triples (the queries start at row 3 except for the whole corpus): rows past the
    sub-batch are the rest of the edge corpus, which would change counts and ranks if read.  (64, 1): one long row and 63
    idle lanes; (612, 1): the 40-type last row alone; (357, 256): a workgroup of other wave kinds than (0, 256)'s."""
    c, q, s = edge_case()
    cb, qb = edge_bufs(cuda)
    before = [b.t.clone() for b in (*cb, *qb)]
    q_first = 0 if n == 613 else 3
    nq = len(q[0]) - 1 - q_first
    ss = s[q_first:, c_first:c_first + n]
    for k in sorted({1, min(n, 70), n + 3}):
        D, I = raw_topk(cb, qb, q_first, nq, c_first, n, k, OFF)
        Dr, Ir = tr.topk(ss, k, OFF)
        assert same(I, Ir) and same(D, Dr), k
    for edges in ((0.2, 0.8), (0.2, 0.5), (0.0,), SEVEN):
        counts, first = raw_bands(cb, qb, q_first, nq, c_first, n, edges, OFF)
        cr, fr = tr.bands(ss, edges, OFF)
        assert same(counts, cr) and same(first, fr), edges
        assert (counts.sum(1) == n).all()
    if n == 613:
        assert first[0, 0] == OFF and counts[0, 0] == n               # the empty query: everything in band 0 of SEVEN
        assert counts[3, 7] >= 1 and first[3, 7] == 9 + OFF           # SEVEN's top band (>= 1.0): the parallel row
        c28, f28 = tr.bands(ss, (0.2, 0.8), OFF)
        assert f28[3, 2] == 1 + OFF                                   # the row exactly on 0.8 is the first of the top band
    for K in (1, 64, 70):
        I = pair_ids(nq, n, K, OFF, 1000 * n + K)
        out, err = raw_pairs(cb, qb, q_first, nq, c_first, n, I, OFF)
        assert err == 0 and same(out, pairs_ref(ss, I, OFF)), K
        assert np.isnan(out[2]).all() and not np.isnan(out[0]).any()
    for b, was in zip((*cb, *qb), before):
        assert b.guards_ok() and torch.equal(b.t, was), "an input was modified"


def test_raw_calls_one_query_zero_offset_and_a_side_stream(cuda):
    c, q, s = edge_case()
    cb, qb = edge_bufs(cuda)
    side = torch.cuda.Stream()
    for f in (0, 2, 9):                                              # the empty query, the 40-type one, the last row's twin
        D, I = raw_topk(cb, qb, f, 1, 0, 613, 10, 0, side)
        Dr, Ir = tr.topk(s[f:f + 1], 10)
        assert same(I, Ir) and same(D, Dr)
        counts, first = raw_bands(cb, qb, f, 1, 0, 613, (0.2, 0.8), 0, side)
        cr, fr = tr.bands(s[f:f + 1], (0.2, 0.8))
        assert same(counts, cr) and same(first, fr)
        ids = np.arange(613, dtype=np.int64)[None, :]
        out, err = raw_pairs(cb, qb, f, 1, 0, 613, ids, 0, side)
        assert err == 0 and same(out, s[f:f + 1])
    # both bags empty: score 0, and the band of the edge 0.0 (0 >= 0.0)
    counts, first = raw_bands(cb, qb, 0, 1, 0, 1, (0.0,), 0)
    assert counts.tolist() == [[0, 1]] and first.tolist() == [[-1, 0]] and np.diff(c[0])[0] == 0


def test_pair_scores_ids_outside_the_corpus(cuda):
    """One id below id_offset, one at id_offset + n (a row the larger triple does hold) and one far away: err == 1, all three
    nan, every other pair as without them."""
    c, q, s = edge_case()
    cb, qb = edge_bufs(cuda)
    nq, n, c_first = len(q[0]) - 1, 300, 5
    I = pair_ids(nq, n, 20, OFF, 7)
    I[0, 4], I[5, 19], I[7, 0] = OFF - 1, OFF + n, 5                  # 5 is a valid row only without the offset
    out, err = raw_pairs(cb, qb, 0, nq, c_first, n, I, OFF)
    want = pairs_ref(s[:, c_first:c_first + n], I, OFF)
    assert err == 1 and same(out, want) and np.isnan([out[0, 4], out[5, 19], out[7, 0]]).all()
    assert int(np.isnan(out).sum()) == int((I == -1).sum()) + 3


def test_index_on_the_edge_case_runs_bit_identically_twice(cuda):
    c, q, s = edge_case()
    index = pt.ProductTypeIndex(N_TYPES, cuda).add(dev(c, cuda))
    index.id_offset = OFF
    qd = dev(q, cuda)
    D, I = (x.clone() for x in index.search(qd, 100))
    D2, I2 = index.search(qd, 100)
    assert torch.equal(D, D2) and torch.equal(I, I2)
    Dr, Ir = tr.topk(s, 100, OFF)
    assert same(I.cpu().numpy(), Ir) and same(D.cpu().numpy(), Dr)
    b1 = [x.clone() for x in index.bands(qd, SEVEN)]
    b2 = index.bands(qd, SEVEN)
    assert torch.equal(b1[0], b2[0]) and torch.equal(b1[1], b2[1])
    p1 = index.pair_scores(I, qd)
    assert same(p1, index.pair_scores(I, qd)) and same(p1, pairs_ref(s, I.cpu().numpy(), OFF))
    assert same(p1.astype(np.float32), D.cpu().numpy())               # the top-k's scores are float32 of the pair scores
    sl = sparse.SessionVectors(qd.ptr[5:12], qd.items, qd.weights)   # a sliced query batch
    counts, first = index.bands(sl, (0.2, 0.8))
    cr, fr = tr.bands(s[5:11], (0.2, 0.8), OFF)
    assert same(counts.cpu().numpy(), cr) and same(first.cpu().numpy(), fr)
    m = pt.mine_triples(index, qd)
    ids, sc, keep = tr.mine(s)
    assert same(np.stack([m.pos, m.half, m.neg], 1), np.where(ids >= 0, ids + OFF, -1)) and same(np.stack([m.pos_score, m.half_score, m.neg_score], 1), sc)
    half = pt.ProductTypeIndex(N_TYPES, cuda).add(sparse.SessionVectors(qd.ptr[:1], qd.items, qd.weights))      # adds nothing
    part = dev(c, cuda)
    half.add(sparse.SessionVectors(part.ptr[:301], part.items, part.weights)).add(sparse.SessionVectors(part.ptr[300:], part.items, part.weights))
    assert half.ntotal == 613 and torch.equal(half.bags.ptr, index.bags.ptr) and torch.equal(half.bags.items, index.bags.items)
    assert torch.equal(half.bags.weights, index.bags.weights)


def test_query_chunks_of_seven(cuda, monkeypatch):
    """The score budget of search decides the chunk (exhaustive_chunk); bands has no matrix and keeps one call."""
    G = gold(cuda)
    D1, I1 = (x.clone() for x in G.index.search(G.bags, 20))
    assert G.index.last_chunks == 1
    monkeypatch.setattr(sparse, "exhaustive_chunk", lambda n, bytes_per_score: 7)       # CsrIndex._pieces reads it
    D7, I7 = G.index.search(G.bags, 20)
    assert G.index.last_chunks == 7 and torch.equal(D1, D7) and torch.equal(I1, I7)
    G.index.bands(G.bags, (0.2, 0.8))
    assert G.index.last_chunks == 1


def test_more_queries_than_one_call_takes(cuda):
    """70 000 queries against 3 rows: the Python layer splits at the 65 535 queries one call takes, for search and bands
    alike.  The queries repeat with period 97, so every one of them has a helper result."""
    nq, period, n_types = 70000, 97, 30
    rng = np.random.default_rng(70)
    pick = lambda m: dict(zip(np.sort(rng.choice(n_types, m, replace=False)).tolist(), rng.integers(1, 4, m).tolist()))
    c = tr.triple([pick(20), pick(2), pick(0)])
    base = [pick(int(m)) for m in rng.integers(0, 6, period)]
    q = tr.triple([base[f % period] for f in range(nq)])
    index = pt.ProductTypeIndex(n_types, cuda).add(dev(c, cuda))
    qd = dev(q, cuda)
    s = tr.scores(tr.triple(base), c, n_types)[np.arange(nq) % period]
    D, I = index.search(qd, 4)
    assert index.last_chunks == 2
    Dr, Ir = tr.topk(s, 4)
    assert same(I.cpu().numpy(), Ir) and same(D.cpu().numpy(), Dr) and (Ir[:, 3] == -1).all() and (Dr[:, 0] > 0).sum() > 30000
    counts, first = index.bands(qd, (0.1, 0.3))
    assert index.last_chunks == 2
    cr, fr = tr.bands(s, (0.1, 0.3))
    assert same(counts.cpu().numpy(), cr) and same(first.cpu().numpy(), fr) and len(np.unique(cr, axis=0)) > 3
    I3 = np.tile(np.arange(3, dtype=np.int64), (nq, 1))
    assert same(index.pair_scores(I3, qd), s)


def test_the_largest_counts_the_contract_allows(cuda):
    """A row's sum of squared counts up to 2^26: dot up to 2^26 and nq2 * nc2 up to 2^52 stay exact; beyond it, a count that
    is no positive integer, and a bag on the host are refused once per batch."""
    rows = [{0: 8192}, {0: 1}, {0: 8191, 1: 127}, {1: 8192}, {0: 4096, 1: 4096, 2: 4096, 3: 4096}, {0: 3, 1: 4}]
    assert 8191 ** 2 + 127 ** 2 <= 2 ** 26 and 4 * 4096 ** 2 == 2 ** 26
    c = tr.triple(rows)
    s = tr.scores(c, c, 4)
    assert s[0, 0] == 1.0 and s[0, 3] == 0 and s[4, 4] == 1.0 and 0 < s[0, 2] < 1 and s[2, 2] == 1.0
    index = pt.ProductTypeIndex(4, cuda).add(dev(c, cuda))
    qd = dev(c, cuda)
    D, I = index.search(qd, 6)
    Dr, Ir = tr.topk(s, 6)
    assert same(I.cpu().numpy(), Ir) and same(D.cpu().numpy(), Dr)
    assert same(index.pair_scores(np.tile(np.arange(6, dtype=np.int64), (6, 1)), qd), s)
    counts, first = index.bands(qd, (0.5, 1.0))
    cr, fr = tr.bands(s, (0.5, 1.0))
    assert same(counts.cpu().numpy(), cr) and same(first.cpu().numpy(), fr)
    for bad in ([{0: 8192, 1: 1}], [{0: 1}, {0: 8193}], [{0: 0}], [{0: 1.5}], [{0: -2}], [{0: float("nan")}], [{0: float("inf")}]):
        with pytest.raises(ValueError, match="2\\^26"):
            index.search(dev(tr.triple(bad), cuda), 1)
    with pytest.raises(ValueError, match="2\\^26"):
        pt.ProductTypeIndex(4, cuda).add(dev(tr.triple([{0: 8192, 3: 1}]), cuda))
    with pytest.raises(_lib.SssError):
        index.search(sparse.SessionVectors(*(torch.from_numpy(x) for x in c)), 1)
    with pytest.raises(TypeError):
        index.search(np.zeros((2, 4), np.float32), 1)


# ------------------------------------------------------------------------------------------------ the builder
def table(sessions):
    """ActionTable of sessions given as lists of item ids, None = a search."""
    flat = [a for s in sessions for a in s]
    return ActionTable(np.r_[0, np.cumsum([len(s) for s in sessions], dtype=np.int64)].astype(np.int64),
                       np.array([a is None for a in flat], bool), np.array([0 if a is None else a for a in flat], np.int64),
                       np.zeros(len(flat), np.int64))


def expected_bags(sessions, item_type, n_types):
    """(helper triple with every flagged session an empty row, the err word)."""
    rows, flags = [], 0
    for s in sessions:
        clicks = [a for a in s if a is not None]
        f = (1 if len(clicks) > 64 else 0) | (2 if any(not 0 <= a < len(item_type) for a in clicks) else 0)
        f |= 4 if any(0 <= a < len(item_type) and not -1 <= item_type[a] < n_types for a in clicks) else 0
        flags |= f
        bag = {}
        if not f:
            for a in clicks:
                if item_type[a] >= 0:
                    bag[int(item_type[a])] = bag.get(int(item_type[a]), 0) + 1
        rows.append(bag)
    return tr.triple(rows), flags


def raw_bags(tab, item_type, n_types, want, stream=None):
    """sss_type_bags_count + _fill through ctypes on guarded, exactly sized buffers, twice; the prefix sum is the helper's."""
    S = tab.num_sessions
    sp, isr, item = dev_buf(tab.sess_ptr), dev_buf(tab.is_search.astype(np.uint8)), dev_buf(tab.item_id)
    ty, ptr = dev_buf(item_type), dev_buf(want[0])
    nnz = int(want[0][-1])
    counts, err = Buf(S, torch.int32), Buf(1, torch.int32)
    items, w = Buf(nnz, torch.int32), Buf(nnz, torch.float32)
    n_items = len(item_type)

    def call():
        rc = L().sss_type_bags_count(sp.ptr, isr.ptr, item.ptr, S, ty.ptr, n_items, n_types, counts.ptr, err.ptr, _st(stream))
        return rc or L().sss_type_bags_fill(sp.ptr, isr.ptr, item.ptr, S, ty.ptr, n_items, n_types, ptr.ptr, items.ptr, w.ptr, err.ptr,
                                            _st(stream))
    run_twice(call, [counts, err, items, w])
    for b in (sp, isr, item, ty, ptr):
        assert b.guards_ok()
    return counts.t.cpu().numpy(), items.t.cpu().numpy(), w.t.cpu().numpy(), int(err.t[0])


def builder_sessions():
    """Sessions at the builder's edges over 40 items: empty, searches only, untyped items only, one type through three items
    and three times through one (a count of 3 either way), exactly 64 item actions of one type (a count of 64), 64 item
    actions among 90 actions (more than one 64-action step), every type once, 64 item actions among exactly 128 and among 129
    actions, the last action an item action (two full steps; a third step of one action), and 300 random ones."""

    def spread(n_raw):
        r = np.random.default_rng(n_raw)
        s = [None] * n_raw
        for at in (*r.choice(n_raw - 1, 63, replace=False), n_raw - 1):
            s[at] = int(r.integers(0, 40))
        return s
    rng = np.random.default_rng(64)
    item_type = rng.integers(0, 9, 40).astype(np.int32)
    item_type[[3, 11, 30]] = -1
    item_type[[0, 1, 2]] = 5
    item_type[39] = 8
    mixed = [None] * 90
    for i, at in enumerate(np.sort(rng.choice(90, 64, replace=False))):
        mixed[at] = int(rng.integers(0, 40))
    fixed = [[], [None, None], [3, 11, 30, 3], [0, 1, 2], [2, 2, None, 2], [39] * 64, mixed, list(range(40)), spread(128), spread(129)]
    rand = [[None if rng.random() < 0.3 else int((rng.zipf(1.3) - 1) % 40) for _ in range(int(rng.integers(1, 20)))] for _ in range(300)]
    return fixed + rand, item_type


def test_builder_equals_the_helper_on_guarded_buffers(cuda):
    sessions, item_type = builder_sessions()
    want, flags = expected_bags(sessions, item_type, 9)
    tab = table(sessions)
    helper = tr.bags(tab, item_type)
    assert flags == 0 and all(same(a, b) for a, b in zip(want, helper))
    counts, items, w, err = raw_bags(tab, item_type, 9, want, torch.cuda.Stream())
    assert err == 0 and same(counts.astype(np.int64), np.diff(want[0])) and same(items, want[1]) and same(w, want[2])
    assert np.diff(want[0])[:6].tolist() == [0, 0, 0, 1, 1, 1] and want[2][:3].tolist() == [3, 3, 64] and w.max() == 64
    got = pt.type_bags(tab, item_type, 9, cuda)
    assert all(same(a, b) for a, b in zip(got.to_numpy(), want))
    one = pt.type_bags(table([[39, 0, 39]]), item_type, device=cuda)         # one session; n_types from the table
    assert one.items.tolist() == [5, 8] and one.weights.tolist() == [1.0, 2.0]
    assert len(pt.type_bags(table([]), item_type, device=cuda)) == 0


@pytest.mark.parametrize("bit", [1, 2, 4, 7])
def test_builder_error_bits_give_an_empty_row_and_the_right_exception(cuda, bit):
    """Bit 1: 65 item actions; bit 2: an item id of n_items, and a negative one; bit 4: a type id of n_types, and one of -2.
    The flagged sessions are empty rows, their neighbours are as without them, and type_bags raises."""
    sessions, item_type = builder_sessions()
    item_type = item_type.copy()
    sessions = [list(s) for s in sessions[:40]]
    if bit & 1:
        sessions[9] = [4] * 65
    if bit & 2:
        sessions[12], sessions[13] = [1, 40, 2], [-1]
    if bit & 4:
        item_type[20], item_type[21] = 9, -2
        sessions[17], sessions[18] = [5, 20, 5], [21, None]
    want, flags = expected_bags(sessions, item_type, 9)
    assert flags == bit
    tab = table(sessions)
    counts, items, w, err = raw_bags(tab, item_type, 9, want)
    assert err == bit and same(counts.astype(np.int64), np.diff(want[0])) and same(items, want[1]) and same(w, want[2])
    for s, on in ((9, 1), (12, 2), (13, 2), (17, 4), (18, 4)):
        if bit & on:
            assert counts[s] == 0
    assert counts.sum() > 30
    msg = {1: "more than 64", 2: "item id", 4: "type id", 7: "more than 64"}[bit]
    with pytest.raises(_lib.SssError, match=msg):
        pt.type_bags(tab, item_type, 9, cuda)


def test_every_argument_error_launches_nothing(cuda):
    """tests/test_type_score_cpu.py's checks again where a launch would be possible: none of the addresses is memory."""
    check_argument_errors(L())
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ sharding
def test_rccl_one_rank_exchange_route(cuda):
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", HSA_ENABLE_IPC_MODE_LEGACY="0")
    res = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "helpers", "rccl_one_rank_ptype.py"), str(port)],
                         capture_output=True, text=True, timeout=600, env=env, cwd=ROOT)
    lines = [ln for ln in res.stdout.splitlines() if ln.startswith("{")]
    assert res.returncode == 0 and lines, f"child failed (rc {res.returncode}):\n{res.stdout[-2000:]}\n{res.stderr[-4000:]}"
    out = json.loads(lines[-1])
    assert out["ok"] and out["backend"] == "nccl" and out["world"] == 1 and all(out["checks"].values()), out
