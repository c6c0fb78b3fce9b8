"""The ground-truth index on the device (include/sss_jaccard.h, csrc/jaccard.hip, sessionsimilaritysearch_amd/jaccard.py).

Fixture parity: on the sessions of tests/golden/eval_metrics.npz, search, bands, mine_triples and neighbourhood_recall are
array_equal to the numpy helper of tests/helpers/jaccard_ref.py, which tests/test_jaccard_cpu.py holds bit for bit to the
matrices the reference's own get_score produced (tests/golden/jaccard_truth.npz); the scores are compared with float32 of
the reference's directly as well.

Kernel edges: both entry points through ctypes on exactly sized, guarded buffers, run twice from two poisons, at the
smallest shapes where the walk of csrc/jaccard.hip can go wrong: rows around the DEPTH items a thread keeps in LDS, every
kind of wave, corpus sizes around the 256-row workgroup, sub-batches of both triples, the ends of the vocabulary."""
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
import jaccard_ref as jr  # noqa: E402
import sparse_ref  # noqa: E402

from sessionsimilaritysearch_amd import evaluation, jaccard, sparse  # noqa: E402
from test_abi_contract_gpu import OFF, Buf, L, _st, dev_buf, run_twice  # noqa: E402
from test_eval_metrics_cpu import golden, host_parts  # noqa: E402
from test_jaccard_cpu import SIM_PART, TRUTH, check_argument_errors  # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEPTH = 32                           # JC_D of csrc/jaccard.hip
TOP = 2 ** 31 - 2                    # the largest item id
SEVEN = (0.1, 0.2, 0.25, 1 / 3, 0.5, 0.8, 1.0)
_CACHE = {}


def dev(pair, cuda):
    return sparse._device_triple(pair[0], pair[1], np.zeros(len(pair[1]), np.float32), cuda)


# ------------------------------------------------------------------------------------------------ fixture parity
def gold(cuda):
    if "gold" not in _CACHE:
        g, tab = golden()
        seq, tar = tab["query"].split(1, 2)
        host, corpus_host = host_parts(tab), sparse_ref.vectors(tab["corpus"], "binary")[:2]
        index = jaccard.JaccardIndex(int(g["n_items"]), cuda).add(sparse.session_vectors(tab["corpus"], "binary", device=cuda))
        _CACHE["gold"] = types.SimpleNamespace(g=g, truth=np.load(TRUTH), parts=evaluation.query_parts(seq, tar, cuda), index=index,
                                               r={sim: jr.ratios(host[p], corpus_host) for sim, p in SIM_PART.items()})
    return _CACHE["gold"]


@pytest.mark.parametrize("sim", ["all_jaccard", "cur_jaccard"])
def test_fixture_search_equals_the_helper_and_the_reference(cuda, sim):
    G = gold(cuda)
    q, r = getattr(G.parts, SIM_PART[sim]), G.r[sim]
    assert G.index.ntotal == 400 and len(q) == 48
    for k in (1, 20, 100, 400, 401, 1024):
        D, I = (t.cpu().numpy() for t in G.index.search(q, k))
        Dr, Ir = jr.topk(r, k)
        assert np.array_equal(I, Ir) and np.array_equal(D, Dr), k
        kk = min(k, 400)
        assert np.array_equal(D[:, :kk], np.take_along_axis(G.truth[f"ref_{sim}"], I[:, :kk], axis=1).astype(np.float32))
        assert (I[:, 400:] == -1).all() and (D[:, 400:] == -jr.FLT_MAX).all()
    assert G.index.last_chunks == 1


@pytest.mark.parametrize("sim", ["all_jaccard", "cur_jaccard"])
def test_fixture_bands_equal_the_helper(cuda, sim):
    G = gold(cuda)
    q, r = getattr(G.parts, SIM_PART[sim]), G.truth[f"ref_{sim}"]
    for edges in ((0.2, 0.8), (0.2, 0.5), (0.0,), (1.0,), (1.5,), SEVEN):
        counts, first = (t.cpu().numpy() for t in G.index.bands(q, edges))
        cr, fr = jr.bands(r, edges)
        assert counts.dtype == np.int64 and first.dtype == np.int64 and counts.shape == (48, len(edges) + 1)
        assert np.array_equal(counts, cr) and np.array_equal(first, fr), edges
        assert (counts.sum(1) == 400).all()
    if sim == "all_jaccard":
        assert (jr.bands(r, (0.2, 0.8))[1][:, 2] == -1).all()                     # the empty top band


@pytest.mark.parametrize("sim", ["all_jaccard", "cur_jaccard"])
def test_fixture_mine_triples_equals_the_restated_loop(cuda, sim):
    G = gold(cuda)
    q, r = getattr(G.parts, SIM_PART[sim]), G.truth[f"ref_{sim}"]
    for lo, hi, kept in ((0.2, 0.8, {"all_jaccard": 0, "cur_jaccard": 2}), (0.2, 0.5, {"all_jaccard": 14, "cur_jaccard": 16})):
        t = jaccard.mine_triples(G.index, q, lo, hi)
        ids, sc, keep = jr.mine(r, lo, hi)
        assert np.array_equal(np.stack([t.pos, t.half, t.neg], 1), ids)
        assert np.array_equal(np.stack([t.pos_score, t.half_score, t.neg_score], 1), sc, equal_nan=True)
        assert np.array_equal(t.keep, keep) and int(t.keep.sum()) == kept[sim] and t.pos_score.dtype == np.float64


@pytest.mark.parametrize("sim", ["all_jaccard", "cur_jaccard"])
def test_fixture_neighbourhood_recall_equals_the_helper(cuda, sim):
    G = gold(cuda)
    q, r = getattr(G.parts, SIM_PART[sim]), G.truth[f"ref_{sim}"]
    I = G.g["I"].copy()
    I[3, 5:] = -1                                                    # missing neighbours never count
    for thres in (0.0, 0.1, 0.25, 0.5):
        got = jaccard.neighbourhood_recall(I, G.index, q, thres)
        want = jr.recall(I, r, thres)
        assert got == want and 0 < got[0] <= 1, (thres, got, want)
    assert jaccard.neighbourhood_recall(I, G.index, q, 0.5)[1] > 0   # some query has no row above 0.5: skipped and counted


def test_empty_index_and_empty_batch(cuda):
    G = gold(cuda)
    empty = jaccard.JaccardIndex(600, cuda)
    D, I = empty.search(G.parts.cur, 3)
    counts, first = empty.bands(G.parts.cur, (0.2, 0.8))
    assert (I == -1).all() and (D == -jr.FLT_MAX).all() and (counts == 0).all() and (first == -1).all() and counts.shape == (48, 3)
    none = sparse.SessionVectors(G.parts.cur.ptr[:1], G.parts.cur.items, G.parts.cur.weights)
    D, I = G.index.search(none, 3)
    counts, first = G.index.bands(none, (0.5,))
    assert tuple(D.shape) == (0, 3) and tuple(I.shape) == (0, 3) and tuple(counts.shape) == (0, 2) and tuple(first.shape) == (0, 2)
    with pytest.raises(ValueError):
        G.index.bands(G.parts.cur, (0.8, 0.2))
    with pytest.raises(ValueError):
        G.index.search(G.parts.cur, 1025)


# ------------------------------------------------------------------------------------------------ kernel edges
SHORT, LONG = (0, 1, DEPTH - 1, DEPTH), (DEPTH + 1, 64, 65, 200)


def edge_case():
    """(corpus, queries, float64 ratios), made once.  Items come from a pool of 400 ids that holds 0 and 2^31 - 2, so that
    most pairs intersect.  Rows, 64 to a wave and 4 waves to a workgroup: wave 0 short rows only (0, 1, DEPTH - 1, DEPTH
    items), waves 1 / 2 / 3 short but for ONE long row at lane 0 / lane 63 / lane 30; wave 4 long rows only (DEPTH + 1, 64,
    65, 200), wave 5 short with DEPTH its longest, wave 6 the same but for one row of DEPTH + 1, wave 7 short; wave 8 short,
    wave 9 the partial last wave of 37 rows whose last row has 200 items.  n = 613."""
    if "edge" in _CACHE:
        return _CACHE["edge"]
    rng = np.random.default_rng(20261019)
    pool = np.unique(np.r_[0, TOP, rng.integers(1, TOP, 398)]).astype(np.int64)
    draw = lambda m: np.sort(rng.choice(pool, m, replace=False))
    lengths = []
    for w in range(10):
        ln = [SHORT[(w + i) % 4] for i in range(64 if w < 9 else 37)]
        if w in (1, 2, 3):
            ln[{1: 0, 2: 63, 3: 30}[w]] = LONG[w]
        if w == 4:
            ln = [LONG[i % 4] for i in range(64)]
        if w == 6:
            ln[17] = DEPTH + 1
        if w == 9:
            ln[-1] = 200
        lengths += ln
    rows = [draw(m) for m in lengths]
    rows[5] = np.asarray([0, TOP])
    rows[64] = np.unique(np.r_[0, draw(63)[1:-1], TOP])             # the long row at lane 0 holds both ends of the vocabulary
    qs = [draw(m) for m in (0, 1, 64, 300, 5, 17, DEPTH, DEPTH + 1)]
    qs += [np.asarray([0]), np.asarray([TOP]), np.asarray([0, TOP]), rows[64].copy(), rows[-1].copy(), rows[4 * 64 + 3].copy(),
           rows[2].copy(), pool.copy()]
    c, q = sparse_ref_sets(rows), sparse_ref_sets(qs)
    _CACHE["edge"] = (c, q, jr.ratios(q, c))
    return _CACHE["edge"]


def sparse_ref_sets(rows):
    ptr = np.zeros(len(rows) + 1, np.int64)
    np.cumsum([len(r) for r in rows], out=ptr[1:])
    return ptr, np.concatenate([np.asarray(r, np.int64) for r in rows] + [np.zeros(0, np.int64)]).astype(np.int32)


def test_edge_case_has_every_kind_of_wave_and_pair():
    c, q, r = edge_case()
    ln = np.diff(c[0])
    n = len(ln)
    assert n == 613 and n % 256 and n % 64 == 37 and set(ln.tolist()) >= {0, 1, DEPTH - 1, DEPTH, DEPTH + 1, 64, 65, 200}
    long_lanes = [np.flatnonzero(ln[w * 64:(w + 1) * 64] > DEPTH).tolist() for w in range(10)]
    assert long_lanes[0] == [] and long_lanes[1] == [0] and long_lanes[2] == [63] and long_lanes[3] == [30]       # one workgroup
    assert len(long_lanes[4]) == 64 and long_lanes[5] == [] and ln[5 * 64:6 * 64].max() == DEPTH and long_lanes[6] == [17]
    assert long_lanes[9] == [36] and ln[-1] == 200
    assert set(np.diff(q[0]).tolist()) >= {0, 1, 64, 300} and c[1].min() == 0 and c[1].max() == TOP
    assert (r[0] == 0).all() and (ln == 0).sum() > 50                 # the empty query: every pair 0, empty rows included
    assert r[11, 64] == 1.0 and r[12, n - 1] == 1.0 and r[13, 4 * 64 + 3] == 1.0 and r[14, 2] == 1.0       # identical sets
    assert (r[12] == 1.0).sum() == 1                                  # ... the last row of the last workgroup alone
    assert ((r > 0) & (r < 1)).mean() > 0.3                           # the walks mostly end with a partial intersection


def raw_topk(cb, qb, q_first, nq, c_first, n, k, off, stream=None):
    D, I = Buf((nq, k), torch.float32), Buf((nq, k), torch.int64)
    ws = Buf(int(L().sss_jaccard_topk_workspace_bytes(nq, n)), torch.uint8)
    run_twice(lambda: L().sss_jaccard_topk(qb[0].ptr + 8 * q_first, qb[1].ptr, nq, cb[0].ptr + 8 * c_first, cb[1].ptr, n, k, off, D.ptr,
                                           I.ptr, ws.ptr, ws.nbytes, _st(stream)), [D, I], [ws])
    return D.t.cpu().numpy(), I.t.cpu().numpy()


def raw_bands(cb, qb, q_first, nq, c_first, n, edges, off, stream=None):
    nb = len(edges) + 1
    counts, first = Buf((nq, nb), torch.int64), Buf((nq, nb), torch.int64)
    e = (ctypes.c_double * len(edges))(*edges)
    run_twice(lambda: L().sss_jaccard_bands(qb[0].ptr + 8 * q_first, qb[1].ptr, nq, cb[0].ptr + 8 * c_first, cb[1].ptr, n,
                                            ctypes.addressof(e), len(edges), off, counts.ptr, first.ptr, _st(stream)),
              [counts, first])
    return counts.t.cpu().numpy(), first.t.cpu().numpy()


def edge_bufs(cuda):
    if "bufs" not in _CACHE:
        c, q, _ = edge_case()
        _CACHE["bufs"] = ([dev_buf(x) for x in c], [dev_buf(x) for x in q])
    return _CACHE["bufs"]


@pytest.mark.parametrize("c_first,n", [(0, 613), (0, 1), (64, 1), (0, 255), (0, 256), (0, 257), (5, 300), (612, 1), (357, 256)])
def test_raw_calls_on_guarded_buffers(cuda, c_first, n):
    """Sub-batches `ptr + first_row` of both triples (the queries start at row 3 except for the whole corpus): rows past the
    sub-batch are the rest of the edge corpus, which would change counts and ranks if read.  (64, 1): one long row and 63
    idle lanes; (612, 1): the 200-item last row alone; (357, 256): a workgroup of other wave kinds than (0, 256)'s."""
    c, q, r = edge_case()
    cb, qb = edge_bufs(cuda)
    before = [b.t.clone() for b in (*cb, *qb)]
    q_first = 0 if n == 613 else 3
    nq = len(q[0]) - 1 - q_first
    rr = r[q_first:, c_first:c_first + n]
    for k in sorted({1, min(n, 70), n + 3}):
        D, I = raw_topk(cb, qb, q_first, nq, c_first, n, k, OFF)
        Dr, Ir = jr.topk(rr, k, OFF)
        assert np.array_equal(I, Ir) and np.array_equal(D, Dr), k
    for edges in ((0.2, 0.8), (0.0,), SEVEN):
        counts, first = raw_bands(cb, qb, q_first, nq, c_first, n, edges, OFF)
        cr, fr = jr.bands(rr, edges, OFF)
        assert np.array_equal(counts, cr) and np.array_equal(first, fr), edges
        assert (counts.sum(1) == n).all()
    if n == 613:
        assert first[12, 7] == 612 + OFF and counts[12, 7] == 1      # the band whose only row is the last of the last workgroup
        assert first[0, 0] == OFF and counts[0, 0] == n               # the empty query: everything in band 0 of SEVEN
    for b, was in zip((*cb, *qb), before):
        assert b.guards_ok() and torch.equal(b.t, was), "an input was modified"


def test_raw_calls_one_query_zero_offset_and_a_side_stream(cuda):
    c, q, r = edge_case()
    cb, qb = edge_bufs(cuda)
    side = torch.cuda.Stream()
    for f in (0, 3, 12):                                             # the empty query, the 300-item one, the last row's twin
        D, I = raw_topk(cb, qb, f, 1, 0, 613, 10, 0, side)
        Dr, Ir = jr.topk(r[f:f + 1], 10)
        assert np.array_equal(I, Ir) and np.array_equal(D, Dr)
        counts, first = raw_bands(cb, qb, f, 1, 0, 613, (0.2, 0.8), 0, side)
        cr, fr = jr.bands(r[f:f + 1], (0.2, 0.8))
        assert np.array_equal(counts, cr) and np.array_equal(first, fr)
    # both sets empty: score 0, and the band of the edge 0.0 (0 >= 0.0)
    counts, first = raw_bands(cb, qb, 0, 1, 0, 4, (0.0,), 0)
    assert counts.tolist() == [[0, 4]] and first.tolist() == [[-1, 0]] and np.diff(c[0])[0] == 0


def test_index_on_the_edge_case_runs_bit_identically_twice(cuda):
    c, q, r = edge_case()
    index = jaccard.JaccardIndex(2 ** 31 - 1, cuda).add(dev(c, cuda))
    index.id_offset = OFF
    qd = dev(q, cuda)
    D, I = (t.clone() for t in index.search(qd, 100))
    D2, I2 = index.search(qd, 100)
    assert torch.equal(D, D2) and torch.equal(I, I2)
    Dr, Ir = jr.topk(r, 100, OFF)
    assert np.array_equal(I.cpu().numpy(), Ir) and np.array_equal(D.cpu().numpy(), Dr)
    sl = sparse.SessionVectors(qd.ptr[5:12], qd.items, qd.weights)   # a sliced query batch
    counts, first = index.bands(sl, (0.2, 0.8))
    cr, fr = jr.bands(r[5:11], (0.2, 0.8), OFF)
    assert np.array_equal(counts.cpu().numpy(), cr) and np.array_equal(first.cpu().numpy(), fr)
    half = jaccard.JaccardIndex(2 ** 31 - 1, cuda).add(sparse.SessionVectors(qd.ptr[:1], qd.items, qd.weights))      # adds nothing
    part = dev(c, cuda)
    half.add(sparse.SessionVectors(part.ptr[:301], part.items, part.weights)).add(sparse.SessionVectors(part.ptr[300:], part.items, part.weights))
    assert half.ntotal == 613 and torch.equal(half.sets.ptr, index.sets.ptr) and torch.equal(half.sets.items, index.sets.items)


def test_query_chunks_of_seven(cuda, monkeypatch):
    """The score budget of search decides the chunk (exhaustive_chunk); bands has no matrix and keeps one call."""
    G = gold(cuda)
    D1, I1 = (t.clone() for t in G.index.search(G.parts.all, 20))
    assert G.index.last_chunks == 1
    monkeypatch.setattr(sparse, "exhaustive_chunk", lambda n, bytes_per_score: 7)       # CsrIndex._pieces reads it
    D7, I7 = G.index.search(G.parts.all, 20)
    assert G.index.last_chunks == 7 and torch.equal(D1, D7) and torch.equal(I1, I7)
    G.index.bands(G.parts.all, (0.2, 0.8))
    assert G.index.last_chunks == 1


def test_more_queries_than_one_call_takes(cuda):
    """70 000 queries against 3 rows: the Python layer splits at the 65 535 queries one call takes, for search and bands
    alike.  The queries repeat with period 97, so every one of them has a helper result."""
    nq, period, n_items = 70000, 97, 30
    rng = np.random.default_rng(70)
    pick = lambda m: np.sort(rng.choice(n_items, m, replace=False))
    c = sparse_ref_sets([pick(20), pick(2), pick(0)])
    base = [pick(int(m)) for m in rng.integers(0, 6, period)]
    q = sparse_ref_sets([base[f % period] for f in range(nq)])
    index = jaccard.JaccardIndex(n_items, cuda).add(dev(c, cuda))
    qd = dev(q, cuda)
    r = jr.ratios(sparse_ref_sets(base), c)[np.arange(nq) % period]
    D, I = index.search(qd, 4)
    assert index.last_chunks == 2
    Dr, Ir = jr.topk(r, 4)
    assert np.array_equal(I.cpu().numpy(), Ir) and np.array_equal(D.cpu().numpy(), Dr) and (Ir[:, 3] == -1).all() and (Dr[:, 0] > 0).sum() > 30000
    counts, first = index.bands(qd, (0.1, 0.3))
    assert index.last_chunks == 2
    cr, fr = jr.bands(r, (0.1, 0.3))
    assert np.array_equal(counts.cpu().numpy(), cr) and np.array_equal(first.cpu().numpy(), fr) and len(np.unique(cr, axis=0)) > 3


def test_every_argument_error_launches_nothing(cuda):
    """tests/test_jaccard_cpu.py's checks again where a launch would be possible: none of the addresses is memory."""
    check_argument_errors(L())
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ sharding
def test_rccl_one_rank_exchange_route(cuda):
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", HSA_ENABLE_IPC_MODE_LEGACY="0")
    res = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "helpers", "rccl_one_rank_jaccard.py"), str(port)],
                         capture_output=True, text=True, timeout=600, env=env, cwd=ROOT)
    lines = [ln for ln in res.stdout.splitlines() if ln.startswith("{")]
    assert res.returncode == 0 and lines, f"child failed (rc {res.returncode}):\n{res.stdout[-2000:]}\n{res.stderr[-4000:]}"
    out = json.loads(lines[-1])
    assert out["ok"] and out["backend"] == "nccl" and out["world"] == 1 and all(out["checks"].values()), out
