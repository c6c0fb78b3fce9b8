"""Scoring a search result on the device (include/sss_eval.h, csrc/overlap.hip, sessionsimilaritysearch_amd/evaluation.py).

Golden: on tests/golden/eval_metrics.npz `inter` / `csize` are equal to the python-set restatement of
tests/helpers/eval_ref.py, `out` is bit-equal to its canonical loop (float64, ascending j), and every drop-in is within
its derived bound of the value the reference's own function returned -- the bounds GAMMA / AVE_TOL are stated and
derived at the head of tests/test_eval_metrics_cpu.py, which holds the helper itself to them.

Edges: sss_item_overlap and sss_overlap_metrics through ctypes on exactly sized, guarded outputs, run twice from two
poisons (every entry written, bit-equal between the runs), at the sizes where csrc/overlap.hip takes another path: the
64 neighbours a wave owns per step, the CAP query items it stages, the LONG items a lane walks alone, the 32-neighbour and
64-query tiles of the reduction."""
import os
import sys
import types

import numpy as np
import pytest
import scipy.sparse
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import eval_ref as ev  # noqa: E402
import sparse_ref  # noqa: E402

from sessionsimilaritysearch_amd import evaluation, sparse  # noqa: E402
from sessionsimilaritysearch_amd.sessions import ActionTable  # noqa: E402
from test_abi_contract_gpu import OFF, Buf, L, _st, dev_buf, run_twice  # noqa: E402
from test_eval_metrics_cpu import GAMMA, check_against_reference, golden, host_parts  # noqa: E402

pytestmark = pytest.mark.gpu

CAP, LONG = 2048, 64                 # OV_QCAP and OV_LONG of csrc/overlap.hip
TOP = 2 ** 31 - 2                    # the largest item id
_CACHE = {}


def bits(x):
    return np.ascontiguousarray(x).view(np.int64)


# ------------------------------------------------------------------------------------------------ golden
def gold(cuda):
    if "gold" not in _CACHE:
        g, tab = golden()
        seq, tar = tab["query"].split(1, 2)
        _CACHE["gold"] = types.SimpleNamespace(g=g, host=host_parts(tab), corpus_host=sparse_ref.vectors(tab["corpus"], "binary")[:2],
                                               parts=evaluation.query_parts(seq, tar, cuda),
                                               corpus=sparse.session_vectors(tab["corpus"], "binary", device=cuda))
    return _CACHE["gold"]


@pytest.mark.parametrize("part", ev.PARTS)
def test_golden_overlap_and_sums_equal_the_helper(cuda, part):
    G = gold(cuda)
    I = G.g["I"]
    q = getattr(G.parts, part)
    assert np.array_equal(q.ptr.cpu().numpy(), G.host[part][0]) and np.array_equal(q.items.cpu().numpy(), G.host[part][1])
    inter, csize, err = ev.overlap(G.host[part], G.corpus_host, I)
    for thres in (None, 0.1, 0.25):
        s = evaluation.part_scores(torch.from_numpy(I).to(cuda), q, G.corpus, thres)
        assert s.inter.dtype == torch.int32 and s.inter.is_cuda and tuple(s.csize.shape) == I.shape
        assert np.array_equal(s.inter.cpu().numpy(), inter) and np.array_equal(s.csize.cpu().numpy(), csize)
        out, flags = ev.metrics(inter, csize, np.diff(G.host[part][0]), np.inf if thres is None else thres)
        assert np.array_equal(bits(s.out), bits(out)) and np.array_equal(s.flags, flags)
    a, c = evaluation.item_overlap(I.astype(np.int32), q, G.corpus)                # numpy ids, as find_K_sparse_dense returns them
    assert np.array_equal(a.cpu().numpy(), inter) and np.array_equal(c.cpu().numpy(), csize)


def test_golden_drop_ins_against_the_reference(cuda):
    G = gold(cuda)
    I, E = G.g["I"], evaluation
    single = {"cur_jaccard": E.get_cur_jaccard, "future_jaccard": E.get_future_jaccard, "all_jaccard": E.get_all_jaccard,
              "cur_recall": E.get_cur_recall, "future_recall": E.get_future_recall, "all_recall": E.get_all_recall,
              "cur_map": E.get_cur_map, "future_map": E.get_future_map, "all_map": E.get_all_map}

    def drop_in(key, thres):
        if key in single:
            v = single[key](I, G.parts, G.corpus)
        elif key.startswith("ave_"):
            v = E.get_ave_score(I, G.parts, G.corpus, key[4:])
        else:
            v = E.get_recall(G.parts, G.corpus, I, key[7:], thres)
        assert type(v) is float
        return v
    worst = check_against_reference(G.g, G.host, drop_in)
    print("largest |difference| / bound:", worst)
    # evaluate: the same figures from three overlap launches
    for thres in (None, 0.1):
        res = E.evaluate(I, G.parts, G.corpus, thres)
        want = ev.evaluate(I, G.host, G.corpus_host, thres)
        assert sorted(res) == sorted(want) and len(res) == (13 if thres is not None else 11)
        for k, v in res.items():
            assert v == drop_in(k, thres), k
            # the float64 sum of the float32 pair scores is the device's, in its own order
            assert (abs(v - want[k]) <= GAMMA(I.size) if k.startswith("ave_") else v == want[k]), k


# ------------------------------------------------------------------------------------------------ sss_item_overlap, edges
def edge_sets():
    """Corpus rows of 0, 1, LONG - 1, LONG, LONG + 1 and 5000 items and 60 more of mixed lengths, inside a larger triple
    (3 rows ahead, 2 behind, holding every pool item: a row read outside [first_row, first_row + n) shows); query rows
    of 0, 1, 64, CAP - 1, CAP and CAP + 1 items.  Items are drawn from a pool of 6 000 ids over the whole int32 range
    that holds 0 and 2^31 - 2, both of which are one-item rows on either side."""
    if "edge" in _CACHE:
        return _CACHE["edge"]
    rng = np.random.default_rng(2048)
    pool = np.unique(np.r_[0, TOP, rng.integers(1, TOP, 6000)])
    draw = lambda m: np.sort(rng.choice(pool, m, replace=False))
    special = [0, 1, LONG - 1, LONG, LONG + 1, 5000]
    rows = [draw(m) for m in special] + [np.array([0]), np.array([TOP])]
    rows += [draw(int(m)) for m in rng.choice([0, 1, 2, 5, 13, 63, 64, 65, 130], 58)]
    first_row, n = 3, len(rows)
    full = [pool] * first_row + rows + [pool] * 2
    qrows = [draw(m) for m in (0, 1, 64, CAP - 1, CAP, CAP + 1)] + [np.array([TOP]), np.array([0]), np.array([0, TOP]), draw(7), draw(300)]
    qrows[4] = np.unique(np.r_[0, TOP, qrows[4][1:-1]])                            # the CAP-item row holds both ends
    assert len(qrows[4]) == CAP and [len(r) for r in qrows[:6]] == [0, 1, 64, CAP - 1, CAP, CAP + 1]
    cp, ci = ev.sets_of(full)
    qp, qi = ev.sets_of(qrows)
    m = scipy.sparse.csr_matrix((np.ones(len(qi), np.float32), qi, qp), shape=(len(qrows), 2 ** 31 - 1))
    _CACHE["edge"] = types.SimpleNamespace(q=(qp, qi), c=ev.sets_of(rows), full=(cp, ci), first_row=first_row, n=n, nq=len(qrows),
                                           qd=sparse.csr_to_vectors(m, "cuda"), cb=[dev_buf(cp), dev_buf(ci)], special=special)
    e = _CACHE["edge"]
    assert np.array_equal(e.qd.ptr.cpu().numpy(), qp) and np.array_equal(e.qd.items.cpu().numpy(), qi)
    return e


def edge_ids(e, K, off):
    """I [nq, K]: random rows; every query meets the six special rows (K >= 6; in turn for smaller K), the same
    neighbour twice and three times in one row, a run of -1 padding, and query 3 has no neighbour at all."""
    rng = np.random.default_rng(K)
    I = rng.integers(0, e.n, (e.nq, K)).astype(np.int64)
    if K <= 2:
        I[:, 0] = (np.arange(e.nq) + K) % 6
    else:
        I[:, K - 1] = I[:, K // 2] = I[:, K // 2 - 1] = I[:, 0]
        free = np.setdiff1d(np.arange(K), [0, K - 1, K // 2, K // 2 - 1])
        for i in range(e.nq):
            I[i, rng.choice(free, 6, replace=False)] = np.arange(6)
    I += off
    if K > 1:
        I[2, K // 3:2 * K // 3 + 1] = -1
    I[3] = -1
    return I


def call_overlap(e, I, off, stream=None):
    """sss_item_overlap through ctypes on guarded outputs, twice; the corpus is `ptr + first_row` of the larger triple."""
    nq, K = I.shape
    Ib = dev_buf(I)
    inter, csize, err = Buf((nq, K), torch.int32), Buf((nq, K), torch.int32), Buf(1, torch.int32)
    run_twice(lambda: L().sss_item_overlap(e.qd.ptr.data_ptr(), e.qd.items.data_ptr(), nq, e.cb[0].ptr + 8 * e.first_row, e.cb[1].ptr, e.n,
                                           Ib.ptr, K, off, inter.ptr, csize.ptr, err.ptr, _st(stream)), [inter, csize, err])
    assert Ib.guards_ok() and all(b.guards_ok() for b in e.cb) and np.array_equal(Ib.t.cpu().numpy(), I)
    return inter.t.cpu().numpy(), csize.t.cpu().numpy(), int(err.t[0])


@pytest.mark.parametrize("K,off", [(1, 0), (63, OFF), (64, 0), (65, OFF), (100, -7), (1024, OFF)])
def test_overlap_edges(cuda, K, off):
    e = edge_sets()
    I = edge_ids(e, K, off)
    stream = torch.cuda.Stream() if K == 100 else None               # a non-default stream
    inter, csize, err = call_overlap(e, I, off, stream)
    ri, rc, rerr = ev.overlap(e.q, e.c, I, off)
    assert rerr == 0 and err == 0                                    # -1 is padding, not an error
    assert np.array_equal(csize, rc) and np.array_equal(inter, ri)
    assert (csize[3] == -1).all() and (inter[3] == 0).all()
    if K > 2:
        assert set(e.special) <= set(rc[0].tolist()) and (ri[4] > 1000).any() and (ri[5] > 1000).any()


def test_overlap_ids_outside_the_corpus(cuda):
    """One id below id_offset, one at id_offset + n (a row the larger triple does hold) and one far away: err == 1,
    all three missing, every other pair as without them."""
    e = edge_sets()
    I = edge_ids(e, 20, OFF)
    good, _, _ = ev.overlap(e.q, e.c, I, OFF)
    I[0, 4], I[5, 19], I[7, 0] = OFF - 1, OFF + e.n, 5                # 5 is a valid row only without the offset
    inter, csize, err = call_overlap(e, I, OFF)
    ri, rc, rerr = ev.overlap(e.q, e.c, I, OFF)
    assert err == 1 == rerr and np.array_equal(inter, ri) and np.array_equal(csize, rc)
    assert [csize[0, 4], csize[5, 19], csize[7, 0]] == [-1, -1, -1] and [inter[0, 4], inter[5, 19], inter[7, 0]] == [0, 0, 0]
    keep = np.ones(I.shape, bool)
    keep[0, 4] = keep[5, 19] = keep[7, 0] = False
    assert np.array_equal(inter[keep], good[keep])
    with pytest.raises(evaluation._lib.SssError, match="outside"):
        evaluation.item_overlap(I, e.qd, sparse._device_triple(e.c[0], e.c[1], np.ones(len(e.c[1]), np.float32), cuda), OFF)


@pytest.mark.parametrize("nq,K", [(1, 5), (70000, 2)])
def test_overlap_one_query_and_seventy_thousand(cuda, nq, K):
    """nq = 1: three idle waves in the workgroup.  nq = 70 000: more workgroups than a 65 535 grid dimension holds; the
    queries repeat with period 97, so the overlap of every (query, row) pair is a table of 97 x 50."""
    rng = np.random.default_rng(nq)
    period, n = 97, 50
    base = [np.sort(rng.choice(40, int(m), replace=False)) for m in rng.integers(0, 9, period)]
    crows = [np.sort(rng.choice(40, int(m), replace=False)) for m in rng.integers(0, 9, n)]
    table = np.array([[len(set(a.tolist()) & set(b.tolist())) for b in crows] for a in base], np.int32)
    qp, qi = ev.sets_of([base[i % period] for i in range(nq)])
    cp, ci = ev.sets_of(crows)
    I = rng.integers(0, n, (nq, K)).astype(np.int64)
    I[nq // 2, 0] = -1
    qb, cb, Ib = [dev_buf(qp), dev_buf(qi)], [dev_buf(cp), dev_buf(ci)], dev_buf(I + OFF * (I >= 0))
    inter, csize, err = Buf((nq, K), torch.int32), Buf((nq, K), torch.int32), Buf(1, torch.int32)
    run_twice(lambda: L().sss_item_overlap(qb[0].ptr, qb[1].ptr, nq, cb[0].ptr, cb[1].ptr, n, Ib.ptr, K, OFF, inter.ptr, csize.ptr, err.ptr,
                                           _st()), [inter, csize, err])
    want = np.where(I >= 0, table[np.arange(nq)[:, None] % period, np.maximum(I, 0)], 0)
    assert int(err.t[0]) == 0 and np.array_equal(inter.t.cpu().numpy(), want)
    assert want.max() >= (4 if nq > 1 else 1)                        # the expectation itself is not all zeros
    assert np.array_equal(csize.t.cpu().numpy(), np.where(I >= 0, np.diff(cp)[np.maximum(I, 0)], -1))
    for b in (*qb, *cb, Ib):
        assert b.guards_ok()


# ------------------------------------------------------------------------------------------------ sss_overlap_metrics, edges
def call_metrics(inter, csize, qsize, thr):
    nq, K = inter.shape
    ib, cb, qb = dev_buf(inter.astype(np.int32)), dev_buf(csize.astype(np.int32)), dev_buf(np.asarray(qsize, np.int32))
    out, flags = Buf((nq, 4), torch.float64), Buf(nq, torch.int32)
    run_twice(lambda: L().sss_overlap_metrics(ib.ptr, cb.ptr, qb.ptr, nq, K, thr, out.ptr, flags.ptr, _st()), [out, flags])
    for b in (ib, cb, qb):
        assert b.guards_ok()
    return out.t.cpu().numpy(), flags.t.cpu().numpy()


def random_pairs(rng, nq, K):
    """Well-formed (inter, csize, qsize): inter <= min(qsize, csize); a fifth of the neighbours missing; rows without a
    hit, with a hit at every rank, with no neighbour at all, empty queries and empty-union pairs."""
    qsize = rng.integers(0, 12, nq)
    csize = rng.integers(0, 12, (nq, K))
    inter = rng.integers(0, 12, (nq, K)) % (np.minimum(qsize[:, None], csize) + 1)
    csize[rng.random((nq, K)) < 0.2] = -1
    for i in range(0, nq, 5):
        kind = (i // 5) % 4
        if kind == 0:
            csize[i] = -1                                            # all missing
        elif kind == 1:
            inter[i] = 0                                             # no hit
        elif kind == 2:
            qsize[i], csize[i] = 3, np.maximum(csize[i], 1)          # a hit at every rank
            inter[i] = 1
        else:
            qsize[i], csize[i, ::2] = 0, 0                           # an empty query, empty-union pairs
    inter[csize < 0] = 0
    inter = np.minimum(inter, np.minimum(qsize[:, None], np.maximum(csize, 0)))
    return inter, csize, qsize


@pytest.mark.parametrize("nq,K", [(1, 1), (3, 20), (64, 32), (65, 33), (130, 100), (7, 1024)])
def test_metrics_bit_equal_the_canonical_loop(cuda, nq, K):
    rng = np.random.default_rng(nq * 10000 + K)
    inter, csize, qsize = random_pairs(rng, nq, K)
    for thr in (0.25, -1.0, float("inf")):
        out, flags = call_metrics(inter, csize, qsize, thr)
        rout, rflags = ev.metrics(inter, csize, qsize, thr)
        assert np.array_equal(bits(out), bits(rout)) and np.array_equal(flags, rflags), thr
    if nq >= 20:
        assert (rflags & 1).any() and (rflags & 2).any() and (rout[:, 2] == 1.0).any() and (csize < 0).all(axis=1).any()


def test_metrics_named_edges(cuda):
    """Row 0: every neighbour missing.  Row 1: qsize 0 against non-empty rows (flag 2).  Row 2: qsize 0 against an empty
    row, union 0 (flags 1 | 2).  Row 3: scores 1/3, 1/4, 1/2 under thr = float32(1/3): strict >, only 1/2 counts.
    Row 4: a missing neighbour ahead of two hits keeps its rank, AP = (1/2 + 2/3) / 2."""
    inter = np.array([[0, 0, 0], [0, 0, 0], [0, 0, 0], [1, 1, 2], [0, 1, 1]])
    csize = np.array([[-1, -1, -1], [2, 5, 1], [0, 3, -1], [1, 2, 3], [-1, 1, 4]])
    qsize = np.array([4, 0, 0, 3, 2])
    thr = float(np.float32(1.0 / 3.0))
    out, flags = call_metrics(inter, csize, qsize, thr)
    rout, rflags = ev.metrics(inter, csize, qsize, thr)
    assert np.array_equal(bits(out), bits(rout)) and np.array_equal(flags, rflags)
    assert flags.tolist() == [0, 2, 3, 0, 0] and out[0].tolist() == [0, 0, 0, 0] and out[1].tolist() == [0, 0, 0, 0]
    assert np.float32(np.float64(1) / np.float64(3)) == np.float32(thr) and out[3, 3] == 1.0
    assert out[3, 0] == 1 / 3 + 1 / 4 + 2 / 4 and out[3, 2] == 1.0
    assert out[4, 2] == (np.float64(1) / 2 + np.float64(2) / 3) / 2 and out[4, 1] == 1.0
    one, _ = call_metrics(inter[3:4], csize[3:4], qsize[3:4], float(np.nextafter(np.float32(thr), np.float32(0))))
    assert one[0, 3] == 2.0                                          # one float32 step below 1/3: 1/3 counts


def test_empty_union_raises_where_the_reference_divides_by_zero(cuda):
    """A query whose `all` set is empty meets a search-only corpus session: get_all_jaccard, get_ave_score('all_jaccard')
    and evaluate raise ZeroDivisionError as the reference's unguarded division does; 'cur_jaccard' scores the pair 0."""
    t = lambda sessions: ActionTable(np.r_[0, np.cumsum([len(s) for s in sessions])].astype(np.int64),
                                     np.array([a is None for s in sessions for a in s], bool),
                                     np.array([0 if a is None else a for s in sessions for a in s], np.int64),
                                     np.zeros(sum(len(s) for s in sessions), np.int64))
    corpus = sparse.session_vectors(t([[1, 2], [None, None], [2, 3, 4]]), "binary", device=cuda)
    seq, tar = t([[None, None, 1, None], [1, 2, None, 5]]).split(1, 2)        # query 0: cur is empty, all is {1}; query 1: all is {1, 2, 5}
    parts = evaluation.query_parts(seq, tar, cuda)
    I = np.array([[0, 1, 2], [0, 2, 1]])
    assert evaluation.get_ave_score(I, parts, corpus, "cur_jaccard") == float(np.float64(np.float32(2 / 2) + np.float32(1 / 4)) / 6)
    assert evaluation.get_all_jaccard(I, parts, corpus) == ((1 / 2 + 0 + 0) + (2 / 3 + 1 / 5 + 0)) / 2 / 3
    assert evaluation.get_cur_jaccard(I, parts, corpus) == (2 / 2 + 1 / 4 + 0) / 3          # query 0 is skipped
    seq0, tar0 = t([[None, None], [1, 2, None, 5]]).split(1, 2)                # query 0 has no item at all
    empty = evaluation.query_parts(seq0, tar0, cuda)
    for fn in (lambda: evaluation.get_all_jaccard(I, empty, corpus), lambda: evaluation.get_ave_score(I, empty, corpus, "all_jaccard"),
               lambda: evaluation.get_recall(empty, corpus, I, "all_jaccard", 0.5), lambda: evaluation.evaluate(I, empty, corpus)):
        with pytest.raises(ZeroDivisionError):
            fn()
    assert evaluation.get_ave_score(I, empty, corpus, "cur_jaccard") == float(np.float64(np.float32(1.0) + np.float32(0.25)) / 6)
    assert evaluation.get_all_recall(I, empty, corpus) == (2 / 3 + 1 / 3 + 0) / 3
    # a -1 in I: a missing neighbour, never the last session
    miss = evaluation.evaluate(np.array([[0, -1, 2], [-1, -1, -1]]), parts, corpus)
    assert miss["all_jaccard"] == (1 / 2 + 0 + 0) / 6 and miss["all_map"] == (1.0 + 0.0) / 2
