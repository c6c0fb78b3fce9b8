"""csrc/sparse.hip where it can go wrong without tests/test_sparse_index_gpu.py noticing: rows longer than the 16-entry LDS
column (the global-memory form of the merge walk, the per-wave choice between the forms, mixed blocks, a long row beside
the corpus end), the order and the precision of the score's sum, negative scores in the top-k, the ends of the
vocabulary, sliced and chunked query batches, and the vector builder over every small session structure, on the top
lanes, across the 64-action step and around its error flags at the C ABI.

Every comparison is `==` on D and I, or on ptr, items and weights, against the numpy float64 oracle of
tests/helpers/sparse_ref.py; stan weights alone keep the one-float32-ulp tolerance of tests/test_sparse_index_gpu.py
(the device's and numpy's float64 exp may differ in the last place).  tests/test_sparse_edges_cpu.py shows, on the
oracle alone, that these inputs tell a wrong order or a float32 sum from the contract's."""
import itertools
import os
import sys
import types

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import sparse_ref as ref  # noqa: E402

from sessionsimilaritysearch_amd import sparse  # noqa: E402
from test_abi_contract_gpu import OFF, Buf, _st, dev_buf, run_twice  # noqa: E402
from test_sparse_index_gpu import L, _action_bufs, table, ulp_diff  # noqa: E402

pytestmark = pytest.mark.gpu

_CACHE = {}


def dev(t, cuda):
    return sparse._device_triple(*t, cuda)


def assert_search(index, qd, s, k, off=0):
    """index.search(qd, k), run twice, == the oracle's top-k of the canonical scores `s`."""
    index.id_offset = off
    D, I = (t.clone() for t in index.search(qd, k))
    D2, I2 = index.search(qd, k)
    assert torch.equal(D, D2) and torch.equal(I, I2), "two runs differ"
    Dr, Ir = ref.topk(s, k, off)
    assert np.array_equal(I.cpu().numpy(), Ir) and np.array_equal(D.cpu().numpy(), Dr)
    return Dr, Ir


def edge(cuda):
    """The edge corpus of sparse_ref.edge_corpus, its queries, their canonical scores and the index (made once)."""
    if "edge" not in _CACHE:
        c = ref.edge_corpus()
        q = ref.edge_queries(c)
        _CACHE["edge"] = types.SimpleNamespace(c=c, q=q, s=ref.scores(q, c, ref.EDGE_ITEMS), qd=dev(q, cuda),
                                               index=sparse.SparseSessionIndex(ref.EDGE_ITEMS, cuda).add(dev(c, cuda)))
    return _CACHE["edge"]


# ------------------------------------------------------------------------ A. row length against the LDS column
def assert_every_kind_of_wave(ptr):
    """The corpus has, grouped as k_sparse_scores groups its rows (64 a wave, 4 waves a block): a block of four short
    waves, one of four long waves (one of them of long rows only), a block of short waves holding exactly one long row at
    lane 0, at lane 63 and mid-wave; a wave whose longest row is exactly 16 (the LDS form) beside one whose longest is
    17; a last wave with inactive lanes whose last row is long."""
    kinds = ref.wave_kinds(ptr)
    n = len(ptr) - 1
    blocks = [kinds[b:b + 4] for b in range(0, len(kinds), 4)]
    is_short = lambda k: k[0] <= 16 and k[1] == 0
    assert any(len(b) == 4 and all(is_short(k) for k in b) for b in blocks), "no block of four short waves"
    assert any(len(b) == 4 and all(k[1] > 0 for k in b) for b in blocks), "no block of four long waves"
    assert any(k[1] == k[3] == 64 for k in kinds), "no wave of long rows only"
    assert any(0 < k[1] < k[3] for k in kinds), "no wave of short and long rows"
    mixed = [b for b in blocks if len(b) == 4 and any(is_short(k) for k in b) and any(k[1] > 0 for k in b)]
    assert mixed, "no block of short and long waves"
    one = [k[2][0] for b in mixed for k in b if k[1] == 1]
    assert 0 in one and 63 in one and any(0 < lane < 63 for lane in one), one
    assert any(a[0] == 16 and b[0] == 17 for a, b in zip(kinds, kinds[1:])), "no wave at exactly 16 beside one at 17"
    assert n % 256 and n % 64 and kinds[-1][3] == n % 64 and kinds[-1][2][-1] == kinds[-1][3] - 1, "the last row is not a long row of a partial wave"


@pytest.mark.parametrize("k", [1, 10, 933, 936])
def test_long_rows_every_wave_kind(cuda, k):
    e = edge(cuda)
    assert_every_kind_of_wave(e.c[0])
    assert e.index.ntotal == 933 and len(e.qd) == 40
    assert set(np.diff(e.q[0]).tolist()) >= {0, 1, 2, 3, 9, 16, 17, 40, 94}
    Dr, Ir = assert_search(e.index, e.qd, e.s, k)
    if k == 936:
        assert (Ir[:, 933:] == -1).all() and (Ir[:, :933] >= 0).all()
        assert (Dr[:2, :933] == 0).all()                             # the queries below and above every row item
    assert e.index.last_chunks == 1


@pytest.mark.parametrize("n", [1, 257])
def test_long_rows_smallest_corpora(cuda, n):
    """n = 1: one 94-item row, 63 inactive lanes.  n = 257: the second block holds one row, a long one."""
    rng = np.random.default_rng(n)
    lengths = np.r_[rng.choice(ref.SHORT + ref.LONG, n - 1), 94 if n == 1 else 65].astype(np.int64)
    c = ref.edge_corpus(10 + n, lengths)
    q = edge(cuda).q
    s = ref.scores(q, c, ref.EDGE_ITEMS)
    index = sparse.SparseSessionIndex(ref.EDGE_ITEMS, cuda).add(dev(c, cuda))
    assert index.ntotal == n and ref.wave_kinds(c[0])[-1][:2] == (int(lengths[-1]), 1) and ref.wave_kinds(c[0])[-1][3] == 1
    for k in (1, n, n + 3):
        assert_search(index, edge(cuda).qd, s, k, off=OFF)


def test_long_rows_raw_call_reads_no_further_row(cuda):
    """sss_sparse_topk on guarded, exactly sized buffers.  The corpus is the head of a larger triple: 64 further rows
    hold every item of the vocabulary with weight 1e30, so a row read past n, or an entry read past the end of the
    long last row, would change a score beyond recognition."""
    e = edge(cuda)
    n, nq, k = 933, 40, 936
    tail = [(np.arange(ref.EDGE_ITEMS), np.full(ref.EDGE_ITEMS, 1e30, np.float32))] * 64
    tp, ti, tw = ref.triple(tail)
    full = (np.r_[e.c[0], e.c[0][-1] + tp[1:]], np.r_[e.c[1], ti], np.r_[e.c[2], tw])
    assert np.diff(full[0])[n - 1] == 65 and np.array_equal(full[0][:n + 1], e.c[0])
    cb, qb = [dev_buf(x) for x in full], [dev_buf(x) for x in e.q]
    before = [b.t.clone() for b in (*cb, *qb)]
    D, I = Buf((nq, k), torch.float32), Buf((nq, k), torch.int64)
    ws = Buf(int(L().sss_sparse_topk_workspace_bytes(nq, n)), torch.uint8)
    run_twice(lambda: L().sss_sparse_topk(qb[0].ptr, qb[1].ptr, qb[2].ptr, nq, cb[0].ptr, cb[1].ptr, cb[2].ptr, n, k, OFF, D.ptr, I.ptr,
                                          ws.ptr, ws.nbytes, _st()), [D, I], [ws])
    Dr, Ir = ref.topk(e.s, k, OFF)
    assert np.array_equal(I.t.cpu().numpy(), Ir) and np.array_equal(D.t.cpu().numpy(), Dr)
    for b, was in zip((*cb, *qb), before):
        assert b.guards_ok() and torch.equal(b.t, was), "an input was modified"


# ------------------------------------------------------------------------ B. sum order and signed scores
@pytest.mark.parametrize("k", [1, 100, 700])
def test_sum_order_and_signed_scores(cuda, k):
    """The batch of sparse_ref.sum_order_batch: a sum in another order, or in float32, changes a quarter of the scores
    and more (tests/test_sparse_edges_cpu.py); the top-k sorts negative, zero and positive scores with ties at zero by
    the hundred."""
    if "order" not in _CACHE:
        q, c, n_items = ref.sum_order_batch()
        _CACHE["order"] = (ref.scores(q, c, n_items), dev(q, cuda), sparse.SparseSessionIndex(n_items, cuda).add(dev(c, cuda)))
    s, qd, index = _CACHE["order"]
    assert index.ntotal == 700 and len(qd) == 24
    Dr, Ir = assert_search(index, qd, s, k)
    if k == 700:
        assert (Dr < 0).any() and (Dr > 0).any() and ((Dr == 0).sum(axis=1) > 64).all()


# ------------------------------------------------------------------------ C. vocabulary ends, slices, chunks
def test_vocabulary_ends(cuda):
    """Items 0 and 2^31 - 2 (one below the walk's sentinel) in rows and queries, in a wave of short rows (the LDS form)
    and in one with 17-item rows (the global form)."""
    V = 2 ** 31 - 1
    top = V - 1
    rng = np.random.default_rng(31)
    w = lambda m: (rng.standard_normal(m) + 2.0).astype(np.float32)
    mid = lambda m: np.sort(rng.choice(np.arange(1, top, 9973), m, replace=False))
    shapes = [lambda: [0, top], lambda: [0], lambda: [top], lambda: [], lambda: np.r_[0, mid(14), top], lambda: np.r_[mid(15), top],
              lambda: np.r_[0, mid(15)], lambda: mid(16)]
    rows = [np.asarray(shapes[r % len(shapes)](), np.int64) for r in range(64)]
    rows += [np.r_[0, mid(15), top], mid(17), np.r_[mid(16), top], np.r_[0, mid(16)], np.r_[0, mid(31), top], np.asarray([0, top])]
    c = ref.triple([(r, w(len(r))) for r in rows])
    qs = [np.asarray([0, top]), np.asarray([top]), np.asarray([0]), rows[64], np.r_[0, mid(15), top], np.r_[0, mid(38), top], rows[4]]
    q = ref.triple([(r, w(len(r))) for r in qs])
    kinds = ref.wave_kinds(c[0])
    assert kinds[0][:2] == (16, 0) and kinds[1][1] >= 5 and c[1].max() == top == 2 ** 31 - 2 and c[1].min() == 0
    s = ref.scores_pairs(q, c)
    assert (s[1] != 0).sum() >= 20 and (s[2] != 0).sum() >= 20                    # the end items alone score in both waves
    index = sparse.SparseSessionIndex(V, cuda).add(dev(c, cuda))
    for k in (1, 70):
        assert_search(index, dev(q, cuda), s, k, off=OFF)


def test_sliced_query_batch(cuda):
    """Rows 5..28 of the query batch as a slice (ptr[5:30], ptr[0] != 0, the whole batch's items and weights) == the
    same rows as a batch of their own == the oracle."""
    e = edge(cuda)
    sl = sparse.SessionVectors(e.qd.ptr[5:30], e.qd.items, e.qd.weights)
    assert len(sl) == 24 and int(sl.ptr[0]) != 0
    own = dev(ref.rows_of(e.q, 5, 29), cuda)
    assert int(own.ptr[0]) == 0 and own.items.numel() < e.qd.items.numel()
    for k in (10, 933):
        D, I = (t.clone() for t in e.index.search(sl, k))
        Do, Io = e.index.search(own, k)
        assert torch.equal(D, Do) and torch.equal(I, Io)
        assert_search(e.index, sl, e.s[5:29], k)


def test_query_chunks_of_seven(cuda, monkeypatch):
    e = edge(cuda)
    q37 = sparse.SessionVectors(e.qd.ptr[:38], e.qd.items, e.qd.weights)
    D1, I1 = (t.clone() for t in e.index.search(q37, 10))
    assert e.index.last_chunks == 1
    monkeypatch.setattr(sparse, "exhaustive_chunk", lambda n, bytes_per_score: 7)
    D6, I6 = e.index.search(q37, 10)
    assert e.index.last_chunks == 6 and torch.equal(D1, D6) and torch.equal(I1, I6)
    assert_search(e.index, q37, e.s[:37], 10)
    assert_search(e.index, q37, e.s[:37], 933, off=OFF)
    assert e.index.last_chunks == 6


def test_more_queries_than_one_call_takes(cuda):
    """65 536 + 3 queries against 3 rows: the Python chunker splits at the 65 535 queries one sss_sparse_topk takes.  The
    queries repeat with period 97, so every one of them has an oracle result."""
    nq, period, n_items = 65536 + 3, 97, 30
    rng = np.random.default_rng(65)
    c = ref.triple([ref._row(rng, 20, 0, n_items, False), ref._row(rng, 2, 0, n_items, False), ref._row(rng, 0, 0, n_items, False)])
    base = [ref._row(rng, int(m), 0, n_items, False) for m in rng.integers(0, 6, period)]
    q = ref.triple([base[f % period] for f in range(nq)])
    index = sparse.SparseSessionIndex(n_items, cuda).add(dev(c, cuda))
    D, I = index.search(dev(q, cuda), 4)
    assert index.last_chunks == 2
    Dr, Ir = ref.topk(ref.scores(ref.triple(base), c, n_items), 4)
    assert (Dr != 0).any(axis=1).sum() >= 30 and (Ir[:, 3] == -1).all()
    D, I, pick = D.cpu().numpy(), I.cpu().numpy(), np.arange(nq) % period
    for f in (0, 1, 65533, 65534, 65535, 65536, nq - 1):            # first, last and both sides of the split
        assert np.array_equal(D[f], Dr[f % period]) and np.array_equal(I[f], Ir[f % period]), f
    assert np.array_equal(D, Dr[pick]) and np.array_equal(I, Ir[pick])


# ------------------------------------------------------------------------ D. the builder
def assert_built(seqs, mode, cuda, lammy=1.04, n_items=None):
    a = table(seqs)
    v = sparse.session_vectors(a, mode, lammy if mode == "stan" else None, cuda, n_items=n_items)
    ptr, items, w = v.to_numpy()
    rp, ri, rw = ref.vectors(a, mode, lammy)
    assert np.array_equal(ptr, rp) and np.array_equal(items, ri) and items.dtype == np.int32 and w.dtype == np.float32
    if mode == "binary":
        assert np.array_equal(w, rw)
    else:
        d = ulp_diff(w, rw)                                          # int32 views: float32 denormals count
        assert d.max(initial=0) <= 1, (int(d.max()), int((d > 1).sum()), len(d))
    return ptr, items, w


SYM = (None, 7, 3, 5)                                                # a search, and three items whose order is not the symbols'


@pytest.mark.parametrize("mode", ["binary", "stan"])
def test_builder_every_small_structure(cuda, mode):
    """All 5 461 sessions of length 0..6 over {search, a, b, c} in one batch: every repeat and first-seen pattern, the
    rank order, stan sums over repeats."""
    seqs = [[SYM[x] for x in p] for n in range(7) for p in itertools.product(range(4), repeat=n)]
    assert len(seqs) == 5461
    assert_built(seqs, mode, cuda)


@pytest.mark.parametrize("mode", ["binary", "stan"])
@pytest.mark.parametrize("filler", ["distinct", "equal"])
def test_builder_every_length5_structure_on_the_top_lanes(cuda, mode, filler):
    """The 1 024 patterns of four items on lanes 59..63 of a 64-item-action session, behind 59 fillers: distinct ones
    (two of the four items are among them), or one item 59 times (one of the four)."""
    items = (2, 40, 99, 41)
    head = list(np.random.default_rng(59).permutation(np.arange(10, 69))) if filler == "distinct" else [40] * 59
    seqs = [head + [items[x] for x in p] for p in itertools.product(range(4), repeat=5)]
    assert len(seqs) == 1024 and all(len(s) == 64 for s in seqs)
    ptr, _, _ = assert_built(seqs, mode, cuda, n_items=100)
    assert np.diff(ptr).max() == (61 if filler == "distinct" else 4)


def step_sessions():
    """Sessions that cross the builder's 64-action step, at most 64 of their actions items."""
    rng = np.random.default_rng(64)

    def mix(n_actions, n_items_actions, vocab=40):
        s = [None] * n_actions
        for p in rng.choice(n_actions, n_items_actions, replace=False):
            s[p] = int(rng.integers(0, vocab))
        return s
    its = lambda m: [int(x) for x in rng.integers(0, 40, m)]
    return [mix(129, 64), mix(64, 64), mix(64, 40), mix(65, 64), mix(65, 30), mix(127, 64), mix(128, 64, 500), mix(129, 1), mix(192, 64),
            mix(192, 63, 500), [None] * 64 + its(64), [None] * 64 + its(3), its(32) + [None] * 64 + its(32), [None] * 128,
            its(1) + [None] * 127, [None] * 127 + its(1), [None] * 63 + its(2) + [None] * 63, list(range(64, 0, -1)) + [None] * 64]


@pytest.mark.parametrize("mode", ["binary", "stan"])
@pytest.mark.parametrize("S", [1, 3, 4, 5, 257])
def test_builder_across_the_64_action_step(cuda, mode, S):
    base = step_sessions()
    assert {len(s) for s in base} >= {64, 65, 127, 128, 129, 192} and max(sum(a is not None for a in s) for s in base) == 64
    seqs = [base[i % len(base)] for i in range(S)]
    ptr, _, _ = assert_built(seqs, mode, cuda, n_items=500)
    assert len(ptr) == S + 1 and ptr[1] > 0


@pytest.mark.parametrize("lammy", [0.1, 1.04, 1e6])
def test_builder_stan_decay_extremes(cuda, lammy):
    """64-item-action sessions under a steep, the usual and a flat decay.  lammy = 0.1: exp(-640) .. exp(-10), most
    weights are float32 denormals or zero; lammy = 1e6: every occurrence weighs the same to 6e-5."""
    rng = np.random.default_rng(10)
    seqs = [list(range(64)), list(range(63, -1, -1)), [5] * 64, [1, 2] * 32] + [[int(x) for x in rng.integers(0, v, 64)] for v in (3, 10, 30, 100, 400) for _ in range(8)]
    _, _, w = assert_built(seqs, "stan", cuda, lammy=lammy, n_items=400)
    if lammy == 0.1:
        tiny = np.abs(w) < np.finfo(np.float32).tiny
        assert (w == 0).any() and (tiny & (w != 0)).any()


# ------------------------------------------------------------------------ D. the builder's flags at the C ABI
N_ITEMS = 50


def flagged_batch(shift, long_bad, id_bad):
    """40 + shift sessions over 50 items; `shift` moves the bad ones through the four wave positions of a block.
    Returns (sessions, the same with every bad one emptied, the bad ones' indices).  The neighbours of the over-long
    sessions have 64 item actions: their LDS slots are full, and the next wave's begins where this one's ends."""
    rng = np.random.default_rng(400 + shift)
    its = lambda m: [int(x) for x in rng.integers(0, N_ITEMS, m)]
    seqs = [[None if rng.random() < 0.25 else int(rng.integers(0, N_ITEMS)) for _ in range(rng.integers(0, 13))] for _ in range(40 + shift)]
    bad = {}
    seqs[4 + shift], seqs[7 + shift] = its(64), list(rng.permutation(N_ITEMS)) + its(14)
    if long_bad:
        bad[5 + shift] = its(65)
        bad[6 + shift] = its(30) + [None] * 50 + its(170)             # 200 item actions over four steps
    if id_bad:
        bad[17 + shift] = [3, N_ITEMS, 4]
        bad[18 + shift] = [1, -1, 2]
        bad[19 + shift] = [7, 2 ** 32 + 7, 9]                        # 7 once narrowed to 32 bits
    clean = list(seqs)
    for i, s in bad.items():
        seqs[i], clean[i] = s, []
    return seqs, clean, sorted(bad)


@pytest.mark.parametrize("shift", [0, 1, 2, 3])
@pytest.mark.parametrize("flags", [1, 2, 3])
def test_builder_flags_at_the_abi(cuda, flags, shift):
    """err is 1 (more than 64 item actions), 2 (an id outside [0, n_items)) or 3; the count zeroes it, the fill ORs
    into it; a flagged session is an empty row, and every other session is what it is without the flagged ones."""
    seqs, clean, bad = flagged_batch(shift, bool(flags & 1), bool(flags & 2))
    a, S = table(seqs), len(seqs)
    sp, isr, item = _action_bufs(a)
    counts, err = Buf(S, torch.int32), Buf(1, torch.int32)
    run_twice(lambda: L().sss_session_vectors_count(sp.ptr, isr.ptr, item.ptr, S, N_ITEMS, counts.ptr, err.ptr, _st()), [counts, err])
    got = counts.t.cpu().numpy()
    assert int(err.t[0]) == flags and (got[bad] == 0).all()
    for mode in ("binary", "stan"):
        rp, ri, rw = ref.vectors(table(clean), mode, 1.04)
        assert np.array_equal(got, np.diff(rp)) and np.array_equal(np.r_[0, np.cumsum(got)], rp)
        ptr = dev_buf(rp)
        items, weights = Buf(len(ri), torch.int32), Buf(len(ri), torch.float32)
        run_twice(lambda: L().sss_session_vectors_fill(sp.ptr, isr.ptr, item.ptr, S, N_ITEMS, int(mode == "stan"), 1.04, ptr.ptr, items.ptr,
                                                       weights.ptr, err.ptr, _st()), [items, weights], prep=lambda: err.t.fill_(4))
        assert int(err.t[0]) == 4 | flags and err.guards_ok() and ptr.guards_ok()
        assert np.array_equal(items.t.cpu().numpy(), ri) and ulp_diff(weights.t.cpu().numpy(), rw).max() <= (mode == "stan")
    for b in (sp, isr, item, counts):
        assert b.guards_ok()


def test_builder_decreasing_sess_ptr_at_the_abi(cuda):
    """sess_ptr[4] < sess_ptr[3]: session 3 is flagged (err 1) and empty; session 4 reads the actions its own pointers
    name; every other session is untouched."""
    rng = np.random.default_rng(9)
    sess_ptr = np.array([0, 5, 9, 20, 12, 30, 30, 41], np.int64)
    S, T = len(sess_ptr) - 1, 41
    is_search = rng.random(T) < 0.2
    item_id = np.where(is_search, 0, rng.integers(0, N_ITEMS, T)).astype(np.int64)
    a = types.SimpleNamespace(num_sessions=S, sess_ptr=sess_ptr, is_search=is_search, item_id=item_id)
    sp, isr, item = _action_bufs(a)
    counts, err = Buf(S, torch.int32), Buf(1, torch.int32)
    run_twice(lambda: L().sss_session_vectors_count(sp.ptr, isr.ptr, item.ptr, S, N_ITEMS, counts.ptr, err.ptr, _st()), [counts, err])
    rp, ri, rw = ref.vectors(a, "binary")                            # the oracle's range(20, 12) is empty, too
    got = counts.t.cpu().numpy()
    assert int(err.t[0]) == 1 and got[3] == 0 and got[4] > 0 and np.array_equal(got, np.diff(rp))
    ptr = dev_buf(rp)
    items, weights = Buf(len(ri), torch.int32), Buf(len(ri), torch.float32)
    run_twice(lambda: L().sss_session_vectors_fill(sp.ptr, isr.ptr, item.ptr, S, N_ITEMS, 0, 0.0, ptr.ptr, items.ptr, weights.ptr, err.ptr,
                                                   _st()), [items, weights], prep=lambda: err.t.zero_())
    assert int(err.t[0]) == 1 and np.array_equal(items.t.cpu().numpy(), ri) and np.array_equal(weights.t.cpu().numpy(), rw)
    for b in (sp, isr, item, counts, err, ptr):
        assert b.guards_ok()
