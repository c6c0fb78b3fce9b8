"""The sparse session index (SKNN / STAN item-vector baselines) on the device: the vector builder and the search against
the numpy oracle of tests/helpers/sparse_ref.py -- bit for bit, D and I, on the weights read back from the index --
the reference's own results (tests/golden/sparse_baselines.npz) at the tolerances derived in
tests/test_sparse_index_cpu.py, in-process shards through sss_topk_merge, and the buffer / stream contract of every
computing entry point of include/sss_sparse.h in the manner of tests/test_abi_contract_gpu.py."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import sparse_ref as ref  # noqa: E402

from sessionsimilaritysearch_amd import _lib, sparse  # noqa: E402
from sessionsimilaritysearch_amd.distributed import shard_range  # noqa: E402
from sessionsimilaritysearch_amd.sessions import ActionTable, synthetic_actions  # noqa: E402
from test_abi_contract_gpu import OFF, Buf, _on_side_stream, _st, dev_buf, run_twice  # noqa: E402
from test_sparse_index_cpu import check_against_reference, golden  # noqa: E402

pytestmark = pytest.mark.gpu

# Computing entry point of include/sss_sparse.h -> the test that makes guarded calls of it (read with ast by
# tests/test_sparse_index_cpu.py).
COVERAGE = {
    "sss_session_vectors_count": "test_contract_session_vectors",
    "sss_session_vectors_fill": "test_contract_session_vectors",
    "sss_sparse_topk": "test_contract_sparse_topk",
}

LAMMY = 1.04
_CACHE = {}


def L():
    return _lib.lib()


def table(seqs):
    """ActionTable of sessions given as lists of item ids (None = a search)."""
    ptr = np.cumsum([0] + [len(s) for s in seqs]).astype(np.int64)
    flat = [a for s in seqs for a in s]
    return ActionTable(ptr, np.array([a is None for a in flat], bool), np.array([0 if a is None else a for a in flat], np.int64),
                       np.zeros(len(flat), np.int64))


def built(n, seed, mode, cuda, n_items=None):
    key = (n, seed, mode, n_items)
    if key not in _CACHE:
        a = synthetic_actions(n, seed) if n_items is None else synthetic_actions(n, seed, n_items, 9)
        v = sparse.session_vectors(a, mode, LAMMY if mode == "stan" else None, cuda)
        _CACHE[key] = (a, v, v.to_numpy())
    return _CACHE[key]


def ulp_diff(a, b):
    return np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64))


# ------------------------------------------------------------------------------------------------ the builder
@pytest.mark.parametrize("mode", ["binary", "stan"])
def test_builder_matches_the_oracle(cuda, mode):
    rng = np.random.default_rng(7)
    a = synthetic_actions(3000, 11, 500, 9)
    extra = [[None, None], [], [0, 0, None, 0], list(range(64)), list(range(63, -1, -1)), [5] * 64,
             [None] * 40 + list(rng.integers(0, 30, 64)) + [None] * 30,       # 134 actions, 64 of them items
             list(rng.integers(0, 499, 33)), [499, None, 499, 0]]
    b = table(extra)
    a = ActionTable(np.r_[a.sess_ptr, a.sess_ptr[-1] + b.sess_ptr[1:]], np.r_[a.is_search, b.is_search], np.r_[a.item_id, b.item_id],
                    np.r_[a.query_tok, b.query_tok])
    v = sparse.session_vectors(a, mode, LAMMY if mode == "stan" else None, cuda, n_items=500)
    ptr, items, w = v.to_numpy()
    rp, ri, rw = ref.vectors(a, mode, LAMMY)
    assert np.array_equal(ptr, rp) and np.array_equal(items, ri) and items.dtype == np.int32 and w.dtype == np.float32
    assert (np.diff(ptr) == 0).any() and (np.diff(ptr) == 64).any()
    if mode == "binary":
        assert np.array_equal(w, rw)
    else:
        assert ulp_diff(w, rw).max() <= 1, ulp_diff(w, rw).max()


def test_builder_flags_bad_sessions(cuda):
    with pytest.raises(_lib.SssError, match="more than 64"):
        sparse.session_vectors(table([[1, 2], list(range(65))]), "binary", device=cuda)
    with pytest.raises(_lib.SssError, match="outside"):
        sparse.session_vectors(table([[1, 2], [3, 100]]), "binary", device=cuda, n_items=100)
    with pytest.raises(_lib.SssError, match="outside"):
        sparse.session_vectors(table([[1, -2]]), "binary", device=cuda)


# ------------------------------------------------------------------------------------------------ search
def check_search(index, q, k, cuda, off=0):
    """Both runs of index.search(q, k) equal, bit for bit, the oracle on the weights read back; returns (D, I)."""
    index.id_offset = off
    D, I = index.search(q, k)
    D2, I2 = (t.clone() for t in index.search(q, k))
    assert torch.equal(D, D2) and torch.equal(I, I2), "two runs differ"
    key = ("scores", id(index), id(q))
    if key not in _CACHE:
        _CACHE[key] = (ref.scores(q.to_numpy(), index.vectors.to_numpy(), index.n_items), index, q)
    Dr, Ir = ref.topk(_CACHE[key][0], k, off)
    assert np.array_equal(I.cpu().numpy(), Ir) and np.array_equal(D.cpu().numpy(), Dr)
    return Dr, Ir


@pytest.mark.parametrize("mode", ["binary", "stan"])
def test_search_20k_sessions(cuda, mode):
    _, c, _ = built(20000, 1, "binary", cuda)
    _, q, qn = built(300, 2, mode, cuda)
    key = ("index20k",)
    if key not in _CACHE:
        _CACHE[key] = sparse.SparseSessionIndex(391572, cuda).add(c)
    index = _CACHE[key]
    assert index.ntotal == 20000
    for k in (1, 10, 100, 1000):
        Dr, _ = check_search(index, q, k, cuda)
    assert (Dr[:, 99] == Dr[:, 100]).mean() > 0.5                    # ties across any rank are the rule
    check_search(index, q, 10, cuda, off=OFF)
    assert index.last_chunks == 1


def test_search_duplicates_padding_and_chunks(cuda):
    rng = np.random.default_rng(3)
    base = [[1, 2, 3], [2, 3], [1, 2, 3, 4], [7], [], [None], [3, 2, 1, 1]]
    c = sparse.session_vectors(table([base[i] for i in rng.integers(0, len(base), 9000)]), "binary", device=cuda)
    q = sparse.session_vectors(table([[1, 2, 3], [2], [9], [], [3, 3, 1], [4, 1, 2, 3]]), "stan", 0.7, cuda)
    index = sparse.SparseSessionIndex(10, cuda).add(c)
    assert (np.diff(c.ptr.cpu().numpy()) == 0).sum() > 1000 and (np.diff(q.ptr.cpu().numpy()) == 0).any()     # empty rows, an empty query
    for k in (1, 100, 1000):                                          # thousands of identical rows straddle every k
        check_search(index, q, k, cuda)
    small = sparse.SparseSessionIndex(10, cuda).add(sparse.session_vectors(table(base), "binary", device=cuda))
    Dr, Ir = check_search(small, q, 20, cuda, off=5)                 # n = 7 < k = 20
    assert (Ir[:, 7:] == -1).all() and (Dr[:, 7:] == -ref.FLT_MAX).all() and Ir[:, :7].min() >= 5
    empty = sparse.SparseSessionIndex(10, cuda)
    D, I = empty.search(q, 3)
    assert (I == -1).all() and (D == -ref.FLT_MAX).all()
    # add() in two pieces == add() at once
    two = sparse.SparseSessionIndex(10, cuda).add(sparse.session_vectors(table(base[:3]), "binary", device=cuda))
    two.add(sparse.session_vectors(table(base[3:]), "binary", device=cuda))
    assert all(np.array_equal(x, y) for x, y in zip(two.vectors.to_numpy(), small.vectors.to_numpy()))
    # user-built batches: an all-empty one without any allocation behind it is valid; an unsorted row is refused
    none = sparse.SessionVectors(torch.zeros(3, dtype=torch.int64, device=cuda), torch.zeros(0, dtype=torch.int32, device=cuda),
                                 torch.zeros(0, dtype=torch.float32, device=cuda))
    D, I = small.search(none, 3)
    assert I.tolist() == [[5, 6, 7]] * 2 and (D == 0).all()
    hollow = sparse.SparseSessionIndex(10, cuda).add(none)
    D, I = hollow.search(q, 3)
    assert hollow.ntotal == 2 and I[0].tolist() == [0, 1, -1] and D[0].tolist()[:2] == [0, 0]
    unsorted = sparse.SessionVectors(torch.tensor([0, 2], device=cuda), torch.tensor([3, 1], dtype=torch.int32, device=cuda),
                                     torch.ones(2, device=cuda))
    for use in (small.search, sparse.SparseSessionIndex(10, cuda).add):
        with pytest.raises(ValueError, match="ascending"):
            use(unsorted, 3) if use == small.search else use(unsorted)
    # dense numpy queries and the drop-in
    dense = np.zeros((2, 10), np.float32)
    dense[0, [1, 2]] = np.float32(1 / np.sqrt(2)); dense[1, 7] = 1
    Dn, In = small.search(dense, 3)
    assert isinstance(Dn, np.ndarray) and In[1, 0] == 3 + 5 and Dn[1, 0] == 1
    from scipy.sparse import csr_matrix
    p, it, w = small.vectors.to_numpy()
    Df, If = sparse.find_K_sparse_dense(csr_matrix((w, it, p), shape=(7, 10)), dense, 3)
    assert Df.dtype == np.float64 and If.dtype == np.int32 and np.array_equal(If + 5, In) and np.array_equal(Df.astype(np.float32), Dn)


def test_search_one_million_sessions(cuda):
    """64 queries in one chunk; 300 queries: more than the 1 GB score budget holds at once (268 rows of 4 MB)."""
    _, c, _ = built(1000000, 4, "binary", cuda)
    index = sparse.SparseSessionIndex(391572, cuda).add(c)
    _, q300, _ = built(300, 5, "stan", cuda)
    check_search(index, q300, 100, cuda)
    assert index.last_chunks == 2
    q64 = sparse.SparseSessionIndex(391572, cuda).add(q300).vectors     # (a copy)
    q64 = sparse.SessionVectors(q64.ptr[:65].contiguous(), q64.items, q64.weights)
    index.id_offset = 0
    D, I = index.search(q64, 100)
    D3, I3 = index.search(q300, 100)
    assert index.last_chunks == 2 and torch.equal(D, D3[:64]) and torch.equal(I, I3[:64])


@pytest.mark.parametrize("mode", ["SKNN", "STAN"])
def test_golden_reference_results(cuda, mode):
    g, tab = golden()
    n_items, K = int(g["n_items"]), int(g["K"])
    c = sparse.session_vectors(tab["corpus"], "binary", device=cuda, n_items=n_items)
    q = sparse.session_vectors(tab["query"], "stan" if mode == "STAN" else "binary", float(g["lammy"]), cuda, n_items)
    index = sparse.SparseSessionIndex(n_items, cuda).add(c)
    D, I = index.search(q, K)
    check_against_reference(g, mode, q.to_numpy(), c.to_numpy(), D.cpu().numpy(), I.cpu().numpy())
    for ours, tag in ((c, "ref_corpus"), (q, f"ref_query_{mode}")):
        p, it, w = ours.to_numpy()
        assert np.array_equal(p, g[f"{tag}_ptr"]) and np.array_equal(it, g[f"{tag}_items"])
        assert np.all(np.abs(w.astype(np.float64) - g[f"{tag}_weights"]) <= 1e-6 * np.abs(w))


@pytest.mark.parametrize("shards", [1, 2, 4])
def test_in_process_shards_merge_to_the_single_index(cuda, shards):
    _, c, cn = built(20000, 1, "binary", cuda)
    _, q, _ = built(300, 2, "stan", cuda)
    nq, k, n = 300, 50, 20000
    whole = sparse.SparseSessionIndex(391572, cuda).add(c)
    Dw, Iw = whole.search(q, k)
    Ds = torch.empty((shards, nq, k), dtype=torch.float32, device=cuda)
    Is = torch.empty((shards, nq, k), dtype=torch.int64, device=cuda)
    for r in range(shards):
        lo, hi = shard_range(n, shards, r)
        part = sparse.SessionVectors(c.ptr[lo:hi + 1].contiguous(), c.items, c.weights)
        idx = sparse.SparseSessionIndex(391572, cuda).add(part)
        idx.id_offset = lo
        assert idx.ntotal == hi - lo
        idx.search_device(q, k, Ds[r], Is[r])
    Do, Io = torch.empty_like(Dw), torch.empty_like(Iw)
    rc = L().sss_topk_merge(Ds.data_ptr(), nq * k, Is.data_ptr(), nq * k, shards, nq, k, Do.data_ptr(), Io.data_ptr(), _st())
    assert rc == 0
    assert torch.equal(Do, Dw) and torch.equal(Io, Iw)


# ------------------------------------------------------------------------------------------------ the ABI contract
def _action_bufs(a):
    return (dev_buf(a.sess_ptr.astype(np.int64)), dev_buf(a.is_search.astype(np.uint8)), dev_buf(a.item_id.astype(np.int64)))


def test_contract_session_vectors(cuda):
    """Guarded, exactly sized buffers; two poisons; inputs unmodified; then the same calls on a side stream."""
    a = synthetic_actions(301, 63, 300, 33)
    Sn = 301
    sp, isr, item = _action_bufs(a)
    before = [b.t.clone() for b in (sp, isr, item)]
    counts, err = Buf(Sn, torch.int32), Buf(1, torch.int32)
    run_twice(lambda: L().sss_session_vectors_count(sp.ptr, isr.ptr, item.ptr, Sn, 300, counts.ptr, err.ptr, _st()), [counts, err])
    for mode in ("binary", "stan"):
        rp, ri, rw = ref.vectors(a, mode, LAMMY)
        assert np.array_equal(counts.t.cpu().numpy(), np.diff(rp)) and int(err.t[0]) == 0
        ptr = dev_buf(rp)
        items, weights = Buf(len(ri), torch.int32), Buf(len(ri), torch.float32)
        err.t.zero_()
        run_twice(lambda: L().sss_session_vectors_fill(sp.ptr, isr.ptr, item.ptr, Sn, 300, int(mode == "stan"), LAMMY, ptr.ptr, items.ptr,
                                                       weights.ptr, err.ptr, _st()), [items, weights])
        assert np.array_equal(items.t.cpu().numpy(), ri) and ulp_diff(weights.t.cpu().numpy(), rw).max() <= (mode == "stan")
        assert int(err.t[0]) == 0 and ptr.guards_ok() and torch.equal(ptr.t, torch.from_numpy(rp).cuda())
    for b, was in zip((sp, isr, item), before):
        assert b.guards_ok() and torch.equal(b.t, was), "an input was modified"
    # stream: the item ids are overwritten on the side stream ahead of the calls that read them
    new_item = item.t.clone()
    item.t.zero_()
    got = _on_side_stream(lambda: item.t.copy_(new_item),
                          lambda s: L().sss_session_vectors_count(sp.ptr, isr.ptr, item.ptr, Sn, 300, counts.ptr, err.ptr, _st(s)),
                          lambda: counts.t.clone())
    rp, ri, rw = ref.vectors(a, "binary")
    assert np.array_equal(got.cpu().numpy(), np.diff(rp))
    item.t.zero_()
    got = _on_side_stream(lambda: item.t.copy_(new_item),
                          lambda s: L().sss_session_vectors_fill(sp.ptr, isr.ptr, item.ptr, Sn, 300, 0, 0.0, ptr.ptr, items.ptr, weights.ptr,
                                                                 err.ptr, _st(s)), lambda: (items.t.clone(), weights.t.clone()))
    assert np.array_equal(got[0].cpu().numpy(), ri) and np.array_equal(got[1].cpu().numpy(), rw)


@pytest.mark.parametrize("n,k", [(5003, 33), (300001, 100), (40, 64)])
def test_contract_sparse_topk(cuda, n, k):
    """n = 300001 takes the compaction tail; n = 40 < k pads.  The corpus triple is the head of a larger one whose
    further rows would win if they were read."""
    nq = 37
    cn = ref.vectors(synthetic_actions(n + 64, 70 + k, 2000, 9), "binary")
    qn = ref.vectors(synthetic_actions(nq, 71, 2000, 9), "stan", LAMMY)
    cn[1][cn[0][n]:] = qn[1][0] if qn[0][1] else 0                    # tail rows hold query 0's first item with a huge weight
    cn[2][cn[0][n]:] = 1e6
    cb, qb = [dev_buf(x) for x in cn], [dev_buf(x) for x in qn]
    before = [b.t.clone() for b in (*cb, *qb)]
    D, I = Buf((nq, k), torch.float32), Buf((nq, k), torch.int64)
    ws = Buf(int(L().sss_sparse_topk_workspace_bytes(nq, n)), torch.uint8)
    call = lambda s=None: L().sss_sparse_topk(qb[0].ptr, qb[1].ptr, qb[2].ptr, nq, cb[0].ptr, cb[1].ptr, cb[2].ptr, n, k, OFF, D.ptr, I.ptr,
                                              ws.ptr, ws.nbytes, _st(s))
    run_twice(call, [D, I], [ws])
    head = (cn[0][:n + 1], cn[1][:cn[0][n]], cn[2][:cn[0][n]])
    Dr, Ir = ref.search(qn, head, 2000, k, OFF)
    assert np.array_equal(I.t.cpu().numpy(), Ir) and np.array_equal(D.t.cpu().numpy(), Dr)
    for b, was in zip((*cb, *qb), before):
        assert b.guards_ok() and torch.equal(b.t, was), "an input was modified"
    # stream: the query weights are overwritten on the side stream ahead of the search that reads them
    new_w = qb[2].t.clone()
    qb[2].t.zero_()
    got = _on_side_stream(lambda: qb[2].t.copy_(new_w), call, lambda: (D.t.clone(), I.t.clone()))
    assert np.array_equal(got[1].cpu().numpy(), Ir) and np.array_equal(got[0].cpu().numpy(), Dr)
