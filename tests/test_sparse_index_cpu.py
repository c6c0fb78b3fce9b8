"""CPU side of the sparse session index (SKNN / STAN item-vector baselines): the numpy oracle against what the
reference's own functions produced (tests/golden/sparse_baselines.npz), the C ABI of include/sss_sparse.h against its
ctypes binding, argument validation without a device, and ShardedSparseIndex on gloo with an oracle engine.

Tolerances (relative, from the number formats): the reference normalises its float64 vectors a second time in float32
-- one float32 rounding plus a float32 sum of at most 19 squares, <= 13 * 2^-24 < 1e-6 on a weight; a score is two such
weights (1e-6 each) and at most 19 positive terms summed in float32 (19 * 2^-24): 4e-6."""
import ast
import os
import socket
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
from abi import declared  # noqa: E402
import sparse_ref as ref  # noqa: E402

from sessionsimilaritysearch_amd import _lib  # noqa: E402
from sessionsimilaritysearch_amd.distributed import ShardedSparseIndex, shard_range  # noqa: E402
from sessionsimilaritysearch_amd.sessions import ActionTable, synthetic_actions  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "sparse_baselines.npz")
W_TOL, S_TOL = 1e-6, 4e-6


def golden():
    g = np.load(GOLDEN)
    tab = {t: ActionTable(g[f"{t}_sess_ptr"], g[f"{t}_is_search"], g[f"{t}_item_id"], np.zeros_like(g[f"{t}_item_id"]))
           for t in ("corpus", "query")}
    return g, tab


def _close(a, b, tol):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return bool(np.all(np.abs(a - b) <= tol * np.maximum(np.abs(a), np.abs(b))))


def check_against_reference(g, mode, q, c, D, I=None):
    """Our (D, I) -- or the oracle's when I is None -- against the reference's: the canonical score of every id the
    reference returned matches its D entry, and the sorted D rows agree (ids cannot be compared: mass ties)."""
    n_items = int(g["n_items"])
    s = ref.scores(q, c, n_items)
    Dr, Ir = g[f"D_{mode}"], g[f"I_{mode}"]
    assert _close(np.take_along_axis(s, Ir.astype(np.int64), axis=1), Dr, S_TOL)
    assert _close(np.sort(D, axis=1), np.sort(Dr, axis=1), S_TOL)
    if I is not None:
        assert np.array_equal(np.take_along_axis(s, I, axis=1), D)


@pytest.mark.parametrize("mode", ["SKNN", "STAN"])
def test_oracle_vectors_and_scores_match_the_reference(mode):
    g, tab = golden()
    c = ref.vectors(tab["corpus"], "binary")
    q = ref.vectors(tab["query"], "stan" if mode == "STAN" else "binary", float(g["lammy"]))
    for ours, tag in ((c, "ref_corpus"), (q, f"ref_query_{mode}")):
        assert np.array_equal(ours[0], g[f"{tag}_ptr"]) and np.array_equal(ours[1], g[f"{tag}_items"])
        assert _close(ours[2], g[f"{tag}_weights"], W_TOL)
    assert (np.diff(c[0]) == 0).any() and (np.diff(q[0]) == 0).any() and (c[1] == 0).any()     # empty rows, item 0
    D, I = ref.search(q, c, int(g["n_items"]), int(g["K"]))
    check_against_reference(g, mode, q, c, D)
    assert (D[:, -1] == D[:, -2]).sum() > 20                       # ties at the boundary are the rule


def test_oracle_binary_weights_and_order():
    a = synthetic_actions(50, 3, 40, 9)
    ptr, items, w = ref.vectors(a, "binary")
    for s in range(50):
        m = ptr[s + 1] - ptr[s]
        clicks = a.item_id[a.sess_ptr[s]:a.sess_ptr[s + 1]][~a.is_search[a.sess_ptr[s]:a.sess_ptr[s + 1]]]
        assert np.array_equal(items[ptr[s]:ptr[s + 1]], np.unique(clicks))
        assert (w[ptr[s]:ptr[s + 1]] == np.float32(1 / np.sqrt(np.float64(m)))).all()
    s = np.array([[1, 3, 3, 0, 3]], np.float32)
    D, I = ref.topk(s, 3, id_offset=10)
    assert I.tolist() == [[11, 12, 14]] and D.tolist() == [[3, 3, 3]]
    D, I = ref.topk(s, 7)
    assert I.tolist() == [[1, 2, 4, 0, 3, -1, -1]] and D[0, 5] == ref.FLT_MAX * -1


# ------------------------------------------------------------------------------------------------ the C ABI
def test_sparse_header_and_binding_declare_the_same_entry_points():
    names = declared("sss_sparse.h")
    assert names == _lib.symbols("sss_sparse.h") and len(names) >= 4
    L = _lib.lib()
    for n in names:
        assert getattr(L, n).argtypes == _lib.HEADERS["sss_sparse.h"][n][1]
    assert declared("sss.h") == _lib.exported_symbols()
    assert not set(names) & set(_lib.exported_symbols())
    text = open(os.path.join(ROOT, "include", "sss_sparse.h")).read()
    assert "CALLER-OWNED DEVICE" in text and "-2 workspace too small" in text


def test_every_sparse_entry_point_has_a_guarded_gpu_test():
    tree = ast.parse(open(os.path.join(ROOT, "tests", "test_sparse_index_gpu.py")).read())
    table = next(ast.literal_eval(n.value) for n in tree.body
                 if isinstance(n, ast.Assign) and any(getattr(t, "id", None) == "COVERAGE" for t in n.targets))
    tests = {n.name for n in tree.body if isinstance(n, ast.FunctionDef)}
    computing = [n for n in declared("sss_sparse.h") if not n.endswith("_bytes")]
    assert sorted(table) == computing and all(t in tests for t in table.values())


_P = 1 << 20                                                          # a non-null, 256-byte aligned address; never dereferenced


def _topk(L, **kw):
    a = dict(qp=_P, qi=_P, qw=_P, nq=4, cp=_P, ci=_P, cw=_P, n=1000, k=10, off=0, D=_P, I=_P, ws=_P, wsb=0)
    a.update(kw)
    return L.sss_sparse_topk(a["qp"], a["qi"], a["qw"], a["nq"], a["cp"], a["ci"], a["cw"], a["n"], a["k"], a["off"], a["D"], a["I"],
                             a["ws"], a["wsb"], 0)


def test_sparse_topk_validates_before_any_launch():
    """Every bad argument is -1 with a workspace that is too small as well: a call that skipped the check would return -2
    (and one that skipped both would launch on addresses that are not memory)."""
    L = _lib.lib()
    assert _topk(L) == -2 and b"workspace" in L.sss_last_error()                          # valid but for the workspace
    need = L.sss_sparse_topk_workspace_bytes(4, 1000)
    assert need >= 4 * 1000 * 4 and _topk(L, wsb=need - 1) == -2
    for bad in (dict(k=0), dict(k=1025), dict(k=-3), dict(nq=0), dict(nq=65536), dict(n=0), dict(n=1 << 31)):
        assert _topk(L, **bad) == -1, (bad, L.sss_last_error())
    for name in ("qp", "qi", "qw", "cp", "ci", "cw", "D", "I", "ws"):
        assert _topk(L, **{name: 0}) == -1 and b"null" in L.sss_last_error(), name
    assert _topk(L, ws=_P + 8) == -1 and b"aligned" in L.sss_last_error()
    assert L.sss_sparse_topk_workspace_bytes(0, 10) == 0 and L.sss_sparse_topk_workspace_bytes(10, 0) == 0


def test_session_vectors_validate_before_any_launch():
    L = _lib.lib()
    cnt = lambda **kw: L.sss_session_vectors_count(*[{**dict(sp=_P, isr=_P, it=_P, S=5, V=100, c=_P, e=_P), **kw}[x]
                                                     for x in ("sp", "isr", "it", "S", "V", "c", "e")], 0)
    for bad in (dict(sp=0), dict(isr=0), dict(it=0), dict(c=0), dict(e=0), dict(S=0), dict(S=1 << 31), dict(V=0), dict(V=1 << 31)):
        assert cnt(**bad) == -1, bad
    fill = lambda **kw: L.sss_session_vectors_fill(*[{**dict(sp=_P, isr=_P, it=_P, S=5, V=100, mode=1, lam=1.0, p=_P, i=_P, w=_P, e=_P), **kw}[x]
                                                     for x in ("sp", "isr", "it", "S", "V", "mode", "lam", "p", "i", "w", "e")], 0)
    for bad in (dict(mode=2), dict(mode=-1), dict(lam=0.0), dict(lam=-1.0), dict(lam=float("nan")), dict(lam=float("inf")),
                dict(p=0), dict(i=0), dict(w=0), dict(e=0), dict(sp=0), dict(S=-1)):
        assert fill(**bad) == -1, bad
    assert b"session_vectors_fill" in L.sss_last_error()


def test_python_surface_rejects_bad_modes_without_a_device():
    from sessionsimilaritysearch_amd import sparse
    a = synthetic_actions(4, 1, 50, 9)
    with pytest.raises(ValueError):
        sparse.session_vectors(a, "tfidf")
    with pytest.raises(ValueError):
        sparse.session_vectors(a, "stan")                             # lammy has no default
    import sessionsimilaritysearch_amd as pkg
    assert pkg.SparseSessionIndex is sparse.SparseSessionIndex and pkg.find_K_sparse_dense is sparse.find_K_sparse_dense


def test_session_vectors_check_rejects_malformed_batches():
    """SessionVectors.check on host tensors (the reductions are device-agnostic): rows must ascend strictly, ptr must be
    non-decreasing inside items; empty rows -- leading, inner, trailing -- and slices of a larger batch are fine."""
    from sessionsimilaritysearch_amd.sparse import SessionVectors

    def mk(ptr, items):
        return SessionVectors(torch.tensor(ptr), torch.tensor(items, dtype=torch.int32), torch.zeros(len(items)))
    for good in (([0, 2, 2, 5], [1, 3, 0, 2, 9]), ([0], []), ([0, 0, 0], []), ([0, 1], [4]), ([2, 4], [9, 9, 1, 3, 0]), ([0, 0, 2, 2], [5, 6])):
        assert mk(*good).check(10) is not None
    for bad in (([0, 2, 5], [1, 1, 0, 2, 9]), ([0, 3, 5], [1, 3, 0, 2, 9]), ([0, 2, 1], [1, 3]), ([0, 2], [1, 10]), ([0, 2], [-1, 3]),
                ([0, 6], [1, 2, 3]), ([0, 3, 3], [1, 3, 2]), ([0, 0, 3], [1, 3, 2])):
        with pytest.raises(ValueError):
            mk(*bad).check(10)
    # strided views: the C ABI reads through bare pointers, so each of the three must be contiguous
    ptr, items, w = torch.tensor([0, 9, 1, 9, 2]), torch.tensor([3, 0, 5, 0], dtype=torch.int32), torch.zeros(4)
    assert SessionVectors(ptr[::2].contiguous(), items[::2].contiguous(), w[::2].contiguous()).check(10) is not None
    for strided in (SessionVectors(ptr[::2], items[:2], w[:2]), SessionVectors(ptr[::2].contiguous(), items[::2], w[:2]),
                    SessionVectors(ptr[::2].contiguous(), items[:2], w[::2])):
        with pytest.raises(ValueError, match="contiguous"):
            strided.check(10)
        with pytest.raises(ValueError, match="contiguous"):
            strided.require_contiguous()


# ------------------------------------------------------------------------------------------------ sharding (gloo)
class OracleEngine:
    def __init__(self, shard, n_items, id_offset):
        self.shard, self.n_items, self.off = shard, n_items, id_offset

    def local_search(self, q, k, D, I):
        d, i = ref.search(q.triple, self.shard, self.n_items, k, self.off)
        D.copy_(torch.from_numpy(d)); I.copy_(torch.from_numpy(i))

    @staticmethod
    def merge(pack_all, chunk, shards, nq, k, D_out, I_out):
        """sss_topk_merge's contract: (score desc, id asc), ids < 0 are padding."""
        nk = nq * k
        d = np.concatenate([pack_all[s * chunk + nk:(s + 1) * chunk].view(torch.float32)[:nk].view(nq, k).numpy() for s in range(shards)], 1)
        i = np.concatenate([pack_all[s * chunk:s * chunk + nk].view(nq, k).numpy() for s in range(shards)], 1)
        for f in range(nq):
            ok = np.flatnonzero(i[f] >= 0)
            o = ok[np.lexsort((i[f, ok], -d[f, ok].astype(np.float64)))][:k]
            D_out[f] = -3.4028234663852886e38; I_out[f] = -1
            D_out[f, :len(o)] = torch.from_numpy(d[f, o]); I_out[f, :len(o)] = torch.from_numpy(i[f, o])


class Triple:
    def __init__(self, triple):
        self.triple = triple

    def __len__(self):
        return len(self.triple[0]) - 1


def _rows(c, lo, hi):
    return c[0][lo:hi + 1] - c[0][lo], c[1][c[0][lo]:c[0][hi]], c[2][c[0][lo]:c[0][hi]]


def _worker(rank, world, port, out_dir, n, k, force):
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        c = ref.vectors(synthetic_actions(n, 5, 60, 9), "binary")
        q = ref.vectors(synthetic_actions(11, 6, 60, 9), "stan", 1.5)
        Dr, Ir = ref.search(q, c, 60, k)
        lo, hi = shard_range(n, world, rank)
        idx = ShardedSparseIndex(OracleEngine(_rows(c, lo, hi), 60, lo), torch.device("cpu"), force_collectives=force)
        D, I = idx.search(Triple(q), k)
        good = idx.exchange and np.array_equal(D.numpy(), Dr) and np.array_equal(I.numpy(), Ir) and (Dr[:, 0] > 0).any()
        if k > n:
            good = good and bool((Ir[:, n:] == -1).all())
        open(os.path.join(out_dir, f"rank{rank}.txt"), "w").write("ok" if good else "MISMATCH")
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("world,n,k,force", [(2, 403, 20, False), (2, 7, 10, False), (1, 100, 10, True)])
def test_sharded_sparse_index_equals_unsharded(tmp_path, world, n, k, force):
    """2 ranks over a corpus where every list is runs of ties; (2, 7, 10): fewer rows than k, padding crosses the merge."""
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    mp.spawn(_worker, args=(world, port, str(tmp_path), n, k, force), nprocs=world, join=True)
    for r in range(world):
        assert open(tmp_path / f"rank{r}.txt").read() == "ok"
