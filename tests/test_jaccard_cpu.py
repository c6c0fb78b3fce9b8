"""CPU side of the ground-truth index (include/sss_jaccard.h): the numpy helper against what the reference's own get_score
produced for every pair (tests/golden/jaccard_truth.npz), the float32 order of small fractions the contract relies on, the
header against its ctypes binding, argument validation of both entry points and of the Python layer without a device, and
ShardedJaccardIndex on gloo with an oracle engine."""
import ctypes
import os
import socket
import sys
from fractions import Fraction

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
from abi import declared  # noqa: E402
import jaccard_ref as jr  # noqa: E402

from sessionsimilaritysearch_amd import _lib  # noqa: E402
from sessionsimilaritysearch_amd.distributed import ShardedJaccardIndex, shard_range  # noqa: E402
from test_eval_metrics_cpu import golden, host_parts  # noqa: E402
from test_sparse_index_cpu import OracleEngine as SparseOracle  # noqa: E402
import sparse_ref  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TRUTH = os.path.join(ROOT, "tests", "golden", "jaccard_truth.npz")
SIM_PART = {"all_jaccard": "all", "cur_jaccard": "cur"}
_CACHE = {}


def truth():
    """(the reference's matrices, the host item sets of the query parts, those of the corpus), loaded once."""
    if "t" not in _CACHE:
        _, tab = golden()
        _CACHE["t"] = (np.load(TRUTH), host_parts(tab), sparse_ref.vectors(tab["corpus"], "binary")[:2])
    return _CACHE["t"]


def helper_ratios(sim):
    if sim not in _CACHE:
        _, parts, corpus = truth()
        _CACHE[sim] = jr.ratios(parts[SIM_PART[sim]], corpus)
    return _CACHE[sim]


@pytest.mark.parametrize("sim", ["all_jaccard", "cur_jaccard"])
def test_helper_reproduces_the_reference_bit_for_bit(sim):
    ref = truth()[0][f"ref_{sim}"]
    r = helper_ratios(sim)
    assert ref.shape == (48, 400) and ref.dtype == np.float64
    assert np.array_equal(ref.astype(np.float32), r.astype(np.float32)) and np.array_equal(ref, r)
    for edges in ((0.2, 0.8), (0.2, 0.5)):
        band = (ref[:, :, None] >= np.asarray(edges)[None, None, :]).sum(2)
        counts, first = jr.bands(r, edges)
        for b in range(3):
            assert np.array_equal(counts[:, b], (band == b).sum(1))
            assert np.array_equal(first[:, b], [np.flatnonzero(row == b)[0] if (row == b).any() else -1 for row in band])
        assert (counts.sum(1) == 400).all()


def test_fixture_holds_what_the_gpu_tests_rely_on():
    A, C = helper_ratios("all_jaccard"), helper_ratios("cur_jaccard")
    full = lambda r, e: int((jr.bands(r, e)[0] > 0).all(1).sum())
    assert (full(A, (0.2, 0.5)), full(C, (0.2, 0.5)), full(C, (0.2, 0.8))) == (14, 16, 2)
    assert A.max() < 0.8 and (jr.bands(A, (0.2, 0.8))[1][:, 2] == -1).all()       # the empty top band
    assert int(np.isin(A, (0.2, 0.5)).sum()) == 598 and int(np.isin(C, (0.2, 0.5)).sum()) == 786
    D, _ = jr.topk(A, 101)
    assert int((D[:, 19] == D[:, 20]).sum()) == 41 and int((D[:, 99] == D[:, 100]).sum()) == 46
    _, parts, corpus = truth()
    assert int((np.diff(corpus[0]) == 0).sum()) == 16 and int((np.diff(parts["cur"][0]) == 0).sum()) == 5
    ids, sc, keep = jr.mine(C)
    assert keep.sum() == 2 and jr.mine(A)[2].sum() == 0


def test_float32_keeps_the_order_of_fractions_up_to_128():
    """The contract's claim for sets of at most 64 items: all a / b with 0 <= a <= b <= 128 map to distinct float32 values
    exactly when they are distinct rationals, in the same order."""
    fr = sorted({Fraction(a, b) for b in range(1, 129) for a in range(b + 1)})
    f32 = np.array([np.float32(np.float64(f.numerator) / np.float64(f.denominator)) for f in fr])
    assert len(fr) > 5000 and (np.diff(f32.astype(np.float64)) > 0).all()
    for a, b in ((1, 3), (2, 6), (64, 128), (43, 128)):
        assert np.float32(np.float64(a) / np.float64(b)) == f32[fr.index(Fraction(a, b))]


# ------------------------------------------------------------------------------------------------ the C ABI
def test_jaccard_header_and_binding_declare_the_same_entry_points():
    names = declared("sss_jaccard.h")
    assert names == _lib.symbols("sss_jaccard.h") == ["sss_jaccard_bands", "sss_jaccard_topk", "sss_jaccard_topk_workspace_bytes"]
    L = _lib.lib()
    for n in names:
        assert getattr(L, n).argtypes == _lib.HEADERS["sss_jaccard.h"][n][1]
    for header, table in _lib.HEADERS.items():
        if header != "sss_jaccard.h":
            assert not set(names) & set(table) and not set(names) & set(declared(header)), header
    assert declared("sss.h") == _lib.exported_symbols()
    text = open(os.path.join(ROOT, "include", "sss_jaccard.h")).read()
    assert "CALLER-OWNED DEVICE" in text and "-2 workspace too small" in text and "HOST array" in text and "2^-14" in text


_P = 1 << 20                                                          # a non-null, 256-byte aligned address; never dereferenced


def _edges(*v):
    return (ctypes.c_double * len(v))(*v)


def _topk(L, **kw):
    a = dict(qp=_P, qi=_P, nq=4, cp=_P, ci=_P, n=1000, k=10, off=0, D=_P, I=_P, ws=_P, wsb=0)
    a.update(kw)
    return L.sss_jaccard_topk(a["qp"], a["qi"], a["nq"], a["cp"], a["ci"], a["n"], a["k"], a["off"], a["D"], a["I"], a["ws"], a["wsb"], 0)


def _bands(L, **kw):
    a = dict(qp=_P, qi=_P, nq=4, cp=_P, ci=_P, n=1000, e=_edges(0.2, 0.8), ne=2, off=0, c=_P, f=_P)
    a.update(kw)
    e = a["e"] if isinstance(a["e"], int) else ctypes.addressof(a["e"])
    return L.sss_jaccard_bands(a["qp"], a["qi"], a["nq"], a["cp"], a["ci"], a["n"], e, a["ne"], a["off"], a["c"], a["f"], 0)


def check_argument_errors(L):
    """Every bad argument of both entry points is -1 (-2 for the workspace) with a message.  No address given here is memory:
    a call that launched would fault, and a top-k that skipped a check would return -2 for its empty workspace."""
    assert _topk(L) == -2 and b"workspace" in L.sss_last_error()                          # valid but for the workspace
    need = L.sss_jaccard_topk_workspace_bytes(4, 1000)
    assert need >= 4 * 1000 * 4 and _topk(L, wsb=need - 1) == -2
    for bad in (dict(k=0), dict(k=1025), dict(k=-3), dict(nq=0), dict(nq=65536), dict(nq=-1), dict(n=0), dict(n=1 << 31)):
        assert _topk(L, **bad) == -1 and L.sss_last_error(), bad
    for name in ("qp", "qi", "cp", "ci", "D", "I", "ws"):
        assert _topk(L, **{name: 0}) == -1 and b"null" in L.sss_last_error(), name
    assert _topk(L, ws=_P + 8) == -1 and b"aligned" in L.sss_last_error()
    assert L.sss_jaccard_topk_workspace_bytes(0, 10) == 0 and L.sss_jaccard_topk_workspace_bytes(10, 0) == 0
    inf, nan = float("inf"), float("nan")
    for bad in (dict(nq=0), dict(nq=65536), dict(n=0), dict(n=1 << 31), dict(ne=0), dict(ne=8), dict(ne=-1), dict(off=-1),
                dict(off=2 ** 63 - 1000), dict(e=_edges(0.8, 0.2)), dict(e=_edges(0.2, 0.2)), dict(e=_edges(0.2, inf)),
                dict(e=_edges(-inf, 0.2)), dict(e=_edges(nan, 0.2)), dict(e=_edges(0.2, nan)),
                dict(e=_edges(.1, .2, .3, .4, .5, .6, .6), ne=7)):
        assert _bands(L, **bad) == -1 and b"jaccard_bands" in L.sss_last_error(), bad
    for name in ("qp", "qi", "cp", "ci", "e", "c", "f"):
        assert _bands(L, **{name: 0}) == -1 and b"null" in L.sss_last_error(), name


def test_both_entry_points_validate_before_any_launch():
    check_argument_errors(_lib.lib())


def test_python_layer_validates_edges_and_chunks_without_a_device():
    from sessionsimilaritysearch_amd import jaccard
    import sessionsimilaritysearch_amd as pkg
    assert pkg.JaccardIndex is jaccard.JaccardIndex and pkg.mine_triples is jaccard.mine_triples
    assert pkg.neighbourhood_recall is jaccard.neighbourhood_recall
    assert jaccard.check_edges(0.5).tolist() == [0.5] and jaccard.check_edges((0.2, 0.8)).dtype == np.float64
    for bad in ((), (0.8, 0.2), (0.2, 0.2), (0.2, float("nan")), (float("inf"),), tuple(range(8)), [[0.1, 0.2]]):
        with pytest.raises(ValueError):
            jaccard.check_edges(bad)
    assert jaccard.query_chunks(0, 10) == [] and jaccard.query_chunks(7, 3) == [(0, 3), (3, 3), (6, 1)]
    assert jaccard.query_chunks(70000, 10 ** 9) == [(0, 65535), (65535, 4465)] and jaccard.query_chunks(3, 0) == [(0, 1), (1, 1), (2, 1)]
    for bad in (0, -1, 2 ** 31):
        with pytest.raises(ValueError):
            jaccard.JaccardIndex(bad, torch.device("cpu"))


# ------------------------------------------------------------------------------------------------ sharding (gloo)
class HostSets:
    def __init__(self, pair):
        self.pair = pair

    def __len__(self):
        return len(self.pair[0]) - 1


def rows_of(c, lo, hi):
    return c[0][lo:hi + 1] - c[0][lo], c[1][c[0][lo]:c[0][hi]]


class OracleEngine:
    """A JaccardIndex shard restated on the helper: search and bands with global ids."""
    merge = staticmethod(SparseOracle.merge)

    def __init__(self, shard, id_offset):
        self.shard, self.off = shard, id_offset

    def local_search(self, q, k, D, I):
        d, i = jr.topk(jr.ratios(q.pair, self.shard), k, self.off)
        D.copy_(torch.from_numpy(d)); I.copy_(torch.from_numpy(i))

    def local_bands(self, q, edges):
        return tuple(torch.from_numpy(x) for x in jr.bands(jr.ratios(q.pair, self.shard), edges, self.off))


def shard_case(n):
    """The `all` queries against the first n - 1 golden corpus rows and, as the LAST row, query 0's own set: no other row
    reaches 0.8, so the top band of query 0 holds that one row, which lives on the last rank that has rows."""
    _, parts, corpus = truth()
    q = parts["all"]
    head = rows_of(corpus, 0, n - 1)
    own = q[1][q[0][0]:q[0][1]]
    return q, (np.r_[head[0], head[0][-1] + len(own)], np.r_[head[1], own])


def _worker(rank, world, port, out_dir, n, k, force):
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        q, c = shard_case(n)
        r = jr.ratios(q, c)
        lo, hi = shard_range(n, world, rank)
        idx = ShardedJaccardIndex(OracleEngine(rows_of(c, lo, hi), lo), torch.device("cpu"), force_collectives=force)
        Dr, Ir = jr.topk(r, k)
        D, I = idx.search(HostSets(q), k)
        checks = {"exchange": idx.exchange, "D": np.array_equal(D.numpy(), Dr), "I": np.array_equal(I.numpy(), Ir),
                  "own_row_first": Ir[0, 0] == n - 1 and Dr[0, 0] == 1.0}
        if k > n:
            checks["padding"] = bool((Ir[:, n:] == -1).all())
        for edges in ((0.2, 0.8), (0.0,), (0.1, 0.2, 0.25, 0.3, 0.5, 0.8, 1.0)):
            cr, fr = jr.bands(r, edges)
            cs, fs = idx.bands(HostSets(q), edges)
            checks[f"bands{len(edges)}"] = (np.array_equal(cs.numpy(), cr) and np.array_equal(fs.numpy(), fr)
                                            and cs.dtype == torch.int64 and fs.dtype == torch.int64 and bool((cr.sum(1) == n).all()))
        cr, fr = jr.bands(r, (0.2, 0.8))
        checks["only_row_on_last_rank"] = cr[0, 2] == 1 and fr[0, 2] == n - 1 and bool((fr[1:, 2] == -1).all())
        bad = [name for name, good in checks.items() if not good]
        open(os.path.join(out_dir, f"rank{rank}.txt"), "w").write("ok" if not bad else "MISMATCH " + " ".join(bad))
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("world,n,k,force", [(1, 101, 20, True), (2, 401, 20, False), (3, 100, 120, False), (3, 2, 5, False)])
def test_sharded_jaccard_index_equals_unsharded(tmp_path, world, n, k, force):
    """(3, 100, 120): padding crosses the merge; (3, 2, 5): fewer rows than ranks, rank 2 holds nothing and rank 1 the one
    row of query 0's top band."""
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    mp.spawn(_worker, args=(world, port, str(tmp_path), n, k, force), nprocs=world, join=True)
    for r in range(world):
        assert open(tmp_path / f"rank{r}.txt").read() == "ok"


def test_one_rank_without_exchange_returns_the_local_result():
    q, c = shard_case(50)
    idx = ShardedJaccardIndex(OracleEngine(c, 0), torch.device("cpu"))
    r = jr.ratios(q, c)
    D, I = idx.search(HostSets(q), 7)
    cs, fs = idx.bands(HostSets(q), (0.2, 0.8))
    assert not idx.exchange and np.array_equal(I.numpy(), jr.topk(r, 7)[1]) and np.array_equal(D.numpy(), jr.topk(r, 7)[0])
    assert np.array_equal(cs.numpy(), jr.bands(r, (0.2, 0.8))[0]) and np.array_equal(fs.numpy(), jr.bands(r, (0.2, 0.8))[1])
