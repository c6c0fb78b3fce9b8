"""CPU side of the product-type index (include/sss_ptype.h): the numpy helper (tests/helpers/type_score_ref.py, the score of
record) against what the reference's own get_score('all_product_type_score') produced for every pair
(tests/golden/type_score_truth.npz), the header against its ctypes binding, every argument error of the entry points and
of the Python layer that needs no device, and ShardedProductTypeIndex on gloo with an oracle engine.

The reference normalises each count vector first and sums the products in first-occurrence order, so its float64 value is
not the score of record: the generator measured their largest distance (max_ulp, in units of the last place) and stored
twice that as the tolerance (tol_ulp) -- the doubling covers orderings the fixture does not contain.  A pair whose score of
record lies within tol_ulp of a band edge can fall on either side of it in the reference; every other pair must be in the
same band, and those near-edge pairs must stay a small share (CAP) of all pairs for the fixture to test the bands at all."""
import ctypes
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
import type_score_ref as tr  # noqa: E402

from sessionsimilaritysearch_amd import _lib  # noqa: E402
from sessionsimilaritysearch_amd.sessions import ActionTable  # noqa: E402
from sessionsimilaritysearch_amd.distributed import ShardedProductTypeIndex, shard_range  # noqa: E402
from test_eval_metrics_cpu import AVE_TOL, GAMMA, golden  # noqa: E402
from test_sparse_index_cpu import OracleEngine as SparseOracle  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TRUTH = os.path.join(ROOT, "tests", "golden", "type_score_truth.npz")
SIM = "all_product_type_score"
EDGE_SETS = ((0.2, 0.8), (0.2, 0.5))
CAP = 0.025                          # the near-edge pairs' largest share of all pairs, per edge set: a condition of the fixture
NAMES = ["sss_ptype_bands", "sss_ptype_pair_scores", "sss_ptype_topk", "sss_ptype_topk_workspace_bytes", "sss_type_bags_count",
         "sss_type_bags_fill"]
_CACHE = {}


def truth():
    """(the generator's arrays, the eval fixture, its action tables, the host bags of the `all` queries, of the corpus, the
    helper's score matrix), made once."""
    if "t" not in _CACHE:
        t = np.load(TRUTH)
        g, tab = golden()
        it = t["item_type"]
        qb = tr.bags(ActionTable.concat(tab["seq"], tab["tar"]), it)
        cb = tr.bags(tab["corpus"], it)
        _CACHE["t"] = (t, g, tab, qb, cb, tr.scores(qb, cb, int(t["n_types"])))
    return _CACHE["t"]


def test_helper_reproduces_the_reference_within_the_stored_tolerance():
    t, g, _, qb, cb, s = truth()
    ref = t["ref_all_product_type_score"]
    assert ref.shape == (48, 400) and ref.dtype == np.float64 and s.shape == ref.shape
    d = tr.ulp_distance(ref, s)
    print("largest distance in ulp:", int(d.max()), "stored:", int(t["max_ulp"]), "tolerance:", int(t["tol_ulp"]))
    assert int(d.max()) == int(t["max_ulp"]) and int(t["tol_ulp"]) == 2 * int(t["max_ulp"]) and 0 < int(t["max_ulp"]) <= 4
    assert (d <= int(t["tol_ulp"])).all()
    assert ((s == 0) == (ref == 0)).all()                            # no shared type: exactly 0 on both sides
    assert s.max() == 1.0 and ref.max() > 1.0                        # parallel bags: 1.0 of record, above 1 in the reference


@pytest.mark.parametrize("which", [0, 1])
def test_helper_bands_equal_the_reference_outside_the_near_edge_pairs(which):
    t, _, _, _, _, s = truth()
    edges = EDGE_SETS[which]
    assert tuple(t["edge_sets"][which]) == edges
    ref = t["ref_all_product_type_score"]
    near = tr.near_edge(s, edges, int(t["tol_ulp"]))
    band = lambda x: (x[:, :, None] >= np.asarray(edges)[None, None, :]).sum(2)
    differ = band(ref) != band(s)
    print(f"edges {edges}: near-edge share {near.mean():.4%}, band disagreements {int(differ.sum())}, outside {int((differ & ~near).sum())}")
    assert not (differ & ~near).any() and int(t["outside_disagreements"]) == 0
    assert near.mean() == float(t["near_share"][which]) and near.mean() <= CAP
    assert differ.any()                                              # the deviation is real: the reference misplaces some pairs
    counts, first = tr.bands(s, edges)
    assert np.array_equal(counts, np.stack([(band(s) == b).sum(1) for b in range(3)], 1)) and (counts.sum(1) == 400).all()
    assert np.array_equal(first[:, 0], [np.flatnonzero(row == 0)[0] if (row == 0).any() else -1 for row in band(s)])


def test_fixture_holds_what_the_gpu_tests_rely_on():
    t, g, tab, qb, cb, s = truth()
    it = t["item_type"]
    assert it.dtype == np.int32 and it.shape == (int(g["n_items"]),) and it.min() == -1 and it.max() == int(t["n_types"]) - 1
    assert 0.05 < (it < 0).mean() < 0.2 and len(np.unique(it[it >= 0])) == int(t["n_types"]) == 12
    for edges in EDGE_SETS:
        assert int((tr.bands(s, edges)[0] > 0).all(1).sum()) >= 10    # queries with rows in all three bands
    D, _ = tr.topk(s, 101)
    assert int((D[:, 19] == D[:, 20]).sum()) >= 5 and int((D[:, 99] == D[:, 100]).sum()) >= 5     # ties at the k-th place
    assert int((np.diff(cb[0]) == 0).sum()) >= 16                     # the 16 corpus sessions without a click, and the untyped
    n_click = np.array([int((~tab["corpus"].is_search[a:b]).sum()) for a, b in zip(tab["corpus"].sess_ptr[:-1], tab["corpus"].sess_ptr[1:])])
    assert int((n_click == 0).sum()) == 16 and (np.diff(cb[0])[n_click == 0] == 0).all()
    assert cb[2].max() >= 3 and cb[2].min() == 1 and (cb[2] == np.round(cb[2])).all()      # counts over actions, not items
    ids, sc, keep = tr.mine(s)
    assert keep.sum() >= 10 and (sc[keep, 0] >= 0.8).all() and (sc[keep, 2] < 0.2).all()
    assert (s == 0.5).any() and (s == 1.0).any()                      # pairs exactly on an edge of (0.2, 0.5), parallel pairs


def test_helper_reproduces_the_reference_metrics():
    """get_ave_score / get_recall restated on the helper's matrix, held to the reference's recorded values by the bounds
    tests/test_eval_metrics_cpu.py derives for the Jaccard kinds (AVE_TOL: a float32 pairwise mean of float32 pair scores;
    GAMMA(nq): two float64 means of the same nq integers)."""
    t, g, _, _, _, s = truth()
    I, thres = g["I"], g["thres"]
    nq, K = I.shape
    s32 = np.take_along_axis(s, I, axis=1).astype(np.float32)
    ave = float(s32.astype(np.float64).sum()) / s32.size
    print("ave:", ave, "reference:", float(t["ref_ave"]), "bound:", AVE_TOL(nq * K))
    assert abs(ave - float(t["ref_ave"])) <= AVE_TOL(nq * K)
    for th, want in zip(thres, t["ref_recall"]):
        got = float(np.mean((s32 > np.float32(th)).sum(1).astype(np.float64))) / K
        print(f"recall > {th}: {got}, reference {float(want)}")
        assert abs(got - float(want)) <= GAMMA(nq)


def test_helper_by_hand():
    q = tr.triple([{3: 2, 5: 1}, {}, {0: 4}, {1: 3, 2: 4}])
    c = tr.triple([{3: 4, 5: 2}, {5: 7}, {}, {0: 1, 9: 1}, {1: 4, 2: 3}])
    s = tr.scores(q, c)
    assert s[0, 0] == 1.0 and s[0, 1] == 7 / np.sqrt(np.float64(5 * 49)) and s[0, 2] == 0 and s[0, 3] == 0
    assert (s[1] == 0).all() and s[2, 3] == 4 / np.sqrt(np.float64(16 * 2)) and s[3, 4] == 24 / np.sqrt(np.float64(625))
    assert s[3, 4] == 0.96 and np.array_equal(tr.dense(q, 6)[0], [0, 0, 0, 2, 0, 1])
    # exactly on 0.8: dot^2 * 25 == 16 * nq2 * nc2 gives the double nearest 0.8; exactly parallel gives 1.0
    on = tr.scores(tr.triple([{0: 4, 1: 3}]), tr.triple([{0: 1}, {0: 8, 1: 6}, {0: 1, 1: 1, 2: 1, 3: 1}]))
    assert on[0].tolist() == [0.8, 1.0, 7 / 10]
    tab = ActionTable(np.array([0, 4, 4, 6], np.int64), np.array([0, 1, 0, 0, 0, 0], bool), np.array([2, 0, 2, 1, 0, 3], np.int64),
                      np.zeros(6, np.int64))
    ptr, ty, cnt = tr.bags(tab, np.array([-1, 7, 4, 4], np.int32))
    assert ptr.tolist() == [0, 2, 2, 3] and ty.tolist() == [4, 7, 4] and cnt.tolist() == [2, 1, 1] and cnt.dtype == np.float32


# ------------------------------------------------------------------------------------------------ the C ABI
def test_ptype_header_and_binding_declare_the_same_entry_points():
    names = declared("sss_ptype.h")
    assert names == _lib.symbols("sss_ptype.h") == NAMES
    L = _lib.lib()
    for n in names:
        assert getattr(L, n).argtypes == _lib.HEADERS["sss_ptype.h"][n][1] and getattr(L, n).restype is _lib.HEADERS["sss_ptype.h"][n][0]
    for header, table in _lib.HEADERS.items():
        if header != "sss_ptype.h":
            assert not set(names) & set(table) and not set(names) & set(declared(header)), header
    assert sorted(_lib.HEADERS) == sorted(f for f in os.listdir(os.path.join(ROOT, "include")) if f.endswith(".h"))
    assert declared("sss.h") == _lib.exported_symbols() and len(_lib.exported_symbols()) == 60
    text = open(os.path.join(ROOT, "include", "sss_ptype.h")).read()
    assert "CALLER-OWNED DEVICE" in text and "-2 workspace too small" in text and "HOST array" in text
    assert "SCORE OF RECORD" in text and "__dsqrt_rn" in text and "2^26" in text and "DEVIATION" in text


_P = 1 << 20                                                          # a non-null, 256-byte aligned address; never dereferenced


def _edges(*v):
    return (ctypes.c_double * len(v))(*v)


def _topk(L, **kw):
    a = dict(qp=_P, qi=_P, qw=_P, nq=4, cp=_P, ci=_P, cw=_P, n=1000, k=10, off=0, D=_P, I=_P, ws=_P, wsb=0)
    a.update(kw)
    return L.sss_ptype_topk(*[a[x] for x in ("qp", "qi", "qw", "nq", "cp", "ci", "cw", "n", "k", "off", "D", "I", "ws", "wsb")], 0)


def _bands(L, **kw):
    a = dict(qp=_P, qi=_P, qw=_P, nq=4, cp=_P, ci=_P, cw=_P, n=1000, e=_edges(0.2, 0.8), ne=2, off=0, c=_P, f=_P)
    a.update(kw)
    a["e"] = a["e"] if isinstance(a["e"], int) else ctypes.addressof(a["e"])
    return L.sss_ptype_bands(*[a[x] for x in ("qp", "qi", "qw", "nq", "cp", "ci", "cw", "n", "e", "ne", "off", "c", "f")], 0)


def _pairs(L, **kw):
    a = dict(qp=_P, qi=_P, qw=_P, nq=4, cp=_P, ci=_P, cw=_P, n=1000, I=_P, K=10, off=0, s=_P, err=_P)
    a.update(kw)
    return L.sss_ptype_pair_scores(*[a[x] for x in ("qp", "qi", "qw", "nq", "cp", "ci", "cw", "n", "I", "K", "off", "s", "err")], 0)


def _count(L, **kw):
    a = dict(sp=_P, isr=_P, item=_P, S=5, ty=_P, ni=100, nt=12, counts=_P, err=_P)
    a.update(kw)
    return L.sss_type_bags_count(*[a[x] for x in ("sp", "isr", "item", "S", "ty", "ni", "nt", "counts", "err")], 0)


def _fill(L, **kw):
    a = dict(sp=_P, isr=_P, item=_P, S=5, ty=_P, ni=100, nt=12, ptr=_P, items=_P, w=_P, err=_P)
    a.update(kw)
    return L.sss_type_bags_fill(*[a[x] for x in ("sp", "isr", "item", "S", "ty", "ni", "nt", "ptr", "items", "w", "err")], 0)


def check_argument_errors(L):
    """Every bad argument of every entry point is -1 (-2 for the workspace) with a message.  No address given here is memory:
    a call that launched would fault, and a top-k that skipped a check would return -2 for its empty workspace."""
    assert _topk(L) == -2 and b"workspace" in L.sss_last_error()                          # valid but for the workspace
    need = L.sss_ptype_topk_workspace_bytes(4, 1000)
    assert need >= 4 * 1000 * 4 and _topk(L, wsb=need - 1) == -2
    for bad in (dict(k=0), dict(k=1025), dict(k=-3), dict(nq=0), dict(nq=65536), dict(nq=-1), dict(n=0), dict(n=1 << 31)):
        assert _topk(L, **bad) == -1 and b"ptype_topk" in L.sss_last_error(), bad
    for name in ("qp", "qi", "qw", "cp", "ci", "cw", "D", "I", "ws"):
        assert _topk(L, **{name: 0}) == -1 and b"null" in L.sss_last_error(), name
    assert _topk(L, ws=_P + 8) == -1 and b"aligned" in L.sss_last_error()
    assert L.sss_ptype_topk_workspace_bytes(0, 10) == 0 and L.sss_ptype_topk_workspace_bytes(10, 0) == 0
    inf, nan = float("inf"), float("nan")
    for bad in (dict(nq=0), dict(nq=65536), dict(n=0), dict(n=1 << 31), dict(ne=0), dict(ne=8), dict(ne=-1), dict(off=-1),
                dict(off=2 ** 63 - 1000), dict(e=_edges(0.8, 0.2)), dict(e=_edges(0.2, 0.2)), dict(e=_edges(0.2, inf)),
                dict(e=_edges(-inf, 0.2)), dict(e=_edges(nan, 0.2)), dict(e=_edges(0.2, nan)),
                dict(e=_edges(.1, .2, .3, .4, .5, .6, .6), ne=7)):
        assert _bands(L, **bad) == -1 and b"ptype_bands" in L.sss_last_error(), bad
    for name in ("qp", "qi", "qw", "cp", "ci", "cw", "e", "c", "f"):
        assert _bands(L, **{name: 0}) == -1 and b"null" in L.sss_last_error(), name
    for bad in (dict(K=0), dict(K=1025), dict(K=-1), dict(nq=0), dict(nq=-5), dict(nq=1 << 31), dict(n=0), dict(n=1 << 31)):
        assert _pairs(L, **bad) == -1 and b"ptype_pair_scores" in L.sss_last_error(), bad
    for name in ("qp", "qi", "qw", "cp", "ci", "cw", "I", "s", "err"):
        assert _pairs(L, **{name: 0}) == -1 and b"null" in L.sss_last_error(), name
    for call, what, ptrs in ((_count, b"type_bags_count", ("sp", "isr", "item", "ty", "counts", "err")),
                             (_fill, b"type_bags_fill", ("sp", "isr", "item", "ty", "ptr", "items", "w", "err"))):
        for bad in (dict(S=0), dict(S=-1), dict(S=1 << 31), dict(ni=0), dict(ni=1 << 31), dict(nt=0), dict(nt=-1), dict(nt=1 << 31)):
            assert call(L, **bad) == -1 and what in L.sss_last_error(), bad
        for name in ptrs:
            assert call(L, **{name: 0}) == -1 and b"null" in L.sss_last_error(), name


def test_every_entry_point_validates_before_any_launch():
    check_argument_errors(_lib.lib())


def test_python_layer_validates_without_a_device():
    import sessionsimilaritysearch_amd as pkg
    from sessionsimilaritysearch_amd import distributed, evaluation, jaccard, product_types as pt
    assert pkg.ProductTypeIndex is pt.ProductTypeIndex and pkg.type_bags is pt.type_bags
    assert "ProductTypeIndex" in pkg.__all__ and "type_bags" in pkg.__all__
    assert issubclass(pt.ProductTypeIndex, pt.BandIndex) and issubclass(jaccard.JaccardIndex, jaccard.BandIndex)
    assert pt.ProductTypeIndex.weighted and not jaccard.JaccardIndex.weighted
    assert pt.mine_triples is jaccard.mine_triples and pt.neighbourhood_recall is jaccard.neighbourhood_recall
    assert callable(jaccard.pair_scores) and callable(jaccard.JaccardIndex.pair_scores) and callable(pt.ProductTypeIndex.pair_scores)
    assert issubclass(distributed.ShardedProductTypeIndex, distributed.ShardedJaccardIndex)
    assert issubclass(distributed.ProductTypeEngine, distributed.JaccardEngine)
    for bad in (0, -1, 2 ** 31):
        with pytest.raises(ValueError):
            pt.ProductTypeIndex(bad, torch.device("cpu"))
    tab = ActionTable(np.array([0, 1], np.int64), np.array([0], bool), np.array([0], np.int64), np.zeros(1, np.int64))
    for bad in (np.zeros((2, 2), np.int32), np.zeros(0, np.int32), np.zeros(3, np.float32)):
        with pytest.raises(ValueError, match="item_type"):
            pt.type_bags(tab, bad)
    for bad in (0, -4, 2 ** 31):
        with pytest.raises(ValueError, match="n_types"):
            pt.type_bags(tab, np.zeros(3, np.int32), n_types=bad)
    with pytest.raises(TypeError, match="SessionVectors"):
        pt.check_bags([[1, 2]])
    with pytest.raises(TypeError, match="SessionVectors"):
        evaluation.get_ave_score(np.zeros((1, 1), np.int64), ([], []), None, SIM)
    with pytest.raises(TypeError, match="SessionVectors"):
        evaluation.get_recall(None, None, np.zeros((1, 1), np.int64), SIM, 0.5)
    # the string kinds keep the ValueError they raised before
    for sim in ("all_query_score", "all_product_title_score", "nonsense"):
        with pytest.raises(ValueError, match="sim_type"):
            evaluation.get_ave_score(None, None, None, sim)
        with pytest.raises(ValueError, match="sim_type"):
            evaluation.get_recall(None, None, None, sim, 0.5)


# ------------------------------------------------------------------------------------------------ sharding (gloo)
class HostBags:
    def __init__(self, triple):
        self.triple = triple

    def __len__(self):
        return len(self.triple[0]) - 1


def rows_of(c, lo, hi):
    return c[0][lo:hi + 1] - c[0][lo], c[1][c[0][lo]:c[0][hi]], c[2][c[0][lo]:c[0][hi]]


class OracleEngine:
    """A ProductTypeIndex shard restated on the helper: search and bands with global ids."""
    merge = staticmethod(SparseOracle.merge)

    def __init__(self, shard, id_offset, n_types):
        self.shard, self.off, self.n_types = shard, id_offset, n_types

    def local_search(self, q, k, D, I):
        d, i = tr.topk(tr.scores(q.triple, self.shard, self.n_types), k, self.off)
        D.copy_(torch.from_numpy(d)); I.copy_(torch.from_numpy(i))

    def local_bands(self, q, edges):
        return tuple(torch.from_numpy(x) for x in tr.bands(tr.scores(q.triple, self.shard, self.n_types), edges, self.off))


def _worker(rank, world, port, out_dir, n, k, force):
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        t, _, _, qb, cb, s = truth()
        n_types = int(t["n_types"])
        c, r = rows_of(cb, 0, n), s[:, :n]
        lo, hi = shard_range(n, world, rank)
        idx = ShardedProductTypeIndex(OracleEngine(rows_of(c, lo, hi), lo, n_types), torch.device("cpu"), force_collectives=force)
        Dr, Ir = tr.topk(r, k)
        D, I = idx.search(HostBags(qb), k)
        checks = {"exchange": idx.exchange, "D": np.array_equal(D.numpy(), Dr), "I": np.array_equal(I.numpy(), Ir)}
        if k > n:
            checks["padding"] = bool((Ir[:, n:] == -1).all())
        for edges in ((0.2, 0.8), (0.0,), (0.1, 0.2, 0.25, 0.3, 0.5, 0.8, 1.0)):
            cr, fr = tr.bands(r, edges)
            cs, fs = idx.bands(HostBags(qb), edges)
            checks[f"bands{len(edges)}"] = (np.array_equal(cs.numpy(), cr) and np.array_equal(fs.numpy(), fr)
                                            and cs.dtype == torch.int64 and fs.dtype == torch.int64 and bool((cr.sum(1) == n).all()))
        bad = [name for name, good in checks.items() if not good]
        open(os.path.join(out_dir, f"rank{rank}.txt"), "w").write("ok" if not bad else "MISMATCH " + " ".join(bad))
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("world,n,k,force", [(1, 101, 20, True), (2, 400, 20, False), (3, 2, 5, False)])
def test_sharded_product_type_index_equals_unsharded(tmp_path, world, n, k, force):
    """(3, 2, 5): fewer rows than ranks -- rank 2 holds nothing -- and padding crosses the merge."""
    with socket.socket() as sock:
        sock.bind(("127.0.0.1", 0))
        port = sock.getsockname()[1]
    mp.spawn(_worker, args=(world, port, str(tmp_path), n, k, force), nprocs=world, join=True)
    for r in range(world):
        assert open(tmp_path / f"rank{r}.txt").read() == "ok"
