"""gloo tests (world sizes 2 and 4, plus the one-rank forced route) of row sharding for the index kinds beyond
inner-product top-k: the L2 metric, range_search in both metrics, and the binary (Hamming) index.

As in tests/test_distributed_cpu.py the HIP engines cannot run here, so oracle-backed engines with the same
interface are injected: what is exercised is the product's packing, the negation that carries an ascending order
through the one descending merge, the two-collective range exchange with its device-side assembly, and the shard
ordering.  Every comparison is np.array_equal against the UNSHARDED reference over the whole corpus.
"""
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from oracle import search_ref as sr
from sessionsimilaritysearch_amd.distributed import ShardedFlatIndex, shard_range


def _merge(pack_all, chunk, shards, nq, k, D_out, I_out):
    """The contract of sss_topk_merge ((score desc, id asc), ids < 0 are padding) through the oracle."""
    nk = nq * k
    Ds, Is = [], []
    for s in range(shards):
        blk = pack_all[s * chunk:(s + 1) * chunk]
        Is.append(blk[:nk].view(nq, k).numpy())
        Ds.append(blk[nk:].view(torch.float32)[:nk].view(nq, k).numpy())
    d, i = sr.merge_topk(Ds, Is, k)
    d, i = np.ascontiguousarray(d), np.ascontiguousarray(i)
    d[i < 0] = sr.NEG_SENTINEL                               # what the kernel writes beside an id of -1
    D_out.copy_(torch.from_numpy(d)); I_out.copy_(torch.from_numpy(i))


class FlatOracleEngine:
    """A FlatIndex shard (either metric) restated on the oracle: search and range_search with global ids."""

    def __init__(self, shard, id_offset, metric):
        self.shard, self.off, self.metric = shard, id_offset, metric
        self.ascending = metric == "l2"

    def _scores(self, q):
        return (sr.canonical_l2 if self.ascending else sr.canonical_scores)(q.numpy(), self.shard)

    def local_search(self, q, k, D, I, status):
        d, i = sr.topk_from_scores(self._scores(q), k, id_offset=self.off, largest=not self.ascending)
        D.copy_(torch.from_numpy(d)); I.copy_(torch.from_numpy(i)); status.zero_()

    def fix_unproven(self, q, k, D, I, status):
        return 0

    def local_range_search(self, q, radius):
        s = self._scores(q)
        rad = np.broadcast_to(np.asarray(radius, np.float32).reshape(-1, 1), (s.shape[0], 1))
        lims, D, I = _kept(s, rad, self.ascending, self.off)
        return torch.from_numpy(lims), torch.from_numpy(D), torch.from_numpy(I)

    merge = staticmethod(_merge)


class HammingOracleEngine:
    def __init__(self, shard, id_offset):
        self.shard, self.off = shard, id_offset

    def local_search(self, codes, k):
        d, i = sr.hamming_search(codes.numpy(), self.shard, k, id_offset=self.off)
        return torch.from_numpy(d), torch.from_numpy(i)

    merge = staticmethod(_merge)


def _kept(scores, rad, ascending, id_offset=0):
    """(lims, D, I) of the rows a range search keeps: score > radius (inner product) / distance < radius (L2),
    queries in order, ids ascending."""
    mask = scores < rad if ascending else scores > rad
    rows, cols = np.nonzero(mask)                            # row-major: query order, then ascending id
    lims = np.zeros(scores.shape[0] + 1, np.int64)
    np.cumsum(mask.sum(1), out=lims[1:])
    return lims, np.ascontiguousarray(scores[rows, cols], np.float32), cols.astype(np.int64) + id_offset


def _hamming_ref(q, c, k):
    """numpy unpackbits popcount, (distance asc, id asc), padding (0x7fffffff, -1)."""
    dist_ = (np.unpackbits(q[:, None, :] ^ c[None, :, :], axis=2).sum(2)).astype(np.int64)
    n = c.shape[0]
    ids = np.broadcast_to(np.arange(n, dtype=np.int64), dist_.shape)
    order = np.lexsort((ids, dist_), axis=1)[:, :k]
    D = np.full((q.shape[0], k), 0x7fffffff, np.int32)
    I = np.full((q.shape[0], k), -1, np.int64)
    D[:, :order.shape[1]] = np.take_along_axis(dist_, order, axis=1)
    I[:, :order.shape[1]] = order
    return D, I


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _run(worker, world, tmp_path, *args):
    mp.spawn(worker, args=(world, _free_port(), str(tmp_path)) + args, nprocs=world, join=True)
    for r in range(world):
        assert open(tmp_path / f"rank{r}.txt").read() == "ok"


def _init(rank, world, port):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)


def _report(out_dir, rank, checks):
    bad = [name for name, good in checks.items() if not good]
    open(os.path.join(out_dir, f"rank{rank}.txt"), "w").write("ok" if not bad else "MISMATCH " + " ".join(bad))


# ------------------------------------------------------------------------------------------------ L2 search
def _l2_case(n, d=32, nq=13):
    rng = np.random.default_rng(99)
    q = rng.standard_normal((nq, d)).astype(np.float32)
    c = rng.standard_normal((n, d)).astype(np.float32)
    if n >= 4:
        c[1] = c[n - 2]                                      # a cross-shard exact tie ...
        q[0] = c[1] + np.float32(0.01)                       # ... at the head of query 0's list
    return q, c


def _worker_l2(rank, world, port, out_dir, n, k, force):
    _init(rank, world, port)
    try:
        q, c = _l2_case(n)
        lo, hi = shard_range(n, world, rank)
        idx = ShardedFlatIndex(FlatOracleEngine(c[lo:hi], lo, "l2"), torch.device("cpu"), force_collectives=force)
        ref = sr.FlatIndexRef(c.shape[1], "l2")
        ref.add(c)
        Dr, Ir = ref.search(q, k)
        tq = torch.from_numpy(q)
        D, I = (t.numpy().copy() for t in idx.search(tq, k))
        D2, I2, st = idx.search_async(tq, k)
        checks = {"exchange": idx.exchange, "ascending": idx.ascending,
                  "search_I": np.array_equal(I, Ir), "search_D": np.array_equal(D, Dr),
                  "async_I": np.array_equal(I2.numpy(), Ir), "async_D": np.array_equal(D2.numpy(), Dr),
                  "status": int(st.sum()) == 0}
        if n >= 4:
            checks["tie_is_first"] = Ir[0, 0] == 1 and Ir[0, 1] == n - 2 and Dr[0, 0] == Dr[0, 1]
        if k > n:
            checks["padding"] = bool((Ir[:, n:] == -1).all() and (Dr[:, n:] == np.float32(3.4028234663852886e38)).all())
        _report(out_dir, rank, checks)
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("world,n,k", [(2, 1001, 10), (4, 403, 10), (2, 5, 10), (4, 3, 10)])
def test_sharded_l2_search_equals_unsharded(tmp_path, world, n, k):
    """(2, 5, 10): fewer than k rows in all, so padding crosses the negation; (4, 3, 10): rank 3 holds no row."""
    _run(_worker_l2, world, tmp_path, n, k, False)


def test_l2_one_rank_forced_exchange_route(tmp_path):
    _run(_worker_l2, 1, tmp_path, 300, 7, True)


def test_one_rank_without_exchange_returns_the_local_l2_result_untouched():
    q, c = _l2_case(50)
    idx = ShardedFlatIndex(FlatOracleEngine(c, 0, "l2"), torch.device("cpu"))
    ref = sr.FlatIndexRef(c.shape[1], "l2")
    ref.add(c)
    Dr, Ir = ref.search(q, 60)
    D, I = idx.search(torch.from_numpy(q), 60)
    assert not idx.exchange and np.array_equal(D.numpy(), Dr) and np.array_equal(I.numpy(), Ir)


# --------------------------------------------------------------------------------------------- range search
def _range_case(metric, variant, n, d=16, nq=9):
    """Corpus, queries and per-query float32 radii.  "edges": query 0 has no hit, query 1 keeps every row, the
    others a few percent of the rows.  "idle_rank": the rows of the second half of the corpus (all that the last rank
    holds at world 2, and the last two at world 4) lie where no query reaches, so those ranks contribute nothing."""
    rng = np.random.default_rng(17)
    q = sr.normalize(rng.standard_normal((nq, d)).astype(np.float32))
    c = sr.normalize(rng.standard_normal((n, d)).astype(np.float32))
    if variant == "idle_rank":
        q = np.abs(q)                                        # inner product: those rows score <= 0; L2: they are far away
        c[n - n // 2:] = -np.abs(c[n - n // 2:]) if metric == "ip" else c[n - n // 2:] + np.float32(20.0)
    s = sr.canonical_l2(q, c) if metric == "l2" else sr.canonical_scores(q, c)
    part = s[:, :n - n // 2] if variant == "idle_rank" else s
    rad = np.quantile(part, 0.05 if metric == "l2" else 0.95, axis=1).astype(np.float32)
    if variant == "edges":
        rad[0] = s.min() - 1 if metric == "l2" else s.max() + 1
        rad[1] = s.max() + 1 if metric == "l2" else s.min() - 1
    return q, c, rad, s


def _worker_range(rank, world, port, out_dir, metric, variant, n, force):
    _init(rank, world, port)
    try:
        q, c, rad, s = _range_case(metric, variant, n)
        lims_r, D_r, I_r = _kept(s, rad[:, None], metric == "l2")
        lo, hi = shard_range(n, world, rank)
        eng = FlatOracleEngine(c[lo:hi], lo, metric)
        idx = ShardedFlatIndex(eng, torch.device("cpu"), force_collectives=force)
        lims, D, I = idx.range_search(torch.from_numpy(q), torch.from_numpy(rad))
        checks = {"exchange": idx.exchange, "lims": np.array_equal(lims.numpy(), lims_r),
                  "I": np.array_equal(I.numpy(), I_r), "D": np.array_equal(D.numpy(), D_r),
                  "dtypes": lims.dtype == torch.int64 and I.dtype == torch.int64 and D.dtype == torch.float32,
                  "some_hits": lims_r[-1] > 0}
        if variant == "edges":
            checks["no_hit_query"] = lims_r[1] == lims_r[0]
            checks["all_rows_query"] = lims_r[2] - lims_r[1] == n
            lims1, D1, I1 = idx.range_search(torch.from_numpy(q), float(rad[2]))        # a scalar radius
            l1, d1, i1 = _kept(s, np.full((q.shape[0], 1), rad[2], np.float32), metric == "l2")
            checks["scalar_radius"] = (np.array_equal(lims1.numpy(), l1) and np.array_equal(I1.numpy(), i1)
                                       and np.array_equal(D1.numpy(), d1))
            lims0, D0, I0 = idx.range_search(torch.from_numpy(q), float(rad[0]))        # nobody has a hit: no payload
            checks["empty_result"] = int(lims0.sum()) == 0 and D0.numel() == 0 and I0.numel() == 0
        else:
            last_lo = shard_range(n, world, world - 1)[0]
            checks["last_rank_idle"] = world == 1 or bool((I_r < last_lo).all())
        _report(out_dir, rank, checks)
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("world", [2, 4])
@pytest.mark.parametrize("variant", ["edges", "idle_rank"])
@pytest.mark.parametrize("metric", ["ip", "l2"])
def test_sharded_range_search_equals_unsharded(tmp_path, metric, variant, world):
    _run(_worker_range, world, tmp_path, metric, variant, 403, False)


@pytest.mark.parametrize("metric", ["ip", "l2"])
def test_range_search_one_rank_forced_exchange_route(tmp_path, metric):
    _run(_worker_range, 1, tmp_path, metric, "edges", 200, True)


def test_range_search_with_fewer_rows_than_ranks(tmp_path):
    """world 4 over 3 rows: rank 3 holds nothing."""
    _run(_worker_range, 4, tmp_path, "l2", "edges", 3, False)


# -------------------------------------------------------------------------------------------------- Hamming
def _hamming_case(name):
    rng = np.random.default_rng(23)
    if name == "ties":                                       # 403 rows drawn from 6 codes: every list is runs of exact ties
        base = rng.integers(0, 256, (6, 16), dtype=np.uint8)
        c = base[rng.integers(0, 6, 403)]
        q = np.concatenate([base[:3], rng.integers(0, 256, (4, 16), dtype=np.uint8)])
        return q, c, 40
    if name == "k_beyond_shard":                             # 10 rows per rank at world 4, k = 25; 50 > n: padding
        return rng.integers(0, 256, (5, 32), dtype=np.uint8), rng.integers(0, 256, (40, 32), dtype=np.uint8), 25
    if name == "k_beyond_corpus":
        return rng.integers(0, 256, (5, 32), dtype=np.uint8), rng.integers(0, 256, (40, 32), dtype=np.uint8), 50
    if name == "fewer_rows_than_ranks":
        return rng.integers(0, 256, (3, 16), dtype=np.uint8), rng.integers(0, 256, (3, 16), dtype=np.uint8), 4
    assert name == "bits1600"                                # the sign code of the 1600-wide vector: 200 bytes
    c = rng.integers(0, 256, (101, 200), dtype=np.uint8)
    c[7] = c[95]
    return np.concatenate([c[7:8], rng.integers(0, 256, (3, 200), dtype=np.uint8)]), c, 10


def _worker_hamming(rank, world, port, out_dir, name, force):
    from sessionsimilaritysearch_amd.distributed import ShardedBinaryIndex
    _init(rank, world, port)
    try:
        q, c, k = _hamming_case(name)
        n = c.shape[0]
        Dr, Ir = _hamming_ref(q, c, k)
        lo, hi = shard_range(n, world, rank)
        idx = ShardedBinaryIndex(HammingOracleEngine(c[lo:hi], lo), torch.device("cpu"), force_collectives=force)
        D, I = idx.search(torch.from_numpy(q), k)
        checks = {"exchange": idx.exchange, "D": np.array_equal(D.numpy(), Dr), "I": np.array_equal(I.numpy(), Ir),
                  "dtypes": D.dtype == torch.int32 and I.dtype == torch.int64}
        if name == "ties":
            checks["ties_present"] = bool((np.diff(Dr, axis=1) == 0).sum() > Dr.size // 2)
        if name == "bits1600":
            checks["tie_pair"] = Ir[0, 0] == 7 and Ir[0, 1] == 95 and Dr[0, 0] == 0 and Dr[0, 1] == 0
        if k > n:
            checks["padding"] = bool((Ir[:, n:] == -1).all() and (Dr[:, n:] == 0x7fffffff).all())
        _report(out_dir, rank, checks)
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("world", [2, 4])
@pytest.mark.parametrize("name", ["ties", "k_beyond_shard", "k_beyond_corpus", "fewer_rows_than_ranks", "bits1600"])
def test_sharded_hamming_search_equals_unsharded(tmp_path, name, world):
    _run(_worker_hamming, world, tmp_path, name, False)


def test_hamming_one_rank_forced_exchange_route(tmp_path):
    _run(_worker_hamming, 1, tmp_path, "ties", True)
