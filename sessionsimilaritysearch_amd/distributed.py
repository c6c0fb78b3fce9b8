"""Row-sharded flat index over the GPUs of one node: one process per GPU, the normalised corpus
split by rows, per-shard exact top-k, ONE all-gather of the packed (ids | scores) block over
RCCL/xGMI, then a k-way merge on every rank.

The reference is single-process (no NCCL/MPI call site anywhere); this is the one parallel
strategy the path needs, and the only collective is that all-gather of ``12 * nq * k`` bytes per
rank -- latency-bound, so it is a single ``all_gather_into_tensor`` rather than a ring of
small messages.  The query batch is embedded cooperatively: every rank embeds nq / world of the
sessions and one all-gather of ``4 * nq * d`` bytes hands every rank the whole batch
(``gather_query_embeddings``) -- once the scan takes ~0.1 ms per shard, embedding the full batch on
every rank would be the Amdahl term of strong scaling.

Every index kind shards this way.  ``ShardedFlatIndex`` serves both metrics and every d / k of ``FlatIndex``
(shapes without a fused scan run the shard's exhaustive kernels) and ``range_search``; ``ShardedBinaryIndex``
serves ``BinaryFlatIndex``; ``ShardedSparseIndex`` serves ``SparseSessionIndex``; ``ShardedJaccardIndex`` serves
``JaccardIndex`` and ``ShardedProductTypeIndex`` ``ProductTypeIndex`` (their band counts by two all-reduces).  All of
them merge through the one ``sss_topk_merge`` -- (score desc, id asc) --
so a contract that orders ascending (L2, Hamming) crosses the exchange NEGATED: float negation is exact and
``(-dist desc, id asc)`` is ``(dist asc, id asc)``.

The local search and the merge are injected (``engine``) so the sharding / packing / gather
logic can be exercised on CPU with the ``gloo`` backend in the tests; the default engines are the
HIP ones and have no CPU fallback.
"""
from __future__ import annotations

import torch
import torch.distributed as dist


def shard_range(n: int, world: int, rank: int):
    """Contiguous row range of ``rank``: sizes differ by at most one row, earlier ranks larger."""
    base, rem = divmod(n, world)
    lo = rank * base + min(rank, rem)
    return lo, lo + base + (1 if rank < rem else 0)


def query_slice(nq: int, world: int, rank: int):
    """Rows of the query batch that ``rank`` embeds; equal sizes (the all-gather needs them), so
    (0, nq) -- every rank embeds everything -- when world does not divide nq."""
    if world <= 1 or nq % world:
        return 0, nq
    per = nq // world
    return rank * per, (rank + 1) * per


def gather_query_embeddings(emb_local: torch.Tensor, nq: int, out: torch.Tensor | None = None, group=None,
                            force_collective: bool = False):
    """All ranks' [nq / world, d] slices (``query_slice`` order) -> the full [nq, d] batch on every rank.
    ``force_collective`` issues the all-gather even where it moves nothing new (one rank, or every rank
    embedded the whole batch and world == 1): the 1-rank RCCL execution of tests / ``bench.py --force-collectives``."""
    world = dist.get_world_size(group) if dist.is_initialized() else 1
    if force_collective and dist.is_initialized() and emb_local.shape[0] * world == nq:
        pass
    elif world == 1 or emb_local.shape[0] == nq:
        return emb_local
    if out is None:
        out = torch.empty((nq, emb_local.shape[1]), dtype=emb_local.dtype, device=emb_local.device)
    dist.all_gather_into_tensor(out, emb_local.contiguous(), group=group)
    return out


FLT_MAX = 3.4028234663852886e38
HAMMING_PAD = 0x7fffffff                # BinaryFlatIndex's distance of a missing result


def _merge_packs(pack_all, chunk, shards, nq, k, D_out, I_out):
    """``sss_topk_merge`` over ``shards`` packed (ids | scores) blocks of ``chunk`` int64 words each."""
    from . import _lib
    i_ptr = pack_all.data_ptr()
    d_ptr = i_ptr + nq * k * 8
    rc = _lib.lib().sss_topk_merge(d_ptr, 2 * chunk, i_ptr, chunk, shards, nq, k, D_out.data_ptr(),
                                   I_out.data_ptr(), _lib.stream_ptr(pack_all.device))
    _lib.check(rc, "sss_topk_merge")


class _Engine:
    """A shard's index and the merge of the ranks' packed results, the same for every index kind."""

    def __init__(self, index):
        self.index = index

    def merge(self, pack_all, chunk, shards, nq, k, D_out, I_out):
        _merge_packs(pack_all, chunk, shards, nq, k, D_out, I_out)


class HipEngine(_Engine):
    """Local search + merge of a ``FlatIndex`` shard through libsss (the product engine)."""

    def __init__(self, index):
        super().__init__(index)
        self.ascending = index.metric == "l2"       # results ordered (distance asc, id asc), padding (+FLT_MAX, -1)
        # running count of queries the fused path could not prove exact (device side, no sync)
        self.unproven = torch.zeros(1, dtype=torch.int32, device=index.device)

    def local_search(self, q, k, D, I, status):
        """This shard's top-k into D / I, no host sync.  With a fused scan (inner product or L2): ``status`` marks the
        queries it left unproven.  Without one (a dtype, d or k no fused scan serves, an empty shard): the exhaustive
        kernels, which are exact for every query, so ``status`` is all zero."""
        index = self.index
        if index._route(k):
            index.search_fused(q, k, (D, I, status), self.unproven)
            return
        status.zero_()
        if index.ntotal == 0:
            D.fill_(FLT_MAX if self.ascending else -FLT_MAX)
            I.fill_(-1)
        elif q.shape[0]:
            from . import _lib
            _lib.require_cuda(q, "q", index._tdtype)
            index._require_d_aligned()
            index.search_exhaustive(q, k, D, I)

    def fix_unproven(self, q, k, D, I, status):
        if not self.index._route(k):
            return 0                                # the exhaustive route left nothing unproven
        return self.index.fix_unproven(q, k, D, I, status)

    def local_range_search(self, q, radius):
        """This shard's (lims, D, I) with global ids, ids ascending per query."""
        return self.index.range_search_device(q, radius)


class HammingEngine(_Engine):
    """Local search + merge of a ``BinaryFlatIndex`` shard through libsss."""

    def local_search(self, codes, k):
        """This shard's (D int32, I int64) by (distance asc, id asc) with global ids, padding (0x7fffffff, -1);
        any k (beyond the fused capacity: the shard's exhaustive route)."""
        return self.index.search(codes, k)


class SparseEngine(_Engine):
    """Local search + merge of a ``SparseSessionIndex`` shard through libsss."""

    def local_search(self, vectors, k, D, I):
        """This shard's top-k by (score desc, id asc) with global ids (``index.id_offset`` = first row of the shard),
        padding (-FLT_MAX, -1), into D / I; no host sync."""
        self.index.search_device(vectors, k, D, I)


class JaccardEngine(_Engine):
    """Local search, bands + merge of a ``JaccardIndex`` shard through libsss."""

    def local_search(self, sets, k, D, I):
        """This shard's top-k by (score desc, id asc) with global ids, padding (-FLT_MAX, -1), into D / I; no host sync."""
        self.index.search_device(sets, k, D, I)

    def local_bands(self, sets, edges):
        """This shard's (counts, first) int64 [nq, len(edges) + 1] with global ids in ``first`` (-1: none)."""
        return self.index.bands(sets, edges)


class ProductTypeEngine(JaccardEngine):
    """Local search, bands + merge of a ``ProductTypeIndex`` shard through libsss: ``JaccardEngine``'s calls, over bags."""


def range_chunk_words(m: int) -> int:
    """int64 words of one rank's range payload of ``m`` entries: m ids, then m float32 scores (as ``_buffers``)."""
    return m + (m + 1) // 2


def pack_range(D: torch.Tensor, I: torch.Tensor, m: int) -> torch.Tensor:
    """One rank's range result as the (ids | scores) block of the exchange, padded to ``m`` entries."""
    t = I.numel()
    pack = torch.zeros(range_chunk_words(m), dtype=torch.int64, device=I.device)
    pack[:t] = I
    pack[m:].view(torch.float32)[:t] = D
    return pack


def assemble_range(counts_all: torch.Tensor, pack_all: torch.Tensor, m: int, total: int):
    """(lims, D, I) of the whole corpus from the gathered per-rank results, on the device.

    ``counts_all`` is int64 [world, nq] (entries of rank r for query i), ``pack_all`` the ``world`` blocks of
    ``pack_range(.., m)`` in rank order, ``total`` = counts_all.sum().  Shards are contiguous row ranges in rank order
    and every rank lists a query's ids ascending, so the merged list of query i is the ranks' lists one after the
    other: segment (i, r) of the output starts at the exclusive scan of the counts in (query, rank) order and is
    read from rank r's block at that rank's own exclusive scan over its queries."""
    world, nq = counts_all.shape
    dev = counts_all.device
    lims = torch.zeros(nq + 1, dtype=torch.int64, device=dev)
    torch.cumsum(counts_all.sum(0), 0, out=lims[1:])
    if total == 0:
        return lims, torch.empty(0, dtype=torch.float32, device=dev), torch.empty(0, dtype=torch.int64, device=dev)
    seg_cnt = counts_all.t().reshape(-1)                                    # (query, rank) order
    dst = torch.cumsum(seg_cnt, 0) - seg_cnt                                # where a segment starts in the output
    src = (torch.cumsum(counts_all, 1) - counts_all).t().reshape(-1)        # ... and in its rank's own list
    seg = torch.repeat_interleave(torch.arange(nq * world, dtype=torch.int64, device=dev), seg_cnt, output_size=total)
    pos = torch.arange(total, dtype=torch.int64, device=dev) - dst[seg] + src[seg]
    rank = seg % world
    chunk = range_chunk_words(m)
    I = pack_all.view(world, chunk)[rank, pos]
    D = pack_all.view(torch.float32).view(world, 2 * chunk)[rank, 2 * m + pos]
    return lims, D, I


class _Sharded:
    """What the sharded indexes share: the rank / world bookkeeping and the packed exchange buffers."""

    def __init__(self, engine, device, group=None, force_collectives: bool = False):
        self.engine = engine
        self.device = device
        self.group = group
        self.world = dist.get_world_size(group) if dist.is_initialized() else 1
        self.rank = dist.get_rank(group) if dist.is_initialized() else 0
        # one rank normally returns its local result as is; with force_collectives (an initialised process
        # group required) it takes the all-gather + merge route of the multi-rank path all the same
        self.exchange = self.world > 1 or (force_collectives and dist.is_initialized())
        self._bufs = {}

    def _buffers(self, nq, k):
        key = (nq, k)
        if key not in self._bufs:
            nk = nq * k
            chunk = nk + (nk + 1) // 2                       # int64 words: ids, then float32 scores
            pack = torch.zeros(chunk, dtype=torch.int64, device=self.device)
            pack_all = torch.zeros(self.world * chunk, dtype=torch.int64, device=self.device)
            I = pack[:nk].view(nq, k)
            D = pack[nk:].view(torch.float32)[:nk].view(nq, k)
            status = torch.zeros(nq, dtype=torch.int32, device=self.device)
            Do = torch.empty((nq, k), dtype=torch.float32, device=self.device)
            Io = torch.empty((nq, k), dtype=torch.int64, device=self.device)
            self._bufs[key] = (chunk, pack, pack_all, D, I, status, Do, Io)
        return self._bufs[key]


class ShardedFlatIndex(_Sharded):
    """``index.search(q, k)`` / ``index.range_search(q, radius)`` over a corpus row-sharded across ``dist`` ranks.

    ``engine.local_search`` must write this rank's exact top-k with GLOBAL ids (id_offset =
    first row of the shard).  Every rank returns the full merged result.  An engine with ``ascending`` set
    (L2) orders by (distance asc, id asc) and pads with (+FLT_MAX, -1).
    """

    def __init__(self, engine, device, group=None, force_collectives: bool = False):
        super().__init__(engine, device, group, force_collectives)
        self.ascending = bool(getattr(engine, "ascending", False))

    def _merge(self, pack_all, shards, nq, k):
        """k-way merge of ``shards`` gathered packs (``pack_all``) into this index's (Do, Io) buffers.  The packs of
        an ascending metric hold -distance (``_pack_for_exchange`` negated them; the padding became the merge's own
        (-FLT_MAX, -1)), so the merged scores are negated back."""
        chunk, _, _, _, _, _, Do, Io = self._buffers(nq, k)
        self.engine.merge(pack_all, chunk, shards, nq, k, Do, Io)
        if self.ascending:
            Do.neg_()
        return Do, Io

    def _pack_for_exchange(self, nq, k):
        """The pack holding this rank's local result, in the form the merge orders: an ascending metric's distances
        negated in place (exact; the next local search rewrites the pack)."""
        _, pack, _, D, _, _, _, _ = self._buffers(nq, k)
        if self.ascending:
            D.neg_()
        return pack

    def _exchange(self, nq, k):
        pack_all = self._buffers(nq, k)[2]
        dist.all_gather_into_tensor(pack_all, self._pack_for_exchange(nq, k), group=self.group)
        return self._merge(pack_all, self.world, nq, k)

    def search_async(self, q, k):
        """Enqueue local search -> all-gather -> merge; no host sync.  Returns (D, I, status):
        status is this rank's per-query "proven exact" vector (0 = proven)."""
        nq = q.shape[0]
        _, _, _, D, I, status, _, _ = self._buffers(nq, k)
        self.engine.local_search(q, k, D, I, status)
        if not self.exchange:
            return D, I, status
        Do, Io = self._exchange(nq, k)
        return Do, Io, status

    def search(self, q, k):
        """Exact search: re-runs locally unproven queries exhaustively before the exchange."""
        nq = q.shape[0]
        _, _, _, D, I, status, _, _ = self._buffers(nq, k)
        self.engine.local_search(q, k, D, I, status)
        self.engine.fix_unproven(q, k, D, I, status)
        if not self.exchange:
            return D, I
        return self._exchange(nq, k)

    def range_search(self, q, radius):
        """Exact range search -> (lims int64 [nq + 1], D float32, I int64) of the WHOLE corpus on every rank, global
        ids ascending per query (the contract of ``FlatIndex.range_search_device``); ``radius`` a scalar or one value
        per query.  Two all-gathers -- the per-query counts, then the (ids | scores) payload padded to the largest
        rank's total -- with one host read in between to size the payload."""
        lims, D, I = self.engine.local_range_search(q, radius)
        if not self.exchange:
            return lims, D, I
        nq = q.shape[0]
        counts = (lims[1:] - lims[:-1]).contiguous()
        counts_all = torch.empty(self.world * nq, dtype=torch.int64, device=self.device)
        dist.all_gather_into_tensor(counts_all, counts, group=self.group)
        counts_all = counts_all.view(self.world, nq)
        totals = counts_all.sum(1).tolist()                  # the one host read
        m, total = max(totals), sum(totals)
        pack_all = torch.empty(self.world * range_chunk_words(m), dtype=torch.int64, device=self.device)
        if m:
            dist.all_gather_into_tensor(pack_all, pack_range(D, I, m), group=self.group)
        return assemble_range(counts_all, pack_all, m, total)


class ShardedBinaryIndex(_Sharded):
    """``BinaryFlatIndex.search(codes, k) -> (D int32, I int64)`` over codes row-sharded across ``dist`` ranks:
    Hamming distance ascending, ties by ascending id, padding (0x7fffffff, -1); every rank returns the full result.

    ``engine.local_search(codes, k)`` returns this rank's result with GLOBAL ids.  The distances cross the exchange
    as -float32(distance) -- exact, a distance is at most 2048 < 2^24 -- and the padding as -FLT_MAX, which is what
    ``sss_topk_merge`` orders and pads with; the merged block is converted back."""

    def _pack_local(self, codes, k):
        """Local search, written into the exchange pack in the form the merge orders; returns the pack."""
        nq = codes.shape[0]
        _, pack, _, Df, If, _, _, _ = self._buffers(nq, k)
        D, I = self.engine.local_search(codes, k)
        If.copy_(I)
        Df.copy_(D).neg_().masked_fill_(I < 0, -FLT_MAX)
        return pack

    def _merge(self, pack_all, shards, nq, k):
        """k-way merge of ``shards`` gathered packs, converted back to (int32 distance, id) with the index's padding."""
        chunk, _, _, _, _, _, Do, Io = self._buffers(nq, k)
        self.engine.merge(pack_all, chunk, shards, nq, k, Do, Io)
        pad = Io < 0
        return Do.neg().masked_fill_(pad, 0.0).to(torch.int32).masked_fill_(pad, HAMMING_PAD), Io

    def search(self, codes, k):
        k = int(k)
        if not self.exchange:
            return self.engine.local_search(codes, k)
        nq = codes.shape[0]
        pack_all = self._buffers(nq, k)[2]
        dist.all_gather_into_tensor(pack_all, self._pack_local(codes, k), group=self.group)
        return self._merge(pack_all, self.world, nq, k)


class ShardedSparseIndex(_Sharded):
    """``SparseSessionIndex.search(vectors, k) -> (D float32, I int64)`` over session vectors row-sharded across ``dist``
    ranks: (score desc, id asc), padding (-FLT_MAX, -1) -- already the order and the padding of ``sss_topk_merge``, so the
    local result crosses the exchange as it is.  ``engine.local_search(vectors, k, D, I)`` writes this rank's result with
    GLOBAL ids; every rank returns the full merged result."""

    def search(self, vectors, k):
        k = int(k)
        nq = len(vectors)
        chunk, pack, pack_all, D, I, _, Do, Io = self._buffers(nq, k)
        self.engine.local_search(vectors, k, D, I)
        if not self.exchange:
            return D, I
        dist.all_gather_into_tensor(pack_all, pack, group=self.group)
        self.engine.merge(pack_all, chunk, self.world, nq, k, Do, Io)
        return Do, Io


INT64_MAX = 2 ** 63 - 1


class ShardedJaccardIndex(ShardedSparseIndex):
    """``JaccardIndex`` over item sets row-sharded across ``dist`` ranks.  ``search`` is ``ShardedSparseIndex``'s: the local
    result is already in the order and the padding of ``sss_topk_merge``.  ``bands(sets, edges) -> (counts, first)`` sums the
    shards' counts (``all_reduce`` SUM) and takes the lowest of their first rows (``all_reduce`` MIN, a band a shard does not
    hold crossing as INT64_MAX in place of its -1); ``engine.local_bands`` returns this rank's pair with GLOBAL ids.  Every
    rank returns the full result."""

    def bands(self, sets, edges):
        counts, first = self.engine.local_bands(sets, edges)
        if not self.exchange:
            return counts, first
        counts = counts.clone()
        first = torch.where(first < 0, torch.full_like(first, INT64_MAX), first)
        dist.all_reduce(counts, op=dist.ReduceOp.SUM, group=self.group)
        dist.all_reduce(first, op=dist.ReduceOp.MIN, group=self.group)
        return counts, torch.where(first == INT64_MAX, torch.full_like(first, -1), first)


class ShardedProductTypeIndex(ShardedJaccardIndex):
    """``ProductTypeIndex`` over type bags row-sharded across ``dist`` ranks, over a ``ProductTypeEngine``:
    ``ShardedJaccardIndex``'s shape -- top-k merged by ``sss_topk_merge``, bands by the all-reduce SUM and MIN."""
