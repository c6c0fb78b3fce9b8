"""Row sharding of every index kind on the GPU: the L2 metric, shapes without a fused scan, range_search and the
binary (Hamming) index.

One GPU is all a test session has, so the multi-shard part is an in-process sweep: the S shard indexes live on the one
device with their id_offsets, the real HipEngine / HammingEngine run the local searches, the packs are stacked exactly
as the all-gather lays them out (rank-major blocks of `chunk` words) and the product's own merge / range assembly
turns them into the result -- which must be array_equal to the single unsharded index AND to the CPU oracle for
S in {1, 2, 4, 8} (a shard-count sweep returns identical (D, I)).  The collectives themselves run
over RCCL with one rank in a fresh child process (tests/helpers/rccl_one_rank_kinds.py)."""
import json
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle import search_ref as sr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SWEEP = (1, 2, 4, 8)


def _corpus(n, d, nq, seed, unit):
    rng = np.random.default_rng(seed)
    c = rng.standard_normal((n, d)).astype(np.float32)
    q = rng.standard_normal((nq, d)).astype(np.float32)
    if unit:
        c, q = sr.normalize(c), sr.normalize(q)
    c[1] = c[n - 2]                                          # an exact tie between the first and the last shard ...
    q[0] = c[1]                                              # ... at the head of query 0's list
    return c, q


def _flat_shards(c, metric, S, dev):
    from sessionsimilaritysearch_amd.distributed import HipEngine, ShardedFlatIndex, shard_range
    from sessionsimilaritysearch_amd.index import FlatIndex
    out = []
    for s in range(S):
        lo, hi = shard_range(c.shape[0], S, s)
        out.append(ShardedFlatIndex(HipEngine(FlatIndex(c.shape[1], metric, dev).adopt(c[lo:hi], id_offset=lo)), dev))
    return out


def _sweep_search(c, q, k, metric, S, dev):
    """search() of S shards without a process group: local search + fix, pack, stack, merge."""
    shards = _flat_shards(c, metric, S, dev)
    nq = q.shape[0]
    chunk = shards[0]._buffers(nq, k)[0]
    stacked = torch.empty(S * chunk, dtype=torch.int64, device=dev)
    for s, sh in enumerate(shards):
        _, _, _, D, I, status, _, _ = sh._buffers(nq, k)
        sh.engine.local_search(q, k, D, I, status)
        sh.engine.fix_unproven(q, k, D, I, status)
        stacked[s * chunk:(s + 1) * chunk] = sh._pack_for_exchange(nq, k)
    D, I = shards[0]._merge(stacked, S, nq, k)
    return D.cpu().numpy(), I.cpu().numpy()


def _check_search_sweep(cuda, metric, n, d, nq, k, unit, expect_fused):
    from sessionsimilaritysearch_amd.index import FlatIndex
    c_h, q_h = _corpus(n, d, nq, 31, unit)
    c, q = torch.from_numpy(c_h).to(cuda), torch.from_numpy(q_h).to(cuda)
    whole = FlatIndex(d, metric, cuda).adopt(c)
    assert whole.fused_ok(k) == expect_fused
    D1, I1 = (t.cpu().numpy() for t in whole.search_device(q, k))
    if metric == "l2":
        Dr, Ir = sr.topk_from_scores(sr.canonical_l2(q_h, c_h), k, largest=False)
    else:
        Dr, Ir = sr.search_exact(q_h, c_h, k)
    assert np.array_equal(I1, Ir) and np.array_equal(D1, Dr)
    assert Ir[0, 0] == 1 and Ir[0, 1] == n - 2 and Dr[0, 0] == Dr[0, 1]            # the tie is there, lower id first
    for S in SWEEP:
        D, I = _sweep_search(c, q, k, metric, S, cuda)
        assert np.array_equal(I, Ir), (S, int((I != Ir).sum()))
        assert np.array_equal(D, Dr), (S, int((D != Dr).sum()))


@pytest.mark.gpu
def test_shard_sweep_l2_d128(cuda):
    _check_search_sweep(cuda, "l2", 20000, 128, 64, 10, unit=False, expect_fused=False)


@pytest.mark.gpu
def test_shard_sweep_ip_d200_has_no_fused_scan(cuda):
    _check_search_sweep(cuda, "ip", 20000, 200, 64, 10, unit=True, expect_fused=False)


@pytest.mark.gpu
def test_shard_sweep_ip_d128_k600_beyond_the_fused_k(cuda):
    _check_search_sweep(cuda, "ip", 20000, 128, 48, 600, unit=True, expect_fused=False)


@pytest.mark.gpu
def test_sweep_with_an_empty_shard_and_padding_l2(cuda):
    """3 rows over 4 shards, k = 10: an empty shard, and padding on both sides of the negation."""
    rng = np.random.default_rng(2)
    c_h, q_h = rng.standard_normal((3, 128)).astype(np.float32), rng.standard_normal((5, 128)).astype(np.float32)
    c, q = torch.from_numpy(c_h).to(cuda), torch.from_numpy(q_h).to(cuda)
    Dr, Ir = sr.topk_from_scores(sr.canonical_l2(q_h, c_h), 10, largest=False)
    D, I = _sweep_search(c, q, 10, "l2", 4, cuda)
    assert np.array_equal(I, Ir) and np.array_equal(D, Dr)
    assert (I[:, 3:] == -1).all() and (D[:, 3:] == np.float32(3.4028234663852886e38)).all()


# --------------------------------------------------------------------------------------------- range search
def _kept(scores, rad, ascending):
    mask = scores < rad[:, None] if ascending else scores > rad[:, None]
    rows, cols = np.nonzero(mask)
    lims = np.zeros(scores.shape[0] + 1, np.int64)
    np.cumsum(mask.sum(1), out=lims[1:])
    return lims, np.ascontiguousarray(scores[rows, cols], np.float32), cols.astype(np.int64)


def _sweep_range(c, q, rad, metric, S, dev):
    """range_search() of S shards without a process group: local results, the counts / payload blocks laid out as
    the two all-gathers deliver them, the product's device-side assembly."""
    from sessionsimilaritysearch_amd.distributed import assemble_range, pack_range
    local = [sh.engine.local_range_search(q, rad) for sh in _flat_shards(c, metric, S, dev)]
    counts_all = torch.stack([lims[1:] - lims[:-1] for lims, _, _ in local]).contiguous()
    totals = counts_all.sum(1).tolist()
    m, total = max(totals), sum(totals)
    pack_all = torch.cat([pack_range(D, I, m) for _, D, I in local])
    return tuple(t.cpu().numpy() for t in assemble_range(counts_all, pack_all, m, total))


@pytest.mark.gpu
@pytest.mark.parametrize("metric", ["ip", "l2"])
def test_shard_sweep_range_search(cuda, metric):
    from sessionsimilaritysearch_amd.index import FlatIndex
    n, d, nq = 20000, 128, 64
    c_h, q_h = _corpus(n, d, nq, 37, unit=True)
    s = sr.canonical_l2(q_h, c_h) if metric == "l2" else sr.canonical_scores(q_h, c_h)
    asc = metric == "l2"
    part = np.sort(s, axis=1)
    rad = (part[:, 25] if asc else part[:, n - 26]).astype(np.float32).copy()          # 25 hits a query ...
    rad[2] = s.min() - 1 if asc else s.max() + 1                                       # ... none for query 2 ...
    rad[3] = s.max() + 1 if asc else s.min() - 1                                       # ... and every row for query 3
    lims_r, D_r, I_r = _kept(s, rad, asc)
    assert lims_r[3] == lims_r[2] and lims_r[4] - lims_r[3] == n and lims_r[1] == 25
    c, q, trad = torch.from_numpy(c_h).to(cuda), torch.from_numpy(q_h).to(cuda), torch.from_numpy(rad).to(cuda)
    got = tuple(t.cpu().numpy() for t in FlatIndex(d, metric, cuda).adopt(c).range_search_device(q, trad))
    assert np.array_equal(got[0], lims_r) and np.array_equal(got[2], I_r) and np.array_equal(got[1], D_r)
    for S in SWEEP:
        lims, D, I = _sweep_range(c, q, trad, metric, S, cuda)
        assert np.array_equal(lims, lims_r), S
        assert np.array_equal(I, I_r), (S, int((I != I_r).sum()))
        assert np.array_equal(D, D_r), (S, int((D != D_r).sum()))


# -------------------------------------------------------------------------------------------------- Hamming
def _sweep_hamming(codes, q, k, nbits, S, dev):
    from sessionsimilaritysearch_amd.distributed import HammingEngine, ShardedBinaryIndex, shard_range
    from sessionsimilaritysearch_amd.index import BinaryFlatIndex
    nq = q.shape[0]
    shards = []
    for s in range(S):
        lo, hi = shard_range(codes.shape[0], S, s)
        index = BinaryFlatIndex(nbits, dev)
        index.add(codes[lo:hi])
        index.id_offset = lo
        shards.append(ShardedBinaryIndex(HammingEngine(index), dev))
    chunk = shards[0]._buffers(nq, k)[0]
    stacked = torch.empty(S * chunk, dtype=torch.int64, device=dev)
    for s, sh in enumerate(shards):
        stacked[s * chunk:(s + 1) * chunk] = sh._pack_local(q, k)
    D, I = shards[0]._merge(stacked, S, nq, k)
    return D.cpu().numpy(), I.cpu().numpy()


@pytest.mark.gpu
@pytest.mark.parametrize("nbits,k", [(256, 10), (256, 200), (1600, 10), (1600, 200)])
def test_shard_sweep_hamming(cuda, nbits, k):
    """k = 200 is inside the fused capacity of the whole index (20000 rows) and beyond that of a 2500-row shard, so at
    8 shards the local searches take the exhaustive route.  Random codes tie in distance all over the corpus."""
    from sessionsimilaritysearch_amd.index import BinaryFlatIndex
    n, nq = 20000, 48
    rng = np.random.default_rng(41)
    c_h = rng.integers(0, 256, (n, nbits // 8), dtype=np.uint8)
    c_h[1] = c_h[n - 2]
    q_h = rng.integers(0, 256, (nq, nbits // 8), dtype=np.uint8)
    q_h[0] = c_h[1]
    Dr, Ir = sr.hamming_search(q_h, c_h, k)
    assert Ir[0, 0] == 1 and Ir[0, 1] == n - 2 and (np.diff(Dr, axis=1) == 0).any()
    c, q = torch.from_numpy(c_h).to(cuda), torch.from_numpy(q_h).to(cuda)
    whole = BinaryFlatIndex(nbits, cuda)
    whole.add(c)
    D1, I1 = (t.cpu().numpy() for t in whole.search(q, k))
    assert np.array_equal(I1, Ir) and np.array_equal(D1, Dr)
    for S in SWEEP:
        D, I = _sweep_hamming(c, q, k, nbits, S, cuda)
        assert D.dtype == np.int32 and I.dtype == np.int64
        assert np.array_equal(I, Ir), (S, int((I != Ir).sum()))
        assert np.array_equal(D, Dr), (S, int((D != Dr).sum()))


# ------------------------------------------------------------------------------ behaviour that must not change
@pytest.mark.gpu
def test_fused_shape_search_async_is_unchanged_and_does_not_sync(cuda):
    """An inner-product index of a fused shape: search_async is still local_search = search_fused into the pack (same
    D, I, status as a direct call), it bumps the engine's device-side unproven counter by the status count, and it
    enqueues without a host sync (torch's sync debug mode raises on one)."""
    from sessionsimilaritysearch_amd.distributed import HipEngine, ShardedFlatIndex
    from sessionsimilaritysearch_amd.index import FlatIndex
    n, d, nq, k = 50000, 128, 256, 10
    c_h, q_h = _corpus(n, d, nq, 43, unit=True)
    c, q = torch.from_numpy(c_h).to(cuda), torch.from_numpy(q_h).to(cuda)
    index = FlatIndex(d, "ip", cuda).adopt(c, id_offset=7)
    assert index.fused_ok(k)
    eng = HipEngine(index)
    assert eng.ascending is False
    sh = ShardedFlatIndex(eng, cuda)
    sh.search_async(q, k)                                    # builds the scan image and the buffers (that part may sync)
    torch.cuda.synchronize()
    before = int(eng.unproven.item())
    torch.cuda.set_sync_debug_mode("error")
    try:
        D, I, status = sh.search_async(q, k)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    D, I, status = D.clone(), I.clone(), status.clone()
    Df, If, stf = index.search_fused(q, k)
    torch.cuda.synchronize()
    assert torch.equal(I, If) and torch.equal(D, Df) and torch.equal(status, stf)
    assert int(eng.unproven.item()) - before == int((status != 0).sum())
    Dr, Ir = sr.search_exact(q_h, c_h, k, id_offset=7)
    D2, I2 = sh.search(q, k)
    assert np.array_equal(I2.cpu().numpy(), Ir) and np.array_equal(D2.cpu().numpy(), Dr)


# ------------------------------------------------------------------------------------------- one-rank RCCL
def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


@pytest.mark.gpu
def test_rccl_one_rank_exchange_route_of_every_kind(cuda):
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", HSA_ENABLE_IPC_MODE_LEGACY="0")
    res = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "helpers", "rccl_one_rank_kinds.py"), str(_free_port())],
                         capture_output=True, text=True, timeout=600, env=env, cwd=ROOT)
    lines = [ln for ln in res.stdout.splitlines() if ln.startswith("{")]
    assert res.returncode == 0 and lines, f"child failed (rc {res.returncode}):\n{res.stdout[-2000:]}\n{res.stderr[-4000:]}"
    out = json.loads(lines[-1])
    assert out["ok"] and out["backend"] == "nccl" and out["world"] == 1
    for kind in ("l2", "l2_async", "ip_d200", "range_ip", "range_l2", "range_scalar", "range_empty", "hamming256", "hamming1600"):
        assert out["checks"][kind + "_vs_unsharded"] and out["checks"][kind + "_vs_oracle"], kind
