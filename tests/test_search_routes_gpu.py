"""Routes of the search that the rest of the suite does not pin: scan plans with 8 to 15 active splits (large query
batches, small corpora), the exhaustive path's compaction pre-pass for 500 < k <= 1024, and the threshold rung at
selection sizes on wave and workgroup boundaries, and one small search per scan family ``FlatIndex`` calls by parameter
name.  Ids and scores are compared with the oracle by array_equal."""
import functools

import numpy as np
import pytest
import torch

from oracle import search_ref as sr

pytestmark = pytest.mark.gpu


def _unit(rng, n, d):
    return sr.normalize(rng.standard_normal((n, d)).astype(np.float32)).astype(np.float32)


def _boot_expired(reset):
    from sessionsimilaritysearch_amd import _lib
    v = _lib.lib().sss_scan_boot_expired(1 if reset else 0)
    assert v >= 0
    return v


@functools.lru_cache(maxsize=None)
def _big(n, d, seed):
    """n random unit rows (generated and normalised on the device), host copy for the oracle."""
    from sessionsimilaritysearch_amd.index import normalize
    g = torch.Generator(device="cuda").manual_seed(seed)
    x = torch.randn((n, d), generator=g, device="cuda", dtype=torch.float32)
    return normalize(x).cpu().numpy()


# ------------------------------------------------------------------------------- plans with S = 8 splits
@functools.lru_cache(maxsize=None)
def _s8_index(cuda_index, scan):
    from sessionsimilaritysearch_amd.index import FlatIndex
    idx = FlatIndex(128, "ip", torch.device("cuda", cuda_index), scan=scan)
    idx.add(_big(1_000_000, 128, 11))
    return idx


def _check_batch(idx, q, k, Dr_q, Ir_q, picks, chunk=1024):
    _boot_expired(True)
    D, I = idx.search(q, k)
    expired = _boot_expired(False)
    assert expired <= 32, expired                        # the shared threshold existed: no wave sat out its bootstrap wait
    for lo in range(0, q.shape[0], chunk):
        Dc, Ic = idx.search(q[lo:lo + chunk], k)
        assert np.array_equal(Ic, I[lo:lo + chunk]) and np.array_equal(Dc, D[lo:lo + chunk]), lo
    assert np.array_equal(I[picks], Ir_q[:, :k]) and np.array_equal(D[picks], Dr_q[:, :k])


@pytest.mark.parametrize("scan", ["f32", "split", "f16"])
@pytest.mark.parametrize("nq", [4097, 5000])
def test_large_batches_take_eight_split_plans(cuda, nq, scan):
    """More than 4096 queries per call: 17+ query groups leave 8 corpus splits, so with k <= 16 only 8 of the 16
    threshold classes publish.  Every query equals the same query searched in 1024-query calls; 16 (the first and
    the last workgroup's) equal the oracle."""
    c = _big(1_000_000, 128, 11)
    q = _unit(np.random.default_rng(nq), nq, 128)
    picks = np.r_[0:8, nq - 8:nq]
    Dr, Ir = sr.search_exact(q[picks], c, 16)
    idx = _s8_index(cuda.index if cuda.index is not None else 0, scan)
    for k in (1, 10, 14, 16):
        _check_batch(idx, q, k, Dr, Ir, picks)
        assert idx.last_scan == scan


def test_bf16_index_d512_eight_split_plan(cuda):
    """1024-byte rows: 128 queries per workgroup, so 2100 queries already make 17 groups and 8 splits."""
    from sessionsimilaritysearch_amd.index import FlatIndex
    c = torch.from_numpy(_big(100_000, 512, 12)).to(torch.bfloat16).float().numpy()
    q = torch.from_numpy(_unit(np.random.default_rng(2100), 2100, 512)).to(torch.bfloat16).float().numpy()
    picks = np.r_[0:8, 2100 - 8:2100]
    Dr, Ir = sr.search_exact(q[picks], c, 16)
    idx = FlatIndex(512, "ip", cuda, dtype="bf16")
    idx.add(c)
    for k in (10, 16):
        _check_batch(idx, q, k, Dr, Ir, picks)
        assert idx.last_scan == "native"


# n chosen from make_plan_for: one query group, 64-row tiles of 512-byte rows, S = 16 (n < 1536) or 24 splits;
# ceil(ceil(n / 64) / ceil(tiles / S)) active splits = 9, 10, 11, 12, 13, 14, 15
FEW_SPLITS_N = [1040, 1216, 1344, 1472, 1600, 1728, 1856]


@pytest.mark.parametrize("scan", ["f32", "split", "f16"])
@pytest.mark.parametrize("n", FEW_SPLITS_N)
def test_small_corpora_with_fewer_than_sixteen_active_splits(cuda, n, scan):
    from sessionsimilaritysearch_amd.index import FlatIndex
    rng = np.random.default_rng(n)
    c, q = _unit(rng, n, 128), _unit(rng, 200, 128)
    idx = FlatIndex(128, "ip", cuda, scan=scan)
    idx.add(c)
    Dr, Ir = sr.search_exact(q, c, 16)
    for k in (1, 7, 10, 14, 16):
        _boot_expired(True)
        D, I = idx.search(q, k)
        expired = _boot_expired(False)
        assert idx.last_scan == scan
        assert np.array_equal(I, Ir[:, :k]) and np.array_equal(D, Dr[:, :k]), k
        assert expired <= 32, (k, expired)


# ------------------------------------------------------------------------------- exhaustive path, 500 < k <= 1024
@pytest.mark.parametrize("k", [501, 1000, 1024])
@pytest.mark.parametrize("n", [262143, 262144, 1_000_000, 1_500_000])
def test_exhaustive_large_k_random_rows(cuda, n, k):
    """k beyond the fused path: the exhaustive kernels, with the compaction pre-pass from n = 262144 on."""
    from sessionsimilaritysearch_amd.index import FlatIndex
    c = _big(1_500_000, 128, 13)[:n]
    q = _unit(np.random.default_rng(k), 8, 128)
    idx = FlatIndex(128, "ip", cuda)
    idx.add(c)
    D, I = idx.search(q, k)
    assert idx.last_fallback_queries == 8
    Dr, Ir = sr.search_exact(q, c, k)
    assert np.array_equal(I, Ir) and np.array_equal(D, Dr)


@pytest.mark.parametrize("n,k", [(262144, 1000), (1_500_000, 1024)])
def test_exhaustive_large_k_sorted_corpus_overflows_the_compaction(cuda, n, k):
    """Rows in ascending score order for query 0: the head sample sees only the lowest scores, every row survives the
    pre-pass, the survivors overflow its capacity and the select reads the full score row."""
    from sessionsimilaritysearch_amd.index import FlatIndex
    c = _big(1_500_000, 128, 13)[:n]
    q = _unit(np.random.default_rng(5), 6, 128)
    c = np.ascontiguousarray(c[np.argsort(c @ q[0], kind="stable")])
    idx = FlatIndex(128, "ip", cuda)
    idx.add(c)
    D, I = idx.search(q, k)
    Dr, Ir = sr.search_exact(q, c, k)
    assert np.array_equal(I, Ir) and np.array_equal(D, Dr)


def test_exhaustive_large_k_tied_group_straddles_rank_k(cuda):
    """2000 copies of the row that ranks 700th for query 0: rank k = 1000 falls inside the tied group, which is cut by
    ascending id."""
    from sessionsimilaritysearch_amd.index import FlatIndex
    rng = np.random.default_rng(17)
    c = _big(1_000_000, 128, 14).copy()
    q = _unit(rng, 6, 128)
    row = c[np.argsort(-(c @ q[0]), kind="stable")[700]].copy()
    c[rng.choice(c.shape[0], 2000, replace=False)] = row
    idx = FlatIndex(128, "ip", cuda)
    idx.add(c)
    D, I = idx.search(q, 1000)
    Dr, Ir = sr.search_exact(q, c, 1000)
    assert np.array_equal(I, Ir) and np.array_equal(D, Dr)
    assert (Dr[0] == Dr[0, 999]).sum() > 1 and Dr[0, 0] > Dr[0, 999]      # the group really straddles rank k for query 0


def test_exhaustive_large_k_l2(cuda):
    from sessionsimilaritysearch_amd.index import build_index
    rng = np.random.default_rng(18)
    c = _big(262144, 128, 15) * np.float32(3.0)
    q = rng.standard_normal((3, 128)).astype(np.float32)
    D, I = build_index(c, "l2", cuda).search(q, 1024)
    Dr, Ir = sr.build_index(c, "l2").search(q, 1024)
    assert np.array_equal(I, Ir) and np.array_equal(D, Dr)


@pytest.mark.parametrize("k", [10, 600])
def test_exhaustive_generic_scorer_at_the_reference_width(cuda, k):
    """d = 200 (the reference's emb_len): no fused scan, the generic k_exact_scores; 300k rows take the compaction."""
    from sessionsimilaritysearch_amd.index import FlatIndex
    c = _big(300_000, 200, 16)
    q = _unit(np.random.default_rng(200 + k), 6, 200)
    idx = FlatIndex(200, "ip", cuda)
    idx.add(c)
    D, I = idx.search(q, k)
    assert idx.last_fallback_queries == 6
    Dr, Ir = sr.search_exact(q, c, k)
    assert np.array_equal(I, Ir) and np.array_equal(D, Dr)


# ------------------------------------------------------------------------------- threshold rung: selection sizes
@functools.lru_cache(maxsize=None)
def _rung_data(d):
    rng = np.random.default_rng(400 + d)
    q, c = _unit(rng, 300, d), _unit(rng, 20000, d)
    Dr, Ir = sr.search_exact(q, c, 10)
    sample = np.sort(rng.choice(c.shape[0], c.shape[0] // 30, replace=False))
    Ds, _ = sr.search_exact(q, c[sample], 10)
    return q, c, Dr, Ir, Ds


RUNG_CASES = [(m, 128, s) for m in ("f16", "split", "f32") for s in (1, 31, 32, 33, 63, 64, 65, 96, 255, 256, 257)] + \
             [("f16", 512, s) for s in (127, 128, 129)]


@pytest.mark.parametrize("mode,d,nsel", RUNG_CASES)
def test_threshold_rung_selection_sizes(cuda, mode, d, nsel):
    """sss_ip_topk_threshold on `nsel` scattered queries of 300: the threshold form's workgroups hold 256 queries (128
    for 1024-byte rows) in waves of 32; padded slots and empty waves must neither write nor lose a row."""
    from sessionsimilaritysearch_amd.index import FlatIndex
    q, c, Dr, Ir, Ds = _rung_data(d)
    nq, k = q.shape[0], 10
    idx = FlatIndex(d, "ip", cuda, scan=mode)
    idx.add(c)
    rows = np.sort(np.random.default_rng(nsel).choice(nq, nsel, replace=False))
    tq = torch.from_numpy(q).to(cuda)
    D = torch.from_numpy(Ds).to(cuda).contiguous()
    I = torch.full((nq, k), -7, dtype=torch.int64, device=cuda)
    status = torch.ones(nq, dtype=torch.int32, device=cuda)
    left = idx.search_threshold(tq, k, D, I, status, torch.from_numpy(rows).to(cuda))
    assert idx.rung_scan() == mode
    done = (status == 0).cpu().numpy()
    sel = np.zeros(nq, bool)
    sel[rows] = True
    assert not done[~sel].any() and done.sum() >= nsel * 0.5 and left.numel() == nsel - done.sum()
    Ic, Dc = I.cpu().numpy(), D.cpu().numpy()
    assert np.array_equal(Ic[done], Ir[done]) and np.array_equal(Dc[done], Dr[done])
    assert (Ic[~done] == -7).all() and np.array_equal(Dc[~sel], Ds[~sel])


# ------------------------------------------------------------------------------- every scan family once, small
# (family of index._TOPK / _THRESHOLD, metric, d, FlatIndex arguments, the scan it must run on)
FAMILY_CASES = [("ip", "ip", 64, dict(scan="f32"), "f32"), ("ip_split", "ip", 128, dict(scan="split"), "split"),
                ("ip_f16", "ip", 128, dict(scan="f16"), "f16"), ("l2", "l2", 64, dict(scan="f32"), "f32"),
                ("pad", "ip", 200, dict(scan="f16", pad_scan=True), "f16"), ("long_ip", "ip", 320, {}, "long"),
                ("long_l2", "l2", 320, {}, "long")]
FAMILY_CASES = [(*c, False) for c in FAMILY_CASES] + [(*c, True) for c in FAMILY_CASES if c[0] in ("ip", "l2", "pad")]


@pytest.mark.parametrize("family,metric,d,kwargs,scan,rung", FAMILY_CASES, ids=[f"{c[0]}-{'rung' if c[-1] else 'topk'}" for c in FAMILY_CASES])
def test_every_scan_family_is_called_with_its_own_arguments(cuda, family, metric, d, kwargs, scan, rung):
    """One search per entry point FlatIndex calls by parameter name, at the family's smallest width, with nq != nsel and
    an id offset so that no two integer arguments can be swapped unseen.  ``rung``: 32 copies of each query in the corpus
    (the construction of test_f16_index_gpu.test_duplicates_at_the_kth_place_go_through_the_rung) tie across rank k, which
    no scan can prove: the family's threshold entry point resolves them."""
    from sessionsimilaritysearch_amd.index import FlatIndex
    rng = np.random.default_rng(500 + d)
    n, nq, k, offset = 2000, 8, 10, 7
    q, c = _unit(rng, nq, d), _unit(rng, n, d)
    if rung:
        for j in range(nq):
            c[rng.choice(n, 32, replace=False)] = q[j]
    if metric == "l2":
        Dr, Ir = sr.topk_from_scores(sr.canonical_l2(q, c), k + 1, offset, largest=False)
    else:
        Dr, Ir = sr.search_exact(q, c, k + 1, offset)
    assert (Dr[:, k - 1] == Dr[:, k]).all() if rung else (Dr[:, k - 1] != Dr[:, k]).all()
    idx = FlatIndex(d, metric, cuda, **kwargs)
    idx.add(c)
    idx.id_offset = offset
    D, I = idx.search(q, k)
    assert idx.last_scan == scan and family in (idx._family(scan), f"{idx._family(scan)}_{scan}")
    assert np.array_equal(I, Ir[:, :k]) and np.array_equal(D, Dr[:, :k])
    if rung:
        assert idx.last_rescan_queries > 0 and idx.last_fallback_queries == 0
