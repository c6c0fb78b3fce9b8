"""L2 top-k on the matrix-core scans: ``FlatIndex(d, "l2")`` of a float32 index takes the candidate scans
(``l2_scan_for``) instead of the exhaustive kernels, and whatever route serves a query -- scan + proof, threshold rung,
exhaustive kernels -- ids and distances equal the oracle's, ``sr.topk_from_scores(sr.canonical_l2(q, c), k,
largest=False)``, with ``array_equal``.

The two seeded corpora: "gauss" (standard normal rows) and "varnorm" (directions of the same rows, norms log-uniform in
[1/4, 4]).  On "varnorm" the exact inner-product top-10 and the L2 top-10 differ as sets for 300 of 300 queries, so a scan
with a missing, mis-indexed or mis-scaled row bias cannot pass by way of the re-score: its candidates would be the wrong
rows."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

from oracle import search_ref as sr

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import bound_inputs_ref  # noqa: E402

SCANS = ("f32", "split", "f16")
KS = (1, 10, 16, 17, 100, 500)
FLT_MAX = np.float32(3.4028234663852886e38)
_cache = {}


def _data():
    if "data" not in _cache:
        rng = np.random.default_rng(20261017)
        c = rng.standard_normal((20000, 128)).astype(np.float32)
        q = rng.standard_normal((300, 128)).astype(np.float32)
        s = np.exp(rng.uniform(np.log(.25), np.log(4), 20000)).astype(np.float32)
        c2 = (c / np.linalg.norm(c, axis=1, keepdims=True) * s[:, None]).astype(np.float32)
        q2 = (q / np.linalg.norm(q, axis=1, keepdims=True)
              * np.exp(rng.uniform(np.log(.25), np.log(4), 300))[:, None]).astype(np.float32)
        _cache["data"] = {"gauss": (c, q), "varnorm": (c2, q2)}
    return _cache["data"]


def _oracle(q, c, k):
    return sr.topk_from_scores(sr.canonical_l2(q, c), k, largest=False)


def _ref(name, k):
    """The oracle's top-k of a seeded corpus: the top 500 computed once, its prefixes serve every k."""
    key = ("ref", name)
    if key not in _cache:
        c, q = _data()[name]
        _cache[key] = _oracle(q, c, 500)
    D, I = _cache[key]
    return D[:, :k], I[:, :k]


def _index(cuda, name, scan):
    from sessionsimilaritysearch_amd.index import FlatIndex
    key = ("index", name, scan)
    if key not in _cache:
        idx = FlatIndex(128, "l2", cuda, scan=scan)
        idx.add(_data()[name][0])
        _cache[key] = idx
    return _cache[key]


def _equal(got, want):
    D, I = got
    Dr, Ir = want
    assert np.array_equal(I, Ir), int((I != Ir).sum())
    assert np.array_equal(D, Dr), int((D != Dr).sum())


# ------------------------------------------------------------------------------------------- 1. the route is taken
@pytest.mark.gpu
@pytest.mark.parametrize("scan", SCANS)
def test_l2_search_takes_the_scan_route(cuda, scan):
    idx = _index(cuda, "gauss", scan)
    assert idx.l2_scan_for(10) == scan
    _equal(idx.search(_data()["gauss"][1], 10), _ref("gauss", 10))
    assert idx.last_scan == scan and idx.last_fallback_queries == 0
    assert idx.fused_ok(10) is False and idx.scan_for(10) == ""          # those two describe the inner-product path


# ------------------------------------------------------------------------------------------- 2. exact, every scan
@pytest.mark.gpu
@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("scan", SCANS)
@pytest.mark.parametrize("name", ["gauss", "varnorm"])
def test_l2_exact_on_both_corpora(cuda, name, scan, k):
    """k = 1 .. 16: the wave-per-query select (and, on the f16 / split scans, the append form where the plan takes it);
    17 .. 500: lane lists certifying 2 .. 16 rows a class, the sort select."""
    idx = _index(cuda, name, scan)
    _equal(idx.search(_data()[name][1], k), _ref(name, k))
    assert idx.last_scan == scan


# ------------------------------------------------------------------------------------------- 3. unproven cap
@pytest.mark.gpu
@pytest.mark.parametrize("k", [10, 100])
@pytest.mark.parametrize("name,scan", [("gauss", "f32"), ("gauss", "split"), ("varnorm", "f32")])
def test_l2_scan_proves_most_queries(cuda, name, scan, k):
    """The scan may not hand everything to the rung.  None of the 300 queries has an exact-distance gap between rank k
    and rank K2 + 1 below four times the scan's documented bound (medians on "gauss": gap 1.59 against 4 B = 0.066 for
    split and 0.0058 for f32; on "varnorm" with f32: 0.0045 against 0.00015), so the expected count is 0; the cap
    leaves room for threshold-status bits."""
    idx = _index(cuda, name, scan)
    _equal(idx.search(_data()[name][1], k), _ref(name, k))
    print(f"l2 unproven: {name} scan={scan} k={k}: {idx.last_rescan_queries} of 300")
    assert idx.last_rescan_queries <= 30 and idx.last_fallback_queries == 0


@pytest.mark.gpu
def test_l2_auto_escalates_off_f16_on_varnorm(cuda):
    """The f16 scan's bound comes from the LARGEST corpus norm, pessimistic against a near row of small norm: on
    "varnorm" most queries sit inside its window.  No cap there -- it must only be exact -- and scan="auto" must have
    moved this k class off f16 after the search."""
    from sessionsimilaritysearch_amd.index import FlatIndex
    c, q = _data()["varnorm"]
    idx = FlatIndex(128, "l2", cuda)                                      # scan="auto"
    idx.add(c)
    before = idx.l2_scan_for(10)
    assert before == "f16"
    _equal(idx.search(q, 10), _ref("varnorm", 10))
    print(f"l2 unproven: varnorm scan=f16 k=10: {idx.last_rescan_queries} of 300, fallbacks {idx.last_fallback_queries}")
    assert idx.last_scan == "f16" and idx.l2_scan_for(10) != before
    after = idx.l2_scan_for(10)
    _equal(idx.search(q, 10), _ref("varnorm", 10))                        # ... and the scan it moved to is exact too
    assert idx.last_scan == after


# ------------------------------------------------------------------------------------------- 4. shapes
def _small(n, d, nq, seed):
    rng = np.random.default_rng(seed)
    c = (rng.standard_normal((n, d)) * np.exp(rng.uniform(-1, 1, (n, 1)))).astype(np.float32)
    q = (rng.standard_normal((nq, d)) * np.exp(rng.uniform(-1, 1, (nq, 1)))).astype(np.float32)
    return c, q


@pytest.mark.gpu
@pytest.mark.parametrize("scan,d", [("f32", 64), ("f32", 256), ("split", 64), ("split", 256), ("f16", 256), ("f16", 512)])
def test_l2_every_row_size_with_a_kernel(cuda, scan, d):
    """d = 64 / 256 / 512 for each scan that has a kernel there (f32 and split: 64, 128, 256; f16: 128, 256, 512)."""
    from sessionsimilaritysearch_amd.index import FlatIndex
    c, q = _small(3000 + 37, d, 33, d)
    idx = FlatIndex(d, "l2", cuda, scan=scan)
    idx.add(c)
    assert idx.l2_scan_for(10) == scan
    for k in (10, 100):
        _equal(idx.search(q, k), _oracle(q, c, k))
        assert idx.last_scan == scan and idx.last_fallback_queries == 0


@pytest.mark.gpu
@pytest.mark.parametrize("n", [37, 63, 64, 65, 4096 + 37])
@pytest.mark.parametrize("scan", SCANS)
def test_l2_tail_tile_and_padding(cuda, scan, n):
    """The last tile carries rows at and beyond n (their biases are never read, their scores never emitted), one row
    more or less than a 64-row step; k = 100 > n pads with (+FLT_MAX, -1)."""
    from sessionsimilaritysearch_amd.index import FlatIndex
    c, q = _small(n, 128, 33, n)
    idx = FlatIndex(128, "l2", cuda, scan=scan)
    idx.add(c)
    for k in (10, 100):
        D, I = idx.search(q, k)
        _equal((D, I), _oracle(q, c, k))
        assert idx.last_scan == scan
        if n < k:
            assert (I[:, n:] == -1).all() and (D[:, n:] == FLT_MAX).all() and (I[:, :n] >= 0).all()


@pytest.mark.gpu
@pytest.mark.parametrize("nq", [1, 33, 300])
@pytest.mark.parametrize("scan", SCANS)
def test_l2_query_counts_and_id_offset(cuda, scan, nq):
    """One query, a partial wave, more than one 256-query group; ids carry the shard's offset (adopt)."""
    from sessionsimilaritysearch_amd.index import FlatIndex
    c, q = _data()["varnorm"]
    off = 10 ** 10
    idx = FlatIndex(128, "l2", cuda, scan=scan).adopt(torch.from_numpy(c[:5000]).to(cuda), id_offset=off)
    D, I = idx.search(q[:nq], 10)
    Dr, Ir = _oracle(q[:nq], c[:5000], 10)
    _equal((D, I), (Dr, Ir + off))
    assert idx.last_scan == scan


# ------------------------------------------------------------------------------------------- 5. near ties
@pytest.mark.gpu
@pytest.mark.parametrize("scan", SCANS)
def test_l2_near_ties_inside_the_window_go_to_the_rung(cuda, scan):
    """40 copies of a query's nearest row, copy j with coordinate j moved by (j + 1) 1e-5: neighbouring distances differ
    by ~1e-4, inside every scan's bound (>= 3e-3 at these norms: 2 x 129 x 2^-24 x (|q||c| + |c|^2 / 2) for the f32 scan),
    and they straddle rank k = 10 -- more of them than the select's second chance re-scores (32).  Exact; the query is
    unproven; the rung resolves it (40 rows, far below its capacity)."""
    from sessionsimilaritysearch_amd.index import FlatIndex
    c, q = _data()["gauss"]
    c, q = c[:4000].copy(), q[:40]
    near = _ref("gauss", 1)[1][0, 0]
    base = _data()["gauss"][0][near]
    for j in range(40):
        row = base.copy()
        row[j] += np.float32((j + 1) * 1e-5)
        c[100 + 7 * j] = row
    idx = FlatIndex(128, "l2", cuda, scan=scan)
    idx.add(c)
    Dr, Ir = _oracle(q, c, 10)
    assert len(set(Dr[0].tolist())) > 1 and Dr[0, 9] - Dr[0, 0] < 3e-3         # near, not exact, ties
    _equal(idx.search(q, 10), (Dr, Ir))
    assert idx.last_rescan_queries >= 1 and idx.last_fallback_queries == 0


# ------------------------------------------------------------------------------------------- 6. duplicates
@pytest.mark.gpu
@pytest.mark.parametrize("scan", SCANS)
def test_l2_duplicate_rows_straddling_rank_k(cuda, scan):
    """50 identical rows nearest to query 0, k = 10: exact ties, lowest ids win (the rung decides)."""
    from sessionsimilaritysearch_amd.index import FlatIndex
    c, q = _data()["gauss"]
    c, q = c[:6000].copy(), q[:40].copy()
    dup = np.arange(50) * 101 + 13
    c[dup] = c[5]
    q[0] = c[5] + np.float32(0.01)
    idx = FlatIndex(128, "l2", cuda, scan=scan)
    idx.add(c)
    Dr, Ir = _oracle(q, c, 10)
    assert Ir[0].tolist() == sorted([5] + dup.tolist())[:10] and (Dr[0] == Dr[0, 0]).all()
    _equal(idx.search(q, 10), (Dr, Ir))
    assert idx.last_rescan_queries >= 1 and idx.last_fallback_queries == 0


@pytest.mark.gpu
def test_l2_more_ties_than_the_rung_holds_go_exhaustive(cuda):
    """9000 identical nearest rows, above the rung's 8192: the exhaustive stage resolves the query."""
    from sessionsimilaritysearch_amd.index import FlatIndex
    c, q = _data()["gauss"]
    c, q = c.copy(), q[:33].copy()
    c[1000:10000] = c[0]
    q[3] = c[0]
    idx = FlatIndex(128, "l2", cuda, scan="f32")
    idx.add(c)
    Dr, Ir = _oracle(q, c, 10)
    assert Dr[3, 9] == 0 and Ir[3].tolist() == [0] + list(range(1000, 1009))
    _equal(idx.search(q, 10), (Dr, Ir))
    assert idx.last_scan == "f32" and idx.last_fallback_queries >= 1


# ------------------------------------------------------------------------------------------- 7. cancellation
@pytest.mark.gpu
@pytest.mark.parametrize("scan", SCANS)
def test_l2_far_from_the_origin_is_still_exact(cuda, scan):
    """"gauss" shifted by +100 in every coordinate, queries too: |c|^2 / 2 ~ 6.4e5 against distances ~ 2e2, so q.c and
    the bias cancel to 3e-4 of their size and the scan's bound (relative to the uncancelled magnitudes) is as wide as the
    gaps.  Exactness does not depend on centring the corpus: such queries come out unproven and are resolved exactly.
    The unproven count is printed, not asserted."""
    from sessionsimilaritysearch_amd.index import FlatIndex
    c, q = _data()["gauss"]
    c, q = (c[:8000] + np.float32(100)).astype(np.float32), (q[:64] + np.float32(100)).astype(np.float32)
    idx = FlatIndex(128, "l2", cuda, scan=scan)
    idx.add(c)
    _equal(idx.search(q, 10), _oracle(q, c, 10))
    assert idx.last_scan == scan
    print(f"l2 unproven: shifted +100 scan={scan} k=10: {idx.last_rescan_queries} of 64, fallbacks {idx.last_fallback_queries}")


# ------------------------------------------------------------------------------------------- 8. growth
@pytest.mark.gpu
@pytest.mark.parametrize("scan", SCANS)
def test_l2_bias_and_images_follow_add_and_adopt(cuda, scan):
    from sessionsimilaritysearch_amd.index import FlatIndex
    c, q = _data()["varnorm"]
    q = q[:33]
    idx = FlatIndex(128, "l2", cuda, scan=scan)
    for lo, hi in ((0, 1000), (1000, 1003), (1003, 7000)):
        idx.add(c[lo:hi])
        _equal(idx.search(q, 10), _oracle(q, c[:hi], 10))
        assert idx.last_scan == scan and idx._bias_done == hi
    want = (-0.5 * (c[:7000].astype(np.float64) ** 2).sum(1)).astype(np.float32)
    got = idx._bias[:7000].cpu().numpy()
    assert np.allclose(got, want, rtol=3e-7, atol=0)                      # (one float32 rounding; the float64 sums differ in order)
    idx.adopt(torch.from_numpy(c[9000:12000]).to(cuda))
    assert idx._bias is None and idx._bias_done == 0
    _equal(idx.search(q, 10), _oracle(q, c[9000:12000], 10))
    assert idx._bias_done == 3000


# ------------------------------------------------------------------------------------------- 9. sharded
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
    return D.cpu().numpy(), I.cpu().numpy(), [sh.engine.index.last_scan for sh in shards]


@pytest.mark.gpu
@pytest.mark.parametrize("S", [1, 2, 4])
def test_l2_sharded_takes_the_scan_route(cuda, S):
    c_h, q_h = _data()["varnorm"]
    c, q = torch.from_numpy(c_h).to(cuda), torch.from_numpy(q_h).to(cuda)
    D, I, scans = _sweep_search(c, q, 10, "l2", S, cuda)
    _equal((D, I), _ref("varnorm", 10))
    assert all(s in SCANS for s in scans), scans


# ------------------------------------------------------------------------------------------- 10. C ABI
P = ctypes.c_void_p


def _abi_setup(cuda):
    from sessionsimilaritysearch_amd import _lib
    L = _lib.lib()
    n, d, nq, k = 2048, 128, 8, 10
    c_h, q_h = _small(n, d, nq, 5)
    t = {"c": torch.from_numpy(c_h).to(cuda), "q": torch.from_numpy(q_h).to(cuda),
         "bias": torch.zeros(n + 4, dtype=torch.float32, device=cuda),
         "D": torch.full((nq, k), 7.0, dtype=torch.float32, device=cuda), "I": torch.full((nq, k), 7, dtype=torch.int64, device=cuda),
         "status": torch.full((nq,), 7, dtype=torch.int32, device=cuda),
         "state": torch.zeros(L.sss_ip_topk_state_bytes(nq), dtype=torch.uint8, device=cuda),
         "cmax": torch.zeros(1, dtype=torch.float32, device=cuda), "sel": torch.arange(nq, dtype=torch.int32, device=cuda)}
    assert L.sss_row_norm_max(t["c"].data_ptr(), n, d, 0, t["cmax"].data_ptr(), None) == 0
    return L, _lib, (n, d, nq, k), t, c_h, q_h


def _untouched(t):
    torch.cuda.synchronize()
    return bool((t["D"] == 7.0).all()) and bool((t["I"] == 7).all()) and bool((t["status"] == 7).all()) and not bool(t["state"].any())


@pytest.mark.gpu
def test_l2_abi_row_bias(cuda):
    L, _lib, (n, d, nq, k), t, c_h, _ = _abi_setup(cuda)
    t["bias"].fill_(5.0)
    assert L.sss_l2_row_bias(t["c"].data_ptr(), n, 6, t["bias"].data_ptr(), None) == -1       # d % 4
    assert L.sss_last_error().decode().startswith("l2_row_bias")
    assert L.sss_l2_row_bias(None, n, d, t["bias"].data_ptr(), None) == -1
    assert L.sss_l2_row_bias(t["c"].data_ptr(), 0, d, t["bias"].data_ptr(), None) == 0         # no-op
    torch.cuda.synchronize()
    assert bool((t["bias"] == 5.0).all())
    assert L.sss_l2_row_bias(t["c"].data_ptr(), n, d, t["bias"].data_ptr(), None) == 0
    got = t["bias"].cpu().numpy()
    want = bound_inputs_ref.bias_ref_rows(c_h)                                                 # ONE rounding of the exact -|c|^2 / 2
    assert np.array_equal(got[:n], want) and (got[n:] == 5.0).all()                            # nothing behind row n - 1


@pytest.mark.gpu
def test_l2_abi_topk_guards_and_result(cuda):
    L, _lib, (n, d, nq, k), t, c_h, q_h = _abi_setup(cuda)
    assert L.sss_l2_row_bias(t["c"].data_ptr(), n, d, t["bias"].data_ptr(), None) == 0
    cmax = float(t["cmax"].item())
    nbytes = L.sss_l2_topk_workspace_bytes(nq, n, d, k, 0)
    assert nbytes > 0 and L.sss_l2_topk_workspace_bytes(nq, n, d, k, 1) == 0 and L.sss_l2_topk_workspace_bytes(nq, n, 200, k, 0) == 0
    ws = torch.empty(nbytes, dtype=torch.uint8, device=cuda)

    def call(bias=None, scan=0, nq_=nq, ws_bytes=nbytes):
        b = t["bias"].data_ptr() if bias is None else bias
        return L.sss_l2_topk(t["q"].data_ptr(), nq_, t["c"].data_ptr(), t["c"].data_ptr(), scan, 0, 0.0, b, n, d, k, 0, cmax,
                             t["D"].data_ptr(), t["I"].data_ptr(), t["status"].data_ptr(), None, t["state"].data_ptr(),
                             t["state"].numel(), ws.data_ptr(), ws_bytes, None)

    for rc, want in ((call(bias=0), -1), (call(bias=t["bias"].data_ptr() + 4), -1), (call(ws_bytes=nbytes - 1), -2),
                     (call(scan=1), -1), (call(nq_=0), -1)):
        assert rc == want
        assert L.sss_last_error().decode().startswith("l2_topk"), L.sss_last_error()
        assert _untouched(t)
    assert call() == 0
    torch.cuda.synchronize()
    Dr, Ir = _oracle(q_h, c_h, k)
    ok = t["status"].cpu().numpy() == 0
    assert ok.any()
    assert np.array_equal(t["I"].cpu().numpy()[ok], Ir[ok]) and np.array_equal(t["D"].cpu().numpy()[ok], Dr[ok])
    assert not bool(t["state"].any())                                                            # handed back zeroed


@pytest.mark.gpu
def test_l2_abi_threshold_guards_and_result(cuda):
    L, _lib, (n, d, nq, k), t, c_h, q_h = _abi_setup(cuda)
    assert L.sss_l2_row_bias(t["c"].data_ptr(), n, d, t["bias"].data_ptr(), None) == 0
    cmax = float(t["cmax"].item())
    nbytes = L.sss_l2_topk_threshold_workspace_bytes(nq, n, d, 0)
    assert nbytes > 0 and L.sss_l2_topk_threshold_workspace_bytes(nq, n, d, 4) == 0
    ws = torch.empty(nbytes, dtype=torch.uint8, device=cuda)

    def call(bias=None, scan=0, nsel=nq, ws_bytes=nbytes):
        b = t["bias"].data_ptr() if bias is None else bias
        return L.sss_l2_topk_threshold(t["q"].data_ptr(), t["sel"].data_ptr(), nsel, t["c"].data_ptr(), t["c"].data_ptr(), scan, 0, 0.0,
                                       b, n, d, k, 0, cmax, t["D"].data_ptr(), t["I"].data_ptr(), t["status"].data_ptr(),
                                       ws.data_ptr(), ws_bytes, None)

    for rc, want in ((call(bias=0), -1), (call(bias=t["bias"].data_ptr() + 4), -1), (call(ws_bytes=nbytes - 1), -2),
                     (call(scan=1), -1), (call(nsel=0), -1)):
        assert rc == want
        assert L.sss_last_error().decode().startswith("l2_topk_threshold"), L.sss_last_error()
        assert _untouched(t)
    # no k-th distance known (+FLT_MAX in column k-1): the rung keeps every row -- 2048 of them, within its capacity
    t["D"].fill_(float(FLT_MAX))
    assert call() == 0
    torch.cuda.synchronize()
    Dr, Ir = _oracle(q_h, c_h, k)
    assert bool((t["status"] == 0).all())
    assert np.array_equal(t["I"].cpu().numpy(), Ir) and np.array_equal(t["D"].cpu().numpy(), Dr)
