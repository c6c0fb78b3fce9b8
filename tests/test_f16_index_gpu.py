"""FlatIndex(d, dtype="f16") -- rows stored as IEEE float16, scanned on the f16 MFMA, re-scored from the same rows --
against the CPU oracle on the float16-ROUNDED vectors (``torch.Tensor.to(torch.float16)`` defines the stored row):
ids and scores compared with ``array_equal``, through FlatIndex and through the raw C ABI (dtype = 4)."""
import functools

import numpy as np
import pytest
import torch

from oracle import search_ref as sr

pytestmark = pytest.mark.gpu


def _unit(rng, n, d):
    x = rng.standard_normal((n, d)).astype(np.float32)
    return sr.normalize(x).astype(np.float32)


def _h(x):
    """float32 array -> its float16 rounding (round to nearest even), back in float32: what the index stores."""
    return np.ascontiguousarray(x, np.float32).astype(np.float16).astype(np.float32)


def _f16_index(c, cuda, metric="ip"):
    from sessionsimilaritysearch_amd.index import FlatIndex
    idx = FlatIndex(c.shape[1], metric, cuda, dtype="f16")
    idx.add(c)
    return idx


def _equal(got, exp):
    D, I = got
    Dr, Ir = exp
    assert I.dtype == np.int64 and D.dtype == np.float32
    assert np.array_equal(I, Ir), np.argwhere(I != Ir)[:5]
    assert np.array_equal(D, Dr)


# ------------------------------------------------------------------------------------------ 1. the fused scan
@functools.lru_cache(maxsize=2)
def _case(d, nq, n):
    """(q, c, D500, I500): float16-rounded unit rows and their oracle top-500 (the top k is its first k columns)."""
    rng = np.random.default_rng(d * 31 + nq * 7 + n)
    q, c = _h(_unit(rng, nq, d)), _h(_unit(rng, n, d))
    Dr, Ir = sr.search_exact(q, c, 500)
    return q, c, Dr, Ir


@pytest.mark.parametrize("k", [1, 10, 100, 500])
@pytest.mark.parametrize("nq", [1, 33, 1024])
@pytest.mark.parametrize("n", [1000, 200_000])
@pytest.mark.parametrize("d", [128, 256, 512])
def test_f16_fused_matches_oracle(cuda, d, n, nq, k):
    q, c, Dr, Ir = _case(d, nq, n)
    idx = _f16_index(c, cuda)
    assert idx._xb.dtype == torch.float16 and idx._f16 is None and idx._split is None     # no copy beside the stored rows
    D, I = idx.search(q, k)
    assert idx.last_scan == "native"
    _equal((D, I), (Dr[:, :k], Ir[:, :k]))


def test_inputs_numpy_f32_f16_and_tensors(cuda):
    """numpy float32 or float16 in -> numpy out; CUDA float32 / float16 tensors in -> tensors out; all the same rows."""
    rng = np.random.default_rng(5)
    q, c = _unit(rng, 40, 128), _unit(rng, 5000, 128)
    exp = sr.search_exact(_h(q), _h(c), 10)
    a = _f16_index(c, cuda)
    _equal(a.search(q, 10), exp)
    _equal(a.search(q.astype(np.float16), 10), exp)
    b = _f16_index(c.astype(np.float16), cuda)
    D, I = b.search(torch.from_numpy(q).to(cuda), 10)
    assert isinstance(D, torch.Tensor) and D.is_cuda
    _equal((D.cpu().numpy(), I.cpu().numpy()), exp)
    e = _f16_index(torch.from_numpy(c).to(cuda).half(), cuda)
    D, I = e.search(torch.from_numpy(q).to(cuda).half(), 10)
    _equal((D.cpu().numpy(), I.cpu().numpy()), exp)
    from sessionsimilaritysearch_amd.index import to_f16
    t = torch.from_numpy(c).to(cuda)
    assert torch.equal(to_f16(t).cpu(), torch.from_numpy(c).to(torch.float16))
    assert torch.equal(a._xb.cpu(), torch.from_numpy(c).to(torch.float16))


# ------------------------------------------------------------------------------------------ 2. hard corpora
def test_duplicates_at_the_kth_place_go_through_the_rung(cuda):
    """40 copies of the best row per query: the k-th place is an exact tie under any scan, the lowest ids win, and the
    threshold rung (not the exhaustive kernels) resolves it."""
    rng = np.random.default_rng(11)
    c = _h(_unit(rng, 20000, 128))
    q = c[rng.integers(0, 20000, 24)].copy()
    for j in range(24):
        where = rng.choice(20000, 40, replace=False)
        c[where] = q[j]
    idx = _f16_index(c, cuda)
    D, I = idx.search(q, 10)
    _equal((D, I), sr.search_exact(q, c, 10))
    assert idx.last_scan == "native" and idx.last_rescan_queries >= 20 and idx.last_fallback_queries == 0
    # every row has 39 exact duplicates, permuted
    base = _h(_unit(rng, 50, 128))
    c2 = np.ascontiguousarray(np.repeat(base, 40, axis=0)[rng.permutation(2000)])
    q2 = _h(_unit(rng, 40, 128))
    _equal(_f16_index(c2, cuda).search(q2, 10), sr.search_exact(q2, c2, 10))


def test_near_ties_one_f16_ulp_apart(cuda):
    """Rows that differ from one another in ONE element by ONE float16 ulp: score gaps far inside the scan's error bound."""
    rng = np.random.default_rng(12)
    d, n = 128, 8000
    c16 = _unit(rng, n, d).astype(np.float16)
    q = _h(_unit(rng, 16, d))
    for j in range(16):                                       # 30 one-ulp variants of the row nearest to query j
        best = int(np.argmax(c16.astype(np.float32) @ q[j]))
        for t, row in enumerate(rng.choice(n, 30, replace=False)):
            v = c16[best].copy()
            bits = v.view(np.uint16)
            bits[(7 * t + j) % d] += np.uint16(1 + t % 2)     # one or two ulps up in magnitude
            c16[row] = v
    c = c16.astype(np.float32)
    assert np.isfinite(c).all()
    idx = _f16_index(c16, cuda)
    _equal(idx.search(q, 10), sr.search_exact(q, c, 10))
    _equal(idx.search(q, 100), sr.search_exact(q, c, 100))


def test_sorted_corpus_zero_rows_and_fewer_rows_than_k(cuda):
    rng = np.random.default_rng(13)
    q = _h(_unit(rng, 4, 128))
    c = _h(_unit(rng, 20000, 128))
    c = np.ascontiguousarray(c[np.argsort(c @ q[0])])        # ascending score for query 0: every row beats the running threshold
    _equal(_f16_index(c, cuda).search(q, 10), sr.search_exact(q, c, 10))
    z = np.zeros((3000, 128), np.float32)                    # all-zero rows: every score ties at 0
    idx = _f16_index(z, cuda)
    D, I = idx.search(q, 10)
    assert np.array_equal(I, np.tile(np.arange(10), (4, 1))) and np.array_equal(D, np.zeros((4, 10), np.float32))
    z[1000:1010] = c[:10]                                    # ... and a few rows that are not
    _equal(_f16_index(z, cuda).search(q, 10), sr.search_exact(q, z, 10))
    few = c[:7]
    D, I = _f16_index(few, cuda).search(q, 10)
    _equal((D, I), sr.search_exact(q, few, 10))
    assert (I[:, 7:] == -1).all() and (D[:, 7:] == sr.NEG_SENTINEL).all()


@pytest.mark.parametrize("d", [128, 512])
def test_subnormal_scale_rows_are_scanned_not_flushed(cuda, d):
    """Rows whose every element is a float16 SUBNORMAL (~1e-6; float16 normals start at 6.1e-5), and rows that mix
    subnormal elements with small normal ones.  The scan's bound assumes the matrix unit keeps float16 subnormal inputs:
    a unit that flushed them would score the first corpus 0 everywhere (nothing proven) and mis-rank the second."""
    rng = np.random.default_rng(14 + d)
    n, nq = 30000, 256
    q = _h(_unit(rng, nq, d))
    c = _h(rng.standard_normal((n, d)).astype(np.float32) * 1e-6)
    assert 0 < np.abs(c).max() < 6.0e-5 and (c != 0).mean() > 0.9
    idx = _f16_index(c, cuda)
    _equal(idx.search(q, 10), sr.search_exact(q, c, 10))
    assert idx.last_scan == "native" and idx.last_rescan_queries <= nq // 8, idx.last_rescan_queries
    m = rng.standard_normal((n, d)).astype(np.float32)
    m[:, ::2] *= 3e-5                                         # subnormal half ...
    m[:, 1::2] *= 1e-4                                        # ... and a normal half of about the same weight
    m = _h(m)
    idx = _f16_index(m, cuda)
    _equal(idx.search(q, 10), sr.search_exact(q, m, 10))
    # tiny queries against tiny rows: products down to 2^-48, still exact in float32
    tq = _h(q * 1e-4)
    _equal(idx.search(tq, 10), sr.search_exact(tq, m, 10))


def test_large_scale_rows(cuda):
    """Elements ~100, row norms ~1e3 (finite in float16), against unit and equally large queries."""
    rng = np.random.default_rng(15)
    c = _h(rng.standard_normal((30000, 128)).astype(np.float32) * 100.0)
    assert np.isfinite(c).all() and 900 < np.linalg.norm(c, axis=1).mean() < 1400
    idx = _f16_index(c, cuda)
    for q in (_h(_unit(rng, 64, 128)), _h(rng.standard_normal((64, 128)).astype(np.float32) * 100.0)):
        _equal(idx.search(q, 10), sr.search_exact(q, c, 10))
        assert idx.last_scan == "native"
    big = np.full((2000, 128), 65504.0, np.float32)           # the largest float16 everywhere: scores of 5.5e11, all tied
    big[::3] *= -1
    idx = _f16_index(big, cuda)
    qb = np.full((3, 128), 65504.0, np.float32)
    _equal(idx.search(qb, 10), sr.search_exact(qb, big, 10))


# ------------------------------------------------------------------------------------------ 3. the other routes
def test_long_rows_d1600_k100(cuda):
    rng = np.random.default_rng(16)
    q, c = _h(_unit(rng, 48, 1600)), _h(_unit(rng, 20000, 1600))
    c[5000:5020] = c[17]                                      # duplicates inside the kept set
    idx = _f16_index(c, cuda)
    D, I = idx.search(q, 100)
    assert idx.last_scan == "long" and idx._f16 is None
    _equal((D, I), sr.search_exact(q, c, 100))


def test_exhaustive_shapes_d200_and_k600(cuda):
    rng = np.random.default_rng(17)
    q, c = _h(_unit(rng, 9, 200)), _h(_unit(rng, 3000, 200))
    idx = _f16_index(c, cuda)
    D, I = idx.search(q, 10)
    assert idx.scan_for(10) == "" and idx.last_fallback_queries == 9
    _equal((D, I), sr.search_exact(q, c, 10))
    q, c = _h(_unit(rng, 5, 128)), _h(_unit(rng, 4000, 128))
    idx = _f16_index(c, cuda)
    D, I = idx.search(q, 600)
    assert idx.scan_for(600) == "" and idx.last_fallback_queries == 5
    _equal((D, I), sr.search_exact(q, c, 600))


@pytest.mark.parametrize("d", [128, 200])
def test_l2_metric(cuda, d):
    rng = np.random.default_rng(18 + d)
    q, c = _h(_unit(rng, 12, d)), _h(_unit(rng, 3000, d) * 1.5)
    c[100:110] = c[5]
    idx = _f16_index(c, cuda, "l2")
    D, I = idx.search(q, 10)
    _equal((D, I), sr.topk_from_scores(sr.canonical_l2(q, c), 10, largest=False))


def _range_expected(q, c, radius, metric, id_offset=0):
    s = (sr.canonical_scores if metric == "ip" else sr.canonical_l2)(q, c)
    keep = s > np.float32(radius) if metric == "ip" else s < np.float32(radius)
    lims = np.zeros(q.shape[0] + 1, np.int64)
    lims[1:] = np.cumsum(keep.sum(1))
    rows = [np.flatnonzero(k) for k in keep]
    D = np.concatenate([s[a, j] for a, j in enumerate(rows)]).astype(np.float32)
    I = np.concatenate(rows).astype(np.int64) + id_offset
    return lims, D, I


@pytest.mark.parametrize("metric,d", [("ip", 128), ("ip", 512), ("ip", 200), ("l2", 128)])
def test_range_search(cuda, metric, d):
    rng = np.random.default_rng(19 + d)
    nq, n = 32, 20000
    q, c = _h(_unit(rng, nq, d)), _h(_unit(rng, n, d))
    s = (sr.canonical_scores if metric == "ip" else sr.canonical_l2)(q, c)
    frac = 25.0 / n                                           # ~25 rows per query
    radius = np.float32(np.quantile(s, 1.0 - frac if metric == "ip" else frac))
    idx = _f16_index(c, cuda, metric)
    lims, D, I = idx.range_search(q, radius)
    el, eD, eI = _range_expected(q, c, radius, metric)
    assert 10 * nq < el[-1] < 60 * nq
    assert idx.last_range_scan == ("native" if metric == "ip" and d in (128, 512) else "")
    assert np.array_equal(lims, el) and np.array_equal(I, eI) and np.array_equal(D, eD)


def test_streaming_add_adopt_and_id_offset(cuda):
    from sessionsimilaritysearch_amd.index import FlatIndex
    rng = np.random.default_rng(20)
    q, c = _h(_unit(rng, 30, 128)), _h(_unit(rng, 5000, 128))
    exp = sr.search_exact(q, c, 10)
    one = _f16_index(c, cuda)
    three = FlatIndex(128, "ip", cuda, dtype="f16")
    for lo, hi in ((0, 1234), (1234, 1235), (1235, 5000)):
        three.add(c[lo:hi])
    assert three.ntotal == 5000 and three.corpus_max_norm() == one.corpus_max_norm()
    _equal(one.search(q, 10), exp)
    _equal(three.search(q, 10), exp)
    xb = torch.from_numpy(c).to(cuda).to(torch.float16)
    ad = FlatIndex(128, "ip", cuda, dtype="f16").adopt(xb, id_offset=1_000_000)
    assert ad._xb.data_ptr() == xb.data_ptr() and ad.prepare(10) == "native"
    _equal(ad.search(q, 10), sr.search_exact(q, c, 10, id_offset=1_000_000))
    with pytest.raises(Exception):
        FlatIndex(128, "ip", cuda, dtype="f16").adopt(xb.float())          # not the index's element type


@pytest.mark.parametrize("shards", [2, 4])
def test_shard_merge_equals_single_index(cuda, shards):
    """Row-sharding invariant: merged per-shard top-k (ShardedFlatIndex's engine + sss_topk_merge) == one index."""
    from sessionsimilaritysearch_amd import _lib
    from sessionsimilaritysearch_amd.distributed import HipEngine
    from sessionsimilaritysearch_amd.index import FlatIndex
    rng = np.random.default_rng(21)
    nq, n, k = 100, 40000, 10
    q, c = _h(_unit(rng, nq, 128)), _h(_unit(rng, n, 128))
    c[n // 2 - 3:n // 2 + 3] = c[7]                           # duplicates across a shard boundary
    single = _f16_index(c, cuda)
    Ds, Is = single.search(q, k)
    _equal((Ds, Is), sr.search_exact(q, c, k))
    tq = single._rows(q, "q")
    per = n // shards
    Dl, Il = [], []
    for s in range(shards):
        idx = FlatIndex(128, "ip", cuda, dtype="f16")
        idx.add(c[s * per:(s + 1) * per])
        idx.id_offset = s * per
        eng = HipEngine(idx)
        D = torch.empty((nq, k), dtype=torch.float32, device=cuda)
        I = torch.empty((nq, k), dtype=torch.int64, device=cuda)
        status = torch.empty((nq,), dtype=torch.int32, device=cuda)
        eng.local_search(tq, k, D, I, status)
        eng.fix_unproven(tq, k, D, I, status)
        Dl.append(D); Il.append(I)
    Din, Iin = torch.stack(Dl).contiguous(), torch.stack(Il).contiguous()
    Dm, Im = torch.empty_like(Dl[0]), torch.empty_like(Il[0])
    rc = _lib.lib().sss_topk_merge(Din.data_ptr(), nq * k, Iin.data_ptr(), nq * k, shards, nq, k, Dm.data_ptr(), Im.data_ptr(),
                                   _lib.stream_ptr(cuda))
    _lib.check(rc, "sss_topk_merge")
    assert np.array_equal(Im.cpu().numpy(), Is) and np.array_equal(Dm.cpu().numpy(), Ds)


def test_add_refuses_rows_that_overflow_float16(cuda):
    from sessionsimilaritysearch_amd.index import FlatIndex
    rng = np.random.default_rng(22)
    c = _unit(rng, 1000, 128)
    idx = FlatIndex(128, "ip", cuda, dtype="f16")
    idx.add(c[:600])
    cmax = idx.corpus_max_norm()
    for bad in (70000.0, -1e9, np.inf, np.nan):
        x = c[600:].copy()
        x[123, 45] = bad
        with pytest.raises(ValueError):
            idx.add(x)
        assert idx.ntotal == 600 and idx.corpus_max_norm() == cmax       # nothing stored, no bound poisoned
    with pytest.raises(ValueError):
        idx.add(torch.full((8, 128), float("inf"), dtype=torch.float16, device=cuda))
    edge = c[600:].copy()
    edge[0, 0] = 65504.0                                      # the largest finite float16 is a value like any other
    idx.add(edge)
    assert idx.ntotal == 1000
    q = _h(_unit(rng, 8, 128))
    full = np.concatenate([c[:600], edge])
    _equal(idx.search(q, 10), sr.search_exact(q, _h(full), 10))


# ------------------------------------------------------------------------------------------ 4. the proof
def test_f16_scan_proves_at_least_what_the_bf16_scan_proves(cuda):
    """Finer inputs must not make the proof weaker: on random unit rows the float16 scan leaves no more queries unproven
    than the bf16 index leaves on the same rows rounded to bfloat16 (both counts from this run)."""
    from sessionsimilaritysearch_amd.index import FlatIndex
    rng = np.random.default_rng(23)
    n, d, nq, k = 200_000, 128, 1024, 10
    q, c = _unit(rng, nq, d), _unit(rng, n, d)
    rescans = {}
    for dtype, rnd in (("bf16", lambda x: torch.from_numpy(x).to(torch.bfloat16).float().numpy()), ("f16", _h)):
        qr, cr = rnd(q), rnd(c)
        Dr, Ir = sr.search_exact(qr, cr, k + 1)
        assert (Dr[:, k - 1] > Dr[:, k]).all(), dtype          # no exact tie at rank k: nothing is unprovable by construction
        idx = FlatIndex(d, "ip", cuda, dtype=dtype)
        idx.add(c)
        D, I = idx.search(q, k)
        _equal((D, I), (Dr[:, :k], Ir[:, :k]))
        assert idx.last_scan == "native"
        rescans[dtype] = idx.last_rescan_queries
    print(f"unproven queries of {nq}: bf16 {rescans['bf16']}, f16 {rescans['f16']}")
    assert rescans["f16"] <= rescans["bf16"] + 2, rescans


# ------------------------------------------------------------------------------------------ 5. the raw C ABI
def test_c_abi_ip_topk_and_threshold_with_dtype_4(cuda):
    """sss_ip_topk(dtype = 4) then sss_ip_topk_threshold(dtype = 4, scan = 4) on float16 device buffers, no FlatIndex:
    duplicates leave some queries unproven (status != 0), the rung resolves them; with every status 0 the result is the
    oracle's."""
    from sessionsimilaritysearch_amd import _lib
    L = _lib.lib()
    rng = np.random.default_rng(24)
    nq, n, d, k = 96, 50000, 256, 10
    q, c = _h(_unit(rng, nq, d)), _h(_unit(rng, n, d))
    for j in range(0, nq, 4):                                 # every fourth query: 40 more copies of its best row -- more
        best = int(np.argmax(c @ q[j]))                       # ties than the fused select can re-score (32 candidates)
        c[rng.choice(n, 40, replace=False)] = c[best]
    st = _lib.stream_ptr(cuda)
    tq = torch.from_numpy(q).to(cuda).to(torch.float16)
    tc = torch.from_numpy(c).to(cuda).to(torch.float16)
    cmax = torch.zeros(1, dtype=torch.float32, device=cuda)
    _lib.check(L.sss_row_norm_max(tc.data_ptr(), n, d, 4, cmax.data_ptr(), st), "sss_row_norm_max")
    cm = float(cmax.item())
    assert float(np.linalg.norm(c.astype(np.float64), axis=1).max()) <= cm <= 1.001
    D = torch.empty((nq, k), dtype=torch.float32, device=cuda)
    I = torch.empty((nq, k), dtype=torch.int64, device=cuda)
    status = torch.empty((nq,), dtype=torch.int32, device=cuda)
    unproven = torch.zeros(1, dtype=torch.int32, device=cuda)
    ws = torch.empty(L.sss_ip_topk_workspace_bytes(nq, n, d, k, 4), dtype=torch.uint8, device=cuda)
    state = torch.zeros(L.sss_ip_topk_state_bytes(nq), dtype=torch.uint8, device=cuda)
    assert ws.numel() > 0
    rc = L.sss_ip_topk(tq.data_ptr(), nq, tc.data_ptr(), n, d, k, 4, 0, cm, D.data_ptr(), I.data_ptr(), status.data_ptr(),
                       unproven.data_ptr(), state.data_ptr(), state.numel(), ws.data_ptr(), ws.numel(), st)
    _lib.check(rc, "sss_ip_topk")
    Dr, Ir = sr.search_exact(q, c, k)
    s0 = status.cpu().numpy()
    assert int(unproven.item()) == int((s0 != 0).sum()) and (s0[0::4] != 0).all() and (s0 != 0).sum() <= nq // 4 + 4
    assert not state.any()                                   # handed back zeroed
    ok = s0 == 0
    assert np.array_equal(I.cpu().numpy()[ok], Ir[ok]) and np.array_equal(D.cpu().numpy()[ok], Dr[ok])
    sel = torch.nonzero(status).flatten().to(torch.int32)
    ws2 = torch.empty(L.sss_ip_topk_threshold_workspace_bytes(sel.numel(), n, d, 4), dtype=torch.uint8, device=cuda)
    rc = L.sss_ip_topk_threshold(tq.data_ptr(), sel.data_ptr(), sel.numel(), tc.data_ptr(), 4, tc.data_ptr(), 4, 0, 0.0, n, d, k, 0,
                                 cm, D.data_ptr(), I.data_ptr(), status.data_ptr(), ws2.data_ptr(), ws2.numel(), st)
    _lib.check(rc, "sss_ip_topk_threshold")
    assert not status.any()
    assert np.array_equal(I.cpu().numpy(), Ir) and np.array_equal(D.cpu().numpy(), Dr)
    # a non-finite row reads as +inf in the norm reduction
    tc2 = tc[:64].clone()
    tc2[3, 5] = float("inf")
    cmax.zero_()
    _lib.check(L.sss_row_norm_max(tc2.data_ptr(), 64, d, 4, cmax.data_ptr(), st), "sss_row_norm_max")
    assert float(cmax.item()) == float("inf")
