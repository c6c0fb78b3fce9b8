"""FlatIndex(d, dtype="i8") -- rows stored as int8, scanned on v_mfma_i32_32x32x32_i8, re-scored from the same rows --
against the CPU oracle on the int8 values as float32 (``oracle.search_ref`` serves as it is: every partial sum of its
float64 chain is an integer): ids and scores compared with ``array_equal``, through FlatIndex and through the raw C ABI
(dtype = 6; 5 stays unassigned)."""
import functools

import numpy as np
import pytest
import torch

from oracle import search_ref as sr

pytestmark = pytest.mark.gpu

I8 = 6
GUARD = 4096


def _codes(rng, n, d, spread=30.0):
    """int8 rows as a quantised embedding has them: rounded normals (sd `spread`), clipped at +-127."""
    return np.clip(np.rint(rng.standard_normal((n, d)) * spread), -127, 127).astype(np.int8)


def _f(x):
    return np.ascontiguousarray(x).astype(np.float32)


def _i8_index(c, cuda, metric="ip"):
    from sessionsimilaritysearch_amd.index import FlatIndex
    idx = FlatIndex(c.shape[1], metric, cuda, dtype="i8")
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
    """(q, c, D500, I500): int8 rows and their oracle top-500 (the top k is its first k columns)."""
    rng = np.random.default_rng(d * 31 + nq * 7 + n)
    q, c = _codes(rng, nq, d), _codes(rng, n, d)
    Dr, Ir = sr.search_exact(_f(q), _f(c), 500)
    return q, c, Dr, Ir


@pytest.mark.parametrize("k", [1, 10, 100, 500])
@pytest.mark.parametrize("nq", [33, 1024])
@pytest.mark.parametrize("n", [1000, 100_003])              # neither a multiple of a 64 / 128 / 256-row tile
@pytest.mark.parametrize("d", [256, 512, 1024])
def test_i8_fused_matches_oracle(cuda, d, n, nq, k):
    q, c, Dr, Ir = _case(d, nq, n)
    idx = _i8_index(c, cuda)
    assert idx._xb.dtype == torch.int8 and idx._f16 is None and idx._split is None      # no copy beside the stored rows
    D, I = idx.search(q, k)
    assert idx.last_scan == "native"
    print(f"d {d} n {n} nq {nq} k {k}: unproven {idx.last_rescan_queries}, exhaustive {idx.last_fallback_queries}")
    _equal((D, I), (Dr[:, :k], Ir[:, :k]))


def test_one_query_fewer_rows_than_k_and_id_offset(cuda):
    from sessionsimilaritysearch_amd.index import FlatIndex
    rng = np.random.default_rng(3)
    c, q = _codes(rng, 70_003, 256), _codes(rng, 1, 256)
    _equal(_i8_index(c, cuda).search(q, 10), sr.search_exact(_f(q), _f(c), 10))
    few, q4 = c[:7], _codes(rng, 4, 256)
    D, I = _i8_index(few, cuda).search(q4, 10)
    _equal((D, I), sr.search_exact(_f(q4), _f(few), 10))
    assert (I[:, 7:] == -1).all() and (D[:, 7:] == sr.NEG_SENTINEL).all()
    xb = torch.from_numpy(c).to(cuda)
    ad = FlatIndex(256, "ip", cuda, dtype="i8").adopt(xb, id_offset=1_000_000)
    assert ad._xb.data_ptr() == xb.data_ptr() and ad.prepare(10) == "native"
    q30 = _codes(rng, 30, 256)
    _equal(ad.search(q30, 10), sr.search_exact(_f(q30), _f(c), 10, id_offset=1_000_000))
    with pytest.raises(Exception):
        FlatIndex(256, "ip", cuda, dtype="i8").adopt(xb.float())          # not the index's element type
    three = FlatIndex(256, "ip", cuda, dtype="i8")                        # streaming adds
    for lo, hi in ((0, 1234), (1234, 1235), (1235, 70_003)):
        three.add(c[lo:hi])
    assert three.ntotal == 70_003 and three.corpus_max_norm() == ad.corpus_max_norm()
    _equal(three.search(q30, 10), sr.search_exact(_f(q30), _f(c), 10))


def test_inputs_numpy_int8_float_and_tensors(cuda):
    """np.int8 / integer-valued float32 in -> numpy out; CUDA int8 / float tensors in -> tensors out; all the same rows."""
    rng = np.random.default_rng(5)
    q, c = _codes(rng, 40, 256), _codes(rng, 5000, 256)
    exp = sr.search_exact(_f(q), _f(c), 10)
    a = _i8_index(c, cuda)
    _equal(a.search(q, 10), exp)
    _equal(a.search(_f(q), 10), exp)                          # float input that holds integers
    b = _i8_index(_f(c), cuda)
    assert torch.equal(b._xb.cpu(), torch.from_numpy(c))
    D, I = b.search(torch.from_numpy(q).to(cuda), 10)
    assert isinstance(D, torch.Tensor) and D.is_cuda
    _equal((D.cpu().numpy(), I.cpu().numpy()), exp)
    e = _i8_index(torch.from_numpy(c).to(cuda), cuda)
    D, I = e.search(torch.from_numpy(_f(q)).to(cuda), 10)
    _equal((D.cpu().numpy(), I.cpu().numpy()), exp)
    from sessionsimilaritysearch_amd.index import quantize_i8
    x = rng.standard_normal((64, 256)).astype(np.float32)
    codes, scale = quantize_i8(torch.from_numpy(x).to(cuda))
    assert codes.is_cuda and codes.dtype == torch.int8
    assert np.array_equal(codes.cpu().numpy(), np.clip(np.rint(x * np.float32(scale)), -127, 127).astype(np.int8))


# ------------------------------------------------------------------------------------------ 2. the other routes
def test_exhaustive_shapes_d48_d1600_and_k600(cuda):
    rng = np.random.default_rng(17)
    for d, n, nq in ((48, 3000, 9), (1600, 3000, 6)):
        q, c = _codes(rng, nq, d), _codes(rng, n, d)
        c[100:105] = c[7]
        idx = _i8_index(c, cuda)
        D, I = idx.search(q, 10)
        assert idx.scan_for(10) == "" and idx.last_fallback_queries == nq
        _equal((D, I), sr.search_exact(_f(q), _f(c), 10))
    q, c = _codes(rng, 5, 256), _codes(rng, 4000, 256)
    idx = _i8_index(c, cuda)
    D, I = idx.search(q, 600)
    assert idx.scan_for(600) == "" and idx.last_fallback_queries == 5
    _equal((D, I), sr.search_exact(_f(q), _f(c), 600))


@pytest.mark.parametrize("d", [256, 48])
def test_l2_metric(cuda, d):
    rng = np.random.default_rng(18 + d)
    q, c = _codes(rng, 12, d), _codes(rng, 3000, d)
    c[100:110] = c[5]
    c[200], c[201] = 127, -128                                # rows at the ends of the range
    q[0], q[1], q[2] = c[5], 127, -128                        # distance 0 eleven times over; distance 0 to row 200 / 201
    idx = _i8_index(c, cuda, "l2")
    D, I = idx.search(q, 10)
    assert idx.scan_for(10) == ""
    _equal((D, I), sr.topk_from_scores(sr.canonical_l2(_f(q), _f(c)), 10, largest=False))
    assert I[1, 0] == 200 and I[2, 0] == 201 and D[1, 0] == 0 and list(I[0, :2]) == [5, 100]
    far = np.full((1, d), 127, np.int8)                       # ... and the largest distance an int8 pair has: d * 255^2
    D, I = _i8_index(c[:1000], cuda, "l2").search(far, 1000)  # (every row returned: the farthest one comes last)
    _equal((D, I), sr.topk_from_scores(sr.canonical_l2(_f(far), _f(c[:1000])), 1000, largest=False))
    assert I[0, -1] == 201 and D[0, -1] == np.float32(d * 255 * 255)


# ------------------------------------------------------------------------------------------ 3. exact ties
def test_duplicate_blocks_straddling_rank_k_below_the_rung_capacity(cuda):
    """40 copies of the best row per query: the k-th place is an exact tie (the only thing an int8 scan cannot prove), the
    lowest ids win, and the threshold rung -- not the exhaustive kernels -- resolves it."""
    rng = np.random.default_rng(11)
    c = _codes(rng, 20000, 256)
    q = c[rng.integers(0, 20000, 24)].copy()
    for j in range(24):
        c[rng.choice(20000, 40, replace=False)] = q[j]
    idx = _i8_index(c, cuda)
    D, I = idx.search(q, 10)
    print(f"40 duplicates: unproven {idx.last_rescan_queries}, exhaustive {idx.last_fallback_queries}")
    _equal((D, I), sr.search_exact(_f(q), _f(c), 10))
    assert idx.last_scan == "native" and idx.last_fallback_queries == 0
    base = _codes(rng, 50, 256)                               # every row has 39 exact duplicates, permuted
    c2 = np.ascontiguousarray(np.repeat(base, 40, axis=0)[rng.permutation(2000)])
    q2 = _codes(rng, 40, 256)
    _equal(_i8_index(c2, cuda).search(q2, 10), sr.search_exact(_f(q2), _f(c2), 10))
    _equal(_i8_index(c2, cuda).search(q2, 100), sr.search_exact(_f(q2), _f(c2), 100))


def test_duplicate_block_beyond_the_rung_capacity(cuda):
    """9000 copies of one row -- more than the rung keeps (8192): queries whose rank k falls inside the block go on to the
    exhaustive kernels; still the oracle's rows, lowest ids first."""
    rng = np.random.default_rng(12)
    n, d = 30000, 512
    c = _codes(rng, n, d)
    hot = c[123].copy()
    where = rng.choice(n, 9000, replace=False)
    c[where] = hot
    q = _codes(rng, 16, d)
    q[:8] = hot                                               # the block is these queries' best score
    idx = _i8_index(c, cuda)
    for k in (10, 100):
        D, I = idx.search(q, k)
        print(f"9000 duplicates, k {k}: unproven {idx.last_rescan_queries}, exhaustive {idx.last_fallback_queries}")
        _equal((D, I), sr.search_exact(_f(q), _f(c), k))
        assert np.array_equal(I[0], np.union1d(where, [123])[:k])


def test_low_magnitude_corpus_where_most_queries_tie_at_rank_k(cuda):
    """Elements in {-1, 0, 1}: scores are small integers, thousands of rows share each value, and rank k nearly always
    falls inside a tie group.  The counts are reported, not asserted."""
    rng = np.random.default_rng(13)
    n, d, nq = 50000, 256, 128
    c = rng.integers(-1, 2, (n, d)).astype(np.int8)
    q = rng.integers(-1, 2, (nq, d)).astype(np.int8)
    idx = _i8_index(c, cuda)
    for k in (10, 100):
        Dr, Ir = sr.search_exact(_f(q), _f(c), k + 1)
        D, I = idx.search(q, k)
        print(f"{{-1,0,1}} corpus, k {k}: ties at rank k {(Dr[:, k - 1] == Dr[:, k]).sum()} of {nq}, "
              f"unproven {idx.last_rescan_queries}, exhaustive {idx.last_fallback_queries}")
        _equal((D, I), (np.ascontiguousarray(Dr[:, :k]), np.ascontiguousarray(Ir[:, :k])))


# ------------------------------------------------------------------------------------------ 4. magnitude ends
def test_magnitude_ends_at_d1024(cuda):
    """All +-127, and all -128 (score 1024 * 2^14 = 2^24, the largest integer a fused int8 shape produces and the last
    one up to which float32 holds every integer)."""
    rng = np.random.default_rng(14)
    d, n = 1024, 3000
    c = (rng.integers(0, 2, (n, d)) * 254 - 127).astype(np.int8)
    q = (rng.integers(0, 2, (8, d)) * 254 - 127).astype(np.int8)
    c[17], c[1999] = q[0], q[0]                               # score 1024 * 127^2, twice
    c[5], q[1] = -128, -128                                   # and 2^24 once
    idx = _i8_index(c, cuda)
    D, I = idx.search(q, 10)
    _equal((D, I), sr.search_exact(_f(q), _f(c), 10))
    assert D[0, 0] == D[0, 1] == np.float32(1024 * 127 * 127) and list(I[0, :2]) == [17, 1999]
    assert D[1, 0] == np.float32(2.0 ** 24) and I[1, 0] == 5
    lo = np.full((n, d), -128, np.int8)                       # every row ties at 2^24 against an all -128 query
    ql = np.full((3, d), -128, np.int8)
    ql[2] = 127
    idx = _i8_index(lo, cuda)
    D, I = idx.search(ql, 10)
    _equal((D, I), sr.search_exact(_f(ql), _f(lo), 10))
    assert np.array_equal(I, np.tile(np.arange(10), (3, 1)))
    assert (D[:2] == np.float32(2.0 ** 24)).all() and (D[2] == np.float32(-1024 * 128 * 127)).all()
    lo[::3] = 127
    _equal(_i8_index(lo, cuda).search(ql, 100), sr.search_exact(_f(ql), _f(lo), 100))


def test_all_zero_corpus(cuda):
    rng = np.random.default_rng(15)
    q = _codes(rng, 4, 256)
    z = np.zeros((3000, 256), np.int8)
    idx = _i8_index(z, cuda)
    D, I = idx.search(q, 10)
    assert idx.corpus_max_norm() == 0.0
    assert np.array_equal(I, np.tile(np.arange(10), (4, 1))) and np.array_equal(D, np.zeros((4, 10), np.float32))
    z[1000:1010] = _codes(rng, 10, 256)                       # ... and a few rows that are not
    _equal(_i8_index(z, cuda).search(q, 10), sr.search_exact(_f(q), _f(z), 10))
    zq = np.zeros((2, 256), np.int8)
    _equal(_i8_index(z, cuda).search(zq, 10), sr.search_exact(_f(zq), _f(z), 10))


# ------------------------------------------------------------------------------------------ 5. range search
def _range_expected(q, c, radius, metric, id_offset=0):
    s = (sr.canonical_scores if metric == "ip" else sr.canonical_l2)(_f(q), _f(c))
    r = np.broadcast_to(np.asarray(radius, np.float32).reshape(-1, 1), (q.shape[0], 1))
    keep = s > r if metric == "ip" else s < r
    lims = np.zeros(q.shape[0] + 1, np.int64)
    lims[1:] = np.cumsum(keep.sum(1))
    rows = [np.flatnonzero(k) for k in keep]
    D = np.concatenate([s[a, j] for a, j in enumerate(rows)]).astype(np.float32)
    I = np.concatenate(rows).astype(np.int64) + id_offset
    return lims, D, I, s


@pytest.mark.parametrize("metric,d", [("ip", 256), ("ip", 1024), ("ip", 48), ("l2", 256)])
def test_range_search_scalar_and_per_query_radii(cuda, metric, d):
    rng = np.random.default_rng(19 + d)
    nq, n = 32, 20000
    q, c = _codes(rng, nq, d), _codes(rng, n, d)
    s = (sr.canonical_scores if metric == "ip" else sr.canonical_l2)(_f(q), _f(c))
    srt = np.sort(s, axis=1)
    idx = _i8_index(c, cuda, metric)
    # a scalar radius near the 25th best of the whole batch; then one radius per query EQUAL to an attained integer
    # score -- its 20th best: the comparison is strict, so that row and its ties stay out
    scalar = np.float32(np.quantile(s, 1.0 - 25.0 / n if metric == "ip" else 25.0 / n))
    per_query = (srt[:, -20] if metric == "ip" else srt[:, 19]).astype(np.float32)
    for radius in (scalar, per_query):
        lims, D, I = idx.range_search(q, radius)
        el, eD, eI, _ = _range_expected(q, c, radius, metric)
        assert 5 * nq < el[-1] < 60 * nq
        assert idx.last_range_scan == ("native" if metric == "ip" and d in (256, 1024) else "")
        assert np.array_equal(lims, el) and np.array_equal(I, eI) and np.array_equal(D, eD)
    attained = (s == per_query[:, None]).sum(1)
    assert (attained >= 1).all()                              # every per-query radius is a score some row has
    assert (np.diff(lims) <= 19).all()                        # ... and that row is not returned
    lims, D, I = idx.range_search(torch.from_numpy(q).to(cuda), torch.from_numpy(per_query).to(cuda))
    assert isinstance(D, torch.Tensor) and np.array_equal(I.cpu().numpy(), eI) and np.array_equal(D.cpu().numpy(), eD)


def test_range_search_overflow_route(cuda):
    """A radius that more than 8192 rows pass: those queries leave the fused route for the exhaustive one."""
    rng = np.random.default_rng(20)
    nq, n, d = 12, 30000, 256
    q, c = _codes(rng, nq, d), _codes(rng, n, d)
    s = sr.canonical_scores(_f(q), _f(c))
    radius = np.sort(s, axis=1)[:, -30].astype(np.float32)
    radius[::3] = np.float32(0.0)                             # ~half the corpus
    radius[1] = np.float32(-3.0e38)                           # every row
    idx = _i8_index(c, cuda)
    lims, D, I = idx.range_search(q, radius)
    el, eD, eI, _ = _range_expected(q, c, radius, "ip")
    assert idx.last_range_scan == "native" and idx.last_range_overflow_queries >= 5
    assert np.array_equal(lims, el) and np.array_equal(I, eI) and np.array_equal(D, eD)
    assert lims[2] - lims[1] == n


# ------------------------------------------------------------------------------------------ 6. input checking
def test_float_input_must_hold_integers_in_range(cuda):
    from sessionsimilaritysearch_amd.index import FlatIndex
    rng = np.random.default_rng(22)
    c = _codes(rng, 1000, 256)
    idx = FlatIndex(256, "ip", cuda, dtype="i8")
    idx.add(_f(c[:600]))
    cmax = idx.corpus_max_norm()
    assert cmax >= float(np.linalg.norm(_f(c[:600]).astype(np.float64), axis=1).max())
    for bad in (0.5, -3.25, 128.0, -129.0, 1e9, np.inf, -np.inf, np.nan):
        x = _f(c[600:])
        x[123, 45] = bad
        with pytest.raises(ValueError):
            idx.add(x)
        with pytest.raises(ValueError):
            idx.add(torch.from_numpy(x).to(cuda))
        assert idx.ntotal == 600 and idx.corpus_max_norm() == cmax       # nothing stored, no bound touched
        with pytest.raises(ValueError):
            idx.search(x[120:130], 10)
        with pytest.raises(ValueError):
            idx.range_search(x[120:130], 0.0)
    edge = _f(c[600:])
    edge[0, 0], edge[0, 1] = -128.0, 127.0                    # the ends of the range are values like any other
    idx.add(edge)
    assert idx.ntotal == 1000
    q = _codes(rng, 8, 256)
    full = np.concatenate([_f(c[:600]), edge])
    _equal(idx.search(q, 10), sr.search_exact(_f(q), full, 10))
    for d in (8, 24, 250):
        with pytest.raises(ValueError):
            FlatIndex(d, "ip", cuda, dtype="i8")
    with pytest.raises(ValueError):
        idx.add(c[:10, :128])                                 # wrong width


# ------------------------------------------------------------------------------------------ 7. the raw C ABI
class Buf:
    """`shape` x `dtype` on the device, exactly that many bytes, 256-byte aligned, between two GUARD-byte bands of a
    known byte pattern."""

    def __init__(self, shape, dtype, seed, zero=False):
        self.shape = tuple(int(s) for s in shape) if isinstance(shape, (tuple, list)) else (int(shape),)
        self.dtype = dtype
        self.nbytes = int(np.prod(self.shape, dtype=np.int64)) * torch.empty((), dtype=dtype).element_size()
        raw = torch.empty(2 * GUARD + self.nbytes + 256, dtype=torch.uint8, device="cuda")
        self.off = GUARD + (-(raw.data_ptr() + GUARD)) % 256
        g = torch.Generator().manual_seed(seed)
        self.pat = torch.randint(0, 256, (raw.numel(),), dtype=torch.uint8, generator=g).to("cuda")
        raw.copy_(self.pat)
        self.raw = raw
        if zero:
            self.bytes.zero_()

    @property
    def ptr(self):
        return self.raw.data_ptr() + self.off

    @property
    def bytes(self):
        return self.raw[self.off:self.off + self.nbytes]

    @property
    def t(self):
        return self.bytes.view(self.dtype).view(self.shape)

    def guards_ok(self):
        e = self.off + self.nbytes
        return torch.equal(self.raw[:self.off], self.pat[:self.off]) and torch.equal(self.raw[e:], self.pat[e:])


def test_c_abi_topk_rung_and_range_with_the_int8_code(cuda):
    """sss_ip_topk(dtype 6), sss_ip_topk_threshold(dtype 6, scan 6, image = corpus) and sss_range_search_count / _fill on
    int8 device buffers of exactly the sizes the sizing calls name, each between guard bands: nothing outside them is
    written, status ends all zero, the state comes back zeroed, the results are the oracle's."""
    from sessionsimilaritysearch_amd import _lib
    L = _lib.lib()
    rng = np.random.default_rng(24)
    nq, n, d, k = 96, 50001, 256, 10
    q, c = _codes(rng, nq, d), _codes(rng, n, d)
    for j in range(0, nq, 4):                                 # every fourth query: 40 more copies of its best row
        best = int(np.argmax(_f(c) @ _f(q[j])))
        c[rng.choice(n, 40, replace=False)] = c[best]
    st = _lib.stream_ptr(cuda)
    tq, tc = Buf((nq, d), torch.int8, 1), Buf((n, d), torch.int8, 2)
    tq.t.copy_(torch.from_numpy(q)); tc.t.copy_(torch.from_numpy(c))
    cmax = Buf(1, torch.float32, 3, zero=True)
    _lib.check(L.sss_row_norm_max(tc.ptr, n, d, I8, cmax.ptr, st), "sss_row_norm_max")
    cm = float(cmax.t.item())
    exact_max = float(np.sqrt((_f(c).astype(np.float64) ** 2).sum(1).max()))
    assert exact_max <= cm <= exact_max * (1 + 1e-6)
    D, I, status = Buf((nq, k), torch.float32, 4), Buf((nq, k), torch.int64, 5), Buf(nq, torch.int32, 6)
    unproven = Buf(1, torch.int32, 7, zero=True)
    nws = L.sss_ip_topk_workspace_bytes(nq, n, d, k, I8)
    assert nws > 0 and L.sss_ip_topk_workspace_bytes(nq, n, 128, k, I8) == 0 and L.sss_ip_topk_workspace_bytes(nq, n, 1600, k, I8) == 0
    ws, state = Buf(nws, torch.uint8, 8), Buf(L.sss_ip_topk_state_bytes(nq), torch.uint8, 9, zero=True)
    rc = L.sss_ip_topk(tq.ptr, nq, tc.ptr, n, d, k, I8, 0, cm, D.ptr, I.ptr, status.ptr, unproven.ptr, state.ptr, state.nbytes,
                       ws.ptr, ws.nbytes, st)
    _lib.check(rc, "sss_ip_topk")
    Dr, Ir = sr.search_exact(_f(q), _f(c), k)
    s0 = status.t.cpu().numpy()
    assert int(unproven.t.item()) == int((s0 != 0).sum()) and (s0[0::4] != 0).all()
    assert not state.bytes.any()                              # handed back zeroed
    ok = s0 == 0
    assert np.array_equal(I.t.cpu().numpy()[ok], Ir[ok]) and np.array_equal(D.t.cpu().numpy()[ok], Dr[ok])
    sel_h = np.flatnonzero(s0).astype(np.int32)
    sel = Buf(sel_h.size, torch.int32, 10)
    sel.t.copy_(torch.from_numpy(sel_h))
    nws2 = L.sss_ip_topk_threshold_workspace_bytes(sel_h.size, n, d, I8)
    assert nws2 > 0 and L.sss_ip_topk_threshold_workspace_bytes(sel_h.size, n, 128, I8) == 0
    ws2 = Buf(nws2, torch.uint8, 11)
    rc = L.sss_ip_topk_threshold(tq.ptr, sel.ptr, sel_h.size, tc.ptr, I8, tc.ptr, I8, 0, 0.0, n, d, k, 0, cm, D.ptr, I.ptr,
                                 status.ptr, ws2.ptr, ws2.nbytes, st)
    _lib.check(rc, "sss_ip_topk_threshold")
    assert not status.t.any()
    assert np.array_equal(I.t.cpu().numpy(), Ir) and np.array_equal(D.t.cpu().numpy(), Dr)
    # range search: radius = each query's 12th best score (attained: strict), counts then fill
    s = sr.canonical_scores(_f(q), _f(c))
    radius_h = np.sort(s, axis=1)[:, -12].astype(np.float32)
    radius = Buf(nq, torch.float32, 12)
    radius.t.copy_(torch.from_numpy(radius_h))
    nws3 = L.sss_range_search_workspace_bytes(nq, n, d, I8)
    assert nws3 > 0 and L.sss_range_search_workspace_bytes(nq, n, 48, I8) == 0
    ws3, counts, rstatus = Buf(nws3, torch.uint8, 13), Buf(nq, torch.int64, 14), Buf(nq, torch.int32, 15)
    rc = L.sss_range_search_count(tq.ptr, nq, tc.ptr, I8, tc.ptr, I8, 0, 0.0, n, d, radius.ptr, cm, counts.ptr, rstatus.ptr,
                                  ws3.ptr, ws3.nbytes, st)
    _lib.check(rc, "sss_range_search_count")
    el, eD, eI, _ = _range_expected(q, c, radius_h, "ip", id_offset=7)
    assert not rstatus.t.any() and np.array_equal(counts.t.cpu().numpy(), np.diff(el))
    lims = Buf(nq + 1, torch.int64, 16)
    lims.t.copy_(torch.from_numpy(el))
    rD, rI = Buf(int(el[-1]), torch.float32, 17), Buf(int(el[-1]), torch.int64, 18)
    _lib.check(L.sss_range_search_fill(nq, lims.ptr, 7, rD.ptr, rI.ptr, ws3.ptr, ws3.nbytes, st), "sss_range_search_fill")
    assert np.array_equal(rI.t.cpu().numpy(), eI) and np.array_equal(rD.t.cpu().numpy(), eD)
    torch.cuda.synchronize()
    for b in (tq, tc, cmax, D, I, status, unproven, ws, state, sel, ws2, radius, ws3, counts, rstatus, lims, rD, rI):
        assert b.guards_ok()
    assert torch.equal(tq.t.cpu(), torch.from_numpy(q)) and torch.equal(tc.t.cpu(), torch.from_numpy(c))     # inputs untouched
    # no long-row scan for int8 rows: -1 with a message, workspace size 0
    assert L.sss_ip_topk_long_workspace_bytes(nq, n, 1600, I8) == 0
    rc = L.sss_ip_topk_long(tq.ptr, nq, tc.ptr, I8, tc.ptr, 0, 0.0, n, d, k, 0, cm, D.ptr, I.ptr, status.ptr, ws.ptr, ws.nbytes, st)
    assert rc == -1 and b"int8" in L.sss_last_error()
    # the exhaustive entry points take the code too (any d % 16 == 0), with and without a bound
    qs = Buf(4, torch.int32, 19)
    qs.t.copy_(torch.tensor([0, 5, 17, 95], dtype=torch.int32))
    wse = Buf(L.sss_ip_topk_exhaustive_workspace_bytes(4, n), torch.uint8, 20)
    D.t.fill_(0); I.t.fill_(0)
    rc = L.sss_ip_topk_exhaustive(tq.ptr, qs.ptr, 4, tc.ptr, n, d, k, I8, 0, 0, D.ptr, I.ptr, wse.ptr, wse.nbytes, st)
    _lib.check(rc, "sss_ip_topk_exhaustive")
    rows = [0, 5, 17, 95]
    assert np.array_equal(I.t.cpu().numpy()[rows], Ir[rows]) and np.array_equal(D.t.cpu().numpy()[rows], Dr[rows])
    lb = Buf(4, torch.float32, 21)
    lb.t.copy_(torch.from_numpy(np.ascontiguousarray(Dr[rows, k - 1])))
    D.t.fill_(0); I.t.fill_(0)
    rc = L.sss_ip_topk_exhaustive_lb(tq.ptr, qs.ptr, 4, tc.ptr, n, d, k, I8, 0, lb.ptr, D.ptr, I.ptr, wse.ptr, wse.nbytes, st)
    _lib.check(rc, "sss_ip_topk_exhaustive_lb")
    assert np.array_equal(I.t.cpu().numpy()[rows], Ir[rows]) and np.array_equal(D.t.cpu().numpy()[rows], Dr[rows])
    torch.cuda.synchronize()
    assert qs.guards_ok() and wse.guards_ok() and lb.guards_ok() and D.guards_ok() and I.guards_ok()


# ------------------------------------------------------------------------------------------ 8. sharding
@pytest.mark.parametrize("shards", [1, 2, 4])
def test_shard_merge_equals_single_index(cuda, shards):
    """Row-sharding invariant: merged per-shard top-k (ShardedFlatIndex's engine + sss_topk_merge) == one index, and the
    per-shard range results concatenated == the single index's."""
    from sessionsimilaritysearch_amd import _lib
    from sessionsimilaritysearch_amd.distributed import HipEngine
    from sessionsimilaritysearch_amd.index import FlatIndex
    rng = np.random.default_rng(21)
    nq, n, k = 100, 40000, 10
    q, c = _codes(rng, nq, 256), _codes(rng, n, 256)
    c[n // 2 - 3:n // 2 + 3] = c[7]                           # duplicates across a shard boundary
    single = _i8_index(c, cuda)
    Ds, Is = single.search(q, k)
    _equal((Ds, Is), sr.search_exact(_f(q), _f(c), k))
    tq = single._rows(q, "q")
    radius = np.sort(sr.canonical_scores(_f(q), _f(c)), axis=1)[:, -15].astype(np.float32)
    ls, Drs, Irs = single.range_search(q, radius)
    per = n // shards
    Dl, Il, ranges = [], [], []
    for s in range(shards):
        idx = FlatIndex(256, "ip", cuda, dtype="i8")
        idx.add(c[s * per:(s + 1) * per])
        idx.id_offset = s * per
        eng = HipEngine(idx)
        D = torch.empty((nq, k), dtype=torch.float32, device=cuda)
        I = torch.empty((nq, k), dtype=torch.int64, device=cuda)
        status = torch.empty((nq,), dtype=torch.int32, device=cuda)
        eng.local_search(tq, k, D, I, status)
        eng.fix_unproven(tq, k, D, I, status)
        Dl.append(D); Il.append(I)
        ranges.append([t.cpu().numpy() for t in eng.local_range_search(tq, radius)])
    Din, Iin = torch.stack(Dl).contiguous(), torch.stack(Il).contiguous()
    Dm, Im = torch.empty_like(Dl[0]), torch.empty_like(Il[0])
    rc = _lib.lib().sss_topk_merge(Din.data_ptr(), nq * k, Iin.data_ptr(), nq * k, shards, nq, k, Dm.data_ptr(), Im.data_ptr(),
                                   _lib.stream_ptr(cuda))
    _lib.check(rc, "sss_topk_merge")
    assert np.array_equal(Im.cpu().numpy(), Is) and np.array_equal(Dm.cpu().numpy(), Ds)
    for j in range(nq):                                       # ids ascending per query: shard after shard
        Ij = np.concatenate([r[2][r[0][j]:r[0][j + 1]] for r in ranges])
        Dj = np.concatenate([r[1][r[0][j]:r[0][j + 1]] for r in ranges])
        assert np.array_equal(Ij, Irs[ls[j]:ls[j + 1]]) and np.array_equal(Dj, Drs[ls[j]:ls[j + 1]])
