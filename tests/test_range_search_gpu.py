"""FlatIndex.range_search against the canonical oracle: every row with score > radius (inner product) or squared
distance < radius (L2), ids ascending, scores the canonical float32 ones -- lims, I and D compared with array_equal,
whichever route (fused threshold scan + re-score, or exhaustive) served a query."""
import numpy as np
import pytest
import torch

from oracle import search_ref as sr
from sessionsimilaritysearch_amd import index as ix
from sessionsimilaritysearch_amd.index import FlatIndex, build_index

pytestmark = pytest.mark.gpu


def _unit(rng, n, d):
    return sr.normalize(rng.standard_normal((n, d)).astype(np.float32)).astype(np.float32)


def _bf16(x):
    return torch.from_numpy(np.ascontiguousarray(x, np.float32)).to(torch.bfloat16).float().numpy()


def _expected(q, c, radius, metric="ip", id_offset=0, block=8192):
    """(lims, D, I) of the contract, scored chunk-wise over the corpus."""
    q = np.asarray(q, np.float32)
    r = np.broadcast_to(np.asarray(radius, np.float32).reshape(-1), (q.shape[0],))
    per_d = [[] for _ in range(q.shape[0])]
    per_i = [[] for _ in range(q.shape[0])]
    for lo in range(0, c.shape[0], block):
        s = (sr.canonical_scores if metric == "ip" else sr.canonical_l2)(q, c[lo:lo + block])
        keep = s > r[:, None] if metric == "ip" else s < r[:, None]
        for a in range(q.shape[0]):
            j = np.flatnonzero(keep[a])
            per_d[a].append(s[a, j])
            per_i[a].append(j.astype(np.int64) + lo + id_offset)
    D = [np.concatenate(x) if x else np.zeros(0, np.float32) for x in per_d]
    I = [np.concatenate(x) if x else np.zeros(0, np.int64) for x in per_i]
    lims = np.zeros(q.shape[0] + 1, np.int64)
    lims[1:] = np.cumsum([len(x) for x in I])
    return lims, np.concatenate(D).astype(np.float32), np.concatenate(I).astype(np.int64)


def _check(got, exp):
    lims, D, I = got
    el, eD, eI = exp
    assert lims.dtype == np.int64 and D.dtype == np.float32 and I.dtype == np.int64
    assert np.array_equal(lims, el), (lims[:10], el[:10])
    assert np.array_equal(I, eI)
    assert np.array_equal(D, eD)


def _radius_for(q, c, per_query, metric="ip"):
    """A float32 radius that keeps about `per_query` rows per query on average."""
    s = (sr.canonical_scores if metric == "ip" else sr.canonical_l2)(q, c[:20000])
    frac = per_query * min(1.0, 20000 / c.shape[0]) / s.shape[1]
    return np.float32(np.quantile(s, 1.0 - frac if metric == "ip" else frac))


# ------------------------------------------------------------------------------------------ 1. routes and scans
RUNG = {64: {"auto": "f32", "f16": "f32", "split": "split", "f32": "f32"},
        128: {"auto": "f16", "f16": "f16", "split": "split", "f32": "f32"},
        256: {"auto": "f16", "f16": "f16", "split": "split", "f32": "f32"},
        512: {"auto": "f16", "f16": "f16", "split": "f16", "f32": "f16"}}


@pytest.mark.parametrize("d", (64, 128, 256, 512))
@pytest.mark.parametrize("scan", ("auto", "f16", "split", "f32"))
def test_f32_index_every_scan(cuda, d, scan):
    rng = np.random.default_rng(10 + d)
    c, q = _unit(rng, 20000, d), _unit(rng, 64, d)
    idx = FlatIndex(d, "ip", cuda, scan=scan)
    idx.add(c)
    r = _radius_for(q, c, 30)
    got = idx.range_search(q, float(r))
    assert idx.last_range_scan == RUNG[d][scan] == idx.rung_scan()
    assert idx.last_range_overflow_queries == 0
    _check(got, _expected(q, c, r))
    assert got[0][-1] > 64 * 5                                  # (the radius kept something)


@pytest.mark.parametrize("d", (128, 256, 512))
def test_bf16_index_native_scan(cuda, d):
    rng = np.random.default_rng(20 + d)
    c, q = _unit(rng, 20000, d), _unit(rng, 64, d)
    idx = FlatIndex(d, "ip", cuda, dtype="bf16")
    idx.add(c)
    cb, qb = _bf16(c), _bf16(q)                                 # the contract is on the stored, rounded vectors
    r = _radius_for(qb, cb, 30)
    got = idx.range_search(q, r)
    assert idx.last_range_scan == "native"
    _check(got, _expected(qb, cb, r))


# ------------------------------------------------------------------------------------------ 2. radius on a tie
@pytest.mark.parametrize("scan", ("f16", "split", "f32"))
def test_radius_equal_to_a_duplicated_score(cuda, scan):
    rng = np.random.default_rng(30)
    c, q = _unit(rng, 6000, 128), _unit(rng, 8, 128)
    dup = (17, 900, 3000, 5999)
    c[list(dup)] = c[5]
    idx = FlatIndex(128, "ip", cuda, scan=scan)
    idx.add(c)
    s = sr.canonical_scores(q, c)
    for a in range(q.shape[0]):
        r = s[a, 5]                                              # exactly the score of row 5 and its copies
        lims, D, I = idx.range_search(q[a:a + 1], r)
        assert not set(I.tolist()) & {5, *dup}
        _check((lims, D, I), _expected(q[a:a + 1], c, r))
        below = np.nextafter(r, np.float32(-np.inf), dtype=np.float32)    # one float32 ulp lower: every copy passes
        lims, D, I = idx.range_search(q[a:a + 1], below)
        assert {5, *dup} <= set(I.tolist())
        _check((lims, D, I), _expected(q[a:a + 1], c, below))


# ------------------------------------------------------------------------------------------ 3. overflow
def test_overflowing_queries_go_exhaustive_and_stay_exact(cuda):
    rng = np.random.default_rng(40)
    base = _unit(rng, 1, 128)
    c = np.concatenate([_unit(rng, 12000, 128), np.repeat(base, 10000, axis=0), _unit(rng, 8000, 128)])
    q = _unit(rng, 40, 128)
    q[::4] = base                                                # 10 queries keep > 10000 rows (the copies of base)
    idx = FlatIndex(128, "ip", cuda)
    idx.add(c)
    exp = _expected(q, c, 0.3)
    got = idx.range_search(q, 0.3)
    assert idx.last_range_scan == "f16"
    # (a query keeps either ~10 rows or the 10000 copies and more: far from the capacity either way)
    assert idx.last_range_overflow_queries == int((np.diff(exp[0]) > 8192).sum()) >= 10
    _check(got, exp)
    # and with a low radius for some queries only (per-query radii): thousands of random rows pass
    r = np.full(40, 0.3, np.float32)
    r[1::8] = -0.2
    exp = _expected(q, c, r)
    got = idx.range_search(q, r)
    assert idx.last_range_overflow_queries == int((np.diff(exp[0]) > 8192).sum()) >= 15
    _check(got, exp)


# ------------------------------------------------------------------------------------------ 4. exhaustive-only shapes
def test_l2_metric(cuda):
    rng = np.random.default_rng(50)
    c = rng.standard_normal((6000, 128)).astype(np.float32)
    q = rng.standard_normal((32, 128)).astype(np.float32)
    idx = build_index(c, "l2", cuda)
    r = _radius_for(q, c, 25, "l2")
    got = idx.range_search(q, r)
    assert idx.last_range_scan == "" and idx.last_range_overflow_queries == 0
    _check(got, _expected(q, c, r, "l2"))
    lims, _, _ = idx.range_search(q, np.inf)                     # every row is closer than +inf
    assert np.array_equal(lims, np.arange(33) * 6000)


@pytest.mark.parametrize("d, n", ((96, 8000), (1600, 3000)))
def test_shapes_without_a_scan(cuda, d, n):
    rng = np.random.default_rng(60 + d)
    c, q = _unit(rng, n, d), _unit(rng, 16, d)
    idx = build_index(c, "ip", cuda)
    r = _radius_for(q, c, 20)
    got = idx.range_search(q, r)
    assert idx.last_range_scan == ""
    _check(got, _expected(q, c, r))


SLAB = 16384                                                     # rows per workgroup of the exhaustive count / compaction


def _slab_edge_case(metric, n):
    """(c, q, per-query radii, the copies of row 7) for the exhaustive-only route at d = 96: one call whose five queries
    keep every row, about half of them, about 20, none, and -- the radius exactly the score of a row copied to the last
    row of the first slab and the first row of the second (where n has them) -- neither copy."""
    rng = np.random.default_rng(65)
    if metric == "ip":
        c, q = _unit(rng, n, 96), _unit(rng, 5, 96)
    else:
        c, q = rng.standard_normal((n, 96)).astype(np.float32), rng.standard_normal((5, 96)).astype(np.float32)
    dup = [r for r in (100, SLAB - 1, SLAB) if r < n]
    c[dup] = c[7]
    score = sr.canonical_scores if metric == "ip" else sr.canonical_l2
    half = np.float32(0.0) if metric == "ip" else _radius_for(q[1:2], c, n // 2, "l2")
    everything, nothing = (-np.inf, np.inf) if metric == "ip" else (np.inf, -np.inf)
    r = np.array([everything, half, _radius_for(q[2:3], c, 20, metric), nothing, score(q[4:5], c[7:8])[0, 0]], np.float32)
    return c, q, r, [7] + dup


@pytest.mark.parametrize("metric, n", (("ip", SLAB - 1), ("ip", SLAB), ("ip", SLAB + 1), ("ip", 2 * SLAB + 1), ("l2", SLAB + 1)))
def test_exhaustive_route_at_slab_edges(cuda, metric, n):
    c, q, r, copies = _slab_edge_case(metric, n)
    exp = _expected(q, c, r, metric)
    counts = np.diff(exp[0])
    assert counts[0] == n and n // 4 < counts[1] < 3 * n // 4 and 0 < counts[2] < 200 and counts[3] == 0 and counts[4] > 0
    idx = build_index(c, metric, cuda)
    lims, D, I = idx.range_search(q, r)
    assert idx.last_range_scan == "" and idx.last_range_overflow_queries == 0
    _check((lims, D, I), exp)
    assert np.array_equal(I[:n], np.arange(n))                   # the query that keeps every row
    assert not set(I[lims[4]:lims[5]].tolist()) & set(copies)    # strict: a row AT the radius does not pass


# ------------------------------------------------------------------------------------------ 5. magnitudes
@pytest.mark.parametrize("kind", ("auto", "split", "f32", "bf16"))
def test_scaled_rows_and_queries(cuda, kind):
    rng = np.random.default_rng(70)
    c, q = _unit(rng, 20000, 128), _unit(rng, 32, 128)
    if kind == "bf16":
        c, q = _bf16(c), _bf16(q)
    r0 = _radius_for(q, c, 20)
    lims0, D0, I0 = _expected(q, c, r0)
    for sq, sc in ((0, 40), (0, -40), (30, 30), (-50, -50), (64, 0), (-20, 60)):
        qs, cs = np.ldexp(q, sq).astype(np.float32), np.ldexp(c, sc).astype(np.float32)
        if kind == "bf16":
            idx = FlatIndex(128, "ip", cuda, dtype="bf16")
        else:
            idx = FlatIndex(128, "ip", cuda, scan=kind)
        idx.add(cs)
        got = idx.range_search(qs, np.ldexp(r0, sq + sc))
        assert idx.last_range_scan != ""
        _check(got, (lims0, np.ldexp(D0, sq + sc).astype(np.float32), I0))


# ------------------------------------------------------------------------------------------ 6. large corpus
def test_one_million_rows(cuda):
    rng = np.random.default_rng(80)
    c = rng.standard_normal((1 << 20, 128), dtype=np.float32)
    c /= np.linalg.norm(c, axis=1, keepdims=True)
    q = _unit(rng, 48, 128)
    idx = FlatIndex(128, "ip", cuda)
    idx.add(c)
    xb = idx._xb.cpu().numpy()
    K = 1024
    Dk, Ik = sr.search_exact(q, xb, K)
    r = np.float32(0.32)
    assert (Dk[:, K - 1] <= r).all()                             # every row passing r is among the top K
    lims, D, I = idx.range_search(q, r)
    assert idx.last_range_scan == "f16" and idx.last_range_overflow_queries == 0
    el = np.zeros(49, np.int64)
    eD, eI = [], []
    for a in range(48):
        keep = Dk[a] > r
        order = np.argsort(Ik[a][keep], kind="stable")
        eD.append(Dk[a][keep][order])
        eI.append(Ik[a][keep][order])
        el[a + 1] = el[a] + keep.sum()
    _check((lims, D, I), (el, np.concatenate(eD), np.concatenate(eI)))
    counts = np.diff(lims)
    assert counts.min() >= 10 and counts.max() <= 1000, (counts.min(), counts.max())


# ------------------------------------------------------------------------------------------ 7. sizes and edge values
def test_more_queries_than_one_chunk(cuda):
    rng = np.random.default_rng(90)
    c, q = _unit(rng, 3000, 64), _unit(rng, ix.RANGE_CHUNK + 500, 64)
    idx = FlatIndex(64, "ip", cuda)
    idx.add(c)
    r = _radius_for(q[:256], c, 5)
    got = idx.range_search(q, r)
    _check(got, _expected(q, c, r))


def test_edge_values(cuda):
    rng = np.random.default_rng(100)
    c, q = _unit(rng, 10000, 128), _unit(rng, 6, 128)
    idx = FlatIndex(128, "ip", cuda)
    idx.add(c)
    lims, D, I = idx.range_search(q[:0], 0.5)                    # nq = 0
    assert np.array_equal(lims, [0]) and D.size == 0 and I.size == 0
    lims, D, I = idx.range_search(q, np.inf)                     # nothing beats +inf
    assert np.array_equal(lims, np.zeros(7, np.int64)) and D.size == 0
    got = idx.range_search(q, -np.inf)                           # every row (more than the fused capacity)
    assert np.array_equal(got[0], np.arange(7) * 10000) and idx.last_range_overflow_queries == 6
    _check(got, _expected(q, c, -np.inf))
    small = FlatIndex(128, "ip", cuda)
    small.add(c[:3000])
    got = small.range_search(q, -np.inf)                         # every row, inside the capacity: the fused route
    assert small.last_range_overflow_queries == 0
    _check(got, _expected(q, c[:3000], -np.inf))
    with pytest.raises(ValueError):
        idx.range_search(q, np.nan)
    with pytest.raises(ValueError):
        idx.range_search(q, np.array([0.1, 0.2, np.nan, 0.0, 0.0, 0.0], np.float32))
    empty = FlatIndex(128, "ip", cuda)                           # empty index
    lims, D, I = empty.range_search(q, 0.0)
    assert np.array_equal(lims, np.zeros(7, np.int64)) and D.size == 0 and I.size == 0
    with pytest.raises(ValueError):                              # wrong width, as search
        idx.range_search(q[:, :64], 0.0)


def test_adopted_index_returns_global_ids_and_tensor_io(cuda):
    rng = np.random.default_rng(110)
    c, q = _unit(rng, 5000, 256), _unit(rng, 16, 256)
    idx = FlatIndex(256, "ip", cuda).adopt(torch.from_numpy(c).to(cuda), id_offset=70000)
    r = _radius_for(q, c, 15)
    exp = _expected(q, c, r, id_offset=70000)
    lims, D, I = idx.range_search(torch.from_numpy(q).to(cuda), torch.tensor(r))
    assert all(isinstance(t, torch.Tensor) and t.is_cuda for t in (lims, D, I))
    assert lims.dtype == torch.int64 and D.dtype == torch.float32 and I.dtype == torch.int64
    _check((lims.cpu().numpy(), D.cpu().numpy(), I.cpu().numpy()), exp)
    got = idx.range_search(q, r)                                 # numpy in -> numpy out
    assert all(isinstance(a, np.ndarray) for a in got)
    _check(got, exp)


# ------------------------------------------------------------------------------------------ 8. consistency with search
def test_consistent_with_search_and_leaves_its_state_alone(cuda):
    """With each query's radius AT its k-th score, no row outside the top k can pass, so the range result is exactly the
    top-k entries scoring above the radius, in id order."""
    rng = np.random.default_rng(120)
    c, q = _unit(rng, 30000, 128), _unit(rng, 128, 128)
    idx = FlatIndex(128, "ip", cuda)
    idx.add(c)
    k = 50
    Dk, Ik = idx.search(q, k)
    state = (idx.last_scan, dict(idx._auto_level), dict(idx._auto_clean), idx.last_rescan_queries, idx.last_fallback_queries)
    r = Dk[:, k - 1].copy()
    lims, D, I = idx.range_search(q, r)
    assert state == (idx.last_scan, dict(idx._auto_level), dict(idx._auto_clean), idx.last_rescan_queries,
                     idx.last_fallback_queries)
    for a in range(q.shape[0]):
        keep = Dk[a] > r[a]
        order = np.argsort(Ik[a][keep])
        assert np.array_equal(I[lims[a]:lims[a + 1]], Ik[a][keep][order])
        assert np.array_equal(D[lims[a]:lims[a + 1]], Dk[a][keep][order])
    D2, I2 = idx.search(q, k)                                    # search itself is unchanged by the range search
    assert np.array_equal(D2, Dk) and np.array_equal(I2, Ik)
