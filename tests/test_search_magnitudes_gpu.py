"""Exactness of FlatIndex.search far from unit magnitudes.

Metamorphic relation: scaling one side by a power of two (np.ldexp, exact) scales every float64 dot product
exactly, and -- while the top-k scores stay normal float32 and nothing overflows -- their rounding to float32 as
well.  So search(q, ldexp(c, s)) must return (ldexp(D, s), I) where (D, I) is the oracle's answer at s = 0: one
oracle call per corpus serves every scale.  Below that range (scores in the float32 subnormal range) the answer is
compared with the oracle directly.

Every scan's error bound is relative to |q| * (largest corpus row norm); these tests catch a norm that underflows
(bound 0: near ties wrongly "proven") or overflows (bound inf: every query sent to the exhaustive kernels), and an
exhaustive pre-test whose margin collapses at tiny magnitudes.  Ids and scores are compared with array_equal.
"""
import functools

import numpy as np
import pytest
import torch

from oracle import search_ref as sr

pytestmark = pytest.mark.gpu

C_SCALES = (-100, -90, -80, -72, -64, -40, 0, 40, 60, 64, 66, 80, 100)
Q_SCALES = (-100, 100)
HUGE = (64, 66, 80, 100)          # corpus norms whose float32 sum of squares overflows
SUBNORMAL = -130                  # scores in the float32 subnormal range
K = 10


def _unit(rng, n, d):
    return sr.normalize(rng.standard_normal((n, d)).astype(np.float32)).astype(np.float32)


def _bf16(x):
    return torch.from_numpy(np.ascontiguousarray(x, np.float32)).to(torch.bfloat16).float().numpy()


def _ldexp(x, s):
    return np.ldexp(np.asarray(x, np.float32), s).astype(np.float32)


@functools.lru_cache(maxsize=None)
def _corpus(kind, d, bf16):
    """(q, c, D, I): queries, corpus and the oracle's top-K at scale 0.
    near: 300 base rows x 40 copies with small noise -- scores 1e-7 .. 1e-5 apart, inside the scan's error window
    (f32 scan: noise 2e-7; f16 scan: 2e-5; bf16 index: every copy one bf16 ulp away in two coordinates)."""
    rng = np.random.default_rng(1000 + d + (7 if bf16 else 0) + len(kind))
    q = _unit(rng, 64, d)
    if kind == "unit":
        c = _unit(rng, 20000, d)
    else:
        base = _unit(rng, 300, d)
        c = np.repeat(base, 40, axis=0)
        if bf16:
            c = _bf16(c)
            bits = c.view(np.uint32)
            rows = np.arange(c.shape[0])
            for _ in range(2):
                col = rng.integers(0, d, c.shape[0])
                step = rng.choice(np.array([-(1 << 16), 1 << 16], np.int64), c.shape[0])
                bits[rows, col] = (bits[rows, col].astype(np.int64) + step).astype(np.uint32)
        else:
            noise = 2e-5 if kind == "near_f16" else 2e-7
            c = c + (rng.standard_normal(c.shape) * noise).astype(np.float32)
        c = np.ascontiguousarray(c[rng.permutation(c.shape[0])]).astype(np.float32)
    if bf16:
        q, c = _bf16(q), _bf16(c)
    D, I = sr.search_exact(q, c, K)
    return q, c, D, I


def _index(cuda, d, scan, bf16, rows):
    from sessionsimilaritysearch_amd.index import FlatIndex
    idx = FlatIndex(d, "ip", cuda, dtype="bf16" if bf16 else "f32", scan=None if bf16 else scan)
    idx.add(rows)
    return idx


# (name, d, scan, bf16 index, near-tie corpus)
ROUTES = [("f16", 128, "f16", False, "near_f16"), ("split", 128, "split", False, "near_f32"),
          ("f32", 128, "f32", False, "near_f32"), ("split64", 64, "split", False, "near_f32"),
          ("bf16", 256, "native", True, "near_bf16")]
SIDES = [("c", s) for s in C_SCALES] + [("q", s) for s in Q_SCALES]


@pytest.mark.parametrize("side,s", SIDES, ids=[f"{a}{s}" for a, s in SIDES])
@pytest.mark.parametrize("corpus", ["near", "unit"])
@pytest.mark.parametrize("route", ROUTES, ids=[r[0] for r in ROUTES])
def test_fused_scans_are_exact_at_every_magnitude(cuda, route, corpus, side, s):
    name, d, scan, bf16, near = route
    q, c, D0, I0 = _corpus(near if corpus == "near" else "unit", d, bf16)
    qs, cs = (q, _ldexp(c, s)) if side == "c" else (_ldexp(q, s), c)
    idx = _index(cuda, d, scan, bf16, cs)
    D, I = idx.search(qs, K)
    assert idx.last_scan == scan
    assert np.array_equal(I, I0) and np.array_equal(D, _ldexp(D0, s)), (name, corpus, side, s)
    if corpus == "near" and s == 0:
        assert idx.last_rescan_queries > 0               # the corpus really sits inside the scan's error window
    if corpus == "unit" and side == "c" and s in HUGE:
        assert idx.last_fallback_queries == 0            # a huge but finite corpus is still proven / resolved by the rung


@pytest.mark.parametrize("corpus", ["near", "unit"])
@pytest.mark.parametrize("route", ROUTES, ids=[r[0] for r in ROUTES])
def test_subnormal_scores_match_the_oracle(cuda, route, corpus):
    """Scores in the float32 subnormal range: no scaling relation holds; whatever the scans prove must be right."""
    name, d, scan, bf16, near = route
    q, c, _, _ = _corpus(near if corpus == "near" else "unit", d, bf16)
    cs = _ldexp(c, SUBNORMAL)
    rows = cs
    if bf16:                                             # round on the host: the index stores exactly these values
        t = torch.from_numpy(cs).to(torch.bfloat16)
        cs, rows = t.float().numpy(), t.to(cuda)
    idx = _index(cuda, d, scan, bf16, rows)
    qin = torch.from_numpy(q).to(torch.bfloat16).to(cuda) if bf16 else q
    D, I = idx.search(qin, K)
    if bf16:
        D, I = D.cpu().numpy(), I.cpu().numpy()
    Dr, Ir = sr.search_exact(q, cs, K)
    assert (np.abs(Dr[:, K - 1]) < 2.0 ** -126).any()     # the case is what it claims to be
    assert idx.last_scan == scan
    assert np.array_equal(I, Ir) and np.array_equal(D, Dr), name


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("s", C_SCALES)
def test_long_rows_are_exact_at_every_magnitude(cuda, dtype, s):
    """d = 1600 (the reference's vector width): the K-tiled long-row scan over the f16 image (f32 index) or the bf16 rows."""
    bf16 = dtype == "bf16"
    q, c, D0, I0 = _long_corpus(bf16)
    idx = _index(cuda, 1600, None, bf16, _ldexp(c, s))
    D, I = idx.search(q, 100)
    assert idx.last_scan == "long"
    assert np.array_equal(I, I0) and np.array_equal(D, _ldexp(D0, s))


@functools.lru_cache(maxsize=None)
def _long_corpus(bf16):
    rng = np.random.default_rng(77)
    q, c = _unit(rng, 16, 1600), _unit(rng, 3000, 1600)
    c[1000:1040] = c[7]                                  # exact ties inside the top 100 of some queries
    if bf16:
        q, c = _bf16(q), _bf16(c)
    D, I = sr.search_exact(q, c, 100)
    return q, c, D, I


@pytest.mark.parametrize("s", C_SCALES)
@pytest.mark.parametrize("mode", ["f16", "split", "f32"])
def test_threshold_rung_is_exact_at_every_magnitude(cuda, mode, s):
    """sss_ip_topk_threshold on every query from a loose lower bound (the k-th best of a 3 % sample): its threshold
    is lb - B - ulp, so a bound that collapses drops rows that reach the k-th score, one that overflows keeps all."""
    q, c, D0, I0 = _corpus("unit", 128, False)
    rng = np.random.default_rng(5)
    sample = np.sort(rng.choice(c.shape[0], c.shape[0] // 30, replace=False))
    Ds, _ = sr.search_exact(q, c[sample], K)
    idx = _index(cuda, 128, mode, False, _ldexp(c, s))
    nq = q.shape[0]
    tq = torch.from_numpy(q).to(cuda)
    D = torch.from_numpy(_ldexp(Ds, s)).to(cuda).contiguous()
    I = torch.full((nq, K), -7, dtype=torch.int64, device=cuda)
    status = torch.ones(nq, dtype=torch.int32, device=cuda)
    left = idx.search_threshold(tq, K, D, I, status, torch.arange(nq, device=cuda))
    assert idx.rung_scan() == mode
    done = (status == 0).cpu().numpy()
    assert done.sum() >= nq * 0.5 and left.numel() == nq - done.sum()
    assert np.array_equal(I.cpu().numpy()[done], I0[done]) and np.array_equal(D.cpu().numpy()[done], _ldexp(D0, s)[done])
    assert (I.cpu().numpy()[~done] == -7).all()


@functools.lru_cache(maxsize=None)
def _dup_corpus(d):
    """Random unit rows with two copies of every query's k-th row placed at LOWER ids: each of them ties with the
    k-th result and, by the id order, displaces it."""
    rng = np.random.default_rng(300 + d)
    q, c = _unit(rng, 32, d), _unit(rng, 4000, d)
    _, I = sr.search_exact(q, c, K)
    c2 = np.ascontiguousarray(np.concatenate([np.repeat(c[I[:, K - 1]], 2, axis=0), c]))
    D2, I2 = sr.search_exact(q, c2, K)
    return q, c2, D2, I2


@pytest.mark.parametrize("s", C_SCALES)
@pytest.mark.parametrize("d", [64, 128, 256])
def test_exhaustive_lower_bound_pretest_at_every_magnitude(cuda, d, s):
    """search_exhaustive(bounded=True) with lb = the true k-th score: its float32 pre-test may skip a row only when
    the row provably scores below lb -- never one of the duplicates that tie with it."""
    q, c, D0, I0 = _dup_corpus(d)
    idx = _index(cuda, d, "f32", False, _ldexp(c, s))
    nq = q.shape[0]
    tq = torch.from_numpy(q).to(cuda)
    D = torch.full((nq, K), -7.0, dtype=torch.float32, device=cuda)
    D[:, K - 1] = torch.from_numpy(_ldexp(D0[:, K - 1], s)).to(cuda)
    I = torch.full((nq, K), -7, dtype=torch.int64, device=cuda)
    idx.search_exhaustive(tq, K, D, I, bounded=True)
    assert np.array_equal(I.cpu().numpy(), I0) and np.array_equal(D.cpu().numpy(), _ldexp(D0, s))


@pytest.mark.parametrize("s", C_SCALES)
def test_identical_rows_resolved_by_the_exhaustive_kernels_at_every_magnitude(cuda, s):
    """280k identical rows: more ties than the threshold rung keeps, so the bounded exhaustive kernels decide."""
    from sessionsimilaritysearch_amd.index import FlatIndex
    row = _unit(np.random.default_rng(33), 1, 128)
    q = _unit(np.random.default_rng(34), 5, 128)
    Dr, _ = sr.search_exact(q, row.repeat(16, axis=0), K)
    idx = FlatIndex(128, "ip", cuda)
    idx.add(torch.from_numpy(_ldexp(row, s)).to(cuda).expand(280000, 128).contiguous())
    D, I = idx.search(q, K)
    assert np.array_equal(I, np.tile(np.arange(K), (5, 1))) and np.array_equal(D, _ldexp(Dr, s))
    assert idx.last_rescan_queries == 5 and idx.last_fallback_queries == 5


@pytest.mark.parametrize("s", [-60, -40, 0, 30, 50])
def test_l2_auto_scan_at_every_magnitude(cuda, s):
    """IndexFlatL2 as ``build_index`` makes it (``scan="auto"``), both sides scaled: distances scale by 2^(2 s).  Every scale
    keeps the largest row norm (2^3.8 at s = 0) inside the routing guard, so ``search`` takes the scan ``auto`` picks for
    k = 10 at d = 128 -- the one-pass f16 scan, not the exhaustive kernels that served this search when the test was
    written -- and the route is asserted.  (tests/test_l2_scan_bound_gpu.py takes every L2 scan through the magnitudes,
    near ties included, and the exhaustive kernels beyond the guard.)"""
    from sessionsimilaritysearch_amd.index import build_index
    rng = np.random.default_rng(9)
    q = rng.standard_normal((10, 128)).astype(np.float32)
    c = rng.standard_normal((2000, 128)).astype(np.float32)
    c[100:110] = c[5]
    qs, cs = _ldexp(q, s), _ldexp(c, s)
    idx = build_index(cs, "l2", cuda)
    assert idx.l2_scan_for(K) == "f16"
    D, I = idx.search(qs, K)
    assert idx.last_scan == "f16"
    Dr, Ir = sr.build_index(cs, "l2").search(qs, K)
    assert np.array_equal(I, Ir) and np.array_equal(D, Dr)
