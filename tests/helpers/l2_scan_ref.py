"""What the short-row L2 bound tests share: the oracle, numpy restatements of the scan images (scaled float16, bf16 hi|lo)
and of the documented bound ``B_l2`` (the table of its terms; ``include/sss_l2.h``), and the seeded inputs on
which one term of that bound, one of its ``+inf`` exits or the routing guard decides.  numpy and torch's CPU conversions
only, never the library: ``tests/test_l2_scan_bound_cpu.py`` proves on the host that each input is what it claims to be,
``tests/test_l2_scan_bound_gpu.py`` searches the same arrays.  Constructors are cached and their arrays read-only."""
import functools
import math

import numpy as np
import torch

from oracle import search_ref as sr
from l2_long_ref import _directions, _equal, _scatter, exact_l2, f16_residual_norms, f16_shift  # noqa: F401

K = 10
SECOND_CHANCE = 32          # rows the wave-per-query select re-scores at most (k <= 16): rank 33 is the first one beyond
RUNG_CAPACITY = 8192        # rows a query may keep in the threshold rung
GUARD_MIN, GUARD_MAX = 2.0 ** -60, 2.0 ** 60
F32_MIN_NORMAL = 2.0 ** -126
KERNELS_128 = (("f32", 128), ("split", 128), ("f16", 128))
KERNELS_WIDE = (("f32", 64), ("split", 256), ("f16", 512))
KERNELS = KERNELS_128 + KERNELS_WIDE


def oracle(q, c, k):
    return sr.topk_from_scores(sr.canonical_l2(q, c), k, largest=False)


_answers = {}


def answer(key, q, c, k=K):
    """The oracle's answer of a named input, computed once."""
    if (key, k) not in _answers:
        _answers[key, k] = oracle(q, c, k)
    return _answers[key, k]


def ldexp32(x, s):
    return np.ldexp(np.asarray(x, np.float32), s).astype(np.float32)


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


def norms(x):
    return np.linalg.norm(np.asarray(x, np.float32).astype(np.float64), axis=1)


def in_guard(c):
    """The routing guard (routing.py: L2_SCAN_MIN_NORM / L2_SCAN_MAX_NORM) restated on float64 norms."""
    return GUARD_MIN <= norms(c).max() <= GUARD_MAX


# ------------------------------------------------------------------------------------------------ the scan images
def f16_image(x, shift):
    """The scaled float16 image in the rows' own units, float64: f16(x 2^shift) 2^-shift."""
    return np.ldexp(np.ldexp(np.asarray(x, np.float32), shift).astype(np.float16).astype(np.float64), -shift)


def rne_bf16(x):
    return torch.from_numpy(np.array(x, np.float32)).to(torch.bfloat16).float().numpy()


def split_image(x):
    """(hi, lo) of the bf16 hi|lo image: hi = rne_bf16(x), lo = rne_bf16(x - hi), the subtraction in float32."""
    x = np.ascontiguousarray(x, np.float32)
    hi = rne_bf16(x)
    return hi, rne_bf16(x - hi)


# ------------------------------------------------------------------------------------------------ the documented bound
def _ip_bound(scan, d, qn, cmax, c_resid, q_resid):
    """The inner-product bound of the scan that ran, for a chain of d terms, 2 % headroom included."""
    rd = math.sqrt(d)
    if scan == "f32":
        b = d * 2.0 ** -24 * qn * cmax + d * 2.0 ** -149
    elif scan == "split":
        b = (3.03 * 2.0 ** -16 + 3.0 * d * 2.0 ** -23 * 1.016) * qn * cmax + 3.0 * (2.0 * d + rd * (qn + cmax)) * 2.0 ** -126
    else:
        b = c_resid * qn + (cmax + c_resid) * q_resid + (2.0 ** -25 * rd + d * 2.0 ** -23) * qn * cmax
    return 1.02 * b


def b_l2(scan, q, c):
    """float64 [nq]: ``B_l2`` of every query as DESIGN 3 documents it -- twice (the scan's inner-product bound for d + 1
    terms + A(d + 1) cmax^2 / 2 + 2^-126 / sigma for f16), + 2^-24 cmax^2 + 2^-149 + (d + 2) 2^-53 |q|^2 +
    (d + 3) 2^-52 (|q| + cmax)^2, 2 % headroom -- and +inf where sigma leaves 2^+-120, cmax^2 sigma / 2 reaches 1e36 or
    the sum is not finite.  cmax: the largest float64 row norm, rounded up to float32."""
    q, c = np.asarray(q, np.float32), np.asarray(c, np.float32)
    d = q.shape[1]
    with np.errstate(over="ignore"):
        cmax = float(np.nextafter(np.float32(norms(c).max()), np.float32(np.inf)))
    qn2 = (q.astype(np.float64) ** 2).sum(1)
    qn = np.sqrt(qn2)
    c_resid, q_resid, sigma = 0.0, np.zeros(q.shape[0]), np.ones(q.shape[0])
    if scan == "f16":
        cshift = f16_shift(np.abs(c).max())
        c_resid = f16_residual_norms(c, cshift).max()
        qshift = np.array([f16_shift(a) for a in np.abs(q).max(1)])
        q_resid = np.array([f16_residual_norms(q[i:i + 1], int(qshift[i]))[0] for i in range(q.shape[0])])
        sigma = np.ldexp(1.0, cshift + qshift)
    d1, half = d + 1, 0.5 * cmax * cmax
    A = d1 * 2.0 ** -24 if scan == "f32" else 3.0 * d1 * 2.0 ** -23 if scan == "split" else d1 * 2.0 ** -23
    scan_term = _ip_bound(scan, d1, qn, cmax, c_resid, q_resid) + 1.02 * (A * half + (2.0 ** -126 / sigma if scan == "f16" else 0.0))
    b = 2.0 * scan_term + 1.02 * (2.0 ** -24 * cmax * cmax + 2.0 ** -149 + (d + 2) * 2.0 ** -53 * qn2 +
                                  (d + 3) * 2.0 ** -52 * (qn + cmax) ** 2)
    ok = np.isfinite(b) & (b < 1e300) & (sigma > 7.5e-37) & (sigma < 1.4e36) & (half * sigma < 1e36)
    return np.where(ok, b, np.inf)


def rank_gaps(q, c, k=K):
    """float64 [nq]: exact distance of the first row beyond the select's second chance - exact k-th distance."""
    edge = SECOND_CHANCE if k <= 16 else k + 12                     # (scan.hip: K2 = k + 12 beyond the wave-per-query select)
    dist = [np.sort(exact_l2(q[i], c)) for i in range(q.shape[0])]
    return np.array([x[edge] - x[k - 1] for x in dist])


def proof_margin(scan, q, c, k=K):
    """float64 [nq]: rank_gaps / (4 B_l2).  Above 1 the documented bound proves the query with room to spare: such a
    query deserves "no fallback"."""
    return rank_gaps(q, c, k) / (4.0 * b_l2(scan, q, c))


# ------------------------------------------------------------------------------------------------ 1. both sides scaled
GAUSS_SCALES = (-62, -40, -20, 0, 20, 40, 55)
NEAR_SCALES = (-59, -40, -20, 0, 20, 40, 59)
# Where the documented bound does NOT prove the "gauss" queries (tests/test_l2_scan_bound_cpu.py derives both): at 2^-62 the
# split scan's subnormal floors, 3 (2 (d + 1) + ...) 2^-126 a pass, are thousands of times the scaled relative terms, and the
# f16 scan's sigma = 2^(corpus shift + query shift) is 2^144: beyond 2^120, B_l2 = +inf.
GAUSS_NO_PROOF = {("split", -62): "floor", ("f16", -62): "inf"}


def _unit(rng, n, d):
    return sr.normalize(rng.standard_normal((n, d)).astype(np.float32)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def gauss(d):
    """Standard normal rows, 64 queries: more rows than the rung keeps, so "no fallbacks" says the proof did not give up."""
    rng = np.random.default_rng(1100 + d)
    n = 10_000 if d <= 128 else 9000
    return _frozen(rng.standard_normal((n, d)).astype(np.float32), rng.standard_normal((64, d)).astype(np.float32))


@functools.lru_cache(maxsize=None)
def near(d, f16):
    """Unit base rows x 40 noisy copies (noise 2e-5 for the f16 scan, else 2e-7), permuted; 64 unit queries, each half a unit off a base row of its own: the 40 copies
    of a query's nearest base row are its 40 nearest rows, all inside the scan's window.  Returns (c, q, base of each row)."""
    rng = np.random.default_rng(1200 + d + (7 if f16 else 0))
    base = _unit(rng, 250 if d == 128 else 150, d)
    c = np.repeat(base, 40, axis=0)
    c = c + (rng.standard_normal(c.shape) * (2e-5 if f16 else 2e-7)).astype(np.float32)
    order = rng.permutation(c.shape[0])
    c = np.ascontiguousarray(c[order]).astype(np.float32)
    q = sr.normalize(base[:64] + 0.5 * _unit(rng, 64, d)).astype(np.float32)     # query i leans towards base row i
    return _frozen(c, q, order // 40)                                            # (the base row of every row)


# ------------------------------------------------------------------------------------------------ 2, 3. unit rows
ONE_SIDE = [("q", s) for s in (-100, -70, -40, 40, 62)] + [("c", s) for s in (-100, -70, -40, 40, 59)]
GUARD_EDGES = (59, -59, 61, -61)
INF_EXITS = {"sigma": (-55, -75), "bias": (55, -100)}               # (corpus exponent, query exponent): f16 scan


@functools.lru_cache(maxsize=None)
def unit(d):
    """Unit-normalised rows (below the rung's capacity: a query whose rows all tie is resolved there) and 32 unit queries."""
    rng = np.random.default_rng(1300 + d)
    return _frozen(_unit(rng, 8000 if d == 128 else 5000, d), _unit(rng, 32, d))


def one_side(side, s, d=128):
    c, q = unit(d)
    return (c, ldexp32(q, s)) if side == "q" else (ldexp32(c, s), q)


# ------------------------------------------------------------------------------------------------ 4. small rows, large cmax
GIANTS, TINY_ROWS, ZERO_ROWS, DWARF_CLUSTER, PER_KIND = 3000, 2000, 10, 30, 8
DWARF_EXPONENTS = (-27, -39)


@functools.lru_cache(maxsize=None)
def small_rows(n=8000, d=128, seed=1400):
    """GIANTS standard normal rows scaled so that the largest |element| of the corpus is 3.0 (a corpus shift of 11, norms
    around 8) over: TINY_ROWS rows with elements of r.m.s. 2^-78 .. 2^-68 (their float32 bias is subnormal), ZERO_ROWS zero
    rows, and dwarfs -- elements of r.m.s. 2^(e-2) .. 2^e for e = -27 (scaled by 2^11 they fall on the f16 subnormals: 6 to
    8 bits survive) and e = -39 (below half the smallest subnormal: the image is zero).  Query 0 is the zero vector,
    queries 1 .. 8 sit next to tiny rows, 9 .. 16 and 17 .. 24 inside a cluster of DWARF_CLUSTER dwarfs c = s q + noise each
    (s log-uniform in [1/2, 2]).  Returns (c, q, info)."""
    rng = np.random.default_rng(seed)
    c = np.zeros((n, d))
    ids = _scatter(rng, n, n)
    rng.shuffle(ids)
    giants, tiny, zero = np.sort(ids[:GIANTS]), np.sort(ids[GIANTS:GIANTS + TINY_ROWS]), np.sort(ids[-ZERO_ROWS:])
    dwarfs = np.array_split(ids[GIANTS + TINY_ROWS:-ZERO_ROWS], len(DWARF_EXPONENTS))
    g = rng.standard_normal((GIANTS, d))
    c[giants] = g * (3.0 / np.abs(g).max())
    c[tiny] = _directions(rng, TINY_ROWS, d) * (np.exp2(rng.uniform(-78, -68, TINY_ROWS)) * math.sqrt(d))[:, None]
    q = np.zeros((1 + PER_KIND * (1 + len(DWARF_EXPONENTS)), d))
    aim = rng.choice(tiny, PER_KIND, replace=False)
    q[1:1 + PER_KIND] = c[aim] * (1.0 + 0.25 * rng.standard_normal((PER_KIND, 1))) + \
        _directions(rng, PER_KIND, d) * np.linalg.norm(c[aim], axis=1, keepdims=True) * 0.25
    clusters = {}
    for j, (exp, rows) in enumerate(zip(DWARF_EXPONENTS, dwarfs)):
        rows = np.sort(rows)
        c[rows] = _directions(rng, rows.size, d) * (np.exp2(rng.uniform(exp - 2, exp, rows.size)) * math.sqrt(d))[:, None]
        own = rng.choice(rows, (PER_KIND, DWARF_CLUSTER), replace=False)
        for i in range(PER_KIND):
            qi = _directions(rng, 1, d)[0] * (2.0 ** (exp - 1) * math.sqrt(d))
            s = np.exp2(rng.uniform(-1, 1, DWARF_CLUSTER))
            c[own[i]] = s[:, None] * qi[None, :] + _directions(rng, DWARF_CLUSTER, d) * (0.02 * np.linalg.norm(qi))
            q[1 + PER_KIND * (1 + j) + i] = qi
        clusters[exp] = (rows, own)
    c, q = _frozen(c.astype(np.float32), q.astype(np.float32))
    return c, q, {"giants": giants, "tiny": tiny, "zero": zero, "clusters": clusters}


# ------------------------------------------------------------------------------------------------ 5. aligned rounding
DECOYS, ALIGNED, N5, NQ5 = 200, 30, 10_000, 21


def _background(rng, n, d, nq, lo, hi):
    """Rows and queries with random directions and norms log-uniform in [lo, hi]."""
    def rows(m):
        return _directions(rng, m, d) * np.exp(rng.uniform(np.log(lo), np.log(hi), m))[:, None]
    return rows(n), rows(nq)


@functools.lru_cache(maxsize=None)
def worst_f16(n=N5, d=128, seed=1500):
    """The leading term of the f16 scan's bound, c_resid |q|.  Query 0 has positive elements of 11 significant bits (its
    own image is exact).  DECOYS rows are q0 with every element moved by +-8 f16 ulps: exact in the image, exact ties
    among themselves; ALIGNED rows are q0 with every element RAISED by 0.40 .. 0.45 ulp: the image rounds them down to q0
    itself, which lowers q.c -- the scan sees them ~0.8 2^-10 |q|^2 too far, behind every decoy, while they are the true
    neighbours.  The background (norms 0.2 .. 0.3, below |q0| ~ 0.5) leaves the corpus residual to the aligned rows."""
    rng = np.random.default_rng(seed)
    c, q = _background(rng, n, d, NQ5, 0.2, 0.3)
    q0 = np.ldexp(1.0 + rng.integers(0, 128, d) / 1024.0, rng.integers(-5, -3, d))       # 1.xxxxxxx000 b: 11 bits
    ulp = np.ldexp(1.0, np.frexp(q0)[1] - 11)                                            # the f16 spacing at each element
    q[0] = q0
    ids = _scatter(rng, n, DECOYS + ALIGNED)
    rng.shuffle(ids)
    decoys, aligned = np.sort(ids[:DECOYS]), np.sort(ids[DECOYS:])
    c[decoys] = q0[None, :] + 8.0 * ulp[None, :] * rng.choice([-1.0, 1.0], (DECOYS, d))
    c[aligned] = q0[None, :] + ulp[None, :] * (rng.integers(410, 461, (ALIGNED, d)) / 1024.0)
    c, q = _frozen(c.astype(np.float32), q.astype(np.float32))
    return c, q, {"decoys": decoys, "aligned": aligned}


@functools.lru_cache(maxsize=None)
def worst_split(n=N5, d=128, seed=1501):
    """The same for the bf16 hi|lo image.  Query 0: positive elements q = (1 + j/128) 2^e, j = 2 .. 16 -- 8 significant
    bits: hi = q, lo = 0.  ALIGNED rows are q + L + r with L = (1 + a/128) 2^(e-9), a < 64 (8 bits, below half a bf16 ulp of
    q: hi = q, lo = L) and r = 0.41 .. 0.45 ulp of L: the residue x - hi - lo = r, positive like every q element.  DECOYS
    rows are q +- 1.75 2^(e-9): hi = q, lo exact, exact ties among themselves, in exact arithmetic ~1.9 times as far as
    the aligned rows -- whose scan distance is ~3 times theirs."""
    rng = np.random.default_rng(seed)
    c, q = _background(rng, n, d, NQ5, 0.2, 0.3)
    e = rng.integers(-5, -3, d)
    q0 = np.ldexp(1.0 + rng.integers(2, 17, d) / 128.0, e)
    q[0] = q0
    ids = _scatter(rng, n, DECOYS + ALIGNED)
    rng.shuffle(ids)
    decoys, aligned = np.sort(ids[:DECOYS]), np.sort(ids[DECOYS:])
    c[decoys] = q0[None, :] + np.ldexp(1.75, e - 9)[None, :] * rng.choice([-1.0, 1.0], (DECOYS, d))
    L = np.ldexp(1.0 + rng.integers(0, 64, (ALIGNED, d)) / 128.0, (e - 9)[None, :])
    c[aligned] = q0[None, :] + L + np.ldexp(rng.integers(52, 59, (ALIGNED, d)).astype(np.float64), (e - 23)[None, :])
    c, q = _frozen(c.astype(np.float32), q.astype(np.float32))
    return c, q, {"decoys": decoys, "aligned": aligned}


ULP_COPIES = 40
ULP_NORMS = (0.25, 4.0, 2.0 ** 30)


@functools.lru_cache(maxsize=None)
def ulp_copies(norm, n=N5, d=128, seed=1502):
    """The f32 scan rounds no input: ULP_COPIES scattered copies of row `base` (of norm `norm`), copy j with ONE coordinate
    j + 1 float32 ulps further from query 0 = base + w, |w| = norm / 32.  Background rows and queries have norms within
    20 % of `norm`.  Returns (c, q, info): info["base"], info["copies"], info["coordinate"]."""
    rng = np.random.default_rng(seed + 10 * ULP_NORMS.index(norm))
    c, q = _background(rng, n, d, NQ5, 0.8 * norm, 1.2 * norm)
    c, q = c.astype(np.float32), q.astype(np.float32)
    base = 5
    c[base] = (c[base].astype(np.float64) * (norm / np.linalg.norm(c[base].astype(np.float64)))).astype(np.float32)
    w = _directions(rng, 1, d)[0] * (norm / 32.0)
    q[0] = (c[base].astype(np.float64) + w).astype(np.float32)
    t = int(np.argmax(np.abs(w)))
    copies = _scatter(rng, n, ULP_COPIES, [base])
    away = -1 if (q[0, t] > c[base, t]) == (c[base, t] > 0) else 1            # steps of the magnitude that lead away from q0
    for j, row in enumerate(copies):
        c[row] = c[base]
        c[row, t:t + 1].view(np.int32)[0] += away * (j + 1)
    return (*_frozen(c, q), {"base": base, "copies": copies, "coordinate": t})
