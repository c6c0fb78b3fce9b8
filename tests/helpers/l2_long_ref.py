"""What the L2 long-row tests share: the oracle applied to blocks of rows, "varnorm" rows, the bit-equality check, and the
generators of the inputs on which one term of the scan's per-row error bound decides
(``sessionsimilaritysearch_amd/csrc/select_thr.hip``: THE PER-ROW BOUND).  numpy only: ``tests/test_l2_long_bound_cpu.py``
proves on the host that each input is what it claims to be, and ``tests/test_l2_long_bound_gpu.py`` searches the same
arrays."""
import math
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np

from oracle import search_ref as sr

ORACLE_BLOCK = 8192


def _oracle(q, c, k):
    q, c = np.ascontiguousarray(q, np.float32), np.ascontiguousarray(c, np.float32)
    if c.shape[0] <= 2 * ORACLE_BLOCK:
        return sr.build_index(c, "l2").search(q, k)

    def block(lo):
        D, I = sr.build_index(c[lo:lo + ORACLE_BLOCK], "l2").search(q, k)
        return D, np.where(I >= 0, I + lo, -1)

    with ThreadPoolExecutor(min(16, os.cpu_count() or 1)) as ex:
        parts = list(ex.map(block, range(0, c.shape[0], ORACLE_BLOCK)))
    D, I = np.concatenate([p[0] for p in parts], 1), np.concatenate([p[1] for p in parts], 1)
    order = np.lexsort((np.where(I < 0, np.iinfo(np.int64).max, I), D), axis=1)[:, :k]
    return np.take_along_axis(D, order, 1), np.take_along_axis(I, order, 1)


def _varnorm(n, d, nq, seed):
    rng = np.random.default_rng(seed)

    def rows(m):
        x = rng.standard_normal((m, d), dtype=np.float32)
        s = np.exp(rng.uniform(np.log(.25), np.log(4), m))
        return (x / np.linalg.norm(x, axis=1, keepdims=True) * s[:, None]).astype(np.float32)

    return rows(n), rows(nq)


def _equal(got, want):
    D, I = got
    Dr, Ir = want
    assert np.array_equal(I, Ir), int((I != Ir).sum())
    assert np.array_equal(D, Dr), int((D != Dr).sum())


# ------------------------------------------------------------------------------------------------ host arithmetic
def f16_shift(amax):
    """``sss_f16_shift`` (sessionsimilaritysearch_amd/csrc/scan.h) restated: the power of two that maps a largest
    magnitude into [2^12, 2^13)."""
    amax = float(np.float32(amax))
    if not (amax > 0.0) or not math.isfinite(amax):
        return 0
    return 13 - math.frexp(amax)[1]


def f16_residual_norms(c, shift):
    """Per row, the norm of what the scaled float16 image loses, in the rows' own units: |c - f16(c 2^shift) 2^-shift|."""
    c64 = np.asarray(c, np.float32).astype(np.float64)
    img = np.ldexp(np.asarray(c, np.float32), shift).astype(np.float16).astype(np.float64)
    return np.linalg.norm(c64 - np.ldexp(img, -shift), axis=1)


def exact_l2(q, c):
    """float64 [n] squared distances of ONE query: what "the exact distance" means in the conditions below."""
    diff = np.asarray(c, np.float32).astype(np.float64) - np.asarray(q, np.float32).astype(np.float64)[None, :]
    return (diff * diff).sum(1)


def _directions(rng, m, d):
    x = rng.standard_normal((m, d))
    return x / np.linalg.norm(x, axis=1, keepdims=True)


def _scatter(rng, n, m, taken=()):
    """m distinct ids spread over all tiles, none of `taken`."""
    free = np.setdiff1d(np.arange(n), np.asarray(list(taken), np.int64))
    return np.sort(rng.choice(free, m, replace=False))


# ------------------------------------------------------------------------------------------------ 1a. dwarfs under giants
GIANTS = 100
DWARF_CLUSTER = 30
DWARF_EXPONENTS = (-39, -31, -27)


def dwarfs_under_giants(exp, n=20_000, d=320, nq=16, seed=101):
    """GIANTS rows with elements of size ~1 (the largest is 3.0: a corpus shift of 11) over n - GIANTS dwarf rows whose
    elements have an r.m.s. log-uniform in [2^(exp-2), 2^exp].  Scaled by 2^11, exp = -39 lands below half the smallest f16
    subnormal (the whole image of a dwarf is zero), -31 and -27 on the f16 subnormals (4 and 8 bits left).  Query i has the
    dwarfs' scale and DWARF_CLUSTER rows c = s q + noise around it, s log-uniform in [1/2, 2]: its neighbours are the rows
    with s nearest to 1, while the bias alone (all the scan sees of a flushed row) prefers the smallest norms.
    Returns (c, q, info): info["giants"], info["clusters"] ([nq, DWARF_CLUSTER] ids), info["shift"]."""
    rng = np.random.default_rng(seed)
    rms = np.exp2(rng.uniform(exp - 2, exp, n))
    c = _directions(rng, n, d) * (rms * math.sqrt(d))[:, None]
    giants = _scatter(rng, n, GIANTS)
    g = rng.standard_normal((GIANTS, d))
    c[giants] = g * (3.0 / np.abs(g).max())
    q = _directions(rng, nq, d) * (2.0 ** (exp - 1) * math.sqrt(d))
    ids = _scatter(rng, n, nq * DWARF_CLUSTER, giants).reshape(DWARF_CLUSTER, nq).T          # (every cluster over all tiles)
    for i in range(nq):
        s = np.exp2(rng.uniform(-1, 1, DWARF_CLUSTER))
        noise = _directions(rng, DWARF_CLUSTER, d) * (0.02 * np.linalg.norm(q[i]))
        c[ids[i]] = s[:, None] * q[i][None, :] + noise
    c, q = c.astype(np.float32), q.astype(np.float32)
    return c, q, {"giants": giants, "clusters": ids, "shift": f16_shift(np.abs(c).max())}


# ------------------------------------------------------------------------------------------------ 1b. subnormal / zero bias
TINY_ROWS = 3000
ZERO_BIAS_ROWS = 100
ZERO_ROWS = 10


def subnormal_bias(n=20_000, d=320, nq=16, seed=102):
    """A varnorm corpus (largest norm ~4: the route guard passes) in which TINY_ROWS rows have elements of r.m.s. 2^-78 to
    2^-68 -- their float32 bias |c|^2 / 2 is subnormal --, ZERO_BIAS_ROWS rows have |c|^2 = 1.5 2^-150 -- a bias that rounds to
    0 while the distance from the origin, 2^-149, does not -- and ZERO_ROWS rows are the zero vector.  Query 0 is the zero
    vector, the others sit next to tiny rows.  Returns (c, q, info) with the three id lists."""
    rng = np.random.default_rng(seed)
    c, _ = _varnorm(n, d, 1, seed)
    c = c.astype(np.float64)
    ids = _scatter(rng, n, TINY_ROWS + ZERO_BIAS_ROWS + ZERO_ROWS)
    rng.shuffle(ids)
    tiny, zbias, zero = np.sort(ids[:TINY_ROWS]), np.sort(ids[TINY_ROWS:TINY_ROWS + ZERO_BIAS_ROWS]), np.sort(ids[-ZERO_ROWS:])
    c[tiny] = _directions(rng, TINY_ROWS, d) * (np.exp2(rng.uniform(-78, -68, TINY_ROWS)) * math.sqrt(d))[:, None]
    c[zbias] = _directions(rng, ZERO_BIAS_ROWS, d) * math.sqrt(1.5 * 2.0 ** -150)
    c[zero] = 0.0
    q = np.zeros((nq, d))
    aim = rng.choice(tiny, nq, replace=False)
    q[1:] = c[aim[1:]] * (1.0 + 0.25 * rng.standard_normal((nq - 1, 1))) + \
        _directions(rng, nq - 1, d) * np.linalg.norm(c[aim[1:]], axis=1, keepdims=True) * 0.25
    return c.astype(np.float32), q.astype(np.float32), {"tiny": tiny, "zero_bias": zbias, "zero": zero}


# ------------------------------------------------------------------------------------------------ 1c. near ties in the window
def near_ties(m, norm, n=20_000, d=320, nq=16, seed=103):
    """A varnorm corpus and queries; row `base` is rescaled to `norm`, query 0 is base + w with |w| = norm / 32, and m
    scattered rows are copies of base with ONE coordinate moved by (j + 1) eps away from the query.  eps makes the exact
    distances of the cluster (base and copies) span 2^-14 |q||c|: half of the 2^-13 |q||c| they must stay inside, a fraction
    of the scan's own error there.  Returns (c, q, info): info["base"], info["copies"] (ids), info["coordinate"]."""
    rng = np.random.default_rng(seed + m)
    c, q = _varnorm(n, d, nq, seed)
    c, q = c.astype(np.float64), q.astype(np.float64)
    base = 5
    c[base] *= norm / np.linalg.norm(c[base])
    w = _directions(rng, 1, d)[0] * (norm / 32.0)
    q[0] = c[base] + w
    t = int(np.argmax(np.abs(w)))
    span = 2.0 ** -14 * np.linalg.norm(q[0]) * norm
    eps = (-abs(w[t]) + math.sqrt(w[t] * w[t] + span)) / m           # 2 m eps |w_t| + (m eps)^2 = span
    copies = _scatter(rng, n, m, [base])
    for j, row in enumerate(copies):
        c[row] = c[base]
        c[row, t] -= math.copysign((j + 1) * eps, w[t])
    return c.astype(np.float32), q.astype(np.float32), {"base": base, "copies": copies, "coordinate": t}


# ------------------------------------------------------------------------------------------------ 1d. magnitudes, wide norms
def magnitude_case(name, n=20_000, d=320, nq=20, seed=104):
    """The three magnitude cases of tests/test_l2_long_gpu.py whose route stays "long", above the capacity."""
    c, q = _varnorm(n, d, nq, seed)
    if name == "both*2^40":
        return c * np.float32(2.0 ** 40), q * np.float32(2.0 ** 40)
    if name == "both*2^-40":
        return c * np.float32(2.0 ** -40), q * np.float32(2.0 ** -40)
    assert name == "shift+100"
    return (c + np.float32(100)).astype(np.float32), (q + np.float32(100)).astype(np.float32)


def wide_norms(n=20_000, d=320, nq=24, seed=105):
    """Row norms log-uniform in [2^-10, 2^10].  A third of the queries sits next to one of the smallest rows each, a third
    next to one of the largest, a third has a random direction and a norm from the same range."""
    rng = np.random.default_rng(seed)
    norms = np.exp2(rng.uniform(-10, 10, n))
    c = _directions(rng, n, d) * norms[:, None]
    order = np.argsort(norms)
    third = nq // 3
    small, large = rng.choice(order[:200], third, replace=False), rng.choice(order[-200:], third, replace=False)
    q = _directions(rng, nq, d) * np.exp2(rng.uniform(-10, 10, nq))[:, None]
    for j, row in enumerate(np.concatenate([small, large])):
        q[j] = c[row] + _directions(rng, 1, d)[0] * (0.1 * norms[row])
    return c.astype(np.float32), q.astype(np.float32), {"small": small, "large": large}


# ------------------------------------------------------------------------------------------------ 1e. the worst f16 rounding
EXACT_ROWS = 200
ROUNDED_ROWS = 30


def worst_rounding(n=20_000, d=320, nq=16, seed=106):
    """The case the leading term of P|c| is made for: every element of a row rounded the same way by almost half an f16 ulp.
    Query 0 has positive elements with 11 significant bits (its own f16 image is exact), mantissas in [1, 1.125).
    * EXACT_ROWS rows are q0 with every element moved by +-8 f16 ulps: exact in the f16 image, 2^-14-odd |q|^2 away;
    * ROUNDED_ROWS rows are q0 with every element RAISED by 0.40 to 0.45 f16 ulps: the image rounds them down to q0 itself,
      so the scan puts them ~0.8 2^-10 |q|^2 too far -- behind every exact row -- while they are the true neighbours
      (2^-22-odd |q|^2 away).
    Both kinds are scattered over a varnorm corpus.  Returns (c, q, info): info["exact"], info["rounded"] (ids)."""
    rng = np.random.default_rng(seed)
    c, q = _varnorm(n, d, nq, seed)
    c, q = c.astype(np.float64), q.astype(np.float64)
    q0 = np.ldexp(1.0 + rng.integers(0, 128, d) / 1024.0, rng.integers(-5, -3, d))      # 1.xxxxxxx000 b: 11 bits
    ulp = np.ldexp(1.0, np.frexp(q0)[1] - 11)                                           # the f16 spacing at each element
    q[0] = q0
    ids = _scatter(rng, n, EXACT_ROWS + ROUNDED_ROWS)
    rng.shuffle(ids)
    exact, rounded = np.sort(ids[:EXACT_ROWS]), np.sort(ids[EXACT_ROWS:])
    c[exact] = q0[None, :] + 8.0 * ulp[None, :] * rng.choice([-1.0, 1.0], (EXACT_ROWS, d))
    c[rounded] = q0[None, :] + ulp[None, :] * (rng.integers(410, 461, (ROUNDED_ROWS, d)) / 1024.0)
    return c.astype(np.float32), q.astype(np.float32), {"exact": exact, "rounded": rounded}


# ------------------------------------------------------------------------------------------------ 2, 3. groups of equal rows
def with_duplicates(n, d, nq, seed, group):
    """Varnorm rows in which `group` scattered rows are copies of row 17, and query 0 next to it."""
    rng = np.random.default_rng(seed)
    c, q = _varnorm(n, d, nq, seed)
    dup = _scatter(rng, n, group, [17])
    c[dup] = c[17]
    q[0] = c[17] + np.float32(0.001)
    return c, q, {"group": np.sort(np.concatenate([[17], dup]))}


def identical_nearest(m, n, d, nq, seed):
    """m identical rows -- scattered, of norm 4, query 0 next to them -- in a varnorm corpus whose other rows are all far
    from query 0 (squared distance above 9 against the group's 1e-6 d): what query 0 keeps is the group and nothing else."""
    rng = np.random.default_rng(seed)
    c, q = _varnorm(n, d, nq, seed)
    row = (_directions(rng, 1, d)[0] * 4.0).astype(np.float32)
    group = _scatter(rng, n, m)
    c[group] = row
    q[0] = row + np.float32(0.001)
    return c, q, {"group": group}


# ------------------------------------------------------------------------------------------------ 4. overlapping levels
def hot_rows(n=300_000, d=320, nq=24, copies=160, seed=107):
    """Varnorm rows, three hot rows with `copies` scattered copies each; queries 0-2 ON the hot rows (their top 100 are 100
    of the exact ties: ids ascending decide), 3-5 near them, the rest plain."""
    rng = np.random.default_rng(seed)
    c, q = _varnorm(n, d, nq, seed)
    hot = c[[11, 22, 33]].copy()
    groups = _scatter(rng, n, 3 * copies, [11, 22, 33]).reshape(copies, 3).T
    for j in range(3):
        c[groups[j]] = hot[j]
    q[:3] = hot
    q[3:6] = hot + (0.05 * np.linalg.norm(hot, axis=1, keepdims=True) * _directions(rng, 3, d)).astype(np.float32)
    return c, q, {"groups": groups}
