"""Exact references for the device-computed inputs of the scans' error bounds, and the case tables of the tests that hold
them to their contracts (``sessionsimilaritysearch_amd/csrc/rowops.hip``: ``norm_up``, ``k_row_norm_max``, ``k_abs_max``,
``k_f16_resid_max`` / ``k_pad_f16_resid_max``, ``k_row_bias`` and the image builders).  Plain Python and numpy, no torch
casts: rational arithmetic for the sums, bit patterns for the roundings.  ``tests/test_bound_inputs_cpu.py`` proves on the
host that each table entry is what it claims to be; ``tests/test_bound_inputs_gpu.py`` feeds the same arrays to the kernels."""
import math
from fractions import Fraction

import numpy as np

FLT_MAX = float(np.finfo(np.float32).max)
F32_MIN_NORMAL = 2.0 ** -126
F32_TINY = 2.0 ** -149                                  # the float32 subnormal step
_FLT_MAX_Q, _TINY_Q, _MIN_NORMAL_Q = Fraction(FLT_MAX), Fraction(F32_TINY), Fraction(F32_MIN_NORMAL)
# norm_up: sqrt(ss) (1 + 1e-12) rounded up to float32, ss low or high by at most d 2^-53 relative (d <= 1040 for the
# floating formats here: 6e-14 on the root; the int8 sum is exact), the root and the product one float64 rounding each:
# the float64 value is below sqrt(S) (1 + 1.1e-12), and the step up to float32 adds at most 2^-23 of it.
TIGHT_REL = Fraction(1, 2 ** 23) + Fraction(2, 10 ** 12)

# storage formats of sss_row_norm_max: code -> (numpy type of the table's arrays, elements per 16-byte chunk).  bfloat16
# rows are float32 arrays whose low 16 bits are zero.
F32, BF16, H16, I8 = 0, 1, 4, 6
PER_CHUNK = {F32: 4, BF16: 8, H16: 8, I8: 16}


# ------------------------------------------------------------------------------------------------ exact sums, the contracts
def sumsq_exact(row):
    """The row's sum of squares as a Fraction (every stored format converts to float exactly); math.inf if the row holds
    an infinity."""
    vals = [float(v) for v in np.asarray(row).ravel()]
    if any(math.isinf(v) for v in vals):
        return math.inf
    return sum((Fraction(v) ** 2 for v in vals), Fraction(0))


def max_sumsq_exact(rows):
    """max_i sumsq_exact(rows[i]) with the rational sum taken only over the rows that can hold it: a row's float64 sum of
    squares is within d 2^-53 of its exact one, so the largest exact sum is among the rows within 1e-9 of the largest
    float64 one."""
    rows = np.asarray(rows)
    if rows.dtype.kind == "f" and np.isinf(rows).any():
        return math.inf
    s64 = (rows.astype(np.float64) ** 2).sum(1)
    cand = np.flatnonzero(s64 >= s64.max() * (1 - 1e-9))
    return max(sumsq_exact(rows[i]) for i in cand)


def is_upper_bound(got, S):
    """got (a float32) >= sqrt(S), decided without any rounding."""
    got = float(got)
    if math.isnan(got):
        return False
    if math.isinf(got):
        return got > 0
    if S == math.inf:
        return False
    return got >= 0 and Fraction(got) ** 2 >= S


def _sqrt_up(S):
    """A rational >= sqrt(S), above it by less than 2^-200 relative (the only rounding in this file's limits)."""
    if S == 0:
        return Fraction(0)
    p, q = S.numerator, S.denominator
    k = max(0, 300 - (p * q).bit_length() // 2)
    return Fraction(math.isqrt(p * q << (2 * k)) + 1, q << k)


def tight_limit(S):
    """The largest value the kernels may return for a largest sum of squares S, from norm_up's own arithmetic (TIGHT_REL):
    sqrt(S) (1 + 2^-23 + 2e-12); in the float32 subnormal range, where a step is 2^-149 whatever the value, sqrt(S) +
    2^-149.  math.inf where that exceeds FLT_MAX (+inf is then a legal result) or S is infinite."""
    if S == math.inf:
        return math.inf
    r = _sqrt_up(S)
    lim = r + _TINY_Q if r < _MIN_NORMAL_Q else r * (1 + TIGHT_REL)
    return math.inf if lim > _FLT_MAX_Q else lim


def within_tight_limit(got, S):
    got, lim = float(got), tight_limit(S)
    if math.isnan(got):
        return False
    if lim == math.inf:
        return True
    return not math.isinf(got) and Fraction(got) <= lim


def ratio(got, S):
    """got / sqrt(S) as a float, for the printed observations (inf / nan where either side is 0 or infinite)."""
    got = float(got)
    if S == math.inf or math.isinf(got) or S == 0:
        return float("nan")
    return math.sqrt(float(Fraction(got) ** 2 / S))


def norm_up_py(ss):
    """rowops.hip: norm_up restated on a float64 sum of squares."""
    r = math.sqrt(ss) * (1.0 + 1e-12)
    with np.errstate(over="ignore"):
        f = np.float32(r)
    if float(f) < r:
        f = np.nextafter(f, np.float32(np.inf))
    return f


def f32_running_sumsq(row):
    """What a float32 accumulator makes of the row's squares, one element after the other."""
    acc = np.float32(0)
    with np.errstate(over="ignore", under="ignore"):
        for v in np.asarray(row, np.float32):
            acc = np.float32(acc + np.float32(v * v))
    return acc


# ------------------------------------------------------------------------------------------------ roundings
def bf16_bits(x):
    """float32 -> bfloat16 bit patterns (uint16), round to nearest even on the uint32 pattern: add 0x7FFF + bit 16, shift.
    A NaN stays a NaN (quiet bit set: the sum would carry a NaN with low payload bits only into inf)."""
    u = np.ascontiguousarray(x, np.float32).view(np.uint32).astype(np.uint64)
    r = (u + 0x7FFF + ((u >> 16) & 1)) >> 16
    nan = (u & 0x7FFFFFFF) > 0x7F800000
    return np.where(nan, (u >> 16) | 0x40, r).astype(np.uint16)


def bf16_rne(x):
    """The float32 values of bf16_bits(x)."""
    return (bf16_bits(x).astype(np.uint32) << 16).view(np.float32).reshape(np.shape(x))


def f16_of(x, shift):
    """float16 of x 2^shift: the scaling is exact in float64, then ONE rounding to nearest even."""
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        return np.ldexp(np.asarray(x, np.float32).astype(np.float64), shift).astype(np.float16)


def split_ref(x):
    """(hi, lo) bit patterns of the split image: hi = bf16_rne(x), lo = bf16_rne(x - hi) in float32, 0 where x - hi is
    not finite."""
    x = np.asarray(x, np.float32)
    hi = bf16_rne(x)
    with np.errstate(invalid="ignore", over="ignore"):
        rem = (x - hi).astype(np.float32)
    lo = bf16_bits(np.where(np.isfinite(rem), rem, np.float32(0)).astype(np.float32)).reshape(x.shape)
    return bf16_bits(x).reshape(x.shape), lo


def f16_shift(amax):
    """``sss_f16_shift`` (csrc/scan.h) restated."""
    amax = float(np.float32(amax))
    if not (amax > 0.0) or not math.isfinite(amax):
        return 0
    return 13 - math.frexp(amax)[1]


def bias_ref(row):
    """float32 of -|row|^2 / 2 with ONE rounding: the products are exact in float64, fsum is correctly rounded and the
    halving exact."""
    with np.errstate(over="ignore"):
        return np.float32(-0.5 * math.fsum(float(v) * float(v) for v in row))


def bias_ref_rows(c):
    return np.array([bias_ref(r) for r in np.asarray(c, np.float32)], np.float32)


def bias_boundary_clearance(c):
    """Per row: (distance of fsum's |row|^2 / 2 from the nearest float32 rounding boundary) / (|row|^2 / 2), inf for a
    zero row.  A float64 sum that is off by less than this relative amount rounds to the same float32."""
    c = np.asarray(c, np.float32)
    h = np.array([0.5 * math.fsum(float(v) * float(v) for v in r) for r in c])
    top = FLT_MAX + 2.0 ** 103                           # the boundary between FLT_MAX and inf
    with np.errstate(over="ignore"):
        f = h.astype(np.float32)
    fin = np.isfinite(f)
    fc = np.where(fin, f, np.float32(0))
    lo = np.nextafter(fc, np.float32(-np.inf)).astype(np.float64)
    with np.errstate(over="ignore"):
        hi = np.nextafter(fc, np.float32(np.inf)).astype(np.float64)
    f64 = fc.astype(np.float64)
    up = np.where(np.isfinite(hi), (f64 + hi) / 2, top)
    dist = np.where(fin, np.minimum(np.abs(h - (f64 + lo) / 2), np.abs(up - h)), h - top)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(h > 0, dist / h, np.inf)


# ------------------------------------------------------------------------------------------------ sss_row_norm_max tables
F32_WIDTHS = (4, 8, 12, 20, 36, 68, 132, 260, 1040)     # lane groups 1, 2, 4 .. 64, 64 + a partial pass, 64 x five passes
OTHER_WIDTHS = {BF16: (8, 520), H16: (8, 520), I8: (16, 1040)}
ROW_COUNTS = (1, 3, 257)
SCALES = (-80, -64, 0, 63, 64, 100)                     # float32 / bfloat16 rows: +-(1 + |N(0,1)|) x 2^s
TINY_SCALE, HUGE_SCALES = -80, (64, 100)                # a float32 sum of squares is 0 / inf there
NORM_GROUPS = [(F32, d) for d in F32_WIDTHS] + [(c, d) for c in (BF16, H16, I8) for d in OTHER_WIDTHS[c]]


def _seed(*key):
    return abs(hash(tuple(int(k) for k in key))) % (2 ** 31)


def normal_rows(code, n, d, scale, seed):
    rng = np.random.default_rng(seed)
    if code == I8:
        return rng.integers(-128, 128, (n, d)).astype(np.int8)
    x = rng.standard_normal((n, d))
    if code == H16:
        return (3.0 * x).astype(np.float16)
    x = np.ldexp(x + np.copysign(1.0, x), scale).astype(np.float32)        # |x| >= 2^scale: at 2^64 every single square overflows float32
    return bf16_rne(x) if code == BF16 else x


def norm_cases(code, d):
    """[(name, rows)] for one storage format and width; rows in the table's numpy type for the format."""
    out = []
    for n in ROW_COUNTS:
        if code in (F32, BF16):
            for s in SCALES:
                out.append((f"n{n} x2^{s}", normal_rows(code, n, d, s, _seed(code, d, n, s + 200))))
        else:
            out.append((f"n{n}", normal_rows(code, n, d, 0, _seed(code, d, n))))
    rng = np.random.default_rng(_seed(code, d, 7))
    if code == F32:
        out.append(("subnormal 2^-149", np.full((3, d), F32_TINY, np.float32)))
        out.append(("subnormal k 2^-149", (rng.integers(1, 2 ** 23, (3, d)) * F32_TINY).astype(np.float32)))
        if d == 4:
            out.append(("norm beyond FLT_MAX", np.full((3, d), FLT_MAX, np.float32)))
    if code == BF16:
        out.append(("subnormal 2^-133", np.full((3, d), 2.0 ** -133, np.float32)))
    if code in (F32, BF16):
        x = np.ones((3, d), np.float32)
        x[1, d // 2] = 2.0 ** 60
        out.append(("2^60 among ones", x))
    if code == H16:
        out.append(("65504", np.full((3, d), 65504.0, np.float16)))
        out.append(("2^-24", np.full((3, d), 2.0 ** -24, np.float16)))
    if code in (F32, BF16, H16):
        x = normal_rows(code, 3, d, 0, _seed(code, d, 8))
        x[0, 1], x[2, d - 1] = np.inf, -np.inf
        out.append(("+inf and -inf", x))
        x = normal_rows(code, 3, d, 0, _seed(code, d, 9))
        x[2, d - 2] = -np.inf
        out.append(("-inf alone", x))
    if code == I8:
        out.append(("all -128", np.full((3, d), -128, np.int8)))
    out.append(("all zero", np.zeros((3, d), out[0][1].dtype)))
    return out


def stride_case(code, n, d, where):
    """n rows at 2^-2 with one row at 2^2 planted at `where`: every other row has less than half its norm (asserted)."""
    x = normal_rows(code, n, d, -2, _seed(code, d, n))
    big = normal_rows(code, 1, d, 2, _seed(code, d, n, where))[0]
    x[where] = big
    norms = np.linalg.norm(x.astype(np.float64), axis=1)
    assert np.delete(norms, where).max() <= 0.5 * norms[where]
    return x


# ------------------------------------------------------------------------------------------------ residual tables
PLAIN_WIDTHS = (8, 64, 72, 520)
PAD_SHAPES = ((4, 8), (4, 64), (12, 64), (200, 256), (252, 256), (260, 512), (64, 64))
RESID_SCALES = (0, -90, 90)
FLUSHED = -40                                           # a row at 2^FLUSHED of the corpus maximum: its image is all zeros


def resid_corpus(d, scale, seed=0):
    """(rows, info): five N(0,1) x 2^scale rows; one row at 2^-30 of the largest magnitude (an image of float16 subnormals);
    one at 2^FLUSHED of it (an image of zeros: its residual is the row); one row the image holds exactly."""
    rng = np.random.default_rng(_seed(d, scale + 100, seed))
    g = np.ldexp(rng.standard_normal((5, d)), scale).astype(np.float32)
    amax = float(np.abs(g).max())
    shift = f16_shift(amax)
    small = np.ldexp(np.sign(rng.standard_normal(d)) * rng.uniform(0.5, 1.0, d) * amax, -30).astype(np.float32)
    flushed = np.ldexp(np.sign(rng.standard_normal(d)) * rng.uniform(0.5, 1.0, d) * amax, FLUSHED).astype(np.float32)
    exact = np.ldexp(rng.integers(-2047, 2048, d).astype(np.float64), -shift).astype(np.float32)
    rows = np.concatenate([g[:3], small[None], flushed[None], exact[None], g[3:]]).astype(np.float32)
    return rows, {"shift": shift, "small": 3, "flushed": 4, "exact": 5}


def resid_subnormal_corpus(d, odd):
    """float32 subnormals k 2^-149, 2048 <= k < 4096: the shift is 150, the image's step there two subnormal steps, so
    an even k is held exactly and an odd one is off by exactly 2^-149.  `odd` elements of row 1 are odd, everything else
    even: the largest residual norm is sqrt(odd) 2^-149."""
    rng = np.random.default_rng(_seed(d, odd))
    k = 2 * rng.integers(1024, 2048, (3, d))
    k[0, 0] = 4094                                      # pins the shift
    k[1, :odd] += 1
    return (k * F32_TINY).astype(np.float32)


def resid_stride_case(n, d):
    """(rows, shift): n - 1 rows the image holds exactly (multiples of 4 below 4096 in the image's units) and a last row of
    N(0,1) that pins the shift and alone has a residual."""
    rng = np.random.default_rng(_seed(n, d, 11))
    last = rng.standard_normal(d).astype(np.float32)
    shift = f16_shift(np.abs(last).max())
    x = np.ldexp(4.0 * rng.integers(-1000, 1001, (n, d)), -shift).astype(np.float32)
    x[-1] = last
    return x, shift


def resid_sumsq_exact(x_row, img_row, shift):
    """sum over the row's own columns of (h 2^-shift - x)^2, exactly."""
    sc = Fraction(2) ** -shift
    return sum(((Fraction(float(h)) * sc - Fraction(float(v))) ** 2 for v, h in zip(x_row, img_row)), Fraction(0))


def max_resid_sumsq_exact(x, img, shift):
    """The largest row's exact residual sum of squares; the rows within 1e-9 of the largest float64 one are summed exactly."""
    d = x.shape[1]
    r64 = ((np.ldexp(img[:, :d].astype(np.float64), -shift) - x.astype(np.float64)) ** 2).sum(1)
    cand = np.flatnonzero(r64 >= r64.max() * (1 - 1e-9))
    return max(resid_sumsq_exact(x[i], img[i, :d], shift) for i in cand)


# ------------------------------------------------------------------------------------------------ bias tables
BIAS_WIDTHS = (4, 8, 12, 16, 20, 200, 1600)
BIAS_ROWS = (1, 63, 65)
BIAS_KINDS = ("normal", "x2^-80", "x2^-64", "x2^63", "x2^64", "zero", "overflow")
BIAS_STRIDE = (2048 * 64 + 3, 4)


def bias_rows(n, d):
    """(rows, kind index per row): row i is of kind i % 7 -- N(0,1), the same at four scales, a zero row and a row of
    2^64 s whose -S / 2 overflows float32."""
    rng = np.random.default_rng(_seed(n, d, 3))
    kind = np.arange(n) % len(BIAS_KINDS)
    exps = np.array([0, -80, -64, 63, 64, 0, 0])[kind]
    x = np.ldexp(rng.standard_normal((n, d)), exps[:, None]).astype(np.float32)
    x[kind == 5] = 0
    x[kind == 6] = 2.0 ** 64
    return x, kind


# ------------------------------------------------------------------------------------------------ rounding-edge block
BF16_TIES = {"even below": 0x3F808000, "even above": 0x3F818000}           # halfway 0x3F80|0x3F81 and 0x3F81|0x3F82
BF16_TO_INF = (0x7F7FFFFF, 0xFF7FFFFF)
EDGE_SHIFT = 3                                          # the f16 edge values below are t 2^-EDGE_SHIFT
F16_TIES = {"even below": 2049.0, "even above": 2051.0}                     # 2048 | 2050 | 2052: steps of 2
F16_ZERO_TIE = 2.0 ** -25                               # halfway between 0 and the smallest subnormal
F16_SUBNORMAL = 3 * 2.0 ** -24 + 2.0 ** -26             # rounds to 3 x 2^-24
F16_UP_TO_MAX = 65489.0                                 # above the tie 65488 of 65472 | 65504
F16_TO_INF = (65520.0, 70000.0)                         # the tie of 65504 | 2^16 and a value beyond it: a stale shift


def edge_block():
    """64 float32 values: the bfloat16 edges by bit pattern, then the float16 edges as t 2^-EDGE_SHIFT."""
    b = []
    for t in BF16_TIES.values():
        b += [t, t | 0x80000000, t - 1, t + 1]
    b += list(BF16_TO_INF)
    b += [0x00000001, 0x007FFFFF, 0x80000001, 0x807FFFFF]                   # smallest / largest float32 subnormal
    b += [0x00000000, 0x80000000, 0x7F800000, 0xFF800000, 0x7FC00000, 0x7F800001]   # +-0, +-inf, a quiet and a low-payload NaN
    vals = np.array(b, np.uint32).view(np.float32)
    t = list(F16_TIES.values()) + [-v for v in F16_TIES.values()]
    t += [F16_ZERO_TIE, -F16_ZERO_TIE, 3 * F16_ZERO_TIE, F16_SUBNORMAL, -F16_SUBNORMAL, 2.0 ** -24, 2.0 ** -14 - 2.0 ** -25]
    t += [F16_UP_TO_MAX, -F16_UP_TO_MAX, 65519.0, 65504.0, *F16_TO_INF, -F16_TO_INF[1]]
    f16 = np.ldexp(np.array(t, np.float64), -EDGE_SHIFT).astype(np.float32)
    assert np.array_equal(np.ldexp(f16.astype(np.float64), EDGE_SHIFT), np.array(t))     # exact float32 values
    rng = np.random.default_rng(64)
    fill = rng.standard_normal(64 - len(vals) - len(f16)).astype(np.float32)
    block = np.concatenate([vals, f16, fill]).astype(np.float32)
    assert block.size == 64
    return block
