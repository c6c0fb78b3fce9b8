"""The inputs of tests/test_bound_inputs_gpu.py are what they claim to be -- numpy and rational arithmetic only, no device.
Each table entry exists to make one edge of a bound input decide (``csrc/rowops.hip``: ``norm_up`` and the kernels around it);
an entry that missed its regime would leave the GPU test green and the edge untested.  Where the GPU file asserts bit equality
of the L2 row bias, the proof that every row deserves it is here."""
import math
import os
import sys
from fractions import Fraction

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import bound_inputs_ref as r  # noqa: E402

GROUP_IDS = [f"{ {0: 'f32', 1: 'bf16', 4: 'f16', 6: 'i8'}[c]}-d{d}" for c, d in r.NORM_GROUPS]


# ------------------------------------------------------------------------------------------------ the helper itself
def test_helper_roundings_on_known_values():
    bits = lambda *p: np.array(p, np.uint32).view(np.float32)
    assert r.bf16_bits(bits(0x3F808000, 0x3F818000, 0x3F808001, 0x3F817FFF, 0x7F7FFFFF, 0x00000001, 0x007FFFFF)).tolist() == \
        [0x3F80, 0x3F82, 0x3F81, 0x3F81, 0x7F80, 0x0000, 0x0080]
    assert np.isnan(r.bf16_rne(bits(0x7FC00000, 0x7F800001, 0xFFFFFFFF))).all()
    assert r.f16_of(np.float32([2049, 2051, 65519, 65520]), 0).tolist() == [2048.0, 2052.0, 65504.0, np.inf]
    assert r.f16_of(np.float32([1.0]), -25).view(np.uint16).tolist() == [0] and r.f16_of(np.float32([3.0]), -25).view(np.uint16).tolist() == [2]
    hi, lo = r.split_ref(bits(0x7F7FFFFF, 0x7F800000, 0x7FC00000, 0x3F808001))
    assert hi[:2].tolist() == [0x7F80, 0x7F80] and lo[:3].tolist() == [0, 0, 0] and (hi[3], lo[3]) == (0x3F81, 0xBB80)        # 1 + 2^-8 + 2^-23 -> hi 1 + 2^-7, lo = rne(-(2^-8 - 2^-23)) = -2^-8
    S = Fraction(2)
    assert not r.is_upper_bound(np.float32(math.sqrt(2.0)), S) and r.is_upper_bound(np.nextafter(np.float32(math.sqrt(2.0)), np.float32(2)), S)
    assert r.within_tight_limit(np.nextafter(np.float32(math.sqrt(2.0)), np.float32(2)), S)
    assert not r.within_tight_limit(np.nextafter(np.float32(math.sqrt(2.0)), np.float32(2)) + np.float32(2.0 ** -22), S)
    assert r.tight_limit(Fraction(r.FLT_MAX) ** 2) == math.inf and r.tight_limit(math.inf) == math.inf
    tiny = Fraction(r.F32_TINY)
    assert 2 * tiny <= r.tight_limit(tiny ** 2) <= 2 * tiny * (1 + Fraction(1, 2 ** 100))      # subnormal range: one step, absolute
    assert r.is_upper_bound(np.float32(np.inf), math.inf) and not r.is_upper_bound(np.float32(r.FLT_MAX), math.inf)
    for amax in (0.0, 2.0 ** -149, 2.0 ** -140, 0.999, 1.0, 3.0, 3.0e38, float("inf"), float("nan")):
        assert r.f16_shift(amax) == (0 if not (0 < amax < np.inf) else 13 - math.frexp(amax)[1])


# ------------------------------------------------------------------------------------------------ sss_row_norm_max
@pytest.mark.parametrize("code,d", r.NORM_GROUPS, ids=GROUP_IDS)
def test_norm_tables_reach_their_regimes_and_norm_up_meets_both_limits(code, d):
    """The float32 running sum of squares of the tiny rows is 0 and that of the huge rows inf; norm_up restated on the float64
    sum is an upper bound within tight_limit on every entry: the limit is reachable by the code as written."""
    names = set()
    worst = 0.0
    for name, x in r.norm_cases(code, d):
        names.add(name.split(" ", 1)[-1] if name.startswith("n") and name[1].isdigit() else name)
        assert x.shape[1] == d and d % r.PER_CHUNK[code] == 0
        if code == r.BF16:
            assert (x.view(np.uint32) & 0xFFFF == 0).all()
        if name.endswith(f"x2^{r.TINY_SCALE}"):
            assert all(r.f32_running_sumsq(row) == 0 for row in x[:3]) and x.any(1).all(), name
        if any(name.endswith(f"x2^{s}") for s in r.HUGE_SCALES):
            assert all(np.isposinf(r.f32_running_sumsq(row)) for row in x[:3]) and np.isfinite(x).all(), name
        S = r.max_sumsq_exact(x)
        if x.dtype.kind == "f" and np.isinf(x).any():
            assert S == math.inf
            continue
        ss = int((x.astype(np.int64) ** 2).sum(1).max()) if code == r.I8 else float((x.astype(np.float64) ** 2).sum(1).max())
        got = r.norm_up_py(float(ss))
        assert r.is_upper_bound(got, S) and r.within_tight_limit(got, S), (name, float(got))
        if name == "norm beyond FLT_MAX":
            assert S > Fraction(r.FLT_MAX) ** 2 and np.isposinf(got)
        if name == "all zero":
            assert S == 0 and got == 0
        if S >= Fraction(r.F32_MIN_NORMAL) ** 2 and np.isfinite(got):          # (subnormal entries: a whole step of 2^-149)
            worst = max(worst, r.ratio(got, S))
    print(f"norm_up restated, code {code} d {d}: largest got / sqrt(S) - 1 = {worst - 1:.3e}")
    assert 1 < worst <= 1 + 2.0 ** -23 + 2e-12 + 1e-15
    if code == r.F32:
        assert {"subnormal 2^-149", "subnormal k 2^-149", "2^60 among ones", "+inf and -inf", "all zero"} <= names


def test_norm_table_specials():
    """2^60 among ones: the float64 sum loses the ones, so only norm_up's headroom keeps the result above the exact norm;
    the int8 row of 65536 x -128 has the norm 2^15 exactly; a cast without the step up lies below about half the rows."""
    x = dict(r.norm_cases(r.F32, 260))["2^60 among ones"]
    S = r.max_sumsq_exact(x)
    assert S == Fraction(2) ** 120 + 259 and float((x.astype(np.float64) ** 2).sum(1).max()) == 2.0 ** 120
    assert not r.is_upper_bound(np.float32(2.0 ** 60), S) and r.is_upper_bound(r.norm_up_py(2.0 ** 120), S)
    big = np.full((1, 65536), -128, np.int8)
    assert r.max_sumsq_exact(big) == Fraction(2) ** 30
    got = r.norm_up_py(float(2 ** 30))
    assert got == np.nextafter(np.float32(32768), np.float32(np.inf)) and r.within_tight_limit(got, Fraction(2) ** 30)
    low = 0
    rows = r.normal_rows(r.F32, 64, 260, 0, 1)
    for row in rows:
        low += not r.is_upper_bound(np.float32(math.sqrt(float((row.astype(np.float64) ** 2).sum()))), r.sumsq_exact(row))
    print(f"a plain cast of the float64 norm lies below the exact norm for {low} of 64 rows at d = 260")
    assert 16 <= low <= 48


@pytest.mark.parametrize("code,n,d", [(r.F32, 8192 + 5, 260), (r.F32, 524288 + 257, 4), (r.BF16, 8192 + 5, 8)])
def test_stride_cases_plant_the_only_row_that_matters(code, n, d):
    lanes = 64
    if code == r.F32:                                                         # lane_group.h: lanes_for
        lanes = 1
        while lanes < d // 4 and lanes < 64:
            lanes *= 2
    first_pass = 2048 * (256 // lanes)                                        # rowops.hip: GRID_CAP workgroups of 256 / lanes rows
    assert n > first_pass                                                     # rows beyond one launch's first pass
    for where in (n - 1, first_pass):
        x = r.stride_case(code, n, d, where)                                 # (asserts the factor 2 itself)
        s64 = (x.astype(np.float64) ** 2).sum(1)
        assert int(np.argmax(s64)) == where and x.nbytes <= 16 * 2 ** 20


# ------------------------------------------------------------------------------------------------ residuals
@pytest.mark.parametrize("scale", r.RESID_SCALES)
@pytest.mark.parametrize("d", sorted({8, 64, 72, 520} | {d for d, _ in r.PAD_SHAPES}))
def test_resid_corpus_rows_are_what_they_claim(d, scale):
    x, info = r.resid_corpus(d, scale)
    shift = info["shift"]
    assert shift == r.f16_shift(np.abs(x).max()) and abs(shift) <= 160 and np.isfinite(x).all()
    img = r.f16_of(x, shift)
    assert 2 ** 12 <= np.abs(img.astype(np.float64)).max() < 2 ** 13
    small = np.abs(img[info["small"]].astype(np.float64))
    assert (small < 2.0 ** -14).all() and small.any()                         # float16 subnormals, not all flushed
    assert not img[info["flushed"]].any() and x[info["flushed"]].all()         # an image of zeros: the residual is the row
    back = np.ldexp(img.astype(np.float64), -shift)
    assert np.array_equal(back[info["exact"]], x[info["exact"]].astype(np.float64)) and x[info["exact"]].any()
    r64 = ((back - x.astype(np.float64)) ** 2).sum(1)
    assert int(np.argmax(r64)) not in (info["exact"], info["flushed"], info["small"])
    assert r.resid_sumsq_exact(x[info["flushed"]], img[info["flushed"]], shift) == r.sumsq_exact(x[info["flushed"]])


@pytest.mark.parametrize("odd", [1, 3])
def test_subnormal_corpus_has_a_residual_of_whole_subnormal_steps(odd):
    x = r.resid_subnormal_corpus(8, odd)
    assert (np.abs(x) < r.F32_MIN_NORMAL).all() and r.f16_shift(np.abs(x).max()) == 150
    img = r.f16_of(x, 150)
    S = r.max_resid_sumsq_exact(x, img, 150)
    assert S == odd * Fraction(r.F32_TINY) ** 2                              # the norm is sqrt(odd) 2^-149: never below one step
    got = r.norm_up_py(float(S))
    assert got >= np.float32(r.F32_TINY) and r.is_upper_bound(got, S) and r.within_tight_limit(got, S)
    assert not r.is_upper_bound(np.float32(0), S)


@pytest.mark.parametrize("n,d", [(65536 + 9, 8), (262144 + 17, 4)])
def test_resid_stride_cases_leave_the_last_row_alone_with_a_residual(n, d):
    x, shift = r.resid_stride_case(n, d)
    assert shift == r.f16_shift(np.abs(x).max()) and n > 16384 * (4 if d == 8 else 16)    # rowops.hip: 16384 workgroups of 4 / 16 rows
    back = np.ldexp(r.f16_of(x, shift).astype(np.float64), -shift)
    assert np.array_equal(back[:-1], x[:-1].astype(np.float64)) and (back[-1] != x[-1]).any()


# ------------------------------------------------------------------------------------------------ L2 row bias
def _bias_tables():
    for d in r.BIAS_WIDTHS:
        for n in r.BIAS_ROWS:
            yield n, d
    yield r.BIAS_STRIDE


def test_no_bias_row_sits_near_a_float32_rounding_boundary():
    """k_row_bias sums exact float64 squares in its own order: at most d + 3 roundings of 2^-53 each.  Every row of the
    tables (none excluded) keeps fsum's -S / 2 farther than that from the nearest float32 rounding boundary, so the kernel's
    ONE rounding to float32 must land on bias_ref bit for bit."""
    closest = np.inf
    for n, d in _bias_tables():
        x, kind = r.bias_rows(n, d)
        clear = r.bias_boundary_clearance(x)
        assert (clear > (d + 3) * 2.0 ** -53).all(), (n, d, float(clear.min()))
        closest = min(closest, float((clear / ((d + 3) * 2.0 ** -53)).min()))
        if n >= 7:
            ref = r.bias_ref_rows(x[:7])
            assert ref[5] == 0 and np.isneginf(ref[6]) and ref[1] == 0 and np.isfinite(ref[:3]).all() and ref[0] < 0
            assert 0 < -ref[2] < r.F32_MIN_NORMAL * d                          # x 2^-64: about d 2^-129, a subnormal float32
    print(f"bias tables: the closest row is {closest:.3g} times its float64 error bound away from a rounding boundary")


def test_the_abi_test_s_bias_rows_deserve_bit_equality_too():
    """tests/test_l2_scan_gpu.py: test_l2_abi_row_bias compares its 2048 x 128 rows with bias_ref bit for bit: the same condition."""
    rng = np.random.default_rng(5)                                            # test_l2_scan_gpu._small(2048, 128, 8, 5), its corpus half
    c = (rng.standard_normal((2048, 128)) * np.exp(rng.uniform(-1, 1, (2048, 1)))).astype(np.float32)
    assert (r.bias_boundary_clearance(c) > (128 + 3) * 2.0 ** -53).all()


def test_bias_ref_is_one_rounding_of_the_exact_value():
    x, _ = r.bias_rows(63, 200)
    for row in x[:3]:                                                        # N(0,1), x 2^-80, x 2^-64: the finite kinds
        S = r.sumsq_exact(row)
        b = Fraction(float(r.bias_ref(row)))
        assert abs(b + S / 2) <= max(Fraction(1, 2 ** 25) * S, Fraction(1, 2 ** 150))


# ------------------------------------------------------------------------------------------------ the rounding-edge block
def test_edge_block_values_sit_on_their_edges():
    blk = r.edge_block()
    u = blk.view(np.uint32)
    for name, t in r.BF16_TIES.items():
        assert t in u and t - 1 in u and t + 1 in u and (t | 0x80000000) in u
        lo, hi = t & 0xFFFF0000, (t & 0xFFFF0000) + 0x10000
        f = lambda p: float(np.array([p], np.uint32).view(np.float32)[0])
        assert f(t) - f(lo) == f(hi) - f(t) > 0                              # exactly halfway between two bfloat16 neighbours
        even = lo if (lo >> 16) & 1 == 0 else hi
        assert (even == lo) == (name == "even below") and int(r.bf16_bits(np.array([f(t)], np.float32))[0]) << 16 == even
        assert int(r.bf16_bits(np.array([f(t - 1)], np.float32))[0]) << 16 == lo and int(r.bf16_bits(np.array([f(t + 1)], np.float32))[0]) << 16 == hi
    for p in r.BF16_TO_INF:
        assert p in u and np.isinf(r.bf16_rne(np.array([p], np.uint32).view(np.float32))).all()
    for p in (0x00000001, 0x007FFFFF, 0x00000000, 0x80000000, 0x7F800000, 0xFF800000, 0x7FC00000, 0x7F800001):
        assert p in u
    with np.errstate(invalid="ignore"):
        scaled = np.ldexp(blk.astype(np.float64), r.EDGE_SHIFT)
    img = r.f16_of(blk, r.EDGE_SHIFT).astype(np.float64)
    at = lambda t: img[np.flatnonzero(scaled == t)[0]]
    for name, t in r.F16_TIES.items():
        assert t in scaled and -t in scaled and t - 1 == 2 * ((t - 1) // 2)    # halfway between t - 1 and t + 1, steps of 2 there
        even = t - 1 if ((t - 1) / 2) % 2 == 0 else t + 1
        assert (even == t - 1) == (name == "even below") and at(t) == even
    assert at(r.F16_ZERO_TIE) == 0 and at(3 * r.F16_ZERO_TIE) == 2.0 ** -23 and at(2.0 ** -24) == 2.0 ** -24
    assert at(r.F16_SUBNORMAL) == 3 * 2.0 ** -24 < 2.0 ** -14                  # a float16 subnormal result
    assert at(r.F16_UP_TO_MAX) == 65504 and at(65519.0) == 65504 and at(-r.F16_UP_TO_MAX) == -65504
    assert all(np.isposinf(at(t)) for t in r.F16_TO_INF) and np.isneginf(at(-r.F16_TO_INF[1]))
    hi, lo = r.split_ref(blk)
    with np.errstate(invalid="ignore"):
        rem_bad = ~np.isfinite(blk - r.bf16_rne(blk))
    assert rem_bad.sum() >= 6 and (lo[rem_bad] == 0).all()
