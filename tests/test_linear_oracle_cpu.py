"""The grouped GEMM's exact oracle (oracle/search_exact.c: oracle_linear_chain, oracle_fmaf) against exact rational
arithmetic: every chain step is one correctly rounded float32 fma, the bias one float32 add, in the kernel's k order.
Also shows why the oracle uses C fmaf: rounding a*b + c in float64 first and then to float32 rounds twice, and on
constructed inputs that lands on the other float32."""
from fractions import Fraction

import numpy as np
import pytest

from oracle import search_ref as sr


def _round32(q: Fraction) -> float:
    """The float32 nearest to the rational q (ties to even), as a Python float (exact in float64)."""
    if q == 0:
        return 0.0
    sign, a = (-1, -q) if q < 0 else (1, q)
    e = a.numerator.bit_length() - a.denominator.bit_length()       # 2^e <= a < 2^(e+1) after the fix-up
    if a < Fraction(2) ** e:
        e -= 1
    quantum = Fraction(2) ** (max(e, -126) - 23)                     # float32 spacing there (subnormals below 2^-126)
    n, rem = divmod(a, quantum)
    if rem > quantum / 2 or (rem == quantum / 2 and n % 2 == 1):
        n += 1
    v = n * quantum
    assert v < Fraction(2) ** 128, "overflow: not used here"
    return sign * float(v)


def _f(v) -> Fraction:
    return Fraction(float(v))


def _fma_via_f64(a, b, c):
    """The float32 fma this suite used before the oracle: a*b is exact in float64, then (a*b + c) is rounded to
    float64 and again to float32."""
    return (np.float64(a) * np.float64(b) + np.float64(c)).astype(np.float32)


def _same(x, y):
    return np.array_equal(np.asarray(x, np.float32), np.asarray(y, np.float32))


def test_fmaf_is_one_rounding_on_random_steps():
    rng = np.random.default_rng(11)
    n = 400
    scale = lambda: np.float32(2.0) ** rng.integers(-30, 30, n).astype(np.float32)
    a = (rng.standard_normal(n).astype(np.float32) * scale()).astype(np.float32)
    b = (rng.standard_normal(n).astype(np.float32) * scale()).astype(np.float32)
    c = (rng.standard_normal(n).astype(np.float32) * scale()).astype(np.float32)
    c[::7] = (-(a[::7].astype(np.float64) * b[::7]).astype(np.float32))    # near-cancellations
    got = sr.fmaf(a, b, c)
    want = np.array([_round32(_f(x) * _f(y) + _f(z)) for x, y, z in zip(a, b, c)], np.float32)
    assert _same(got, want)


def _double_rounding_cases():
    """c = 1 + odd * 2^-23 (odd float32 mantissa), a*b = 2^-24 - 2^-(24+2t) with a = 1 + 2^-t, b = (1 - 2^-t) 2^-24:
    the exact sum lies a tiny bit below the midpoint c + 2^-24 between c and its upper float32 neighbour, so one
    rounding gives c.  In float64 the sum first rounds to that midpoint (the deficit is under half a float64 ulp
    for t >= 15) and the tie then rounds to the even neighbour, c + 2^-23.  Scaled by powers of two and negated."""
    out = []
    for t in (15, 18, 21, 23):
        for odd in (1, 3, 77, 2 ** 22 - 1):
            for s in (-20, 0, 9):
                for sg in (1.0, -1.0):
                    a = np.float32(1 + 2.0 ** -t)
                    b = np.float32(sg * (1 - 2.0 ** -t) * 2.0 ** (s - 24))
                    c = np.float32(sg * (1 + odd * 2.0 ** -23) * 2.0 ** s)
                    out.append((a, b, c))
    return out


def test_fmaf_is_exact_where_float64_double_rounds():
    cases = _double_rounding_cases()
    a, b, c = (np.array(v, np.float32) for v in zip(*cases))
    exact = np.array([_round32(_f(x) * _f(y) + _f(z)) for x, y, z in cases], np.float32)
    assert _same(sr.fmaf(a, b, c), exact)
    via64 = _fma_via_f64(a, b, c)
    assert (via64 != exact).all()                                     # every constructed case double-rounds
    assert _same(exact, c)                                            # one rounding keeps c ...
    assert (np.abs(via64) > np.abs(c)).all()                          # ... two round away from it


def _chain_exact(x, w, bias):
    """The kernel's chain per element with exact rationals, rounded to float32 after every step."""
    n, K = x.shape
    m = w.shape[0]
    out = np.empty((n, m), np.float32)
    order = [k0 + 8 * u + i + 4 * h for k0 in range(0, K, 32) for u in range(4) for i in range(4) for h in range(2)]
    assert sorted(order) == list(range(K))
    for r in range(n):
        for c in range(m):
            acc = 0.0
            for k in order:
                acc = _round32(_f(x[r, k]) * _f(w[c, k]) + Fraction(acc))
            out[r, c] = _round32(Fraction(acc) + (_f(bias[c]) if bias is not None else 0))
    return out


@pytest.mark.parametrize("K,with_bias", [(32, True), (96, False), (256, True)])
def test_linear_chain_is_the_kernel_order_fmaf_chain(K, with_bias):
    rng = np.random.default_rng(K)
    n, m = 3, 4
    x = rng.standard_normal((n, K)).astype(np.float32)
    w = rng.standard_normal((m, K)).astype(np.float32)
    b = rng.standard_normal(m).astype(np.float32) if with_bias else None
    got = sr.linear_chain(x, w, b)
    assert _same(got, _chain_exact(x, w, b))
    # the order is not the plain k order: somewhere a sequential fmaf chain rounds differently
    if K == 256:
        seq = np.zeros((n, m), np.float32)
        for k in range(K):
            seq = sr.fmaf(np.repeat(x[:, k:k + 1], m, 1), np.repeat(w[None, :, k], n, 0), seq)
        seq = (seq + (b if b is not None else np.float32(0))).astype(np.float32)
        assert not _same(got, seq)


def test_linear_chain_carries_a_double_rounding_step():
    """A chain whose last step is one of the constructed cases: the oracle takes the single rounding."""
    a, b, c = _double_rounding_cases()[5]
    x = np.zeros((1, 32), np.float32)
    w = np.zeros((1, 32), np.float32)
    x[0, 0], w[0, 0] = c, np.float32(1)                               # k = 0 is the first step: acc = c
    x[0, 7], w[0, 7] = a, b                                           # k = 7 is the last step of the order
    got = sr.linear_chain(x, w)[0, 0]
    assert got == c and _fma_via_f64(a, b, c) != c
