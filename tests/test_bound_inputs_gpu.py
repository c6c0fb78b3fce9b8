"""The device-computed inputs of the scans' error bounds, held to their one-sided contracts at the edges (csrc/rowops.hip):
``sss_row_norm_max`` and the two residual maxima return a true upper bound of the exact value and stay within norm_up's own
arithmetic of it; ``sss_abs_max`` is the maximum bit for bit; ``sss_l2_row_bias`` is ONE rounding of -|c|^2 / 2; the image
builders round to nearest even on ties, into inf and into the subnormal range.  The references are rational arithmetic and bit
patterns (tests/helpers/bound_inputs_ref.py); tests/test_bound_inputs_cpu.py proves that the inputs reach their regimes.  Every
call goes to libsss through ctypes with guarded buffers, as in tests/test_abi_contract_gpu.py."""
import math
import os
import sys
from fractions import Fraction

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import bound_inputs_ref as r  # noqa: E402
from test_abi_contract_gpu import Buf, L, _st, dev_buf  # noqa: E402

pytestmark = pytest.mark.gpu

NAMES = {r.F32: "f32", r.BF16: "bf16", r.H16: "f16", r.I8: "i8"}
GROUP_IDS = [f"{NAMES[c]}-d{d}" for c, d in r.NORM_GROUPS]
INF_BITS = 0x7F800000


def _dev(x, code=r.F32):
    """The table's array in the storage format `code`, in a guarded device buffer."""
    x = np.ascontiguousarray(x)
    if code == r.BF16:
        return dev_buf(torch.from_numpy(r.bf16_bits(x).reshape(x.shape).view(np.int16)).view(torch.bfloat16))
    return dev_buf(torch.from_numpy(x))


def _scalar(call, preset=0.0):
    """One atomically maximised float: *out = preset, call(out pointer), the float32 that came back."""
    out = Buf(1, torch.float32)
    out.t[0] = float(preset)
    rc = call(out.ptr)
    assert rc == 0, (rc, L().sss_last_error())
    torch.cuda.synchronize()
    assert out.guards_ok()
    return out.t.cpu().numpy()[0]


def _bits(f):
    return int(np.array([f], np.float32).view(np.uint32)[0])


def _norm_max(x, code, preset=0.0):
    b = _dev(x, code)
    got = _scalar(lambda o: L().sss_row_norm_max(b.ptr, x.shape[0], x.shape[1], code, o, _st()), preset)
    assert b.guards_ok()
    return got


def _check_bound(what, got, S):
    """The two sides of the contract; returns got / sqrt(S) where that is a finite number."""
    lim = r.tight_limit(S)
    print(f"{what}: got {float(got)!r} got/sqrt(S) - 1 = {r.ratio(got, S) - 1:.3e}" + (" (limit: inf allowed)" if lim == math.inf else ""))
    assert r.is_upper_bound(got, S), f"{what}: {float(got)!r} lies BELOW the exact value"
    assert r.within_tight_limit(got, S), f"{what}: {float(got)!r} is above sqrt(S) (1 + 2^-23 + 2e-12) / sqrt(S) + 2^-149"
    if S == 0:
        assert _bits(got) == 0, what
    return r.ratio(got, S)


def _merge_checks(what, call, got):
    """A preset *out above the result is unchanged bit for bit; one below is raised to the same value as from zero."""
    assert got > 0 and np.isfinite(got)
    for above in (np.nextafter(got, np.float32(np.inf)), np.float32(2) * got, np.float32(np.inf)):
        assert _bits(_scalar(call, above)) == _bits(above), f"{what}: preset {float(above)!r} above the maximum changed"
    for below in (np.nextafter(got, np.float32(0)), got / np.float32(2), np.float32(r.F32_TINY)):
        assert _bits(_scalar(call, below)) == _bits(got), f"{what}: preset {float(below)!r} below the maximum"


# ------------------------------------------------------------------------------------------------ sss_row_norm_max
@pytest.mark.parametrize("code,d", r.NORM_GROUPS, ids=GROUP_IDS)
def test_row_norm_max_is_an_upper_bound_within_the_tight_limit(cuda, code, d):
    worst = (0.0, "")
    for name, x in r.norm_cases(code, d):
        S = r.max_sumsq_exact(x)
        got = _norm_max(x, code)
        what = f"row_norm_max {NAMES[code]} d={d} {name}"
        if S == math.inf or S > Fraction(r.FLT_MAX) ** 2:
            print(f"{what}: got {float(got)!r}")
            assert _bits(got) == INF_BITS, f"{what}: an infinite or overflowing row must give +inf"
            continue
        ratio = _check_bound(what, got, S)
        if S >= Fraction(r.F32_MIN_NORMAL) ** 2 and np.isfinite(got):
            worst = max(worst, (ratio, name))
    print(f"OBSERVED row_norm_max {NAMES[code]} d={d}: largest got/sqrt(S) - 1 = {worst[0] - 1:.4e} ({worst[1]})")


def test_row_norm_max_int8_row_of_norm_2_15(cuda):
    x = np.full((1, 65536), -128, np.int8)
    _check_bound("row_norm_max i8 d=65536 all -128", _norm_max(x, r.I8), Fraction(2) ** 30)


@pytest.mark.parametrize("where", ["last", "second pass"])
@pytest.mark.parametrize("code,n,d,first_pass", [(r.F32, 8192 + 5, 260, 8192), (r.F32, 524288 + 257, 4, 524288), (r.BF16, 8192 + 5, 8, 8192)],
                         ids=["f32-64lanes", "f32-1lane", "bf16"])
def test_row_norm_max_grid_stride(cuda, code, n, d, first_pass, where):
    at = n - 1 if where == "last" else first_pass
    x = r.stride_case(code, n, d, at)
    _check_bound(f"row_norm_max {NAMES[code]} n={n} d={d} planted at {at}", _norm_max(x, code), r.sumsq_exact(x[at]))


@pytest.mark.parametrize("code,d", [(r.F32, 4), (r.F32, 260), (r.BF16, 8), (r.H16, 520), (r.I8, 16)], ids=["f32-d4", "f32-d260", "bf16", "f16", "i8"])
def test_row_norm_max_merges_into_a_preset_out(cuda, code, d):
    x = r.normal_rows(code, 257, d, 0, 5)
    b = _dev(x, code)
    call = lambda o: L().sss_row_norm_max(b.ptr, x.shape[0], d, code, o, _st())
    got = _scalar(call)
    _check_bound(f"row_norm_max {NAMES[code]} d={d} from zero", got, r.max_sumsq_exact(x))
    _merge_checks(f"row_norm_max {NAMES[code]} d={d}", call, got)


# ------------------------------------------------------------------------------------------------ sss_abs_max
def _abs_max(x, preset=0.0):
    x = np.ascontiguousarray(x, np.float32)
    b = dev_buf(torch.from_numpy(x))
    got = _scalar(lambda o: L().sss_abs_max(b.ptr, x.size, o, _st()), preset)
    assert b.guards_ok()
    return got


def test_abs_max_is_the_maximum_bit_for_bit(cuda):
    f = lambda *v: np.array(v, np.float32)
    nan = np.float32(np.nan)
    assert _bits(_abs_max(f(1, -3, 2, 0.5))) == _bits(3.0)                                     # count = 4, the maximum negative
    sub = np.float32(5 * r.F32_TINY)
    assert _bits(_abs_max(f(0, 0, -sub, 0))) == _bits(sub) == 5                                # a float32 subnormal, the rest zero
    assert _bits(_abs_max(f(0, 0, r.F32_TINY, 0))) == 1
    assert _bits(_abs_max(f(-0.0, -0.0, -0.0, -0.0))) == 0                                     # -0.0 only: +0.0
    assert _bits(_abs_max(f(1, -np.inf, 2, 3))) == INF_BITS
    assert _bits(_abs_max(f(nan, 1, -2, nan))) == _bits(2.0)                                   # NaNs are ignored
    assert _bits(_abs_max(f(nan, nan, nan, nan))) == 0
    assert _bits(_abs_max(f(nan, nan, nan, nan), 0.25)) == _bits(0.25)
    rng = np.random.default_rng(2)
    x = rng.standard_normal(257 * 4).astype(np.float32)
    assert _bits(_abs_max(x)) == _bits(np.abs(x).max())


def test_abs_max_grid_stride_and_merge(cuda):
    count = 4096 * 256 * 4 + 4                                   # one float4 beyond the first pass of 4096 workgroups
    rng = np.random.default_rng(3)
    x = rng.standard_normal(count).astype(np.float32)
    top = np.float32(-(np.abs(x).max() + 1.5))
    x[-2] = top                                                  # the maximum in the last float4
    b = dev_buf(torch.from_numpy(x))
    call = lambda o: L().sss_abs_max(b.ptr, count, o, _st())
    got = _scalar(call)
    assert _bits(got) == _bits(-top) and b.guards_ok()
    _merge_checks("abs_max", call, got)


# ------------------------------------------------------------------------------------------------ residual maxima
def _image(x, shift, ds=None):
    """The library's own scaled float16 image of x ([n, d] -> [n, ds or d]), checked bit for bit against f16_of with zeros in
    the padding columns; returned as a numpy float16 array with its device buffer."""
    n, d = x.shape
    xb = dev_buf(torch.from_numpy(x))
    y = Buf((n, ds or d), torch.float16)
    y.poison(0)
    if ds is None:
        rc = L().sss_scale_f16(xb.ptr, n * d, shift, y.ptr, _st())
    else:
        rc = L().sss_pad_scale_f16(xb.ptr, n, d, ds, shift, y.ptr, _st())
    assert rc == 0, L().sss_last_error()
    torch.cuda.synchronize()
    assert y.guards_ok() and xb.guards_ok()
    img = y.t.cpu().numpy()
    want = np.zeros((n, ds or d), np.float16)
    want[:, :d] = r.f16_of(x, shift)
    assert np.array_equal(img.view(np.uint16), want.view(np.uint16)), "the image is not rne_f16(x 2^shift) | +0 padding"
    return xb, y, img


def _resid_call(xb, y, n, d, ds, shift):
    if ds is None:
        return lambda o: L().sss_f16_resid_max(xb.ptr, y.ptr, n, d, shift, o, _st())
    return lambda o: L().sss_pad_f16_resid_max(xb.ptr, y.ptr, n, d, ds, shift, o, _st())


def _resid_corpora(d):
    for scale in r.RESID_SCALES:
        yield f"x2^{scale}", r.resid_corpus(d, scale)[0]
    for odd in (1, 3):
        yield f"subnormal, {odd} odd", r.resid_subnormal_corpus(d, odd)


def _check_resid(kind, d, ds):
    worst = 0.0
    for name, x in _resid_corpora(d):
        n = x.shape[0]
        shift = int(L().sss_f16_shift(float(np.abs(x).max())))
        assert shift == r.f16_shift(np.abs(x).max())
        xb, y, img = _image(x, shift, ds)
        S = r.max_resid_sumsq_exact(x, img, shift)
        got = _scalar(_resid_call(xb, y, n, d, ds, shift))
        ratio = _check_bound(f"{kind} d={d} ds={ds} {name}", got, S)
        if name.startswith("subnormal"):
            assert S > 0 and got >= np.float32(r.F32_TINY)           # never 0: the residual is whole subnormal steps
        else:
            worst = max(worst, ratio)
    print(f"OBSERVED {kind} d={d} ds={ds}: largest got/sqrt(S) - 1 = {worst - 1:.4e}")


@pytest.mark.parametrize("d", r.PLAIN_WIDTHS)
def test_f16_resid_max_is_an_upper_bound_within_the_tight_limit(cuda, d):
    _check_resid("f16_resid_max", d, None)


@pytest.mark.parametrize("d,ds", r.PAD_SHAPES, ids=[f"{d}-{ds}" for d, ds in r.PAD_SHAPES])
def test_pad_f16_resid_max_is_an_upper_bound_within_the_tight_limit(cuda, d, ds):
    _check_resid("pad_f16_resid_max", d, ds)


@pytest.mark.parametrize("n,d,ds", [(65536 + 9, 8, None), (262144 + 17, 4, 8)], ids=["plain", "pad"])
def test_resid_max_grid_stride_and_merge(cuda, n, d, ds):
    """The only row with a residual is the last one, beyond the first pass of 16384 workgroups."""
    x, shift = r.resid_stride_case(n, d)
    assert shift == int(L().sss_f16_shift(float(np.abs(x).max())))
    xb, y, img = _image(x, shift, ds)
    call = _resid_call(xb, y, n, d, ds, shift)
    got = _scalar(call)
    _check_bound(f"resid_max grid stride n={n} d={d} ds={ds}", got, r.resid_sumsq_exact(x[-1], img[-1, :d], shift))
    _merge_checks(f"resid_max n={n} d={d} ds={ds}", call, got)


# ------------------------------------------------------------------------------------------------ sss_l2_row_bias
def _bias(x):
    n, d = x.shape
    xb = dev_buf(torch.from_numpy(x))
    out = Buf(n, torch.float32)                                  # exactly n floats between guards: nothing behind row n - 1
    out.poison(1)
    assert L().sss_l2_row_bias(xb.ptr, n, d, out.ptr, _st()) == 0, L().sss_last_error()
    torch.cuda.synchronize()
    assert out.guards_ok() and xb.guards_ok(), "a write landed behind row n - 1"
    return out.t.cpu().numpy()


def _check_bias(x, kind, exact_rows):
    got, want = _bias(x), r.bias_ref_rows(x)
    bad = np.flatnonzero(~((got == want) | (np.isnan(got) & np.isnan(want))))
    assert bad.size == 0, (bad[:5], got[bad[:5]], want[bad[:5]])
    assert (got[kind == 5] == 0).all() and np.isneginf(got[kind == 6]).all()
    worst = 0.0
    for i in exact_rows:
        if not np.isfinite(got[i]) or not x[i].any():
            continue
        S = r.sumsq_exact(x[i])
        err = abs(Fraction(float(got[i])) + S / 2)
        if S / 2 >= Fraction(r.F32_MIN_NORMAL):                   # (the observation: normal results only)
            worst = max(worst, float(err / S))
        assert err <= max(Fraction(1, 2 ** 25) * S * (1 + Fraction(1, 2 ** 20)), Fraction(1, 2 ** 150)), (i, float(err / S))
    return worst


@pytest.mark.parametrize("d", r.BIAS_WIDTHS)
def test_l2_row_bias_is_one_rounding_of_the_exact_value(cuda, d):
    """Bit equality with bias_ref on every row; independently, |bias + S / 2| <= 2^-25 S (1 + 2^-20) in rational arithmetic on
    the finite rows (below the float32 normal range the one rounding is half a subnormal step, 2^-150, instead)."""
    worst = 0.0
    for n in r.BIAS_ROWS:
        x, kind = r.bias_rows(n, d)
        worst = max(worst, _check_bias(x, kind, range(min(n, 14))))
    print(f"OBSERVED l2_row_bias d={d}: largest |bias + S/2| / S = {worst:.4e} (2^-25 = {2.0 ** -25:.4e})")


def test_l2_row_bias_grid_stride(cuda):
    n, d = r.BIAS_STRIDE
    x, kind = r.bias_rows(n, d)
    _check_bias(x, kind, range(n - 7, n))


# ------------------------------------------------------------------------------------------------ image builders at their edges
def _same_bits_or_both_nan(got_bits, want_bits, nan_mask_of):
    gn, wn = nan_mask_of(got_bits), nan_mask_of(want_bits)
    return np.array_equal(gn, wn) and np.array_equal(got_bits[~wn], want_bits[~wn])


_bf16_nan = lambda b: (b & 0x7FFF) > 0x7F80
_f16_nan = lambda b: (b & 0x7FFF) > 0x7C00


def test_image_builders_at_their_rounding_edges(cuda):
    """One block of 64 edge values (ties either way, one ulp beside them, into inf, into and inside the subnormal range, +-0,
    +-inf, NaN) through the five builders; bit for bit with the helper, NaN as NaN, lo == 0 wherever x - hi is not finite."""
    n, d, shift = 3, 64, r.EDGE_SHIFT
    x = np.tile(r.edge_block(), (n, 1))
    xb = dev_buf(torch.from_numpy(x))
    u16 = lambda buf: buf.t.cpu().view(torch.int16).numpy().view(np.uint16)
    hi_w, lo_w = r.split_ref(x)
    with np.errstate(invalid="ignore"):
        no_rem = ~np.isfinite(x - r.bf16_rne(x))
    assert no_rem.any() and (lo_w[no_rem] == 0).all()

    y = Buf((n, d), torch.bfloat16)
    assert L().sss_f32_to_bf16(xb.ptr, n * d, y.ptr, _st()) == 0
    torch.cuda.synchronize()
    assert y.guards_ok() and _same_bits_or_both_nan(u16(y), hi_w, _bf16_nan), "f32_to_bf16"

    sp = Buf((n, 2 * d), torch.bfloat16)
    assert L().sss_split_bf16(xb.ptr, n, d, sp.ptr, _st()) == 0
    torch.cuda.synchronize()
    got = u16(sp)
    assert sp.guards_ok() and _same_bits_or_both_nan(got[:, :d], hi_w, _bf16_nan), "split_bf16 hi"
    assert np.array_equal(got[:, d:], lo_w), "split_bf16 lo"

    f16_w = r.f16_of(x, shift).view(np.uint16)
    f = Buf((n, d), torch.float16)
    assert L().sss_scale_f16(xb.ptr, n * d, shift, f.ptr, _st()) == 0
    torch.cuda.synchronize()
    assert f.guards_ok() and _same_bits_or_both_nan(u16(f), f16_w, _f16_nan), "scale_f16"
    # the stale shift: an element beyond the float16 range is inf in the image, and that is what the image's norm reports
    assert np.isposinf(r.f16_of(np.float32([r.F16_TO_INF[1] * 2.0 ** -shift]), shift)).all()
    finite_rows = np.where(np.abs(x) < 1e30, x, np.float32(1))                                  # only the stale elements overflow
    fb, img = dev_buf(torch.from_numpy(finite_rows)), Buf((n, d), torch.float16)
    assert L().sss_scale_f16(fb.ptr, n * d, shift, img.ptr, _st()) == 0
    assert _bits(_scalar(lambda o: L().sss_row_norm_max(img.ptr, n, d, r.H16, o, _st()))) == INF_BITS

    # the two widening builders: the same values as rows of 12 in rows of 64
    dp, ds = 12, 64
    xp = np.ascontiguousarray(x.reshape(-1, dp))
    npad = xp.shape[0]
    pb = dev_buf(torch.from_numpy(xp))
    hi_p, lo_p = r.split_ref(xp)
    pf = Buf((npad, ds), torch.float16)
    assert L().sss_pad_scale_f16(pb.ptr, npad, dp, ds, shift, pf.ptr, _st()) == 0
    torch.cuda.synchronize()
    got = u16(pf)
    assert pf.guards_ok() and _same_bits_or_both_nan(got[:, :dp], r.f16_of(xp, shift).view(np.uint16), _f16_nan), "pad_scale_f16"
    assert not got[:, dp:].any(), "pad_scale_f16: padding columns are not +0"
    ps = Buf((npad, 2 * ds), torch.bfloat16)
    assert L().sss_pad_split_bf16(pb.ptr, npad, dp, ds, ps.ptr, _st()) == 0
    torch.cuda.synchronize()
    got = u16(ps)
    assert ps.guards_ok() and _same_bits_or_both_nan(got[:, :dp], hi_p, _bf16_nan), "pad_split_bf16 hi"
    assert np.array_equal(got[:, ds:ds + dp], lo_p), "pad_split_bf16 lo"
    assert not got[:, dp:ds].any() and not got[:, ds + dp:].any(), "pad_split_bf16: padding columns are not +0"
