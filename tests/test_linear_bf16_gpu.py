"""sss_linear_grouped_bf16 (k_linear_grouped_bf16, csrc/linear_bf16.hip) through the C ABI: exact on small integers at every
K path and tile edge, the float32 -> bfloat16 rounding of X bit for bit, the per-element error contract of
include/lowp/sss_linear_bf16.h on Gaussian data, a grouped launch against its single launches, the shared epilogue, and a
row's independence of its tile neighbours.  Every launch runs on strides wider than needed over NaN-filled buffers and
must leave everything outside y[:n, :m] untouched."""
import numpy as np
import pytest
import torch

from sessionsimilaritysearch_amd import _lib

pytestmark = pytest.mark.gpu
TOL = 1e-5                                  # times max(1, max |ref|), the project's float32 kernel tolerance
KS = [32, 64, 96, 800, 3072]                # one half chunk, one chunk, a half-chunk tail, 12.5 chunks, bert-base's widest K
SHAPES = [(1, 1), (127, 96), (129, 129), (257, 200)]     # (n, m): a 128-tile edge straddled in both directions


def bf16_round(a):
    """float32 array -> its bfloat16 rounding (torch CPU, round to nearest even) as float32."""
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).bfloat16().float().numpy()


def launch(cuda, probs, K):
    """One launch of `probs` = [dict(x [n, K] float32, w [m, K] float32 (rounded to bf16 here), bias [m] or None, act, post =
    (scale, shift) or None)]: the list of y[:n, :m] float32 arrays.  ldx = K + 4, ldw = K + 8, ldy = m + 3; x, w and y sit in
    NaN-filled buffers with a spare row, and y must come back NaN everywhere else."""
    L, keep, structs, ys = _lib.lib(), [], [], []
    for p in probs:
        n, m = p["x"].shape[0], p["w"].shape[0]
        x = torch.full((n + 1, K + 4), float("nan"), dtype=torch.float32, device=cuda)
        x[:n, :K] = torch.from_numpy(p["x"]).to(cuda)
        w = torch.full((m + 1, K + 8), float("nan"), dtype=torch.bfloat16, device=cuda)
        w[:m, :K] = torch.from_numpy(p["w"]).bfloat16().to(cuda)
        y = torch.full((n + 2, m + 3), float("nan"), dtype=torch.float32, device=cuda)
        dev = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(cuda)
        bias, post = dev(p.get("bias")), p.get("post")
        post = None if post is None else (dev(post[0]), dev(post[1]))
        keep += [x, w, bias, post]
        structs.append(_lib.linear_problem(x, w, bias, y, n, m, p.get("act", 0), post))
        ys.append(y)
    arr = (_lib.LinearProblem * len(structs))(*structs)
    rc = L.sss_linear_grouped_bf16(arr, len(structs), K, _lib.stream_ptr(cuda))
    assert rc == 0, L.sss_last_error()
    out = []
    for p, y in zip(probs, ys):
        n, m = p["x"].shape[0], p["w"].shape[0]
        y = y.cpu().numpy()
        assert np.isnan(y[n:]).all() and np.isnan(y[:, m:]).all(), "a store outside y[:n, :m]"
        out.append(y[:n, :m].copy())
    return out


@pytest.mark.parametrize("K", KS)
def test_small_integers_are_exact(cuda, K):
    """x and w integers in [-8, 8] (exact in bfloat16), every partial sum below 64 K <= 2^18 < 2^24: float32 accumulation in
    any order is exact, so y must equal the int64 product.  A wrong operand lane map, LDS swizzle, tile offset or K tail
    fails here exactly; random w is not symmetric, so a transposed output fails too."""
    rng = np.random.default_rng(K)
    for n, m in SHAPES:
        x, w = rng.integers(-8, 9, (n, K)), rng.integers(-8, 9, (m, K))
        b = rng.integers(-100, 101, m)
        ref = x.astype(np.int64) @ w.astype(np.int64).T
        got, got_b = launch(cuda, [dict(x=x.astype(np.float32), w=w.astype(np.float32))], K)[0], \
            launch(cuda, [dict(x=x.astype(np.float32), w=w.astype(np.float32), bias=b)], K)[0]
        assert np.array_equal(got.astype(np.int64), ref) and np.array_equal(got, ref.astype(np.float32)), (K, n, m)
        assert np.array_equal(got_b, (ref + b[None, :]).astype(np.float32)), (K, n, m)


def test_x_is_rounded_to_nearest_even(cuda):
    """K = M = 32, w the identity (one 1.0 per row): y[r, c] = 0 + bf16(x[r, c]) * 1 + zeros.  Rows 0..3 hold, in every
    column, finite values: bfloat16 ties that round down to even and up to even, the float32 neighbours one ulp either side
    of each tie, ordinary values and the largest finite bfloat16; they must equal x.bfloat16().float() bit for bit.
    The special rows hold ONE special value each (the rest +0, since inf * 0 = NaN would spread it): -0, +inf, -inf, NaN
    and the largest finite float32 (which rounds to +inf); there the reference is the IEEE value of the same sum,
    float64(bf16(x)) @ w^T -- a -0 product added to the +0 accumulator is +0, inf stays inf in its column and turns the
    other columns of its row into inf * 0 = NaN -- compared bit for bit, NaN by isnan.  No subnormals."""
    K = M = 32
    bits = lambda u: np.asarray(u, dtype=np.uint32).view(np.float32)
    base = np.uint32(0x3F800000) + (np.arange(8, dtype=np.uint32) << np.uint32(16))   # bf16 values 1.0, 1 + 2^-7, ...
    tie = base + np.uint32(0x8000)                                       # exactly between bf16 neighbours: even / odd alternate
    finite = np.concatenate([bits(tie), bits(tie - 1), bits(tie + 1), -bits(tie), bits(base),
                             bits([0x7F7F0000, 0xFF7F0000, 0x00800000, 0x80800000]),        # largest bf16, smallest normals
                             np.float32([0.1, -3.3, 1e-20, 7e20, 65504.0, 1 / 3])])
    rng = np.random.default_rng(5)
    x = np.zeros((4 + 6, K), dtype=np.float32)
    x[:4] = rng.permutation(np.resize(finite, 4 * K)).reshape(4, K)
    assert all(v in x[:4] for v in finite)
    specials = [(-0.0, 3), (np.inf, 0), (-np.inf, 31), (np.nan, 17), (np.finfo(np.float32).max, 8), (-np.finfo(np.float32).max, 30)]
    for i, (v, c) in enumerate(specials):
        x[4 + i, c] = v
    xb = bf16_round(x)
    assert np.array_equal(bf16_round(bits(tie)).view(np.uint32), base + (np.arange(8, dtype=np.uint32) & np.uint32(1)) * np.uint32(0x10000))
    assert np.isinf(xb[8, 8]) and np.isinf(xb[9, 30]) and np.signbit(xb[4, 3])
    with np.errstate(invalid="ignore"):
        ref = (xb.astype(np.float64) @ np.eye(M)).astype(np.float32)
    assert np.array_equal(ref[:4].view(np.uint32), xb[:4].view(np.uint32))      # finite rows: the sum is the rounded value itself
    got = launch(cuda, [dict(x=x, w=np.eye(M, dtype=np.float32))], K)[0]
    assert np.array_equal(got[:4].view(np.uint32), xb[:4].view(np.uint32))
    nan = np.isnan(ref)
    assert nan[5:10].sum() == 4 * 31 + 32 and not nan[:5].any()
    assert np.array_equal(np.isnan(got), nan)
    assert np.array_equal(got[~nan].view(np.uint32), ref[~nan].view(np.uint32))
    assert got[4, 3] == 0.0 and not np.signbit(got[4, 3]) and got[5, 0] == np.inf and got[6, 31] == -np.inf and got[8, 8] == np.inf


@pytest.mark.parametrize("K", KS)
def test_error_contract_on_gaussian_data(cuda, K):
    """x ~ N(0, 1), w ~ N(0, 1 / sqrt(K)), bias ~ N(0, 1).  Reference: the float64 product of the bfloat16-rounded operands (its
    own error, 2^-53 relative per step, is 2^-30 of the bound).  Per element
        |y - (s + bias)| <= K 2^-23 sum_k |x^_k w^_k| + 2^-23 |s + bias|."""
    rng = np.random.default_rng(100 + K)
    for n, m in SHAPES:
        x = rng.standard_normal((n, K)).astype(np.float32)
        w = (rng.standard_normal((m, K)) / np.sqrt(K)).astype(np.float32)
        b = rng.standard_normal(m).astype(np.float32)
        xb, wb = bf16_round(x).astype(np.float64), bf16_round(w).astype(np.float64)
        ref = xb @ wb.T + b.astype(np.float64)
        bound = K * 2.0 ** -23 * (np.abs(xb) @ np.abs(wb).T) + 2.0 ** -23 * np.abs(ref)
        got = launch(cuda, [dict(x=x, w=w, bias=b)], K)[0]
        err = np.abs(got.astype(np.float64) - ref)
        print(f"K={K} n={n} m={m}: max err = {err.max():.3e}, worst err / bound = {(err / bound).max():.4f}")
        assert (err <= bound).all(), (K, n, m)


def test_a_grouped_launch_equals_its_single_launches(cuda):
    """Four problems of different (n, m) in one launch -- one with n = 0, one with m = 1, one of several tiles in both
    directions, each with its own bias and activation -- equal their single-problem launches bit for bit."""
    K, rng = 96, np.random.default_rng(9)
    probs = []
    for (n, m), act in zip([(130, 140), (0, 70), (77, 1), (5, 300)], (0, 5, 2, 1)):
        probs.append(dict(x=rng.standard_normal((n, K)).astype(np.float32), w=(rng.standard_normal((m, K)) / 8).astype(np.float32),
                          bias=rng.standard_normal(m).astype(np.float32), act=act))
    together = launch(cuda, probs, K)
    assert together[1].shape == (0, 70)
    for p, y in zip(probs, together):
        alone = launch(cuda, [p], K)[0]
        assert y.shape == alone.shape and np.array_equal(y.view(np.uint32), alone.view(np.uint32))
    # and in another order, behind the empty problem
    again = launch(cuda, [probs[1], probs[3], probs[0]], K)
    assert np.array_equal(again[1], together[3]) and np.array_equal(again[2], together[0])


def test_epilogue_is_the_float32_kernels(cuda):
    """(n, m, K) = (65, 96, 32).  The pre-activation v is what the act = 0 launch writes (the same accumulation); act 1..5 and
    the post stage must be that activation of exactly these float32 values.  act = 5 is held to the bound of
    tests/test_bert_encoder_gpu.py::test_linear_grouped_exact_gelu (8 x torch's CPU float32 error + 1e-7), the others to
    TOL * max(1, max |ref|) against the float64 function; relu and sign, which round nothing, are also exact."""
    n, m, K = 65, 96, 32
    rng = np.random.default_rng(55)
    x = rng.standard_normal((n, K)).astype(np.float32)
    w = (rng.standard_normal((m, K)) * 0.5).astype(np.float32)
    b = rng.standard_normal(m).astype(np.float32)
    x[3], b[5] = 0.0, 0.0                                               # v[3, 5] = 0 exactly
    ps, pt = (1 + 0.3 * rng.standard_normal(m)).astype(np.float32), rng.standard_normal(m).astype(np.float32)
    run = lambda act, post=None: launch(cuda, [dict(x=x, w=w, bias=b, act=act, post=post)], K)[0]
    v = run(0)
    assert v[3, 5] == 0.0 and not np.isnan(v).any()
    v64 = v.astype(np.float64)
    erf = lambda a: torch.erf(torch.from_numpy(a)).numpy()
    refs = {1: np.maximum(v64, 0.0), 2: np.tanh(v64), 3: np.sign(v64), 4: np.tanh(np.tanh(v64)), 5: 0.5 * v64 * (1.0 + erf(v64 / np.sqrt(2.0)))}
    for act, ref in refs.items():
        got = run(act)
        err = float(np.abs(got - ref).max())
        if act == 5:
            bound = 8 * float(np.abs(torch.nn.functional.gelu(torch.from_numpy(v)).numpy() - ref).max()) + 1e-7
        else:
            bound = TOL * max(1.0, float(np.abs(ref).max()))
        print(f"act={act}: max err = {err:.3e}, bound {bound:.3e}")
        assert err <= bound, act
        if act in (1, 3):
            assert np.array_equal(got, ref.astype(np.float32))
        assert got[3, 5] == 0.0
    for act in (0, 2):
        ref = np.maximum(refs.get(act, v64) * ps.astype(np.float64) + pt.astype(np.float64), 0.0)
        got = run(act, (ps, pt))
        err, bound = float(np.abs(got - ref).max()), TOL * max(1.0, float(np.abs(ref).max()))
        print(f"act={act} + post: max err = {err:.3e}, bound {bound:.3e}")
        assert err <= bound and (got >= 0).all() and (got == 0).any()


def test_a_row_does_not_depend_on_its_tile_neighbours(cuda):
    """(129, 129, 96): with every other row of x replaced by NaN, rows 0, 63, 64, 127 and 128 come out bit for bit as they do
    among finite neighbours, and every other row is NaN."""
    n, m, K = 129, 129, 96
    rng = np.random.default_rng(12)
    x = rng.standard_normal((n, K)).astype(np.float32)
    w = (rng.standard_normal((m, K)) / 8).astype(np.float32)
    b = rng.standard_normal(m).astype(np.float32)
    full = launch(cuda, [dict(x=x, w=w, bias=b, act=2)], K)[0]
    rows = [0, 63, 64, 127, 128]
    alone = np.full_like(x, np.nan)
    alone[rows] = x[rows]
    got = launch(cuda, [dict(x=alone, w=w, bias=b, act=2)], K)[0]
    assert not np.isnan(full).any()
    assert np.array_equal(got[rows].view(np.uint32), full[rows].view(np.uint32))
    assert np.isnan(np.delete(got, rows, 0)).all()
