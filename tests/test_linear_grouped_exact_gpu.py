"""sss_linear_grouped (k_linear_grouped, csrc/linear.hip) bit for bit against the exact fma-chain oracle.

Every output element of the grouped GEMM is one k-ordered float32 fma chain (v_mfma_f32_32x32x2_f32 is an fmaf chain,
bitwise), followed by a float32 bias add and the epilogue.  ``oracle.search_ref.linear_chain`` restates that chain with C
``fmaf`` in the kernel's own k order, so the comparisons here are bit for bit: a changed k order, a crossed problem
field, a fused epilogue or a tile edge that reads the wrong row would all show.  Row strides are wider than the rows;
input padding columns, input rows past N and output guard columns / rows hold a NaN bit pattern, and the guards are
read back unchanged.
"""
import numpy as np
import pytest
import torch

from oracle import search_ref as sr
from sessionsimilaritysearch_amd import _lib

pytestmark = pytest.mark.gpu

GUARD_BITS = np.uint32(0x7FC0DEAD)           # a quiet NaN no kernel computes
# HIP device math, tanhf: 2 ulp maximum error (HIP documentation, "HIP math API" reference, table of single-precision
# mathematical functions).  Taken from the documentation, not measured here.
TANHF_ULP = 2


def _st(dev):
    return _lib.stream_ptr(dev)


def _guarded(rows, cols, ld, data=None):
    """Host float32 buffer [rows, ld] of the guard NaN; ``data`` [r, cols] goes to the top-left corner."""
    buf = np.full((rows, ld), GUARD_BITS, np.uint32).view(np.float32)
    if data is not None:
        buf[:data.shape[0], :cols] = data
    return buf


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _rand(rng, *shape):
    return rng.standard_normal(shape).astype(np.float32)


class Prob:
    """One problem of a launch: host data, its device buffers (strided, NaN padded) and its LinearProblem."""

    def __init__(self, cuda, rng, n, m, K, act=0, bias=True, post=False, gather=False, zero_rows=(), n_table=97):
        self.n, self.m, self.K, self.act, self.gather = n, m, K, act, gather
        self.ldx, self.ldw, self.ldy = K + 8, K + 4, m + 3
        self.w = _rand(rng, m, K)
        self.w[list(zero_rows)] = 0.0                                   # exactly zero pre-activations ...
        self.b = _rand(rng, m) if bias else None
        if bias:
            self.b[list(zero_rows)] = 0.0                               # ... with a zero bias
        self.post = (rng.uniform(0.25, 2.0, m).astype(np.float32), _rand(rng, m) * np.float32(0.5)) if post else None
        if gather:
            self.table = _rand(rng, n_table, K)
            ids = rng.integers(0, n_table, n).astype(np.int64)
            if n >= 3:
                ids[0] = n_table - 1                                    # the last table row
                ids[1] = ids[2]                                         # a repeat
            self.ids = ids
            self.x = self.table[ids]
            self.ldc = K + 4
        else:
            self.x = _rand(rng, n, K)
        d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(cuda)
        self.wd = d(_guarded(m, K, self.ldw, self.w))
        self.bd = d(self.b) if bias else None
        self.sd = None if self.post is None else (d(self.post[0]), d(self.post[1]))
        if gather:
            self.td, self.idd = d(self.table), d(self.ids if n else np.zeros(1, np.int64))
            self.xcopy0 = _guarded(n + 2, K, self.ldc)
            self.xcd = d(self.xcopy0)
        else:
            self.xd = d(_guarded(n + 2, K, self.ldx, self.x))          # rows past n: NaN, never to be read
        self.y0 = _guarded(n + 2, m, self.ldy)
        self.yd = d(self.y0)

    def problem(self):
        P = _lib.LinearProblem
        common = dict(w=self.wd.data_ptr(), ldw=self.ldw, bias=0 if self.bd is None else self.bd.data_ptr(),
                      y=self.yd.data_ptr(), ldy=self.ldy, n=self.n, m=self.m, act=self.act,
                      post_scale=0 if self.sd is None else self.sd[0].data_ptr(),
                      post_shift=0 if self.sd is None else self.sd[1].data_ptr())
        if self.gather:
            return P(x=0, ldx=0, ids=self.idd.data_ptr(), table=self.td.data_ptr(), xcopy=self.xcd.data_ptr(),
                     ld_xcopy=self.ldc, **common)
        return P(x=self.xd.data_ptr(), ldx=self.ldx, ids=0, table=0, xcopy=0, ld_xcopy=0, **common)

    def reset(self):
        self.yd.copy_(torch.from_numpy(self.y0))
        if self.gather:
            self.xcd.copy_(torch.from_numpy(self.xcopy0))

    def pre(self):
        """The exact pre-activation: the chain, then the bias."""
        return sr.linear_chain(self.x, self.w, self.b)

    def expected(self):
        assert self.act in (0, 1, 3)
        v = self.pre()
        if self.act == 1:
            v = sr.relu32(v)
        elif self.act == 3:
            v = sr.sign32(v)
        if self.post is not None:
            v = sr.post32(v, self.post[0][None, :], self.post[1][None, :])
        return v

    def result(self):
        """The written block [n, m]; asserts every guard (columns past m, rows past n, xcopy's) is untouched."""
        torch.cuda.synchronize()
        y = self.yd.cpu().numpy()
        got = y[:self.n, :self.m].copy()
        keep = np.ones(y.shape, bool)
        keep[:self.n, :self.m] = False
        assert np.array_equal(_bits(y)[keep], _bits(self.y0)[keep]), "y guard overwritten"
        if self.gather:
            xc = self.xcd.cpu().numpy()
            assert np.array_equal(_bits(xc[:self.n, :self.K]), _bits(self.x)), "xcopy != the gathered rows"
            keep = np.ones(xc.shape, bool)
            keep[:self.n, :self.K] = False
            assert np.array_equal(_bits(xc)[keep], _bits(self.xcopy0)[keep]), "xcopy guard overwritten"
        return got


def _launch(cuda, probs, K):
    arr = (_lib.LinearProblem * len(probs))(*[p.problem() for p in probs])
    _lib.check(_lib.lib().sss_linear_grouped(arr, len(probs), K, _st(cuda)), "sss_linear_grouped")


# a covering subset of N in {1, 63, 64, 65, 130} x M in {1, 2, 31, 33, 63, 64, 65, 250, 898} x K in {32, 64, 96, 800, 3616}:
# every value of each axis, both sides of the 64-row and 64-column tile edges, one K chunk and up to 113 of them
SHAPES = [(1, 1, 32), (63, 2, 64), (64, 31, 96), (65, 33, 800), (130, 63, 32), (1, 64, 3616), (64, 65, 96),
          (65, 250, 64), (130, 898, 800), (63, 898, 32), (130, 64, 3616), (65, 1, 3616), (64, 250, 800), (130, 2, 96),
          (63, 65, 3616), (64, 33, 32)]


@pytest.mark.parametrize("n,m,K", SHAPES)
def test_single_problem_is_the_fma_chain(cuda, n, m, K):
    rng = np.random.default_rng(n * 100003 + m * 101 + K)
    p = Prob(cuda, rng, n, m, K, bias=(n + m) % 2 == 0)
    _launch(cuda, [p], K)
    assert np.array_equal(_bits(p.result()), _bits(p.expected()))


# launches of 1..4 problems of different N, M and act, with zero-row problems first, in the middle and last
SLOTS = [
    [(65, 33, 1)],
    [(0, 40, 0), (130, 65, 3)],
    [(64, 250, 1), (0, 31, 0), (63, 2, 3)],
    [(1, 64, 0), (130, 33, 1), (65, 898, 3), (0, 65, 1)],
    [(0, 7, 3), (0, 64, 0), (63, 129, 1), (2, 1, 0)],
    [(130, 31, 3), (0, 33, 1), (1, 1, 1), (64, 64, 0)],
]


@pytest.mark.parametrize("K", [64, 800])
@pytest.mark.parametrize("slots", range(len(SLOTS)))
def test_problem_slots(cuda, slots, K):
    """Each problem of a grouped launch equals the oracle and, bit for bit, its own single-problem launch; zero-row
    problems write nothing."""
    rng = np.random.default_rng(7000 + 31 * slots + K)
    probs = [Prob(cuda, rng, n, m, K, act=act, zero_rows=(0,) if m > 1 else ()) for n, m, act in SLOTS[slots]]
    _launch(cuda, probs, K)
    grouped = [p.result() for p in probs]
    for p, got in zip(probs, grouped):
        assert np.array_equal(_bits(got), _bits(p.expected())), (p.n, p.m, p.act)
        p.reset()
        _launch(cuda, [p], K)                                           # the same problem alone
        assert np.array_equal(_bits(p.result()), _bits(got)), (p.n, p.m, p.act)


@pytest.mark.parametrize("n,m,K", [(130, 130, 96), (64, 65, 800), (1, 33, 32), (0, 5, 64)])
def test_gather_mode(cuda, n, m, K):
    """Rows = table[ids] (repeats, the last table row); xcopy holds exactly the gathered rows below N whatever the
    number of column tiles, and nothing else; next to it a strided problem in the same launch."""
    rng = np.random.default_rng(9100 + n + m + K)
    p = Prob(cuda, rng, n, m, K, act=1, gather=True)
    q = Prob(cuda, rng, 65, 31, K, act=3)
    _launch(cuda, [p, q], K)
    assert np.array_equal(_bits(p.result()), _bits(p.expected()))
    assert np.array_equal(_bits(q.result()), _bits(q.expected()))


@pytest.mark.parametrize("post", [False, True])
@pytest.mark.parametrize("act", [0, 1, 3])
def test_epilogues_bit_exact(cuda, act, post):
    """relu / sign / none, each with and without the BatchNorm stage relu(fl(fl(v s) + t)) (two roundings, no fma),
    with exactly zero pre-activations (zero weight rows with zero bias): sign(0) = 0, relu(0) = 0, post(0) = relu(t)."""
    rng = np.random.default_rng(9300 + act * 2 + post)
    zero_cols = [0, 5, 64, 97]
    p = Prob(cuda, rng, 130, 98, 96, act=act, post=post, zero_rows=zero_cols)
    _launch(cuda, [p], 96)
    got, want = p.result(), p.expected()
    assert np.array_equal(_bits(got), _bits(want))
    pre = p.pre()
    assert (pre[:, zero_cols] == 0).all()
    if act == 3 and not post:
        assert (got[:, zero_cols] == 0).all() and set(np.unique(got).tolist()) == {-1.0, 0.0, 1.0}
    if post and act != 3:
        # not vacuous: on this data a fused fma(v, s, t) differs from the two-rounding stage somewhere
        v = sr.relu32(pre) if act == 1 else pre
        s, t = (np.broadcast_to(a[None, :], v.shape) for a in p.post)
        assert not np.array_equal(sr.relu32(sr.fmaf(v, s, t)), want)


def _ulp32(v):
    """float32 ulp at the magnitude of the float64 value v."""
    return np.spacing(np.abs(v).astype(np.float32)).astype(np.float64)


@pytest.mark.parametrize("act", [2, 4])
def test_tanh_epilogues_within_documented_ulp(cuda, act):
    """act 2 = tanhf(pre), act 4 = tanhf(tanhf(pre)), pre = the exact chain + bias.  Against float64 tanh of that same
    float32 pre-activation: within TANHF_ULP ulp for one tanhf; for two, the inner error (<= TANHF_ULP ulp of
    t1 = tanh(pre)) passes through the outer tanh (slope <= 1) and the outer adds its own TANHF_ULP ulp."""
    rng = np.random.default_rng(9500 + act)
    p = Prob(cuda, rng, 65, 250, 64, act=act, zero_rows=(3,))
    _launch(cuda, [p], 64)
    got = p.result().astype(np.float64)
    pre = p.pre().astype(np.float64)
    t1 = np.tanh(pre)
    if act == 2:
        want, bound = t1, TANHF_ULP * _ulp32(t1)
    else:
        want = np.tanh(t1)
        bound = TANHF_ULP * _ulp32(want) + TANHF_ULP * _ulp32(t1)
    err = np.abs(got - want)
    assert (err <= bound).all(), float(np.max(err / np.maximum(bound, 1e-300)))
    assert (got[:, 3] == 0).all()                                                 # tanh(0) = 0
    assert np.abs(pre).max() > 2.0 and np.abs(pre[:, 4:]).min() < 0.1             # the data spans tanh's curve
