"""The C ABI's buffer, state and stream contract (include/sss.h), entry point by entry point.

Every call here goes straight to libsss through ctypes -- no Python wrapper pre-fills, chunks or
reuses anything -- with every output, workspace and state buffer allocated at exactly the size the
ABI asks for, at the alignment it requires, between two 4 KB guard bands of random bytes.  Each
call runs twice, its outputs and workspace first filled with 0xFF bytes, then with a NaN / 0x5A
pattern: the guards must be intact, both runs must give the same bits (every element written,
nothing read from the workspace), the outputs must equal the oracle, and `state` must come back
all zero.  Inputs are the first rows of larger tensors whose further rows would win if a kernel
read them; row strides are wider than the rows, input padding columns hold NaN and output padding
columns are guards.  Search results and integer outputs are compared bit for bit; float kernels
use the tolerances of tests/test_encoder_gpu.py and tests/test_variants_gpu.py.
"""
import ctypes
import itertools
import math
import os
import sys

import numpy as np
import pytest
import torch

from oracle import gnn_ref
from oracle.encoder_kernels_ref import gat_ref as _gat_ref, gru_ref as _gru_ref
from oracle import search_ref as sr
from sessionsimilaritysearch_amd import _lib
from sessionsimilaritysearch_amd import sessions as S
from sessionsimilaritysearch_amd.encoder import EncoderConfig, SessionEncoder, init_weights

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import bound_inputs_ref as bir  # noqa: E402

pytestmark = pytest.mark.gpu

# Entry point -> the test that makes guarded calls of it.  Plain data: tests/test_abi_contract_cpu.py reads it
# with ast (no import of this module) and checks it against the declarations of include/sss.h.
COVERAGE = {
    "sss_ip_topk": "test_fused_search",
    "sss_ip_topk_split": "test_fused_search",
    "sss_ip_topk_f16": "test_fused_search",
    "sss_ip_topk_threshold": "test_threshold_rung",
    "sss_ip_topk_long": "test_long_scan",
    "sss_ip_topk_exhaustive": "test_exhaustive",
    "sss_ip_topk_exhaustive_lb": "test_exhaustive_lb",
    "sss_range_search_count": "test_range_fused",
    "sss_range_search_fill": "test_range_fused",
    "sss_range_search_exhaustive_count": "test_range_exhaustive",
    "sss_range_search_exhaustive_fill": "test_range_exhaustive",
    "sss_topk_merge": "test_topk_merge",
    "sss_normalize_rows": "test_normalize_rows",
    "sss_row_norm_max": "test_row_norm_max",
    "sss_f32_to_bf16": "test_image_conversions",
    "sss_split_bf16": "test_image_conversions",
    "sss_abs_max": "test_image_maxima",
    "sss_scale_f16": "test_image_conversions",
    "sss_f16_resid_max": "test_image_maxima",
    "sss_gather_rows": "test_gather_rows",
    "sss_gather_concat_rows": "test_gather_concat_rows",
    "sss_linear": "test_linear",
    "sss_linear_grouped": "test_linear_grouped",
    "sss_gat_aggregate": "test_gat_aggregate",
    "sss_csr_weighted_sum": "test_csr_weighted_sum_and_gru",
    "sss_gru_combine": "test_csr_weighted_sum_and_gru",
    "sss_hetero_layer_update": "test_hetero_layer_update",
    "sss_pool_expand": "test_pool_expand_segment_pool",
    "sss_segment_pool": "test_pool_expand_segment_pool",
    "sss_segment_ptr": "test_segment_ptr",
    "sss_pool_expand_mean": "test_pool_expand_mean_attention",
    "sss_pool_attention": "test_pool_expand_mean_attention",
    "sss_pool_attention_tab": "test_pool_attention_tab",
    "sss_csr_mean": "test_csr_mean",
    "sss_segment_reduce": "test_segment_reduce",
    "sss_attention_dot_pool": "test_attention_dot_pool",
    "sss_graph_counts": "test_graph_builder",
    "sss_graph_fill": "test_graph_builder",
    "sss_pack_sign_bits": "test_pack_sign_bits",
    "sss_hamming_topk": "test_hamming",
    "sss_hamming_topk_exhaustive": "test_hamming",
    "sss_knn_item_vote": "test_knn_item_vote",
}

GUARD = 4096
OFF = 2 ** 33 + 5                       # id_offset: catches a 32-bit id anywhere on the way out
FMAX = float(np.finfo(np.float32).max)
TOL = 1e-5
_SEEDS = itertools.count(1)


def L():
    return _lib.lib()


def _st(stream=None):
    return (stream or torch.cuda.current_stream()).cuda_stream


class Buf:
    """`shape` x `dtype` on the device, exactly that many bytes, at `align`, between two GUARD-byte bands of random
    bytes (kept in `pat`)."""

    def __init__(self, shape, dtype, align=256, zero=False):
        self.shape = tuple(int(s) for s in shape) if isinstance(shape, (tuple, list)) else (int(shape),)
        self.dtype = dtype
        self.nbytes = int(np.prod(self.shape, dtype=np.int64)) * torch.empty((), dtype=dtype).element_size()
        raw = torch.empty(2 * GUARD + self.nbytes + align, dtype=torch.uint8, device="cuda")
        self.off = GUARD + (-(raw.data_ptr() + GUARD)) % align
        g = torch.Generator().manual_seed(next(_SEEDS))
        self.pat = torch.randint(0, 256, (raw.numel(),), dtype=torch.uint8, generator=g).to("cuda")
        raw.copy_(self.pat)
        self.raw = raw
        if zero:
            self.bytes.zero_()

    @property
    def ptr(self):
        return self.raw.data_ptr() + self.off

    @property
    def bytes(self):
        return self.raw[self.off:self.off + self.nbytes]

    @property
    def t(self):
        return self.bytes.view(self.dtype).view(self.shape)

    def guards_ok(self):
        e = self.off + self.nbytes
        return torch.equal(self.raw[:self.off], self.pat[:self.off]) and torch.equal(self.raw[e:], self.pat[e:])

    def poison(self, which):
        b = self.bytes
        if which == 0:
            b.fill_(0xFF)
        elif self.dtype == torch.float32:
            b.view(torch.int32).fill_(0x7FC05A5A)
        elif self.dtype == torch.float64:
            b.view(torch.int64).fill_(0x7FF85A5A5A5A5A5A)
        else:
            b.fill_(0x5A)


def dev_buf(x, dtype=None, align=256):
    """A guarded input buffer holding `x` (tensor / ndarray)."""
    x = torch.as_tensor(x)
    b = Buf(x.shape, dtype or x.dtype, align)
    b.t.copy_(x.to(b.dtype))
    return b


def run_twice(call, outs, scratch=(), states=(), prep=None, written=None):
    """Run `call` twice, `outs` and `scratch` filled with poison 0, then 1 (`prep` runs after each fill).  `written`
    (one bool mask or None per out, device tensors of the out's shape): where the call must write -- elsewhere the
    out must still hold its poison.  Asserts rc 0, intact guards, zero state, identical written bits; returns the
    poison-1 pre-call bytes of the outs."""
    written = written or [None] * len(outs)
    snaps, before = [], None
    for p in (0, 1):
        for b in (*outs, *scratch):
            b.poison(p)
        if prep is not None:
            prep()
        torch.cuda.synchronize()
        before = [b.t.clone() for b in outs]
        rc = call()
        assert rc == 0, (rc, L().sss_last_error())
        torch.cuda.synchronize()
        snaps.append([b.t.clone() for b in outs])
        for b in (*outs, *scratch, *states):
            assert b.guards_ok(), "a write landed in a guard band"
        for s in states:
            assert not bool(s.bytes.any()), "state not handed back zeroed"
    for i, (a, b) in enumerate(zip(*snaps)):
        m = written[i]
        ab, bb = _bits(a), _bits(b)
        if m is None:
            assert torch.equal(ab, bb), f"output {i}: not every element written (differs between poisons)"
        else:
            assert torch.equal(ab[m], bb[m]), f"output {i}: not every element written (differs between poisons)"
            assert torch.equal(_bits(before[i])[~m], bb[~m]), f"output {i}: written outside its rows / columns"
    return before


def _bits(t):
    """Integer view (NaN-safe bitwise comparison)."""
    return t.view({4: torch.int32, 8: torch.int64, 2: torch.int16, 1: torch.uint8}[t.element_size()])


def _rows_mask(shape, rows):
    m = torch.zeros(shape, dtype=torch.bool, device="cuda")
    m[torch.as_tensor(rows, device="cuda").long()] = True
    return m


def _cols_mask(shape, ncols):
    m = torch.zeros(shape, dtype=torch.bool, device="cuda")
    m[:, :ncols] = True
    return m


def _strided(x, ld, fill=float("nan")):
    """x [n, d] -> guarded [n, ld] float32 buffer, columns d.. = fill."""
    x = torch.as_tensor(x, dtype=torch.float32)
    full = torch.full((x.shape[0], ld), fill, dtype=torch.float32)
    full[:, :x.shape[1]] = x
    return dev_buf(full)


# ------------------------------------------------------------------------------------------------ corpora
def _unit_rows(rng, n, d):
    x = rng.standard_normal((n, d)).astype(np.float32)
    return x / np.linalg.norm(x, axis=1, keepdims=True)


class Corpus:
    """n rows (dtype "f32" or "bf16") followed by TAIL rows that would win every query if a kernel read them (the
    queries x 1e3); queries followed by NaN rows; rows 100.. 100+DUP of the corpus are copies of query 0 (exact
    ties at every rank up to DUP: unproven queries)."""
    TAIL, QTAIL, DUP = 300, 8, 600

    def __init__(self, n, d, nq, dtype="f32", seed=0, dup=True):
        rng = np.random.default_rng(seed)
        self.n, self.d, self.nq, self.dtype = n, d, nq, dtype
        c = _unit_rows(rng, n + self.TAIL, d)
        q = _unit_rows(rng, nq, d)
        q[1::3] = 0.6 * c[rng.integers(0, n, len(q[1::3]))] + 0.4 * q[1::3]        # near neighbours
        if dup and n > 100 + self.DUP:
            c[100:100 + self.DUP] = q[0]
            q[2 % nq] = q[0]
        c[n:] = 1e3 * np.resize(q, (self.TAIL, d))
        self.tdtype = torch.float32 if dtype == "f32" else torch.bfloat16
        qt = np.full((nq + self.QTAIL, d), np.nan, np.float32)
        qt[:nq] = q
        self.c_t = torch.from_numpy(c).to("cuda").to(self.tdtype)
        self.q_t = torch.from_numpy(qt).to("cuda").to(self.tdtype)
        self.c = self.c_t[:n].float().cpu().numpy()           # the stored (rounded) values: what the contract scores
        self.q = self.q_t[:nq].float().cpu().numpy()
        self.cmax = float(np.linalg.norm(self.c.astype(np.float64), axis=1).max()) * (1 + 1e-6)
        self._f16 = self._split = None
        self._oracle = {}

    def f16(self):
        if self._f16 is None:
            amax = float(np.abs(self.c).max())
            self.shift = int(L().sss_f16_shift(amax))
            self._f16 = (self.c_t.float() * 2.0 ** self.shift).half()          # the tail overflows to inf
            r = (self._f16[:self.n].double() * 2.0 ** -self.shift - self.c_t[:self.n].double()).norm(dim=1).max()
            self.resid = float(r) * (1 + 1e-6)
        return self._f16

    def split(self):
        if self._split is None:
            hi = self.c_t.bfloat16()
            lo = (self.c_t - hi.float()).bfloat16()
            self._split = torch.cat([hi, lo], dim=1).contiguous()
        return self._split

    def oracle(self, k):
        if k not in self._oracle:
            self._oracle[k] = sr.search_exact(self.q, self.c, k, id_offset=OFF)
        return self._oracle[k]


def _check_search(D, I, status, ref, n, lower_bound_ok=True):
    """Rows with status 0 equal the oracle bit for bit; the others are fully written with column k-1 a valid lower
    bound of the k-th score.  No id outside [OFF, OFF + n)."""
    Dr, Ir = ref
    D, I = D.cpu().numpy(), I.cpu().numpy()
    ok = status.cpu().numpy() == 0
    valid = I[I >= 0]
    assert ((valid >= OFF) & (valid < OFF + n)).all(), "an id outside the corpus rows (tail row or 32-bit truncation)"
    assert np.array_equal(I[ok], Ir[ok]) and np.array_equal(D[ok], Dr[ok]), "proven rows differ from the oracle"
    if (~ok).any():
        assert not np.isnan(D[~ok]).any() and (I[~ok] >= -1).all(), "an unproven row was left partly unwritten"
        if lower_bound_ok:
            assert (D[~ok, -1] <= Dr[~ok, -1]).all(), "column k-1 of an unproven row is not a lower bound"
    return int((~ok).sum())


def _fused_call(kind, C, k, D, I, status, state, ws, unproven=0, nq=None, stream=None):
    nq = C.nq if nq is None else nq
    st = _st(stream)
    Dp, Ip, sp = (x if isinstance(x, int) else x.ptr for x in (D, I, status))
    sb, sptr = state.nbytes, state.ptr
    if kind in ("f32", "bf16"):
        return L().sss_ip_topk(C.q_t.data_ptr(), nq, C.c_t.data_ptr(), C.n, C.d, k, 0 if kind == "f32" else 1, OFF, C.cmax,
                               Dp, Ip, sp, unproven, sptr, sb, ws.ptr, ws.nbytes, st)
    if kind == "split":
        return L().sss_ip_topk_split(C.q_t.data_ptr(), nq, C.c_t.data_ptr(), C.split().data_ptr(), C.n, C.d, k, OFF, C.cmax,
                                     Dp, Ip, sp, unproven, sptr, sb, ws.ptr, ws.nbytes, st)
    img = C.f16()
    return L().sss_ip_topk_f16(C.q_t.data_ptr(), nq, C.c_t.data_ptr(), img.data_ptr(), C.shift, C.resid, C.n, C.d, k, OFF,
                               C.cmax, Dp, Ip, sp, unproven, sptr, sb, ws.ptr, ws.nbytes, st)


def _fused_ws_bytes(kind, nq, n, d, k):
    if kind == "f16":
        return int(L().sss_ip_topk_f16_workspace_bytes(nq, n, d, k))
    return int(L().sss_ip_topk_workspace_bytes(nq, n, d, k, 1 if kind == "bf16" else 0))


_CORPORA = {}


def corpus(n, d, nq, dtype="f32", seed=0):
    key = (n, d, nq, dtype, seed)
    if key not in _CORPORA:
        _CORPORA.clear()
        _CORPORA[key] = Corpus(n, d, nq, dtype, seed)
    return _CORPORA[key]


# ------------------------------------------------------------------------------------------------ search
@pytest.mark.parametrize("kind,d,n,nq,k", [
    ("f32", 128, 70001, 150, 1), ("f32", 64, 20011, 77, 500), ("f32", 256, 9001, 33, 17),
    ("bf16", 128, 30001, 100, 16), ("bf16", 256, 12007, 64, 100),
    ("split", 128, 70001, 150, 10), ("split", 64, 20011, 77, 17),
    ("f16", 128, 70001, 150, 100), ("f16", 256, 12007, 64, 500), ("f16", 512, 5003, 40, 10)])
def test_fused_search(cuda, kind, d, n, nq, k):
    C = corpus(n, d, nq, "bf16" if kind == "bf16" else "f32", seed=d + n)
    D, I, status = Buf((nq, k), torch.float32), Buf((nq, k), torch.int64), Buf(nq, torch.int32)
    wsb = _fused_ws_bytes(kind, nq, n, d, k)
    assert wsb > 0
    ws, state = Buf(wsb, torch.uint8), Buf(int(L().sss_ip_topk_state_bytes(nq)), torch.uint8, align=16, zero=True)
    cnt = Buf(1, torch.int32, zero=True)
    seen = []

    def call():
        rc = _fused_call(kind, C, k, D, I, status, state, ws, cnt.ptr)
        torch.cuda.synchronize()
        seen.append(int((status.t != 0).sum()))
        return rc
    for p in (0, 1):                # every element written: no poison survives, whichever it was
        for b in (D, I, status, ws):
            b.poison(p)
        assert call() == 0, L().sss_last_error()
        for b in (D, I, status, ws, state, cnt):
            assert b.guards_ok()
        assert not bool(state.bytes.any()), "state not handed back zeroed"
        assert int(status.t.min()) >= 0 and int(status.t.max()) <= 7        # 0 or a mask of the reasons a proof failed
        _check_search(D.t, I.t, status.t, C.oracle(k), n)
    assert int(cnt.t[0]) == sum(seen), "unproven_count != number of status != 0 rows"


def _fused_plain(kind, C, k, nq=None):
    nq = C.nq if nq is None else nq
    D = torch.empty((nq, k), dtype=torch.float32, device="cuda")
    I = torch.empty((nq, k), dtype=torch.int64, device="cuda")
    status = torch.empty(nq, dtype=torch.int32, device="cuda")
    ws = Buf(_fused_ws_bytes(kind, nq, C.n, C.d, k), torch.uint8)
    state = Buf(int(L().sss_ip_topk_state_bytes(nq)), torch.uint8, align=16, zero=True)
    assert _fused_call(kind, C, k, D.data_ptr(), I.data_ptr(), status.data_ptr(), state, ws, nq=nq) == 0
    return D, I, status


@pytest.mark.parametrize("scan,kind,d,n,nq,k", [(0, "f32", 128, 70001, 150, 10), (1, "bf16", 256, 30001, 64, 100),
                                                (2, "split", 128, 70001, 150, 17), (3, "f16", 128, 70001, 150, 100)])
def test_threshold_rung(cuda, scan, kind, d, n, nq, k):
    """The rung on a non-contiguous subset of query rows (the tied ones among them): rows not selected keep their
    poison in D / I / status, the selected ones come out exact."""
    C = corpus(n, d, nq, "bf16" if kind == "bf16" else "f32", seed=d + n)
    D0, I0, s0 = _fused_plain(kind, C, k)
    sel = np.r_[0:3, 5:nq:7].astype(np.int32)
    qsel = dev_buf(torch.from_numpy(sel))
    image, shift, resid = C.c_t, 0, 0.0
    if scan == 2:
        image = C.split()
    elif scan == 3:
        image, shift, resid = C.f16(), C.shift, C.resid
    D, I, status = Buf((nq, k), torch.float32), Buf((nq, k), torch.int64), Buf(nq, torch.int32)
    ws = Buf(int(L().sss_ip_topk_threshold_workspace_bytes(len(sel), n, d, scan)), torch.uint8)
    rows = torch.from_numpy(sel).long().cuda()

    def prep():
        D.t[rows], I.t[rows], status.t[rows] = D0[rows], I0[rows], 1
    call = lambda: L().sss_ip_topk_threshold(C.q_t.data_ptr(), qsel.ptr, len(sel), C.c_t.data_ptr(), 1 if kind == "bf16" else 0,
                                             image.data_ptr(), scan, shift, resid, n, d, k, OFF, C.cmax, D.ptr, I.ptr,
                                             status.ptr, ws.ptr, ws.nbytes, _st())
    run_twice(call, [D, I, status], [ws], prep=prep,
              written=[_rows_mask((nq, k), sel), _rows_mask((nq, k), sel), _rows_mask((nq,), sel)])
    assert int(status.t[rows].abs().sum()) == 0
    Dr, Ir = C.oracle(k)
    assert np.array_equal(I.t[rows].cpu().numpy(), Ir[sel]) and np.array_equal(D.t[rows].cpu().numpy(), Dr[sel])
    assert qsel.guards_ok()


@pytest.mark.parametrize("dtype,d,n,nq", [(0, 320, 20001, 40), (1, 320, 20001, 40), (0, 1600, 3001, 24), (1, 1600, 3001, 24)])
def test_long_scan(cuda, dtype, d, n, nq):
    k = 100
    C = corpus(n, d, nq, "bf16" if dtype else "f32", seed=d + n + dtype)
    image, shift, resid = (C.c_t, 0, 0.0) if dtype else (C.f16(), C.shift, C.resid)
    D, I, status = Buf((nq, k), torch.float32), Buf((nq, k), torch.int64), Buf(nq, torch.int32)
    ws = Buf(int(L().sss_ip_topk_long_workspace_bytes(nq, n, d, dtype)), torch.uint8)
    for p in (0, 1):
        for b in (D, I, status, ws):
            b.poison(p)
        rc = L().sss_ip_topk_long(C.q_t.data_ptr(), nq, C.c_t.data_ptr(), dtype, image.data_ptr(), shift, resid, n, d, k, OFF,
                                  C.cmax, D.ptr, I.ptr, status.ptr, ws.ptr, ws.nbytes, _st())
        assert rc == 0, L().sss_last_error()
        torch.cuda.synchronize()
        assert all(b.guards_ok() for b in (D, I, status, ws))
        assert int(status.t.min()) >= 0 and int(status.t.max()) <= 1
        _check_search(D.t, I.t, status.t, C.oracle(k), n)


def _ref_l2(q, c, k):
    return sr.topk_from_scores(sr.canonical_l2(q, c), k, OFF, largest=False)


@pytest.mark.parametrize("metric,dtype,d,n,nq,k", [(0, 0, 96, 300, 20, 400), (1, 0, 64, 1001, 20, 50),
                                                   (0, 1, 128, 300, 20, 1024), (1, 1, 40, 500, 20, 600),
                                                   (0, 0, 128, 70001, 30, 10)])
def test_exhaustive(cuda, metric, dtype, d, n, nq, k):
    C = Corpus(n, d, nq, "bf16" if dtype else "f32", seed=n + d, dup=False)
    if metric == 1:
        C.c_t[n:] = C.q_t[:1].float().to(C.tdtype)       # L2: copies of query 0 win its row
    sel = np.r_[1, 4:nq:3, 0].astype(np.int32)
    qsel = dev_buf(torch.from_numpy(sel))
    D, I = Buf((nq, k), torch.float32), Buf((nq, k), torch.int64)
    ws = Buf(int(L().sss_ip_topk_exhaustive_workspace_bytes(len(sel), n)), torch.uint8)
    call = lambda: L().sss_ip_topk_exhaustive(C.q_t.data_ptr(), qsel.ptr, len(sel), C.c_t.data_ptr(), n, d, k, dtype, OFF, metric,
                                              D.ptr, I.ptr, ws.ptr, ws.nbytes, _st())
    run_twice(call, [D, I], [ws], written=[_rows_mask((nq, k), sel)] * 2)
    Dr, Ir = (C.oracle(k) if metric == 0 else _ref_l2(C.q, C.c, k))
    assert np.array_equal(I.t.cpu().numpy()[sel], Ir[sel]) and np.array_equal(D.t.cpu().numpy()[sel], Dr[sel])


@pytest.mark.parametrize("dtype,d,n", [(0, 128, 70001), (1, 256, 30001), (0, 96, 5003)])
def test_exhaustive_lb(cuda, dtype, d, n):
    nq, k = 40, 17
    C = Corpus(n, d, nq, "bf16" if dtype else "f32", seed=7 + n)
    Dr, Ir = C.oracle(k)
    sel = np.r_[0, 2, 3:nq:4].astype(np.int32)
    lb = Dr[sel, k - 1].copy()
    lb[1::3] = -FMAX                                     # no bound known
    lb[2::3] = np.nextafter(lb[2::3], -np.inf)           # a bound just below the k-th score
    qsel, lbb = dev_buf(torch.from_numpy(sel)), dev_buf(torch.from_numpy(lb))
    D, I = Buf((nq, k), torch.float32), Buf((nq, k), torch.int64)
    ws = Buf(int(L().sss_ip_topk_exhaustive_workspace_bytes(len(sel), n)), torch.uint8)
    call = lambda: L().sss_ip_topk_exhaustive_lb(C.q_t.data_ptr(), qsel.ptr, len(sel), C.c_t.data_ptr(), n, d, k, dtype, OFF,
                                                 lbb.ptr, D.ptr, I.ptr, ws.ptr, ws.nbytes, _st())
    run_twice(call, [D, I], [ws], written=[_rows_mask((nq, k), sel)] * 2)
    assert np.array_equal(I.t.cpu().numpy()[sel], Ir[sel]) and np.array_equal(D.t.cpu().numpy()[sel], Dr[sel])


def _radii(scores, rng, metric):
    """Per query: the score at a random rank (strict comparison: that row itself is out), one query with nothing."""
    nq = scores.shape[0]
    srt = np.sort(scores, axis=1)
    ranks = rng.integers(0, 120, nq)
    rad = srt[np.arange(nq), ranks] if metric == 1 else srt[np.arange(nq), -1 - ranks]
    rad[3] = -FMAX if metric == 1 else FMAX
    return rad.astype(np.float32)


def _range_ref(scores, rad, rows, metric):
    lims, D, I = [0], [], []
    for r in rows:
        keep = np.flatnonzero(scores[r] < rad[r] if metric else scores[r] > rad[r])
        D.append(scores[r, keep])
        I.append(keep + OFF)
        lims.append(lims[-1] + len(keep))
    return np.array(lims, np.int64), np.concatenate(D).astype(np.float32), np.concatenate(I).astype(np.int64)


def _range_fill_checked(nq_rows, counts, fill, ws):
    """lims from counts; guarded D / I of exactly lims[-1]; fill twice; the workspace is read-only to fill."""
    lims_h = np.zeros(nq_rows + 1, np.int64)
    np.cumsum(counts, out=lims_h[1:])
    lims = dev_buf(torch.from_numpy(lims_h))
    total = int(lims_h[-1])
    assert total > 0
    D, I = Buf(total, torch.float32), Buf(total, torch.int64)
    ws_before = ws.bytes.clone()
    run_twice(lambda: fill(lims, D, I), [D, I])
    assert torch.equal(ws.bytes, ws_before), "fill wrote into the workspace"
    return lims_h, D.t.cpu().numpy(), I.t.cpu().numpy()


@pytest.mark.parametrize("scan,kind,d,n", [(3, "f16", 128, 70001), (1, "bf16", 256, 30001), (0, "f32", 64, 20011)])
def test_range_fused(cuda, scan, kind, d, n):
    nq = 48
    C = Corpus(n, d, nq, "bf16" if kind == "bf16" else "f32", seed=3 + n, dup=False)
    scores = sr.canonical_scores(C.q, C.c)
    rad = _radii(scores, np.random.default_rng(n), 0)
    radb = dev_buf(torch.from_numpy(rad))
    image, shift, resid = (C.f16(), C.shift, C.resid) if scan == 3 else (C.c_t, 0, 0.0)
    counts, status = Buf(nq, torch.int64), Buf(nq, torch.int32)
    ws = Buf(int(L().sss_range_search_workspace_bytes(nq, n, d, scan)), torch.uint8)
    call = lambda: L().sss_range_search_count(C.q_t.data_ptr(), nq, C.c_t.data_ptr(), 1 if kind == "bf16" else 0, image.data_ptr(),
                                              scan, shift, resid, n, d, radb.ptr, C.cmax, counts.ptr, status.ptr, ws.ptr,
                                              ws.nbytes, _st())
    run_twice(call, [counts, status], [ws])
    assert int(status.t.abs().sum()) == 0
    lims_r, Dr, Ir = _range_ref(scores, rad, range(nq), 0)
    cnt = counts.t.cpu().numpy()
    assert np.array_equal(cnt, np.diff(lims_r))
    fill = lambda lims, D, I: L().sss_range_search_fill(nq, lims.ptr, OFF, D.ptr, I.ptr, ws.ptr, ws.nbytes, _st())
    lims_h, D, I = _range_fill_checked(nq, cnt, fill, ws)
    assert np.array_equal(I, Ir) and np.array_equal(D, Dr)


@pytest.mark.parametrize("metric,dtype,d,n", [(0, 0, 96, 20011), (1, 0, 64, 5003), (0, 1, 128, 9001), (1, 1, 40, 3001)])
def test_range_exhaustive(cuda, metric, dtype, d, n):
    nq = 40
    C = Corpus(n, d, nq, "bf16" if dtype else "f32", seed=5 + n, dup=False)
    if metric == 1:
        C.c_t[n:] = C.q_t[:1].float().to(C.tdtype)
    scores = sr.canonical_l2(C.q, C.c) if metric else sr.canonical_scores(C.q, C.c)
    rad = _radii(scores, np.random.default_rng(n), metric)
    radb = dev_buf(torch.from_numpy(rad))
    sel = np.r_[3, 1, 6:nq:3].astype(np.int32)
    qsel = dev_buf(torch.from_numpy(sel))
    counts = Buf(len(sel), torch.int64)
    ws = Buf(int(L().sss_range_search_exhaustive_workspace_bytes(len(sel), n)), torch.uint8)
    call = lambda: L().sss_range_search_exhaustive_count(C.q_t.data_ptr(), qsel.ptr, len(sel), C.c_t.data_ptr(), n, d, dtype, metric,
                                                         radb.ptr, counts.ptr, ws.ptr, ws.nbytes, _st())
    run_twice(call, [counts], [ws])
    lims_r, Dr, Ir = _range_ref(scores, rad, sel, metric)
    cnt = counts.t.cpu().numpy()
    assert np.array_equal(cnt, np.diff(lims_r))
    fill = lambda lims, D, I: L().sss_range_search_exhaustive_fill(qsel.ptr, len(sel), n, metric, radb.ptr, lims.ptr, OFF, D.ptr,
                                                                   I.ptr, ws.ptr, ws.nbytes, _st())
    _, D, I = _range_fill_checked(len(sel), cnt, fill, ws)
    assert np.array_equal(I, Ir) and np.array_equal(D, Dr)


def test_topk_merge(cuda):
    """Three shards, some rows holding fewer than k results, blocks `stride` apart with a gap of entries that would
    win the merge if read."""
    rng = np.random.default_rng(11)
    nq, k, shards = 37, 25, 3
    stride = nq * k + 131
    Dp, Ip = [], []
    Din = np.full(shards * stride, 1e30, np.float32)
    Iin = np.full(shards * stride, 7, np.int64)
    for s in range(shards):
        sc = rng.integers(0, 40, (nq, k)).astype(np.float32) / 8          # many equal scores across shards
        ids = OFF + s * 100000 + np.argsort(rng.random((nq, k)), axis=1)
        order = np.lexsort((ids, -sc.astype(np.float64)), axis=1)
        d_, i_ = np.take_along_axis(sc, order, 1), np.take_along_axis(ids, order, 1)
        short = rng.integers(0, k + 1, nq) if s else np.full(nq, k)     # shards 1, 2: fewer than k rows for some queries
        for r in range(nq):
            d_[r, short[r]:], i_[r, short[r]:] = -FMAX, -1
        Dp.append(d_), Ip.append(i_)
        Din[s * stride:s * stride + nq * k] = d_.ravel()
        Iin[s * stride:s * stride + nq * k] = i_.ravel()
    Dr, Ir = sr.merge_topk(Dp, Ip, k)
    Db, Ib = dev_buf(torch.from_numpy(Din)), dev_buf(torch.from_numpy(Iin))
    D, I = Buf((nq, k), torch.float32), Buf((nq, k), torch.int64)
    run_twice(lambda: L().sss_topk_merge(Db.ptr, stride, Ib.ptr, stride, shards, nq, k, D.ptr, I.ptr, _st()), [D, I])
    assert np.array_equal(I.t.cpu().numpy(), Ir) and np.array_equal(D.t.cpu().numpy(), Dr)


# ------------------------------------------------------------------------------------------------ state, rejections
def test_state_reuse_and_unproven_count(cuda):
    """One state buffer sized for the largest nq serves smaller nq', other n / k / dtype / scan; zero after every
    call; unproven_count grows by exactly the unproven rows of each call and is never reset."""
    nq_max = 600
    state = Buf(int(L().sss_ip_topk_state_bytes(nq_max)), torch.uint8, align=16, zero=True)
    cnt = Buf(1, torch.int32, zero=True)
    total = 0
    for kind, n, d, nq, k in [("f32", 70001, 128, 600, 10), ("f16", 20011, 128, 37, 100), ("split", 70001, 128, 200, 17),
                              ("bf16", 12007, 256, 64, 500), ("f32", 901, 64, 1, 1), ("f16", 70001, 128, 300, 16)]:
        C = corpus(n, d, nq, "bf16" if kind == "bf16" else "f32", seed=d + n)
        D, I, status = Buf((nq, k), torch.float32), Buf((nq, k), torch.int64), Buf(nq, torch.int32)
        ws = Buf(_fused_ws_bytes(kind, nq, n, d, k), torch.uint8)
        assert _fused_call(kind, C, k, D, I, status, state, ws, cnt.ptr) == 0, L().sss_last_error()
        torch.cuda.synchronize()
        assert state.guards_ok() and not bool(state.bytes.any()), "state not zero after the call"
        bad = _check_search(D.t, I.t, status.t, C.oracle(k), n)
        total += bad
        assert int(cnt.t[0]) == total and cnt.guards_ok()
    assert total > 0, "the duplicate rows left no query unproven: the count was not exercised"


def test_rejected_calls_touch_nothing(cuda):
    """A workspace one byte short returns -2, one 16 bytes off its alignment -1; outputs, state and guards as they
    were."""
    C = corpus(70001, 128, 150, "f32", seed=128 + 70001)
    nq, n, d, k = C.nq, C.n, C.d, 10
    D, I, status = Buf((nq, k), torch.float32), Buf((nq, k), torch.int64), Buf(nq, torch.int32)
    state = Buf(int(L().sss_ip_topk_state_bytes(nq)), torch.uint8, align=16, zero=True)
    need = _fused_ws_bytes("f32", nq, n, d, k)
    ws = Buf(need + 256, torch.uint8)
    qsel = dev_buf(torch.arange(0, nq, 3, dtype=torch.int32))
    nsel = qsel.shape[0]
    img = C.f16()
    rad = dev_buf(torch.zeros(nq))
    counts = Buf(nq, torch.int64)
    calls = {
        "ip_topk": (need, lambda p, b: L().sss_ip_topk(C.q_t.data_ptr(), nq, C.c_t.data_ptr(), n, d, k, 0, OFF, C.cmax, D.ptr, I.ptr,
                                                      status.ptr, 0, state.ptr, state.nbytes, p, b, _st())),
        "threshold": (int(L().sss_ip_topk_threshold_workspace_bytes(nsel, n, d, 3)),
                      lambda p, b: L().sss_ip_topk_threshold(C.q_t.data_ptr(), qsel.ptr, nsel, C.c_t.data_ptr(), 0, img.data_ptr(), 3,
                                                             C.shift, C.resid, n, d, k, OFF, C.cmax, D.ptr, I.ptr, status.ptr, p, b,
                                                             _st())),
        "long": (int(L().sss_ip_topk_long_workspace_bytes(nq, n, d, 0)),
                 lambda p, b: L().sss_ip_topk_long(C.q_t.data_ptr(), nq, C.c_t.data_ptr(), 0, img.data_ptr(), C.shift, C.resid, n, d,
                                                   k, OFF, C.cmax, D.ptr, I.ptr, status.ptr, p, b, _st())),
        "range": (int(L().sss_range_search_workspace_bytes(nq, n, d, 3)),
                  lambda p, b: L().sss_range_search_count(C.q_t.data_ptr(), nq, C.c_t.data_ptr(), 0, img.data_ptr(), 3, C.shift,
                                                          C.resid, n, d, rad.ptr, C.cmax, counts.ptr, status.ptr, p, b, _st())),
        "range_exhaustive": (int(L().sss_range_search_exhaustive_workspace_bytes(nsel, n)),
                             lambda p, b: L().sss_range_search_exhaustive_count(C.q_t.data_ptr(), qsel.ptr, nsel, C.c_t.data_ptr(),
                                                                                n, d, 0, 0, rad.ptr, counts.ptr, p, b, _st())),
    }
    for name, (nb, fn) in calls.items():
        ws = Buf(nb + 256, torch.uint8)
        for b in (D, I, status, counts):
            b.poison(1)
        torch.cuda.synchronize()
        snap = [b.bytes.clone() for b in (D, I, status, counts, ws)]
        assert fn(ws.ptr, nb - 1) == -2, (name, L().sss_last_error())
        assert fn(ws.ptr + 16, nb) == -1, (name, L().sss_last_error())
        torch.cuda.synchronize()
        for b, s in zip((D, I, status, counts, ws), snap):
            assert torch.equal(b.bytes, s) and b.guards_ok(), f"{name}: a rejected call wrote"
        assert state.guards_ok() and not bool(state.bytes.any())


# ------------------------------------------------------------------------------------------------ images, row ops
@pytest.mark.parametrize("rule,eps", [(0, 1e-6), (1, 1e-4)])
def test_normalize_rows(cuda, rule, eps):
    g = torch.Generator().manual_seed(20 + rule)
    n, d, ld = 1001, 100, 108
    x = torch.randn((n, d), generator=g) * torch.rand((n, 1), generator=g) * 3
    x[5] = 0
    x[6] = 1e-5
    buf = _strided(x, ld)
    pad_before = buf.t[:, d:].clone()
    assert L().sss_normalize_rows(buf.ptr, n, d, ld, eps, rule, _st()) == 0
    torch.cuda.synchronize()
    assert buf.guards_ok() and torch.equal(_bits(buf.t[:, d:]), _bits(pad_before)), "wrote into the padding columns"
    x64 = x.double()
    s = (x64 * x64).sum(1, keepdim=True)
    ref = x64 / torch.sqrt(s.clamp(min=eps)) if rule == 0 else x64 / (torch.sqrt(s) + eps)
    np.testing.assert_allclose(buf.t[:, :d].cpu().double().numpy(), ref.numpy(), rtol=2e-6, atol=1e-8)


@pytest.mark.parametrize("dtype", [0, 1])
def test_row_norm_max(cuda, dtype):
    g = torch.Generator().manual_seed(30 + dtype)
    n, d = 7001, 136
    x = torch.randn((n + 64, d), generator=g)
    x[n:] = 1e6                                                          # tail rows: would set the maximum
    xt = x.cuda() if dtype == 0 else x.cuda().bfloat16()
    out = Buf(1, torch.float32, zero=True)
    assert L().sss_row_norm_max(xt.data_ptr(), n, d, dtype, out.ptr, _st()) == 0
    torch.cuda.synchronize()
    norms = xt[:n].double().norm(dim=1)
    ref = float(norms.max())
    exact = math.sqrt(math.fsum(float(v) * float(v) for v in xt[int(norms.argmax())].float().cpu().numpy()))
    assert abs(ref - exact) <= 1e-12 * exact
    assert out.guards_ok() and ref <= float(out.t[0]) <= ref * (1 + 2e-6)       # an upper bound: never below the norm


def test_image_conversions(cuda):
    """f32 -> bf16, the [hi | lo] split image and the scaled f16 image, bit for bit against torch's round to nearest even."""
    g = torch.Generator().manual_seed(40)
    n, d = 3001, 128
    x = (torch.randn((n + 8, d), generator=g) * torch.rand((n + 8, 1), generator=g)).cuda()
    x[n:] = float("nan")
    cnt = n * d
    y = Buf(cnt, torch.bfloat16)
    run_twice(lambda: L().sss_f32_to_bf16(x.data_ptr(), cnt, y.ptr, _st()), [y])
    assert torch.equal(_bits(y.t), _bits(x[:n].reshape(-1).bfloat16()))
    sp = Buf((n, 2 * d), torch.bfloat16)
    run_twice(lambda: L().sss_split_bf16(x.data_ptr(), n, d, sp.ptr, _st()), [sp])
    hi = x[:n].bfloat16()
    lo = (x[:n] - hi.float()).bfloat16()
    assert torch.equal(_bits(sp.t), _bits(torch.cat([hi, lo], 1)))
    shift = int(L().sss_f16_shift(float(x[:n].abs().max())))
    f16 = Buf(cnt, torch.float16)
    run_twice(lambda: L().sss_scale_f16(x.data_ptr(), cnt, shift, f16.ptr, _st()), [f16])
    assert torch.equal(_bits(f16.t), _bits((x[:n] * 2.0 ** shift).half().reshape(-1)))


def test_image_maxima(cuda):
    """sss_abs_max and sss_f16_resid_max: one atomically maximised float each (the caller zeroes it); rows past n
    hold values that would set the maximum."""
    g = torch.Generator().manual_seed(41)
    n, d = 5001, 128
    x = torch.randn((n + 16, d), generator=g).cuda()
    x[n:] = -1e5
    out = Buf(1, torch.float32, zero=True)
    assert L().sss_abs_max(x.data_ptr(), n * d, out.ptr, _st()) == 0
    torch.cuda.synchronize()
    assert out.guards_ok() and float(out.t[0]) == float(x[:n].abs().max())
    shift = int(L().sss_f16_shift(float(out.t[0])))
    img = (x * 2.0 ** shift).clamp(-65504, 65504).half()
    img[n:] = 0                                                          # residual of the tail rows: 1e5
    res = Buf(1, torch.float32, zero=True)
    assert L().sss_f16_resid_max(x.data_ptr(), img.data_ptr(), n, d, shift, res.ptr, _st()) == 0
    torch.cuda.synchronize()
    S = bir.max_resid_sumsq_exact(x[:n].cpu().numpy(), img[:n].cpu().numpy(), shift)      # exact: no float64 norm that may round either way
    got = float(res.t[0])
    assert res.guards_ok() and bir.is_upper_bound(got, S) and got <= math.sqrt(float(S)) * (1 + 1e-5)


# ------------------------------------------------------------------------------------------------ encoder pieces
def test_gather_rows(cuda):
    g = torch.Generator().manual_seed(50)
    table = torch.randn((500, 64), generator=g).cuda()
    ids = torch.randint(0, 500, (333,), generator=g).cuda()
    out = Buf((333, 76), torch.float32)
    run_twice(lambda: L().sss_gather_rows(table.data_ptr(), ids.data_ptr(), 333, 64, out.ptr, 76, _st()), [out],
              written=[_cols_mask((333, 76), 64)])
    assert torch.equal(out.t[:, :64], table[ids])


def test_gather_concat_rows(cuda):
    g = torch.Generator().manual_seed(51)
    table, feat = torch.randn((40, 32), generator=g), torch.randn((77, 64), generator=g)
    ids = torch.randint(0, 40, (77,), generator=g)
    fb = _strided(feat, 72)
    td, idd = table.cuda(), ids.cuda()
    out = Buf((77, 140), torch.float32)
    run_twice(lambda: L().sss_gather_concat_rows(td.data_ptr(), idd.data_ptr(), 32, fb.ptr, 72, 64, 8, 77, out.ptr, 140, _st()),
              [out], written=[_cols_mask((77, 140), 104)])
    assert torch.equal(out.t[:, :104].cpu(), torch.cat([table[ids], feat, torch.zeros(77, 8)], 1))
    run_twice(lambda: L().sss_gather_concat_rows(0, 0, 0, fb.ptr, 72, 64, 32, 77, out.ptr, 140, _st()), [out],
              written=[_cols_mask((77, 140), 96)])
    assert torch.equal(out.t[:, :96].cpu(), torch.cat([feat, torch.zeros(77, 32)], 1))


def _lin_tol(ref, k):
    return 2e-6 * max(float(ref.abs().max()), 1.0) * np.sqrt(k / 32)


@pytest.mark.parametrize("n,m,k", [(130, 108, 96), (1001, 37, 64)])
def test_linear(cuda, n, m, k):
    g = torch.Generator().manual_seed(n + m)
    x, w, b = torch.randn((n, k), generator=g), torch.randn((m, k), generator=g), torch.randn(m, generator=g)
    xb, wb, bb = _strided(x, k + 8), _strided(w, k + 4), dev_buf(b)
    y = Buf((n, m + 5), torch.float32)
    run_twice(lambda: L().sss_linear(xb.ptr, k + 8, wb.ptr, k + 4, bb.ptr, y.ptr, m + 5, n, m, k, _st()), [y],
              written=[_cols_mask((n, m + 5), m)])
    ref = x.double() @ w.double().T + b.double()
    assert (y.t[:, :m].cpu().double() - ref).abs().max() <= _lin_tol(ref, k)


def test_linear_grouped(cuda):
    """Two problems in one launch: gather mode (rows = table[ids], copied to xcopy) and strided rows with the tanh
    epilogue and a post scale / shift."""
    g = torch.Generator().manual_seed(52)
    K, n1, n2, m1, m2 = 64, 301, 77, 90, 33
    table = torch.randn((200, K), generator=g)
    ids = torch.randint(0, 200, (n1,), generator=g)
    x2 = torch.randn((n2, K), generator=g)
    w1, w2 = torch.randn((m1, K), generator=g) * 0.2, torch.randn((m2, K), generator=g) * 0.2
    b1 = torch.randn(m1, generator=g)
    sc, sh = torch.rand(m2, generator=g) + 0.5, torch.randn(m2, generator=g) * 0.1
    td, idd, x2b, w1b, w2b, b1d = table.cuda(), ids.cuda(), _strided(x2, K + 4), _strided(w1, K + 8), dev_buf(w2), dev_buf(b1)
    scd, shd = sc.cuda(), sh.cuda()
    y1, y2, xc = Buf((n1, m1 + 3), torch.float32), Buf((n2, m2 + 7), torch.float32), Buf((n1, K + 4), torch.float32)
    P = _lib.LinearProblem
    arr = (P * 2)(P(x=0, ldx=0, ids=idd.data_ptr(), table=td.data_ptr(), xcopy=xc.ptr, ld_xcopy=K + 4, w=w1b.ptr, ldw=K + 8,
                    bias=b1d.ptr, y=y1.ptr, ldy=m1 + 3, n=n1, m=m1, act=0),
                  P(x=x2b.ptr, ldx=K + 4, ids=0, table=0, xcopy=0, ld_xcopy=0, w=w2b.ptr, ldw=K, bias=0, y=y2.ptr, ldy=m2 + 7,
                    n=n2, m=m2, act=2, post_scale=scd.data_ptr(), post_shift=shd.data_ptr()))
    run_twice(lambda: L().sss_linear_grouped(arr, 2, K, _st()), [y1, y2, xc],
              written=[_cols_mask((n1, m1 + 3), m1), _cols_mask((n2, m2 + 7), m2), _cols_mask((n1, K + 4), K)])
    r1 = table[ids].double() @ w1.double().T + b1.double()
    r2 = torch.relu(torch.tanh(x2.double() @ w2.double().T) * sc.double() + sh.double())
    assert (y1.t[:, :m1].cpu().double() - r1).abs().max() <= _lin_tol(r1, K)
    assert (y2.t[:, :m2].cpu().double() - r2).abs().max() <= _lin_tol(r2, K)
    assert torch.equal(xc.t[:, :K].cpu(), table[ids])


def _csr(rng, n_src, n_dst, e):
    src, dst = rng.integers(0, n_src, e), rng.integers(0, n_dst, e)
    dst[: min(n_dst, 5)] = np.arange(min(n_dst, 5))
    src[: min(n_dst, 5)] = np.arange(min(n_dst, 5))                  # src == dst edges (dropped by the self-loop rewrite)
    order = np.argsort(dst, kind="stable")
    rowptr = np.zeros(n_dst + 1, np.int32)
    np.cumsum(np.bincount(dst, minlength=n_dst), out=rowptr[1:])
    return rowptr, src[order].astype(np.int32)


@pytest.mark.parametrize("n_self_loop", [0, 29])
def test_gat_aggregate(cuda, n_self_loop):
    rng = np.random.default_rng(53)
    ns, nd, h = 37, 29, 64
    g = torch.Generator().manual_seed(53)
    xs, a_s, a_d, b = torch.randn((ns, h), generator=g), torch.randn(ns, generator=g), torch.randn(nd, generator=g), torch.randn(h, generator=g)
    rowptr, col = _csr(rng, ns, nd, 90)
    xsb = _strided(xs, h + 4)
    asb = _strided(a_s[:, None], 3)                                    # strided scalars, NaN in between
    adb = _strided(a_d[:, None], 2)
    rpb, colb, bb = dev_buf(torch.from_numpy(rowptr)), dev_buf(torch.from_numpy(col)), dev_buf(b)
    out = Buf((nd, h + 8), torch.float32)
    run_twice(lambda: L().sss_gat_aggregate(xsb.ptr, h + 4, asb.ptr, 3, adb.ptr, 2, rpb.ptr, colb.ptr, nd, h, bb.ptr, 0, n_self_loop,
                                            out.ptr, h + 8, _st()), [out], written=[_cols_mask((nd, h + 8), h)])
    ref = _gat_ref(xs.double(), a_s.double(), a_d.double(), rowptr, col, nd, b.double(), n_self_loop)
    assert (out.t[:, :h].cpu().double() - ref).abs().max() < 2e-5


def test_csr_weighted_sum_and_gru(cuda):
    rng = np.random.default_rng(54)
    g = torch.Generator().manual_seed(54)
    n, h, dx = 50, 64, 40
    m = torch.randn((n, h), generator=g)
    rowptr, col = _csr(rng, n, n, 120)
    w = torch.rand(len(col), generator=g) + 0.5
    mb, rpb, colb, wb = _strided(m, h + 4), dev_buf(torch.from_numpy(rowptr)), dev_buf(torch.from_numpy(col)), dev_buf(w)
    for use_w in (False, True):
        out = Buf((n, h + 4), torch.float32)
        run_twice(lambda: L().sss_csr_weighted_sum(mb.ptr, h + 4, rpb.ptr, colb.ptr, wb.ptr if use_w else 0, n, h, out.ptr, h + 4,
                                                   _st()), [out], written=[_cols_mask((n, h + 4), h)])
        ref = torch.zeros((n, h), dtype=torch.float64)
        for i in range(n):
            for e in range(rowptr[i], rowptr[i + 1]):
                ref[i] += (float(w[e]) if use_w else 1.0) * m[col[e]].double()
        assert (out.t[:, :h].cpu().double() - ref).abs().max() < 2e-5
    gi, gh, x, add = (torch.randn((n, 3 * h), generator=g), torch.randn((n, 3 * h), generator=g), torch.randn((n, dx), generator=g),
                      torch.randn((n, h), generator=g))
    gib, ghb, xb, addb = _strided(gi, 3 * h + 4), _strided(gh, 3 * h + 8), _strided(x, dx + 28), _strided(add, h + 4)
    for use_add in (False, True):
        out = Buf((n, h + 4), torch.float32)
        run_twice(lambda: L().sss_gru_combine(gib.ptr, 3 * h + 4, ghb.ptr, 3 * h + 8, xb.ptr, dx + 28, dx, addb.ptr if use_add else 0,
                                              h + 4, n, h, out.ptr, h + 4, _st()), [out], written=[_cols_mask((n, h + 4), h)])
        ref = _gru_ref(gi.double(), gh.double(), x.double(), add.double() if use_add else None)
        assert (out.t[:, :h].cpu().double() - ref).abs().max() < 3e-5


@pytest.mark.parametrize("table_mode", [False, True])
def test_hetero_layer_update(cuda, table_mode):
    """One HeteroGGNN layer after the transforms, against a float64 restatement of the column layout of
    include/sss.h (GAT q->p + GatedGraphConv + GRU + sum + relu per product, GAT p->q + relu per query)."""
    rng = np.random.default_rng(55)
    g = torch.Generator().manual_seed(55)
    n_p, n_q, h, dx = 150, 90, 64, 48
    n_rows_p, n_rows_q = (400, 70) if table_mode else (n_p, n_q)          # table rows (table mode) or node rows
    yp = torch.randn((n_rows_p, 7 * h + 2), generator=g) * 0.5
    yq = torch.randn((n_rows_q, h + 2), generator=g) * 0.5
    xin = torch.randn((n_rows_p, dx), generator=g)
    xq_tab = torch.randn((n_rows_q, dx), generator=g)
    row_p = torch.from_numpy(rng.integers(0, n_rows_p, n_p)) if table_mode else torch.arange(n_p)
    row_q = torch.from_numpy(rng.integers(0, n_rows_q, n_q)) if table_mode else torch.arange(n_q)
    rp_qp, c_qp = _csr(rng, n_q, n_p, 300)
    rp_pq, c_pq = _csr(rng, n_p, n_q, 300)
    rp_pp, c_pp = _csr(rng, n_p, n_p, 400)
    w_pp = torch.rand(len(c_pp), generator=g) + 0.5
    bias_qp, bias_pq, b_ih = torch.randn(h, generator=g), torch.randn(h, generator=g), torch.randn(3 * h, generator=g)
    nsl = min(n_p, n_q)
    ypb, yqb, xinb = _strided(yp, 7 * h + 8), _strided(yq, h + 8), _strided(xin, dx + 12)      # 16-byte row strides
    xqb = _strided(xq_tab, dx + 4)
    ib = lambda a: dev_buf(torch.from_numpy(a))
    bufs = dict(rp_qp=ib(rp_qp), c_qp=ib(c_qp), rp_pq=ib(rp_pq), c_pq=ib(c_pq), rp_pp=ib(rp_pp), c_pp=ib(c_pp), w_pp=dev_buf(w_pp),
                bqp=dev_buf(bias_qp), bpq=dev_buf(bias_pq), bih=dev_buf(b_ih), row_p=dev_buf(row_p), row_q=dev_buf(row_q))
    out_p, out_q = Buf((n_p, h + 4), torch.float32), Buf((n_q, h + 12), torch.float32)
    outs, written = [out_p, out_q], [_cols_mask((n_p, h + 4), h), _cols_mask((n_q, h + 12), h)]
    x0p = x0q = None
    if table_mode:
        x0p, x0q = Buf((n_p, dx + 8), torch.float32), Buf((n_q, dx + 4), torch.float32)
        outs += [x0p, x0q]
        written += [_cols_mask((n_p, dx + 8), dx), _cols_mask((n_q, dx + 4), dx)]
    la = _lib.LayerArgs(yp=ypb.ptr, ld_yp=7 * h + 8, yq=yqb.ptr, ld_yq=h + 8, h=h, d_x=dx, rowptr_qp=bufs["rp_qp"].ptr,
                        col_qp=bufs["c_qp"].ptr, rowptr_pp=bufs["rp_pp"].ptr, col_pp=bufs["c_pp"].ptr, w_pp=bufs["w_pp"].ptr,
                        bias_qp=bufs["bqp"].ptr, b_ih=bufs["bih"].ptr, xin_p=xinb.ptr, ld_xin=dx + 12, out_p=out_p.ptr,
                        ld_out_p=h + 4, np=n_p, rowptr_pq=bufs["rp_pq"].ptr, col_pq=bufs["c_pq"].ptr, bias_pq=bufs["bpq"].ptr,
                        out_q=out_q.ptr, ld_out_q=h + 12, nq=n_q, n_self_loop=nsl,
                        row_p=bufs["row_p"].ptr if table_mode else 0, row_q=bufs["row_q"].ptr if table_mode else 0,
                        x0_p=x0p.ptr if table_mode else 0, ld_x0_p=dx + 8, xq_table=xqb.ptr if table_mode else 0,
                        ld_xq=dx + 4, x0_q=x0q.ptr if table_mode else 0, ld_x0_q=dx + 4)
    run_twice(lambda: L().sss_hetero_layer_update(ctypes.byref(la), _st()), outs, written=written)
    Yp, Yq, X = yp.double()[row_p], yq.double()[row_q], xin.double()[row_p]
    gat_p = _gat_ref(Yq[:, :h], Yq[:, h], Yp[:, 7 * h + 1], rp_qp, c_qp, n_p, bias_qp.double(), nsl)
    gi = torch.zeros((n_p, 3 * h), dtype=torch.float64)
    for i in range(n_p):
        for e in range(rp_pp[i], rp_pp[i + 1]):
            gi[i] += float(w_pp[e]) * Yp[c_pp[e], h:4 * h]
    ref_p = _gru_ref(gi + b_ih.double(), Yp[:, 4 * h:7 * h], X, gat_p)
    ref_q = torch.relu(_gat_ref(Yp[:, :h], Yp[:, 7 * h], Yq[:, h + 1], rp_pq, c_pq, n_q, bias_pq.double(), nsl))
    assert (out_p.t[:, :h].cpu().double() - ref_p).abs().max() < 5e-5 * max(1.0, float(ref_p.abs().max()))
    assert (out_q.t[:, :h].cpu().double() - ref_q).abs().max() < 5e-5 * max(1.0, float(ref_q.abs().max()))
    if table_mode:
        assert torch.equal(x0p.t[:, :dx].cpu(), xin[row_p]) and torch.equal(x0q.t[:, :dx].cpu(), xq_tab[row_q])


def _pool_setup(cuda, seed):
    cfg = EncoderConfig(d_in=32, h=32, n_layers=1, d_out=96, n_items=300, n_query=33)
    w = init_weights(cfg, seed)
    b = S.build_batch(S.synthetic_actions(37, seed, 300, 33))
    enc = SessionEncoder(cfg, w, cuda)
    pb = enc.prepare(b.to(cuda))
    g = torch.Generator().manual_seed(seed)
    W = cfg.node_width
    nq_, np_ = torch.randn((pb.Nq, W), generator=g), torch.randn((pb.Np, W), generator=g)
    bt = b.to_torch("cpu")
    ref = gnn_ref.pos_att_pool(nq_, np_, bt["query"].pos_emb_id, bt["query"].batch, bt["product"].cnt,
                               bt["product"].pos_emb_id, bt["product"].batch, bt.num_graphs, w)
    pw = enc.pool
    Dl = cfg.d_out - cfg.max_seq_len
    lin_p = np_.double() @ pw["wp"].cpu().double().T + pw["bp"].cpu().double()
    lin_q = nq_.double() @ pw["wq"].cpu().double().T + pw["bq"].cpu().double()
    return cfg, enc, pb, ref, lin_p.float(), lin_q.float(), Dl


def test_pool_expand_mean_attention(cuda):
    cfg, enc, pb, ref, lin_p, lin_q, Dl = _pool_setup(cuda, 56)
    D, P, pw = cfg.d_out, cfg.max_seq_len, enc.pool
    ldl = Dl + 4
    lpb, lqb = _strided(lin_p, ldl), _strided(lin_q, ldl)
    n_exp = pb.n_clicks + pb.Nq
    node, coarse = Buf((n_exp, D + 4), torch.float32), Buf((pb.B, D + 8), torch.float32)
    run_twice(lambda: L().sss_pool_expand_mean(lpb.ptr, lqb.ptr, ldl, pb.src_row.data_ptr(), pb.pos_id.data_ptr(), pb.pptr.data_ptr(),
                                               pb.qptr.data_ptr(), pb.n_clicks, pb.B, Dl, P, pw["pos"].data_ptr(), node.ptr, D + 4,
                                               coarse.ptr, D + 8, _st()), [node, coarse],
              written=[_cols_mask((n_exp, D + 4), D), _cols_mask((pb.B, D + 8), D)])
    nd, cd = node.t[:, :D].cpu().double(), coarse.t[:, :D].cpu().double()
    A = nd @ pw["wn"].cpu().double().T + pw["bn"].cpu().double()
    Bc = cd @ pw["wc"].cpu().double().T
    nb, Ab, Bb = _strided(nd, D + 4), _strided(A, D + 12), _strided(Bc, D + 4)
    for normalize in (0, 1):
        out = Buf((pb.B, D + 4), torch.float32)
        run_twice(lambda: L().sss_pool_attention(nb.ptr, D + 4, Ab.ptr, D + 12, Bb.ptr, D + 4, pw["watt"].data_ptr(), pb.pptr.data_ptr(),
                                                 pb.qptr.data_ptr(), pb.n_clicks, pb.B, D, normalize, 1e-6, 0, out.ptr, D + 4, _st()),
                  [out], written=[_cols_mask((pb.B, D + 4), D)])
        r = ref.numpy() if not normalize else sr.normalize(ref.numpy())
        assert np.abs(out.t[:, :D].cpu().numpy() - r).max() < TOL * max(1.0, float(np.abs(r).max()))


def test_pool_expand_segment_pool(cuda):
    cfg, enc, pb, ref, lin_p, lin_q, Dl = _pool_setup(cuda, 57)
    D, P, pw = cfg.d_out, cfg.max_seq_len, enc.pool
    ldl = Dl + 8
    lpb, lqb = _strided(lin_p, ldl), _strided(lin_q, ldl)
    n_exp = pb.n_clicks + pb.Nq
    node = Buf((n_exp, D + 4), torch.float32)
    run_twice(lambda: L().sss_pool_expand(lpb.ptr, lqb.ptr, ldl, pb.src_row.data_ptr(), pb.pos_id.data_ptr(), pb.n_clicks, n_exp, Dl, P,
                                          pw["pos"].data_ptr(), node.ptr, D + 4, _st()), [node],
              written=[_cols_mask((n_exp, D + 4), D)])
    nd = node.t[:, :D].cpu().double()
    nb = _strided(nd, D + 4)
    coarse = Buf((pb.B, D + 4), torch.float32)
    run_twice(lambda: L().sss_segment_pool(nb.ptr, D + 4, pb.pptr.data_ptr(), pb.qptr.data_ptr(), pb.n_clicks, pb.B, D, 0, 0, 0, 0, 0,
                                           coarse.ptr, D + 4, _st()), [coarse], written=[_cols_mask((pb.B, D + 4), D)])
    A = nd @ pw["wn"].cpu().double().T + pw["bn"].cpu().double()
    Bc = coarse.t[:, :D].cpu().double() @ pw["wc"].cpu().double().T
    Ab, Bb = _strided(A, D + 12), _strided(Bc, D + 4)
    out = Buf((pb.B, D + 4), torch.float32)
    run_twice(lambda: L().sss_segment_pool(nb.ptr, D + 4, pb.pptr.data_ptr(), pb.qptr.data_ptr(), pb.n_clicks, pb.B, D, Ab.ptr, D + 12,
                                           Bb.ptr, D + 4, pw["watt"].data_ptr(), out.ptr, D + 4, _st()), [out],
              written=[_cols_mask((pb.B, D + 4), D)])
    assert np.abs(out.t[:, :D].cpu().numpy() - ref.numpy()).max() < TOL * max(1.0, float(ref.abs().max()))


def test_pool_attention_tab(cuda):
    """The fused pooling: t = tanh(lin) with NaN past d_lin, ac = [A1 | C1] formed in float64; normalised output."""
    cfg, enc, pb, ref, lin_p, lin_q, Dl = _pool_setup(cuda, 58)
    D, P, pw, pt = cfg.d_out, cfg.max_seq_len, enc.pool, enc.pool_tab
    T = torch.tanh(torch.cat([lin_p, lin_q]).double())
    wn, wc = pw["wn"].cpu().double(), pw["wc"].cpu().double()
    AC = torch.cat([T @ wn[:, :Dl].T, T @ wc[:, :Dl].T], 1)
    Tb, ACb = _strided(T, pt["KT"] + 4), _strided(AC, 2 * D + 4)
    out = Buf((pb.B, D + 4), torch.float32)
    run_twice(lambda: L().sss_pool_attention_tab(Tb.ptr, pt["KT"] + 4, ACb.ptr, 2 * D + 4, pt["tanhpos"].data_ptr(), pt["a2"].data_ptr(),
                                                 pt["c2"].data_ptr(), pw["watt"].data_ptr(), pb.src_row.data_ptr(), pb.pos_id.data_ptr(),
                                                 pb.pptr.data_ptr(), pb.qptr.data_ptr(), pb.n_clicks, pb.Np, pb.B, Dl, P, 1, 1e-6,
                                                 out.ptr, D + 4, _st()), [out], written=[_cols_mask((pb.B, D + 4), D)])
    r = sr.normalize(ref.numpy())
    assert np.abs(out.t[:, :D].cpu().numpy() - r).max() < TOL


def test_segment_ptr(cuda):
    batch = np.sort(np.random.default_rng(59).choice(np.r_[0:3, 5:9, 12], 500))          # graphs 3, 4, 9-11, 13 empty
    bb = dev_buf(torch.from_numpy(batch))
    ptr = Buf(15, torch.int32)
    run_twice(lambda: L().sss_segment_ptr(bb.ptr, 500, 14, ptr.ptr, _st()), [ptr])
    assert np.array_equal(ptr.t.cpu().numpy(), np.searchsorted(batch, np.arange(15), "left"))


def _segments():
    ptr = np.array([0, 5, 5, 17, 18, 40, 40, 77], np.int32)                           # two empty segments
    return ptr, len(ptr) - 1


def test_csr_mean(cuda):
    rng = np.random.default_rng(60)
    g = torch.Generator().manual_seed(60)
    n_src, n_dst, d = 80, 45, 96
    rowptr, col = _csr(rng, n_src, n_dst, 150)
    a, b = rowptr[10], rowptr[11]                                                      # drop target 10's edges: an empty row
    col = np.r_[col[:a], col[b:]].astype(np.int32)
    rowptr[11:] -= b - a
    x = torch.randn((n_src, d), generator=g)
    xb, rpb, cb = _strided(x, d + 4), dev_buf(torch.from_numpy(rowptr)), dev_buf(torch.from_numpy(col))
    out = Buf((n_dst, d + 4), torch.float32)
    run_twice(lambda: L().sss_csr_mean(xb.ptr, d + 4, rpb.ptr, cb.ptr, n_dst, d, out.ptr, d + 4, _st()), [out],
              written=[_cols_mask((n_dst, d + 4), d)])
    ref = torch.stack([x.double()[col[rowptr[i]:rowptr[i + 1]]].mean(0) if rowptr[i + 1] > rowptr[i]
                       else torch.zeros(d, dtype=torch.float64) for i in range(n_dst)])
    assert (out.t[:, :d].cpu().double() - ref).abs().max() < TOL


@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("use_w", [False, True])
def test_segment_reduce(cuda, mode, use_w):
    g = torch.Generator().manual_seed(61 + mode)
    ptr, G = _segments()
    d = 96
    x = torch.randn((int(ptr[-1]), d), generator=g)
    w = torch.rand(int(ptr[-1]), generator=g) * 2 - 0.5
    xb, wb, pb_ = _strided(x, d + 8), dev_buf(w), dev_buf(torch.from_numpy(ptr))
    out = Buf((G, d + 4), torch.float32)
    run_twice(lambda: L().sss_segment_reduce(xb.ptr, d + 8, wb.ptr if use_w else 0, pb_.ptr, G, d, mode, out.ptr, d + 4, _st()),
              [out], written=[_cols_mask((G, d + 4), d)])
    xs = x.double() * (w.double()[:, None] if use_w else 1.0)
    ref = torch.zeros((G, d), dtype=torch.float64)
    for s in range(G):
        seg = xs[ptr[s]:ptr[s + 1]]
        if len(seg):
            ref[s] = seg.mean(0) if mode == 0 else seg.sum(0) if mode == 1 else seg.max(0).values
    assert (out.t[:, :d].cpu().double() - ref).abs().max() < TOL * max(1.0, float(ref.abs().max()))


def test_attention_dot_pool(cuda):
    g = torch.Generator().manual_seed(62)
    ptr, G = _segments()
    d = 96
    x = torch.randn((int(ptr[-1]), d), generator=g)
    xb, pb_ = _strided(x, d + 4), dev_buf(torch.from_numpy(ptr))
    out = Buf((G, d + 8), torch.float32)
    run_twice(lambda: L().sss_attention_dot_pool(xb.ptr, d + 4, pb_.ptr, G, d, out.ptr, d + 8, _st()), [out],
              written=[_cols_mask((G, d + 8), d)])
    ref = torch.zeros((G, d), dtype=torch.float64)
    for s in range(G):
        seg = x.double()[ptr[s]:ptr[s + 1]]
        if len(seg):
            ref[s] = (seg * (seg @ seg.mean(0))[:, None]).mean(0)
    assert (out.t[:, :d].cpu().double() - ref).abs().max() < 2 * TOL * max(1.0, float(ref.abs().max()))


# ------------------------------------------------------------------------------------------------ graph builder
def _graph_oracle(acts):
    from oracle import graph_ref
    o = graph_ref.collate([graph_ref.session_to_graph(s_) for s_ in graph_ref.actions_to_sessions(acts)])
    Nq, Np = len(o["q_x"]), len(o["p_x"])

    def csr(src, dst, n_dst, w=None):
        order = np.argsort(dst, kind="stable")
        rowptr = np.zeros(n_dst + 1, np.int64)
        np.cumsum(np.bincount(dst, minlength=n_dst), out=rowptr[1:])
        return rowptr, src[order], None if w is None else w[order]
    return o, Nq, Np, csr(o["qp0"], o["qp1"], Np), csr(o["qp1"], o["qp0"], Nq), csr(o["pp0"], o["pp1"], Np, o["pp_w"])


def _graph_inputs(acts, extra=5):
    """The action table as device arrays, with `extra` further sessions after the last one (not to be read)."""
    more = S.synthetic_actions(extra, 99, 300, 33)
    n_act = int(acts.sess_ptr[-1])
    ptr = np.r_[acts.sess_ptr, n_act + more.sess_ptr[1:]].astype(np.int64)
    cat = lambda a, b: np.r_[a, b]
    return (dev_buf(torch.from_numpy(ptr)), dev_buf(torch.from_numpy(cat(acts.is_search, more.is_search).astype(np.uint8))),
            dev_buf(torch.from_numpy(cat(acts.item_id, more.item_id).astype(np.int64))),
            dev_buf(torch.from_numpy(cat(acts.query_tok, more.query_tok).astype(np.int64))))


def test_graph_builder(cuda):
    acts = S.synthetic_actions(301, 63, 300, 33)
    Sn = 301
    sp, isr, item, tok = _graph_inputs(acts)
    bases, err = Buf((5, Sn + 1), torch.int32), Buf(1, torch.int32)
    scratch = Buf(int(L().sss_graph_scratch_ints(Sn)), torch.int32)
    run_twice(lambda: L().sss_graph_counts(sp.ptr, isr.ptr, item.ptr, Sn, bases.ptr, scratch.ptr, err.ptr, _st()), [bases, err], [scratch])
    assert int(err.t[0]) == 0
    Nq, Np, Xp, E, Epp = (int(v) for v in bases.t[:, Sn].cpu())
    o, Nq_r, Np_r, (rp_qp, c_qp, _), (rp_pq, c_pq, _), (rp_pp, c_pp, w_pp) = _graph_oracle(acts)
    assert (Nq, Np, E, Epp) == (Nq_r, Np_r, len(c_qp), len(c_pp))
    i32, i64, f32 = torch.int32, torch.int64, torch.float32
    spec = [("q_x", Nq, i64), ("q_batch", Nq, i64), ("q_pos", Nq, i32), ("p_x", Np, i64), ("p_batch", Np, i64), ("p_cnt", Np, i64),
            ("rowptr_qp", Np + 1, i32), ("col_qp", E, i32), ("rowptr_pq", Nq + 1, i32), ("col_pq", E, i32),
            ("rowptr_pp", Np + 1, i32), ("col_pp", Epp, i32), ("w_pp", Epp, f32), ("src_row", Xp + Nq, i32), ("pos_id", Xp + Nq, i32)]
    outs = {name: Buf(size, dt) for name, size, dt in spec}
    go = _lib.GraphOut(**{name: b.ptr for name, b in outs.items()})
    run_twice(lambda: L().sss_graph_fill(sp.ptr, isr.ptr, item.ptr, tok.ptr, Sn, bases.ptr, ctypes.byref(go), _st()), list(outs.values()))
    npy = lambda name: outs[name].t.cpu().numpy().astype(np.int64)
    for name, want in (("rowptr_qp", rp_qp), ("col_qp", c_qp), ("rowptr_pq", rp_pq), ("col_pq", c_pq), ("rowptr_pp", rp_pp),
                       ("col_pp", c_pp), ("q_x", o["q_x"]), ("p_x", o["p_x"]), ("q_batch", o["q_batch"]), ("p_batch", o["p_batch"]),
                       ("p_cnt", o["p_cnt"])):
        assert np.array_equal(npy(name), want), name
    assert np.array_equal(outs["w_pp"].t.cpu().numpy(), w_pp)
    assert np.array_equal(npy("src_row"), np.r_[np.repeat(np.arange(Np), o["p_cnt"]), np.arange(Nq)])
    assert np.array_equal(npy("pos_id"), np.r_[o["p_pos"], o["q_pos"]])
    qptr = np.r_[0, np.cumsum(np.bincount(o["q_batch"], minlength=Sn))]
    assert np.array_equal(bases.t[0].cpu().numpy(), qptr)
    assert np.array_equal(bases.t[2].cpu().numpy(), np.r_[0, np.cumsum(np.bincount(o["p_batch"], weights=o["p_cnt"], minlength=Sn))])


# ------------------------------------------------------------------------------------------------ binary codes, vote
def test_pack_sign_bits(cuda):
    rng = np.random.default_rng(64)
    n, c, ldx, nbytes = 501, 250, 260, 40                           # ceil(250 / 8) = 32 < 40: padding bytes
    x = rng.choice(np.array([-1, 1, 0, 2.5, -3, 0.999], np.float32), (n, c))
    xb = _strided(torch.from_numpy(x), ldx)
    out = Buf((n, nbytes), torch.uint8)
    run_twice(lambda: L().sss_pack_sign_bits(xb.ptr, n, c, ldx, out.ptr, nbytes, _st()), [out])
    ref = np.zeros((n, nbytes), np.uint8)
    ref[:, :32] = np.packbits(((x + 1) / 2).astype(int), axis=1)
    assert np.array_equal(out.t.cpu().numpy(), ref)


@pytest.mark.parametrize("nbytes", [16, 32, 64])
def test_hamming(cuda, nbytes):
    """Fused top-k (k = 10, 100) with tail rows equal to the query codes; exhaustive on a qsel subset, also k > n."""
    rng = np.random.default_rng(65 + nbytes)
    nq = 50
    for n, k, fused in ((70001, 10, True), (20011, 100, True), (300, 400, False), (5003, 33, False)):
        codes = rng.integers(0, 256, (n + 64, nbytes), dtype=np.uint8)
        q = rng.integers(0, 256, (nq + 4, nbytes), dtype=np.uint8)
        codes[n:] = np.resize(q[:nq], (64, nbytes))
        codes[7:400:3] = codes[7]                                    # duplicated rows: ties broken by id
        q[5] = codes[7]
        cb, qb = dev_buf(torch.from_numpy(codes)), dev_buf(torch.from_numpy(q))
        Dr, Ir = sr.hamming_search(q[:nq], codes[:n], k, OFF)
        D, I = Buf((nq, k), torch.int32), Buf((nq, k), torch.int64)
        if fused:
            assert k <= L().sss_hamming_topk_capacity(nq, n)
            status = Buf(nq, torch.int32)
            ws = Buf(int(L().sss_hamming_topk_workspace_bytes(nq, n)), torch.uint8)
            for p in (0, 1):
                for b in (D, I, status, ws):
                    b.poison(p)
                assert L().sss_hamming_topk(qb.ptr, nq, cb.ptr, n, nbytes, k, OFF, D.ptr, I.ptr, status.ptr, ws.ptr, ws.nbytes, _st()) == 0
                torch.cuda.synchronize()
                assert all(b.guards_ok() for b in (D, I, status, ws))
                ok = status.t.cpu().numpy() == 0
                assert np.array_equal(I.t.cpu().numpy()[ok], Ir[ok]) and np.array_equal(D.t.cpu().numpy()[ok], Dr[ok])
                assert (I.t.cpu().numpy() < OFF + n).all()
        else:
            sel = np.r_[5, 0, 3:nq:4].astype(np.int32)
            qsel = dev_buf(torch.from_numpy(sel))
            ws = Buf(int(L().sss_hamming_topk_exhaustive_workspace_bytes(len(sel), n)), torch.uint8)
            run_twice(lambda: L().sss_hamming_topk_exhaustive(qb.ptr, qsel.ptr, len(sel), cb.ptr, n, nbytes, k, OFF, D.ptr, I.ptr,
                                                              ws.ptr, ws.nbytes, _st()), [D, I], [ws],
                      written=[_rows_mask((nq, k), sel)] * 2)
            assert np.array_equal(I.t.cpu().numpy()[sel], Ir[sel]) and np.array_equal(D.t.cpu().numpy()[sel], Dr[sel])


def _vote_case(rng, nq=24, s=256, n_sessions=4000):
    sizes = rng.integers(1, 81, n_sessions + 10)
    sizes[:300] = 80                                                  # big sessions: the heavy queries below use them
    items = [rng.choice(3000, size=z, replace=False).astype(np.int32) for z in sizes]
    ptr = np.r_[0, np.cumsum(sizes)].astype(np.int64)                 # 10 more sessions after n_sessions (not to be read)
    D = -np.sort(-rng.random((nq, s)).astype(np.float32), axis=1)
    I = rng.integers(0, n_sessions, (nq, s)).astype(np.int64)
    I[0::3, :] = rng.integers(0, 300, (len(range(0, nq, 3)), s))     # 256 x 80 pairs > 16384: status 1
    I[1::3, 70:] = -1                                                 # 70 x ~40 pairs: first launch
    I[2::3, :] = rng.integers(0, 300, (len(range(2, nq, 3)), s))
    I[2::3, 90:] = -1                                                 # 90 x 80 = 7200 pairs: the second launch
    D[I < 0] = 0
    return D, np.where(I >= 0, I + OFF, -1), ptr, items


def test_knn_item_vote(cuda):
    rng = np.random.default_rng(66)
    nq, s, k, n_sessions = 24, 256, 20, 4000
    D, I, ptr, items = _vote_case(rng, nq, s, n_sessions)
    Db, Ib, pb_, ib = dev_buf(torch.from_numpy(D)), dev_buf(torch.from_numpy(I)), dev_buf(torch.from_numpy(ptr)), dev_buf(
        torch.from_numpy(np.concatenate(items)))
    oi, ow, st = Buf((nq, k), torch.int64), Buf((nq, k), torch.float64), Buf(nq, torch.int32)
    run_twice(lambda: L().sss_knn_item_vote(Db.ptr, Ib.ptr, nq, s, pb_.ptr, ib.ptr, OFF, n_sessions, k, oi.ptr, ow.ptr, st.ptr, _st()),
              [oi, ow, st])
    status = st.t.cpu().numpy()
    assert (status[0::3] == 1).all() and (status[1::3] == 0).all() and (status[2::3] == 0).all()
    got_i, got_w = oi.t.cpu().numpy(), ow.t.cpu().numpy()
    assert (got_i[status == 1] == -1).all()
    for r in np.flatnonzero(status == 0):
        ri, rw = sr.knn_item_vote_weights(D[r], np.where(I[r] >= 0, I[r] - OFF, -1), items, k)
        assert got_i[r, :len(ri)].tolist() == ri and (got_i[r, len(ri):] == -1).all(), r
        assert got_w[r, :len(rw)].tolist() == rw, r


# ------------------------------------------------------------------------------------------------ streams
SLEEP_CYCLES = 20_000_000


def _on_side_stream(overwrite, call, read):
    """On a fresh stream: a sleep, then `overwrite` (new input data), then `call(stream)`, then `read()`; all of it
    queued on that stream with no sync in between.  A launch, memset or copy that lands on another stream (or a
    host sync) sees the old data."""
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        torch.cuda._sleep(SLEEP_CYCLES)
        overwrite()
        assert call(s) == 0, L().sss_last_error()
        out = read()
    s.synchronize()
    return out


def test_streams_search_family(cuda):
    C = corpus(70001, 128, 150, "f32", seed=128 + 70001)
    nq, n, d, k = C.nq, C.n, C.d, 10
    rng = np.random.default_rng(67)
    new_q = torch.from_numpy(_unit_rows(rng, nq, d)).cuda()
    old_q = C.q_t[:nq].clone()
    C2 = Corpus.__new__(Corpus)
    C2.__dict__.update(C.__dict__)
    C2.q = new_q.cpu().numpy()
    C2._oracle = {}
    Dr, Ir = C2.oracle(k)
    over = lambda: C.q_t[:nq].copy_(new_q)

    def restore():
        C.q_t[:nq].copy_(old_q)
        torch.cuda.synchronize()
    D, I, status = (torch.empty((nq, k), device=cuda), torch.empty((nq, k), dtype=torch.int64, device=cuda),
                    torch.empty(nq, dtype=torch.int32, device=cuda))
    ws = Buf(_fused_ws_bytes("f16", nq, n, d, k), torch.uint8)
    state = Buf(int(L().sss_ip_topk_state_bytes(nq)), torch.uint8, align=16, zero=True)
    C.f16()
    # fused search (f16 scan)
    got = _on_side_stream(over, lambda s: _fused_call("f16", C, k, D.data_ptr(), I.data_ptr(), status.data_ptr(), state, ws, stream=s),
                          lambda: (D.clone(), I.clone(), status.clone()))
    _check_search(*got, (Dr, Ir), n)
    restore()
    # threshold rung on every query (bounds from the fused search just made)
    sel = dev_buf(torch.arange(nq, dtype=torch.int32))
    wst = Buf(int(L().sss_ip_topk_threshold_workspace_bytes(nq, n, d, 3)), torch.uint8)
    D0, I0 = got[0].clone(), got[1].clone()

    def over_rung():
        over()
        D.copy_(D0), I.copy_(I0), status.fill_(1)
    got = _on_side_stream(over_rung, lambda s: L().sss_ip_topk_threshold(C.q_t.data_ptr(), sel.ptr, nq, C.c_t.data_ptr(), 0, C._f16.data_ptr(), 3,
                                                                         C.shift, C.resid, n, d, k, OFF, C.cmax, D.data_ptr(),
                                                                         I.data_ptr(), status.data_ptr(), wst.ptr, wst.nbytes, _st(s)),
                          lambda: (D.clone(), I.clone(), status.clone()))
    assert int(got[2].abs().sum()) == 0
    _check_search(*got, (Dr, Ir), n)
    restore()
    # exhaustive
    wse = Buf(int(L().sss_ip_topk_exhaustive_workspace_bytes(nq, n)), torch.uint8)
    got = _on_side_stream(over, lambda s: L().sss_ip_topk_exhaustive(C.q_t.data_ptr(), sel.ptr, nq, C.c_t.data_ptr(), n, d, k, 0, OFF, 0,
                                                                     D.data_ptr(), I.data_ptr(), wse.ptr, wse.nbytes, _st(s)),
                          lambda: (D.clone(), I.clone()))
    assert np.array_equal(got[1].cpu().numpy(), Ir) and np.array_equal(got[0].cpu().numpy(), Dr)
    restore()
    # range (exhaustive route): count then fill, both on the side stream
    rad = torch.from_numpy(Dr[:, 4].copy()).cuda()
    cnt = torch.empty(nq, dtype=torch.int64, device=cuda)
    wsr = Buf(int(L().sss_range_search_exhaustive_workspace_bytes(nq, n)), torch.uint8)
    got = _on_side_stream(over, lambda s: L().sss_range_search_exhaustive_count(C.q_t.data_ptr(), sel.ptr, nq, C.c_t.data_ptr(), n, d, 0, 0,
                                                                                rad.data_ptr(), cnt.data_ptr(), wsr.ptr, wsr.nbytes, _st(s)),
                          lambda: cnt.clone())
    assert (got.cpu().numpy() == 4).all()
    lims = torch.arange(0, 4 * nq + 1, 4, dtype=torch.int64, device=cuda)
    Dg, Ig = torch.empty(4 * nq, device=cuda), torch.empty(4 * nq, dtype=torch.int64, device=cuda)
    got = _on_side_stream(lambda: None, lambda s: L().sss_range_search_exhaustive_fill(sel.ptr, nq, n, 0, rad.data_ptr(), lims.data_ptr(), OFF,
                                                                                      Dg.data_ptr(), Ig.data_ptr(), wsr.ptr, wsr.nbytes,
                                                                                      _st(s)), lambda: Ig.clone())
    assert np.array_equal(got.view(nq, 4).cpu().numpy(), np.sort(Ir[:, :4], axis=1))
    restore()


def test_streams_long_scan(cuda):
    C = corpus(3001, 1600, 24, "f32", seed=1600 + 3001)
    nq, n, d, k = C.nq, C.n, C.d, 100
    new_q = torch.from_numpy(_unit_rows(np.random.default_rng(68), nq, d)).cuda()
    Dr, Ir = sr.search_exact(new_q.cpu().numpy(), C.c, k, id_offset=OFF)
    img = C.f16()
    D, I, status = (torch.empty((nq, k), device=cuda), torch.empty((nq, k), dtype=torch.int64, device=cuda),
                    torch.empty(nq, dtype=torch.int32, device=cuda))
    ws = Buf(int(L().sss_ip_topk_long_workspace_bytes(nq, n, d, 0)), torch.uint8)
    old = C.q_t[:nq].clone()
    got = _on_side_stream(lambda: C.q_t[:nq].copy_(new_q),
                          lambda s: L().sss_ip_topk_long(C.q_t.data_ptr(), nq, C.c_t.data_ptr(), 0, img.data_ptr(), C.shift, C.resid, n, d, k,
                                                         OFF, C.cmax, D.data_ptr(), I.data_ptr(), status.data_ptr(), ws.ptr, ws.nbytes, _st(s)),
                          lambda: (D.clone(), I.clone(), status.clone()))
    C.q_t[:nq].copy_(old)
    _check_search(*got, (Dr, Ir), n)


def test_streams_hamming_vote_graph_encoder(cuda):
    rng = np.random.default_rng(69)
    # Hamming: the query codes are overwritten on the side stream
    nq, n, nb, k = 40, 20011, 32, 10
    codes = torch.from_numpy(rng.integers(0, 256, (n, nb), dtype=np.uint8)).cuda()
    q = torch.zeros((nq, nb), dtype=torch.uint8, device=cuda)
    new_q = rng.integers(0, 256, (nq, nb), dtype=np.uint8)
    nq_t = torch.from_numpy(new_q).cuda()
    Dr, Ir = sr.hamming_search(new_q, codes.cpu().numpy(), k, OFF)
    D, I, status = (torch.empty((nq, k), dtype=torch.int32, device=cuda), torch.empty((nq, k), dtype=torch.int64, device=cuda),
                    torch.empty(nq, dtype=torch.int32, device=cuda))
    ws = Buf(int(L().sss_hamming_topk_workspace_bytes(nq, n)), torch.uint8)
    got = _on_side_stream(lambda: q.copy_(nq_t), lambda s: L().sss_hamming_topk(q.data_ptr(), nq, codes.data_ptr(), n, nb, k, OFF, D.data_ptr(),
                                                                                 I.data_ptr(), status.data_ptr(), ws.ptr, ws.nbytes, _st(s)),
                          lambda: (D.clone(), I.clone(), status.clone()))
    ok = got[2].cpu().numpy() == 0
    assert ok.any() and np.array_equal(got[1].cpu().numpy()[ok], Ir[ok]) and np.array_equal(got[0].cpu().numpy()[ok], Dr[ok])
    # vote: the neighbour lists are overwritten
    Dv, Iv, ptr, items = _vote_case(rng)
    Dd, Id = torch.zeros(Dv.shape, device=cuda), torch.full(Iv.shape, -1, dtype=torch.int64, device=cuda)
    Dn, In = torch.from_numpy(Dv).cuda(), torch.from_numpy(Iv).cuda()
    pt, it = torch.from_numpy(ptr).cuda(), torch.from_numpy(np.concatenate(items)).cuda()
    oi, st = torch.empty((24, 20), dtype=torch.int64, device=cuda), torch.empty(24, dtype=torch.int32, device=cuda)
    got = _on_side_stream(lambda: (Dd.copy_(Dn), Id.copy_(In)),
                          lambda s: L().sss_knn_item_vote(Dd.data_ptr(), Id.data_ptr(), 24, 256, pt.data_ptr(), it.data_ptr(), OFF, 4000, 20,
                                                          oi.data_ptr(), 0, st.data_ptr(), _st(s)), lambda: (oi.clone(), st.clone()))
    for r in np.flatnonzero(got[1].cpu().numpy() == 0):
        ri, _ = sr.knn_item_vote_weights(Dv[r], np.where(Iv[r] >= 0, Iv[r] - OFF, -1), items, 20)
        assert got[0][r, :len(ri)].tolist() == ri
    # graph builder: the item ids are overwritten (counts and fill both on the side stream)
    acts = S.synthetic_actions(120, 70, 300, 33)
    Sn = 120
    sp, isr, item, tok = (torch.from_numpy(np.asarray(a)).cuda() for a in
                          (acts.sess_ptr.astype(np.int64), acts.is_search.astype(np.uint8), acts.item_id.astype(np.int64),
                           acts.query_tok.astype(np.int64)))
    new_item = item.clone()
    item.zero_()
    bases, err = torch.empty((5, Sn + 1), dtype=torch.int32, device=cuda), torch.empty(1, dtype=torch.int32, device=cuda)
    scratch = torch.empty(int(L().sss_graph_scratch_ints(Sn)), dtype=torch.int32, device=cuda)
    tot = _on_side_stream(lambda: item.copy_(new_item),
                          lambda s: L().sss_graph_counts(sp.data_ptr(), isr.data_ptr(), item.data_ptr(), Sn, bases.data_ptr(),
                                                         scratch.data_ptr(), err.data_ptr(), _st(s)), lambda: bases[:, Sn].clone())
    o, Nq, Np, (rp_qp, c_qp, _), _, _ = _graph_oracle(acts)
    assert int(tot[0]) == Nq and int(tot[1]) == Np
    # encoder forward, the item table overwritten on the side stream before the forward that reads it
    cfg = EncoderConfig(d_in=64, h=64, n_layers=2, d_out=64, n_items=500, n_query=65)
    w = init_weights(cfg, 71)
    enc = SessionEncoder(cfg, w, cuda)
    b = S.build_batch(S.synthetic_actions(40, 71, 500, 65))
    new_tab = torch.randn(w["item_table"].shape, generator=torch.Generator().manual_seed(72))
    w2 = dict(w, item_table=new_tab)
    ref = gnn_ref.encoder_forward(b.to_torch("cpu"), w2, cfg.n_layers)
    nt = new_tab.to(cuda)
    bd = b.to(cuda)
    out = []
    got = _on_side_stream(lambda: enc.item_table.copy_(nt), lambda s: out.append(enc(bd)) or 0, lambda: out[0].clone())
    assert (got.cpu() - ref).abs().max() < TOL * max(1.0, float(ref.abs().max()))


def test_concurrent_searches_on_two_streams(cuda):
    """two FlatIndex objects over the same rows, searched on two streams at once while a
    third stream's GEMMs hold CUs.  Results exact after fix_unproven, states zero.  sss_scan_boot_expired (the scans'
    bounded inter-workgroup wait giving up) is reported, not asserted."""
    from sessionsimilaritysearch_amd.index import FlatIndex
    rng = np.random.default_rng(73)
    n, d, nq = 300001, 128, 256
    xb = torch.from_numpy(_unit_rows(rng, n, d)).cuda()
    qa = torch.from_numpy(_unit_rows(rng, nq, d)).cuda()
    qb = torch.from_numpy(_unit_rows(rng, nq, d)).cuda()
    big = torch.randn((8192, 8192), device=cuda)
    xh = xb.cpu().numpy()
    L().sss_scan_boot_expired(1)
    for k in (10, 100):
        ia, ib = FlatIndex(d, "ip", cuda).adopt(xb), FlatIndex(d, "ip", cuda).adopt(xb)
        ia.prepare(k), ib.prepare(k)
        torch.cuda.synchronize()
        s1, s2, s3 = torch.cuda.Stream(), torch.cuda.Stream(), torch.cuda.Stream()
        with torch.cuda.stream(s3):
            for _ in range(6):
                big = big @ big * 1e-4
        with torch.cuda.stream(s1):
            ra = ia.search_fused(qa, k)
        with torch.cuda.stream(s2):
            rb = ib.search_fused(qb, k)
        torch.cuda.synchronize()
        for idx, q, (D, I, status) in ((ia, qa, ra), (ib, qb, rb)):
            assert not bool(idx._state.any()), "state not zero after a concurrent search"
            idx.fix_unproven(q, k, D, I, status)
            Dr, Ir = sr.search_exact(q.cpu().numpy(), xh, k)
            assert np.array_equal(I.cpu().numpy(), Ir) and np.array_equal(D.cpu().numpy(), Dr)
    expired = L().sss_scan_boot_expired(0)
    print(f"\nsss_scan_boot_expired after the concurrent searches: {expired}")
    assert expired >= 0
