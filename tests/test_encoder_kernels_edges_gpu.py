"""The fused encoder kernels of csrc/gnn_fused.hip at their shape and structure edges, through the C ABI, each case against the
float64 restatement of oracle/encoder_kernels_ref.py (itself pinned to oracle/gnn_ref64.py on the CPU by
tests/test_encoder_kernels_ref_cpu.py, which also proves every case generated here well formed).

Buffers are the guarded / strided ones of tests/test_abi_contract_gpu.py: row strides wider than the rows, NaN in input
padding, output padding and guard bands must come back untouched (a dead-lane bug shows there first).

Bound of every floating-point output (`_close`): e_ref = max |float32 restatement - float64 restatement| of the SAME case,
and the kernel must satisfy max |kernel - float64| <= 4 * e_ref + one float32 ulp of the case's largest output (4x: the
margin of test_encoder_matches_oracle for equally valid summation orders -- online softmax, slot-wise partial sums).
Cases on O(1) inputs also hold the fixed bounds of the older tests (1e-5 relative on pooled vectors, 5e-5 on node outputs).
Exact copies (x0_p, x0_q) are compared bit for bit.

Width -> lane-group size (LPR, `lanes_for`) -> case id; every templated kernel is run at every width of its row:
    width   4   8  12*  16  20*  32  36*  64  96* 100* 128 132* 160* 192* 224* 252* 256 | 260* 800* 1600*
    LPR     1   2   4    4   8    8  16   16  32   32   32  64   64   64   64   64   64 |  64   64    64
    (* = dead lanes in the group, or for the wide rows a last column chunk that is not full)
  k_layer_update           test_layer_widths[<width>-node|table]
  k_gat_aggregate, k_csr_weighted_sum, k_gru_combine    test_per_op_kernels_widths[<width>]
  k_pool_expand_mean       test_pool_expand_mean[<width>-<graphs>]
  k_pool_attention         test_pool_attention_and_segment_pool[<width>-<graphs>]   (width <= 256)
  k_segment_pool           test_pool_attention_and_segment_pool[<width>-<graphs>]   (every width through sss_segment_pool,
                           260 / 800 / 1600 also through sss_pool_attention: mean, sum, normalise)
  k_pool_attention_tab     test_pool_attention_tab[<width>-<graphs>]
Measured on one MI355X: the file (245 cases) runs in 14 s, most of it the float64 loops.
"""
import ctypes

import numpy as np
import pytest
import torch

from oracle import encoder_kernels_ref as kr
from oracle import gnn_ref, gnn_ref64
from sessionsimilaritysearch_amd import _lib
from sessionsimilaritysearch_amd import sessions as S
from sessionsimilaritysearch_amd.encoder import EncoderConfig, SessionEncoder, init_weights
from test_abi_contract_gpu import Buf, L, _cols_mask, _st, _strided, dev_buf, run_twice

pytestmark = pytest.mark.gpu

TOL = 1e-5            # pooled vectors on O(1) inputs (tests/test_encoder_gpu.py)
NODE_TOL = 5e-5       # node outputs on O(1) inputs


def _close(name, got, r64, r32, rel=None):
    """finite, and no further from float64 than 4x the float32 restatement is (+ one ulp of the largest output)."""
    got = got.detach().cpu().double()
    assert got.shape == r64.shape, (name, got.shape, r64.shape)
    if got.numel() == 0:
        return
    assert torch.isfinite(got).all(), f"{name}: non-finite output"
    err, e_ref, top = float((got - r64).abs().max()), float((r32.double() - r64).abs().max()), float(r64.abs().max())
    floor = float(np.spacing(np.float32(top)))
    print(f"{name}: err {err:.3e}  e_ref {e_ref:.3e}  floor {floor:.1e}  max|ref| {top:.3e}  err/(4 e_ref + floor) {err / (4 * e_ref + floor):.2f}")
    assert err <= 4 * e_ref + floor, f"{name}: {err:.3e} > 4 * {e_ref:.3e} + {floor:.1e}"
    if rel is not None:
        assert err < rel * max(1.0, top), f"{name}: {err:.3e} over the fixed bound {rel}"


def _ib(a):
    return dev_buf(torch.from_numpy(np.ascontiguousarray(a)))


def _pad4(n, extra=4):
    return (n + 3) // 4 * 4 + extra


# ================================================================================================ layer update
def _run_layer(c):
    """sss_hetero_layer_update on case `c` in guarded buffers -> (out_p, out_q, x0_p, x0_q) on the CPU."""
    h, dx, n_p, n_q = c.h, c.d_x, c.n_p, c.n_q
    ldyp, ldyq, ldx, ldxq = 7 * h + 8, h + 8, _pad4(dx, 8), _pad4(dx)
    ypb, yqb, xinb, xqb = _strided(c.yp, ldyp), _strided(c.yq, ldyq), _strided(c.xin, ldx), _strided(c.xq_tab, ldxq)
    keep = [ypb, yqb, xinb, xqb]
    ib = {k: _ib(getattr(c, k)) for k in ("rp_qp", "c_qp", "rp_pq", "c_pq", "rp_pp", "c_pp")}
    fb = {k: dev_buf(getattr(c, k)) for k in ("bias_qp", "bias_pq", "b_ih")}
    wb = None if c.w_pp is None else dev_buf(c.w_pp)
    rpb = None if c.row_p is None else dev_buf(c.row_p)
    rqb = None if c.row_q is None else dev_buf(c.row_q)
    ldo_p, ldo_q, ld0p, ld0q = h + 4, h + 12, _pad4(dx, 8), _pad4(dx)
    out_p, out_q = Buf((n_p, ldo_p), torch.float32), Buf((n_q, ldo_q), torch.float32)
    x0p, x0q = Buf((n_p, ld0p), torch.float32), Buf((n_q, ld0q), torch.float32)
    la = _lib.LayerArgs(yp=ypb.ptr, ld_yp=ldyp, yq=yqb.ptr, ld_yq=ldyq, h=h, d_x=dx, rowptr_qp=ib["rp_qp"].ptr, col_qp=ib["c_qp"].ptr,
                        rowptr_pp=ib["rp_pp"].ptr, col_pp=ib["c_pp"].ptr, w_pp=0 if wb is None else wb.ptr, bias_qp=fb["bias_qp"].ptr,
                        b_ih=fb["b_ih"].ptr, xin_p=xinb.ptr, ld_xin=ldx, out_p=out_p.ptr, ld_out_p=ldo_p, np=n_p,
                        rowptr_pq=ib["rp_pq"].ptr, col_pq=ib["c_pq"].ptr, bias_pq=fb["bias_pq"].ptr, out_q=out_q.ptr, ld_out_q=ldo_q,
                        nq=n_q, n_self_loop=c.n_self_loop, row_p=0 if rpb is None else rpb.ptr, row_q=0 if rqb is None else rqb.ptr,
                        x0_p=x0p.ptr, ld_x0_p=ld0p, xq_table=xqb.ptr, ld_xq=ldxq, x0_q=x0q.ptr, ld_x0_q=ld0q)
    run_twice(lambda: L().sss_hetero_layer_update(ctypes.byref(la), _st()), [out_p, out_q, x0p, x0q],
              written=[_cols_mask((n_p, ldo_p), h), _cols_mask((n_q, ldo_q), h), _cols_mask((n_p, ld0p), dx), _cols_mask((n_q, ld0q), dx)])
    for b in (*keep, *ib.values(), *fb.values(), *(x for x in (wb, rpb, rqb) if x is not None)):
        assert b.guards_ok()
    return out_p.t[:, :h].cpu(), out_q.t[:, :h].cpu(), x0p.t[:, :dx].cpu(), x0q.t[:, :dx].cpu()


def _check_layer(c, rel=NODE_TOL):
    kr.check_layer_case(c)
    got = _run_layer(c)
    r64, r32 = kr.layer_update_ref(c, torch.float64), kr.layer_update_ref(c, torch.float32)
    tag = f"layer[{c.structure} h={c.h} {'table' if c.table_mode else 'node'}]"
    _close(tag + " out_p", got[0], r64[0], r32[0], rel)
    _close(tag + " out_q", got[1], r64[1], r32[1], rel)
    assert torch.equal(got[2], r64[2]) and torch.equal(got[3], r64[3]), tag + ": x0 copies differ"
    return got, r64


@pytest.mark.parametrize("mode", ["node", "table"])
@pytest.mark.parametrize("h", kr.WIDTHS)
def test_layer_widths(cuda, h, mode):
    """Every lane-group size of k_layer_update; d_x = 3h/4 is mostly no multiple of 4 (scalar tails of the x / x0 copies)."""
    _check_layer(kr.layer_case("random", h, mode == "table", seed=1))


_O1 = [s for s in kr.LAYER_STRUCTURES if not s.startswith(("logits", "gru_sat"))]


@pytest.mark.parametrize("mode", ["node", "table"])
@pytest.mark.parametrize("h", [64, 100])
@pytest.mark.parametrize("structure", _O1)
def test_layer_structures(cuda, structure, h, mode):
    """One named graph structure per case (see oracle.encoder_kernels_ref.layer_case), at a full lane group (64) and at
    one with dead lanes (100)."""
    c = kr.layer_case(structure, h, mode == "table", seed=2)
    got, r64 = _check_layer(c)
    if structure in ("no_edges", "all_self_edges"):
        # the GAT term of a query is its bias, or its lone self edge (softmax weight 1 / (1 + 1e-16) == 1): exact in float32
        rp = torch.arange(c.n_p) if c.row_p is None else c.row_p
        want = c.bias_pq.repeat(c.n_q, 1)
        want[:c.n_self_loop] += c.yp[rp][:c.n_self_loop, :h]
        assert torch.equal(got[1], torch.relu(want))


@pytest.mark.parametrize("mode", ["node", "table"])
@pytest.mark.parametrize("h", [64, 100])
@pytest.mark.parametrize("structure", ["logits_asc", "logits_desc", "logits_shuffled"])
def test_layer_large_logits(cuda, structure, h, mode):
    """|leaky_relu argument| up to ~80: a softmax without its maximum overflows float32 (exp(80)); the online softmax
    must not, in whatever order the scores arrive (ascending: every edge rescales the running sums)."""
    _check_layer(kr.layer_case(structure, h, mode == "table", seed=3), rel=None)


@pytest.mark.parametrize("mode", ["node", "table"])
@pytest.mark.parametrize("h", [64, 100])
@pytest.mark.parametrize("structure", ["gru_sat_30", "gru_sat_100"])
def test_layer_saturated_gates(cuda, structure, h, mode):
    """GRU pre-activations of +-30 / +-100 / +-120: expf overflows inside the kernel's sigmoid, the result must still be
    the limit value.  The case has no q-p edges, so the GAT term is exactly bias_qp and where float64 says z is 1 (0) to
    float32 precision the output is exactly relu(bias + x) (relu(bias + tanh limit))."""
    c = kr.layer_case(structure, h, mode == "table", seed=4)
    got, _ = _check_layer(c, rel=None)
    rp = torch.arange(c.n_p) if c.row_p is None else c.row_p
    Yp = c.yp[rp].double()
    gi = torch.cat([kr.csr_weighted_sum_ref(Yp[:, (1 + k) * h:(2 + k) * h], c.rp_pp, c.c_pp, c.w_pp.double(), c.n_p) for k in range(3)], 1)
    _, z, n = kr.gru_gates(gi + c.b_ih.double(), Yp[:, 4 * h:7 * h])
    xp = torch.nn.functional.pad(c.xin[rp], (0, h - c.d_x))
    one, zero = z.float() == 1, (z.float() == 0) & (n.float().abs() == 1)
    assert one.any() and (structure == "gru_sat_30" or zero.any())
    assert torch.equal(got[0][one], torch.relu(c.bias_qp + xp)[one])
    assert torch.equal(got[0][zero], torch.relu(c.bias_qp + n.float())[zero])


# ================================================================================================ per-op kernels
@pytest.mark.parametrize("h", kr.WIDTHS)
def test_per_op_kernels_widths(cuda, h):
    """sss_gat_aggregate (with / without the rewrite, with / without relu), sss_csr_weighted_sum (with / without
    weights) and sss_gru_combine (with / without add) at every lane-group size, on the arrays of a layer case."""
    c = kr.check_layer_case(kr.layer_case("hub", h, False, seed=5))
    xs, a_s, a_d = c.yq[:, :h].contiguous(), c.yq[:, h].contiguous(), c.yp[:, 7 * h + 1].contiguous()
    xsb, asb, adb = _strided(xs, h + 4), _strided(a_s[:, None], 3), _strided(a_d[:, None], 2)
    rpb, colb, bb = _ib(c.rp_qp), _ib(c.c_qp), dev_buf(c.bias_qp)
    for nsl, relu in ((0, 0), (c.n_self_loop, 1)):
        out = Buf((c.n_p, h + 8), torch.float32)
        run_twice(lambda: L().sss_gat_aggregate(xsb.ptr, h + 4, asb.ptr, 3, adb.ptr, 2, rpb.ptr, colb.ptr, c.n_p, h, bb.ptr, relu, nsl,
                                                out.ptr, h + 8, _st()), [out], written=[_cols_mask((c.n_p, h + 8), h)])
        ref = [kr.gat_ref(xs.to(t), a_s.to(t), a_d.to(t), c.rp_qp, c.c_qp, c.n_p, c.bias_qp.to(t), nsl) for t in (torch.float64, torch.float32)]
        ref = [torch.relu(r) if relu else r for r in ref]
        _close(f"gat[h={h} loops={nsl} relu={relu}]", out.t[:, :h], ref[0], ref[1], 2e-5)
    m = c.yp[:, h:2 * h].contiguous()
    mb, rp2, col2, wb = _strided(m, h + 4), _ib(c.rp_pp), _ib(c.c_pp), dev_buf(c.w_pp)
    for use_w in (False, True):
        out = Buf((c.n_p, h + 4), torch.float32)
        run_twice(lambda: L().sss_csr_weighted_sum(mb.ptr, h + 4, rp2.ptr, col2.ptr, wb.ptr if use_w else 0, c.n_p, h, out.ptr, h + 4,
                                                   _st()), [out], written=[_cols_mask((c.n_p, h + 4), h)])
        ref = [kr.csr_weighted_sum_ref(m.to(t), c.rp_pp, c.c_pp, c.w_pp.to(t) if use_w else None, c.n_p) for t in (torch.float64, torch.float32)]
        _close(f"csr_sum[h={h} w={use_w}]", out.t[:, :h], ref[0], ref[1], 2e-5)
    gi, gh, x, add = c.yp[:, h:4 * h].contiguous(), c.yp[:, 4 * h:7 * h].contiguous(), c.xin, c.yp[:, :h].contiguous()
    ldx = _pad4(c.d_x, 8)
    gib, ghb, xb, addb = _strided(gi, 3 * h + 4), _strided(gh, 3 * h + 8), _strided(x, ldx), _strided(add, h + 4)
    for use_add in (False, True):
        out = Buf((c.n_p, h + 4), torch.float32)
        run_twice(lambda: L().sss_gru_combine(gib.ptr, 3 * h + 4, ghb.ptr, 3 * h + 8, xb.ptr, ldx, c.d_x, addb.ptr if use_add else 0,
                                              h + 4, c.n_p, h, out.ptr, h + 4, _st()), [out], written=[_cols_mask((c.n_p, h + 4), h)])
        ref = [kr.gru_ref(gi.to(t), gh.to(t), x.to(t), add.to(t) if use_add else None) for t in (torch.float64, torch.float32)]
        _close(f"gru[h={h} add={use_add}]", out.t[:, :h], ref[0], ref[1], 3e-5)


@pytest.mark.parametrize("structure", ["gru_sat_30", "gru_sat_100"])
def test_gru_combine_saturated(cuda, structure):
    """sss_gru_combine with gh of +-30 / +-100 / +-120: finite, within the measured bound, and exactly the limit
    expression relu(add + x) (relu(add +- 1)) where float64 puts z at 1 (at 0, with a saturated tanh) in float32."""
    h = 100
    c = kr.layer_case(structure, h, False, seed=6)
    gi, gh, x, add = c.yp[:, h:4 * h].contiguous(), c.yp[:, 4 * h:7 * h].contiguous(), c.xin, c.yp[:, :h].contiguous()
    ldx = _pad4(c.d_x, 8)
    gib, ghb, xb, addb = _strided(gi, 3 * h + 4), _strided(gh, 3 * h + 8), _strided(x, ldx), _strided(add, h + 4)
    out = Buf((c.n_p, h + 4), torch.float32)
    run_twice(lambda: L().sss_gru_combine(gib.ptr, 3 * h + 4, ghb.ptr, 3 * h + 8, xb.ptr, ldx, c.d_x, addb.ptr, h + 4, c.n_p, h, out.ptr,
                                          h + 4, _st()), [out], written=[_cols_mask((c.n_p, h + 4), h)])
    got = out.t[:, :h].cpu()
    ref = [kr.gru_ref(gi.to(t), gh.to(t), x.to(t), add.to(t)) for t in (torch.float64, torch.float32)]
    _close(f"gru[{structure}]", got, ref[0], ref[1])
    _, z, n = kr.gru_gates(gi.double(), gh.double())
    xp = torch.nn.functional.pad(x, (0, h - c.d_x))
    one, zero = z.float() == 1, (z.float() == 0) & (n.float().abs() == 1)
    assert one.any() and (structure == "gru_sat_30" or zero.any())
    assert torch.equal(got[one], torch.relu(add + xp)[one]) and torch.equal(got[zero], torch.relu(add + n.float())[zero])


# ================================================================================================ pooling
_POOL_CASES = ([(D, kr.pool_p_for(D), "lengths") for D in kr.WIDTHS] +
               [(D, kr.pool_p_for(D), k) for D in (12, 96, 100, 256) for k in ("interleaved", "single")] +
               [(D, P, "lengths") for D in (96, 132) for P in (18, 22)])              # d_lin % 4 == 2: columns straddle lin | pos
_POOL_IDS = [f"{D}-P{P}-{k}" for D, P, k in _POOL_CASES]
_WIDE_CASES = [(D, 20, k) for D in kr.WIDE for k in ("lengths", "interleaved")]


def _t(x, t):
    return x.to(t)


@pytest.mark.parametrize("D,P,kind", _POOL_CASES, ids=_POOL_IDS)
def test_pool_expand_mean(cuda, D, P, kind):
    c = kr.check_pool_case(kr.pool_case(D, P, kind, seed=7))
    ldl = c.Dl + 5                                                    # lin is read element-wise: no alignment asked
    lpb, lqb, posb = _strided(c.lin_p, ldl), _strided(c.lin_q, ldl), dev_buf(c.pos_emb)
    srb, pib, ppb, qpb = _ib(c.src_row), _ib(c.pos_id), _ib(c.pptr), _ib(c.qptr)
    node, coarse = Buf((c.n_exp, D + 4), torch.float32), Buf((c.B, D + 8), torch.float32)
    run_twice(lambda: L().sss_pool_expand_mean(lpb.ptr, lqb.ptr, ldl, srb.ptr, pib.ptr, ppb.ptr, qpb.ptr, c.n_clicks, c.B, c.Dl, P, posb.ptr,
                                               node.ptr, D + 4, coarse.ptr, D + 8, _st()), [node, coarse],
              written=[_cols_mask((c.n_exp, D + 4), D), _cols_mask((c.B, D + 8), D)])
    ref = [kr.pool_expand_mean_ref(_t(c.lin_p, t), _t(c.lin_q, t), c.src_row, c.pos_id, c.pptr, c.qptr, c.n_clicks, c.B, _t(c.pos_emb, t))
           for t in (torch.float64, torch.float32)]
    _close(f"expand_mean[{D} P{P} {kind}] node", node.t[:, :D], ref[0][0], ref[1][0], TOL)
    _close(f"expand_mean[{D} P{P} {kind}] coarse", coarse.t[:, :D], ref[0][1], ref[1][1], TOL)


@pytest.mark.parametrize("D,P,kind", _POOL_CASES + _WIDE_CASES, ids=_POOL_IDS + [f"{D}-P{P}-{k}" for D, P, k in _WIDE_CASES])
def test_pool_attention_and_segment_pool(cuda, D, P, kind):
    """sss_pool_attention (mean, mean + normalise, sum; D > 256 runs k_segment_pool's wide branches) and
    sss_segment_pool (plain mean with watt == NULL, attention mean) on the same graphs."""
    c = kr.check_pool_case(kr.pool_case(D, P, kind, seed=8))
    nb, ab, bb, wb = _strided(c.node, D + 4), _strided(c.a, D + 12), _strided(c.b, D + 4), dev_buf(c.watt)
    ppb, qpb = _ib(c.pptr), _ib(c.qptr)
    args = lambda t: (_t(c.node, t), _t(c.a, t), _t(c.b, t), _t(c.watt, t), c.pptr, c.qptr, c.n_clicks, c.B)
    for normalize, rsum in ((0, 0), (1, 0), (0, 1)):
        out = Buf((c.B, D + 4), torch.float32)
        run_twice(lambda: L().sss_pool_attention(nb.ptr, D + 4, ab.ptr, D + 12, bb.ptr, D + 4, wb.ptr, ppb.ptr, qpb.ptr, c.n_clicks, c.B, D,
                                                 normalize, 1e-6, rsum, out.ptr, D + 4, _st()), [out], written=[_cols_mask((c.B, D + 4), D)])
        ref = [kr.pool_attention_ref(*args(t), bool(normalize), 1e-6, bool(rsum)) for t in (torch.float64, torch.float32)]
        _close(f"pool_attention[{D} {kind} norm={normalize} sum={rsum}]", out.t[:, :D], ref[0], ref[1], TOL)
    for use_w in (False, True):
        out = Buf((c.B, D + 4), torch.float32)
        run_twice(lambda: L().sss_segment_pool(nb.ptr, D + 4, ppb.ptr, qpb.ptr, c.n_clicks, c.B, D, ab.ptr if use_w else 0, D + 12,
                                               bb.ptr if use_w else 0, D + 4, wb.ptr if use_w else 0, out.ptr, D + 4, _st()), [out],
                  written=[_cols_mask((c.B, D + 4), D)])
        ref = [kr.segment_pool_ref(_t(c.node, t), c.pptr, c.qptr, c.n_clicks, c.B, _t(c.a, t), _t(c.b, t), _t(c.watt, t) if use_w else None)
               for t in (torch.float64, torch.float32)]
        _close(f"segment_pool[{D} {kind} watt={use_w}]", out.t[:, :D], ref[0], ref[1], TOL)


def _run_tab(c, normalize):
    D, P = c.D, c.P
    ldt = c.Dl + 5                                                    # t is read element-wise
    tb, acb = _strided(c.t, ldt), _strided(c.ac, 2 * D + 4)
    tpb, a2b, c2b, wb = dev_buf(c.tanhpos), dev_buf(c.a2tab), dev_buf(c.c2tab), dev_buf(c.watt)
    srb, pib, ppb, qpb = _ib(c.src_row), _ib(c.pos_id), _ib(c.pptr), _ib(c.qptr)
    out = Buf((c.B, D + 4), torch.float32)
    run_twice(lambda: L().sss_pool_attention_tab(tb.ptr, ldt, acb.ptr, 2 * D + 4, tpb.ptr, a2b.ptr, c2b.ptr, wb.ptr, srb.ptr, pib.ptr, ppb.ptr,
                                                 qpb.ptr, c.n_clicks, c.n_p, c.B, c.Dl, P, normalize, 1e-6, out.ptr, D + 4, _st()), [out],
              written=[_cols_mask((c.B, D + 4), D)])
    ref = [kr.pool_attention_tab_ref(_t(c.t, t), _t(c.ac, t), _t(c.tanhpos, t), _t(c.a2tab, t), _t(c.c2tab, t), _t(c.watt, t), c.src_row,
                                     c.pos_id, c.pptr, c.qptr, c.n_clicks, c.n_p, c.B, c.Dl, bool(normalize)) for t in (torch.float64, torch.float32)]
    return out.t[:, :D], ref


@pytest.mark.parametrize("D,P,kind", _POOL_CASES, ids=_POOL_IDS)
def test_pool_attention_tab(cuda, D, P, kind):
    """Graphs of 0 .. 200 rows: the 64-row chunk loop, the row-slot butterflies (width 4 / 8 / 16: 64 / 32 / 16 slots per
    wave), one slot per wave at width 132 .. 256."""
    c = kr.check_pool_case(kr.pool_case(D, P, kind, seed=9))
    for normalize in (0, 1):
        got, ref = _run_tab(c, normalize)
        _close(f"pool_attention_tab[{D} P{P} {kind} norm={normalize}]", got, ref[0], ref[1], TOL)


@pytest.mark.parametrize("D", [100, 256])
def test_pooling_saturated(cuda, D):
    """tanh / sigmoid inputs of the order of +-100 (up to several hundred) in all three pooling kernels: finite and
    within the measured bound (the fixed 1e-5 does not apply at these magnitudes)."""
    c = kr.check_pool_case(kr.pool_case(D, 20, "lengths", seed=10, scale=100.0))
    assert float(c.a.abs().max()) > 300 and float(c.lin_p.abs().max()) > 300
    got, ref = _run_tab(c, 0)
    _close(f"pool_attention_tab[{D} x100]", got, ref[0], ref[1])
    nb, ab, bb, wb = _strided(c.node, D + 4), _strided(c.a, D + 12), _strided(c.b, D + 4), dev_buf(c.watt)
    ppb, qpb = _ib(c.pptr), _ib(c.qptr)
    out = Buf((c.B, D + 4), torch.float32)
    run_twice(lambda: L().sss_pool_attention(nb.ptr, D + 4, ab.ptr, D + 12, bb.ptr, D + 4, wb.ptr, ppb.ptr, qpb.ptr, c.n_clicks, c.B, D, 0,
                                             1e-6, 0, out.ptr, D + 4, _st()), [out], written=[_cols_mask((c.B, D + 4), D)])
    ref = [kr.pool_attention_ref(_t(c.node, t), _t(c.a, t), _t(c.b, t), _t(c.watt, t), c.pptr, c.qptr, c.n_clicks, c.B) for t in (torch.float64, torch.float32)]
    _close(f"pool_attention[{D} x100]", out.t[:, :D], ref[0], ref[1])
    ldl = c.Dl + 5
    lpb, lqb, posb = _strided(c.lin_p, ldl), _strided(c.lin_q, ldl), dev_buf(c.pos_emb)
    srb, pib = _ib(c.src_row), _ib(c.pos_id)
    node, coarse = Buf((c.n_exp, D + 4), torch.float32), Buf((c.B, D + 8), torch.float32)
    run_twice(lambda: L().sss_pool_expand_mean(lpb.ptr, lqb.ptr, ldl, srb.ptr, pib.ptr, ppb.ptr, qpb.ptr, c.n_clicks, c.B, c.Dl, 20, posb.ptr,
                                               node.ptr, D + 4, coarse.ptr, D + 8, _st()), [node, coarse],
              written=[_cols_mask((c.n_exp, D + 4), D), _cols_mask((c.B, D + 8), D)])
    ref = [kr.pool_expand_mean_ref(_t(c.lin_p, t), _t(c.lin_q, t), c.src_row, c.pos_id, c.pptr, c.qptr, c.n_clicks, c.B, _t(c.pos_emb, t))
           for t in (torch.float64, torch.float32)]
    _close(f"expand_mean[{D} x100] node", node.t[:, :D], ref[0][0], ref[1][0])
    _close(f"expand_mean[{D} x100] coarse", coarse.t[:, :D], ref[0][1], ref[1][1])


def test_widths_the_host_checks_refuse(cuda):
    """Rows wider than 256 floats are refused (-1, with a message) by the entry points whose kernels own one float4
    column per lane; nothing is launched."""
    c = kr.pool_case(260, 20, "single", seed=11)
    tiny = Buf((4, 264), torch.float32)
    ppb, qpb, srb, pib = _ib(c.pptr), _ib(c.qptr), _ib(c.src_row), _ib(c.pos_id)
    rc = L().sss_pool_expand_mean(tiny.ptr, tiny.ptr, 264, srb.ptr, pib.ptr, ppb.ptr, qpb.ptr, c.n_clicks, c.B, 240, 20, tiny.ptr, tiny.ptr, 264,
                                  tiny.ptr, 264, _st())
    assert rc == -1 and b"pool_expand_mean" in L().sss_last_error()
    rc = L().sss_pool_attention_tab(tiny.ptr, 264, tiny.ptr, 528, tiny.ptr, tiny.ptr, tiny.ptr, tiny.ptr, srb.ptr, pib.ptr, ppb.ptr, qpb.ptr,
                                    c.n_clicks, c.n_p, c.B, 240, 20, 0, 1e-6, tiny.ptr, 264, _st())
    assert rc == -1 and b"pool_attention_tab" in L().sss_last_error()
    la = _lib.LayerArgs(h=260, d_x=4, ld_yp=7 * 260 + 8, ld_yq=268, ld_out_p=264, ld_out_q=264, ld_xin=4, np=1, nq=1)
    assert L().sss_hetero_layer_update(ctypes.byref(la), _st()) == -1 and b"layer_update" in L().sss_last_error()
    for D in (6, 98):                                                  # not a multiple of 4
        rc = L().sss_pool_attention(tiny.ptr, 264, tiny.ptr, 264, tiny.ptr, 264, tiny.ptr, ppb.ptr, qpb.ptr, c.n_clicks, c.B, D, 0, 1e-6, 0,
                                    tiny.ptr, 264, _st())
        assert rc == -1 and b"pool_attention" in L().sss_last_error()


# ================================================================================================ whole encoder
_REF = {}


def _encoder_refs(cfg, kind, loops, seed=21):
    key = (cfg.d_in, cfg.h, cfg.n_layers, cfg.d_out, cfg.max_seq_len, kind, loops)
    if key not in _REF:
        w = init_weights(cfg, seed)
        acts = S.ActionTable(*kr.session_table(kr.edge_sessions(kind, cfg.n_items, cfg.n_query, seed)))
        b = S.build_batch(acts)
        r64, n64 = gnn_ref64.encoder_forward(b, w, cfg.n_layers, self_loops=loops, get_node=True)
        r32, n32 = gnn_ref.encoder_forward(b.to_torch("cpu"), w, cfg.n_layers, self_loops=loops, get_node=True)
        _REF[key] = (w, acts, b, torch.from_numpy(r64), {k: torch.from_numpy(v) for k, v in n64.items()}, r32, n32)
    return _REF[key]


def _check_encoder(cuda, cfg, kind, loops, paths=("actions", "batch")):
    cfg.self_loop_rule = "pyg_bipartite_global" if loops else "none"
    w, acts, b, r64, n64, r32, n32 = _encoder_refs(cfg, kind, loops)
    outs = {}
    for fused in (True, False):
        enc = SessionEncoder(cfg, w, cuda, fused=fused)
        assert enc.fused_ok() == fused                                 # the fused kernels serve every shape validate() admits up to 256
        for path in paths:
            got, nodes = enc(acts if path == "actions" else b.to(cuda), get_node=True)
            tag = f"encoder[{kind} h={cfg.h} D={cfg.d_out} P={cfg.max_seq_len} loops={loops} fused={fused} {path}]"
            assert got.shape == (acts.num_sessions, cfg.d_out)
            for t in ("query", "product"):
                _close(tag + " node_" + t, nodes[t], n64[t], n32[t], NODE_TOL)
            _close(tag, got, r64, r32, TOL)
            outs[(fused, path)] = got.cpu().double()
    e_ref, top = float((r32.double() - r64).abs().max()), float(r64.abs().max())
    for path in paths:
        d = float((outs[(True, path)] - outs[(False, path)]).abs().max())
        print(f"fused vs unfused [{kind} {path}]: {d:.3e}")
        assert d <= 4 * e_ref + float(np.spacing(np.float32(top)))


@pytest.mark.parametrize("loops", [True, False])
@pytest.mark.parametrize("kind", ["cap", "one_item_60", "one_action", "batch_of_one", "cap_among_ones"])
def test_encoder_on_session_shapes_the_generator_does_not_draw(cuda, kind, loops):
    """Sessions at the 64-action cap (65 expanded rows: the chunk loop of the fused pooling), cnt = 60, single actions,
    a batch of one; the positional table has 68 rows so position id 64 exists."""
    cfg = EncoderConfig(d_in=32, h=32, n_layers=2, d_out=96, max_seq_len=68, n_items=50, n_query=9)
    _check_encoder(cuda, cfg, kind, loops)


@pytest.mark.parametrize("d_in,h,d_out", [(32, 96, 160), (64, 256, 256), (32, 160, 192), (64, 192, 224), (96, 224, 96)])
def test_encoder_fused_shapes_no_other_test_uses(cuda, d_in, h, d_out):
    cfg = EncoderConfig(d_in=d_in, h=h, n_layers=1, d_out=d_out, n_items=50, n_query=9)
    _check_encoder(cuda, cfg, "short", True, paths=("batch",))


def test_encoder_with_a_positional_width_that_straddles(cuda):
    """max_seq_len = 18 with d_out = 96: d_lin = 78, so a float4 column of the pooled row straddles lin | pos.  The
    encoder's preparation serves it (t is stored 96 wide with zero padding), fused and unfused."""
    cfg = EncoderConfig(d_in=32, h=32, n_layers=1, d_out=96, max_seq_len=18, n_items=50, n_query=9)
    _check_encoder(cuda, cfg, "short", True)
    _check_encoder(cuda, cfg, "short", False)
