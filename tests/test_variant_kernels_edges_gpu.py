"""The variant row kernels (csrc/variants.hip: k_csr_mean, k_segment_reduce, k_attention_dot_pool), the Python classes
built on them and the MLP / binarize heads, at their edges, against float64 with stated rounding-error bounds.

Bounds (u = 2^-24, gamma_j = j u / (1 - j u), the classic bound for j float32 roundings on one path):
* a sum of m float32 terms accumulated in sequence, each term one rounding (the optional weight product), then for a
  mean a rounded 1/m and a rounded product: |got - exact| <= gamma_(m+2) * sum|terms| (/ m for a mean);
* max is exact: bit-equal to the max of the same float32 values (the weighted ones rounded once, as the kernel does);
* empty segments / targets without edges: exactly 0;
* attention_dot_pool, out = mean_t x_t <x_t, mean>: the mean (cnt + 1 roundings), the dot (d), the weighted sum
  (cnt) and the final 1/cnt (2) add up to gamma_(d + 2 cnt + 4) times the same expression evaluated in float64 on |x|;
* a float32 GEMM step of depth K (fma chain + bias): gamma_(K+1) (|h| |W|^T + |b|), plus |W| times the input's error.
Through a network the errors add up path by path; the ``abs`` evaluations below (float64, every input and weight
replaced by its magnitude) bound every intermediate magnitude, so the sum of the step counts times u times that
evaluation bounds the whole (first order; gamma absorbs the rest).
"""
import numpy as np
import pytest
import torch

from oracle import variants_ref as vr
from oracle.gnn_ref import EDGE_PP, EDGE_PQ, EDGE_QP
from sessionsimilaritysearch_amd import _lib
from sessionsimilaritysearch_amd.encoder import build_csr

pytestmark = pytest.mark.gpu
U = 2.0 ** -24
TOL = 1e-5
TANHF_ULP = 2            # HIP documentation, "HIP math API" reference: tanhf max error 2 ulp (not measured here)
NAN = float("nan")

WIDTHS = [4, 8, 16, 32, 64, 128, 256, 260, 512, 800, 1028, 2044, 2048]     # LPR 1 .. 64, ragged last column chunks
GRAPHS = [1, 63, 65, 257]                                                  # not multiples of the rows per block


def gamma(j):
    j = np.asarray(j, np.float64)
    return j * U / (1 - j * U)


def _st(dev):
    return _lib.stream_ptr(dev)


def _lengths(G, rng):
    """Segment lengths: empty ones first, in the middle and last, single-row ones, one of 5000 rows."""
    if G == 1:
        return np.array([5000])
    L = rng.integers(0, 6, G)
    L[0] = L[G // 2] = L[-1] = 0
    L[1] = L[2] = 1
    L[3] = 5000
    return L


def _strided(x, cuda):
    """Device copy of x [r, d] with row stride d + 4; the padding columns hold NaN."""
    buf = torch.full((x.shape[0], x.shape[1] + 4), NAN, dtype=torch.float32)
    buf[:, :x.shape[1]] = torch.from_numpy(np.ascontiguousarray(x, np.float32))
    return buf.to(cuda)


def _out(rows, d, cuda):
    return torch.full((rows, d + 4), NAN, dtype=torch.float32, device=cuda)


def _read(out, d):
    o = out.cpu().numpy()
    assert np.isnan(o[:, d:]).all(), "guard columns written"
    return o[:, :d].astype(np.float64)


def _seg_reduce(cuda, xd, wd, ptrd, G, d, mode):
    out = _out(G, d, cuda)
    rc = _lib.lib().sss_segment_reduce(xd.data_ptr(), xd.stride(0), 0 if wd is None else wd.data_ptr(), ptrd.data_ptr(), G, d,
                                       mode, out.data_ptr(), out.stride(0), _st(cuda))
    _lib.check(rc, "sss_segment_reduce")
    return _read(out, d)


@pytest.mark.parametrize("d", WIDTHS)
def test_segment_reduce_and_attention_dot_pool_edges(cuda, d):
    rng = np.random.default_rng(4000 + d)
    rows = 5000 + 6 * 257
    x = rng.uniform(-1, 1, (rows, d)).astype(np.float32)
    w = rng.uniform(-0.5, 1.5, rows).astype(np.float32)
    xd, wd = _strided(x, cuda), torch.from_numpy(w).to(cuda)
    x64 = x.astype(np.float64)
    for G in GRAPHS:
        L = _lengths(G, rng)
        ptr = np.zeros(G + 1, np.int32)
        np.cumsum(L, out=ptr[1:])
        ptrd = torch.from_numpy(ptr).to(cuda)
        segs = [(int(ptr[s]), int(ptr[s + 1])) for s in range(G)]
        for use_w in (False, True):
            t64 = x64 * w[:, None] if use_w else x64                      # exact terms (float64 products of float32)
            t32 = (x * w[:, None]).astype(np.float32) if use_w else x     # what the kernel maxes over
            got_mean = _seg_reduce(cuda, xd, wd if use_w else None, ptrd, G, d, 0)
            got_add = _seg_reduce(cuda, xd, wd if use_w else None, ptrd, G, d, 1)
            got_max = _seg_reduce(cuda, xd, wd if use_w else None, ptrd, G, d, 2)
            for s, (a, b) in enumerate(segs):
                m = b - a
                if m == 0:
                    for got in (got_mean, got_add, got_max):
                        assert (got[s] == 0).all(), (G, s)
                    continue
                ssum, sabs = t64[a:b].sum(0), np.abs(t64[a:b]).sum(0)
                assert (np.abs(got_add[s] - ssum) <= gamma(m + 2) * sabs).all(), (G, s, use_w)
                assert (np.abs(got_mean[s] - ssum / m) <= gamma(m + 2) * sabs / m).all(), (G, s, use_w)
                assert np.array_equal(got_max[s], t32[a:b].max(0).astype(np.float64)), (G, s, use_w)
        out = _out(G, d, cuda)
        rc = _lib.lib().sss_attention_dot_pool(xd.data_ptr(), xd.stride(0), ptrd.data_ptr(), G, d, out.data_ptr(),
                                               out.stride(0), _st(cuda))
        _lib.check(rc, "sss_attention_dot_pool")
        got = _read(out, d)
        for s, (a, b) in enumerate(segs):
            cnt = b - a
            if cnt == 0:
                assert (got[s] == 0).all(), (G, s)
                continue
            seg, sa = x64[a:b], np.abs(x64[a:b])
            ref = (seg * (seg @ seg.mean(0))[:, None]).mean(0)
            mag = (sa * (sa @ sa.mean(0))[:, None]).mean(0)
            assert (np.abs(got[s] - ref) <= gamma(d + 2 * cnt + 4) * mag).all(), (G, s)


@pytest.mark.parametrize("d", WIDTHS)
def test_csr_mean_edges(cuda, d):
    """Isolated targets (first, middle, last), duplicate edges, self edges (source index == target index) and a hub
    target with 5000 in-edges."""
    rng = np.random.default_rng(4100 + d)
    n_src, n_dst = 700, 257
    src = rng.integers(0, n_src, 1500)
    dst = rng.integers(1, n_dst - 1, 1500)
    src = np.r_[src, rng.integers(0, n_src, 5000), [9, 9, 9, 40, 40], np.arange(20, 30)]
    dst = np.r_[dst, np.full(5000, 7), [11, 11, 11, 12, 12], np.arange(20, 30)]       # hub, duplicates, self edges
    keep = (dst != 128)
    src, dst = src[keep], dst[keep]
    order = np.argsort(dst, kind="stable")
    rowptr = np.zeros(n_dst + 1, np.int32)
    np.cumsum(np.bincount(dst, minlength=n_dst), out=rowptr[1:])
    col = src[order].astype(np.int32)
    assert rowptr[1] == 0 and rowptr[129] == rowptr[128] and rowptr[-1] == rowptr[-2]
    x = rng.uniform(-1, 1, (n_src, d)).astype(np.float32)
    xd, rpd, cd = _strided(x, cuda), torch.from_numpy(rowptr).to(cuda), torch.from_numpy(col).to(cuda)   # alive until read
    out = _out(n_dst, d, cuda)
    rc = _lib.lib().sss_csr_mean(xd.data_ptr(), xd.stride(0), rpd.data_ptr(), cd.data_ptr(), n_dst, d, out.data_ptr(),
                                 out.stride(0), _st(cuda))
    _lib.check(rc, "sss_csr_mean")
    got = _read(out, d)
    x64 = x.astype(np.float64)
    for i in range(n_dst):
        js = col[rowptr[i]:rowptr[i + 1]]
        m = len(js)
        if m == 0:
            assert (got[i] == 0).all(), i
            continue
        ref, mag = x64[js].mean(0), np.abs(x64[js]).mean(0)
        assert (np.abs(got[i] - ref) <= gamma(m + 2) * mag).all(), (i, m)


def test_max_of_only_minus_inf_is_outside_the_contract(cuda):
    """Pooling inputs are finite by contract (they are relu / linear outputs).  Out of contract, a segment that holds
    only -inf: k_segment_reduce returns the IEEE max, -inf, where the oracle (``graph_pooling``'s torch.where on
    isinf) returns 0.  Pinned so that a change of this behaviour is deliberate."""
    x = np.array([[1.0, -np.inf], [-np.inf, -np.inf], [-np.inf, -np.inf], [2.0, 3.0]], np.float32)
    x = np.repeat(x, 2, axis=1)                                      # d = 4
    ptr = torch.tensor([0, 1, 3, 4], dtype=torch.int32, device=cuda)
    got = _seg_reduce(cuda, _strided(x, cuda), None, ptr, 3, 4, 2)
    assert got[0].tolist() == [1.0, 1.0, -np.inf, -np.inf]
    assert np.isneginf(got[1]).all()                                 # the oracle would give 0 here
    assert got[2].tolist() == [2.0, 2.0, 3.0, 3.0]


# --------------------------------------------------------------------------------------- classes on hand-built graphs
def _rand(g, *shape, scale=1.0):
    return (torch.rand(shape, generator=g, dtype=torch.float64) * 2 - 1).float() * scale


def _abs(w):
    return {k: v.double().abs() for k, v in w.items()}


def _hand_graph(B):
    """B sessions' worth of query / product nodes; some queries get no pq edges, some products no qp / pp edges, one
    graph (the second, when B > 1) has no product node at all."""
    rng = np.random.default_rng(4200 + B)
    per = [0 if (B > 1 and s == 1) else int(rng.integers(1, 9)) for s in range(B)]
    Np = sum(per)
    Nq = B + 3
    batch = np.repeat(np.arange(B), per)
    ptr = np.zeros(B + 1, np.int32)
    np.cumsum(per, out=ptr[1:])
    qs = rng.integers(0, Nq - 2, 3 * Np)                               # queries Nq-2, Nq-1: no pq edges
    ps = rng.integers(0, Np, 3 * Np)
    keep_qp = ps % 4 != 1                                             # products p % 4 == 1: no qp edges
    eid = {EDGE_QP: torch.tensor(np.stack([qs[keep_qp], ps[keep_qp]]), dtype=torch.long),
           EDGE_PQ: torch.tensor(np.stack([ps, qs]), dtype=torch.long)}
    pa, pb = rng.integers(0, Np, 2 * Np), rng.integers(0, Np, 2 * Np)
    keep_pp = pb % 3 != 0                                             # products p % 3 == 0: no pp edges
    eid[EDGE_PP] = torch.tensor(np.stack([pa[keep_pp], pb[keep_pp]]), dtype=torch.long)
    return Nq, Np, torch.from_numpy(batch), ptr, eid


def _max_indeg(ei, n):
    return int(np.bincount(ei[1].numpy(), minlength=n).max()) if ei.shape[1] else 0


@pytest.mark.parametrize("B", [1, 6])
def test_variant_classes_on_hand_built_graphs(cuda, B):
    from sessionsimilaritysearch_amd.variants import AttentionPooling, GraphPooling, HeteroSAGE, SRGNNPooling
    Nq, Np, batch, ptr, eid = _hand_graph(B)
    g = torch.Generator().manual_seed(4300 + B)
    d, h, out = 64, 96, 40
    w = {}
    for l in range(3):
        din = d if l == 0 else h
        for e in ("qp", "pq", "pp"):
            w[f"sage.{l}.{e}.lin_l.w"] = _rand(g, h, din, scale=0.3)
            w[f"sage.{l}.{e}.lin_l.b"] = _rand(g, h, scale=0.2)
            w[f"sage.{l}.{e}.lin_r.w"] = _rand(g, h, din, scale=0.3)
    xq, xp = _rand(g, Nq, d), _rand(g, Np, d)
    csr = {k: build_csr(eid[k].to(cuda), n)[:2] for k, n in ((EDGE_QP, Np), (EDGE_PQ, Nq), (EDGE_PP, Np))}
    got = HeteroSAGE(w, 3, cuda).forward(xq.to(cuda), xp.to(cuda), csr[EDGE_QP], csr[EDGE_PQ], csr[EDGE_PP])
    ref32 = vr.hetero_sage(xq, xp, eid, w)
    ref = vr.hetero_sage(xq.double(), xp.double(), eid, {k: v.double() for k, v in w.items()})
    mag = vr.hetero_sage(xq.double().abs(), xp.double().abs(), eid, _abs(w))
    deg = max(_max_indeg(eid[k], n) for k, n in ((EDGE_QP, Np), (EDGE_PQ, Nq), (EDGE_PP, Np)))
    steps = 3 * (deg + 3 * h + 4)                       # per layer: mean (deg + 2), GEMM over [agg ; agg ; x] (K + 1)
    for t in ("query", "product"):
        gt = got[t].cpu()
        assert (gt - ref32[t]).abs().max() < TOL * max(1.0, float(ref32[t].abs().max())), t
        assert ((gt.double() - ref[t]).abs() <= gamma(steps) * mag[t]).all(), t

    # pooling over the products of these graphs (an empty graph when B > 1), rows = the SAGE output
    x = got["product"].cpu()
    x64, xa = x.double(), x.double().abs()
    ptrd = torch.from_numpy(ptr).to(cuda)
    seg = int(np.diff(ptr).max())
    lin = {"lin.w": _rand(g, out, h, scale=0.2), "lin.b": _rand(g, out, scale=0.2)}
    lin64 = {k: v.double() for k, v in lin.items()}
    for key in ("mean", "add", "max"):
        o = GraphPooling(key, lin, cuda).forward(x.to(cuda), ptrd).cpu()
        r32 = vr.graph_pooling(x, batch, B, key, lin)
        assert (o - r32).abs().max() < TOL * max(1.0, float(r32.abs().max())), key
        r = vr.graph_pooling(x64, batch, B, key, lin64)
        m = vr.graph_pooling(xa, batch, B, key, _abs(lin))
        assert ((o.double() - r).abs() <= gamma(seg + h + 4) * m).all(), key
    o = AttentionPooling(lin, cuda).forward(x.to(cuda), ptrd).cpu()
    r32 = vr.attention_pooling(x, batch, B, lin)
    assert (o - r32).abs().max() < 2 * TOL * max(1.0, float(r32.abs().max()))
    r, m = vr.attention_pooling(x64, batch, B, lin64), vr.attention_pooling(xa, batch, B, _abs(lin))
    assert ((o.double() - r).abs() <= gamma(h + 2 * seg + 4 + h + 1) * m).all()
    ws = {"lin1.w": _rand(g, h, h, scale=0.2), "lin1.b": _rand(g, h, scale=0.2), "lin2.w": _rand(g, h, h, scale=0.2),
          "lin2.b": _rand(g, h, scale=0.2), "lin3.w": _rand(g, 1, h, scale=0.3), "lin4.w": _rand(g, out, 2 * h, scale=0.2),
          "lin4.b": _rand(g, out, scale=0.2)}
    mask = torch.zeros(Np)
    mask[torch.from_numpy(ptr[1:][np.diff(ptr) > 0].astype(np.int64) - 1)] = 1.0
    o = SRGNNPooling(ws, cuda).forward(x.to(cuda), ptrd, mask).cpu()
    r32 = vr.srgnn_pooling(x, batch, B, mask, ws)
    assert (o - r32).abs().max() < TOL * max(1.0, float(r32.abs().max()))
    r = vr.srgnn_pooling(x64, batch, B, mask.double(), {k: v.double() for k, v in ws.items()})
    m = vr.srgnn_pooling(xa, batch, B, mask.double(), _abs(ws))
    # local sum (seg), lin1 / lin2 (h + 1), expf-based sigmoid (a few ulp: 8), lin3 (h), attention sum (seg + 1),
    # lin4 (2h + 1); the |.| evaluation's sigmoid is >= 1/2 where the true one is <= 1: x2
    assert ((o.double() - r).abs() <= 2 * gamma(2 * seg + 4 * h + 12) * m).all()


# ----------------------------------------------------------------------------------------------------------- heads
def _pad32(n):
    return (n + 31) // 32 * 32


def _mlp_weights(g, n_in, n_hid, n_out, nh, jump):
    w = {}
    dims = [n_in] + [n_hid] * (nh + 1)
    for i in range(nh + 1):
        w[f"layers.{i}.w"] = _rand(g, dims[i + 1], dims[i], scale=1.0 / np.sqrt(dims[i]))
        w[f"layers.{i}.b"] = _rand(g, dims[i + 1], scale=0.2)
        w[f"bn.{i}.mean"] = _rand(g, n_hid, scale=0.2)
        w[f"bn.{i}.var"] = torch.rand(n_hid, generator=g) + 0.5
        w[f"bn.{i}.gamma"] = torch.rand(n_hid, generator=g) + 0.5
        w[f"bn.{i}.beta"] = _rand(g, n_hid, scale=0.2)
    k = n_hid + (n_in if jump else 0)
    w[f"layers.{nh + 1}.w"] = _rand(g, n_out, k, scale=1.0 / np.sqrt(k))
    w[f"layers.{nh + 1}.b"] = _rand(g, n_out, scale=0.2)
    return w


def _gemm_err(h, e, W, b, K):
    """Error of a float32 GEMM step on an input h (float64 truth) known to within e: |W| e + gamma_(K+1) (|h|+e)|W|^T + |b|."""
    Wa = W.abs()
    return e @ Wa.T + gamma(K + 1) * ((h.abs() + e) @ Wa.T + b.abs())


def _mlp_with_bound(x, w, nh, jump, last_act):
    """vr.mlp in float64 and an elementwise bound on the float32 head's distance from it, step by step: the GEMM,
    relu (1-Lipschitz), the BatchNorm stage relu(v s + t) (s and t rounded to float32 once each, then a product and a
    sum: 4 roundings), the final GEMM and tanh (TANHF_ULP ulp, and ulp <= 2^-23 on [-1, 1])."""
    w = {k: v.double() for k, v in w.items()}
    h, e = x.double(), torch.zeros_like(x, dtype=torch.float64)
    inp = h
    for i in range(nh + 1):
        W, b = w[f"layers.{i}.w"], w[f"layers.{i}.b"]
        v = torch.relu(h @ W.T + b)
        ev = _gemm_err(h, e, W, b, _pad32(W.shape[1]))
        s = w[f"bn.{i}.gamma"] / torch.sqrt(w[f"bn.{i}.var"] + 1e-5)
        t = w[f"bn.{i}.beta"] - w[f"bn.{i}.mean"] * s
        h = torch.relu(v * s + t)
        e = s.abs() * ev + gamma(4) * (s.abs() * (v.abs() + ev) + t.abs())
    if jump:
        h, e = torch.cat([inp, h], 1), torch.cat([torch.zeros_like(inp), e], 1)
    W, b = w[f"layers.{nh + 1}.w"], w[f"layers.{nh + 1}.b"]
    K = (_pad32(inp.shape[1]) + _pad32(W.shape[1] - inp.shape[1])) if jump else _pad32(W.shape[1])
    y, ey = h @ W.T + b, _gemm_err(h, e, W, b, K)
    if last_act:
        y, ey = torch.tanh(y), ey + TANHF_ULP * 2.0 ** -23
    return y, ey


MLP_CASES = [  # n_in, n_hid, n_out, nh, jump, n
    (1, 31, 1, 0, False, 1), (33, 65, 250, 1, True, 63), (250, 31, 250, 2, False, 64), (33, 31, 1, 2, True, 65),
    (250, 65, 1, 0, True, 64), (1, 65, 250, 1, False, 65), (250, 65, 250, 0, False, 63),
]


@pytest.mark.parametrize("case", MLP_CASES)
@pytest.mark.parametrize("last_act", [True, False])
def test_mlp_head_ragged_widths(cuda, case, last_act):
    from sessionsimilaritysearch_amd.variants import MLPHead
    n_in, n_hid, n_out, nh, jump, n = case
    g = torch.Generator().manual_seed(4400 + sum(case[:4]) * 7 + n + jump)
    w = _mlp_weights(g, n_in, n_hid, n_out, nh, jump)
    x = _rand(g, n, n_in, scale=2.0)
    got = MLPHead(w, nh, cuda, last_act, jump).forward(x.to(cuda)).cpu()
    assert got.shape == (n, n_out)
    ref32 = vr.mlp(x, w, nh, last_act, jump)
    assert (got - ref32).abs().max() < TOL * max(1.0, float(ref32.abs().max()))
    ref, bound = _mlp_with_bound(x, w, nh, jump, last_act)
    assert ((got.double() - ref).abs() <= bound).all()


BIN_CASES = [  # n_in, n_hid, m_out, code, nh, jump (None: no mlp), n
    (1, None, None, 1, 0, None, 63), (33, None, None, 250, 0, None, 64), (250, 65, 31, 250, 1, False, 65),
    (33, 31, 65, 1, 2, True, 64), (250, 31, 1, 250, 0, True, 1), (1, 65, 250, 33, 1, False, 63),
]


@pytest.mark.parametrize("case", BIN_CASES)
def test_binarize_head_ragged_widths_and_zero_code(cuda, case):
    from sessionsimilaritysearch_amd.index import pack_sign_bits
    from sessionsimilaritysearch_amd.variants import BinarizeHead, MLPHead
    n_in, n_hid, m_out, code, nh, jump, n = case
    g = torch.Generator().manual_seed(4500 + n_in + code * 3 + n)
    mw = None if n_hid is None else _mlp_weights(g, n_in, n_hid, m_out, nh, False)
    k1 = n_in if mw is None else m_out + (n_in if jump else 0)
    w = {"lin1.w": _rand(g, code, k1, scale=1.0 / np.sqrt(k1)), "lin1.b": _rand(g, code, scale=0.05)}
    w["lin1.w"][0] = 0.0                                   # column 0: an exactly zero pre-activation
    w["lin1.b"][0] = 0.0
    x = _rand(g, n, n_in, scale=2.0)
    head = BinarizeHead(w, None if mw is None else MLPHead(mw, nh, cuda, True, False), cuda, jump=bool(jump))
    pre = head(x.to(cuda), pre_sign=True).cpu()
    ref32 = vr.binarize_head(x, w, mw, nh, True, bool(jump), pre_sign=True)
    assert (pre - ref32).abs().max() < TOL * max(1.0, float(ref32.abs().max()))
    # float64 truth and bound: h = x, or tanh(tanh(mlp(x))) (+ x) -- the head's own tanh on the mlp's tanh output
    if mw is None:
        h, e = x.double(), torch.zeros((n, n_in), dtype=torch.float64)
        K = _pad32(n_in)
    else:
        y, ey = _mlp_with_bound(x, mw, nh, False, True)
        h, e = torch.tanh(y), ey + TANHF_ULP * 2.0 ** -23
        K = _pad32(m_out)
        if jump:
            h, e = torch.cat([h, x.double()], 1), torch.cat([e, torch.zeros((n, n_in), dtype=torch.float64)], 1)
            K += _pad32(n_in)
    W, b = w["lin1.w"].double(), w["lin1.b"].double()
    ref, bound = h @ W.T + b, _gemm_err(h, e, W, b, K)
    assert ((pre.double() - ref).abs() <= bound).all()
    codes = head(x.to(cuda)).cpu()
    safe = ref.abs() > bound
    assert torch.equal(codes[safe], torch.sign(ref[safe]).float())
    assert (pre[:, 0] == 0).all() and (codes[:, 0] == 0).all()                # sign(0) = 0 ...
    packed = pack_sign_bits(codes.to(cuda)).cpu().numpy()
    assert np.array_equal(packed, np.packbits(((codes.numpy() + 1) / 2).astype(int), axis=1))
    assert (packed[:, 0] & 0x80 == 0).all()                                   # ... and bit 0: int((0 + 1) / 2) = 0
