"""GPU side of the HGT encoder: sss_hgt_aggregate called directly against the float64 loop restatement at the shapes where
its lane map can go wrong, its exact cases, hand-made rows, sss_hgt_skip, and variants.HGT end to end (followed by the
two-tower pooling) against the float64 torch restatement.  Tolerance: the project's 1e-5 on O(1) values."""
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import hgt_ref as hr  # noqa: E402

from sessionsimilaritysearch_amd import _lib  # noqa: E402
from sessionsimilaritysearch_amd import sessions as S  # noqa: E402
from sessionsimilaritysearch_amd.sessions import EDGE_PP, EDGE_PQ, EDGE_QP  # noqa: E402

pytestmark = pytest.mark.gpu
TOL = 1e-5                                  # times max(1, max |ref|), as tests/test_variants_gpu.py
_CACHE = {}


def graph():
    """The 80-session batch every test shares, built once: (Nq, Np, edges, {edge type: (rowptr, col)} by target, per-graph
    node pointers {type: int32 [B + 1]}, node -> graph {type: int64})."""
    if "g" not in _CACHE:
        b = S.build_batch(S.synthetic_actions(80, 70, 500, 65)).to_numpy()
        ei = b.edge_index_dict
        edges = {"qp": ei[EDGE_QP], "pq": ei[EDGE_PQ], "pp": ei[EDGE_PP]}
        n = {t: len(b[t].x) for t in hr.TYPES}
        batch = {t: np.asarray(b[t].batch, dtype=np.int64) for t in hr.TYPES}
        ptr = {t: np.searchsorted(batch[t], np.arange(int(b.num_graphs) + 1)).astype(np.int32) for t in hr.TYPES}
        _CACHE["g"] = (n["query"], n["product"], edges, {e: hr.csr_by_target(edges[e], n[t]) for e, _, t in hr.EDGES}, ptr, batch)
    return _CACHE["g"]


def _close(got, ref, what=""):
    ref = np.asarray(ref)
    err = float(np.abs(got.double().cpu().numpy() - ref).max()) if ref.size else 0.0
    bound = TOL * max(1.0, float(np.abs(ref).max()) if ref.size else 0.0)
    print(f"{what}: max|err| = {err:.3e}, bound {bound:.3e}")
    assert err < bound, (what, err, bound)


class Rows:
    """float32 rows [n, width] inside a wider device buffer (leading dimension > width, a 16-byte aligned column offset);
    ``pair`` puts k | v side by side in one buffer, as the encoder's node transforms are."""

    def __init__(self, g, n, width, dev, scale, pair=False, off=8, pad=12, fill=None):
        self.host = [torch.randn((n, width), generator=g) * scale for _ in range(2 if pair else 1)]
        self.buf = torch.full((n, off + len(self.host) * width + pad), float("nan") if fill is None else fill, dtype=torch.float32)
        for i, t in enumerate(self.host):
            self.buf[:, off + i * width:off + (i + 1) * width] = t
        self.buf = self.buf.to(dev)
        self.views = [self.buf[:, off + i * width:off + (i + 1) * width] for i in range(len(self.host))]


def _run(q, slots, heads, n_dst, gelu, out):
    """slots: [(k view, v view, rowptr dev, col dev)]; q / out 2-D device views; only the first n_dst targets."""
    from sessionsimilaritysearch_amd.variants import hgt_aggregate
    return hgt_aggregate(q[:n_dst], slots, heads, out[:n_dst], gelu)


@pytest.mark.parametrize("heads,head_dim", [(8, 4), (4, 16), (2, 48), (4, 200), (1, 264), (8, 256)])
def test_aggregate_matches_the_loop_restatement(cuda, heads, head_dim):
    """(8, 4): one float4 per head; (2, 48): idle lanes in every head; (4, 200): the reference, a ragged last step; (1, 264):
    a ragged second step; (8, 256): eight float4 columns per lane, width 2048.  One and two slots, leading dimensions wider
    than the rows, k | v adjacent, n_dst in {1, 5, all}; nothing is written outside [n_dst, width]."""
    nq, np_, _, csr = graph()[:4]
    g = torch.Generator().manual_seed(100 * heads + head_dim)
    W = heads * head_dim
    sc = head_dim ** -0.25                                             # logits ~ N(0, 1)
    q = Rows(g, np_, W, cuda, sc)
    src_q, src_p = Rows(g, nq, W, cuda, sc, pair=True), Rows(g, np_, W, cuda, sc, pair=True, off=4, pad=4)
    dcsr = {e: tuple(torch.from_numpy(a).to(cuda) for a in csr[e]) for e in ("qp", "pp")}
    dev_slots = [(src_q.views[0], src_q.views[1]) + dcsr["qp"], (src_p.views[0], src_p.views[1]) + dcsr["pp"]]
    host_slots = [(src_q.host[0].numpy(), src_q.host[1].numpy()) + csr["qp"], (src_p.host[0].numpy(), src_p.host[1].numpy()) + csr["pp"]]
    for n_slots in (1, 2):
        ref = hr.attention_loops(q.host[0].numpy(), host_slots[:n_slots], heads, gelu=True)
        for n_dst in (1, 5, np_):
            out = torch.full((np_ + 3, W + 8), -7.0, dtype=torch.float32, device=cuda)
            _run(q.views[0], dev_slots[:n_slots], heads, n_dst, True, out[:, 4:4 + W])
            _close(out[:n_dst, 4:4 + W], ref[:n_dst], f"H={heads} D={head_dim} slots={n_slots} n_dst={n_dst}")
            assert bool((out[n_dst:] == -7.0).all()) and bool((out[:, :4] == -7.0).all()) and bool((out[:, 4 + W:] == -7.0).all())


@pytest.mark.parametrize("heads,head_dim", [(8, 4), (4, 200), (8, 256)])
def test_exact_cases(cuda, heads, head_dim):
    """Zero in-degree gives exact zeros (gelu on and off), in-degree 1 without gelu gives the source's v row bit for bit
    (from either slot, the other one empty for that target), and two runs of the whole batch are bit-identical."""
    g = torch.Generator().manual_seed(7)
    W, n_dst, n_src = heads * head_dim, 70, 9                          # 70 targets: more than one workgroup at 64 lanes
    sc = head_dim ** -0.25                                             # logits ~ N(0, 1)
    q, a, b = Rows(g, n_dst, W, cuda, sc), Rows(g, n_src, W, cuda, sc, pair=True), Rows(g, n_src, W, cuda, sc, pair=True)
    deg_a = np.array([(0, 1, 0, 3)[i % 4] for i in range(n_dst)])      # i % 4: 0 nothing, 1 one edge in a, 2 one edge in b, 3 both
    deg_b = np.array([(0, 0, 1, 2)[i % 4] for i in range(n_dst)])
    rng = np.random.default_rng(3)
    csr = []
    for deg in (deg_a, deg_b):
        rowptr = np.concatenate([[0], np.cumsum(deg)]).astype(np.int32)
        csr.append((rowptr, rng.integers(0, n_src, int(rowptr[-1])).astype(np.int32)))
    dev = [tuple(torch.from_numpy(x).to(cuda) for x in c) for c in csr]
    slots = [(a.views[0], a.views[1]) + dev[0], (b.views[0], b.views[1]) + dev[1]]
    outs = {}
    for gelu in (False, True):
        out = torch.full((n_dst, W), float("nan"), dtype=torch.float32, device=cuda)
        _run(q.views[0], slots, heads, n_dst, gelu, out)
        outs[gelu] = out.cpu()
        again = torch.full((n_dst, W), float("nan"), dtype=torch.float32, device=cuda)
        _run(q.views[0], slots, heads, n_dst, gelu, again)
        assert torch.equal(out, again)
        assert bool((outs[gelu][0::4] == 0.0).all())
    for i in range(n_dst):
        if i % 4 == 1:
            assert torch.equal(outs[False][i], a.host[1][int(csr[0][1][csr[0][0][i]])]), i
        if i % 4 == 2:
            assert torch.equal(outs[False][i], b.host[1][int(csr[1][1][csr[1][0][i]])]), i
    host = [(a.host[0].numpy(), a.host[1].numpy()) + csr[0], (b.host[0].numpy(), b.host[1].numpy()) + csr[1]]
    _close(outs[True], hr.attention_loops(q.host[0].numpy(), host, heads, True), "exact-case graph, gelu")


def test_hand_made_rows(cuda):
    """In-degree 300 with duplicate sources, logits of exactly +-90 (the max subtraction must hold; everything stays finite)
    and all-equal logits (the plain mean of the v rows)."""
    heads, D, n_src = 4, 16, 40
    W = heads * D
    g = torch.Generator().manual_seed(9)
    rng = np.random.default_rng(9)
    q, src = Rows(g, 4, W, cuda, 0.5), Rows(g, n_src, W, cuda, 0.5, pair=True)
    qh, kh = q.host[0], src.host[0]
    qh[0, ::D] = 0.0                                                   # target 0: O(1) logits, the +-90 column unread
    qh[1:3] = 0.0
    qh[1:3, ::D] = 1.0                                                 # targets 1, 2: the dot is k's first column, exactly
    kh[:, ::D] = torch.from_numpy(rng.choice([-90.0, 90.0], size=(n_src, heads)).astype(np.float32))
    kh[0, ::D], kh[1, ::D] = 90.0, -90.0
    qh[3] = 0.0                                                        # target 3: all logits equal (zero)
    q.views[0].copy_(qh)
    src.views[0].copy_(kh)
    cols = [rng.integers(0, n_src, 300), np.array([0, 1, 1, 0, 5, 5, 5]), np.array([1, 1, 1]), rng.integers(0, n_src, 33)]
    rowptr = np.concatenate([[0], np.cumsum([len(c) for c in cols])]).astype(np.int32)
    col = np.concatenate(cols).astype(np.int32)
    slot = (src.views[0], src.views[1], torch.from_numpy(rowptr).to(cuda), torch.from_numpy(col).to(cuda))
    out = torch.full((4, W), float("nan"), dtype=torch.float32, device=cuda)
    _run(q.views[0], [slot], heads, 4, False, out)
    assert bool(torch.isfinite(out).all())
    ref = hr.attention_loops(qh.numpy(), [(kh.numpy(), src.host[1].numpy(), rowptr, col)], heads, False)
    _close(out, ref, "hand-made rows")
    mean = src.host[1].double()[torch.from_numpy(cols[3])].mean(0).numpy()
    assert np.abs(ref[3] - mean).max() < 1e-12 and np.abs(ref[2] - src.host[1][1].double().numpy()).max() < 1e-12


def test_skip_adds_beta_x_in_place(cuda):
    g = torch.Generator().manual_seed(12)
    for n, h in ((1, 4), (77, 96), (300, 800)):
        buf = torch.randn((n, 2 * h + 8), generator=g)
        d = buf.to(cuda)
        rc = _lib.lib().sss_hgt_skip(d[:, h + 4:].data_ptr(), d.stride(0), d.data_ptr(), d.stride(0), 0.375, n, h, _lib.stream_ptr(cuda))
        assert rc == 0
        want = buf.clone()
        want[:, h + 4:2 * h + 4] += 0.375 * buf[:, :h]                 # one rounding of the product, one of the sum (or one fma)
        assert (d.cpu() - want).abs().max() <= 2.0 ** -23 * want.abs().max() and torch.equal(d.cpu()[:, :h + 4], buf[:, :h + 4])
        assert torch.equal(d.cpu()[:, 2 * h + 4:], buf[:, 2 * h + 4:])


# The float32 run of the unfolded torch restatement against its float64 run on the inputs of the two cases below, measured
# on the CPU: max |err| / max(1, max |ref|) = 4.6e-7 (64 -> 96) and 6.7e-7 (768 -> 800) over the node features.  The device
# differs from that run only in summation order and in the folded weights' one extra rounding; four times the worst of
# these, 2.7e-6, is inside TOL = 1e-5, so the project's TOL stands as the bound.
@pytest.mark.parametrize("d,h,heads", [(64, 96, 2), (768, 800, 4)])
def test_hgt_end_to_end_and_two_tower_pooling(cuda, d, h, heads):
    """variants.HGT against the float64 restatement, then GraphPooling('mean') of both node types and their concatenation
    (GraphLevelEncoder.forward, model/model.py:244-254)."""
    from sessionsimilaritysearch_amd.variants import HGT, GraphPooling
    nq, np_, edges, csr, ptr, batch = graph()
    L, B = 3, 80
    g = torch.Generator().manual_seed(d)
    w = hr.make_weights(g, d, d, h, heads, L)
    xq, xp = torch.randn((nq, d), generator=g), torch.randn((np_, d), generator=g)
    ref = hr.hgt_torch(xq, xp, edges, w, heads, L)
    dcsr = {e: tuple(torch.from_numpy(a).to(cuda) for a in csr[e]) for e in csr}
    got = HGT(w, heads, L, cuda).forward(xq.to(cuda), xp.to(cuda), dcsr["qp"], dcsr["pq"], dcsr["pp"])
    for t in hr.TYPES:
        assert got[t].shape == ref[t].shape == ((nq if t == "query" else np_), h * (L + 1))
        _close(got[t], ref[t].numpy(), f"HGT {d}->{h} {t}")
    pooled, pooled_ref = [], []
    for t in hr.TYPES:
        assert ptr[t].shape == (B + 1,) and (np.diff(ptr[t]) > 0).all()
        lin = {"lin.w": (torch.rand((h // 2, h * (L + 1)), generator=g) * 2 - 1) / math.sqrt(h * (L + 1)),
               "lin.b": (torch.rand(h // 2, generator=g) * 2 - 1) * 0.1}
        pooled.append(GraphPooling("mean", lin, cuda).forward(got[t], torch.from_numpy(ptr[t]).to(cuda)))
        mean = torch.zeros((B, h * (L + 1)), dtype=torch.float64).index_add_(0, torch.from_numpy(batch[t]), ref[t])
        mean = mean / torch.from_numpy(np.diff(ptr[t]))[:, None]
        pooled_ref.append(mean @ lin["lin.w"].double().T + lin["lin.b"].double())
    emb, emb_ref = torch.cat(pooled, 1), torch.cat(pooled_ref, 1)
    assert emb.shape == (B, h)
    _close(emb, emb_ref.numpy(), f"two-tower embedding {d}->{h}")


def test_input_widths_that_differ_and_need_padding(cuda):
    """lin_t maps d_t -> h per node type: 40-wide query features (padded to the GEMM's K = 64 with zero columns) beside
    96-wide product features take two input launches; one layer at H = 8, D = 4."""
    from sessionsimilaritysearch_amd.variants import HGT
    nq, np_, edges, csr = graph()[:4]
    g = torch.Generator().manual_seed(40)
    w = hr.make_weights(g, 40, 96, 32, 8, 1)
    xq, xp = torch.randn((nq, 40), generator=g), torch.randn((np_, 96), generator=g)
    ref = hr.hgt_torch(xq, xp, edges, w, 8, 1)
    dcsr = {e: tuple(torch.from_numpy(a).to(cuda) for a in csr[e]) for e in csr}
    got = HGT(w, 8, 1, cuda).forward(xq.to(cuda), xp.to(cuda), dcsr["qp"], dcsr["pq"], dcsr["pp"])
    for t in hr.TYPES:
        _close(got[t], ref[t].numpy(), f"HGT 40 / 96 -> 32 {t}")
