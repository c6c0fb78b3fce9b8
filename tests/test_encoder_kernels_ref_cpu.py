"""oracle/encoder_kernels_ref.py is trustworthy on its own, without a GPU: chained into a whole encoder forward the
per-kernel restatements reproduce oracle/gnn_ref64.py (plain loops from the SURVEY.md formulas, no shared code) to
float64 round-off, the `_tab` restatement equals the expand / attention one, and every case the GPU edge tests feed to
a kernel is well formed (indices in range, rowptr monotone, pptr / qptr consistent with src_row / pos_id)."""
import numpy as np
import pytest
import torch

from oracle import encoder_kernels_ref as kr
from oracle import gnn_ref64
from sessionsimilaritysearch_amd import sessions as S
from sessionsimilaritysearch_amd.encoder import EncoderConfig, init_weights

# float64 against float64 in another summation order: 1e-12 of the largest output (measured: below 2e-15)
REL = 1e-12


def _batch(kind, cfg, seed):
    if kind == "synthetic":
        return S.build_batch(S.synthetic_actions(9, seed, cfg.n_items, cfg.n_query))
    return S.build_batch(S.ActionTable(*kr.session_table(kr.edge_sessions(kind, cfg.n_items, cfg.n_query, seed))))


@pytest.mark.parametrize("kind,P", [("synthetic", 20), ("short", 18), ("one_action", 20), ("cap_among_ones", 68)])
@pytest.mark.parametrize("loops", [True, False])
def test_chained_restatements_reproduce_gnn_ref64(kind, P, loops):
    cfg = EncoderConfig(d_in=32, h=32, n_layers=2, d_out=96, max_seq_len=P, n_items=40, n_query=9)
    w = init_weights(cfg, 11)
    b = _batch(kind, cfg, 3)
    ref, rn = gnn_ref64.encoder_forward(b, w, cfg.n_layers, self_loops=loops, get_node=True)
    for tab in (True, False):
        got, gn = kr.encoder_forward(b, w, cfg.n_layers, self_loops=loops, tab=tab, get_node=True)
        err = np.abs(got.numpy() - ref).max()
        print(f"{kind} loops={loops} tab={tab}: max|diff| = {err:.3e}, max|ref| = {np.abs(ref).max():.3e}")
        assert err <= REL * np.abs(ref).max()
        for t in ("query", "product"):
            assert np.abs(gn[t].numpy() - rn[t]).max() <= REL * np.abs(rn[t]).max()


def test_self_loop_rewrite_matters_on_these_batches():
    """The comparison above can tell the rewrite from its absence (a restatement that dropped it would not pass)."""
    cfg = EncoderConfig(d_in=32, h=32, n_layers=1, d_out=96, n_items=40, n_query=9)
    w = init_weights(cfg, 11)
    b = _batch("synthetic", cfg, 3)
    a, c = kr.encoder_forward(b, w, 1, self_loops=True), kr.encoder_forward(b, w, 1, self_loops=False)
    assert (a - c).abs().max() > 1e-6


@pytest.mark.parametrize("D,P", [(96, 20), (96, 18), (132, 22), (12, 6), (256, 20)])
@pytest.mark.parametrize("kind", ["lengths", "interleaved", "single"])
def test_tab_restatement_equals_expand_attention_restatement(D, P, kind):
    c = kr.check_pool_case(kr.pool_case(D, P, kind, seed=1))
    g = torch.Generator().manual_seed(D + P)
    d = lambda t: t.double()
    wn, bn, wc = (torch.randn((D, D), generator=g, dtype=torch.float64) / D ** 0.5, torch.randn(D, generator=g, dtype=torch.float64),
                  torch.randn((D, D), generator=g, dtype=torch.float64) / D ** 0.5)
    for normalize in (False, True):
        node, coarse = kr.pool_expand_mean_ref(d(c.lin_p), d(c.lin_q), c.src_row, c.pos_id, c.pptr, c.qptr, c.n_clicks, c.B, d(c.pos_emb))
        two = kr.pool_attention_ref(node, node @ wn.T + bn, coarse @ wc.T, d(c.watt), c.pptr, c.qptr, c.n_clicks, c.B, normalize)
        t, ac, tp, a2, c2 = kr.tab_inputs(d(c.lin_p), d(c.lin_q), d(c.pos_emb), wn, bn, wc)
        one = kr.pool_attention_tab_ref(t, ac, tp, a2, c2, d(c.watt), c.src_row, c.pos_id, c.pptr, c.qptr, c.n_clicks, c.n_p, c.B,
                                        c.Dl, normalize)
        assert (one - two).abs().max() <= REL * max(1.0, float(two.abs().max()))
    if kind == "lengths":                                            # its first graph is empty: zeros, and only there
        assert not two[0].any() and not one[0].any() and not two[1:].eq(0).all(1).any()


def test_segment_pool_sum_mean_and_normalise_agree():
    c = kr.pool_case(100, 20, "lengths", seed=2)
    d = lambda t: t.double()
    cnt = torch.from_numpy(np.diff(c.pptr) + np.diff(c.qptr)).double().clamp(min=1)[:, None]
    for watt in (None, d(c.watt)):
        mean = kr.segment_pool_ref(d(c.node), c.pptr, c.qptr, c.n_clicks, c.B, d(c.a), d(c.b), watt)
        total = kr.segment_pool_ref(d(c.node), c.pptr, c.qptr, c.n_clicks, c.B, d(c.a), d(c.b), watt, reduce_sum=True)
        assert (total / cnt - mean).abs().max() < 1e-14
    n = kr.pool_attention_ref(d(c.node), d(c.a), d(c.b), d(c.watt), c.pptr, c.qptr, c.n_clicks, c.B, normalize=True)
    assert ((n * n).sum(1)[1:] - 1).abs().max() < 1e-12 and not n[0].any()


def test_sigmoid_and_gates_do_not_overflow():
    v = torch.tensor([-1e4, -800.0, -100.0, -30.0, 0.0, 30.0, 100.0, 800.0, 1e4], dtype=torch.float64)
    s = kr.sigmoid(v)
    assert torch.isfinite(s).all() and s[0] == 0 and s[-1] == 1 and s[4] == 0.5 and (s + kr.sigmoid(-v) - 1).abs().max() < 1e-15
    assert torch.equal(kr.sigmoid(v.float()).double()[[0, 4, 8]], torch.tensor([0.0, 0.5, 1.0], dtype=torch.float64))


@pytest.mark.parametrize("table_mode", [False, True])
@pytest.mark.parametrize("structure", kr.LAYER_STRUCTURES)
def test_layer_cases_are_well_formed_and_say_what_they_claim(structure, table_mode):
    for h in (4, 64, 100, 256):
        c = kr.check_layer_case(kr.layer_case(structure, h, table_mode))
        out_p, out_q, x0p, x0q = kr.layer_update_ref(c)
        assert out_p.shape == (c.n_p, h) and out_q.shape == (c.n_q, h) and torch.isfinite(out_p).all() and torch.isfinite(out_q).all()
        assert x0p.shape == (c.n_p, c.d_x) and x0q.shape == (c.n_q, c.d_x)
    c = kr.layer_case(structure, 64, table_mode)
    deg = lambda rp: np.diff(rp)
    rq = (lambda j: j) if c.row_q is None else (lambda j: c.row_q[torch.as_tensor(np.asarray(j, np.int64))].numpy())
    if structure == "ascending":
        s = c.yq[torch.as_tensor(rq(c.c_qp[c.rp_qp[0]:c.rp_qp[1]])), 64].numpy()
        assert len(s) == 48 and np.all(np.diff(s) >= 0) and np.sum(np.diff(s) > 0) >= (20 if table_mode else 40)      # table mode: nodes share rows, hence ties
    if structure == "hub":
        assert deg(c.rp_qp)[1] == 300 and deg(c.rp_pq)[1] == 300
    if structure == "no_edges":
        assert len(c.c_qp) == len(c.c_pq) == len(c.c_pp) == 0 and c.n_self_loop > 0
    if structure == "all_self_edges":
        assert all(kr.incoming(c.rp_qp, c.c_qp, i, c.n_self_loop) == ([i] if i < c.n_self_loop else []) for i in range(c.n_p))
        assert all(len(kr.incoming(c.rp_qp, c.c_qp, i, 0)) == (i < c.n_self_loop) for i in range(c.n_p))
    if structure in ("np_gt_nq", "nq_gt_np"):
        assert 0 < c.n_self_loop == min(c.n_p, c.n_q) < max(c.n_p, c.n_q)
    if structure == "partial_self_loop":
        assert 0 < c.n_self_loop < min(c.n_p, c.n_q)
    if structure in ("np_zero", "nq_zero"):
        assert min(c.n_p, c.n_q) == 0 and c.n_self_loop == 0
    if structure == "no_w_pp":
        assert c.w_pp is None and len(c.c_pp) > 0
    if structure.startswith("dx"):
        assert c.d_x == {"dx_odd": 62, "dx_full": 64, "dx_tiny": 3}[structure]
    if structure == "shared_rows" and table_mode:
        assert c.yp.shape[0] == 3 and c.yq.shape[0] == 2
    if structure.startswith("logits"):
        e = [float(c.yq[int(rq([j])[0]), 64] + (c.yp if c.row_p is None else c.yp[c.row_p])[i, 7 * 64 + 1])
             for i in range(c.n_p) for j in c.c_qp[c.rp_qp[i]:c.rp_qp[i + 1]]]
        assert max(abs(v) for v in e) > 60
    if structure.startswith("gru_sat"):
        Yp = (c.yp if c.row_p is None else c.yp[c.row_p]).double()
        pre = Yp[:, 4 * 64:7 * 64].abs()
        assert float(pre.min()) >= 30 and float(pre.max()) == (30 if structure == "gru_sat_30" else 120)


@pytest.mark.parametrize("kind", ["lengths", "interleaved", "single"])
def test_pool_cases_are_well_formed(kind):
    for D in kr.WIDTHS + kr.WIDE:
        kr.check_pool_case(kr.pool_case(D, kr.pool_p_for(D), kind))
    for D, P in ((96, 18), (96, 22), (132, 18), (132, 22)):
        assert kr.check_pool_case(kr.pool_case(D, P, kind)).Dl % 4 == 2
    lens = sorted(a + b for a, b in kr.pool_graphs("lengths"))
    assert set(kr.GRAPH_LENGTHS) <= set(lens) and (70, 0) in kr.pool_graphs("lengths") and (0, 70) in kr.pool_graphs("lengths")
    assert all(len(kr.pool_graphs(k)) % 4 for k in ("lengths", "interleaved", "single"))


def test_every_lane_group_size_is_reached_by_the_width_sweep():
    assert {kr.lanes_for(w) for w in kr.WIDTHS} == {1, 2, 4, 8, 16, 32, 64}
    dead = {kr.lanes_for(w) for w in kr.WIDTHS if kr.lanes_for(w) * 4 > w}
    assert dead == {4, 8, 16, 32, 64}                                # 12, 20, 36, 96 / 100, 132 .. 252


@pytest.mark.parametrize("kind", ["cap", "one_item_60", "one_action", "batch_of_one", "cap_among_ones", "short"])
def test_edge_sessions_are_what_they_claim(kind):
    ss = kr.edge_sessions(kind, 50, 9)
    assert all(1 <= len(s) <= 64 for s in ss)
    b = S.build_batch(S.ActionTable(*kr.session_table(ss)))
    src_row, pos_id, pptr, qptr, n_clicks = kr.pool_indices(b)
    assert pos_id.max() <= max(len(s) for s in ss) and len(src_row) == len(pos_id) == n_clicks + qptr[-1]
    if kind in ("cap", "cap_among_ones"):
        assert max(len(s) for s in ss) == 64 and pos_id.max() == 64
    if kind == "one_item_60":
        assert int(np.asarray(b["product"].cnt).max()) == 60 and (np.diff(pptr) + np.diff(qptr)).max() > 64
