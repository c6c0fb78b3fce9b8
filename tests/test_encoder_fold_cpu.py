"""session_fold_weights on the CPU, with no device and no library: the blocks that are copies of a source weight are
held exactly, every pad exactly zero, and the folded blocks (the alpha rows lin^T att, the u block W_ggc W_ih^T, the pooling
tables) are applied to seeded float64 rows and held to the columns oracle/encoder_kernels_ref forms from the RAW weights.

The bound of the folded parts is derived: elementwise
    |got - ref| <= 2^-24 (|x| @ |W_ref|^T + |b_ref|) + K 2^-52 (|x| @ |W_ref|^T).
First term: each stored weight is one float32 rounding of its float64 value (relative 2^-24), the copied blocks and the biases
carry none.  Second term: the float64 sums -- a dot product of n terms is off by at most n 2^-53 of the sum of its terms'
magnitudes, to first order; a folded column goes through one sum inside the fold (h terms, or D - P for the tables) and one
over the row's `din` columns, in the fold and again, in another order, in the oracle: K = 2 (inner + din)."""
import functools

import pytest
import torch

from oracle import encoder_kernels_ref as kr
from sessionsimilaritysearch_amd import _lib
from sessionsimilaritysearch_amd.encoder import ALPHA_PAD, EncoderConfig, init_weights, session_fold_weights

CONFIGS = [(32, 0, 32, 1, 64),          # smallest
           (32, 0, 64, 2, 96),          # D - P = 76: KT = 96 has pad columns; layer 1 has din = h > d_in
           (32, 32, 64, 2, 128)]        # use_id_embedding: zero columns behind the query rows and inside pool.query_lin.w
F32, F64 = 2.0 ** -24, 2.0 ** -52


@functools.lru_cache(maxsize=None)
def folded(config):
    d_in, d_id, h, n_layers, d_out = config
    cfg = EncoderConfig(d_in=d_in, d_id=d_id, h=h, n_layers=n_layers, d_out=d_out, n_items=50, n_query=40)
    w = init_weights(cfg, 100 + CONFIGS.index(config))
    return cfg, w, session_fold_weights(cfg, w)


def bound(x, w_abs_t, b_abs, k):
    """The module docstring's bound; `w_abs_t` = |W_ref|^T [K, M], `b_abs` = |b_ref| [M] or 0."""
    mag = x.abs() @ w_abs_t
    return F32 * (mag + b_abs) + k * F64 * mag


def is_zero(t):
    return t.numel() == 0 or not bool(t.any())


@pytest.mark.parametrize("config", CONFIGS)
def test_copied_blocks_are_exact_and_pads_are_zero(config, monkeypatch):
    def no_library():
        raise AssertionError("session_fold_weights loaded the library")
    monkeypatch.setattr(_lib, "lib", no_library)
    cfg, w, _ = folded(config)
    f = session_fold_weights(cfg, w)                # folded again under the patch: it must not ask for libsss.so
    d_in, d_id, h, P, D = cfg.d_in, cfg.d_id, cfg.h, cfg.max_seq_len, cfg.d_out
    assert f["cfg"] == EncoderConfig(**{**cfg.__dict__, "d_in": cfg.d_p, "d_id": 0})
    assert set(f) == {"cfg", "tables", "layers", "pool", "pool_tab"} and len(f["layers"]) == cfg.n_layers

    blocks = [f["tables"], f["pool"], f["pool_tab"]] + f["layers"]
    for t in (t for blk in blocks for t in blk.values() if torch.is_tensor(t)):
        assert t.dtype == torch.float32 and t.is_contiguous() and t.device.type == "cpu"
    assert all(type(lay["din"]) is int for lay in f["layers"]) and type(f["pool_tab"]["KT"]) is int

    # tables: use_id_embedding makes product rows [id | text] and query rows [text | d_id zeros]
    tab = f["tables"]
    if d_id:
        assert set(tab) == {"item_table", "query_table", "id_table"} and torch.equal(tab["id_table"], w["item_table"])
        assert torch.equal(tab["item_table"], torch.cat([w["item_table"], w["item_text_table"]], 1))
        assert torch.equal(tab["query_table"][:, :d_in], w["query_table"]) and is_zero(tab["query_table"][:, d_in:])
        assert tab["query_table"].shape[1] == cfg.d_p
    else:
        assert set(tab) == {"item_table", "query_table"}
        assert torch.equal(tab["item_table"], w["item_table"]) and torch.equal(tab["query_table"], w["query_table"])

    for l, lay in enumerate(f["layers"]):
        g = lambda name: w[name.format(l)]
        din = cfg.d_p if l == 0 else h
        dq = d_in if l == 0 else h                  # columns of a query row that carry data
        assert list(lay) == ["wp", "bp", "wq", "w_ih", "b_ih", "bias_qp", "bias_pq", "din", "w7", "b7"] and lay["din"] == din
        wp, w7, wq, bp, b7 = lay["wp"], lay["w7"], lay["wq"], lay["bp"], lay["b7"]
        assert wp.shape == (5 * h + ALPHA_PAD, din) and w7.shape == (7 * h + ALPHA_PAD, din) and wq.shape == (h + ALPHA_PAD, din)
        assert bp.shape == (5 * h + ALPHA_PAD,) and b7.shape == (7 * h + ALPHA_PAD,)
        # product side: xs_p, then m (per-op) or u (fused), then gh, then the two alpha rows and 30 pad rows
        assert torch.equal(wp[:h], g("gat_pq.{}.lin_src")) and torch.equal(w7[:h], g("gat_pq.{}.lin_src"))
        assert torch.equal(wp[h:2 * h], g("ggc.{}.weight").T[:, :din])
        assert torch.equal(wp[2 * h:5 * h], g("ggc.{}.w_hh")[:, :din]) and torch.equal(w7[4 * h:7 * h], g("ggc.{}.w_hh")[:, :din])
        assert is_zero(wp[5 * h + 2:]) and is_zero(w7[7 * h + 2:]) and is_zero(wq[h + 2:])
        assert torch.equal(bp[2 * h:5 * h], g("ggc.{}.b_hh")) and is_zero(bp[:2 * h]) and is_zero(bp[5 * h:])
        assert torch.equal(b7[4 * h:7 * h], g("ggc.{}.b_hh")) and is_zero(b7[:4 * h]) and is_zero(b7[7 * h:])
        # query side: xs_q and the two alpha rows read query rows -- zero columns behind their dq data columns
        assert torch.equal(wq[:h, :dq], g("gat_qp.{}.lin_src")) and is_zero(wq[:, dq:])
        assert wq[:, dq:].shape[1] == (d_id if l == 0 else 0)
        for name in ("w_ih", "b_ih"):
            assert torch.equal(lay[name], g("ggc.{}." + name))
        assert torch.equal(lay["bias_qp"], g("gat_qp.{}.bias")) and torch.equal(lay["bias_pq"], g("gat_pq.{}.bias"))

    pool, ql = f["pool"], w["pool.query_lin.w"]
    assert list(pool) == ["wq", "bq", "wp", "bp", "pos", "wn", "bn", "wc", "watt"]
    assert pool["wq"].shape == (D - P, cfg.node_width)
    assert torch.equal(pool["wq"][:, :d_in], ql[:, :d_in]) and is_zero(pool["wq"][:, d_in:d_in + d_id])
    assert torch.equal(pool["wq"][:, d_in + d_id:], ql[:, d_in:])
    for key, name in (("bq", "query_lin.b"), ("wp", "product_lin.w"), ("bp", "product_lin.b"), ("pos", "pos_emb"),
                      ("wn", "node_lin.w"), ("bn", "node_lin.b"), ("wc", "coarse_lin.w"), ("watt", "att_lin.w")):
        assert torch.equal(pool[key], w["pool." + name]), key

    pt, Dl = f["pool_tab"], D - P
    assert list(pt) == ["KT", "tanhpos", "a2", "c2", "wnc"] and pt["KT"] == (Dl + 31) // 32 * 32
    assert pt["tanhpos"].shape == (P, P) and pt["a2"].shape == pt["c2"].shape == (P, D) and pt["wnc"].shape == (2 * D, pt["KT"])
    assert torch.equal(pt["wnc"][:D, :Dl], w["pool.node_lin.w"][:, :Dl]) and torch.equal(pt["wnc"][D:, :Dl], w["pool.coarse_lin.w"][:, :Dl])
    assert is_zero(pt["wnc"][:, Dl:]) and pt["KT"] > Dl


@pytest.mark.parametrize("config", CONFIGS)
def test_folded_blocks_against_the_float64_oracle(config):
    cfg, w, f = folded(config)
    d_in, h, P, D = cfg.d_in, cfg.h, cfg.max_seq_len, cfg.d_out
    W = {k: v.double() for k, v in w.items()}
    gen = torch.Generator().manual_seed(7)
    rows = lambda n, d: torch.randn((n, d), generator=gen, dtype=torch.float64)
    for l, lay in enumerate(f["layers"]):
        din = lay["din"]
        dq = d_in if l == 0 else h
        x_p, x_q = rows(7, din), rows(5, din)       # (use_id_embedding, layer 0: the query rows' pad columns hold data here --
        x_q_ref = x_q[:, :dq]                       #  the oracle never sees it, so it must meet exact zeros in wq)
        yp, yq = kr.node_transforms(W, l, x_p, x_q_ref)
        # |W_ref|^T and |b_ref| out of the oracle itself: its columns for unit rows, minus its columns for a zero row
        bp_ref, bq_ref = (y[0] for y in kr.node_transforms(W, l, torch.zeros((1, din), dtype=torch.float64),
                                                           torch.zeros((1, dq), dtype=torch.float64)))
        ep, eq = kr.node_transforms(W, l, torch.eye(din, dtype=torch.float64), torch.eye(dq, dtype=torch.float64))
        assert is_zero(bq_ref)
        k = 2 * (h + din)
        got_p = x_p @ lay["w7"].double().T + lay["b7"].double()
        got_q = x_q @ lay["wq"].double().T
        assert yp.shape == (7, 7 * h + 2) and yq.shape == (5, h + 2)
        tol_p = bound(x_p, (ep - bp_ref).abs(), bp_ref.abs(), k)
        tol_q = bound(x_q_ref, eq.abs(), 0.0, k)
        err_p, err_q = (got_p[:, :7 * h + 2] - yp).abs(), (got_q[:, :h + 2] - yq).abs()
        assert bool((err_p <= tol_p).all()), (l, "yp", float((err_p / tol_p).max()))
        assert bool((err_q <= tol_q).all()), (l, "yq", float((err_q / tol_q).max()))
        # the per-op stack carries the same two alpha rows behind its 5h columns
        got_a = x_p @ lay["wp"].double()[5 * h:5 * h + 2].T
        assert bool(((got_a - yp[:, 7 * h:]).abs() <= tol_p[:, 7 * h:]).all()), (l, "wp alpha rows")

    pt, Dl = f["pool_tab"], D - P
    wn, bn, wc = W["pool.node_lin.w"], W["pool.node_lin.b"], W["pool.coarse_lin.w"]
    t, ac, tp, a2, c2 = kr.tab_inputs(rows(7, Dl), rows(5, Dl), W["pool.pos_emb"], wn, bn, wc)
    t_pad = torch.zeros((12, pt["KT"]), dtype=torch.float64)
    t_pad[:, :Dl] = t
    k = 2 * (Dl + P)
    ident = torch.eye(P, dtype=torch.float64)
    for name, got, ref, tol in (
            ("tanhpos", pt["tanhpos"], tp, bound(ident, tp.abs(), 0.0, k)),
            ("a2", pt["a2"], a2, bound(tp, wn[:, Dl:].abs().T, bn.abs(), k)),
            ("c2", pt["c2"], c2, bound(tp, wc[:, Dl:].abs().T, 0.0, k)),
            ("t @ wnc^T", t_pad @ pt["wnc"].double().T, ac, bound(t, torch.cat([wn[:, :Dl], wc[:, :Dl]]).abs().T, 0.0, k))):
        err = (got.double() - ref).abs()
        assert err.shape == ref.shape and bool((err <= tol).all()), (name, float((err / tol.clamp_min(1e-300)).max()))


def test_a_bad_config_raises_the_config_errors():
    cfg, w, _ = folded(CONFIGS[0])
    for bad in (dict(d_in=48), dict(h=40), dict(d_out=72), dict(d_id=16), dict(d_id=-32), dict(d_in=64),
                dict(d_id=32), dict(d_out=0, max_seq_len=0), dict(self_loop_rule="pyg")):
        with pytest.raises(ValueError):
            session_fold_weights(EncoderConfig(**{**cfg.__dict__, **bad}), w)


def test_package_exports_the_fold():
    import sessionsimilaritysearch_amd as pkg
    from sessionsimilaritysearch_amd import encoder
    assert pkg.session_fold_weights is encoder.session_fold_weights and "session_fold_weights" in pkg.__all__
