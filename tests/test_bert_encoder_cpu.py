"""CPU side of the node text encoder (include/sss_bert.h, text.BertNodeEncoder): the dense helper of
tests/helpers/bert_ref.py against the stored outputs of the `transformers` BertModel (and against a live one where the
library is installed), bert_fold_weights against the unfolded helper, bert_pack_rows against a few lines of numpy under both
pools, the header against its ctypes binding, and every rejection, which comes before any device work."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
from abi import declared  # noqa: E402
import bert_ref as br  # noqa: E402

from sessionsimilaritysearch_amd import _lib  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def load_fixture():
    """(weights {state_dict name: float32 array}, heads, eps, {the other arrays})."""
    z = np.load(os.path.join(ROOT, "tests", "golden", "bert_encoder.npz"))
    w = {k[2:]: z[k].astype(np.float32) for k in z.files if k.startswith("w:")}
    return w, int(z["heads"]), float(z["eps"]), {k: z[k] for k in z.files if not k.startswith("w:")}


def close(got, want, what):
    """The bound of tests/test_text_transformer_cpu.py: 2e-5 * max(1, max |ref|), some 10x the float32 model's own rounding."""
    err, bound = np.abs(got - want).max(), 2e-5 * max(1.0, np.abs(want).max())
    print(f"{what}: max|err| = {err:.3e}, bound {bound:.3e}")
    assert err <= bound, (what, err, bound)


# ------------------------------------------------------------------------------------------------ helper vs transformers
def test_helper_reproduces_the_fixture():
    w, heads, eps, rec = load_fixture()
    assert rec["input_ids"].shape == (7, 12) and rec["lengths"].tolist() == [12, 1, 7, 3, 12, 2, 5]
    assert len(np.unique(rec["token_type_ids"])) == 2 and eps == 1e-12
    ids, tt, am = rec["input_ids"], rec["token_type_ids"], rec["attention_mask"]
    s = br.token_states(w, heads, ids, tt, am, eps)
    assert s.dtype == np.float64
    close(s, rec["last_hidden_state"], "last_hidden_state")
    close(br.pool(s, am, "masked"), rec["pooled_masked"], "masked mean")
    close(br.pool(s, am, "mean"), rec["pooled_mean"], "plain mean")
    assert np.abs(br.pool(s, am, "masked") - br.pool(s, am, "mean")).max() > 0.1          # two different poolings
    # the stored errors are the model's float32 rounding, of the size the float32 helper shows
    s32 = br.token_states(w, heads, ids, tt, am, eps, torch.float32)
    assert s32.dtype == np.float32 and 0 < float(rec["err_states"]) < 2e-5 and np.abs(s32 - s).max() < 2e-5


def test_padded_ids_do_not_reach_the_valid_rows():
    """Replacing every padded id changes no bit of the valid rows or of the masked mean -- in the stored `transformers`
    outputs and in the helper -- while the padded rows, and with them the plain mean, do change."""
    w, heads, eps, rec = load_fixture()
    valid = rec["attention_mask"].astype(bool)
    assert ((rec["input_ids_alt"] != rec["input_ids"]) == ~valid).all()
    a, b = rec["last_hidden_state"], rec["last_hidden_state_alt"]
    assert np.array_equal(a[valid], b[valid]) and (a[~valid] != b[~valid]).any()
    s = br.token_states(w, heads, rec["input_ids"], rec["token_type_ids"], rec["attention_mask"], eps)
    s_alt = br.token_states(w, heads, rec["input_ids_alt"], rec["token_type_ids"], rec["attention_mask"], eps)
    assert np.array_equal(s[valid], s_alt[valid]) and (s[~valid] != s_alt[~valid]).any()
    assert np.array_equal(br.pool(s, valid, "masked"), br.pool(s_alt, valid, "masked"))
    assert not np.array_equal(br.pool(s, valid, "mean"), br.pool(s_alt, valid, "mean"))


def test_helper_matches_a_live_bert_model():
    """128 / 2 heads (D = 64, the attention kernel's ceiling) / 96 / 1 layer, weights from the helper's seed."""
    tf = pytest.importorskip("transformers")
    cfg = tf.BertConfig(vocab_size=50, hidden_size=128, num_attention_heads=2, intermediate_size=96, num_hidden_layers=1,
                        max_position_embeddings=16, type_vocab_size=2)
    model = tf.BertModel(cfg, add_pooling_layer=False).eval()
    w = br.seeded_weights(3, 50, 128, 2, 96, 1, 16)
    assert set(w) == set(model.state_dict())
    model.load_state_dict(w)
    rng = np.random.default_rng(3)
    ids, tt = rng.integers(0, 50, (5, 9)), rng.integers(0, 2, (5, 9))
    am = (np.arange(9)[None, :] < np.array([9, 1, 4, 2, 8])[:, None]).astype(np.int64)
    with torch.no_grad():
        want = model(input_ids=torch.from_numpy(ids), token_type_ids=torch.from_numpy(tt), attention_mask=torch.from_numpy(am)).last_hidden_state
    close(br.token_states(w, 2, ids, tt, am, cfg.layer_norm_eps), want.numpy(), "live BertModel")


# ------------------------------------------------------------------------------------------------ bert_fold_weights
def _unfold(f):
    """The folded weights back under HF's names, pad columns cut off (q still carries 1 / sqrt(D))."""
    e, inter = f["e"], f["inter"]
    w = {"embeddings.word_embeddings.weight": f["word"], "embeddings.position_embeddings.weight": f["pos"],
         "embeddings.token_type_embeddings.weight": f["type"], "embeddings.LayerNorm.weight": f["emb_g"], "embeddings.LayerNorm.bias": f["emb_b"]}
    for l, lay in enumerate(f["layers"]):
        p = br.LAYER.format(l)
        for i, n in enumerate(("query", "key", "value")):
            w[p + f"attention.self.{n}.weight"], w[p + f"attention.self.{n}.bias"] = lay["in_w"][i * e:(i + 1) * e, :e], lay["in_b"][i * e:(i + 1) * e]
        w.update({p + "attention.output.dense.weight": lay["out_w"][:, :e], p + "attention.output.dense.bias": lay["out_b"],
                  p + "intermediate.dense.weight": lay["l1_w"][:inter, :e], p + "intermediate.dense.bias": lay["l1_b"][:inter],
                  p + "output.dense.weight": lay["l2_w"][:, :inter], p + "output.dense.bias": lay["l2_b"],
                  p + "attention.output.LayerNorm.weight": lay["n1_w"], p + "attention.output.LayerNorm.bias": lay["n1_b"],
                  p + "output.LayerNorm.weight": lay["n2_w"], p + "output.LayerNorm.bias": lay["n2_b"]})
    return w


@pytest.mark.parametrize("geometry", ["fixture D=16", "128/2 D=64", "96/4 D=24 inter=100"])
def test_fold_weights(geometry):
    """Shapes, zero pads, and the fold: the helper on the unfolded weights with q scaled back by sqrt(D) equals the helper on
    the raw weights within float64 rounding.  At D = 16 and D = 64 the factor is a power of two, so the float32 q rows the
    device gets are exactly the raw rows / sqrt(D)."""
    from sessionsimilaritysearch_amd.text import bert_fold_weights
    if geometry.startswith("fixture"):
        w, heads, _, _ = load_fixture()
        w["lin.weight"], w["lin.bias"] = np.ones((10, 64), np.float32), np.arange(10, dtype=np.float32)
    elif geometry.startswith("128"):
        w, heads = br.seeded_weights(5, 40, 128, 2, 96, 1, 16), 2
    else:
        w, heads = br.seeded_weights(6, 40, 96, 4, 100, 2, 16), 4
    wt = {k: torch.as_tensor(v) for k, v in w.items()}
    f = bert_fold_weights(wt, heads)
    e, inter = wt["embeddings.word_embeddings.weight"].shape[1], wt["encoder.layer.0.intermediate.dense.weight"].shape[0]
    D, K, H = e // heads, (e + 31) // 32 * 32, (inter + 31) // 32 * 32
    assert (f["e"], f["heads"], f["inter"], f["nlayers"]) == (e, heads, inter, br.n_layers(w))
    assert f["word"].shape == wt["embeddings.word_embeddings.weight"].shape and f["pos"].shape[1] == e and f["type"].shape == (2, e)
    for l, lay in enumerate(f["layers"]):
        assert all(v.dtype == torch.float64 for v in lay.values())
        assert lay["in_w"].shape == (3 * e, K) and lay["in_b"].shape == (3 * e,) and lay["out_w"].shape == (e, K)
        assert lay["l1_w"].shape == (H, K) and lay["l1_b"].shape == (H,) and lay["l2_w"].shape == (e, H)
        for n in ("in_w", "out_w", "l1_w"):
            assert bool((lay[n][:, e:] == 0).all())
        assert bool((lay["l1_w"][inter:] == 0).all()) and bool((lay["l1_b"][inter:] == 0).all()) and bool((lay["l2_w"][:, inter:] == 0).all())
        p = br.LAYER.format(l)
        q_w, q_b = wt[p + "attention.self.query.weight"].double(), wt[p + "attention.self.query.bias"].double()
        assert torch.allclose(lay["in_w"][:e, :e] * D ** 0.5, q_w, rtol=1e-15, atol=0) and torch.allclose(lay["in_b"][:e] * D ** 0.5, q_b, rtol=1e-15, atol=0)
        assert torch.equal(lay["in_w"][e:2 * e, :e], wt[p + "attention.self.key.weight"].double())
        assert torch.equal(lay["in_w"][2 * e:, :e], wt[p + "attention.self.value.weight"].double())
        if D in (16, 64):                                               # exact in float32 too
            assert torch.equal(lay["in_w"][:e, :e].float() * D ** 0.5, wt[p + "attention.self.query.weight"])
            assert torch.equal(lay["in_b"][:e].float() * D ** 0.5, wt[p + "attention.self.query.bias"])
    if "lin.weight" in w:
        assert f["lin_w"].shape == (10, K) and torch.equal(f["lin_w"][:, :e], wt["lin.weight"].double()) and torch.equal(f["lin_b"], wt["lin.bias"].double())
    else:
        assert f["lin_w"] is None and f["lin_b"] is None
    rng = np.random.default_rng(1)
    ids, tt = rng.integers(0, 40, (4, 7)), rng.integers(0, 2, (4, 7))
    am = (np.arange(7)[None, :] < np.array([7, 1, 3, 6])[:, None]).astype(np.int64)
    raw = {k: v for k, v in w.items() if not k.startswith("lin.")}
    a = br.token_states(raw, heads, ids, tt, am)
    un = _unfold(f)
    assert np.abs(br.token_states(un, heads, ids, tt, am) - a).max() > 1e-6          # the fold is not a no-op
    for l in range(f["nlayers"]):
        p = br.LAYER.format(l)
        un[p + "attention.self.query.weight"], un[p + "attention.self.query.bias"] = (un[p + "attention.self.query.weight"] * D ** 0.5,
                                                                                     un[p + "attention.self.query.bias"] * D ** 0.5)
    assert np.abs(br.token_states(un, heads, ids, tt, am) - a).max() < 1e-12
    with pytest.raises(ValueError):
        bert_fold_weights(wt, 7)


def test_both_folds_give_the_same_layers():
    """bert_fold_weights and text_fold_weights share one layer fold: BERT layers re-keyed under the transformer's names, with
    query | key | value stacked into one in_proj, fold to bit-equal layer dicts (96 / 4: 1 / sqrt(24) is not a power of two,
    intermediate 100 needs row and column pads)."""
    from sessionsimilaritysearch_amd.text import LAYER, bert_fold_weights, text_fold_weights
    heads = 4
    wb = {k: torch.as_tensor(v) for k, v in br.seeded_weights(6, 40, 96, heads, 100, 2, 16).items()}
    wt = {"embedding.weight": wb["embeddings.word_embeddings.weight"], "pos_encoder.pe": wb["embeddings.position_embeddings.weight"]}
    names = {"attention.output.dense": "self_attn.out_proj", "intermediate.dense": "linear1", "output.dense": "linear2",
             "attention.output.LayerNorm": "norm1", "output.LayerNorm": "norm2"}
    for l in range(2):
        pb, pt = br.LAYER.format(l), LAYER.format(l)
        for kind, to in (("weight", "in_proj_weight"), ("bias", "in_proj_bias")):
            wt[pt + "self_attn." + to] = torch.cat([wb[pb + f"attention.self.{n}.{kind}"] for n in ("query", "key", "value")])
        for a, b in names.items():
            wt[pt + b + ".weight"], wt[pt + b + ".bias"] = wb[pb + a + ".weight"], wb[pb + a + ".bias"]
    fb, ft = bert_fold_weights(wb, heads), text_fold_weights(wt, heads)
    assert (ft["nlayers"], ft["nhid"], ft["ninp"]) == (fb["nlayers"], fb["inter"], fb["e"]) == (2, 100, 96)
    for lb, lt in zip(fb["layers"], ft["layers"]):
        assert lb.keys() == lt.keys() and len(lb) == 12
        for k in lb:
            assert lb[k].dtype == lt[k].dtype == torch.float64 and torch.equal(lb[k], lt[k]), k


# ------------------------------------------------------------------------------------------------ bert_pack_rows
def _pack_np(ids, tt, am, pool, all_rows):
    tok, typ, pos, key, w, ptr = [], [], [], [], [], [0]
    B, T = ids.shape
    for b in range(B):
        n_valid = int((am[b] != 0).sum())
        for t in range(T):
            if pool == "mean" or all_rows or am[b, t]:
                tok.append(ids[b, t]); typ.append(tt[b, t]); pos.append(t); key.append(am[b, t] != 0)
                w.append(np.float32(1.0 / T) if pool == "mean" else (np.float32(1.0) / np.float32(n_valid) if am[b, t] else np.float32(0.0)))
        ptr.append(len(tok))
    return (np.array(tok, np.int64), np.array(pos, np.int32), np.array(ptr, np.int32), np.array(key, np.uint8), np.array(typ, np.int32),
            np.array(w, np.float32))


@pytest.mark.parametrize("pool,all_rows", [("masked", False), ("masked", True), ("mean", False), ("mean", True)])
def test_pack_rows_under_both_pools(pool, all_rows):
    """Position = index in the padded row, key_ok = attention mask; "masked" without get_token drops the padded rows, every
    other setting keeps all T.  The weights of a sequence's rows add up to 1 over the rows its pool counts."""
    from sessionsimilaritysearch_amd.text import BertRows, bert_pack_rows
    rng = np.random.default_rng(9)
    cases = []
    for T, lengths in ((12, [12, 1, 7, 3]), (1, [1, 1]), (64, [64, 1, 63])):
        am = (np.arange(T)[None, :] < np.asarray(lengths)[:, None]).astype(np.int64)
        cases.append((rng.integers(0, 30, am.shape), rng.integers(0, 2, am.shape), am))
    holes = np.ones((2, 6), np.int64)
    holes[0, 0] = holes[1, 2] = holes[1, 5] = 0                          # not prefix masks
    cases.append((rng.integers(0, 30, (2, 6)), rng.integers(0, 2, (2, 6)), holes))
    for ids, tt, am in cases:
        for conv in (lambda a: a, torch.from_numpy):
            got = bert_pack_rows(conv(ids), conv(tt), conv(am), pool, all_rows, n_word=30, n_type=2)
            assert isinstance(got, BertRows) and got.rows.T == ids.shape[1]
            want = _pack_np(ids, tt, am, pool, all_rows)
            for g, w in zip(list(got.rows[:4]) + [got.tt, got.w], want):
                assert g.dtype == w.dtype and np.array_equal(g, w)
        sums = np.add.reduceat(got.w.astype(np.float64), got.rows.ptr[:-1])
        assert np.abs(sums - 1).max() < 1e-6
        if pool == "masked" and not all_rows:
            assert len(got.w) == int((am != 0).sum()) and got.rows.key_ok.all()
        else:
            assert len(got.w) == am.size and np.array_equal(got.rows.key_ok, (am != 0).reshape(-1))
    ids, tt, am = cases[0]
    with pytest.raises(ValueError):
        bert_pack_rows(ids, tt, am, "max")
    with pytest.raises(ValueError):
        bert_pack_rows(ids, tt[:, :5], am, pool)
    dead = am.copy()
    dead[2] = 0
    with pytest.raises(ValueError):
        bert_pack_rows(ids, tt, dead, pool, all_rows)
    bad = tt.copy()
    bad[1, 3] = 2
    with pytest.raises(IndexError):
        bert_pack_rows(ids, bad, am, pool, all_rows, n_word=30, n_type=2)
    bad = ids.copy()
    bad[1, 3] = 30
    with pytest.raises(IndexError):
        bert_pack_rows(bad, tt, am, pool, all_rows, n_word=30, n_type=2)


def test_unique_rows_partitions_like_numpy():
    """The distinct (ids, types, mask) rows: the partition np.unique(axis=0) gives over the int64 columns.  A row that differs
    only in one type, one mask bit or one id (by 2^16: another byte) is distinct; a non-zero mask value counts as 1."""
    from sessionsimilaritysearch_amd.text import unique_rows
    rng = np.random.default_rng(2)
    B, T = 40, 6
    ids, tt, am = rng.integers(0, 1 << 20, (B, T)), rng.integers(0, 2, (B, T)), rng.integers(0, 2, (B, T))
    for dst, src in ((5, 1), (9, 1), (30, 12), (31, 12), (32, 12), (33, 12)):
        ids[dst], tt[dst], am[dst] = ids[src], tt[src], am[src]
    tt[31, 2] ^= 1
    am[32, 5] ^= 1
    ids[33, 0] ^= 1 << 16
    first, inverse = unique_rows(ids, tt, am * 7)
    assert first.dtype == np.int64 and inverse.dtype == np.int64 and inverse.shape == (B,)
    rows = np.concatenate([ids, tt, am], axis=1)
    assert len(first) == len(np.unique(rows, axis=0)) == B - 3 and np.array_equal(rows[first][inverse], rows)
    assert inverse[5] == inverse[1] == inverse[9] and inverse[30] == inverse[12] and len({*inverse[[12, 31, 32, 33]]}) == 4
    f0, i0 = unique_rows(ids[:0], tt[:0], am[:0])
    assert len(f0) == 0 and len(i0) == 0


# ------------------------------------------------------------------------------------------------ symbols
def test_bert_header_and_binding_declare_the_same_entry_point():
    names = declared("sss_bert.h")
    assert names == _lib.symbols("sss_bert.h") == ["sss_bert_embed"]
    L = _lib.lib()
    assert L.sss_bert_embed.argtypes == _lib.HEADERS["sss_bert.h"]["sss_bert_embed"][1] and L.sss_bert_embed.restype is ctypes.c_int
    for header, table in _lib.HEADERS.items():
        if header != "sss_bert.h":
            assert not set(names) & set(table) and not set(names) & set(declared(header)), header
    assert sorted(_lib.HEADERS) == sorted(f for f in os.listdir(os.path.join(ROOT, "include")) if f.endswith(".h"))
    assert declared("sss.h") == _lib.exported_symbols() and len(_lib.exported_symbols()) == 60
    text = open(os.path.join(ROOT, "include", "sss_bert.h")).read()
    for phrase in ("CALLER-OWNED DEVICE", "nothing is allocated", "no host synchronisation", "enqueued on `stream`",
                   "-1 bad argument", "-3 HIP error", "bert_embed:"):
        assert phrase in text, phrase
    plain = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    params = re.search(r"\bsss_bert_embed\s*\(([^)]*)\)", plain, re.S).group(1)
    assert len(params.split(",")) == len(_lib.HEADERS["sss_bert.h"]["sss_bert_embed"][1])
    assert "5 gelu" in open(os.path.join(ROOT, "include", "sss.h")).read()


def test_package_exports_the_bert_encoder():
    import sessionsimilaritysearch_amd as pkg
    from sessionsimilaritysearch_amd import text
    assert pkg.BertNodeEncoder is text.BertNodeEncoder and pkg.bert_fold_weights is text.bert_fold_weights
    assert pkg.bert_pack_rows is text.bert_pack_rows and pkg.BertRows is text.BertRows
    assert {"BertNodeEncoder", "bert_fold_weights", "bert_pack_rows", "BertRows"} <= set(pkg.__all__)


# ------------------------------------------------------------------------------------------------ rejections
_P = 1 << 20                                                          # a non-null, 16-byte aligned address; never dereferenced


def _embed(L, **kw):
    a = dict(word=_P, n_word=50, type=_P, n_type=2, pos=_P, n_pos=64, tok=_P, tt=_P, p=_P, gamma=_P, beta=_P, eps=1e-12, n=7, e=200,
             x=_P, ld_x=224, err=_P, st=0)
    a.update(kw)
    return L.sss_bert_embed(*a.values())


def test_argument_checks_return_before_any_device_work():
    """No address given here is memory: a call that launched would fault."""
    L = _lib.lib()
    for kw in (dict(e=0), dict(e=6), dict(e=1028), dict(ld_x=196), dict(ld_x=226), dict(n_word=0), dict(n_type=0), dict(n_pos=0),
               dict(eps=0.0), dict(eps=-1.0), dict(n=-1), dict(n=1 << 31), dict(word=0), dict(type=0), dict(pos=0), dict(gamma=0),
               dict(beta=_P + 8), dict(x=0), dict(x=_P + 4), dict(tok=0), dict(tt=0), dict(p=0), dict(err=0)):
        assert _embed(L, **kw) == -1 and L.sss_last_error().startswith(b"bert_embed:"), kw
    assert _embed(L, n=0) == 0 and _embed(L, n=0, word=0, type=0, pos=0, tok=0, tt=0, p=0, gamma=0, beta=0, x=0, err=0) == 0
    assert _embed(L, n=0, e=6) == -1 and _embed(L, n=0, n_type=0) == -1     # an empty batch's scalars are still checked
    # the grouped GEMM takes act 0..5 now and nothing past it
    for act in (-1, 6):
        prob = (_lib.LinearProblem * 1)(_lib.LinearProblem(x=_P, ldx=32, w=_P, ldw=32, y=_P, ldy=32, n=4, m=4, act=act))
        assert L.sss_linear_grouped(prob, 1, 32, 0) == -1 and b"0..5" in L.sss_last_error()


def test_encoder_rejects_before_any_device_work():
    """Construction: an activation other than the erf GELU, non-absolute positions, e % 4, e > 1024, head width > 64, heads
    that do not divide e, a pool it does not know, an embeddings_project.  Call: T > 64, T > max_position_embeddings, a
    sequence with no attended token, a token type out of range.  device="cpu": nothing here reaches a kernel."""
    from sessionsimilaritysearch_amd.text import BertNodeEncoder
    w = br.seeded_weights(1, 30, 64, 4, 40, 1, 80)
    ok = BertNodeEncoder(w, 4, device="cpu")
    assert (ok.ninp, ok.nhead, ok.inter, ok.nlayers, ok.nout, ok.eps, ok.pool, ok.dedup) == (64, 4, 40, 1, 64, 1e-12, "masked", True)
    for kw in (dict(hidden_act="gelu_new"), dict(hidden_act="relu"), dict(position_embedding_type="relative_key"), dict(pool="max"),
               dict(chunk_rows=10), dict(eps=0.0)):
        with pytest.raises(ValueError):
            BertNodeEncoder(w, 4, device="cpu", **kw)
    for heads in (3, 0):                                                # 64 % 3; no head
        with pytest.raises(ValueError):
            BertNodeEncoder(w, heads, device="cpu")
    for e, heads in ((66, 3), (1056, 33), (260, 4), (128, 1)):          # e % 4; e > 1024; head width 65; head width 128
        with pytest.raises(ValueError):
            BertNodeEncoder(br.seeded_weights(1, 5, e, heads, 8, 1, 4), heads, device="cpu")
    with pytest.raises(ValueError):
        BertNodeEncoder(dict(w, **{"embeddings_project.weight": torch.zeros(64, 32)}), 4, device="cpu")

    class Cfg:
        num_attention_heads, layer_norm_eps, hidden_act, position_embedding_type = 4, 1e-12, "gelu", "absolute"

    class Model:
        config = Cfg()
        state_dict = staticmethod(lambda: w)
    enc = BertNodeEncoder.from_transformers(Model(), lin=torch.nn.Linear(64, 10), device="cpu", pool="mean")
    assert (enc.nhead, enc.eps, enc.nout, enc.pool) == (4, 1e-12, 10, "mean")
    Cfg.hidden_act = "relu"
    with pytest.raises(ValueError):
        BertNodeEncoder.from_transformers(Model(), device="cpu")
    Cfg.hidden_act, Cfg.position_embedding_type = "gelu", "relative_key_query"
    with pytest.raises(ValueError):
        BertNodeEncoder.from_transformers(Model(), device="cpu")

    one = lambda T: (np.zeros((2, T), np.int64), np.zeros((2, T), np.int64), np.ones((2, T), np.int64))
    with pytest.raises(ValueError):
        ok(*one(65))                                                    # the attention kernel's 64
    short = BertNodeEncoder(br.seeded_weights(1, 30, 64, 4, 40, 1, 8), 4, device="cpu")
    with pytest.raises(ValueError):
        short(*one(9))                                                  # max_position_embeddings = 8
    ids, tt, am = one(6)
    am[1] = 0
    for get_token in (False, True):
        with pytest.raises(ValueError):
            ok(ids, tt, am, get_token=get_token)
    with pytest.raises(ValueError):
        ok(ids, tt[:, :5], np.ones((2, 6), np.int64))
    tt[0, 2] = 2
    with pytest.raises(IndexError):
        ok(ids, tt, np.ones((2, 6), np.int64))
