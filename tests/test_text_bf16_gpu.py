"""The ``gemm=`` switch of text.BertNodeEncoder and text.NodeTextTransformer on the device: ``gemm="f32"`` is the object built
without the keyword, bit for bit; ``gemm="bf16"`` is held to the full-precision float64 reference through a calibrated bound
(below); dedup and chunking change no bit under bf16 either.

THE BOUND.  No pointwise contract against a rounding-matched oracle exists for a forward: float32 noise flips bfloat16
roundings.  So ``ref`` is the float64 helper (bert_ref / text_ref), ``dev_lowp`` the max abs
deviation from ``ref`` of the float64 restatement that rounds both operands of every GEMM to bfloat16
(tests/helpers/lowp_ref.py), and the device must satisfy
    max |got - ref|  <=  3 * dev_lowp + 1e-5 * max(1, max |ref|).
The device performs the same roundings on slightly different values: its deviation is a draw from the same distribution, and
the maximum over a few thousand elements of two such draws differs by a small factor -- 3.  A wiring fault (a wrong weight,
a missing 1 / sqrt(D) fold, float32 weights read as bf16) deviates by O(max |ref|), about 100 x the bound."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import bert_ref as br  # noqa: E402
import lowp_ref as lr  # noqa: E402
import text_ref as tr  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_CACHE = {}


def bert_fixture():
    z = np.load(os.path.join(ROOT, "tests", "golden", "bert_encoder.npz"))
    w = {k[2:]: torch.from_numpy(z[k].astype(np.float32)) for k in z.files if k.startswith("w:")}
    return w, int(z["heads"]), float(z["eps"]), z["input_ids"], z["token_type_ids"], z["attention_mask"]


def text_fixture(name="cfg_like"):
    z = np.load(os.path.join(ROOT, "tests", "golden", "text_transformer.npz"))
    w = {k.split(":w:")[1]: torch.from_numpy(z[k].astype(np.float32)) for k in z.files if k.startswith(name + ":w:")}
    src = z[name + ":src"]                                            # [9, 20], lengths 20 1 2 5 12 3 19 20 7
    return w, int(z[name + ":nhead"]), src, tr.prefix_mask(z[name + ":lengths"], src.shape[1])


def held(what, got, ref, lowp):
    got = got.double().cpu().numpy()
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    dev_gpu, dev_lowp, scale = float(np.abs(got - ref).max()), float(np.abs(lowp - ref).max()), float(np.abs(ref).max())
    bound = 3 * dev_lowp + 1e-5 * max(1.0, scale)
    print(f"{what}: dev_gpu = {dev_gpu:.3e}, dev_lowp = {dev_lowp:.3e}, ratio {dev_gpu / dev_lowp:.3f}, bound {bound:.3e}, max|ref| {scale:.2f}")
    assert dev_lowp > 1e-4 * scale, "the restatement does not round: the bound would hold float32 noise only"
    assert dev_gpu <= bound, what


def test_gemm_f32_is_the_object_without_the_keyword(cuda):
    from sessionsimilaritysearch_amd.text import BertNodeEncoder, NodeTextTransformer
    w, heads, eps, ids, tt, am = bert_fixture()
    for pool in ("masked", "mean"):
        plain, f32 = BertNodeEncoder(w, heads, pool=pool, eps=eps, device=cuda), BertNodeEncoder(w, heads, pool=pool, eps=eps, device=cuda, gemm="f32")
        assert plain.gemm == f32.gemm == "f32" and all(t.dtype == torch.float32 for lay in f32.layers for t in lay.values())
        (a, a_tok), (b, b_tok) = plain(ids, tt, am, get_token=True), f32(ids, tt, am, get_token=True)
        assert torch.equal(a, b) and torch.equal(a_tok, b_tok)
    tw, nhead, src, mask = text_fixture()
    for rule in ("compute", "zero"):
        plain, f32 = NodeTextTransformer(tw, nhead, pad_rule=rule, device=cuda), NodeTextTransformer(tw, nhead, pad_rule=rule, device=cuda, gemm="f32")
        assert torch.equal(plain.forward(src, mask), f32.forward(src, mask))


GEOMETRIES = {"128/2/96 x 1": (128, 2, 96, 1), "64/4/80 x 2": (64, 4, 80, 2)}      # e / heads / intermediate x layers


def bert_case(name):
    """(weights, heads, ids, tt, am, float64 states, restated states), built once: B = 6, T = 8, a half-masked row, a
    single-token row, a Linear(e, 10) head."""
    if name not in _CACHE:
        e, heads, inter, nlayers = GEOMETRIES[name]
        w = br.seeded_weights(len(name) + e, 50, e, heads, inter, nlayers, 16, nout=10)
        rng = np.random.default_rng(e)
        B, T, lengths = 6, 8, [8, 4, 1, 8, 5, 7]
        ids, tt = rng.integers(0, 50, (B, T)).astype(np.int64), rng.integers(0, 2, (B, T)).astype(np.int64)
        am = (np.arange(T)[None, :] < np.asarray(lengths)[:, None]).astype(np.int64)
        _CACHE[name] = (w, heads, ids, tt, am, br.token_states(w, heads, ids, tt, am), lr.bert_token_states(w, heads, ids, tt, am))
    return _CACHE[name]


@pytest.mark.parametrize("name", list(GEOMETRIES))
@pytest.mark.parametrize("pool", ["masked", "mean"])
def test_bert_encoder_bf16_against_the_float64_reference(cuda, name, pool):
    """Token states (get_token=True, every position) and the pooled output through the lin head, both under THE BOUND; only
    the bf16 copy of the GEMM weights is on the device.  Observed ratios: DESIGN.md section 5.10."""
    from sessionsimilaritysearch_amd.text import GEMM_WEIGHTS, BertNodeEncoder
    w, heads, ids, tt, am, ref, lowp = bert_case(name)
    enc = BertNodeEncoder(w, heads, pool=pool, device=cuda, gemm="bf16")
    assert enc.lin_w.dtype == torch.bfloat16 and enc.lin_b.dtype == torch.float32
    assert all(t.dtype == (torch.bfloat16 if n in GEMM_WEIGHTS else torch.float32) for lay in enc.layers for n, t in lay.items())
    out, tokens = enc(ids, tt, am, get_token=True)
    assert out.shape == (6, 10) and tokens.shape == (6, 8, GEOMETRIES[name][0]) and out.dtype == tokens.dtype == torch.float32
    held(f"{name} {pool} tokens", tokens, ref, lowp)
    held(f"{name} {pool} pooled", out, br.head(w, ref, am, pool), lr.bert_head(w, lowp, am, pool))
    assert torch.equal(enc(ids, tt, am), out)                           # without get_token; a second call


@pytest.mark.parametrize("rule", ["compute", "zero"])
def test_text_transformer_bf16_against_the_float64_reference(cuda, rule):
    """The text fixture's module (100 / nhid 48: K = 128 and 64 after pad32) on its own batch, under both padding rules."""
    from sessionsimilaritysearch_amd.text import NodeTextTransformer
    tw, nhead, src, mask = text_fixture()
    if "text" not in _CACHE:
        _CACHE["text"] = {r: (tr.forward(tw, nhead, src, mask, r), lr.text_forward(tw, nhead, src, mask, r)) for r in ("compute", "zero")}
    enc = NodeTextTransformer(tw, nhead, pad_rule=rule, device=cuda, gemm="bf16")
    assert enc.layers[0]["in_w"].dtype == torch.bfloat16 and enc.layers[0]["in_b"].dtype == torch.float32 and enc.table.dtype == torch.float32
    held(f"text {rule}", enc.forward(src, mask), *_CACHE["text"][rule])


def test_invariances_hold_under_bf16(cuda):
    """dedup on and off, and two chunk sizes, are bit-equal: the GEMM's sum order depends on K alone, never on the row count
    or on a row's place in its tile."""
    from sessionsimilaritysearch_amd.text import BertNodeEncoder, NodeTextTransformer
    w = br.seeded_weights(77, 60, 96, 4, 100, 2, 64, nout=10)
    rng = np.random.default_rng(77)
    T, lengths = 40, [40, 2, 2, 17, 2, 40, 1, 17, 33]
    B = len(lengths)
    ids, tt = rng.integers(0, 60, (B, T)).astype(np.int64), rng.integers(0, 2, (B, T)).astype(np.int64)
    am = (np.arange(T)[None, :] < np.asarray(lengths)[:, None]).astype(np.int64)
    for dst, src in ((2, 1), (4, 1), (7, 3), (5, 0)):
        ids[dst], tt[dst] = ids[src], tt[src]
    for pool in ("masked", "mean"):
        on = BertNodeEncoder(w, 4, pool=pool, device=cuda, gemm="bf16")
        off = BertNodeEncoder(w, 4, pool=pool, device=cuda, gemm="bf16", dedup=False)
        one = BertNodeEncoder(w, 4, pool=pool, device=cuda, gemm="bf16", dedup=False, chunk_rows=64)
        (a, a_tok), (b, b_tok), (c, c_tok) = (e(ids, tt, am, get_token=True) for e in (on, off, one))
        assert torch.equal(a, b) and torch.equal(a_tok, b_tok) and torch.equal(a, c) and torch.equal(a_tok, c_tok)
        assert not torch.equal(a, BertNodeEncoder(w, 4, pool=pool, device=cuda)(ids, tt, am))      # and it is not the f32 path
    tw, nhead, src, mask = text_fixture()
    big, small = (NodeTextTransformer(tw, nhead, device=cuda, gemm="bf16", chunk_rows=c) for c in (131072, 64))
    assert torch.equal(big.forward(src, mask), small.forward(src, mask))
