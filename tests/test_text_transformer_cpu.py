"""CPU side of the query text encoder (include/sss_text.h, text.NodeTextTransformer): the float64 helper of
tests/helpers/text_ref.py against the reference's own stored outputs under both padding rules, pack_tokens against a few
lines of numpy, text_fold_weights against the unfolded helper, the header against its ctypes binding, and the argument
checks of the three entry points, which return before any device work."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
from abi import declared  # noqa: E402
import text_ref as tr  # noqa: E402

from sessionsimilaritysearch_amd import _lib  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RECORDS = ("cfg_like", "t64", "t1", "full")


def load_record(name):
    """(weights {state_dict name: float32 array}, nhead, {the record's other arrays})."""
    z = np.load(os.path.join(ROOT, "tests", "golden", "text_transformer.npz"))
    wname = "t64" if name == "t1" else name                            # t1 ran t64's module
    w = {k.split(":w:")[1]: z[k].astype(np.float32) for k in z.files if k.startswith(wname + ":w:")}
    rec = {k.split(":", 1)[1]: z[k] for k in z.files if k.startswith(name + ":") and ":w:" not in k}
    return w, int(rec["nhead"]), rec


# ------------------------------------------------------------------------------------------------ helper vs reference
@pytest.mark.parametrize("name", RECORDS)
def test_helper_matches_the_reference_under_both_rules(name):
    """max |ref - helper| <= 2e-5 * max(1, max |ref|): more than 10x the reference's own float32 rounding at these shapes
    (worst measured 3.6e-6 at scale 2.7), far below the O(1) gap between the two rules, which is asserted too."""
    w, nhead, rec = load_record(name)
    src, T = rec["src"], rec["src"].shape[1]
    mask = tr.prefix_mask(rec["lengths"], T)
    ref = {r: tr.forward(w, nhead, src, mask, r) for r in ("compute", "zero")}

    def close(got, want, what):
        err, bound = np.abs(got - want).max(), 2e-5 * max(1.0, np.abs(got).max())
        print(f"{name} {what}: max|err| = {err:.3e}, bound {bound:.3e}")
        assert err <= bound, (name, what, err, bound)

    close(rec["out_slow"], ref["compute"], "fast path off")
    rule = rec["rule_fast"]
    want = np.stack([ref["zero"][b] if rule[b] == 1 else ref["compute"][b] for b in range(len(rule))])
    close(rec["out_fast"], want, "fast path on")
    padded = mask.any(axis=1)
    assert ((rule == 2) == ~padded).all()
    if "mask_np" in rec:
        m = rec["mask_np"]
        assert m[0, 0] and not m[0, 1] and m[1].sum() == 1 and not m[1, 0] and not m[1, -1]       # not prefix masks
        close(rec["out_np"], tr.forward(w, nhead, src, m, "compute"), "non-prefix mask")
    if padded.any():
        gap = np.abs(ref["compute"] - ref["zero"])[padded].max(axis=1)
        assert gap.max() > 1.0 and gap.min() > 1e-3, gap                # O(1) apart; one padded position of 64 still shows
        assert np.abs(ref["compute"] - ref["zero"])[~padded].max() == 0.0
    # the stored errors are the ones measured against this helper
    assert abs(float(rec["err_slow"]) - np.abs(rec["out_slow"] - ref["compute"]).max()) < 1e-9


def test_helper_positions_are_the_modules_table():
    w, _, _ = load_record("cfg_like")
    pe = w["pos_encoder.pe"]
    assert np.abs(tr.sinusoid(pe.shape[0], pe.shape[1]) - pe).max() < 1e-6


# ------------------------------------------------------------------------------------------------ pack_tokens
def _pack_np(src, mask, rule):
    tok, pos, key, ptr = [], [], [], [0]
    for b in range(src.shape[0]):
        for t in range(src.shape[1]):
            if rule == "compute" or not mask[b, t]:
                tok.append(src[b, t]); pos.append(t); key.append(not mask[b, t])
        ptr.append(len(tok))
    return np.array(tok, np.int64), np.array(pos, np.int32), np.array(ptr, np.int32), np.array(key, np.uint8)


@pytest.mark.parametrize("rule", ["compute", "zero"])
def test_pack_tokens(rule):
    from sessionsimilaritysearch_amd.text import TokenRows, pack_tokens
    rng = np.random.default_rng(4)
    cases = []
    for T, lengths in ((20, [20, 1, 2, 5, 19]), (1, [1, 1]), (64, [64, 1, 63])):
        src = rng.integers(0, 30, (len(lengths), T))
        cases.append((src, tr.prefix_mask(lengths, T)))
    src = rng.integers(0, 30, (3, 9))
    holes = np.zeros((3, 9), dtype=bool)
    holes[0, 0] = holes[1, 4] = holes[1, 8] = holes[2, 1:] = True         # first token masked; a hole; only the first kept
    cases.append((src, holes))
    for src, mask in cases:
        for conv in (lambda a: a, torch.from_numpy):
            got = pack_tokens(conv(src), conv(mask), rule, ntoken=30)
            assert isinstance(got, TokenRows) and got.T == src.shape[1]
            for g, w in zip(got[:4], _pack_np(src, mask, rule)):
                assert g.dtype == w.dtype and np.array_equal(g, w)
        if rule == "zero":                                              # exactly the unmasked tokens and positions, in order
            assert np.array_equal(got.tok, src[~mask]) and np.array_equal(got.pos, np.nonzero(~mask)[1]) and got.key_ok.all()
        else:
            assert len(got.tok) == src.size and np.array_equal(got.key_ok, (~mask).reshape(-1))
    empty = pack_tokens(np.zeros((0, 20), np.int64), np.zeros((0, 20), bool), rule, ntoken=30)
    assert empty.ptr.tolist() == [0] and len(empty.tok) == len(empty.pos) == len(empty.key_ok) == 0 and empty.T == 20
    ok = np.zeros((2, 5), bool)
    with pytest.raises(ValueError):
        pack_tokens(np.zeros((1, 65), np.int64), np.zeros((1, 65), bool), rule)
    with pytest.raises(ValueError):
        pack_tokens(np.zeros((2, 5), np.int64), np.array([[0, 0, 1, 1, 1], [1, 1, 1, 1, 1]], bool), rule)
    with pytest.raises(ValueError):
        pack_tokens(np.zeros((2, 5), np.int64), ok, "mean")
    for bad in (-1, 30):
        src = np.zeros((2, 5), np.int64)
        src[1, 3] = bad
        with pytest.raises(IndexError):
            pack_tokens(src, ok, rule, ntoken=30)


def test_split_chunks_keeps_sequences_whole():
    from sessionsimilaritysearch_amd.text import split_chunks
    ptr = np.array([0, 20, 21, 23, 43, 63, 64], dtype=np.int32)
    assert split_chunks(ptr, 63) == [(0, 5), (5, 6)] and split_chunks(ptr, 23) == [(0, 3), (3, 4), (4, 6)]
    assert split_chunks(ptr, 1 << 20) == [(0, 6)] and split_chunks(np.array([0], np.int32), 64) == []
    for cap in (20, 21, 40, 64):
        ch = split_chunks(ptr, cap)
        assert ch[0][0] == 0 and ch[-1][1] == 6 and all(a[1] == b[0] for a, b in zip(ch, ch[1:]))
        assert all(ptr[s1] - ptr[s0] <= cap for s0, s1 in ch)


# ------------------------------------------------------------------------------------------------ text_fold_weights
@pytest.mark.parametrize("name", ["cfg_like", "t64", "full"])
def test_fold_weights_reproduces_the_unfolded_helper(name):
    """The helper on the folded weights (pad columns cut off, its own 1 / sqrt(D) dropped) equals the helper on the raw
    weights within float64 rounding; the padded columns, rows and biases are exact zeros."""
    from sessionsimilaritysearch_amd.text import text_fold_weights
    w, nhead, rec = load_record(name)
    wt = {k: torch.from_numpy(v) for k, v in w.items()}
    f = text_fold_weights(wt, nhead)
    e, nhid = w["embedding.weight"].shape[1], w["transformer_encoder.layers.0.linear1.weight"].shape[0]
    K, H = (e + 31) // 32 * 32, (nhid + 31) // 32 * 32
    assert (f["ninp"], f["nhead"], f["nhid"], f["nlayers"]) == (e, nhead, nhid, tr.n_layers(w))
    assert f["scale"] == float(np.float32(np.sqrt(np.float64(e)))) and f["pe"].shape == w["pos_encoder.pe"].shape
    folded = {"embedding.weight": f["table"].numpy(), "pos_encoder.pe": f["pe"].numpy()}
    for l, lay in enumerate(f["layers"]):
        assert all(v.dtype == torch.float64 for v in lay.values())
        assert lay["in_w"].shape == (3 * e, K) and lay["out_w"].shape == (e, K) and lay["l1_w"].shape == (H, K) and lay["l2_w"].shape == (e, H)
        for n in ("in_w", "out_w", "l1_w"):
            assert bool((lay[n][:, e:] == 0).all())
        assert bool((lay["l1_w"][nhid:] == 0).all()) and bool((lay["l1_b"][nhid:] == 0).all()) and bool((lay["l2_w"][:, nhid:] == 0).all())
        p = tr.LAYER.format(l)
        folded.update({p + "self_attn.in_proj_weight": lay["in_w"][:, :e].numpy(), p + "self_attn.in_proj_bias": lay["in_b"].numpy(),
                       p + "self_attn.out_proj.weight": lay["out_w"][:, :e].numpy(), p + "self_attn.out_proj.bias": lay["out_b"].numpy(),
                       p + "linear1.weight": lay["l1_w"][:nhid, :e].numpy(), p + "linear1.bias": lay["l1_b"][:nhid].numpy(),
                       p + "linear2.weight": lay["l2_w"][:, :nhid].numpy(), p + "linear2.bias": lay["l2_b"].numpy(),
                       p + "norm1.weight": lay["n1_w"].numpy(), p + "norm1.bias": lay["n1_b"].numpy(),
                       p + "norm2.weight": lay["n2_w"].numpy(), p + "norm2.bias": lay["n2_b"].numpy()})
    src = rec["src"]
    mask = rec["mask_np"]
    for rule in ("compute", "zero"):
        a = tr.forward(w, nhead, src, mask, rule)
        b = tr.forward(folded, nhead, src, mask, rule, attn_scale=False)
        assert np.abs(a - b).max() < 1e-12, (rule, np.abs(a - b).max())
    assert np.abs(tr.forward(folded, nhead, src, mask, "compute") - a).max() > 1e-6      # the fold is not a no-op
    with pytest.raises(ValueError):
        text_fold_weights(wt, 7)


def test_constructor_rejects_bad_arguments_before_any_device_work():
    """These raise while folding on the host: no device is needed (and none is present here)."""
    from sessionsimilaritysearch_amd.text import NodeTextTransformer
    w, nhead, _ = load_record("t64")
    wt = {k: torch.from_numpy(v) for k, v in w.items()}
    with pytest.raises(ValueError):
        NodeTextTransformer(wt, nhead, pad_rule="mean", device="cpu")
    with pytest.raises(ValueError):
        NodeTextTransformer(wt, 3, device="cpu")
    with pytest.raises(ValueError):
        NodeTextTransformer(wt, nhead, device="cpu", chunk_rows=10)


def test_package_exports_the_text_encoder():
    import sessionsimilaritysearch_amd as pkg
    from sessionsimilaritysearch_amd import text
    assert pkg.NodeTextTransformer is text.NodeTextTransformer and pkg.pack_tokens is text.pack_tokens
    assert pkg.text_fold_weights is text.text_fold_weights and pkg.TokenRows is text.TokenRows
    assert {"NodeTextTransformer", "pack_tokens", "text_fold_weights", "TokenRows"} <= set(pkg.__all__)


# ------------------------------------------------------------------------------------------------ the C ABI
def test_text_header_and_binding_declare_the_same_entry_points():
    names = declared("sss_text.h")
    assert names == _lib.symbols("sss_text.h") == ["sss_add_layernorm", "sss_seq_attention", "sss_text_embed"]
    L = _lib.lib()
    for n in names:
        assert getattr(L, n).argtypes == _lib.HEADERS["sss_text.h"][n][1] and getattr(L, n).restype is ctypes.c_int
    for header, table in _lib.HEADERS.items():
        if header != "sss_text.h":
            assert not set(names) & set(table) and not set(names) & set(declared(header)), header
    assert declared("sss.h") == _lib.exported_symbols() and len(_lib.exported_symbols()) == 60
    text = open(os.path.join(ROOT, "include", "sss_text.h")).read()
    for phrase in ("CALLER-OWNED DEVICE", "nothing is allocated", "no host synchronisation", "enqueued on `stream`",
                   "-1 bad argument", "-3 HIP error"):
        assert phrase in text, phrase
    # the struct mirrors the header field for field (names in order); the scalar argument lists have the header's arity
    plain = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    body = re.search(r"typedef struct \{([^}]*)\} sss_seq_attention_args;", plain, re.S).group(1)
    assert re.findall(r"(\w+)\s*;", body) == [n for n, _ in _lib.SeqAttentionArgs._fields_]
    for n in names:
        params = re.search(r"\b" + n + r"\s*\(([^)]*)\)", plain, re.S).group(1)
        assert len(params.split(",")) == len(_lib.HEADERS["sss_text.h"][n][1]), n


_P = 1 << 20                                                          # a non-null, 16-byte aligned address; never dereferenced


def _embed(L, **kw):
    a = dict(table=_P, n_token=50, pe=_P, n_pos=64, tok=_P, pos=_P, n=7, e=200, scale=2.0, x=_P, ld_x=224, err=_P, st=0)
    a.update(kw)
    return L.sss_text_embed(*a.values())


def _attention(L, **kw):
    a = dict(qkv=_P, ld_qkv=600, ptr=_P, key_ok=_P, n_rows=40, n_seq=2, heads=4, head_dim=50, max_len=20, out=_P, ld_out=224)
    a.update(kw)
    return L.sss_seq_attention(ctypes.byref(_lib.SeqAttentionArgs(**a)), 0)


def _layernorm(L, **kw):
    a = dict(x=_P, ld_x=224, res=_P + 4096, ld_res=200, gamma=_P, beta=_P, eps=1e-5, n=7, e=200, y=_P, ld_y=224, st=0)
    a.update(kw)
    return L.sss_add_layernorm(*a.values())


def test_argument_checks_return_before_any_device_work():
    """No address given here is memory: a call that launched would fault."""
    L = _lib.lib()
    for kw in (dict(e=0), dict(e=6), dict(e=1028), dict(ld_x=196), dict(ld_x=226), dict(n_token=0), dict(n_pos=0), dict(n=-1),
               dict(n=1 << 31), dict(table=0), dict(pe=0), dict(x=0), dict(x=_P + 4), dict(tok=0), dict(pos=0), dict(err=0)):
        assert _embed(L, **kw) == -1 and L.sss_last_error().startswith(b"text_embed:"), kw
    assert _embed(L, n=0) == 0 and _embed(L, n=0, table=0, pe=0, tok=0, pos=0, x=0, err=0) == 0
    assert _embed(L, n=0, e=6) == -1 and _embed(L, n=0, n_pos=0) == -1     # an empty batch's scalars are still checked

    for kw in (dict(head_dim=0), dict(head_dim=65, heads=4, ld_qkv=4096, ld_out=4096), dict(heads=0), dict(heads=17, head_dim=64, ld_qkv=4096, ld_out=4096),
               dict(heads=1025, head_dim=1, ld_qkv=4096, ld_out=4096), dict(max_len=0), dict(max_len=65), dict(n_seq=-1), dict(n_seq=1 << 31), dict(n_rows=-1),
               dict(n_rows=1 << 31), dict(ld_qkv=599), dict(ld_out=199), dict(qkv=0), dict(out=0), dict(ptr=0), dict(key_ok=0),
               dict(qkv=_P + 2)):
        assert _attention(L, **kw) == -1 and L.sss_last_error().startswith(b"seq_attention:"), kw
    assert L.sss_seq_attention(None, 0) == -1 and L.sss_last_error().startswith(b"seq_attention:")
    assert _attention(L, n_seq=0) == 0 and _attention(L, n_rows=0) == 0
    assert _attention(L, n_seq=0, qkv=0, out=0, ptr=0, key_ok=0) == 0
    assert _attention(L, n_seq=0, head_dim=65) == -1 and _attention(L, n_seq=0, max_len=65) == -1

    for kw in (dict(e=0), dict(e=6), dict(e=1028), dict(ld_x=196), dict(ld_res=198), dict(ld_y=222), dict(ld_y=196), dict(eps=0.0),
               dict(eps=-1.0), dict(n=-1), dict(n=1 << 31), dict(x=0), dict(res=0), dict(gamma=0), dict(beta=_P + 8), dict(y=0),
               dict(ld_y=448)):                                         # the last: in place needs the same leading dimension
        assert _layernorm(L, **kw) == -1 and L.sss_last_error().startswith(b"add_layernorm:"), kw
    assert _layernorm(L, n=0) == 0 and _layernorm(L, n=0, x=0, res=0, gamma=0, beta=0, y=0) == 0
    assert _layernorm(L, n=0, e=6) == -1 and _layernorm(L, n=0, eps=0.0) == -1
