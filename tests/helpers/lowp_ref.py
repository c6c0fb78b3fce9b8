"""float64 restatements of the two text encoders with bfloat16 rounding at the GEMM inputs: bert_ref.token_states and
text_ref.token_states with BOTH operands of every dense layer (query, key, value, attention output, the two feed-forward
layers; the optional lin head in `bert_head`) rounded to bfloat16 with torch's ``.bfloat16()`` (round to nearest even)
before an exact float64 product.  Everything else -- embeddings, softmax, LayerNorm, residuals, activations, biases -- is
the float64 arithmetic of the two helpers this one imports.

These are NOT oracles of text.py under gemm="bf16": float32 noise on the device flips bf16 roundings, so no pointwise
bound against them holds.  They measure how far bfloat16 GEMM inputs move a forward from the
full-precision reference at a given shape: ``dev_lowp = max |restatement - reference|``, the scale the device's own
deviation is held to."""
import math

import numpy as np
import torch

import bert_ref as br
import text_ref as tr


def bf16(a):
    """`a` (numpy or torch, any float dtype) rounded to float32 and then to bfloat16, as a float64 torch tensor."""
    return torch.as_tensor(np.asarray(a)).float().bfloat16().double()


def linear(x, w, b):
    """bf16(x) bf16(w)^T + b in float64: products of two bf16 values are exact, the sum is float64."""
    return bf16(x) @ bf16(w).T + b


def bert_token_states(w, heads, input_ids, token_type_ids, attention_mask, eps=1e-12):
    """bert_ref.token_states in float64 with `linear` at the six GEMMs of every layer: [B, T, e] numpy float64."""
    t = lambda name: torch.as_tensor(np.asarray(w[name].detach().cpu() if hasattr(w[name], "detach") else w[name])).double()
    ids, tt = torch.as_tensor(np.asarray(input_ids)).long(), torch.as_tensor(np.asarray(token_type_ids)).long()
    key = torch.as_tensor(np.asarray(attention_mask)) != 0
    B, T = ids.shape
    word = t("embeddings.word_embeddings.weight")
    e = word.shape[1]
    D = e // heads
    x = (word[ids] + t("embeddings.token_type_embeddings.weight")[tt]) + t("embeddings.position_embeddings.weight")[:T][None]
    x = br.layer_norm(x, t("embeddings.LayerNorm.weight"), t("embeddings.LayerNorm.bias"), eps)
    neg = torch.zeros((B, 1, 1, T), dtype=torch.float64).masked_fill(~key[:, None, None, :], float("-inf"))
    for l in range(br.n_layers(w)):
        g = lambda n: t(br.LAYER.format(l) + n)
        lin = lambda y, n: linear(y, g(n + ".weight"), g(n + ".bias"))
        split = lambda y: y.reshape(B, T, heads, D).permute(0, 2, 1, 3)
        q, k, v = (split(lin(x, "attention.self." + n)) for n in ("query", "key", "value"))
        p = torch.softmax(q @ k.transpose(-1, -2) / math.sqrt(D) + neg, dim=-1)
        a = lin((p @ v).permute(0, 2, 1, 3).reshape(B, T, e), "attention.output.dense")
        x = br.layer_norm(x + a, g("attention.output.LayerNorm.weight"), g("attention.output.LayerNorm.bias"), eps)
        h = lin(br.gelu(lin(x, "intermediate.dense")), "output.dense")
        x = br.layer_norm(x + h, g("output.LayerNorm.weight"), g("output.LayerNorm.bias"), eps)
    return x.numpy()


def bert_head(w, states, attention_mask, how):
    """bert_ref.head in float64, the optional lin head through `linear` (under gemm="bf16" it is a bf16 GEMM as well)."""
    out = br.pool(states, attention_mask, how)
    if "lin.weight" in w:
        f = lambda a: torch.as_tensor(np.asarray(a.detach().cpu() if hasattr(a, "detach") else a)).double()
        out = linear(out, f(w["lin.weight"]), f(w["lin.bias"])).numpy()
    return out


def text_token_states(w, nhead, src, mask, eps=1e-5):
    """text_ref.token_states in float64 with `linear` at in_proj, out_proj, linear1 and linear2 of every layer."""
    src, mask = np.asarray(src), np.asarray(mask, dtype=bool)
    B, T = src.shape
    table = tr.f64(w["embedding.weight"])
    e = table.shape[1]
    D = e // nhead
    pe = tr.f64(w["pos_encoder.pe"]).reshape(-1, e)
    x = table[src] * math.sqrt(e) + pe[:T][None]
    for l in range(tr.n_layers(w)):
        g = lambda n: tr.f64(w[tr.LAYER.format(l) + n])
        lin = lambda y, wn, bn: linear(y, g(wn), torch.from_numpy(g(bn))).numpy()
        qkv = lin(x, "self_attn.in_proj_weight", "self_attn.in_proj_bias")
        q, k, v = (qkv[..., i * e:(i + 1) * e].reshape(B, T, nhead, D) for i in range(3))
        s = np.einsum("bihd,bjhd->bhij", q, k) / math.sqrt(D)
        s = np.where(mask[:, None, None, :], -np.inf, s)
        p = np.exp(s - s.max(-1, keepdims=True))
        p = p / p.sum(-1, keepdims=True)
        a = lin(np.einsum("bhij,bjhd->bihd", p, v).reshape(B, T, e), "self_attn.out_proj.weight", "self_attn.out_proj.bias")
        x = tr.layer_norm(x + a, g("norm1.weight"), g("norm1.bias"), eps)
        h = np.maximum(lin(x, "linear1.weight", "linear1.bias"), 0.0)
        h = lin(h, "linear2.weight", "linear2.bias")
        x = tr.layer_norm(x + h, g("norm2.weight"), g("norm2.bias"), eps)
    return x


def text_forward(w, nhead, src, mask, rule, **kw):
    """text_ref.forward on `text_token_states`."""
    x = text_token_states(w, nhead, src, mask, **kw)
    if rule == "zero":
        x = np.where(np.asarray(mask, dtype=bool)[:, :, None], 0.0, x)
    elif rule != "compute":
        raise ValueError(rule)
    return x.sum(1) / x.shape[1]
