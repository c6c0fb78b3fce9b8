"""numpy float64 restatement of the reference's NodeTextTransformer in eval mode (model/NodeEmbedding.py:62-98:
embedding * sqrt(ninp) + sinusoidal positions, post-norm TransformerEncoderLayers with relu and a key-padding mask, an
unmasked mean over the T positions) on the PADDED [B, T] layout, under both padding rules:

  "compute"  a padded position is an ordinary row (it attends over the valid keys, is never a key itself) and is averaged in
  "zero"     padded positions come back as zeros: sum over the real tokens / T

Written independently of the packed route (it imports neither the package's text.py nor oracle/): dense [B, T, T] scores
with -inf at masked keys.  Weights are a {name: array} dict under the module's state_dict() names; `pos_encoder.pe` may
be the module's [1, max_len, ninp] buffer or any [n_pos >= T, ninp] prefix of it."""
import math

import numpy as np

LAYER = "transformer_encoder.layers.{}."


def f64(a):
    if hasattr(a, "detach"):
        a = a.detach().cpu().numpy()
    return np.asarray(a, dtype=np.float64)


def sinusoid(n_pos, e):
    """PositionalEncoding.__init__'s table in float64 (the module builds it in float32)."""
    pos = np.arange(n_pos, dtype=np.float64)[:, None]
    div = np.exp(np.arange(0, e, 2, dtype=np.float64) * (-math.log(10000.0) / e))
    pe = np.zeros((n_pos, e))
    pe[:, 0::2], pe[:, 1::2] = np.sin(pos * div), np.cos(pos * div)
    return pe


def layer_norm(x, g, b, eps):
    mu = x.mean(-1, keepdims=True)
    var = ((x - mu) ** 2).mean(-1, keepdims=True)
    return (x - mu) / np.sqrt(var + eps) * g + b


def n_layers(w):
    n = 0
    while LAYER.format(n) + "self_attn.in_proj_weight" in w:
        n += 1
    return n


def token_states(w, nhead, src, mask, eps=1e-5, attn_scale=True, embed_scale=None):
    """[B, T, ninp] after the last layer, every position computed (masked keys excluded from every softmax)."""
    src, mask = np.asarray(src), np.asarray(mask, dtype=bool)
    B, T = src.shape
    table = f64(w["embedding.weight"])
    e = table.shape[1]
    D = e // nhead
    pe = f64(w["pos_encoder.pe"]).reshape(-1, e)
    x = table[src] * (math.sqrt(e) if embed_scale is None else embed_scale) + pe[:T][None]
    for l in range(n_layers(w)):
        g = lambda n: f64(w[LAYER.format(l) + n])
        qkv = x @ g("self_attn.in_proj_weight").T + g("self_attn.in_proj_bias")
        q, k, v = (qkv[..., i * e:(i + 1) * e].reshape(B, T, nhead, D) for i in range(3))
        s = np.einsum("bihd,bjhd->bhij", q, k)
        if attn_scale:
            s = s / math.sqrt(D)
        s = np.where(mask[:, None, None, :], -np.inf, s)
        s = s - s.max(-1, keepdims=True)
        p = np.exp(s)
        p = p / p.sum(-1, keepdims=True)
        a = np.einsum("bhij,bjhd->bihd", p, v).reshape(B, T, e)
        a = a @ g("self_attn.out_proj.weight").T + g("self_attn.out_proj.bias")
        x = layer_norm(x + a, g("norm1.weight"), g("norm1.bias"), eps)
        h = np.maximum(x @ g("linear1.weight").T + g("linear1.bias"), 0.0)
        h = h @ g("linear2.weight").T + g("linear2.bias")
        x = layer_norm(x + h, g("norm2.weight"), g("norm2.bias"), eps)
    return x


def forward(w, nhead, src, mask, rule, **kw):
    """[B, ninp]: the module's output under `rule`."""
    x = token_states(w, nhead, src, mask, **kw)
    mask = np.asarray(mask, dtype=bool)
    if rule == "zero":
        x = np.where(mask[:, :, None], 0.0, x)
    elif rule != "compute":
        raise ValueError(rule)
    return x.sum(1) / x.shape[1]


def prefix_mask(lengths, T):
    return np.arange(T)[None, :] >= np.asarray(lengths)[:, None]
