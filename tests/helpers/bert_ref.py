"""Dense restatement, in plain torch on the CPU, of a BERT encoder without its pooling layer (BertModel(config,
add_pooling_layer=False): three embedding tables summed + LayerNorm, post-norm layers of softmax attention under an
additive -inf key mask and an erf-GELU feed-forward block) and of the two poolings the reference puts on it
(model/NodeEmbedding.py:114 the masked mean, test_amazon_filterd.py main2('QAEA') the plain mean), on the PADDED [B, T]
layout with [B, heads, T, T] scores.

Written independently of the packed route (it imports neither the package's text.py nor oracle/).  Every function takes a
dtype: torch.float64 is the reference, torch.float32 the yardstick of what float32 arithmetic costs at a shape.  Weights
are a {name: array or tensor} dict under HF's state_dict() names, optionally with lin.weight / lin.bias."""
import math

import numpy as np
import torch

LAYER = "encoder.layer.{}."


def n_layers(w):
    n = 0
    while LAYER.format(n) + "attention.self.query.weight" in w:
        n += 1
    return n


def layer_norm(x, g, b, eps):
    mu = x.mean(-1, keepdim=True)
    var = ((x - mu) ** 2).mean(-1, keepdim=True)
    return (x - mu) / torch.sqrt(var + eps) * g + b


def gelu(x):
    return 0.5 * x * (1.0 + torch.erf(x / math.sqrt(2.0)))


def token_states(w, heads, input_ids, token_type_ids, attention_mask, eps=1e-12, dtype=torch.float64):
    """last_hidden_state [B, T, e] as a numpy array of `dtype`: every position computed, masked keys left out of every softmax."""
    t = lambda name: torch.as_tensor(np.asarray(w[name].detach().cpu() if hasattr(w[name], "detach") else w[name])).to(dtype)
    ids, tt = torch.as_tensor(np.asarray(input_ids)).long(), torch.as_tensor(np.asarray(token_type_ids)).long()
    key = torch.as_tensor(np.asarray(attention_mask)) != 0
    B, T = ids.shape
    word = t("embeddings.word_embeddings.weight")
    e = word.shape[1]
    D = e // heads
    x = (word[ids] + t("embeddings.token_type_embeddings.weight")[tt]) + t("embeddings.position_embeddings.weight")[:T][None]
    x = layer_norm(x, t("embeddings.LayerNorm.weight"), t("embeddings.LayerNorm.bias"), eps)
    neg = torch.zeros((B, 1, 1, T), dtype=dtype).masked_fill(~key[:, None, None, :], float("-inf"))
    for l in range(n_layers(w)):
        g = lambda n: t(LAYER.format(l) + n)
        split = lambda y: y.reshape(B, T, heads, D).permute(0, 2, 1, 3)
        q = split(x @ g("attention.self.query.weight").T + g("attention.self.query.bias"))
        k = split(x @ g("attention.self.key.weight").T + g("attention.self.key.bias"))
        v = split(x @ g("attention.self.value.weight").T + g("attention.self.value.bias"))
        s = q @ k.transpose(-1, -2) / math.sqrt(D) + neg
        p = torch.softmax(s, dim=-1)
        a = (p @ v).permute(0, 2, 1, 3).reshape(B, T, e)
        a = a @ g("attention.output.dense.weight").T + g("attention.output.dense.bias")
        x = layer_norm(x + a, g("attention.output.LayerNorm.weight"), g("attention.output.LayerNorm.bias"), eps)
        h = gelu(x @ g("intermediate.dense.weight").T + g("intermediate.dense.bias"))
        h = h @ g("output.dense.weight").T + g("output.dense.bias")
        x = layer_norm(x + h, g("output.LayerNorm.weight"), g("output.LayerNorm.bias"), eps)
    return x.numpy()


def pool(states, attention_mask, how):
    """"masked": sum(states * mask) / sum(mask) (the reference's own line); "mean": states.mean(1)."""
    if how == "mean":
        return states.mean(1)
    if how != "masked":
        raise ValueError(how)
    m = (np.asarray(attention_mask) != 0).astype(states.dtype)
    return (states * m[:, :, None]).sum(1) / m.sum(1)[:, None]


def head(w, states, attention_mask, how):
    """[B, e], or [B, nout] when w holds lin.weight: the pooled states through the optional Linear, in the states' dtype."""
    out = pool(states, attention_mask, how)
    if "lin.weight" in w:
        f = lambda a: np.asarray(a.detach().cpu() if hasattr(a, "detach") else a).astype(out.dtype)
        out = out @ f(w["lin.weight"]).T + f(w["lin.bias"])
    return out


def forward(w, heads, input_ids, token_type_ids, attention_mask, how="masked", eps=1e-12, dtype=torch.float64):
    """The encoder's output: head() of token_states()."""
    return head(w, token_states(w, heads, input_ids, token_type_ids, attention_mask, eps, dtype), attention_mask, how)


def seeded_weights(seed, vocab, e, heads, inter, nlayers, n_pos, n_type=2, nout=None):
    """A float32 weight dict under HF's names from a seed: N(0, 1/sqrt(fan_in)) matrices (in_proj x 2, so that the softmax is
    not flat), N(0, 0.3) biases, LayerNorm weights 1 + N(0, 0.2), tables N(0, 1)."""
    g = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=g)
    w = {"embeddings.word_embeddings.weight": rn(vocab, e), "embeddings.position_embeddings.weight": rn(n_pos, e) * 0.5,
         "embeddings.token_type_embeddings.weight": rn(n_type, e) * 0.5,
         "embeddings.LayerNorm.weight": 1 + 0.2 * rn(e), "embeddings.LayerNorm.bias": 0.3 * rn(e)}
    for l in range(nlayers):
        p = LAYER.format(l)
        for name, m, k, scale in (("attention.self.query", e, e, 2.0), ("attention.self.key", e, e, 2.0), ("attention.self.value", e, e, 1.0),
                                  ("attention.output.dense", e, e, 1.0), ("intermediate.dense", inter, e, 1.0), ("output.dense", e, inter, 1.0)):
            w[p + name + ".weight"], w[p + name + ".bias"] = rn(m, k) * (scale / math.sqrt(k)), 0.3 * rn(m)
        for name in ("attention.output.LayerNorm", "output.LayerNorm"):
            w[p + name + ".weight"], w[p + name + ".bias"] = 1 + 0.2 * rn(e), 0.3 * rn(e)
    if nout is not None:
        w["lin.weight"], w["lin.bias"] = rn(nout, e) / math.sqrt(e), 0.3 * rn(nout)
    return w
