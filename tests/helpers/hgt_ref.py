"""Two restatements of the reference's HGT (model/gnn.py:9-41 over PyG 2.0.4's HGTConv, group='sum') that share no code
(PyG is not installed, so the parity is unpinned: the formulas are DESIGN.md section 5.8):

* ``hgt_torch``  vectorised torch, any dtype, in HGTConv's operation order and UNFOLDED (k_lin then a_rel, the score
                 times p_rel and then over sqrt(D), scatter softmax, a_lin then the skip blend);
* ``hgt_loops``  plain numpy float64 with explicit loops over edges and heads, written from the formulas.

Edges are ``{"qp" | "pq" | "pp": int64 [2, E]}`` (row 0 sources, row 1 targets), weights the flat dict of ``variants.HGT``."""
import math

import numpy as np
import torch

EDGES = (("qp", "query", "product"), ("pq", "product", "query"), ("pp", "product", "product"))
TYPES = ("query", "product")


def make_weights(g, d_q, d_p, h, heads, n_layers):
    """Seeded float32 weights, every matrix scaled 1 / sqrt(fan_in) so activations and logits stay O(1)."""
    u = lambda *shape, scale=1.0: (torch.rand(shape, generator=g) * 2 - 1) * scale
    D = h // heads
    w = {}
    for t, d in (("query", d_q), ("product", d_p)):
        w[f"hgt.lin.{t}.w"], w[f"hgt.lin.{t}.b"] = u(h, d, scale=1 / math.sqrt(d)), u(h, scale=0.1)
    for l in range(n_layers):
        for t in TYPES:
            for n in "kqva":
                w[f"hgt.{l}.{t}.{n}.w"], w[f"hgt.{l}.{t}.{n}.b"] = u(h, h, scale=1 / math.sqrt(h)), u(h, scale=0.1)
            w[f"hgt.{l}.{t}.skip"] = u(1, scale=2.0)
        for e, _, _ in EDGES:
            w[f"hgt.{l}.{e}.a_rel"] = u(heads, D, D, scale=1 / math.sqrt(D))
            w[f"hgt.{l}.{e}.m_rel"] = u(heads, D, D, scale=1 / math.sqrt(D))
            w[f"hgt.{l}.{e}.p_rel"] = u(heads) * 0.5 + 1.0
    return w


def csr_by_target(ei, n_dst):
    """COO [2, E] -> (rowptr int32 [n_dst + 1], col int32 [E]): edges grouped by target, in their COO order."""
    ei = np.asarray(ei, dtype=np.int64).reshape(2, -1)
    order = np.argsort(ei[1], kind="stable")
    rowptr = np.zeros(n_dst + 1, dtype=np.int64)
    np.add.at(rowptr, ei[1] + 1, 1)
    return np.cumsum(rowptr).astype(np.int32), ei[0][order].astype(np.int32)


# ------------------------------------------------------------------------------------------------ vectorised torch
def _scatter_softmax(alpha, index, n):
    """PyG's softmax(src, index): exp(src - max) / (sum exp(src - max) + 1e-16) per target and column."""
    idx = index[:, None].expand_as(alpha)
    mx = torch.full((n, alpha.shape[1]), float("-inf"), dtype=alpha.dtype).scatter_reduce(0, idx, alpha, "amax", include_self=True)
    ex = (alpha - mx[index]).exp()
    den = torch.zeros((n, alpha.shape[1]), dtype=alpha.dtype).index_add_(0, index, ex)
    return ex / (den[index] + 1e-16)


def hgt_conv_torch(x, edges, w, l, heads, parts=None):
    """One HGTConv layer on ``x = {type: [N, h]}``.  ``parts`` (a dict) receives the intermediates a folding test needs:
    ``k.e`` / ``v.e`` [N_src, H, D], ``alpha.e`` [E, H] before the softmax, ``agg.t`` [N, h] before gelu."""
    dt = next(iter(x.values())).dtype
    g = lambda n: w[n].to(dt)
    h = x["query"].shape[1]
    D = h // heads
    lin = lambda t, n: (x[t] @ g(f"hgt.{l}.{t}.{n}.w").T + g(f"hgt.{l}.{t}.{n}.b")).view(-1, heads, D)
    k, q, v = ({t: lin(t, n) for t in TYPES} for n in "kqv")
    outs = {t: [] for t in TYPES}
    for e, s, t in EDGES:
        ke = (k[s].transpose(0, 1) @ g(f"hgt.{l}.{e}.a_rel")).transpose(1, 0)
        ve = (v[s].transpose(0, 1) @ g(f"hgt.{l}.{e}.m_rel")).transpose(1, 0)
        src, dst = torch.as_tensor(edges[e][0]).long(), torch.as_tensor(edges[e][1]).long()
        alpha = (q[t][dst] * ke[src]).sum(-1) * g(f"hgt.{l}.{e}.p_rel")
        alpha = alpha / math.sqrt(D)
        sm = _scatter_softmax(alpha, dst, x[t].shape[0])
        msg = (ve[src] * sm.view(-1, heads, 1)).reshape(-1, h)
        outs[t].append(torch.zeros((x[t].shape[0], h), dtype=dt).index_add_(0, dst, msg))
        if parts is not None:
            parts[f"k.{e}"], parts[f"v.{e}"], parts[f"alpha.{e}"] = ke, ve, alpha
    new = {}
    for t in TYPES:
        agg = torch.stack(outs[t], 0).sum(0)
        if parts is not None:
            parts[f"agg.{t}"] = agg
        y = torch.nn.functional.gelu(agg) @ g(f"hgt.{l}.{t}.a.w").T + g(f"hgt.{l}.{t}.a.b")
        sig = g(f"hgt.{l}.{t}.skip").reshape(()).sigmoid()
        new[t] = sig * y + (1 - sig) * x[t]
    return new


def hgt_torch(x_q, x_p, edges, w, heads, n_layers, dtype=torch.float64):
    x = {"query": x_q.to(dtype), "product": x_p.to(dtype)}
    cur = {t: torch.relu(x[t] @ w[f"hgt.lin.{t}.w"].to(dtype).T + w[f"hgt.lin.{t}.b"].to(dtype)) for t in TYPES}
    outs = [cur]
    for l in range(n_layers):
        outs.append(hgt_conv_torch(outs[-1], edges, w, l, heads))
    return {t: torch.cat([o[t] for o in outs], 1) for t in TYPES}


# ------------------------------------------------------------------------------------------------ numpy loops, float64
def _gelu(a):
    return 0.5 * a * (1.0 + np.vectorize(math.erf, otypes=[np.float64])(a / math.sqrt(2.0)))


def attention_loops(q, slots, heads, gelu):
    """What sss_hgt_aggregate computes, in float64: q [n_dst, H D]; slots = [(k, v, rowptr, col)] with k already scaled
    (plain dot products).  Per target, slot and head: softmax over the slot's incoming edges, weighted sum of v."""
    q = np.asarray(q, dtype=np.float64)
    n, width = q.shape
    D = width // heads
    out = np.zeros((n, width))
    for k, v, rowptr, col in slots:
        k, v = np.asarray(k, dtype=np.float64), np.asarray(v, dtype=np.float64)
        for i in range(n):
            js = [int(col[e]) for e in range(int(rowptr[i]), int(rowptr[i + 1]))]
            if not js:
                continue
            for eta in range(heads):
                c = slice(eta * D, (eta + 1) * D)
                a = [float(np.dot(q[i, c], k[j, c])) for j in js]
                m = max(a)
                ex = [math.exp(x - m) for x in a]
                den = sum(ex) + 1e-16
                for x, j in zip(ex, js):
                    out[i, c] += (x / den) * v[j, c]
    return _gelu(out) if gelu else out


def hgt_loops(x_q, x_p, edges, w, heads, n_layers):
    f = lambda n: w[n].detach().cpu().numpy().astype(np.float64)
    x = {"query": np.asarray(x_q, dtype=np.float64), "product": np.asarray(x_p, dtype=np.float64)}
    cur = {t: np.maximum(x[t] @ f(f"hgt.lin.{t}.w").T + f(f"hgt.lin.{t}.b"), 0.0) for t in TYPES}
    outs = [cur]
    h = cur["query"].shape[1]
    D = h // heads
    for l in range(n_layers):
        x = outs[-1]
        K, Q, V = ({t: x[t] @ f(f"hgt.{l}.{t}.{n}.w").T + f(f"hgt.{l}.{t}.{n}.b") for t in TYPES} for n in "kqv")
        agg = {t: np.zeros_like(x[t]) for t in TYPES}
        for e, s, t in EDGES:
            a_rel, m_rel, p_rel = f(f"hgt.{l}.{e}.a_rel"), f(f"hgt.{l}.{e}.m_rel"), f(f"hgt.{l}.{e}.p_rel")
            ke, ve = np.zeros_like(K[s]), np.zeros_like(V[s])
            for eta in range(heads):
                c = slice(eta * D, (eta + 1) * D)
                for n in range(K[s].shape[0]):
                    ke[n, c] = K[s][n, c] @ a_rel[eta]
                    ve[n, c] = V[s][n, c] @ m_rel[eta]
            incoming = [[] for _ in range(x[t].shape[0])]
            for j, i in zip(np.asarray(edges[e][0]).tolist(), np.asarray(edges[e][1]).tolist()):
                incoming[i].append(j)
            for i, js in enumerate(incoming):
                for eta in range(heads if js else 0):
                    c = slice(eta * D, (eta + 1) * D)
                    a = [float(np.dot(Q[t][i, c], ke[j, c])) * p_rel[eta] / math.sqrt(D) for j in js]
                    m = max(a)
                    ex = [math.exp(v - m) for v in a]
                    den = sum(ex) + 1e-16
                    for v, j in zip(ex, js):
                        agg[t][i, c] += (v / den) * ve[j, c]
        new = {}
        for t in TYPES:
            y = _gelu(agg[t]) @ f(f"hgt.{l}.{t}.a.w").T + f(f"hgt.{l}.{t}.a.b")
            sig = 1.0 / (1.0 + math.exp(-float(f(f"hgt.{l}.{t}.skip").reshape(-1)[0])))
            new[t] = sig * y + (1.0 - sig) * x[t]
        outs.append(new)
    return {t: np.concatenate([o[t] for o in outs], 1) for t in TYPES}
