"""Per-kernel restatements of the encoder entry points of ``include/sss.h`` and the hand-built edge
cases the kernels are tested on.  TEST INFRASTRUCTURE ONLY (see ``oracle/__init__.py``).

Every function takes the arrays its entry point takes (CSR by target, ``row_p`` / ``row_q``,
``pptr`` / ``qptr``, ``src_row``, ``pos_id``) as CPU torch tensors / numpy index arrays and works in
the dtype of its float inputs: float64 is the reference, the SAME code on float32 inputs is the
"float32 restatement" whose distance from the float64 one is the error yardstick of
``tests/test_encoder_kernels_edges_gpu.py``.  One target / one graph at a time, vectorised over its
edges / rows; sums over edges / rows are accumulated left to right, one row after the other (`seq_sum`), as a plain loop
does -- not with torch's blocked reduction, whose float32 error would understate that of any loop.  The softmax is the textbook three-pass one (maximum, exponentials, weighted sum)
with PyG's ``+ 1e-16``; ``sigmoid`` never exponentiates a positive number, so it cannot overflow.
Written from ``include/sss.h`` and SURVEY.md Appendix A.2-A.4.

``tests/test_encoder_kernels_ref_cpu.py`` chains these restatements into a whole encoder forward
and requires ``oracle/gnn_ref64.py`` (which shares no code with this file) to agree to float64
round-off; it also runs ``check_layer_case`` / ``check_pool_case`` on every generated case.
"""
from __future__ import annotations

from types import SimpleNamespace

import numpy as np
import torch


# ------------------------------------------------------------------------------------------ GAT / GGC / GRU
def sigmoid(v):
    """1 / (1 + exp(-v)) with only non-positive arguments to exp."""
    e = torch.exp(-v.abs())
    return torch.where(v >= 0, 1 / (1 + e), e / (1 + e))


def seq_sum(v):
    """sum over dim 0, accumulated row after row in the dtype of v."""
    acc = torch.zeros(v.shape[1:], dtype=v.dtype)
    for r in v:
        acc = acc + r
    return acc


def incoming(rowptr, col, i, n_self_loop):
    """Source ids of target i after the n_self_loop rewrite of sss_gat_aggregate: edges with source == target
    dropped, one edge i -> i appended for i < n_self_loop; n_self_loop == 0: the CSR row as it is."""
    js = [int(j) for j in col[rowptr[i]:rowptr[i + 1]]]
    if n_self_loop:
        js = [j for j in js if j != i] + ([i] if i < n_self_loop else [])
    return js


def gat_ref(xs, a_src, a_dst, rowptr, col, n_dst, bias, n_self_loop):
    """sss_gat_aggregate (relu = 0): per target softmax over leaky_relu(a_src[j] + a_dst[i], 0.2), weighted sum of
    xs[j], + bias; a target without incoming edges gets bias."""
    out = torch.zeros((n_dst, xs.shape[1]), dtype=xs.dtype)
    for i in range(n_dst):
        js = incoming(rowptr, col, i, n_self_loop)
        if js:
            e = torch.nn.functional.leaky_relu(a_src[js] + a_dst[i], 0.2)
            w = torch.exp(e - e.max())
            w = w / (seq_sum(w) + 1e-16)
            out[i] = seq_sum(w[:, None] * xs[js])
    return out + bias


def csr_weighted_sum_ref(m, rowptr, col, w, n_dst):
    """sss_csr_weighted_sum: out[i] = sum_{e in row i} (w[e] if w is not None else 1) * m[col[e]]."""
    out = torch.zeros((n_dst, m.shape[1]), dtype=m.dtype)
    for i in range(n_dst):
        e0, e1 = int(rowptr[i]), int(rowptr[i + 1])
        if e1 > e0:
            rows = m[torch.as_tensor(np.asarray(col[e0:e1]), dtype=torch.int64)]
            out[i] = seq_sum(rows if w is None else w[e0:e1, None] * rows)
    return out


def gru_gates(gi, gh):
    h = gh.shape[1] // 3
    r = sigmoid(gi[:, :h] + gh[:, :h])
    z = sigmoid(gi[:, h:2 * h] + gh[:, h:2 * h])
    n = torch.tanh(gi[:, 2 * h:] + r * gh[:, 2 * h:])
    return r, z, n


def gru_ref(gi, gh, x, add):
    """sss_gru_combine: relu(add + (1 - z) n + z x), x zero-padded from d_x to h columns, add may be None."""
    h = gh.shape[1] // 3
    _, z, n = gru_gates(gi, gh)
    xp = torch.zeros((x.shape[0], h), dtype=gi.dtype)
    xp[:, :x.shape[1]] = x
    return torch.relu((0 if add is None else add) + (1 - z) * n + z * xp)


def layer_update_ref(c, dtype=torch.float64):
    """sss_hetero_layer_update on a layer case `c` (see `layer_case`): (out_p, out_q, x0_p, x0_q); x0_* are the raw
    feature rows the table mode also copies out (float32, exact)."""
    h = c.h
    rp = torch.arange(c.n_p) if c.row_p is None else c.row_p
    rq = torch.arange(c.n_q) if c.row_q is None else c.row_q
    Yp, Yq, X = c.yp.to(dtype)[rp], c.yq.to(dtype)[rq], c.xin.to(dtype)[rp]
    f = lambda t: None if t is None else t.to(dtype)
    gat_p = gat_ref(Yq[:, :h], Yq[:, h], Yp[:, 7 * h + 1], c.rp_qp, c.c_qp, c.n_p, f(c.bias_qp), c.n_self_loop)
    gi = torch.cat([csr_weighted_sum_ref(Yp[:, (1 + k) * h:(2 + k) * h], c.rp_pp, c.c_pp, f(c.w_pp), c.n_p) for k in range(3)], 1)
    out_p = gru_ref(gi + f(c.b_ih), Yp[:, 4 * h:7 * h], X, gat_p)
    out_q = torch.relu(gat_ref(Yp[:, :h], Yp[:, 7 * h], Yq[:, h + 1], c.rp_pq, c.c_pq, c.n_q, f(c.bias_pq), c.n_self_loop))
    return out_p, out_q, c.xin[rp], c.xq_tab[rq]


# ------------------------------------------------------------------------------------------ pooling
def graph_rows(pptr, qptr, n_clicks, g):
    """Expanded rows of graph g: product-click rows [pptr[g], pptr[g+1]), then query rows n_clicks + [qptr[g], qptr[g+1])."""
    return torch.cat([torch.arange(int(pptr[g]), int(pptr[g + 1])), n_clicks + torch.arange(int(qptr[g]), int(qptr[g + 1]))])


def normalize_ref(x, eps):
    return x / torch.sqrt(torch.clamp((x * x).sum(1, keepdim=True), min=eps))


def pool_expand_ref(lin_p, lin_q, src_row, pos_id, n_clicks, pos_emb):
    """sss_pool_expand: node[e] = tanh([lin[src_row[e]] ; pos_emb[pos_id[e]]]), rows e < n_clicks read lin_p, the rest lin_q."""
    src, pid = torch.as_tensor(src_row, dtype=torch.int64), torch.as_tensor(pos_id, dtype=torch.int64)
    lin = torch.cat([lin_p[src[:n_clicks]], lin_q[src[n_clicks:]]])
    return torch.tanh(torch.cat([lin, pos_emb[pid]], 1))


def segment_pool_ref(node, pptr, qptr, n_clicks, n_graphs, a=None, bcoarse=None, watt=None, reduce_sum=False):
    """sss_segment_pool (and the body of sss_pool_attention): watt None: mean of the graph's rows; else
    mean_e(node[e] * (watt . sigmoid(a[e] + bcoarse[g]))); reduce_sum: sum instead of mean.  An empty graph gives zeros."""
    out = torch.zeros((n_graphs, node.shape[1]), dtype=node.dtype)
    for g in range(n_graphs):
        rows = graph_rows(pptr, qptr, n_clicks, g)
        if rows.numel() == 0:
            continue
        v = node[rows]
        if watt is not None:
            v = v * (sigmoid(a[rows] + bcoarse[g]) * watt).sum(1, keepdim=True)
        out[g] = seq_sum(v) if reduce_sum else seq_sum(v) / rows.numel()
    return out


def pool_expand_mean_ref(lin_p, lin_q, src_row, pos_id, pptr, qptr, n_clicks, n_graphs, pos_emb):
    """sss_pool_expand_mean: (node, coarse)."""
    node = pool_expand_ref(lin_p, lin_q, src_row, pos_id, n_clicks, pos_emb)
    return node, segment_pool_ref(node, pptr, qptr, n_clicks, n_graphs)


def pool_attention_ref(node, a, b, watt, pptr, qptr, n_clicks, n_graphs, normalize=False, eps=1e-6, reduce_sum=False):
    """sss_pool_attention."""
    out = segment_pool_ref(node, pptr, qptr, n_clicks, n_graphs, a, b, watt, reduce_sum)
    return normalize_ref(out, eps) if normalize else out


def pool_attention_tab_ref(t, ac, tanhpos, a2tab, c2tab, watt, src_row, pos_id, pptr, qptr, n_clicks, n_p, n_graphs, d_lin,
                           normalize=False, eps=1e-6):
    """sss_pool_attention_tab: per graph bc = mean_e(C1[node(e)] + c2tab[pid(e)]), att_e = watt . sigmoid(A1[node] +
    a2tab[pid] + bc), out = mean_e([t[node, :d_lin] ; tanhpos[pid]] * att_e); node(e) = src_row[e] for product rows,
    n_p + src_row[e] for query rows; ac = [A1 | C1]."""
    D = a2tab.shape[1]
    src, pid_all = torch.as_tensor(src_row, dtype=torch.int64), torch.as_tensor(pos_id, dtype=torch.int64)
    out = torch.zeros((n_graphs, D), dtype=t.dtype)
    for g in range(n_graphs):
        rows = graph_rows(pptr, qptr, n_clicks, g)
        if rows.numel() == 0:
            continue
        node = src[rows] + torch.where(rows < n_clicks, 0, n_p)
        pid = pid_all[rows]
        bc = seq_sum(ac[node, D:2 * D] + c2tab[pid]) / rows.numel()
        att = (sigmoid(ac[node, :D] + a2tab[pid] + bc) * watt).sum(1, keepdim=True)
        out[g] = seq_sum(torch.cat([t[node, :d_lin], tanhpos[pid]], 1) * att) / rows.numel()
    return normalize_ref(out, eps) if normalize else out


def tab_inputs(lin_p, lin_q, pos_emb, wn, bn, wc):
    """The weights-only tables and per-batch arrays sss_pool_attention_tab reads, from what the expand / attention pair
    reads (include/sss.h): t = tanh(lin), ac = t [Wn[:, :d_lin] ; Wc[:, :d_lin]]^T, tanhpos, a2tab, c2tab."""
    d_lin = lin_p.shape[1]
    t = torch.tanh(torch.cat([lin_p, lin_q]))
    tp = torch.tanh(pos_emb)
    ac = torch.cat([t @ wn[:, :d_lin].T, t @ wc[:, :d_lin].T], 1)
    return t, ac, tp, tp @ wn[:, d_lin:].T + bn, tp @ wc[:, d_lin:].T


# ------------------------------------------------------------------------------------------ whole encoder
def csr_by_target(edge_index, n_dst):
    """COO [2, E] (row 0 source, row 1 target) -> (rowptr int32 [n_dst + 1], col int32 [E]), edge order kept per target."""
    src, dst = np.asarray(edge_index[0], np.int64), np.asarray(edge_index[1], np.int64)
    order = np.argsort(dst, kind="stable")
    rowptr = np.zeros(n_dst + 1, np.int32)
    np.cumsum(np.bincount(dst, minlength=n_dst), out=rowptr[1:])
    return rowptr, src[order].astype(np.int32)


def pool_indices(batch):
    """(src_row, pos_id, pptr, qptr, n_clicks) of a numpy SessionBatch: expanded product rows first (node i repeated
    cnt[i] times), then one row per query node."""
    q, p = batch["query"], batch["product"]
    B = int(batch.num_graphs)
    cnt = np.asarray(p.cnt, np.int64)
    src_p = np.repeat(np.arange(cnt.shape[0]), cnt)
    src_row = np.r_[src_p, np.arange(np.asarray(q.batch).shape[0])].astype(np.int32)
    pos_id = np.r_[np.asarray(p.pos_emb_id), np.asarray(q.pos_emb_id)].astype(np.int32)
    pptr, qptr = np.zeros(B + 1, np.int32), np.zeros(B + 1, np.int32)
    np.cumsum(np.bincount(np.asarray(p.batch)[src_p], minlength=B), out=pptr[1:])
    np.cumsum(np.bincount(np.asarray(q.batch), minlength=B), out=qptr[1:])
    return src_row, pos_id, pptr, qptr, int(src_p.shape[0])


def node_transforms(W, l, cp, cq):
    """(yp, yq) of layer `l` from the raw weights `W` (flat dict of tensors in the dtype of the rows): the node transforms
    of the product rows `cp` and the query rows `cq` in the column layout of sss_hetero_layer_update."""
    g = lambda name: W[name.format(l)]
    din = cp.shape[1]
    xs_p, xs_q = cp @ g("gat_pq.{}.lin_src").T, cq @ g("gat_qp.{}.lin_src").T
    u = cp @ (g("ggc.{}.weight")[:din] @ g("ggc.{}.w_ih").T)
    gh = cp @ g("ggc.{}.w_hh")[:, :din].T + g("ggc.{}.b_hh")
    yp = torch.cat([xs_p, u, gh, (xs_p @ g("gat_pq.{}.att_src"))[:, None],
                    ((cp @ g("gat_qp.{}.lin_dst").T) @ g("gat_qp.{}.att_dst"))[:, None]], 1)
    yq = torch.cat([xs_q, (xs_q @ g("gat_qp.{}.att_src"))[:, None],
                    ((cq @ g("gat_pq.{}.lin_dst").T) @ g("gat_pq.{}.att_dst"))[:, None]], 1)
    return yp, yq


def encoder_forward(batch, w, n_layers, self_loops=True, tab=True, get_node=False):
    """The fused encoder as a chain of the restatements above, float64: per layer the node transforms in the column
    layout of sss_hetero_layer_update (yp = xs_p | u | gh | alpha_src(pq) alpha_dst(qp), yq = xs_q | alpha_src(qp)
    alpha_dst(pq), u = pad(x) W_ggc W_ih^T), the layer update, then the pooling through sss_pool_attention_tab
    (`tab`) or through expand_mean + attention.  `batch`: numpy SessionBatch, `w`: the flat weight dict."""
    from .gnn_ref import EDGE_PP, EDGE_PQ, EDGE_QP
    W = {k: torch.as_tensor(np.asarray(v), dtype=torch.float64) for k, v in w.items()}
    q, p = batch["query"], batch["product"]
    xq = W["query_table"][torch.as_tensor(np.asarray(q.x), dtype=torch.int64)]
    xp = W["item_table"][torch.as_tensor(np.asarray(p.x), dtype=torch.int64)]
    n_q, n_p = xq.shape[0], xp.shape[0]
    ei = batch.edge_index_dict
    c = SimpleNamespace(n_p=n_p, n_q=n_q, row_p=None, row_q=None, w_pp=None, n_self_loop=min(n_p, n_q) if self_loops else 0)
    (c.rp_qp, c.c_qp), (c.rp_pq, c.c_pq), (c.rp_pp, c.c_pp) = (csr_by_target(ei[EDGE_QP], n_p), csr_by_target(ei[EDGE_PQ], n_q),
                                                              csr_by_target(ei[EDGE_PP], n_p))
    nq_, np_ = [xq], [xp]
    for l in range(n_layers):
        g = lambda name: W[name.format(l)]
        cp, cq = np_[-1], nq_[-1]
        c.yp, c.yq = node_transforms(W, l, cp, cq)
        c.h, c.xin, c.xq_tab = g("ggc.{}.weight").shape[0], cp, cq
        c.bias_qp, c.bias_pq, c.b_ih = g("gat_qp.{}.bias"), g("gat_pq.{}.bias"), g("ggc.{}.b_ih")
        out_p, out_q, _, _ = layer_update_ref(c)
        np_.append(out_p)
        nq_.append(out_q)
    NQ, NP = torch.cat(nq_, 1), torch.cat(np_, 1)
    lin_p = NP @ W["pool.product_lin.w"].T + W["pool.product_lin.b"]
    lin_q = NQ @ W["pool.query_lin.w"].T + W["pool.query_lin.b"]
    wn, bn, wc, watt, pos = W["pool.node_lin.w"], W["pool.node_lin.b"], W["pool.coarse_lin.w"], W["pool.att_lin.w"], W["pool.pos_emb"]
    src_row, pos_id, pptr, qptr, n_clicks = pool_indices(batch)
    B = int(batch.num_graphs)
    if tab:
        t, ac, tp, a2, c2 = tab_inputs(lin_p, lin_q, pos, wn, bn, wc)
        out = pool_attention_tab_ref(t, ac, tp, a2, c2, watt, src_row, pos_id, pptr, qptr, n_clicks, n_p, B, lin_p.shape[1])
    else:
        node, coarse = pool_expand_mean_ref(lin_p, lin_q, src_row, pos_id, pptr, qptr, n_clicks, B, pos)
        out = pool_attention_ref(node, node @ wn.T + bn, coarse @ wc.T, watt, pptr, qptr, n_clicks, B)
    return (out, {"query": NQ, "product": NP}) if get_node else out


# ------------------------------------------------------------------------------------------ case generators
WIDTHS = (4, 8, 12, 16, 20, 32, 36, 64, 96, 100, 128, 132, 160, 192, 224, 252, 256)        # every lane-group size, with and without dead lanes
WIDE = (260, 800, 1600)                                                              # sss_pool_attention / sss_segment_pool only


def lanes_for(width):
    """Lane-group size the launchers pick (csrc/lane_group.h: lanes_for) for a row of `width` floats (for the case tables only)."""
    l = 1
    while l < width // 4 and l < 64:
        l <<= 1
    return l


def _csr(rng, n_src, n_dst, e, self_edges=5):
    """Random CSR by target; the first `self_edges` edges are source == target ones (dropped by the self-loop rewrite)."""
    if n_src == 0 or n_dst == 0:
        return np.zeros(n_dst + 1, np.int32), np.zeros(0, np.int32)
    src, dst = rng.integers(0, n_src, e), rng.integers(0, n_dst, e)
    k = min(n_dst, n_src, self_edges, e)
    dst[:k] = src[:k] = np.arange(k)
    return csr_by_target(np.stack([src, dst]), n_dst)


LAYER_STRUCTURES = ("random", "ascending", "hub", "no_edges", "all_self_edges", "np_gt_nq", "nq_gt_np", "np_zero", "nq_zero",
                    "no_w_pp", "dx_odd", "dx_full", "dx_tiny", "shared_rows", "logits_asc", "logits_desc", "logits_shuffled",
                    "gru_sat_30", "gru_sat_100", "partial_self_loop")


def layer_case(structure, h, table_mode=False, seed=0):
    """One sss_hetero_layer_update problem.  Float arrays are float32 tensors (what the kernel is given), index arrays
    numpy int32 (CSR) / torch int64 (row_p, row_q; None in node mode).  Structures:
      random          ~2-3 edges per target, O(1) logits, n_self_loop = min(n_p, n_q), d_x = 3h/4
      ascending       target 0 of both types has 48 incoming edges whose scores increase edge after edge
      hub             target 1 of both types has 300 incoming edges
      no_edges        no q-p / p-q / p-p edge at all (GAT gives the bias; with the rewrite the lone self edge)
      all_self_edges  every edge is source == target: the rewrite drops them all
      np_gt_nq / nq_gt_np   n_self_loop = min(n_p, n_q) < the larger side: only part of its targets get the self edge
      partial_self_loop     0 < n_self_loop < min(n_p, n_q): the C ABI takes any count, not only the encoder's minimum
      np_zero / nq_zero     one node type absent
      no_w_pp         w_pp = NULL (weights 1)
      dx_odd / dx_full / dx_tiny   d_x = h - 2 (h > 4), h, 3: the scalar tails of the x / x0 copies
      shared_rows     (table mode) 3 product and 2 query table rows serve all nodes
      logits_*        |leaky_relu argument| up to ~60-80, incoming scores sorted ascending / descending / shuffled
      gru_sat_30/100  GRU pre-activations of +-30 / +-100..120 (sigmoid and tanh saturated); no q-p edges and no self
                      loops, so the GAT term of a product is exactly bias_qp
    """
    rng = np.random.default_rng([seed, h, LAYER_STRUCTURES.index(structure), int(table_mode)])
    g = torch.Generator().manual_seed(int(rng.integers(1 << 31)))
    rn = lambda *s: torch.randn(s, generator=g)
    n_p, n_q = {"np_gt_nq": (130, 37), "nq_gt_np": (41, 150), "np_zero": (0, 50), "nq_zero": (60, 0)}.get(structure, (90, 70))
    d_x = {"dx_odd": h - 2 if h > 4 else 2, "dx_full": h, "dx_tiny": min(3, h)}.get(structure, max(3 * h // 4, 1))
    rows_p, rows_q = n_p, n_q
    if table_mode:
        rows_p, rows_q = (3, 2) if structure == "shared_rows" else (211, 53)
    c = SimpleNamespace(structure=structure, h=h, d_x=d_x, n_p=n_p, n_q=n_q, table_mode=table_mode)
    c.yp, c.yq = rn(rows_p, 7 * h + 2) * 0.5, rn(rows_q, h + 2) * 0.5
    c.xin, c.xq_tab = rn(rows_p, d_x), rn(rows_q, d_x)
    c.row_p = torch.from_numpy(rng.integers(0, rows_p, n_p)) if table_mode and n_p else (torch.zeros(0, dtype=torch.int64) if table_mode else None)
    c.row_q = torch.from_numpy(rng.integers(0, rows_q, n_q)) if table_mode and n_q else (torch.zeros(0, dtype=torch.int64) if table_mode else None)
    e_qp, e_pp = (0, 0) if structure == "no_edges" else (3 * max(n_p, n_q), 3 * n_p)
    if structure.startswith("gru_sat"):
        e_qp = 0
    c.rp_qp, c.c_qp = _csr(rng, n_q, n_p, e_qp)
    c.rp_pq, c.c_pq = _csr(rng, n_p, n_q, e_qp)
    c.rp_pp, c.c_pp = _csr(rng, n_p, n_p, e_pp)
    c.n_self_loop = 0 if structure.startswith("gru_sat") else min(n_p, n_q) // (2 if structure == "partial_self_loop" else 1)

    def set_row(which, i, cols):                                  # replace the incoming edges of target i
        rp, col = (c.rp_qp, c.c_qp) if which == "qp" else (c.rp_pq, c.c_pq)
        cols = np.asarray(cols, np.int32)
        new = np.r_[col[:rp[i]], cols, col[rp[i + 1]:]].astype(np.int32)
        rp = rp.copy()
        rp[i + 1:] += len(cols) - (rp[i + 1] - rp[i])
        if which == "qp":
            c.rp_qp, c.c_qp = rp, new
        else:
            c.rp_pq, c.c_pq = rp, new

    if structure == "all_self_edges":
        k = min(n_p, n_q)
        ident = (np.r_[np.arange(k + 1), np.full(max(n_p, n_q) - k, k)].astype(np.int32), np.arange(k, dtype=np.int32))
        c.rp_qp, c.c_qp = ident[0][:n_p + 1].copy(), ident[1].copy()
        c.rp_pq, c.c_pq = ident[0][:n_q + 1].copy(), ident[1].copy()
        c.rp_pp, c.c_pp = np.arange(n_p + 1, dtype=np.int32), np.arange(n_p, dtype=np.int32)
    if structure == "hub":
        set_row("qp", 1, rng.integers(0, n_q, 300))
        set_row("pq", 1, rng.integers(0, n_p, 300))
    if structure == "ascending":                                   # 48 distinct sources
        set_row("qp", 0, rng.permutation(n_q)[:48])
        set_row("pq", 0, rng.permutation(n_p)[:48])
    src_score_col = {"qp": (c.yq, h, c.row_q), "pq": (c.yp, 7 * h, c.row_p)}
    if structure.startswith("logits"):
        for y, cols in ((c.yq, (h, h + 1)), (c.yp, (7 * h, 7 * h + 1))):
            for col in cols:
                y[:, col] = (torch.rand(y.shape[0], generator=g) * 2 - 1) * 40
    if structure.startswith("logits") or structure == "ascending":
        for which in ("qp", "pq"):                                 # order every target's incoming scores
            rp, col = (c.rp_qp, c.c_qp) if which == "qp" else (c.rp_pq, c.c_pq)
            y, colno, rows = src_score_col[which]
            col = col.copy()
            for i in range(len(rp) - 1):
                seg = col[rp[i]:rp[i + 1]]
                srow = seg if rows is None else rows[torch.from_numpy(seg.astype(np.int64))].numpy()
                s = y[torch.from_numpy(np.asarray(srow, np.int64)), colno].numpy()
                if structure in ("logits_asc", "ascending"):
                    seg = seg[np.argsort(s, kind="stable")]
                elif structure == "logits_desc":
                    seg = seg[np.argsort(-s, kind="stable")]
                else:
                    seg = rng.permutation(seg)
                col[rp[i]:rp[i + 1]] = seg
            if which == "qp":
                c.c_qp = col
            else:
                c.c_pq = col
    c.w_pp = None if structure == "no_w_pp" else torch.rand(len(c.c_pp), generator=g) + 0.5
    c.bias_qp, c.bias_pq, c.b_ih = rn(h), rn(h), rn(3 * h)
    if structure.startswith("gru_sat"):
        # gh columns carry the whole pre-activation: sign patterns per (node, column), magnitude 30 or 100 / 120
        big = [30.0] if structure == "gru_sat_30" else [100.0, 120.0]
        c.yp[:, h:4 * h] *= 0.01                                   # u: negligible next to the saturating gh
        c.b_ih *= 0.01
        sg = lambda *s: (torch.randint(0, 2, s, generator=g) * 2 - 1).float()
        mag = torch.tensor(big)[torch.randint(0, len(big), (rows_p, 3 * h), generator=g)]
        c.yp[:, 4 * h:7 * h] = sg(rows_p, 3 * h) * mag
    return c


def check_layer_case(c):
    """Every index a kernel would dereference is in range, every CSR well formed."""
    h = c.h
    rows_p, rows_q = c.yp.shape[0], c.yq.shape[0]
    assert c.yp.shape[1] == 7 * h + 2 and c.yq.shape[1] == h + 2 and h % 4 == 0 and 0 < h <= 256 and 0 <= c.d_x <= h
    assert c.xin.shape == (rows_p, c.d_x) and c.xq_tab.shape == (rows_q, c.d_x)
    for rows, n, nrows in ((c.row_p, c.n_p, rows_p), (c.row_q, c.n_q, rows_q)):
        if rows is None:
            assert n == nrows
        else:
            assert rows.dtype == torch.int64 and rows.shape == (n,) and (n == 0 or (0 <= int(rows.min()) and int(rows.max()) < nrows))
    for rp, col, n_src, n_dst in ((c.rp_qp, c.c_qp, c.n_q, c.n_p), (c.rp_pq, c.c_pq, c.n_p, c.n_q), (c.rp_pp, c.c_pp, c.n_p, c.n_p)):
        assert rp.dtype == np.int32 and col.dtype == np.int32 and rp.shape == (n_dst + 1,)
        assert rp[0] == 0 and rp[-1] == len(col) and np.all(np.diff(rp) >= 0)
        assert len(col) == 0 or (col.min() >= 0 and col.max() < n_src)
    assert c.w_pp is None or c.w_pp.shape == (len(c.c_pp),)
    assert 0 <= c.n_self_loop <= min(c.n_p, c.n_q)
    assert c.bias_qp.shape == c.bias_pq.shape == (h,) and c.b_ih.shape == (3 * h,)
    return c


GRAPH_LENGTHS = (0, 1, 3, 4, 5, 63, 64, 65, 128, 129, 200)


def pool_graphs(kind, seed=0):
    """Per-graph (product rows, query rows) lists.  'lengths': one graph per total in GRAPH_LENGTHS (rows split between
    the two kinds), an only-product and an only-query graph of 70 rows; 'interleaved': 200, 1, 200, 1, ... so long and
    short graphs share a wave; 'single': one graph of 77 rows.  The graph counts (15, 11, 1) are no multiple of 4, hence
    of no graphs-per-block count of the kernels (4 to 256)."""
    rng = np.random.default_rng([seed, 77])
    if kind == "lengths":
        out = [(int(rng.integers(0, n + 1)),) for n in GRAPH_LENGTHS]
        out = [(a[0], n - a[0]) for a, n in zip(out, GRAPH_LENGTHS)]
        out[GRAPH_LENGTHS.index(1)] = (0, 1)
        return out + [(70, 0), (0, 70), (1, 0), (2, 2)]
    if kind == "interleaved":
        return [(120, 80), (1, 0), (200, 0), (0, 1), (0, 200), (1, 0), (37, 163), (0, 1), (200, 0), (0, 1), (150, 50)]
    if kind == "single":
        return [(40, 37)]
    raise ValueError(kind)


def pool_case(D, P, kind="lengths", seed=0, scale=1.0):
    """Inputs of the three pooling entry points on hand-built graphs.  lin / pos_emb feed sss_pool_expand_mean; node /
    a / b / watt feed sss_pool_attention and sss_segment_pool; t / ac / tanhpos / a2tab / c2tab feed
    sss_pool_attention_tab.  `scale` multiplies every pre-activation (tanh and sigmoid inputs): 100 saturates them."""
    graphs = pool_graphs(kind, seed)
    rng = np.random.default_rng([seed, D, P, len(graphs)])
    g = torch.Generator().manual_seed(int(rng.integers(1 << 31)))
    rn = lambda *s: torch.randn(s, generator=g)
    c = SimpleNamespace(D=D, P=P, Dl=D - P, kind=kind, B=len(graphs), n_p=23, n_q=17)
    npr, nqr = np.array([a for a, _ in graphs]), np.array([b for _, b in graphs])
    c.pptr, c.qptr = np.zeros(c.B + 1, np.int32), np.zeros(c.B + 1, np.int32)
    np.cumsum(npr, out=c.pptr[1:])
    np.cumsum(nqr, out=c.qptr[1:])
    c.n_clicks, c.n_exp = int(npr.sum()), int(npr.sum() + nqr.sum())
    c.src_row = np.r_[rng.integers(0, c.n_p, c.n_clicks), rng.integers(0, c.n_q, c.n_exp - c.n_clicks)].astype(np.int32)
    c.pos_id = rng.integers(0, max(P, 1), c.n_exp).astype(np.int32)
    c.lin_p, c.lin_q, c.pos_emb = rn(c.n_p, c.Dl) * scale, rn(c.n_q, c.Dl) * scale, rn(P, P) * scale
    c.node, c.a, c.b, c.watt = torch.tanh(rn(c.n_exp, D) * scale), rn(c.n_exp, D) * scale, rn(c.B, D) * scale, rn(D) / D ** 0.5
    c.t, c.tanhpos = torch.tanh(rn(c.n_p + c.n_q, c.Dl) * scale), torch.tanh(rn(P, P) * scale)
    c.ac, c.a2tab, c.c2tab = rn(c.n_p + c.n_q, 2 * D) * scale, rn(P, D) * scale, rn(P, D) * scale
    return c


def check_pool_case(c):
    """pptr / qptr monotone and consistent with the lengths of src_row / pos_id; every index in range."""
    assert c.D == c.Dl + c.P and c.D % 4 == 0 and c.Dl > 0 and c.P >= 0
    for ptr in (c.pptr, c.qptr):
        assert ptr.dtype == np.int32 and ptr.shape == (c.B + 1,) and ptr[0] == 0 and np.all(np.diff(ptr) >= 0)
    assert c.pptr[-1] == c.n_clicks and c.n_clicks + c.qptr[-1] == c.n_exp
    assert c.src_row.dtype == c.pos_id.dtype == np.int32 and c.src_row.shape == c.pos_id.shape == (c.n_exp,)
    if c.n_exp:
        assert c.src_row.min() >= 0 and c.src_row[:c.n_clicks].max(initial=0) < c.n_p and c.src_row[c.n_clicks:].max(initial=0) < c.n_q
        assert c.pos_id.min() >= 0 and c.pos_id.max() < c.P
    assert c.lin_p.shape == (c.n_p, c.Dl) and c.lin_q.shape == (c.n_q, c.Dl) and c.pos_emb.shape == (c.P, c.P)
    assert c.node.shape == c.a.shape == (c.n_exp, c.D) and c.b.shape == (c.B, c.D) and c.watt.shape == (c.D,)
    assert c.t.shape == (c.n_p + c.n_q, c.Dl) and c.ac.shape == (c.n_p + c.n_q, 2 * c.D)
    assert c.tanhpos.shape == (c.P, c.P) and c.a2tab.shape == c.c2tab.shape == (c.P, c.D)
    return c


def pool_p_for(D):
    """Positional width used with row width D in the width sweep: the default 20 where it fits, else D / 2 (which puts
    d_lin % 4 == 2 at D = 4 and 12)."""
    return 20 if D >= 36 else D // 2


def session_table(sessions):
    """Hand-written sessions -> the four ActionTable arrays.  A session is a list of actions: ('s', query_token) or
    ('c', item_id)."""
    ptr = np.zeros(len(sessions) + 1, np.int64)
    np.cumsum([len(s) for s in sessions], out=ptr[1:])
    flat = [a for s in sessions for a in s]
    is_search = np.array([k == "s" for k, _ in flat], bool)
    ids = np.array([v for _, v in flat], np.int64)
    return ptr, is_search, np.where(is_search, 0, ids), np.where(is_search, ids, 0)


def edge_sessions(kind, n_items, n_query, seed=0):
    """Session shapes the synthetic generator does not draw (at most 64 actions each)."""
    rng = np.random.default_rng([seed, 5])
    click = lambda: ("c", int(rng.integers(1, n_items)))
    search = lambda: ("s", int(rng.integers(1, n_query)))
    mixed = lambda n: [search() if rng.random() < 0.3 else click() for _ in range(n)]
    if kind == "cap":                      # two sessions at the 64-action cap between short ones
        return [mixed(64), mixed(3), mixed(64), mixed(2)]
    if kind == "one_item_60":              # one item clicked 60 times: cnt = 60, position ids 1..64
        return [[search()] + [("c", 7)] * 60 + [click(), search(), click()], mixed(4)]
    if kind == "one_action":               # sessions of a single action, clicks and searches
        return [[click()], [search()], [click()], [search()], [click()]]
    if kind == "batch_of_one":
        return [mixed(9)]
    if kind == "cap_among_ones":           # a capped session whose wave neighbours have one action
        return [[click()], [search()], mixed(64), [click()], [search()], [click()], [click()]]
    if kind == "short":
        return [mixed(int(rng.integers(2, 7))) for _ in range(5)]
    raise ValueError(kind)
