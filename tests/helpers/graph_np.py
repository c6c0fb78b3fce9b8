"""Plain-numpy test helpers of the session-graph tests: the CSR-by-target conversion, the reference-run fixture
(tests/golden/reference_graph.npz) read back per session, relabelled to first-occurrence product order and collated
with numpy offsets, and the expected arrays of a prepared batch.  No product code in here."""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "golden")
COLLATED_KEYS = ("q_x", "q_pos", "q_batch", "p_x", "p_cnt", "p_pos", "p_batch", "qp0", "qp1", "pp0", "pp1", "pp_w")


def csr_by_target(src, dst, n_dst, w=None):
    """COO (src, dst) -> (rowptr int64 [n_dst + 1], col, weights) grouped by target, edge order kept inside a target."""
    order = np.argsort(dst, kind="stable")
    rowptr = np.zeros(n_dst + 1, np.int64)
    np.cumsum(np.bincount(dst, minlength=n_dst), out=rowptr[1:])
    return rowptr, src[order], None if w is None else w[order]


# ------------------------------------------------------------------------------------ the reference-run fixture
def load_fixture(path=None):
    with np.load(path or os.path.join(GOLDEN, "reference_graph.npz"), allow_pickle=False) as z:
        return {k: z[k] for k in z.files}                   # read every array once


def fixture_sessions(z):
    """Input side: one python session [(is_search, item_id, query_tok)] per record."""
    sp = z["sess_ptr"]
    return [[(bool(z["is_search"][t]), int(z["item_id"][t]), int(z["query_tok"][t])) for t in range(sp[r], sp[r + 1])]
            for r in range(len(sp) - 1)]


def fixture_graph(z, r):
    """Output side of record r, exactly as the reference's sequence_to_graph returned it (hash-ordered products)."""
    cut = lambda key, ptr, ax=0: z[key][..., z[ptr][r]:z[ptr][r + 1]] if ax else z[key][z[ptr][r]:z[ptr][r + 1]]
    return dict(p_x=cut("p_x", "p_ptr"), p_cnt=cut("p_cnt", "p_ptr"), p_last=cut("p_last", "p_ptr"),
                p_pos=cut("p_pos", "pos_ptr"), q_pos=cut("q_pos", "q_ptr"), q_mask=cut("q_mask", "q_ptr"),
                qp=cut("qp", "qp_ptr", 1), pq=cut("pq", "qp_ptr", 1), pp=cut("pp", "pp_ptr", 1), pp_w=cut("pp_w", "pp_ptr"))


def relabel_first_occurrence(g):
    """The one documented difference: the reference numbers a session's products in `list(set())` order, this project
    in first-occurrence order.  The click edges are in action order, so a product's first occurrence is its first
    appearance among their targets: renumber by that, permute the per-node arrays (the position ids move as whole
    per-node groups) and map the edge endpoints.  Edge ORDER is untouched -- it does not depend on the numbering."""
    n = len(g["p_x"])
    targets = g["qp"][1]
    assert np.array_equal(g["pq"][0], targets) and np.array_equal(g["pq"][1], g["qp"][0])
    if len(targets) == 0:                                   # no click: the single "unknown item" node
        assert n == 1
        return dict(g)
    _, first = np.unique(targets, return_index=True)        # first[i]: first click edge into reference node i
    assert len(first) == n                                  # every product node is clicked
    old_of_new = np.argsort(first, kind="stable")
    new_of_old = np.empty(n, np.int64)
    new_of_old[old_of_new] = np.arange(n)
    groups = np.split(g["p_pos"], np.cumsum(g["p_cnt"])[:-1])
    out = dict(g)
    for k in ("p_x", "p_cnt", "p_last"):
        out[k] = g[k][old_of_new]
    out["p_pos"] = np.concatenate([groups[i] for i in old_of_new])
    out["qp"] = np.stack([g["qp"][0], new_of_old[targets]])
    out["pq"] = out["qp"][::-1]
    out["pp"] = new_of_old[g["pp"]]
    return out


def collate_fixture(z):
    """Every record relabelled and concatenated with numpy offsets (Batch.from_data_list: per node type, edge endpoints
    offset by the node count of their type), in oracle.graph_ref.collate's key layout.  q_x is taken from the INPUT
    table (root 0, then the searches' query_tok): the reference produces no query id."""
    R = len(z["sess_ptr"]) - 1
    gs = [relabel_first_occurrence(fixture_graph(z, r)) for r in range(R)]
    nq = np.array([len(g["q_pos"]) for g in gs])
    n_p = np.array([len(g["p_x"]) for g in gs])
    qo, po = np.r_[0, np.cumsum(nq)], np.r_[0, np.cumsum(n_p)]
    cat = lambda f: np.concatenate([f(r, g) for r, g in enumerate(gs)]).astype(np.int64)
    sp = z["sess_ptr"]
    o = dict(
        q_x=cat(lambda r, g: np.r_[0, z["query_tok"][sp[r]:sp[r + 1]][z["is_search"][sp[r]:sp[r + 1]]]]),
        q_pos=cat(lambda r, g: g["q_pos"]), q_batch=np.repeat(np.arange(R), nq),
        p_x=cat(lambda r, g: g["p_x"]), p_cnt=cat(lambda r, g: g["p_cnt"]), p_pos=cat(lambda r, g: g["p_pos"]),
        p_batch=np.repeat(np.arange(R), n_p),
        qp0=cat(lambda r, g: g["qp"][0] + qo[r]), qp1=cat(lambda r, g: g["qp"][1] + po[r]),
        pp0=cat(lambda r, g: g["pp"][0] + po[r]), pp1=cat(lambda r, g: g["pp"][1] + po[r]))
    o["pp_w"] = np.concatenate([g["pp_w"] for g in gs]).astype(np.float32)
    o["p_last"] = np.concatenate([g["p_last"] for g in gs]).astype(np.float32)
    return o


def batch_to_collated(b):
    """A host SessionBatch (numpy) in the same key layout."""
    q, p = b["query"], b["product"]
    ei = b.edge_index_dict
    qp, pp = ei[("query", "clicks", "product")], ei[("product", "to", "product")]
    return dict(q_x=q.x, q_pos=q.pos_emb_id, q_batch=q.batch, p_x=p.x, p_cnt=p.cnt, p_pos=p.pos_emb_id, p_batch=p.batch,
                qp0=qp[0], qp1=qp[1], pp0=pp[0], pp1=pp[1], pp_w=b.edge_weight_dict[("product", "to", "product")])


# ------------------------------------------------------------------------------------ expected prepared batch
def expected_prepared(o, n_graphs):
    """Every array of a prepared batch from collated COO graphs: node ids, batch vectors, the three CSRs by target,
    the pooling's src_row / pos_id (expanded product rows, then the query nodes) and the per-graph pointers."""
    Nq, Np = len(o["q_x"]), len(o["p_x"])
    e = dict(Nq=Nq, Np=Np, B=n_graphs, n_clicks=int(np.sum(o["p_cnt"])),
             q_ids=o["q_x"], p_ids=o["p_x"], q_batch=o["q_batch"], p_batch=o["p_batch"], p_cnt=o["p_cnt"],
             csr_qp=csr_by_target(o["qp0"], o["qp1"], Np), csr_pq=csr_by_target(o["qp1"], o["qp0"], Nq),
             csr_pp=csr_by_target(o["pp0"], o["pp1"], Np, o["pp_w"]),
             src_row=np.r_[np.repeat(np.arange(Np), o["p_cnt"]), np.arange(Nq)], pos_id=np.r_[o["p_pos"], o["q_pos"]])
    clicks_per_graph = np.bincount(o["p_batch"], weights=o["p_cnt"], minlength=n_graphs).astype(np.int64)
    e["pptr"] = np.r_[0, np.cumsum(clicks_per_graph)]
    e["qptr"] = np.r_[0, np.cumsum(np.bincount(o["q_batch"], minlength=n_graphs))]
    e["p_ptr"] = np.r_[0, np.cumsum(np.bincount(o["p_batch"], minlength=n_graphs))]
    return e


def assert_prepared_equal(got, e):
    """`got`: a PreparedBatch of SessionEncoder.prepare_actions (device tensors); every comparison is array_equal."""
    npy = lambda t: t.cpu().numpy().astype(np.int64)
    assert (got.Nq, got.Np, got.B, got.n_clicks) == (e["Nq"], e["Np"], e["B"], e["n_clicks"])
    for name in ("q_ids", "p_ids", "q_batch", "p_batch", "p_cnt", "src_row", "pos_id", "qptr", "p_ptr", "pptr"):
        assert np.array_equal(npy(getattr(got, name)), e[name]), name
    assert np.array_equal(npy(got.q_pos), e["pos_id"][e["n_clicks"]:]), "q_pos"
    for name in ("csr_qp", "csr_pq", "csr_pp"):
        assert np.array_equal(npy(getattr(got, name)[0]), e[name][0]), name + ".rowptr"
        assert np.array_equal(npy(getattr(got, name)[1]), e[name][1]), name + ".col"
    w = got.w_pp.cpu().numpy()
    assert w.dtype == np.float32 and np.array_equal(w, e["csr_pp"][2]), "w_pp"
