"""Generates tests/golden/reference_graph.npz by RUNNING the reference's own `sequence_to_graph`
(util_amazon_filtered.py:98-230) on seeded and hand-written sessions.  Build container only (needs /root/reference):
    python tests/golden/make_golden_graph.py [output directory]

The file cannot be imported here (`torch_geometric`, `Levenshtein` at its top), but the function bodies need neither:
the `def`s of `get_query_node_tokens`, `get_item`, `get_all_query`, `get_item_title`, `get_item_pos_cnt`,
`session_to_text` and `sequence_to_graph` are located in the file's syntax tree and compiled together into one
namespace that holds numpy, torch and two stand-ins.  Nothing of the reference's text is written anywhere -- the .npz
holds inputs and the outputs the reference's code produced for them.

The stand-ins supply NO ARITHMETIC and no structure:
  * `HeteroData` -> an attribute bag keyed by strings and tuples (what `data['product'].x = ...` needs);
  * the tokenizer -> zero tensors of shape [len(texts), max_length] (token tensors are not recorded).
Distinct items, counts, grouped position ids, click edges, de-duplicated transitions with their weights, the
last-click mask, the query positions and the `ignore_query` filtering (:101-103) are all the reference function's own.

Inputs are sessions of reference action tuples `(ts, type, keyword, asin, ptype, brand, title, item_id)`; search
keywords come from the numbered list KEYWORDS and the fixture stores the keyword's NUMBER as `query_tok`.  The
reference produces no query id (its query nodes carry token tensors), so `q_x` is NOT pinned by this fixture.

Every session is stored twice, interleaved: record 2i with ignore_query=False, record 2i+1 with ignore_query=True.
The stored input table of a record is the sequence the reference itself kept (`data['ori_seq'][0]`): for
ignore_query=True that is the search-free session, filtered by the reference.
"""
import ast
import os
import sys
import types

import numpy as np
import torch

REF = "/root/reference"
HERE = os.path.dirname(os.path.abspath(__file__))
NAMES = ("get_query_node_tokens", "get_item", "get_all_query", "get_item_title", "get_item_pos_cnt", "session_to_text",
         "sequence_to_graph")
KEYWORDS = [None] + [f"keyword {i}" for i in range(1, 9)]         # number -> keyword; 0 is the root's empty query
LENGTHS = (0, 1, 2, 3, 5, 8, 19, 20, 63, 64)
SHARES = (0.0, 0.3, 0.7, 1.0)
VOCABS = (2, 3, 6, 391572)                                        # item ids 1 .. V-1 (0 = the reserved unknown item)
QUERY_MAX_LEN = 4


class Bag:
    """Stands in for HeteroData: `bag[key]` is an attribute store created on first use; `bag[key] = v` stores v."""

    def __init__(self):
        self._d = {}

    def __getitem__(self, key):
        if key not in self._d:
            self._d[key] = types.SimpleNamespace()
        return self._d[key]

    def __setitem__(self, key, value):
        self._d[key] = value


def zero_tokenizer(texts, padding=None, max_length=None, truncation=None, return_tensors=None):
    z = torch.zeros((len(texts), max_length), dtype=torch.long)
    return {"input_ids": z, "token_type_ids": z.clone(), "attention_mask": z.clone()}


def extract_together(path, names):
    """The top-level `def`s called `names` of a reference file, compiled together into one namespace."""
    src = open(os.path.join(REF, path)).read()
    defs = [n for n in ast.parse(src).body if isinstance(n, ast.FunctionDef) and n.name in names]
    assert sorted(d.name for d in defs) == sorted(names), [d.name for d in defs]
    ns = {"np": np, "torch": torch, "HeteroData": Bag}
    exec(compile(ast.Module(body=defs, type_ignores=[]), os.path.join(REF, path), "exec"), ns)
    return ns


def search(tok):
    return (0, "s", KEYWORDS[tok], None, None, None, None, 0)


def click(item):
    return (0, "c", None, f"asin{item}", None, None, f"title {item}", item)


def seeded_sessions():
    rng = np.random.default_rng(20261017)
    out = []
    for n in LENGTHS:
        for share in SHARES:
            for vocab in VOCABS:
                for _ in range(2):
                    is_s = rng.random(n) < share
                    items = 1 + rng.integers(0, vocab - 1, n)
                    toks = 1 + rng.integers(0, len(KEYWORDS) - 1, n)
                    out.append([search(int(toks[t])) if is_s[t] else click(int(items[t])) for t in range(n)])
    return out


def hand_sessions():
    A, B, C = 11, 5, 8
    return [
        [],                                                              # no actions
        [search(3)],                                                     # one search
        [click(A)],                                                      # one click
        [click(A), click(B), click(C), click(B)],                        # click-only
        [search(1), search(2), search(1)],                               # search-only
        [click(A), click(A), click(A), click(A)],                        # self transition, weight 3
        [click(A), click(B), click(A), click(B)],                        # A->B twice, B->A once
        [click(A), search(4), click(A)],                                 # a search between two clicks of one item
        [search(1 + t % 8) if t % 3 == 0 else click(1 + t % 7) for t in range(63)] + [click(C)],    # 64, click last
        [click(1 + t % 5) if t % 4 else search(1 + t % 8) for t in range(63)] + [search(7)],        # 64, search last
    ]


def main(out_dir):
    ns = extract_together("util_amazon_filtered.py", NAMES)
    sequence_to_graph = ns["sequence_to_graph"]
    sessions = hand_sessions() + seeded_sessions()
    keys = ("is_search", "item_id", "query_tok", "p_x", "p_cnt", "p_pos", "p_last", "q_pos", "q_mask",
            "qp", "pq", "pp", "pp_w")
    cat = {k: [] for k in keys}
    ptr = {k: [0] for k in ("sess_ptr", "p_ptr", "pos_ptr", "q_ptr", "qp_ptr", "pp_ptr")}
    ignore = []
    tok_of = {kw: i for i, kw in enumerate(KEYWORDS)}
    for idx, seq in enumerate(sessions):
        for ig in (False, True):
            d = sequence_to_graph(idx, list(seq), [], zero_tokenizer, QUERY_MAX_LEN, ignore_query=ig)
            kept = d["ori_seq"][0]                                       # the sequence the reference built the graph from
            cat["is_search"] += [a[1] == "s" for a in kept]
            cat["item_id"] += [0 if a[1] == "s" else a[-1] for a in kept]
            cat["query_tok"] += [tok_of[a[2]] if a[1] == "s" else 0 for a in kept]
            p, q = d["product"], d["query"]
            e_qp, e_pq = d["query", "clicks", "product"], d["product", "clicked by", "query"]
            e_pp = d["product", "to", "product"]
            assert e_qp.edge_weight is None and e_pq.edge_weight is None
            cat["p_x"].append(p.x.numpy()); cat["p_cnt"].append(p.cnt.numpy()); cat["p_pos"].append(p.pos_emb_id.numpy())
            cat["p_last"].append(p.last_click_mask.numpy())
            cat["q_pos"].append(q.pos_emb_id.numpy()); cat["q_mask"].append(q.mask.numpy())
            cat["qp"].append(e_qp.edge_index.numpy().reshape(2, -1)); cat["pq"].append(e_pq.edge_index.numpy().reshape(2, -1))
            cat["pp"].append(e_pp.edge_index.numpy().reshape(2, -1)); cat["pp_w"].append(e_pp.edge_weight.numpy())
            ptr["sess_ptr"].append(len(cat["is_search"]))
            for pk, k, ax in (("p_ptr", "p_x", 0), ("pos_ptr", "p_pos", 0), ("q_ptr", "q_pos", 0), ("qp_ptr", "qp", 1),
                              ("pp_ptr", "pp", 1)):
                ptr[pk].append(ptr[pk][-1] + cat[k][-1].shape[ax])
            ignore.append(ig)
    out = {k: np.asarray(v, np.int64) for k, v in ptr.items()}
    out["ignore_query"] = np.asarray(ignore, bool)
    out["n_hand"] = np.int64(len(hand_sessions()))
    out["is_search"] = np.asarray(cat["is_search"], bool)
    out["item_id"] = np.asarray(cat["item_id"], np.int64)
    out["query_tok"] = np.asarray(cat["query_tok"], np.int64)
    for k in ("p_x", "p_cnt", "p_pos", "q_pos"):
        out[k] = np.concatenate(cat[k]).astype(np.int64)
    for k in ("qp", "pq", "pp"):
        out[k] = np.concatenate(cat[k], axis=1).astype(np.int64)
    for k in ("p_last", "q_mask", "pp_w"):
        out[k] = np.concatenate(cat[k]).astype(np.float32)
    path = os.path.join(out_dir, "reference_graph.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}: {len(ignore)} records, {len(out['is_search'])} actions, {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else HERE)
