"""Generates tests/golden/jaccard_truth.npz by RUNNING the reference's own get_item and get_score on EVERY (query, corpus)
pair of the sessions already in tests/golden/eval_metrics.npz (48 x 400 pairs).
Build container only (needs /root/reference):  python tests/golden/make_golden_jaccard.py

As in make_golden_eval.py each `def` is located in its file's syntax tree, compiled alone into a namespace and called;
nothing of the reference's text is written anywhere.  The inputs are read from eval_metrics.npz, not duplicated; the .npz
holds the two float64 matrices

  ref_all_jaccard [48, 400]    get_score((seq, tar), (corpus session, []), 'all_jaccard')    fine_tune_ours.py:42-47
  ref_cur_jaccard [48, 400]    get_score((seq, tar), (corpus session, []), 'cur_jaccard')    fine_tune_ours.py:48-55

and the generator asserts what the tests rely on the fixture to contain.
"""
import ast
import os

import numpy as np

REF = "/root/reference"
HERE = os.path.dirname(os.path.abspath(__file__))
NS = {"np": np}


def extract(path, name):
    """The top-level `def name` of a reference file, compiled alone into the shared namespace."""
    src = open(os.path.join(REF, path)).read()
    fn = next(n for n in ast.parse(src).body if isinstance(n, ast.FunctionDef) and n.name == name)
    exec(compile(ast.Module(body=[fn], type_ignores=[]), os.path.join(REF, path), "exec"), NS)
    return NS[name]


get_item = extract("util_amazon_filtered.py", "get_item")
get_score = extract("fine_tune_ours.py", "get_score")


def sessions(g, tag):
    """Raw action tuples (session, 's' | 'c', text, item) of a stored action table, as make_golden_eval.py made them."""
    ptr, srch, item = g[f"{tag}_sess_ptr"], g[f"{tag}_is_search"], g[f"{tag}_item_id"]
    return [[(s, "s", "q", 0) if srch[a] else (s, "c", None, int(item[a])) for a in range(ptr[s], ptr[s + 1])]
            for s in range(len(ptr) - 1)]


g = np.load(os.path.join(HERE, "eval_metrics.npz"))
corpus, seqs, tars = sessions(g, "corpus"), sessions(g, "seq"), sessions(g, "tar")
out = {}
for sim in ("all_jaccard", "cur_jaccard"):
    out[f"ref_{sim}"] = np.array([[get_score((a, b), (c, []), sim) for c in corpus] for a, b in zip(seqs, tars)], np.float64)


def full(r, edges):
    """Queries with rows in every band of `edges`."""
    band = (r[:, :, None] >= np.asarray(edges)[None, None, :]).sum(2)
    return int(sum(all((band[f] == b).any() for b in range(len(edges) + 1)) for f in range(r.shape[0])))


def tied_at(r, k):
    s = -np.sort(-r.astype(np.float32), axis=1)
    return int((s[:, k - 1] == s[:, k]).sum())


A, C = out["ref_all_jaccard"], out["ref_cur_jaccard"]
facts = {
    "shape": A.shape == (48, 400) and C.shape == (48, 400),
    "all: 14 queries with all three bands of (0.2, 0.5)": full(A, (0.2, 0.5)) == 14,
    "cur: 16 queries with all three bands of (0.2, 0.5)": full(C, (0.2, 0.5)) == 16,
    "cur: 2 queries with all three bands of (0.2, 0.8)": full(C, (0.2, 0.8)) == 2,
    "all: no query reaches 0.8": float(A.max()) < 0.8,
    "598 / 786 pairs exactly on an edge of (0.2, 0.5)": (int(np.isin(A, (0.2, 0.5)).sum()), int(np.isin(C, (0.2, 0.5)).sum())) == (598, 786),
    "41 of 48 queries tied at rank 20, 46 at rank 100": (tied_at(A, 20), tied_at(A, 100)) == (41, 46),
    "16 empty corpus sets": sum(len(get_item(c)) == 0 for c in corpus) == 16,
    "5 empty cur query sets": sum(len(get_item(a)) == 0 for a in seqs) == 5,
}
for name, ok in facts.items():
    print(f"{'ok ' if ok else 'FAILED'}  {name}")
assert all(facts.values())
np.savez_compressed(os.path.join(HERE, "jaccard_truth.npz"), **out)
print("wrote jaccard_truth.npz:", os.path.getsize(os.path.join(HERE, "jaccard_truth.npz")), "bytes")
