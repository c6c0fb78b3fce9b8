"""Generates tests/golden/eval_metrics.npz by RUNNING the reference's own metric functions on seeded sessions.
Build container only (needs /root/reference, scipy and scikit-learn):  python tests/golden/make_golden_eval.py

As in make_golden_sparse.py each `def` is located in its file's syntax tree, compiled alone into a namespace holding only
numpy, sklearn's average_precision_score and the other extracted functions it calls, and called; nothing of the
reference's text is written anywhere.  The .npz holds the inputs (action tables of the corpus, of the query sessions and
of their (seq, tar) halves, and I) and the reference's value of every metric:

  get_item                                  util_amazon_filtered.py:33-34
  get_score, get_ave_score                  fine_tune_ours.py:42-97
  get_future_map                            test_amazon_filterd.py:226-244
  get_cur / all / future_jaccard            test_amazon_filterd.py:286-312, 331-343
  get_cur / all / future_recall             test_amazon_filterd.py:345-382
  get_recall                                test_amazon_filterd.py:443-450
  sequence_to_binary_vec, find_K_sparse_dense, normalize     (as make_golden_sparse.py: half of I is their result)

ref_cur_map / ref_all_map are get_future_map fed the cur / all sessions in place of the future ones: the reference's own
get_cur_map / get_all_map index an older dataset layout (train_data[0][...], sets of raw actions).

The (seq, tar) cut is ActionTable.split(1, 2): the first ceil(len / 2) actions, the rest.
"""
import ast
import os

import numpy as np
from scipy.sparse import csr_matrix, vstack
from sklearn.metrics import average_precision_score

REF = "/root/reference"
HERE = os.path.dirname(os.path.abspath(__file__))
NS = {"np": np, "average_precision_score": average_precision_score}


def extract(path, name):
    """The top-level `def name` of a reference file, compiled alone into the shared namespace."""
    src = open(os.path.join(REF, path)).read()
    fn = next(n for n in ast.parse(src).body if isinstance(n, ast.FunctionDef) and n.name == name)
    exec(compile(ast.Module(body=[fn], type_ignores=[]), os.path.join(REF, path), "exec"), NS)
    return NS[name]


get_item = extract("util_amazon_filtered.py", "get_item")
get_score = extract("fine_tune_ours.py", "get_score")
get_ave_score = extract("fine_tune_ours.py", "get_ave_score")
METRICS = {n: extract("test_amazon_filterd.py", n) for n in
           ("get_future_map", "get_cur_jaccard", "get_all_jaccard", "get_future_jaccard", "get_cur_recall", "get_all_recall",
            "get_future_recall")}
get_recall = extract("test_amazon_filterd.py", "get_recall")
to_binary = extract("test_amazon_filterd.py", "sequence_to_binary_vec")
find_K = extract("test_amazon_filterd.py", "find_K_sparse_dense")
normalize = extract("util_amazon_filtered.py", "normalize")

N_ITEMS, N_CORPUS, N_QUERY, K = 600, 400, 48, 20
# 0.25 and 0.5 are pair scores (get_recall's > is strict); 0.1 is one too, and float32(0.1) > 0.1: the comparison's width shows
THRES = np.array([0.0, 0.1, 0.25, 0.5], np.float64)


def click(rng, s):
    return (s, "c", None, int((rng.zipf(1.2) - 1) % N_ITEMS))


def corpus_sessions(rng, count):
    """Raw action tuples as in make_golden_sparse.py: 2..19 actions, 30 % searches, Zipf item draws that include item 0,
    repeats; every 25th session has searches only."""
    out = []
    for s in range(count):
        n = int(np.clip(2 + rng.poisson(6.0), 2, 19))
        out.append([(s, "s", "q", 0) if rng.random() < 0.3 or s % 25 == 7 else click(rng, s) for _ in range(n)])
    return out


def query_sessions(rng, count):
    """The same, but every session has a click; s % 12 == 3: the first half (seq) is searches only, s % 12 == 8: the
    second half (tar) is."""
    out = []
    for s in range(count):
        n = int(np.clip(2 + rng.poisson(6.0), 2, 19))
        cut = -(-n // 2)
        seq = [(s, "s", "q", 0) if rng.random() < 0.3 else click(rng, s) for _ in range(n)]
        if s % 12 == 3:
            seq[:cut] = [(s, "s", "q", 0)] * cut
            seq[n - 1] = click(rng, s)
        elif s % 12 == 8:
            seq[cut:] = [(s, "s", "q", 0)] * (n - cut)
            seq[0] = click(rng, s)
        elif not any(a[1] == "c" for a in seq):
            seq[0] = click(rng, s)
        out.append(seq)
    return out


def table(seqs, tag, out):
    out[f"{tag}_sess_ptr"] = np.cumsum([0] + [len(s) for s in seqs]).astype(np.int64)
    out[f"{tag}_is_search"] = np.array([a[1] == "s" for s in seqs for a in s], bool)
    out[f"{tag}_item_id"] = np.array([0 if a[1] == "s" else a[-1] for s in seqs for a in s], np.int64)


rng = np.random.default_rng(20261018)
corpus, queries = corpus_sessions(rng, N_CORPUS), query_sessions(rng, N_QUERY)
seqs = [q[:-(-len(q) // 2)] for q in queries]
tars = [q[-(-len(q) // 2):] for q in queries]
alls = [a + b for a, b in zip(seqs, tars)]
out = {"n_items": np.int64(N_ITEMS), "K": np.int64(K), "thres": THRES}
for seq_list, tag in ((corpus, "corpus"), (queries, "query"), (seqs, "seq"), (tars, "tar")):
    table(seq_list, tag, out)

# I: even rows from the reference's SKNN search on the cur vectors, odd rows seeded random ids
data = vstack([csr_matrix(normalize(to_binary(s, N_ITEMS).astype("float32"))) for s in corpus])
emb = normalize(np.array([to_binary(s, N_ITEMS) for s in seqs]).astype("float32"))
_, I = find_K(data, emb, K)
I = I.astype(np.int64)
I[1::2] = rng.integers(0, N_CORPUS, (N_QUERY // 2, K))
out["I"] = I

# ---- the conditions the fixture must satisfy, on the reference's own functions
sets = {"cur": [get_item(s) for s in seqs], "future": [get_item(s) for s in tars], "all": [get_item(s) for s in alls]}
csets = [get_item(s) for s in corpus]
hits = {p: np.array([[len(sets[p][i] & csets[I[i, j]]) > 0 for j in range(K)] for i in range(N_QUERY)]) for p in sets}
cond = {
    "every all set non-empty": all(len(s) > 0 for s in sets["all"]),
    "a query with an empty cur set": any(len(s) == 0 for s in sets["cur"]),
    "a query with an empty future set": any(len(s) == 0 for s in sets["future"]),
    "a search-only corpus session in I": any(len(csets[r]) == 0 for r in I.ravel()),
    "N >= K and no -1 in I": N_CORPUS >= K and int(I.min()) >= 0 and int(I.max()) < N_CORPUS,
}
for p in sets:
    cond[f"{p}: a query with no hit"] = bool((~hits[p].any(axis=1)).any())
    cond[f"{p}: a non-empty query with no hit"] = bool(any(len(sets[p][i]) and not hits[p][i].any() for i in range(N_QUERY)))
for p in ("cur", "all"):
    cond[f"{p}: a query with a hit at every rank"] = bool(hits[p].all(axis=1).any())
for name, ok in cond.items():
    print(f"{'ok ' if ok else 'FAILED'}  {name}")
print("future: queries with a hit at every rank:", int(hits["future"].all(axis=1).sum()), "(not required)")
assert all(cond.values())

# ---- the reference's values
test_data, pairs = (seqs, tars), list(zip(seqs, tars))
for name, fn in METRICS.items():
    out["ref_" + name[4:]] = np.float64(fn(I, test_data, corpus))
out["ref_cur_map"] = np.float64(METRICS["get_future_map"](I, (None, seqs), corpus))
out["ref_all_map"] = np.float64(METRICS["get_future_map"](I, (None, alls), corpus))
for sim in ("all_jaccard", "cur_jaccard"):
    v = get_ave_score(I, pairs, corpus, sim)
    assert v.dtype == np.float32                                   # a float32 mean: the bound of the test follows from it
    out[f"ref_ave_{sim}"] = np.float64(v)
    # thres as the Python float a caller passes: `gt > thres` is then a float32 comparison under either numpy promotion rule
    out[f"ref_recall_{sim}"] = np.array([get_recall(pairs, corpus, I, sim, float(t)) for t in THRES], np.float64)
for k in sorted(out):
    if k.startswith("ref_"):
        print(k, out[k])
assert (np.diff(out["ref_recall_all_jaccard"]) < 0).all()           # every threshold separates some pairs
np.savez_compressed(os.path.join(HERE, "eval_metrics.npz"), **out)
print("wrote eval_metrics.npz:", os.path.getsize(os.path.join(HERE, "eval_metrics.npz")), "bytes")
