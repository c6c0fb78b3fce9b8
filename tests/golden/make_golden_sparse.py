"""Generates tests/golden/sparse_baselines.npz by RUNNING the reference's own SKNN / STAN functions on seeded sessions.
Build container only (needs /root/reference and scipy):  python tests/golden/make_golden_sparse.py

As in make_golden_pure.py each `def` is located in its file's syntax tree, compiled alone into a namespace holding only
numpy, and called; nothing of the reference's text is written anywhere.  The .npz holds the inputs (an action table),
the vectors the reference built from them in CSR form (indices + float32 values) and its (D, I) for both modes:

  sequence_to_binary_vec  test_amazon_filterd.py:48-57
  sequence_to_stan_vec    test_amazon_filterd.py:37-46
  find_K_sparse_dense     test_amazon_filterd.py:403-412
  normalize               util_amazon_filtered.py:28-31

and the steps of main2's 'SKNN' / 'STAN' branch (:582-603) around them: astype('float32'), normalize, csr_matrix, vstack.
"""
import ast
import os

import numpy as np
from scipy.sparse import csr_matrix, vstack

REF = "/root/reference"
HERE = os.path.dirname(os.path.abspath(__file__))


def extract(path, name):
    """The top-level `def name` of a reference file, compiled alone (as make_golden_pure.py does)."""
    src = open(os.path.join(REF, path)).read()
    fn = next(n for n in ast.parse(src).body if isinstance(n, ast.FunctionDef) and n.name == name)
    ns = {"np": np}
    exec(compile(ast.Module(body=[fn], type_ignores=[]), os.path.join(REF, path), "exec"), ns)
    return ns[name], (fn.lineno, fn.end_lineno)


to_binary, _ = extract("test_amazon_filterd.py", "sequence_to_binary_vec")
to_stan, _ = extract("test_amazon_filterd.py", "sequence_to_stan_vec")
find_K, _ = extract("test_amazon_filterd.py", "find_K_sparse_dense")
normalize, _ = extract("util_amazon_filtered.py", "normalize")

N_ITEMS, N_CORPUS, N_QUERY, K, LAMMY = 600, 400, 48, 20, 1.04


def sessions(rng, count):
    """Raw action tuples (session id, 's' or 'c', query text or None, item id): 2..19 actions, 30 % searches, Zipf item
    draws that include item 0, repeats; every 25th session has searches only."""
    out = []
    for s in range(count):
        seq = []
        for _ in range(int(np.clip(2 + rng.poisson(6.0), 2, 19))):
            if rng.random() < 0.3 or s % 25 == 7:
                seq.append((s, "s", "q", 0))
            else:
                seq.append((s, "c", None, int((rng.zipf(1.2) - 1) % N_ITEMS)))
        out.append(seq)
    return out


def table(seqs, tag, out):
    out[f"{tag}_sess_ptr"] = np.cumsum([0] + [len(s) for s in seqs]).astype(np.int64)
    out[f"{tag}_is_search"] = np.array([a[1] == "s" for s in seqs for a in s], bool)
    out[f"{tag}_item_id"] = np.array([0 if a[1] == "s" else a[-1] for s in seqs for a in s], np.int64)


def csr_out(m, tag, out):
    m = csr_matrix(m)
    m.sort_indices()
    out[f"{tag}_ptr"], out[f"{tag}_items"], out[f"{tag}_weights"] = m.indptr.astype(np.int64), m.indices.astype(np.int32), m.data.astype(np.float32)


rng = np.random.default_rng(20261017)
corpus, queries = sessions(rng, N_CORPUS), sessions(rng, N_QUERY)
out = {"n_items": np.int64(N_ITEMS), "K": np.int64(K), "lammy": np.float64(LAMMY)}
table(corpus, "corpus", out)
table(queries, "query", out)
data = vstack([csr_matrix(normalize(to_binary(seq, N_ITEMS).astype("float32"))) for seq in corpus])
csr_out(data, "ref_corpus", out)
for mode in ("SKNN", "STAN"):
    if mode == "STAN":
        emb = np.array([to_stan(seq, N_ITEMS, LAMMY) for seq in queries]).astype("float32")
    else:
        emb = np.array([to_binary(seq, N_ITEMS) for seq in queries]).astype("float32")
    emb = normalize(emb)
    D, I = find_K(data, emb, K)
    csr_out(emb, f"ref_query_{mode}", out)
    out[f"D_{mode}"], out[f"I_{mode}"] = D, I
    tied = int(sum(np.sum(data.dot(emb[i]) == D[i, -1]) > 1 for i in range(N_QUERY)))
    print(mode, "queries tied at rank K:", tied, "of", N_QUERY)
np.savez_compressed(os.path.join(HERE, "sparse_baselines.npz"), **out)
print("wrote sparse_baselines.npz:", os.path.getsize(os.path.join(HERE, "sparse_baselines.npz")), "bytes")
