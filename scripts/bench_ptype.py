"""Dev helper: the product-type index (exact cosine of product-type count vectors, include/sss_ptype.h) beside the item-set
JaccardIndex at the same corpus and query counts: 1M synthetic sessions x 1024 queries, k = 100, edges (0.2, 0.8).  The
sessions are synthetic_actions' (Zipf(1.2) item draws); every item gets one of --types product types of Zipf-like
popularity from a seeded table, a tenth of the items none.  Prints one JSON line; for each of "ptype" and "jaccard":
  build_ms                   type_bags / session_vectors over the corpus' action table (wall clock, one call after a warm-up)
  search_ms                  index.search over the whole batch (all query chunks): hipEvent median after warm-up
  score_kernel_ms, topk_ms   the same search's kernels, summed per repetition from the profiler's device durations
  bands_ms                   index.bands (its two memsets and the band kernel): hipEvent median
  mine_triples_ms            mine_triples: bands, one pair-score launch and the copies to the host; wall clock, median
and "ratio": ptype / jaccard of each figure.  The weighted walk stages 16 (type, count) entries a row where the item-set walk
stages 32 items; type bags are shorter than item sets (several items share a type), which the two nnz figures show.
A report, not a gate.  --lib PATH times another build of libsss.so with the same C ABI (another commit's)."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bench_jaccard import event_median_ms, kernel_medians_ms, wall_median_ms  # noqa: E402
from sessionsimilaritysearch_amd import _lib, jaccard, product_types, sparse  # noqa: E402
from sessionsimilaritysearch_amd.sessions import ASIN_NUM, synthetic_actions  # noqa: E402


def type_table(n_types, seed):
    """item -> type, int32 [ASIN_NUM]: Zipf-like popularity over n_types types, a tenth of the items without a type (-1)."""
    rng = np.random.default_rng(seed)
    ty = ((rng.zipf(1.3, ASIN_NUM) - 1) % n_types).astype(np.int32)
    ty[rng.random(ASIN_NUM) < 0.1] = -1
    return ty


def wall_ms(fn):
    fn()
    torch.cuda.synchronize(); t0 = time.perf_counter(); fn(); torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def measure(index, q, k, edges, score_kernel, reps):
    D, I = index.search_device(q, k)
    run = lambda: index.search_device(q, k, D, I)
    search = event_median_ms(run, 2, reps)
    kern = kernel_medians_ms(run, 1, reps)
    if score_kernel not in kern or "k_topk_radix" not in kern:
        raise RuntimeError(f"search kernels not found in the profile: {sorted(kern)}")
    bands = event_median_ms(lambda: index.bands(q, edges), 2, reps)
    counts, _ = index.bands(q, edges)
    mine = wall_median_ms(lambda: jaccard.mine_triples(index, q, *edges), 1, reps)
    return {"search_ms": search, "search_chunks": index.last_chunks, "score_kernel_ms": kern[score_kernel],
            "topk_ms": sum(v for name, v in kern.items() if name != score_kernel), "bands_ms": bands, "mine_triples_ms": mine,
            "band_rows_per_query": [round(float(x), 2) for x in counts.double().mean(0).tolist()],
            "triples_kept": int(jaccard.mine_triples(index, q, *edges).keep.sum())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1000000)
    ap.add_argument("--nq", type=int, default=1024)
    ap.add_argument("--k", type=int, default=100)
    ap.add_argument("--types", type=int, default=500)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--lib", default=None)
    a = ap.parse_args()
    if a.lib:
        _lib.LIB_PATH = os.path.abspath(a.lib)
    dev = torch.device("cuda", 0)
    edges = (0.2, 0.8)
    ca, qa = synthetic_actions(a.n, 1), synthetic_actions(a.nq, 2)
    ty = torch.from_numpy(type_table(a.types, 3)).to(dev)
    out = {"n": a.n, "nq": a.nq, "k": a.k, "edges": edges, "n_items": ASIN_NUM, "n_types": a.types, "reps": a.reps,
           "lib": _lib.LIB_PATH if a.lib else "default"}
    cb, qb = product_types.type_bags(ca, ty, a.types, dev), product_types.type_bags(qa, ty, a.types, dev)
    cs, qs = sparse.session_vectors(ca, "binary", device=dev), sparse.session_vectors(qa, "binary", device=dev)
    pi = product_types.ProductTypeIndex(a.types, dev).add(cb)
    ji = jaccard.JaccardIndex(ASIN_NUM, dev).add(cs)
    out["ptype"] = {"corpus_nnz": int(cb.items.numel()), "query_nnz": int(qb.items.numel()),
                    "rows_longer_than_16": int(((cb.ptr[1:] - cb.ptr[:-1]) > 16).sum().item()),
                    "build_ms": wall_ms(lambda: product_types.type_bags(ca, ty, a.types, dev)), **measure(pi, qb, a.k, edges, "k_ptype_scores", a.reps)}
    out["jaccard"] = {"corpus_nnz": int(cs.items.numel()), "query_nnz": int(qs.items.numel()),
                      "rows_longer_than_32": int(((cs.ptr[1:] - cs.ptr[:-1]) > 32).sum().item()),
                      "build_ms": wall_ms(lambda: sparse.session_vectors(ca, "binary", device=dev)), **measure(ji, qs, a.k, edges, "k_jaccard_scores", a.reps)}
    out["ratio"] = {key: round(out["ptype"][key] / out["jaccard"][key], 4)
                    for key in ("build_ms", "search_ms", "score_kernel_ms", "topk_ms", "bands_ms", "mine_triples_ms")}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
