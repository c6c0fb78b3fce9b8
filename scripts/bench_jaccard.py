"""Dev helper: the ground-truth index (exact item-set Jaccard) at 1M synthetic sessions x 1024 queries, k = 100, edges
(0.2, 0.8), on two corpora: "zipf", the sessions of synthetic_actions (Zipf(1.2) item draws: most pairs share the head
item), and "uniform", the same row lengths with item draws uniform over the 391 572 ids (most pairs share nothing).
Prints one JSON line; per corpus:
  search_ms                  JaccardIndex.search over the whole batch (all query chunks): hipEvent median after warm-up
  score_kernel_ms, topk_ms   the same search's kernels, summed per repetition from the profiler's device durations
  bands_ms                   JaccardIndex.bands (its two memsets and k_jaccard_bands): hipEvent median
  mine_triples_ms            mine_triples: bands, one item_overlap launch and the copies to the host; wall clock, median
  sparse_search_ms           SparseSessionIndex.search on the same sets with binary weights, same process: the nearest
                             thing the library had before this index (k_sparse_scores + the same top-k)
  score_traffic_bound_ms     the score matrix's own traffic, 2 * nq * n * 4 bytes (written once, read once), at 8 TB/s
  bands_traffic_bound_ms     the corpus ptr and items once per query range, no output matrix, at 8 TB/s
  host_restatement_ms        the reference's algorithm on the host -- get_score's python sets, one pair at a time, single
                             thread -- on --host-queries x --host-rows pairs, SCALED to nq x n
--lib PATH times another build of libsss.so with the same C ABI (another commit's, or an experiment's: DESIGN.md 5.7)."""
import argparse
import json
import os
import re
import sys
import time

import numpy as np
import torch
from torch.profiler import ProfilerActivity, profile

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sessionsimilaritysearch_amd import _lib, jaccard, sparse  # noqa: E402
from sessionsimilaritysearch_amd.sessions import ASIN_NUM, synthetic_actions  # noqa: E402

HBM_BYTES_PER_S = 8.0e12
KERNEL_NAME = re.compile(r"\bk_[A-Za-z0-9_]+")


def event_median_ms(fn, warmup, reps):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); fn(); b.record(); b.synchronize()
        ts.append(a.elapsed_time(b))
    return float(np.median(ts))


def wall_median_ms(fn, warmup, reps):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize(); t0 = time.perf_counter(); fn(); torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts))


def kernel_medians_ms(fn, warmup, reps):
    """{kernel name: median over reps of its summed device time in one fn()} (names without arguments / namespaces)."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    runs = []
    for _ in range(reps):
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        one = {}
        for e in prof.events():
            if e.device_type == torch.autograd.DeviceType.CUDA:
                found = KERNEL_NAME.search(e.name)
                name = found.group(0) if found else e.name
                one[name] = one.get(name, 0.0) + e.device_time / 1e3
        runs.append(one)
    return {k: float(np.median([r.get(k, 0.0) for r in runs])) for k in set().union(*runs)}


def uniform_like(ptr, seed):
    """Host item sets with (nearly) the row lengths of `ptr` and item draws uniform over the vocabulary: (ptr, items)."""
    rng = np.random.default_rng(seed)
    row = np.repeat(np.arange(len(ptr) - 1, dtype=np.int64), np.diff(ptr))
    key = np.unique(row * ASIN_NUM + rng.integers(0, ASIN_NUM, row.size))       # sorted by (row, item); a repeat in a row drops out
    out = np.zeros(len(ptr), np.int64)
    np.cumsum(np.bincount(key // ASIN_NUM, minlength=len(ptr) - 1), out=out[1:])
    return out, (key % ASIN_NUM).astype(np.int32)


def binary_vectors(ptr, items, dev):
    """SessionVectors of host item sets with sequence_to_binary_vec's weights, float32(1 / sqrt(m))."""
    m = np.diff(ptr)
    w = np.repeat((1.0 / np.sqrt(np.maximum(m, 1).astype(np.float64))).astype(np.float32), m)
    return sparse._device_triple(ptr, items, w, dev)


def host_ms_scaled(q, c, host_queries, host_rows, nq, n):
    qp, qi, _ = q.to_numpy()
    cp, ci, _ = c.to_numpy()
    qs = [set(qi[qp[f]:qp[f + 1]].tolist()) for f in range(min(host_queries, len(qp) - 1))]
    cs = [set(ci[cp[r]:cp[r + 1]].tolist()) for r in range(min(host_rows, len(cp) - 1))]
    t0 = time.perf_counter()
    for a in qs:
        for b in cs:
            u = len(a | b)
            _ = 0 if u == 0 else len(a & b) / u
    return (time.perf_counter() - t0) * 1e3 / (len(qs) * len(cs)) * nq * n, len(qs) * len(cs)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1000000)
    ap.add_argument("--nq", type=int, default=1024)
    ap.add_argument("--k", type=int, default=100)
    ap.add_argument("--host-queries", type=int, default=8)
    ap.add_argument("--host-rows", type=int, default=20000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--lib", default=None)
    a = ap.parse_args()
    if a.lib:
        _lib.LIB_PATH = os.path.abspath(a.lib)
    dev = torch.device("cuda", 0)
    edges = (0.2, 0.8)
    zc = sparse.session_vectors(synthetic_actions(a.n, 1), "binary", device=dev)
    zq = sparse.session_vectors(synthetic_actions(a.nq, 2), "binary", device=dev)
    corpora = {"zipf": (zc, zq),
               "uniform": (binary_vectors(*uniform_like(zc.ptr.cpu().numpy(), 3), dev), binary_vectors(*uniform_like(zq.ptr.cpu().numpy(), 4), dev))}
    out = {"n": a.n, "nq": a.nq, "k": a.k, "edges": edges, "n_items": ASIN_NUM, "reps": a.reps, "lib": _lib.LIB_PATH if a.lib else "default"}
    ok = True
    for name, (c, q) in corpora.items():
        index = jaccard.JaccardIndex(ASIN_NUM, dev).add(c)
        base = sparse.SparseSessionIndex(ASIN_NUM, dev).add(c)
        D, I = index.search_device(q, a.k)
        run = lambda: index.search_device(q, a.k, D, I)
        search = event_median_ms(run, 2, a.reps)
        kern = kernel_medians_ms(run, 1, a.reps)
        if "k_jaccard_scores" not in kern or "k_topk_radix" not in kern:
            raise RuntimeError(f"search kernels not found in the profile: {sorted(kern)}")
        bands = event_median_ms(lambda: index.bands(q, edges), 2, a.reps)
        counts, _ = index.bands(q, edges)
        inter = event_median_ms(lambda: index.bands(q, (np.nextafter(0.0, 1.0),)), 1, 1)
        nonzero = int(index.bands(q, (np.nextafter(0.0, 1.0),))[0][:, 1].sum().item())
        mine = wall_median_ms(lambda: jaccard.mine_triples(index, q, *edges), 1, a.reps)
        kept = int(jaccard.mine_triples(index, q, *edges).keep.sum())
        Ds, Is = base.search_device(q, a.k)
        sp = event_median_ms(lambda: base.search_device(q, a.k, Ds, Is), 2, a.reps)
        spk = kernel_medians_ms(lambda: base.search_device(q, a.k, Ds, Is), 1, a.reps)
        host, pairs = host_ms_scaled(q, c, a.host_queries, a.host_rows, a.nq, a.n)
        nnz = int(c.items.numel())
        res = {"corpus_nnz": nnz, "query_nnz": int(q.items.numel()), "pairs_with_a_shared_item": nonzero / (a.n * a.nq),
               "band_rows_per_query": [round(float(x), 2) for x in counts.double().mean(0).tolist()], "triples_kept": kept,
               "search_ms": search, "search_chunks": index.last_chunks, "score_kernel_ms": kern["k_jaccard_scores"],
               "topk_ms": sum(v for k, v in kern.items() if k != "k_jaccard_scores"), "bands_ms": bands, "bands_one_edge_ms": inter,
               "mine_triples_ms": mine, "sparse_search_ms": sp, "sparse_score_kernel_ms": spk.get("k_sparse_scores"),
               "score_traffic_bound_ms": 2.0 * a.nq * a.n * 4 / HBM_BYTES_PER_S * 1e3,
               "bands_traffic_bound_ms": (nnz * 4 + (a.n + 1) * 8) / HBM_BYTES_PER_S * 1e3,
               "host_restatement_ms": host, "host_pairs_timed": pairs,
               "search_beats_host": bool(search < host), "bands_beats_host": bool(bands < host), "bands_not_slower_than_search": bool(bands <= search)}
        ok = ok and res["search_beats_host"] and res["bands_beats_host"]
        out[name] = res
    out["host_threads"] = 1
    print(json.dumps(out))
    if not ok:
        raise SystemExit("a device call did not beat the host restatement")


if __name__ == "__main__":
    main()
