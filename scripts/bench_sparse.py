"""Dev helper: the sparse session index (SKNN / STAN baselines) at 1M synthetic sessions x 1024 queries, k = 100.
Prints one JSON line, per mode:
  search_ms                 sss_sparse_topk over the whole batch (all query chunks): hipEvent median after warm-up
  score_kernel_ms, topk_ms  the same search's kernels, summed per repetition from the profiler's device durations,
                            median over the repetitions after warm-up (the top-k is not callable on its own)
  score_traffic_bound_ms    the score matrix's own traffic, 2 * nq * n * 4 bytes (written once, read once), at 8 TB/s
  host_restatement_ms       the reference's algorithm on the host (scipy CSR . dense per query, argsort + sort, as
                            find_K_sparse_dense does it; single-threaded, as scipy's product is) on the first
                            --host-queries queries, scaled to the batch
and for the builder the device time of its two kernels (binary, 1M sessions) beside the wall time of
session_vectors, which also uploads the action table and reads the total back (medians after warm-up, both).
--lib PATH times another build of libsss.so with the same C ABI (another commit's: DESIGN.md 5.11)."""
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
from sessionsimilaritysearch_amd import _lib, sparse  # noqa: E402
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
                found = KERNEL_NAME.search(e.name)               # "void sss::k_topk_radix<1024>(...)" -> "k_topk_radix"
                name = found.group(0) if found else e.name
                one[name] = one.get(name, 0.0) + e.device_time / 1e3
        runs.append(one)
    return {k: float(np.median([r.get(k, 0.0) for r in runs])) for k in set().union(*runs)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1000000)
    ap.add_argument("--nq", type=int, default=1024)
    ap.add_argument("--k", type=int, default=100)
    ap.add_argument("--lammy", type=float, default=1.04)
    ap.add_argument("--host-queries", type=int, default=8)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--lib", default=None)
    a = ap.parse_args()
    if a.lib:
        _lib.LIB_PATH = os.path.abspath(a.lib)
    dev = torch.device("cuda", 0)
    corpus_actions, query_actions = synthetic_actions(a.n, 1), synthetic_actions(a.nq, 2)
    out = {"n": a.n, "nq": a.nq, "k": a.k, "n_items": ASIN_NUM, "reps": a.reps, "lib": _lib.LIB_PATH if a.lib else "default"}
    build = lambda: sparse.session_vectors(corpus_actions, "binary", device=dev)
    kb = kernel_medians_ms(build, 1, 3)
    out["builder_kernels_ms"] = {k: round(v, 4) for k, v in kb.items() if "k_svec" in k}
    if len(out["builder_kernels_ms"]) != 2:
        raise RuntimeError(f"builder kernels not found in the profile: {sorted(kb)}")
    walls = []
    for _ in range(a.reps):                              # warm: the profiled runs above already built it four times
        torch.cuda.synchronize(); t0 = time.perf_counter(); corpus = build(); torch.cuda.synchronize()
        walls.append((time.perf_counter() - t0) * 1e3)
    out["session_vectors_wall_ms"] = float(np.median(walls))
    index = sparse.SparseSessionIndex(ASIN_NUM, dev).add(corpus)
    out["corpus_nnz"] = int(corpus.items.numel())
    from scipy.sparse import csr_matrix
    p, it, w = corpus.to_numpy()
    host = csr_matrix((w, it, p), shape=(a.n, ASIN_NUM))
    bound = 2.0 * a.nq * a.n * 4 / HBM_BYTES_PER_S * 1e3
    for mode in ("binary", "stan"):
        q = sparse.session_vectors(query_actions, mode, a.lammy if mode == "stan" else None, dev)
        D, I = index.search_device(q, a.k)
        run = lambda: index.search_device(q, a.k, D, I)
        total = event_median_ms(run, 2, a.reps)
        kern = kernel_medians_ms(run, 1, a.reps)
        if "k_sparse_scores" not in kern or "k_topk_radix" not in kern:
            raise RuntimeError(f"search kernels not found in the profile: {sorted(kern)}")
        score = kern["k_sparse_scores"]
        topk = sum(v for name, v in kern.items() if name != "k_sparse_scores")
        dq = np.zeros((a.host_queries, ASIN_NUM), np.float32)
        qp, qi, qw = q.to_numpy()
        for f in range(a.host_queries):
            dq[f, qi[qp[f]:qp[f + 1]]] = qw[qp[f]:qp[f + 1]]
        t0 = time.perf_counter()
        for f in range(a.host_queries):
            val = np.squeeze(host.dot(dq[f]))
            np.argsort(val)[-a.k:][::-1]; np.sort(val)[-a.k:][::-1]
        host_ms = (time.perf_counter() - t0) * 1e3 / a.host_queries * a.nq
        out[mode] = {"search_ms": total, "score_kernel_ms": score, "topk_ms": topk, "chunks": index.last_chunks,
                     "kernels_ms": {k: round(v, 4) for k, v in sorted(kern.items())},
                     "score_traffic_bound_ms": bound, "score_kernel_over_bound": score / bound,
                     "host_restatement_ms": host_ms, "host_queries_timed": a.host_queries,
                     "device_beats_host": bool(total < host_ms)}
    out["host_threads"] = 1
    out["host_cores_available"] = len(os.sched_getaffinity(0))
    print(json.dumps(out))
    if not all(out[m]["device_beats_host"] for m in ("binary", "stan")):
        raise SystemExit("the device search did not beat the host restatement")


if __name__ == "__main__":
    main()
