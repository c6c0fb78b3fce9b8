"""Dev helper: scoring a search result (sessionsimilaritysearch_amd/evaluation.py) at 1M synthetic corpus sessions x 100k
queries, K = 100.  I holds seeded random ids (of sessions with at least one item): no two neighbours of a query share
a cache line, the worst case of the gather (a real result's neighbours share items, not addresses, so it is no better
placed).  Prints one JSON line:
  item_overlap_ms           sss_item_overlap alone on the `all` part (hipEvent median after warm-up), with pairs_per_s
  overlap_metrics_ms        sss_overlap_metrics on its outputs
  min_bytes_per_pair        the algorithmic minimum 16 + 4 |C_r| + 8 (two ptr words, the row, the id), averaged over the
                            pairs; min_traffic_ms is that at 8 TB/s, overlap_over_min_traffic the kernel's multiple of it
  evaluate_wall_ms          evaluate(): three parts, six launches, the copies of nq doubles and the numpy means (wall clock
                            around a synchronise, median)
  host_restatement_ms       tests/helpers/eval_ref.evaluate (python sets, the canonical loop) on the first
                            --host-queries queries, scaled to the batch"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import eval_ref  # noqa: E402
from sessionsimilaritysearch_amd import evaluation, sparse  # noqa: E402
from sessionsimilaritysearch_amd.sessions import synthetic_actions  # noqa: E402

HBM_BYTES_PER_S = 8.0e12


def event_median_ms(fn, warmup, reps):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); fn(); b.record(); b.synchronize()
        ts.append(a.elapsed_time(b))
    return float(np.median(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1000000)
    ap.add_argument("--nq", type=int, default=100000)
    ap.add_argument("--k", type=int, default=100)
    ap.add_argument("--host-queries", type=int, default=200)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    corpus = sparse.session_vectors(synthetic_actions(a.n, 1), "binary", device=dev)
    seq, tar = synthetic_actions(a.nq, 2).split(1, 2)
    parts = evaluation.query_parts(seq, tar, dev)
    # ids of sessions with an item: a search-only query against a search-only neighbour is the empty union on which
    # get_all_jaccard divides by zero, in the reference and here
    with_item = torch.nonzero(corpus.ptr[1:] > corpus.ptr[:-1]).flatten()
    I = with_item[torch.from_numpy(np.random.default_rng(3).integers(0, with_item.numel(), (a.nq, a.k))).to(dev)].contiguous()
    pairs = a.nq * a.k
    out = {"n": a.n, "nq": a.nq, "k": a.k, "reps": a.reps, "pairs": pairs, "corpus_nnz": int(corpus.items.numel()),
           "mean_query_items": {p: float(getattr(parts, p).items.numel()) / a.nq for p in evaluation.PARTS}}

    L, st, q = evaluation._lib.lib(), evaluation._lib.stream_ptr(dev), parts.all
    inter = torch.empty((a.nq, a.k), dtype=torch.int32, device=dev)
    csize, err = torch.empty_like(inter), torch.zeros(1, dtype=torch.int32, device=dev)
    qsize = (q.ptr[1:] - q.ptr[:-1]).to(torch.int32)
    sums, flags = torch.empty((a.nq, 4), dtype=torch.float64, device=dev), torch.empty(a.nq, dtype=torch.int32, device=dev)

    def overlap():
        evaluation._lib.check(L.sss_item_overlap(q.ptr.data_ptr(), q.items.data_ptr(), a.nq, corpus.ptr.data_ptr(), corpus.items.data_ptr(),
                                                 a.n, I.data_ptr(), a.k, 0, inter.data_ptr(), csize.data_ptr(), err.data_ptr(), st),
                              "sss_item_overlap")

    def reduce():
        evaluation._lib.check(L.sss_overlap_metrics(inter.data_ptr(), csize.data_ptr(), qsize.data_ptr(), a.nq, a.k, 0.5, sums.data_ptr(),
                                                    flags.data_ptr(), st), "sss_overlap_metrics")
    out["item_overlap_ms"] = event_median_ms(overlap, 2, a.reps)
    out["overlap_metrics_ms"] = event_median_ms(reduce, 2, a.reps)
    out["pairs_per_s"] = pairs / (out["item_overlap_ms"] * 1e-3)
    out["min_bytes_per_pair"] = 24.0 + 4.0 * float(csize.double().mean().item())
    out["min_traffic_ms"] = pairs * out["min_bytes_per_pair"] / HBM_BYTES_PER_S * 1e3
    out["overlap_over_min_traffic"] = out["item_overlap_ms"] / out["min_traffic_ms"]
    out["min_bytes_per_s_achieved"] = pairs * out["min_bytes_per_pair"] / (out["item_overlap_ms"] * 1e-3)

    walls = []
    for _ in range(a.reps + 1):
        torch.cuda.synchronize(); t0 = time.perf_counter(); res = evaluation.evaluate(I, parts, corpus, 0.5); torch.cuda.synchronize()
        walls.append((time.perf_counter() - t0) * 1e3)
    out["evaluate_wall_ms"] = float(np.median(walls[1:]))
    out["evaluate"] = {k: round(v, 6) for k, v in res.items()}

    h = a.host_queries
    cut = lambda v: (v.ptr[:h + 1].cpu().numpy(), v.items.cpu().numpy())
    host_parts = {p: cut(getattr(parts, p)) for p in evaluation.PARTS}
    host_corpus, host_I = (corpus.ptr.cpu().numpy(), corpus.items.cpu().numpy()), I[:h].cpu().numpy()
    t0 = time.perf_counter()
    eval_ref.evaluate(host_I, host_parts, host_corpus, 0.5)
    out["host_restatement_ms"] = (time.perf_counter() - t0) * 1e3 / h * a.nq
    out["host_queries_timed"] = h
    out["device_beats_host"] = bool(out["evaluate_wall_ms"] < out["host_restatement_ms"])
    print(json.dumps(out))
    if not out["device_beats_host"]:
        raise SystemExit("evaluate() did not beat the host restatement")


if __name__ == "__main__":
    main()
