"""Time FlatIndex.range_search against search(x, 100) on a 1M x 128 index of unit rows, 1024 queries.

Two radii: one keeping about 10 rows per query, one about 1000 (picked from the scores of the first queries' top 1024).
Device events around each call (warmed up), median of --iters calls.  Prints one JSON line: ms per call, results per
query, the route and the overflow count of every range search.
--metric l2 has no fused range route: it times the exhaustive range kernels (scores, count, scan, compact).
--lib PATH times another build of libsss.so with the same C ABI (another commit's).
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from sessionsimilaritysearch_amd import _lib  # noqa: E402
from sessionsimilaritysearch_amd.index import FlatIndex, normalize_  # noqa: E402


def _median_ms(fn, warmup, iters):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        times.append(e0.elapsed_time(e1))
    return float(np.median(times))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--d", type=int, default=128)
    ap.add_argument("--nq", type=int, default=1024)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--metric", choices=("ip", "l2"), default="ip")
    ap.add_argument("--lib", default=None)
    a = ap.parse_args()
    if a.lib:
        _lib.LIB_PATH = os.path.abspath(a.lib)
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev)
    g.manual_seed(7)
    c = torch.randn((a.n, a.d), device=dev, generator=g)
    normalize_(c)
    q = torch.randn((a.nq, a.d), device=dev, generator=g)
    normalize_(q)
    idx = FlatIndex(a.d, a.metric, dev).adopt(c)

    out = {"n": a.n, "d": a.d, "nq": a.nq, "iters": a.iters, "metric": a.metric, "lib": _lib.LIB_PATH if a.lib else "default"}
    # radii: the 10th / 1000th best score (smallest distance), averaged over the first 64 queries (the index's own exact search)
    Dk, _ = idx.search(q[:64], 1024)
    radii = {"r10": float(Dk[:, 9].mean()), "r1000": float(Dk[:, 999].mean())}
    for name, r in radii.items():
        res = {}

        def call():
            res["out"] = idx.range_search(q, r)

        ms = _median_ms(call, a.warmup, a.iters)
        lims = res["out"][0]
        out[name] = {"radius": round(r, 6), "ms": round(ms, 4), "results_per_query": round(float(lims[-1]) / a.nq, 2),
                     "route": idx.last_range_scan, "overflow_queries": idx.last_range_overflow_queries}
    ms = _median_ms(lambda: idx.search(q, 100), a.warmup, a.iters)
    out["search_k100"] = {"ms": round(ms, 4), "scan": idx.last_scan, "rescan_queries": idx.last_rescan_queries}
    for name in radii:
        out[name]["vs_search_k100"] = round(out[name]["ms"] / ms, 3)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
