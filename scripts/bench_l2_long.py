"""Time the L2 search of a float32 FlatIndex with LONG rows (the reference's own D = 1600, K = 100) on three routes:

  (a) ``l2_long``     the L2 search as ``search_device`` runs it: the K-tiled long-row scan (``sss_l2_topk_long``) plus
                      whatever it leaves to the exhaustive kernels;
  (b) ``exhaustive``  ``search_exhaustive`` called directly on the same index: what every L2 search of such rows ran on
                      before the long-row L2 scan existed;
  (c) ``ip_long``     the inner-product search of the same rows and queries on the long-row scan (``sss_ip_topk_long``).

1M x 1600 rows, Gaussian directions with row norms log-uniform in [1/4, 4] (queries likewise), 1024 queries.  The three
routes run in one process, alternating call by call (a, b, c, a, b, c, ...), device events around each call, median of
--iters calls each after --warmup rounds.  Prints one JSON line: ms per call, the unproven / fallback counts, (b) / (a)
and (a) / (c).
"""
import argparse
import json
import math
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from sessionsimilaritysearch_amd.index import FlatIndex  # noqa: E402


def _varnorm(n, d, dev, g):
    x = torch.randn((n, d), device=dev, generator=g)
    s = torch.exp(torch.empty(n, device=dev).uniform_(math.log(.25), math.log(4), generator=g))
    x *= (s / x.norm(dim=1)).unsqueeze(1)
    return x


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--d", type=int, default=1600)
    ap.add_argument("--nq", type=int, default=1024)
    ap.add_argument("--k", type=int, default=100)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev)
    g.manual_seed(1600)
    c = _varnorm(a.n, a.d, dev, g)
    q = _varnorm(a.nq, a.d, dev, g)
    k = a.k

    l2 = FlatIndex(a.d, "l2", dev).adopt(c)
    ip = FlatIndex(a.d, "ip", dev).adopt(c)
    if l2.prepare(k) != "long" or ip.prepare(k) != "long":
        raise SystemExit(f"not a long-row shape: l2 route {l2._route(k)!r}, ip route {ip._route(k)!r}")
    D = torch.empty((a.nq, k), dtype=torch.float32, device=dev)
    I = torch.empty((a.nq, k), dtype=torch.int64, device=dev)
    routes = {"l2_long": lambda: l2.search_device(q, k),
              "exhaustive": lambda: l2.search_exhaustive(q, k, D, I),
              "ip_long": lambda: ip.search_device(q, k)}
    times = {name: [] for name in routes}
    for it in range(a.warmup + a.iters):
        for name, fn in routes.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            if it >= a.warmup:
                times[name].append(e0.elapsed_time(e1))
    # the two L2 routes must agree (both are exact): a cheap guard against timing a route that computes something else
    Dl, Il = l2.search_device(q, k)
    l2.search_exhaustive(q, k, D, I)
    same = bool(torch.equal(Dl, D)) and bool(torch.equal(Il, I))
    ms = {name: float(np.median(t)) for name, t in times.items()}
    out = {"n": a.n, "d": a.d, "nq": a.nq, "k": k, "iters": a.iters,
           "l2_long": {"ms": round(ms["l2_long"], 4), "min_ms": round(min(times["l2_long"]), 4), "scan": l2.last_scan,
                       "unproven_queries": l2.last_rescan_queries, "fallback_queries": l2.last_fallback_queries},
           "exhaustive": {"ms": round(ms["exhaustive"], 3), "min_ms": round(min(times["exhaustive"]), 3)},
           "ip_long": {"ms": round(ms["ip_long"], 4), "min_ms": round(min(times["ip_long"]), 4), "scan": ip.last_scan,
                       "unproven_queries": ip.last_rescan_queries, "fallback_queries": ip.last_fallback_queries},
           "exhaustive_over_l2_long": round(ms["exhaustive"] / ms["l2_long"], 2),
           "l2_long_over_ip_long": round(ms["l2_long"] / ms["ip_long"], 3),
           "l2_routes_agree": same}
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
