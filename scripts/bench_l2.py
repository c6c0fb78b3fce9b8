"""Time the L2 search of a float32 FlatIndex per candidate scan, against the inner-product search of the same rows on
the same scan and against the exhaustive route (``search_exhaustive`` called directly: what every L2 search ran on before
the L2 scans existed).

1M x 128 standard-normal rows, 1024 queries, k = 10 and 100.  Device events around each call (warmed up), median of
--iters calls.  Prints one JSON line: ms per call and the unproven counts of every leg, the L2 / IP ratio per scan and
the speed-up over the exhaustive route.
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from sessionsimilaritysearch_amd.index import FlatIndex  # noqa: E402


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
    ap.add_argument("--exhaustive-iters", type=int, default=3, help="timed calls of the exhaustive route (seconds each)")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev)
    g.manual_seed(7)
    c = torch.randn((a.n, a.d), device=dev, generator=g)
    q = torch.randn((a.nq, a.d), device=dev, generator=g)

    out = {"n": a.n, "d": a.d, "nq": a.nq, "iters": a.iters}
    for k in (10, 100):
        leg = {}
        for scan in ("f16", "split", "f32"):
            res = {}
            for metric in ("l2", "ip"):
                idx = FlatIndex(a.d, metric, dev, scan=scan).adopt(c)
                if (idx.l2_scan_for(k) if metric == "l2" else idx.scan_for(k)) != scan:
                    continue
                ms = _median_ms(lambda: idx.search_device(q, k), a.warmup, a.iters)
                res[metric] = {"ms": round(ms, 4), "rescan_queries": idx.last_rescan_queries,
                               "fallback_queries": idx.last_fallback_queries}
            if "l2" in res and "ip" in res:
                res["l2_over_ip"] = round(res["l2"]["ms"] / res["ip"]["ms"], 3)
            leg[scan] = res
        # the route every L2 search took before: the float64 chain over every (query, row) pair + radix select
        idx = FlatIndex(a.d, "l2", dev).adopt(c)
        D = torch.empty((a.nq, k), dtype=torch.float32, device=dev)
        I = torch.empty((a.nq, k), dtype=torch.int64, device=dev)
        ms = _median_ms(lambda: idx.search_exhaustive(q, k, D, I), 1, a.exhaustive_iters)
        leg["exhaustive"] = {"ms": round(ms, 3)}
        for scan in ("f16", "split", "f32"):
            if "l2" in leg[scan]:
                leg[scan]["speedup_over_exhaustive"] = round(ms / leg[scan]["l2"]["ms"], 1)
        out[f"k{k}"] = leg
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
