"""Time BinaryFlatIndex.search(x, 100) on 1M random codes, 1024 random queries, one code length after another.

Random codes have no ties to speak of, so the fused scan proves every query (last_fallback_queries is reported: it
should be 0).  Device events around each call (warmed up), median of --iters calls, the whole measurement --repeats
times over so that the run-to-run spread is visible.  Prints one JSON line per --nbits value: the median ms of every
repeat, their median and spread ((max - min) / median), the stored row bytes, and corpus bytes read per second --
every group of 256 queries streams the whole stored corpus once, so bytes = ceil(nq / 256) * n * row bytes.  A last
line gives each width's time relative to 512 bits when 512 is among the widths.
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from sessionsimilaritysearch_amd.index import BinaryFlatIndex  # noqa: E402


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
    ap.add_argument("--nq", type=int, default=1024)
    ap.add_argument("--k", type=int, default=100)
    ap.add_argument("--nbits", type=int, nargs="+", default=[256, 512, 1024, 1600, 2048])
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=5)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev)
    g.manual_seed(7)
    med = {}
    for nbits in a.nbits:
        idx = BinaryFlatIndex(nbits, dev)
        idx.add(torch.randint(0, 256, (a.n, nbits // 8), dtype=torch.uint8, device=dev, generator=g))
        q = torch.randint(0, 256, (a.nq, nbits // 8), dtype=torch.uint8, device=dev, generator=g)
        ms = [_median_ms(lambda: idx.search(q, a.k), a.warmup, a.iters) for _ in range(a.repeats)]
        med[nbits] = float(np.median(ms))
        scanned = ((a.nq + 255) // 256) * a.n * idx._w
        print(json.dumps({"nbits": nbits, "row_bytes": idx._w, "n": a.n, "nq": a.nq, "k": a.k, "iters": a.iters,
                          "ms": round(med[nbits], 4), "ms_repeats": [round(m, 4) for m in ms],
                          "spread": round((max(ms) - min(ms)) / med[nbits], 4),
                          "last_fallback_queries": idx.last_fallback_queries,
                          "corpus_bytes_per_s": round(scanned / (med[nbits] * 1e-3), 1)}), flush=True)
        del idx
    if 512 in med:
        print(json.dumps({"ms_over_ms_512_bits": {str(b): round(m / med[512], 3) for b, m in med.items()}}), flush=True)


if __name__ == "__main__":
    main()
