"""Time the search of a float32 FlatIndex whose width has no scan of its own (d = 200: the reference's emb_len; d = 68),
three legs per shape, in one process, the legs alternating call by call:

  (a) ``pad_scan=True``   the scans at the next width they have, re-scored from the d-wide rows;
  (b) ``pad_scan=False``  the exhaustive kernels: what every search of such an index runs on without the switch;
  (c) a native index at the scan width over the zero-extended rows and queries: the same scan without the padding plumbing.

1M x d standard-normal rows (unit rows for "ip", as ``build_index(emb, "cos")`` makes them), 1024 queries, k = 10 and 100,
both metrics.  Device events around each call (warmed up), median of --iters calls.  Also timed on its own: the launch
that pads the query batch.  Prints one JSON line: ms per call and the unproven counts of every leg, (b) / (a) and (a) / (c).
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from sessionsimilaritysearch_amd.index import FlatIndex, normalize_  # noqa: E402


def _timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def _alternating_median_ms(legs, warmup, iters):
    """{name: median ms}: one call of every leg per round, so drift of the device hits all of them alike.  A leg's own
    ``iters`` (name -> (fn, iters)) caps how many rounds it joins (the exhaustive leg takes seconds a call)."""
    for w in range(warmup):
        for fn, own in legs.values():
            if w == 0 or own >= iters:
                fn()
    torch.cuda.synchronize()
    times = {name: [] for name in legs}
    for r in range(iters):
        for name, (fn, own) in legs.items():
            if r < own:
                times[name].append(_timed(fn))
    return {name: float(np.median(t)) for name, t in times.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--dims", type=int, nargs="+", default=[200, 68])
    ap.add_argument("--nq", type=int, default=1024)
    ap.add_argument("--ks", type=int, nargs="+", default=[10, 100])
    ap.add_argument("--metrics", nargs="+", default=["ip", "l2"])
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--exhaustive-iters", type=int, default=2, help="timed calls of leg (b) (seconds each)")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev)
    g.manual_seed(7)
    out = {"n": a.n, "nq": a.nq, "iters": a.iters, "shapes": []}
    for d in a.dims:
        c0 = torch.randn((a.n, d), device=dev, generator=g)
        q0 = torch.randn((a.nq, d), device=dev, generator=g)
        for metric in a.metrics:
            c, q = (normalize_(c0.clone()), normalize_(q0.clone())) if metric == "ip" else (c0, q0)
            pad = FlatIndex(d, metric, dev, pad_scan=True).adopt(c)
            off = FlatIndex(d, metric, dev).adopt(c)
            for k in a.ks:
                scan = pad.prepare(k)
                ds = pad.scan_width(scan)
                cz = torch.zeros((a.n, ds), device=dev)
                cz[:, :d] = c
                qz = torch.zeros((a.nq, ds), device=dev)
                qz[:, :d] = q
                native = FlatIndex(ds, metric, dev, scan=scan).adopt(cz)
                counts = {}

                def leg(idx, qq, name):
                    def run():
                        idx.search_device(qq, k)
                        counts[name] = {"rescan_queries": idx.last_rescan_queries, "fallback_queries": idx.last_fallback_queries}
                    return run
                ms = _alternating_median_ms({"pad": (leg(pad, q, "pad"), a.iters), "native": (leg(native, qz, "native"), a.iters),
                                             "exhaustive": (leg(off, q, "exhaustive"), a.exhaustive_iters),
                                             "query_pad": (lambda: pad._padded_queries(q, ds), a.iters)}, a.warmup, a.iters)
                assert pad.last_scan == native.last_scan == scan
                out["shapes"].append({
                    "d": d, "metric": metric, "k": k, "scan": scan, "scan_width": ds,
                    "pad_ms": round(ms["pad"], 4), "exhaustive_ms": round(ms["exhaustive"], 3), "native_ms": round(ms["native"], 4),
                    "query_pad_ms": round(ms["query_pad"], 4),
                    "speedup_over_exhaustive": round(ms["exhaustive"] / ms["pad"], 1),
                    "pad_over_native": round(ms["pad"] / ms["native"], 3), **{f"{n}_{key}": v for n, cnt in counts.items() for key, v in cnt.items()}})
                del native, cz, qz
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
