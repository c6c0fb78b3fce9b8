"""Dev helper (not the official bench): time the fused search of a 16-bit index -- ``--dtype bf16`` or ``--dtype f16`` --
on random unit rows.  Per shape: ``--warmup`` untimed searches, then ``--repeats`` timed windows of ``--steps`` searches
each (device events around the window); prints one JSON line per shape with the median window, the fastest and the
slowest, so that two dtypes (or two builds: ``--lib`` loads another libsss.so) can be compared against the spread of
one of them.

    python scripts/bench_index_dtype.py --dtype f16 1024,1000000,128,10 4096,10000000,256,10
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def run(nq, n, d, k, dtype, steps, warmup, repeats):
    import torch
    from sessionsimilaritysearch_amd.index import FlatIndex, normalize_
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev)
    g.manual_seed(1)
    tdtype = torch.bfloat16 if dtype == "bf16" else torch.float16
    c = torch.empty((n, d), dtype=tdtype, device=dev)
    for lo in range(0, n, 1 << 20):                 # (float32 staging a million rows at a time: 10M x 256 stays in memory)
        part = torch.randn((min(n, lo + (1 << 20)) - lo, d), device=dev, generator=g)
        c[lo:lo + part.shape[0]] = normalize_(part).to(tdtype)
    q = normalize_(torch.randn((nq, d), device=dev, generator=g)).to(tdtype)
    idx = FlatIndex(d, "ip", dev, dtype=dtype).adopt(c)
    idx.corpus_max_norm()
    out = idx.search_fused(q, k)
    for _ in range(warmup):
        idx.search_fused(q, k, out)
    torch.cuda.synchronize()
    windows = []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(steps):
            idx.search_fused(q, k, out)
        e1.record()
        torch.cuda.synchronize()
        windows.append(e0.elapsed_time(e1) / steps)
    ms = statistics.median(windows)
    print(json.dumps(dict(dtype=dtype, nq=nq, n=n, d=d, k=k, scan=idx.last_scan, ms_median=round(ms, 4), ms_min=round(min(windows), 4),
                          ms_max=round(max(windows), 4), steps=steps, repeats=repeats, qps=round(nq / (ms * 1e-3)),
                          tflops=round(2.0 * nq * n * d / (ms * 1e-3) / 1e12, 1), unproven=int((out[2] != 0).sum().item()))), flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--dtype", choices=("bf16", "f16"), default="f16")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--lib", default=None, help="another build of libsss.so to load instead of the package's own")
    ap.add_argument("shapes", nargs="*", default=["1024,1000000,128,10", "4096,1000000,128,10", "1024,10000000,256,10", "4096,10000000,256,10"],
                    help="nq,n,d,k")
    a = ap.parse_args()
    if a.lib:
        from sessionsimilaritysearch_amd import _lib
        _lib.LIB_PATH = os.path.abspath(a.lib)
    for s in a.shapes:
        run(*(int(v) for v in s.split(",")), a.dtype, a.steps, a.warmup, a.repeats)
