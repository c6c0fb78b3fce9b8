"""Dev helper (not the official bench): time the fused search of a 16-bit or int8 index -- ``--dtype bf16``, ``f16`` or
``i8``, or several separated by commas, which are then timed ALTERNATING in one process (one window of each in turn),
so that one dtype can be the yardstick of another in the same run -- on random unit rows (int8: quantised with
``quantize_i8``, scale 127 / max|x|).  Per shape: ``--warmup`` untimed searches, then ``--repeats`` timed windows of ``--steps`` searches
each (device events around the window); prints one JSON line per shape with the median window, the fastest and the
slowest, so that two dtypes (or two builds: ``--lib`` loads another libsss.so) can be compared against the spread of
one of them.

    python scripts/bench_index_dtype.py --dtype f16 1024,1000000,128,10 4096,10000000,256,10
    python scripts/bench_index_dtype.py --dtype f16,i8 --repeats 10 1024,1000000,256,10
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def build(nq, n, d, dtype):
    """(index, queries) of one dtype on the same random unit rows (seed 1)."""
    import torch
    from sessionsimilaritysearch_amd.index import FlatIndex, normalize_, quantize_i8
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev)
    g.manual_seed(1)
    tdtype = {"bf16": torch.bfloat16, "f16": torch.float16, "i8": torch.int8}[dtype]
    # int8: one scale for the whole corpus, from the largest |element| a unit row of this d can be expected to hold
    # (6 / sqrt(d): elements are ~N(0, 1/d)); what exceeds it is clipped at +-127
    scale = 127.0 / (6.0 / d ** 0.5)
    conv = (lambda x: quantize_i8(x, scale)[0]) if dtype == "i8" else (lambda x: x.to(tdtype))
    c = torch.empty((n, d), dtype=tdtype, device=dev)
    for lo in range(0, n, 1 << 20):                 # (float32 staging a million rows at a time: 10M x 256 stays in memory)
        part = torch.randn((min(n, lo + (1 << 20)) - lo, d), device=dev, generator=g)
        c[lo:lo + part.shape[0]] = conv(normalize_(part))
    q = conv(normalize_(torch.randn((nq, d), device=dev, generator=g)))
    idx = FlatIndex(d, "ip", dev, dtype=dtype).adopt(c)
    idx.corpus_max_norm()
    return idx, q


def run(nq, n, d, k, dtypes, steps, warmup, repeats):
    import torch
    legs = []
    for dtype in dtypes:
        idx, q = build(nq, n, d, dtype)
        out = idx.search_fused(q, k)
        for _ in range(warmup):
            idx.search_fused(q, k, out)
        legs.append((dtype, idx, q, out, []))
    torch.cuda.synchronize()
    for _ in range(repeats):                        # one window of each dtype in turn
        for dtype, idx, q, out, windows in legs:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(steps):
                idx.search_fused(q, k, out)
            e1.record()
            torch.cuda.synchronize()
            windows.append(e0.elapsed_time(e1) / steps)
    for dtype, idx, q, out, windows in legs:
        ms = statistics.median(windows)
        print(json.dumps(dict(dtype=dtype, nq=nq, n=n, d=d, k=k, scan=idx.last_scan, ms_median=round(ms, 4), ms_min=round(min(windows), 4),
                              ms_max=round(max(windows), 4), steps=steps, repeats=repeats, qps=round(nq / (ms * 1e-3)),
                              tflops=round(2.0 * nq * n * d / (ms * 1e-3) / 1e12, 1), unproven=int((out[2] != 0).sum().item()))), flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--dtype", default="f16", help="bf16, f16 or i8; several separated by commas are timed alternating")
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
    dtypes = a.dtype.split(",")
    if not dtypes or any(t not in ("bf16", "f16", "i8") for t in dtypes):
        ap.error("--dtype takes bf16, f16, i8 or a comma-separated list of them")
    for s in a.shapes:
        run(*(int(v) for v in s.split(",")), dtypes, a.steps, a.warmup, a.repeats)
