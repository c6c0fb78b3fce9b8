"""Child process of tests/test_distributed_kinds_gpu.py: the exchange route of every sharded index kind on a ONE-rank
RCCL group ("nccl" on ROCm).  Started as a fresh process, so the process group is created before anything else of this
process touches the GPU.  Prints one JSON line; exit code 0 = every check passed.

What runs, each with force_collectives=True and an id_offset, each compared with the unsharded index's own answer and
with the CPU oracle (array_equal): ShardedFlatIndex.search / search_async on an L2 index and on an inner-product index
of d = 200 (local exhaustive route, RCCL all-gather of the pack, k_topk_merge, the negation for L2);
ShardedFlatIndex.range_search in both metrics (RCCL all-gather of the counts, of the payload, device assembly), with a
scalar radius and with a radius nothing passes (no payload); ShardedBinaryIndex.search at 256 and 1600 bits.

With --time as the second argument it also measures the one-rank forced-exchange overhead of range_search (1024
queries, 25 hits each) and of the Hamming search against the unsharded calls (wall clock around a synchronised call,
median of 20: range_search syncs by itself)."""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402

OFF = 1000


def _kept(scores, rad, ascending):
    mask = scores < rad[:, None] if ascending else scores > rad[:, None]
    rows, cols = np.nonzero(mask)
    lims = np.zeros(scores.shape[0] + 1, np.int64)
    np.cumsum(mask.sum(1), out=lims[1:])
    return lims, np.ascontiguousarray(scores[rows, cols], np.float32), cols.astype(np.int64) + OFF


def _same(got, want):
    return bool(all(np.array_equal(g.cpu().numpy() if isinstance(g, torch.Tensor) else g,
                                   w.cpu().numpy() if isinstance(w, torch.Tensor) else w) for g, w in zip(got, want)))


def _median_ms(fn, reps=20):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return round(float(np.median(ts)), 4)


def main():
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ.setdefault("MASTER_PORT", sys.argv[1] if len(sys.argv) > 1 else "29534")
    dev = torch.device("cuda", 0)
    dist.init_process_group("nccl", world_size=1, rank=0, device_id=dev)
    torch.cuda.set_device(dev)
    from oracle import search_ref as sr
    from sessionsimilaritysearch_amd.distributed import HammingEngine, HipEngine, ShardedBinaryIndex, ShardedFlatIndex
    from sessionsimilaritysearch_amd.index import BinaryFlatIndex, FlatIndex

    out = {"backend": dist.get_backend(), "world": dist.get_world_size()}
    checks = {}
    rng = np.random.default_rng(53)
    n, nq, k = 20000, 64, 10

    def flat(metric, d, unit):
        c_h = rng.standard_normal((n, d)).astype(np.float32)
        q_h = rng.standard_normal((nq, d)).astype(np.float32)
        if unit:
            c_h, q_h = sr.normalize(c_h), sr.normalize(q_h)
        c_h[1] = c_h[n - 2]
        q_h[0] = c_h[1]
        c, q = torch.from_numpy(c_h).to(dev), torch.from_numpy(q_h).to(dev)
        index = FlatIndex(d, metric, dev).adopt(c, id_offset=OFF)
        return c_h, q_h, q, index, ShardedFlatIndex(HipEngine(index), dev, force_collectives=True)

    # --- top-k: L2, and an inner-product shape without a fused scan
    c_h, q_h, q, index, sh = flat("l2", 128, False)
    routes = [sh.exchange, sh.ascending]
    Dr, Ir = sr.topk_from_scores(sr.canonical_l2(q_h, c_h), k, id_offset=OFF, largest=False)
    Du, Iu = index.search_device(q, k)
    got = sh.search(q, k)
    checks["l2_vs_unsharded"], checks["l2_vs_oracle"] = _same(got, (Du, Iu)), _same(got, (Dr, Ir))
    Da, Ia, st = sh.search_async(q, k)
    checks["l2_async_vs_unsharded"] = _same((Da, Ia), (Du, Iu)) and int(st.sum()) == 0
    checks["l2_async_vs_oracle"] = _same((Da, Ia), (Dr, Ir))

    c_h, q_h, q, index, sh = flat("ip", 200, True)
    routes += [sh.exchange, not sh.ascending, not index.fused_ok(k)]
    Dr, Ir = sr.search_exact(q_h, c_h, k, id_offset=OFF)
    Du, Iu = index.search_device(q, k)
    got = sh.search(q, k)
    checks["ip_d200_vs_unsharded"], checks["ip_d200_vs_oracle"] = _same(got, (Du, Iu)), _same(got, (Dr, Ir))

    # --- range_search, both metrics
    for metric in ("ip", "l2"):
        asc = metric == "l2"
        c_h, q_h, q, index, sh = flat(metric, 128, True)
        s = sr.canonical_l2(q_h, c_h) if asc else sr.canonical_scores(q_h, c_h)
        part = np.sort(s, axis=1)
        rad = (part[:, 25] if asc else part[:, n - 26]).astype(np.float32).copy()
        rad[2] = s.min() - 1 if asc else s.max() + 1        # no hit
        rad[3] = s.max() + 1 if asc else s.min() - 1        # every row
        trad = torch.from_numpy(rad).to(dev)
        want_u, want_o = index.range_search_device(q, trad), _kept(s, rad, asc)
        got = sh.range_search(q, trad)
        checks[f"range_{metric}_vs_unsharded"], checks[f"range_{metric}_vs_oracle"] = _same(got, want_u), _same(got, want_o)
        if metric == "ip":
            got = sh.range_search(q, float(rad[5]))
            checks["range_scalar_vs_unsharded"] = _same(got, index.range_search_device(q, float(rad[5])))
            checks["range_scalar_vs_oracle"] = _same(got, _kept(s, np.full(nq, rad[5], np.float32), asc))
            got = sh.range_search(q, float(rad[2]))
            checks["range_empty_vs_unsharded"] = _same(got, index.range_search_device(q, float(rad[2])))
            checks["range_empty_vs_oracle"] = _same(got, _kept(s, np.full(nq, rad[2], np.float32), asc)) and got[1].numel() == 0

    # --- Hamming
    for nbits in (256, 1600):
        c_h = rng.integers(0, 256, (n, nbits // 8), dtype=np.uint8)
        c_h[1] = c_h[n - 2]
        q_h = rng.integers(0, 256, (nq, nbits // 8), dtype=np.uint8)
        q_h[0] = c_h[1]
        bindex = BinaryFlatIndex(nbits, dev)
        bindex.add(c_h)
        bindex.id_offset = OFF
        bsh = ShardedBinaryIndex(HammingEngine(bindex), dev, force_collectives=True)
        routes.append(bsh.exchange)
        tq = torch.from_numpy(q_h).to(dev)
        got = bsh.search(tq, k)
        checks[f"hamming{nbits}_vs_unsharded"] = _same(got, bindex.search(tq, k)) and got[0].dtype == torch.int32
        checks[f"hamming{nbits}_vs_oracle"] = _same(got, sr.hamming_search(q_h, c_h, k, id_offset=OFF))
    torch.cuda.synchronize()

    if len(sys.argv) > 2 and sys.argv[2] == "--time":
        g = torch.Generator(device=dev); g.manual_seed(9)
        tn, tnq = 100_000, 1024
        c = torch.nn.functional.normalize(torch.randn((tn, 128), device=dev, generator=g))
        q = torch.nn.functional.normalize(torch.randn((tnq, 128), device=dev, generator=g))
        trad = torch.topk(q @ c.T, 26, dim=1).values[:, 25].contiguous()           # 25 rows score above the 26th best
        index = FlatIndex(128, "ip", dev).adopt(c)
        sh = ShardedFlatIndex(HipEngine(index), dev, force_collectives=True)
        hits = int(sh.range_search(q, trad)[0][-1])
        codes = torch.randint(0, 256, (tn, 32), dtype=torch.uint8, device=dev, generator=g)
        qc = torch.randint(0, 256, (tnq, 32), dtype=torch.uint8, device=dev, generator=g)
        bindex = BinaryFlatIndex(256, dev)
        bindex.add(codes)
        bsh = ShardedBinaryIndex(HammingEngine(bindex), dev, force_collectives=True)
        out["ms"] = {"range_hits_per_query": round(hits / tnq, 2),
                     "range_search_unsharded": _median_ms(lambda: index.range_search_device(q, trad)),
                     "range_search_forced_exchange": _median_ms(lambda: sh.range_search(q, trad)),
                     "hamming_search_unsharded": _median_ms(lambda: bindex.search(qc, 10)),
                     "hamming_search_forced_exchange": _median_ms(lambda: bsh.search(qc, 10))}

    out["checks"] = checks
    out["ok"] = bool(all(checks.values()) and all(routes) and out["backend"] == "nccl")
    print(json.dumps(out), flush=True)
    dist.destroy_process_group()
    return 0 if out["ok"] else 1


if __name__ == "__main__":
    sys.exit(main())
