"""Dev helper: the HGT encoder's forward (variants.HGT) at the reference's shape -- 768 -> 800, 4 heads, 3 layers
(train_session_subsession_embedding.py:139-160) -- on a batch of 1024 synthetic sessions.  Prints one JSON line:
  forward_ms        the whole forward (1 + 6 L launches): hipEvent median after warm-up
  kernels_ms        the same forward's kernels by family (k_linear_grouped, k_hgt_aggregate, k_hgt_skip), summed per
                    repetition from the profiler's device durations, median over the repetitions
  torch_ms          a plain torch-on-device restatement (unfolded; index_select / scatter softmax / index_add) on the same
                    inputs and weights, float32: hipEvent median after warm-up
  max_abs_diff      between the two results (a sanity check, not a parity test: tests/test_hgt_gpu.py is that)
  gemm_flop, gather_bytes   what one forward needs by arithmetic: 2 h (5 h Np + 3 h Nq) + 2 h^2 (Np + Nq) per layer plus the
                    input transform, and 2 h floats gathered per edge and layer."""
import argparse
import json
import math
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bench_sparse import event_median_ms, kernel_medians_ms  # noqa: E402
from sessionsimilaritysearch_amd import sessions as S  # noqa: E402
from sessionsimilaritysearch_amd.sessions import EDGE_PP, EDGE_PQ, EDGE_QP  # noqa: E402
from sessionsimilaritysearch_amd.variants import HGT  # noqa: E402

EDGES = (("qp", "query", "product"), ("pq", "product", "query"), ("pp", "product", "product"))
TYPES = ("query", "product")


def make_weights(g, d, h, heads, n_layers):
    u = lambda *shape, scale=1.0: (torch.rand(shape, generator=g) * 2 - 1) * scale
    D = h // heads
    w = {}
    for t in TYPES:
        w[f"hgt.lin.{t}.w"], w[f"hgt.lin.{t}.b"] = u(h, d, scale=1 / math.sqrt(d)), u(h, scale=0.1)
    for l in range(n_layers):
        for t in TYPES:
            for n in "kqva":
                w[f"hgt.{l}.{t}.{n}.w"], w[f"hgt.{l}.{t}.{n}.b"] = u(h, h, scale=1 / math.sqrt(h)), u(h, scale=0.1)
            w[f"hgt.{l}.{t}.skip"] = u(1, scale=2.0)
        for e, _, _ in EDGES:
            w[f"hgt.{l}.{e}.a_rel"] = u(heads, D, D, scale=1 / math.sqrt(D))
            w[f"hgt.{l}.{e}.m_rel"] = u(heads, D, D, scale=1 / math.sqrt(D))
            w[f"hgt.{l}.{e}.p_rel"] = u(heads) * 0.5 + 1.0
    return w


def csr_by_target(ei, n_dst, dev):
    order = np.argsort(ei[1], kind="stable")
    rowptr = np.concatenate([[0], np.cumsum(np.bincount(ei[1], minlength=n_dst))]).astype(np.int32)
    return torch.from_numpy(rowptr).to(dev), torch.from_numpy(ei[0][order].astype(np.int32)).to(dev)


def torch_forward(x, edges, w, heads, n_layers):
    """HGT in plain torch on the device, unfolded, in HGTConv's operation order."""
    cur = {t: torch.relu(x[t] @ w[f"hgt.lin.{t}.w"].T + w[f"hgt.lin.{t}.b"]) for t in TYPES}
    outs = [cur]
    h = cur["query"].shape[1]
    D = h // heads
    for l in range(n_layers):
        x = outs[-1]
        lin = lambda t, n: (x[t] @ w[f"hgt.{l}.{t}.{n}.w"].T + w[f"hgt.{l}.{t}.{n}.b"]).view(-1, heads, D)
        k, q, v = ({t: lin(t, n) for t in TYPES} for n in "kqv")
        agg = {t: torch.zeros_like(x[t]) for t in TYPES}
        for e, s, t in EDGES:
            src, dst = edges[e]
            ke = (k[s].transpose(0, 1) @ w[f"hgt.{l}.{e}.a_rel"]).transpose(1, 0)
            ve = (v[s].transpose(0, 1) @ w[f"hgt.{l}.{e}.m_rel"]).transpose(1, 0)
            alpha = (q[t].index_select(0, dst) * ke.index_select(0, src)).sum(-1) * w[f"hgt.{l}.{e}.p_rel"] / math.sqrt(D)
            idx = dst[:, None].expand_as(alpha)
            mx = torch.full((x[t].shape[0], heads), float("-inf"), device=alpha.device).scatter_reduce(0, idx, alpha, "amax")
            ex = (alpha - mx.index_select(0, dst)).exp()
            den = torch.zeros((x[t].shape[0], heads), device=alpha.device).index_add_(0, dst, ex)
            sm = ex / (den.index_select(0, dst) + 1e-16)
            agg[t].index_add_(0, dst, (ve.index_select(0, src) * sm[:, :, None]).reshape(-1, h))
        new = {}
        for t in TYPES:
            y = torch.nn.functional.gelu(agg[t]) @ w[f"hgt.{l}.{t}.a.w"].T + w[f"hgt.{l}.{t}.a.b"]
            sig = torch.sigmoid(w[f"hgt.{l}.{t}.skip"].reshape(()))
            new[t] = sig * y + (1 - sig) * x[t]
        outs.append(new)
    return {t: torch.cat([o[t] for o in outs], 1) for t in TYPES}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sessions", type=int, default=1024)
    ap.add_argument("--d", type=int, default=768)
    ap.add_argument("--h", type=int, default=800)
    ap.add_argument("--heads", type=int, default=4)
    ap.add_argument("--layers", type=int, default=3)
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_hgt.py needs a HIP device; none is visible")
    dev = torch.device("cuda", 0)
    b = S.build_batch(S.synthetic_actions(a.sessions, 1)).to_numpy()
    ei = {"qp": b.edge_index_dict[EDGE_QP], "pq": b.edge_index_dict[EDGE_PQ], "pp": b.edge_index_dict[EDGE_PP]}
    n = {t: len(b[t].x) for t in TYPES}
    g = torch.Generator().manual_seed(1)
    w = make_weights(g, a.d, a.h, a.heads, a.layers)
    x = {t: torch.randn((n[t], a.d), generator=g).to(dev) for t in TYPES}
    csr = {e: csr_by_target(ei[e], n[t], dev) for e, _, t in EDGES}
    enc = HGT(w, a.heads, a.layers, dev)
    ours = lambda: enc.forward(x["query"], x["product"], csr["qp"], csr["pq"], csr["pp"])
    wd = {k: v.to(dev) for k, v in w.items()}
    ed = {e: (torch.from_numpy(ei[e][0]).to(dev), torch.from_numpy(ei[e][1]).to(dev)) for e in ei}
    base = lambda: torch_forward(x, ed, wd, a.heads, a.layers)
    got, ref = ours(), base()
    diff = max(float((got[t] - ref[t]).abs().max()) for t in TYPES)
    h, L = a.h, a.layers
    n_edges = {e: int(ei[e].shape[1]) for e in ei}
    out = {"sessions": a.sessions, "d": a.d, "h": h, "heads": a.heads, "layers": L, "n_query": n["query"], "n_product": n["product"],
           "edges": n_edges, "reps": a.reps, "launches": 1 + 6 * L,
           "gemm_flop": 2 * a.d * h * (n["query"] + n["product"]) + L * (2 * h * (5 * h * n["product"] + 3 * h * n["query"])
                                                                           + 2 * h * h * (n["query"] + n["product"])),
           "gather_bytes": L * sum(n_edges.values()) * 2 * h * 4}
    out["forward_ms"] = event_median_ms(ours, 3, a.reps)
    out["torch_ms"] = event_median_ms(base, 3, a.reps)
    kern = kernel_medians_ms(ours, 1, min(a.reps, 5))
    fam = {f: sum(v for k, v in kern.items() if k == f) for f in ("k_linear_grouped", "k_hgt_aggregate", "k_hgt_skip")}
    if not all(fam.values()):
        raise RuntimeError(f"HGT kernels not found in the profile: {sorted(kern)}")
    out["kernels_ms"] = {k: round(v, 4) for k, v in fam.items()}
    out["other_kernels_ms"] = round(sum(v for k, v in kern.items() if k not in fam), 4)
    out["max_abs_diff"] = diff
    out["speedup_over_torch"] = out["torch_ms"] / out["forward_ms"]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
