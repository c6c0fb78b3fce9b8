"""Dev helper: the catalogue heads (sessionsimilaritysearch_amd/catalogue.py) at the reference's shape -- V = 391 572 items,
d = 200, B = 200 sessions -- against a plain-torch restatement of the reference's functions on the same device, which
materialises its [B, V] matrices and draws its random numbers on the device (the reference draws them on the host).  The two
alternate in one process, ``--rounds`` times; every figure is a wall clock around work that ends in a device synchronise
(both sides end in a host read-back of the result), the median of ``--reps`` calls after ``--warmup``.  Prints one JSON line:
  rounds[i].fused_bce_1000_ms / torch_bce_1000_ms      n_neg = 1000 (the reference's rate 1000 / V)
  rounds[i].fused_bce_all_ms / torch_bce_all_ms        every negative kept
  rounds[i].fused_bce_1000_device_ms                   sss_catalogue_bce + finish alone (device events, no read-back)
  rounds[i].fused_predict_ms / torch_predict_ms        top-20
  speedup_*                                            per pair: (min, max) over the rounds of torch / fused
  spread_*                                             per figure: (max - min) / median over the rounds
  table_bytes, restatement_bytes                       the padded table's single pass, and what the restatement writes: its
                                                       float32 [B, V] matrices (y, the logits, sigmoid, clip, log(val),
                                                       log(1 - val), 1 - y, 1 - val, two products, their sum, the negation,
                                                       rand, |val - y|) and its bool ones (neg_mask, loss_mask, diff_mask)
  loss_fused_all / loss_torch_all                      the two losses where no mask differs (same inputs)"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from sessionsimilaritysearch_amd import catalogue  # noqa: E402
from sessionsimilaritysearch_amd.sparse import _device_triple  # noqa: E402

F32_MATRICES, BOOL_MATRICES = 14, 3


def torch_bce(rep, weight, rows, cols, rate):
    """The reference's loss in plain torch: every [B, V] matrix it makes is made."""
    y = torch.zeros(rep.shape[0], weight.shape[0], device=rep.device)
    y[rows, cols] = 1.
    val = torch.clip(torch.sigmoid(rep @ weight.T), min=1e-4, max=0.9999)
    loss_mat = -(y * torch.log(val) + (1 - y) * torch.log(1 - val))
    neg_mask = torch.rand(loss_mat.shape, device=rep.device) < rate
    loss_mask = torch.logical_or(neg_mask, y)
    diff_mask = torch.abs(val - y) > 0.5                     # the reference computes it and does not use it
    assert torch.sum(loss_mask) > 0 and diff_mask.shape == y.shape
    return torch.mean(loss_mat[loss_mask]).item()


def torch_predict(rep, weight, K):
    val = torch.clip(torch.sigmoid(rep @ weight.T), min=1e-4, max=0.9999)
    return torch.topk(val, K, dim=1)[1].cpu()


def wall_median_ms(fn, warmup, reps):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts))


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
    ap.add_argument("--v", type=int, default=391572)
    ap.add_argument("--d", type=int, default=200)
    ap.add_argument("--b", type=int, default=200)
    ap.add_argument("--k", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_catalogue needs a HIP device: there is no CPU fallback and no CPU timing")
    dev = torch.device("cuda", 0)
    r = np.random.default_rng(0)
    V, d, B = a.v, a.d, a.b
    table = (r.standard_normal((V, d)) / np.sqrt(d)).astype(np.float32)
    rep = (2.0 * r.standard_normal((B, d))).astype(np.float32)
    sets = [np.sort(r.choice(V, size=int(r.integers(1, 9)), replace=False)) for _ in range(B)]
    ptr = np.zeros(B + 1, np.int64)
    np.cumsum([len(s) for s in sets], out=ptr[1:])
    items = np.concatenate(sets).astype(np.int32)
    targets = _device_triple(ptr, items, np.zeros(len(items), np.float32), dev)
    head = catalogue.CatalogueHead(table, device=dev)
    weight, rep_t = head._rows, torch.from_numpy(rep).to(dev)
    rows = torch.from_numpy(np.repeat(np.arange(B), np.diff(ptr))).to(dev)
    cols = torch.from_numpy(items.astype(np.int64)).to(dev)
    head.predict(rep_t, a.k)                                  # builds the index and its scan image

    figures = {
        "fused_bce_1000_ms": lambda: wall_median_ms(lambda: head.bce(rep_t, targets, 1000, 1), a.warmup, a.reps),
        "torch_bce_1000_ms": lambda: wall_median_ms(lambda: torch_bce(rep_t, weight, rows, cols, 1000 / V), a.warmup, a.reps),
        "fused_bce_all_ms": lambda: wall_median_ms(lambda: head.bce(rep_t, targets, "all"), a.warmup, a.reps),
        "torch_bce_all_ms": lambda: wall_median_ms(lambda: torch_bce(rep_t, weight, rows, cols, 2.0), a.warmup, a.reps),
        "fused_bce_1000_device_ms": lambda: event_median_ms(lambda: head.bce_device(rep_t, targets, 1000, 1), a.warmup, a.reps),
        "fused_bce_all_device_ms": lambda: event_median_ms(lambda: head.bce_device(rep_t, targets, "all"), a.warmup, a.reps),
        "fused_predict_ms": lambda: wall_median_ms(lambda: head.predict(rep_t, a.k)[1].cpu(), a.warmup, a.reps),
        "torch_predict_ms": lambda: wall_median_ms(lambda: torch_predict(rep_t, weight, a.k), a.warmup, a.reps),
    }
    rounds = [{name: fn() for name, fn in figures.items()} for _ in range(a.rounds)]
    out = {"V": V, "d": d, "B": B, "K": a.k, "reps": a.reps, "rounds": rounds,
           "table_bytes": V * head.kp * 4, "restatement_bytes": B * V * (4 * F32_MATRICES + BOOL_MATRICES),
           "gemm_flop": 2 * B * V * d, "loss_fused_all": head.bce(rep_t, targets, "all").loss,
           "loss_torch_all": torch_bce(rep_t, weight, rows, cols, 2.0)}
    for name in figures:
        vals = [x[name] for x in rounds]
        out["spread_" + name[:-3]] = (max(vals) - min(vals)) / float(np.median(vals))
    for what in ("bce_1000", "bce_all", "predict"):
        ratios = [x[f"torch_{what}_ms"] / x[f"fused_{what}_ms"] for x in rounds]
        out["speedup_" + what] = (min(ratios), max(ratios))
    _, I = head.predict(rep_t, a.k)
    Ir = torch_predict(rep_t, weight, a.k)
    out["predict_sets_equal_rows"] = int(sum(set(x.tolist()) == set(y.tolist()) for x, y in zip(I.cpu(), Ir)))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
