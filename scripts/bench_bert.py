"""Dev helper: the node text encoder's forward (text.BertNodeEncoder) at bert-base's geometry -- hidden 768, 12 heads,
intermediate 3072, 12 layers, T = 20 -- on B = 3072 nodes (a 1024-session query batch) and a larger batch, token counts drawn
clip(2 + Poisson(3), 2, 20) as in bench_text.py, weights from a seed.  A share --dup of the rows (default 0.5) are copies of
other rows of the batch (every session's root query is the same tokens, an item's title repeats across sessions).
Prints one JSON line; per size, pool and dedup setting:
  forward_ms        the whole enc(input_ids, token_type_ids, attention_mask) from host token arrays -- np.unique, packing,
                    the uploads, 7 * nlayers + 2 launches per chunk, the scatter, the one read of err: hipEvent median after
                    warm-ups
  host_ms           the host side alone (unique_rows + bert_pack_rows), a host clock median; it is inside forward_ms
  kernels_ms        the same forward's kernels by family, summed per repetition from the profiler's device durations in a
                    pass of its own, median over the repetitions
  torch_ms          a plain torch restatement on the same device with the same float32 weights (F.scaled_dot_product_attention
                    under a boolean key mask, F.gelu, F.layer_norm), inputs already on the device, all T positions of all B
                    rows, walked in chunks of 8192 sequences: hipEvent median
  max_abs_diff      between the two results (a sanity check, not a parity test: tests/test_bert_encoder_gpu.py is that)
  rows, unique      packed token rows that reach the kernels, distinct sequences; gemm_flop what the rows' GEMMs need by
                    arithmetic: 2 (4 e^2 + 2 e inter) per row and layer
--gemm f32,bf16 builds one encoder per GEMM path (text.BertNodeEncoder(gemm=...)) and times them ALTERNATING in one process,
one forward of each in turn per repetition, after the same warm-ups (the style of bench_index_dtype.py); each gets a
result record of its own ("gemm"), a profiler pass of its own, and max_abs_diff_to_f32, the largest difference between its
output and the f32 encoder's."""
import argparse
import json
import math
import os
import sys
import time

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bench_sparse import event_median_ms, kernel_medians_ms  # noqa: E402
from sessionsimilaritysearch_amd.text import BertNodeEncoder, bert_pack_rows, unique_rows  # noqa: E402

GEMM_FAMILY = {"f32": "k_linear_grouped", "bf16": "k_linear_grouped_bf16"}
OTHER_FAMILIES = ("k_seq_attention", "k_add_layernorm", "k_bert_embed", "k_segment_reduce")
TORCH_CHUNK = 8192
LAYER = "encoder.layer.{}."


def seeded_weights(seed, vocab, e, inter, nlayers, n_pos, dev):
    """float32 weights under HF's state_dict() names, on the device: N(0, 1 / sqrt(fan_in)) matrices, small random biases."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=g).to(dev)
    w = {"embeddings.word_embeddings.weight": rn(vocab, e), "embeddings.position_embeddings.weight": rn(n_pos, e) * 0.5,
         "embeddings.token_type_embeddings.weight": rn(2, e) * 0.5, "embeddings.LayerNorm.weight": 1 + 0.2 * rn(e),
         "embeddings.LayerNorm.bias": 0.3 * rn(e)}
    for l in range(nlayers):
        p = LAYER.format(l)
        for name, m, k in (("attention.self.query", e, e), ("attention.self.key", e, e), ("attention.self.value", e, e),
                           ("attention.output.dense", e, e), ("intermediate.dense", inter, e), ("output.dense", e, inter)):
            w[p + name + ".weight"], w[p + name + ".bias"] = rn(m, k) / math.sqrt(k), 0.3 * rn(m)
        for name in ("attention.output.LayerNorm", "output.LayerNorm"):
            w[p + name + ".weight"], w[p + name + ".bias"] = 1 + 0.2 * rn(e), 0.3 * rn(e)
    return w


@torch.no_grad()
def torch_forward(w, heads, nlayers, ids, tt, am, pool, eps=1e-12):
    outs = []
    for i in range(0, ids.shape[0], TORCH_CHUNK):
        s, t, m = ids[i:i + TORCH_CHUNK], tt[i:i + TORCH_CHUNK], am[i:i + TORCH_CHUNK]
        B, T = s.shape
        e = w["embeddings.word_embeddings.weight"].shape[1]
        x = (w["embeddings.word_embeddings.weight"][s] + w["embeddings.token_type_embeddings.weight"][t]) + w["embeddings.position_embeddings.weight"][:T][None]
        x = F.layer_norm(x, (e,), w["embeddings.LayerNorm.weight"], w["embeddings.LayerNorm.bias"], eps)
        key = (m != 0)[:, None, None, :]
        for l in range(nlayers):
            g = lambda n: w[LAYER.format(l) + n]
            split = lambda y: y.view(B, T, heads, e // heads).transpose(1, 2)
            q, k, v = (split(F.linear(x, g(f"attention.self.{n}.weight"), g(f"attention.self.{n}.bias"))) for n in ("query", "key", "value"))
            a = F.scaled_dot_product_attention(q, k, v, attn_mask=key).transpose(1, 2).reshape(B, T, e)
            a = F.linear(a, g("attention.output.dense.weight"), g("attention.output.dense.bias"))
            x = F.layer_norm(x + a, (e,), g("attention.output.LayerNorm.weight"), g("attention.output.LayerNorm.bias"), eps)
            h = F.gelu(F.linear(x, g("intermediate.dense.weight"), g("intermediate.dense.bias")))
            h = F.linear(h, g("output.dense.weight"), g("output.dense.bias"))
            x = F.layer_norm(x + h, (e,), g("output.LayerNorm.weight"), g("output.LayerNorm.bias"), eps)
        if pool == "mean":
            outs.append(x.mean(1))
        else:
            mf = (m != 0).to(x.dtype)
            outs.append((x * mf[:, :, None]).sum(1) / mf.sum(1)[:, None])
    return torch.cat(outs)


def make_batch(B, T, vocab, dup, seed):
    """(ids, types, mask, distinct): the last round(dup * B) rows are copies of rows drawn from the first B - that many."""
    rng = np.random.default_rng(seed)
    lengths = np.clip(2 + rng.poisson(3, B), 2, T)
    ids, tt = rng.integers(0, vocab, (B, T)).astype(np.int64), rng.integers(0, 2, (B, T)).astype(np.int64)
    am = (np.arange(T)[None, :] < lengths[:, None]).astype(np.int64)
    n_dup = int(round(dup * B))
    if n_dup:
        src = rng.integers(0, B - n_dup, n_dup)
        ids[B - n_dup:], tt[B - n_dup:], am[B - n_dup:] = ids[src], tt[src], am[src]
    perm = rng.permutation(B)
    return ids[perm], tt[perm], am[perm], B - n_dup


def alternating_event_medians_ms(fns, warmup, reps):
    """{name: hipEvent median of fn()} with the functions run in turn: warm-ups of each, then one timed call of each per
    repetition.  With one function this is bench_sparse.event_median_ms."""
    for fn in fns.values():
        for _ in range(warmup):
            fn()
    ts = {name: [] for name in fns}
    for _ in range(reps):
        for name, fn in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(); fn(); b.record(); b.synchronize()
            ts[name].append(a.elapsed_time(b))
    return {name: float(np.median(t)) for name, t in ts.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="3072,32768")
    ap.add_argument("--vocab", type=int, default=30522)
    ap.add_argument("--hidden", type=int, default=768)
    ap.add_argument("--heads", type=int, default=12)
    ap.add_argument("--inter", type=int, default=3072)
    ap.add_argument("--nlayers", type=int, default=12)
    ap.add_argument("--T", type=int, default=20)
    ap.add_argument("--dup", type=float, default=0.5)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--gemm", default="f32", help="f32, bf16 or both separated by a comma: timed alternating in one process")
    a = ap.parse_args()
    gemms = a.gemm.split(",")
    if not gemms or any(g not in GEMM_FAMILY for g in gemms) or len(set(gemms)) != len(gemms):
        raise SystemExit(f"--gemm takes f32, bf16 or f32,bf16; got {a.gemm!r}")
    if not torch.cuda.is_available():
        raise SystemExit("bench_bert.py needs a HIP device; none is visible")
    dev = torch.device("cuda", 0)
    w = seeded_weights(1, a.vocab, a.hidden, a.inter, a.nlayers, 512, dev)
    per_row = a.nlayers * 2 * (4 * a.hidden * a.hidden + 2 * a.hidden * a.inter)
    out = {"vocab": a.vocab, "hidden": a.hidden, "heads": a.heads, "inter": a.inter, "nlayers": a.nlayers, "T": a.T, "dup": a.dup,
           "reps": a.reps, "gemm": gemms, "launches_per_chunk": 7 * a.nlayers + 2, "results": []}
    for B in (int(s) for s in a.sizes.split(",")):
        ids, tt, am, distinct = make_batch(B, a.T, a.vocab, a.dup, B)
        d_ids, d_tt, d_am = (torch.from_numpy(x).to(dev) for x in (ids, tt, am))
        for pool in ("masked", "mean"):
            base = lambda: torch_forward(w, a.heads, a.nlayers, d_ids, d_tt, d_am, pool)
            torch_ms = None
            for dedup in (True, False):
                encs = {g: BertNodeEncoder(w, a.heads, pool=pool, device=dev, dedup=dedup, gemm=g) for g in gemms}
                ours = {g: (lambda enc=enc: enc(ids, tt, am)) for g, enc in encs.items()}

                def host():
                    u = unique_rows(ids, tt, am)[0] if dedup else slice(None)
                    return bert_pack_rows(ids[u], tt[u], am[u], pool)
                rows = len(host().rows.tok)
                ts = []
                for _ in range(a.reps):
                    t0 = time.perf_counter()
                    host()
                    ts.append((time.perf_counter() - t0) * 1e3)
                host_ms = round(float(np.median(ts)), 3)
                ref, exact = base(), (ours["f32"]() if "f32" in ours else None)
                forward_ms = alternating_event_medians_ms(ours, 2, a.reps)
                if torch_ms is None:                                    # the restatement does not de-duplicate: once per pool
                    torch_ms = round(event_median_ms(base, 2, a.reps), 3)
                for g in gemms:
                    got = ours[g]()
                    r = {"B": B, "pool": pool, "dedup": dedup, "gemm": g, "unique": distinct if dedup else B, "rows": rows,
                         "gemm_flop": rows * per_row, "max_abs_diff": float((got - ref).abs().max())}
                    if exact is not None and g != "f32":
                        r["max_abs_diff_to_f32"] = float((got - exact).abs().max())
                    r["host_ms"], r["forward_ms"], r["torch_ms"] = host_ms, round(forward_ms[g], 3), torch_ms
                    r["speedup_over_torch"] = round(torch_ms / r["forward_ms"], 3)
                    kern = kernel_medians_ms(ours[g], 1, min(a.reps, 3))
                    families = (GEMM_FAMILY[g],) + OTHER_FAMILIES
                    if not all(kern.get(f) for f in families):
                        raise RuntimeError(f"encoder kernels not found in the profile: {sorted(kern)}")
                    r["kernels_ms"] = {f: round(kern[f], 4) for f in families}
                    r["other_kernels_ms"] = round(sum(v for k, v in kern.items() if k not in families), 4)
                    r["gemm_tflops"] = round(r["gemm_flop"] / (kern[GEMM_FAMILY[g]] * 1e-3) / 1e12, 2)
                    out["results"].append(r)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
