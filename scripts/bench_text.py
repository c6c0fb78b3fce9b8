"""Dev helper: the query text encoder's forward (text.NodeTextTransformer) at the reference's shape -- ninp 200, 4 heads,
nhid 800, 4 layers, T = 20 (CFG; train_session_subsession_embedding.py:127-133) -- on B = 3072 query nodes (a 1024-session
query batch) and B = 300 000 (a corpus slice), token counts drawn clip(2 + Poisson(3), 2, 20), under both padding rules.
Prints one JSON line; per size and rule:
  forward_ms        the whole forward(src, mask) from host token arrays -- packing, the uploads, 7 * nlayers + 2 launches per
                    chunk, the one read of err: hipEvent median after warm-up
  pack_ms           the host packing alone (pack_tokens), a host clock median; it is inside forward_ms
  kernels_ms        the same forward's kernels by family, summed per repetition from the profiler's device durations in a
                    run of its own, median over the repetitions
  torch_ms          torch.nn.TransformerEncoder in eval() under no_grad() on the same device with the same weights, inputs
                    already on the device, walked in chunks of 16384 sequences: fast path off for "compute", on (nested
                    tensors) for "zero" -- the setting under which torch itself follows that rule: hipEvent median
  max_abs_diff      between the two results (a sanity check, not a parity test: tests/test_text_transformer_gpu.py is that)
  rows, gemm_flop   packed token rows and what their GEMMs need by arithmetic: 2 (3 e^2 + e^2 + 2 e nhid) per row and layer
  active_lanes      the attention kernel's share of lanes with a query row: rows / (64 * B)"""
import argparse
import json
import math
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bench_sparse import event_median_ms, kernel_medians_ms  # noqa: E402
from sessionsimilaritysearch_amd.text import NodeTextTransformer, pack_tokens  # noqa: E402

FAMILIES = ("k_linear_grouped", "k_seq_attention", "k_add_layernorm", "k_text_embed", "k_segment_reduce")
TORCH_CHUNK = 16384


class TorchText(torch.nn.Module):
    """The module in plain torch under the reference's state_dict() names; seeded, biases and LayerNorms randomised."""

    def __init__(self, ntoken, ninp, nhead, nhid, nlayers, seed):
        super().__init__()
        torch.manual_seed(seed)
        self.ninp = ninp
        self.embedding = torch.nn.Embedding(ntoken, ninp)
        pos = torch.arange(0, 64, dtype=torch.float).unsqueeze(1)
        div = torch.exp(torch.arange(0, ninp, 2).float() * (-math.log(10000.0) / ninp))
        pe = torch.zeros(64, ninp)
        pe[:, 0::2], pe[:, 1::2] = torch.sin(pos * div), torch.cos(pos * div)
        self.pos_encoder = torch.nn.Module()
        self.pos_encoder.register_buffer("pe", pe[None])
        self.transformer_encoder = torch.nn.TransformerEncoder(torch.nn.TransformerEncoderLayer(ninp, nhead, nhid, 0.5, batch_first=True),
                                                               nlayers)
        with torch.no_grad():
            for name, p in self.named_parameters():
                if name.endswith("bias"):
                    p.copy_(torch.randn_like(p) * 0.3)
                elif "norm" in name and name.endswith("weight"):
                    p.copy_(1.0 + torch.randn_like(p) * 0.2)
        self.eval()

    @torch.no_grad()
    def forward(self, src, mask, rule):
        torch.backends.mha.set_fastpath_enabled(rule == "zero")
        try:
            outs = []
            for i in range(0, src.shape[0], TORCH_CHUNK):
                s, m = src[i:i + TORCH_CHUNK], mask[i:i + TORCH_CHUNK]
                x = self.embedding(s) * math.sqrt(self.ninp) + self.pos_encoder.pe[:, :s.shape[1]]
                outs.append(self.transformer_encoder(x, src_key_padding_mask=m).mean(1))
            return torch.cat(outs)
        finally:
            torch.backends.mha.set_fastpath_enabled(True)


def make_batch(B, T, ntoken, seed):
    rng = np.random.default_rng(seed)
    lengths = np.clip(2 + rng.poisson(3, B), 2, T)
    return rng.integers(0, ntoken, (B, T)).astype(np.int64), np.arange(T)[None, :] >= lengths[:, None]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="3072,300000")
    ap.add_argument("--ntoken", type=int, default=30522)
    ap.add_argument("--ninp", type=int, default=200)
    ap.add_argument("--nhead", type=int, default=4)
    ap.add_argument("--nhid", type=int, default=800)
    ap.add_argument("--nlayers", type=int, default=4)
    ap.add_argument("--T", type=int, default=20)
    ap.add_argument("--reps", type=int, default=7)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_text.py needs a HIP device; none is visible")
    dev = torch.device("cuda", 0)
    module = TorchText(a.ntoken, a.ninp, a.nhead, a.nhid, a.nlayers, seed=1)
    on_dev = TorchText(a.ntoken, a.ninp, a.nhead, a.nhid, a.nlayers, seed=1).to(dev)
    e, per_row = a.ninp, a.nlayers * 2 * (4 * a.ninp * a.ninp + 2 * a.ninp * a.nhid)
    out = {"ntoken": a.ntoken, "ninp": e, "nhead": a.nhead, "nhid": a.nhid, "nlayers": a.nlayers, "T": a.T, "reps": a.reps,
           "launches_per_chunk": 7 * a.nlayers + 2, "results": []}
    for B in (int(s) for s in a.sizes.split(",")):
        src, mask = make_batch(B, a.T, a.ntoken, B)
        d_src, d_mask = torch.from_numpy(src).to(dev), torch.from_numpy(mask).to(dev)
        for rule in ("compute", "zero"):
            enc = NodeTextTransformer.from_torch(module, pad_rule=rule, device=dev)
            ours = lambda: enc.forward(src, mask)
            base = lambda: on_dev(d_src, d_mask, rule)
            rows = len(pack_tokens(src, mask, rule).tok)
            r = {"B": B, "pad_rule": rule, "rows": rows, "gemm_flop": rows * per_row, "active_lanes": round(rows / (64.0 * B), 4),
                 "max_abs_diff": float((ours() - base()).abs().max())}
            ts = []
            for _ in range(a.reps):
                t0 = time.perf_counter()
                pack_tokens(src, mask, rule, a.ntoken)
                ts.append((time.perf_counter() - t0) * 1e3)
            r["pack_ms"] = round(float(np.median(ts)), 3)
            r["forward_ms"] = round(event_median_ms(ours, 2, a.reps), 3)      # the two alternate: other work shares the host
            r["torch_ms"] = round(event_median_ms(base, 2, a.reps), 3)
            r["forward_ms_again"] = round(event_median_ms(ours, 1, a.reps), 3)
            r["speedup_over_torch"] = round(r["torch_ms"] / r["forward_ms"], 3)
            kern = kernel_medians_ms(ours, 1, min(a.reps, 3))
            if not all(kern.get(f) for f in FAMILIES):
                raise RuntimeError(f"text encoder kernels not found in the profile: {sorted(kern)}")
            r["kernels_ms"] = {f: round(kern[f], 4) for f in FAMILIES}
            r["other_kernels_ms"] = round(sum(v for k, v in kern.items() if k not in FAMILIES), 4)
            r["gemm_tflops"] = round(r["gemm_flop"] / (kern["k_linear_grouped"] * 1e-3) / 1e12, 2)
            out["results"].append(r)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
