"""Generates tests/golden/text_transformer.npz from the reference's own NodeTextTransformer.

Run in the build container only (needs /root/reference):  python tests/golden/make_golden_text.py
model/NodeEmbedding.py is loaded by FILE PATH, as make_golden.py does; nothing from the reference is copied -- the .npz
holds seeded weights, inputs and the module's outputs.  Per record R (keys "R:..."):
  w:<state_dict name>   the weights, nhead.  Biases and LayerNorm parameters are randomised and in_proj is scaled by 2 so
                        that every term matters; every parameter is rounded to a float16-representable value BEFORE the
                        reference runs and is stored as float16 (exact; it halves the file); pos_encoder.pe is the
                        module's float32 buffer cut to its first T rows.  Record "t1" runs the module of "t64" and
                        stores no weights of its own
  src, lengths          token ids [B, T] and the prefix lengths; padded ids are random
  out_fast, rule_fast   eval() under no_grad() with torch's fast path ON and the prefix mask; per row the rule it took:
                        0 "compute", 1 "zero" (changing the padded token ids changed nothing), 2 no padding in the row
  out_slow              the same with the fast path OFF (rule "compute")
  mask_np, out_np       a NON-prefix mask (row 0: first token masked, row 1: a hole) and the fast-path-off output under it
  err_fast, err_slow, err_np   max |reference float32 - float64 helper| of each (tests/helpers/text_ref.py)
"""
import importlib.util
import os
import sys

import numpy as np
import torch

REF = "/root/reference/model/NodeEmbedding.py"
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "helpers"))
import text_ref as tr  # noqa: E402

spec = importlib.util.spec_from_file_location("ref_node_embedding", REF)
mod = importlib.util.module_from_spec(spec)
spec.loader.exec_module(mod)

RECORDS = {  # name: (ntoken, ninp, nhead, nhid, nlayers, T, lengths)
    "cfg_like": (50, 100, 2, 48, 2, 20, [20, 1, 2, 5, 12, 3, 19, 20, 7]),
    "t64": (30, 20, 4, 8, 1, 64, [64, 1, 63, 33, 2]),
    "t1": (30, 20, 4, 8, 1, 1, [1, 1, 1]),
    "full": (40, 24, 8, 16, 3, 7, [7, 7, 7, 7]),
}


def build(ntoken, ninp, nhead, nhid, nlayers, seed):
    torch.manual_seed(seed)
    m = mod.NodeTextTransformer(ntoken, ninp, nhead, nhid, nlayers).eval()
    with torch.no_grad():
        for name, p in m.named_parameters():
            if name.endswith("in_proj_weight"):
                p.mul_(2.0)
            elif name.endswith("bias"):
                p.copy_(torch.randn_like(p) * 0.3)
            elif "norm" in name and name.endswith("weight"):
                p.copy_(1.0 + torch.randn_like(p) * 0.2)
        for p in m.parameters():
            p.copy_(p.half().float())
    return m


def run(m, src, mask, fast):
    torch.backends.mha.set_fastpath_enabled(fast)
    try:
        with torch.no_grad():
            return m(torch.from_numpy(src), torch.from_numpy(mask)).numpy()
    finally:
        torch.backends.mha.set_fastpath_enabled(True)


out = {}
for i, (name, (ntoken, ninp, nhead, nhid, nlayers, T, lengths)) in enumerate(RECORDS.items()):
    m = build(ntoken, ninp, nhead, nhid, nlayers, 20260100 + (1 if name == "t1" else i))   # t1 shares t64's weights
    rng = np.random.default_rng(77 + i)
    B = len(lengths)
    src = rng.integers(0, ntoken, (B, T)).astype(np.int64)
    mask = tr.prefix_mask(lengths, T)
    w = {k: v.numpy() for k, v in m.state_dict().items()}
    w["pos_encoder.pe"] = w["pos_encoder.pe"][0, :T].copy()
    for k, v in w.items():
        if name != "t1":
            out[f"{name}:w:{k}"] = v if k == "pos_encoder.pe" else v.astype(np.float16)
            assert (out[f"{name}:w:{k}"].astype(np.float32) == v).all(), k
    out[f"{name}:nhead"] = np.int64(nhead)
    out[f"{name}:src"], out[f"{name}:lengths"] = src, np.asarray(lengths, dtype=np.int64)
    ref = {r: tr.forward(w, nhead, src, mask, r) for r in ("compute", "zero")}
    fast = run(m, src, mask, True)
    other = np.where(mask, (src + 1 + rng.integers(0, ntoken - 1, src.shape)) % ntoken, src)   # every padded id changed
    same = (run(m, other, mask, True) == fast).all(axis=1)
    rule = np.where(~mask.any(axis=1), 2, np.where(same, 1, 0)).astype(np.int8)
    want = np.stack([ref["zero"][b] if rule[b] == 1 else ref["compute"][b] for b in range(B)])
    out[f"{name}:out_fast"], out[f"{name}:rule_fast"] = fast, rule
    out[f"{name}:err_fast"] = np.abs(fast - want).max()
    slow = run(m, src, mask, False)
    out[f"{name}:out_slow"], out[f"{name}:err_slow"] = slow, np.abs(slow - ref["compute"]).max()
    msg = f"{name}: rule_fast {rule.tolist()} err_fast {out[f'{name}:err_fast']:.2e} err_slow {out[f'{name}:err_slow']:.2e}"
    msg += f" scale {np.abs(slow).max():.2f} rule gap {np.abs(ref['compute'] - ref['zero']).max():.2f}"
    if T > 2:
        mask_np = mask.copy()
        mask_np[0, 0] = True
        mask_np[1] = False
        mask_np[1, T // 2] = True
        out_np = run(m, src, mask_np, False)
        out[f"{name}:mask_np"], out[f"{name}:out_np"] = mask_np, out_np
        out[f"{name}:err_np"] = np.abs(out_np - tr.forward(w, nhead, src, mask_np, "compute")).max()
        msg += f" err_np {out[f'{name}:err_np']:.2e}"
    print(msg)

path = os.path.join(HERE, "text_transformer.npz")
np.savez(path, **out)
print("wrote text_transformer.npz", os.path.getsize(path), "bytes")
