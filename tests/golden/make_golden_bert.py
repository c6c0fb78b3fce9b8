"""Generates tests/golden/bert_encoder.npz from the `transformers` library's own BertModel.

Run where `transformers` is installed:  python tests/golden/make_golden_bert.py
Nothing is fetched: the model is built from a BertConfig alone (hidden 64, 4 heads, intermediate 128, 2 layers, vocab 97,
32 positions, 2 token types; add_pooling_layer=False) and its weights come from a seed.  The .npz holds:
  w:<state_dict name>   the weights.  HF's initialisation (N(0, 0.02), zero biases, unit LayerNorms) leaves most terms idle, so
                        the matrices are redrawn N(0, 1 / sqrt(fan_in)) (query and key x 2), the biases N(0, 0.3), the LayerNorm
                        weights 1 + N(0, 0.2) and the tables N(0, 1); every parameter is rounded to a float16-representable
                        value BEFORE the model runs and is stored as float16 (exact; it halves the file)
  heads, eps            num_attention_heads and layer_norm_eps of the config
  input_ids, token_type_ids, attention_mask, lengths    B = 7, T = 12, prefix masks of the lengths, mixed token types;
                        padded ids and types are random
  last_hidden_state     the float32 model's, [B, T, 64]
  pooled_masked         sum(last_hidden_state * mask) / sum(mask), the reference encoder's own line, in float32 torch
  pooled_mean           last_hidden_state.mean(1), main2('QAEA')'s
  input_ids_alt, last_hidden_state_alt    the same batch with EVERY padded id replaced, and the float32 model's output on it
  err_states, err_masked, err_mean        max |float32 model - a float64 copy of the same model| for each output
"""
import copy
import math
import os

import numpy as np
import torch
from transformers import BertConfig, BertModel

HERE = os.path.dirname(os.path.abspath(__file__))
LENGTHS = [12, 1, 7, 3, 12, 2, 5]
B, T, VOCAB = len(LENGTHS), 12, 97

torch.manual_seed(20260200)
cfg = BertConfig(vocab_size=VOCAB, hidden_size=64, num_attention_heads=4, intermediate_size=128, num_hidden_layers=2,
                 max_position_embeddings=32, type_vocab_size=2, hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0)
assert cfg.hidden_act == "gelu" and cfg.layer_norm_eps == 1e-12
model = BertModel(cfg, add_pooling_layer=False).eval()
with torch.no_grad():
    for name, p in model.named_parameters():
        if "LayerNorm.weight" in name:
            p.copy_(1.0 + torch.randn_like(p) * 0.2)
        elif name.endswith("bias"):
            p.copy_(torch.randn_like(p) * 0.3)
        elif "embeddings." in name:
            p.copy_(torch.randn_like(p))
        else:
            scale = 2.0 if ("query" in name or "key" in name) else 1.0
            p.copy_(torch.randn_like(p) * (scale / math.sqrt(p.shape[1])))
    for p in model.parameters():
        p.copy_(p.half().float())
model64 = copy.deepcopy(model).double()

rng = np.random.default_rng(20260201)
ids = rng.integers(0, VOCAB, (B, T)).astype(np.int64)
types = rng.integers(0, 2, (B, T)).astype(np.int64)
mask = (np.arange(T)[None, :] < np.asarray(LENGTHS)[:, None]).astype(np.int64)
ids_alt = np.where(mask == 0, (ids + 1 + rng.integers(0, VOCAB - 1, ids.shape)) % VOCAB, ids)
assert ((ids_alt != ids) == (mask == 0)).all()


def run(m, ids):
    with torch.no_grad():
        s = m(input_ids=torch.from_numpy(ids), token_type_ids=torch.from_numpy(types), attention_mask=torch.from_numpy(mask)).last_hidden_state
        am = torch.from_numpy(mask)
        masked = torch.sum(s * am.unsqueeze(-1), dim=1) / torch.sum(am, dim=1).view(-1, 1)
        return s.numpy(), masked.numpy(), torch.mean(s, 1).numpy()


s32, masked32, mean32 = run(model, ids)
s64, masked64, mean64 = run(model64, ids)
assert s32.dtype == np.float32 and s64.dtype == np.float64
alt32, masked_alt, _ = run(model, ids_alt)
valid = mask.astype(bool)
print("padded ids replaced: valid rows bit-equal", np.array_equal(alt32[valid], s32[valid]), "masked pool bit-equal",
      np.array_equal(masked_alt, masked32), "padded rows changed", bool((alt32[~valid] != s32[~valid]).any()))

out = {"w:" + k: v.numpy().astype(np.float16) for k, v in model.state_dict().items()}
for k, v in model.state_dict().items():
    assert (out["w:" + k].astype(np.float32) == v.numpy()).all(), k
out.update(heads=np.int64(cfg.num_attention_heads), eps=np.float64(cfg.layer_norm_eps), input_ids=ids, token_type_ids=types,
           attention_mask=mask, lengths=np.asarray(LENGTHS, dtype=np.int64), last_hidden_state=s32, pooled_masked=masked32,
           pooled_mean=mean32, input_ids_alt=ids_alt, last_hidden_state_alt=alt32, err_states=np.abs(s32 - s64).max(),
           err_masked=np.abs(masked32 - masked64).max(), err_mean=np.abs(mean32 - mean64).max())
print(f"err_states {out['err_states']:.2e} err_masked {out['err_masked']:.2e} err_mean {out['err_mean']:.2e} scale {np.abs(s32).max():.2f}")
path = os.path.join(HERE, "bert_encoder.npz")
np.savez(path, **out)
print("wrote bert_encoder.npz", os.path.getsize(path), "bytes")
