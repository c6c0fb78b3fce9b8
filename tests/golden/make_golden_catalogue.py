"""Generates tests/golden/catalogue_heads.npz by RUNNING the reference's four catalogue functions on seeded small inputs.
Build container only (needs /root/reference):  python tests/golden/make_golden_catalogue.py

  get_next_product_asin_loss      train_subsession_embedding.py  (the live def; two more bodies of that name sit in strings)
  get_next_product_asin_accuracy  train_subsession_embedding.py
  get_all_product_asin_loss       train_session_embedding.py
  get_all_product_asin_accuracy   train_session_embedding.py

The files cannot be imported (torch_geometric at their tops), but the function bodies need torch and numpy only: each live
``def`` is located in its file's syntax tree, compiled on its own and called, as make_golden_pure.py does.  The stand-ins
supply INPUTS only: a namespace for ``data`` (``num_graphs``, ``['product_target' | 'product'].batch / .y``), a real
``nn.Embedding`` holding the item table, and a ``torch.rand`` that returns 0.0 where the project's hash
(tests/helpers/catalogue_ref.py) keeps an element and 1.0 elsewhere, so that the reference's ``rand < 1000 / V`` draws
exactly the project's mask; every other attribute of ``torch`` is torch's own.  The .npz holds the inputs, the mask seed and
the numbers the reference's code returned (and the element count of its final ``mean``) -- none of its text.

Inputs are stored compactly: the item table as int8 ``q`` with ``table = q / 64`` (exact in float32), the representations
as float32.  Cases (tag: V, B, d): a (257, 7, 200), b (4099, 64, 32), c (257, 1, 32, logits scaled so that both clip limits
are hit), e (4099, 7, 32).  Every case has a row without targets and a row with duplicate targets; the accuracies are taken
at K = 1 and 20 over rows whose top-K is not tied at the K-th place in the reference's own float32 values, with the same
top-K set as the float64 logits give (checked below; the seed is advanced until it holds).
"""
import ast
import os
import sys
import types

import numpy as np
import torch

REF = "/root/reference"
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), os.path.join(os.path.dirname(HERE), "helpers")]

import catalogue_ref as cr  # noqa: E402

N_NEG = 1000                                             # the reference's rate 1000 / V
KS = (1, 20)


class TorchWithRand:
    """``torch`` with ``rand`` replaced: 0.0 where the project's mask keeps (seed, row, item), 1.0 elsewhere; ``mean`` is
    torch's own and records the size of its argument (the reference returns no count)."""

    def __init__(self):
        self.seed = 0

    def rand(self, shape):
        B, V = shape
        return torch.from_numpy(np.where(cr.hash_rows(self.seed, np.arange(B), V) < np.uint32(min(cr.keep_threshold(N_NEG, V), 2 ** 32 - 1)),
                                         0.0, 1.0).astype(np.float32))

    def mean(self, x):
        """torch.mean, noting how many elements it was given: the loss functions' last mean is over the kept elements."""
        self.last_mean_numel = int(x.numel())
        return torch.mean(x)

    def __getattr__(self, name):
        return getattr(torch, name)


TORCH = TorchWithRand()


def extract(path, name):
    """The live top-level ``def name`` of a reference file (bodies inside string literals are no FunctionDef), compiled alone."""
    src = open(os.path.join(REF, path)).read()
    defs = [n for n in ast.parse(src).body if isinstance(n, ast.FunctionDef) and n.name == name]
    assert len(defs) == 1, (path, name, len(defs))
    ns = {"np": np, "torch": TORCH}
    exec(compile(ast.Module(body=defs, type_ignores=[]), os.path.join(REF, path), "exec"), ns)
    return ns[name]


next_loss = extract("train_subsession_embedding.py", "get_next_product_asin_loss")
next_acc = extract("train_subsession_embedding.py", "get_next_product_asin_accuracy")
all_loss = extract("train_session_embedding.py", "get_all_product_asin_loss")
all_acc = extract("train_session_embedding.py", "get_all_product_asin_accuracy")


class Data(dict):
    pass


def make_data(rows, key):
    """The batch as the reference reads it: the rows' item lists flattened, duplicates kept, with their graph index."""
    d = Data()
    d.num_graphs = len(rows)
    d[key] = types.SimpleNamespace(batch=torch.tensor([b for b, r in enumerate(rows) for _ in r], dtype=torch.long),
                                   y=torch.tensor([x for r in rows for x in r], dtype=torch.long))
    return d


def untied(vals, s64, rows, K):
    """Rows whose reference top-K is not tied at the K-th place and is the set the float64 logits give."""
    ok = []
    for b in rows:
        v = np.sort(vals[b])[::-1]
        if K < len(v) and not v[K - 1] > v[K]:
            return None
        if set(np.argsort(-vals[b], kind="stable")[:K].tolist()) != set(np.argsort(-s64[b], kind="stable")[:K].tolist()):
            return None
        ok.append(b)
    return ok


def case(tag, V, B, d, scale, seed):
    while True:
        r = np.random.default_rng(seed)
        q = r.integers(-64, 65, (V, d)).astype(np.int8)
        table = (q.astype(np.float32) / np.float32(64))
        rep = (scale * r.standard_normal((B, d)) / np.sqrt(d)).astype(np.float32)
        s64 = rep.astype(np.float64) @ table.astype(np.float64).T
        # targets: random items, and (so that the accuracies are not all zero) a few of the row's 30 best-scored ones
        rows = [r.choice(V, size=int(r.integers(1, 9)), replace=False).tolist() for _ in range(B)]
        rows = [sorted(set(x) | set(r.choice(np.argsort(-s64[b])[:30], size=int(r.integers(0, 4)), replace=False).tolist()))
                for b, x in enumerate(rows)]
        rows[0] = rows[0] + rows[0][:1] + rows[0][:1]                # duplicate targets
        if B > 1:
            rows[B // 2] = []                                          # a row without targets
        rows[-1] = sorted(set(rows[-1]) | {0, V - 1}) if B > 2 else rows[-1]
        emb = torch.nn.Embedding(V, d)
        with torch.no_grad():
            emb.weight.copy_(torch.from_numpy(table))
        with torch.no_grad():
            vals = torch.clip(torch.sigmoid(torch.from_numpy(rep) @ emb.weight.clone().T), min=1e-4, max=0.9999).numpy()
        if scale > 8 or all(untied(vals, s64, range(B), K) is not None for K in KS if K < V):
            break
        seed += 1000
    out = {"q": q, "rep": rep, "seed": np.uint64(seed), "V": np.int64(V)}
    ptr = np.zeros(B + 1, np.int64)
    np.cumsum([len(x) for x in rows], out=ptr[1:])
    out["ptr"], out["items"] = ptr, np.array([x for x in rows for x in x], np.int64)      # duplicates kept, any order
    TORCH.seed = seed
    with torch.no_grad():
        g = torch.from_numpy(rep)
        out["next_loss"] = np.float64(next_loss(g, None, make_data(rows, "product_target"), emb, "cpu").item())
        out["next_kept"] = np.int64(TORCH.last_mean_numel)
        nonempty = [x if x else [int(r.integers(0, V))] for x in rows]    # the all-product pair divides by len(gt): no empty row
        nptr = np.zeros(B + 1, np.int64)
        np.cumsum([len(x) for x in nonempty], out=nptr[1:])
        out["all_ptr"], out["all_items"] = nptr, np.array([x for x in nonempty for x in x], np.int64)
        out["all_loss"] = np.float64(all_loss(g, None, make_data(nonempty, "product"), emb, "cpu").item())
        out["all_kept"] = np.int64(TORCH.last_mean_numel)
        if scale <= 8:
            for K in KS:
                out[f"next_acc{K}"] = np.array(next_acc(g, None, make_data(rows, "product_target"), emb, K), np.float64)
                out[f"all_acc{K}"] = np.array(all_acc(g, None, make_data(nonempty, "product"), emb, K), np.float64)
    hit_lo, hit_hi = float((vals <= np.float32(1e-4)).mean()), float((vals >= np.float32(0.9999)).mean())
    print(f"case {tag}: V={V} B={B} d={d} seed={seed} next_loss={out['next_loss']:.6f} all_loss={out['all_loss']:.6f} "
          f"clipped low {hit_lo:.3f} high {hit_hi:.3f} |s|max={np.abs(s64).max():.2f}")
    if scale > 8:
        assert hit_lo > 0 and hit_hi > 0, "the clip case must hit both limits"
    return {f"{tag}_{k}": v for k, v in out.items()}


if __name__ == "__main__":
    out = {}
    out.update(case("a", 257, 7, 200, 3.0, 11))
    out.update(case("b", 4099, 64, 32, 3.0, 12))
    out.update(case("c", 257, 1, 32, 40.0, 13))
    out.update(case("e", 4099, 7, 32, 3.0, 14))
    out["tags"] = np.array(["a", "b", "c", "e"])
    out["ks"] = np.array(KS, np.int64)
    out["n_neg"] = np.int64(N_NEG)
    path = os.path.join(HERE, "catalogue_heads.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes,", len(out), "arrays")
