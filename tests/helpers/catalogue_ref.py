"""Host restatement of the catalogue heads (include/heads/sss_catalogue.h), TEST INFRASTRUCTURE ONLY: the mask hash in numpy
uint64, the logits from ``oracle.search_ref.linear_chain`` on the zero-extended operands (the kernel's own fma chain, bit for
bit), the loss terms in float64, and the accuracy by Python sets as the reference computes it."""
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle import search_ref as sr  # noqa: E402

M64 = (1 << 64) - 1
GOLDEN, MUL1, MUL2 = 0x9E3779B97F4A7C15, 0xBF58476D1CE4E5B9, 0x94D049BB133111EB
_f = np.float32
# the four clamp limits, derived here (the header's literals are compared with these)
P_LO = float(_f(-math.log(float(_f(0.9999)))))
P_HI = float(_f(-math.log(float(_f(1e-4)))))
N_LO = float(_f(-math.log(float(_f(1) - _f(1e-4)))))
N_HI = float(_f(-math.log(float(_f(1) - _f(0.9999)))))


def hash_scalar(seed, g, i, V):
    """H(seed, g, i) of the header in Python integers."""
    x = (seed + (g * V + i) * GOLDEN) & M64
    x = ((x ^ (x >> 30)) * MUL1) & M64
    x = ((x ^ (x >> 27)) * MUL2) & M64
    x ^= x >> 31
    return x >> 32


def hash_rows(seed, rows, V):
    """H for every (g in rows, i in range(V)): uint32 [len(rows), V], in numpy uint64 arithmetic (wrapping)."""
    with np.errstate(over="ignore"):
        g = np.asarray(rows, np.uint64)[:, None]
        i = np.arange(V, dtype=np.uint64)[None, :]
        x = np.uint64(seed) + (g * np.uint64(V) + i) * np.uint64(GOLDEN)
        x = (x ^ (x >> np.uint64(30))) * np.uint64(MUL1)
        x = (x ^ (x >> np.uint64(27))) * np.uint64(MUL2)
        x = x ^ (x >> np.uint64(31))
    return (x >> np.uint64(32)).astype(np.uint32)


def keep_threshold(n_neg, V):
    """floor(min(1, n_neg / V) * 2^32); 2^32 keeps every negative."""
    return 1 << 32 if n_neg == "all" or n_neg >= V else (int(n_neg) << 32) // V


def keep_mask(seed, rows, V, n_neg):
    thr = keep_threshold(n_neg, V)
    if thr >> 32:
        return np.ones((len(rows), V), bool)
    return hash_rows(seed, rows, V) < np.uint32(thr)


def pad32(x):
    x = np.ascontiguousarray(x, np.float32)
    k = (x.shape[1] + 31) // 32 * 32
    out = np.zeros((x.shape[0], k), np.float32)
    out[:, :x.shape[1]] = x
    return out


def logits(rep, table):
    """float32 [B, V]: the kernel's logits, bit for bit."""
    return sr.linear_chain(pad32(rep), pad32(table))


def target_matrix(ptr, items, V):
    y = np.zeros((len(ptr) - 1, V), bool)
    for b in range(len(ptr) - 1):
        y[b, np.asarray(items[ptr[b]:ptr[b + 1]], np.int64)] = True
    return y


def softplus64(z):
    z = np.asarray(z, np.float64)
    return np.maximum(z, 0.0) + np.log1p(np.exp(-np.abs(z)))


def clamp_nan(t, lo, hi):
    """The kernel's clamp: a NaN passes through."""
    return np.where(t < lo, lo, np.where(t > hi, hi, t))


def terms64(s, y):
    """float64 [B, V]: every pair's loss term as the header defines it, from float32 logits ``s`` and the target matrix."""
    s = np.asarray(s, np.float32).astype(np.float64)
    return np.where(y, clamp_nan(softplus64(-s), P_LO, P_HI), clamp_nan(softplus64(s), N_LO, N_HI))


def bce(s, ptr, items, n_neg=1000, seed=0, row_offset=0):
    """``(loss, sums float64 [B, 2], counts int64 [B, 2])`` from the logits ``s`` [B, V]."""
    B, V = s.shape
    y = target_matrix(ptr, items, V)
    t = terms64(s, y)
    neg = keep_mask(seed, row_offset + np.arange(B), V, n_neg) & ~y
    sums = np.stack([np.where(y, t, 0.0).sum(1), np.where(neg, t, 0.0).sum(1)], 1)    # (a NaN outside the kept set is not seen)
    counts = np.stack([y.sum(1), neg.sum(1)], 1).astype(np.int64)
    kept = int(counts.sum())
    return (float(sums.sum()) / kept if kept else float("nan")), sums, counts


def topk(rep, table, K):
    """(D, I) by (score desc, id asc): the exact search of the oracle."""
    return sr.search_exact(np.ascontiguousarray(rep, np.float32), np.ascontiguousarray(table, np.float32), K)


def hits(I, ptr, items):
    """Per row: the distinct ids of I[b] in the row's target set."""
    return np.array([len(set(int(x) for x in I[b]) & set(int(x) for x in items[ptr[b]:ptr[b + 1]])) for b in range(len(ptr) - 1)], np.int64)


def accuracy(I, ptr, items, skip_empty):
    """(precision, recall) as the reference's loops compute them: np.mean of the per-row Python floats."""
    K = I.shape[1]
    precision, recall = [], []
    for b in range(len(ptr) - 1):
        gt = set(int(x) for x in items[ptr[b]:ptr[b + 1]])
        if len(gt) == 0 and skip_empty:
            continue
        hit = float(len(gt & set(int(x) for x in I[b])))
        precision.append(hit / K)
        recall.append(hit / len(gt))
    return float(np.mean(precision)), float(np.mean(recall))


def csr(rows):
    """Lists of item ids (any order, duplicates allowed) -> (ptr int64, items int32) with rows strictly ascending."""
    ptr, items = [0], []
    for r in rows:
        u = sorted(set(int(x) for x in r))
        items += u
        ptr.append(len(items))
    return np.array(ptr, np.int64), np.array(items, np.int32)
