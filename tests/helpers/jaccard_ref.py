"""numpy restatement of include/sss_jaccard.h.  An item-set batch is the (ptr, items) pair of a CSR triple."""
import numpy as np

FLT_MAX = np.float32(3.4028234663852886e38)


def ratios(q, c):
    """float64 inter / uni of every (query, corpus) pair, 0 where the union is empty; the score of record is its float32."""
    qs = [set(q[1][q[0][i]:q[0][i + 1]].tolist()) for i in range(len(q[0]) - 1)]
    cs = [set(c[1][c[0][r]:c[0][r + 1]].tolist()) for r in range(len(c[0]) - 1)]
    inter = np.array([[len(a & b) for b in cs] for a in qs], np.float64).reshape(len(qs), len(cs))
    uni = np.array([[len(a | b) for b in cs] for a in qs], np.float64).reshape(len(qs), len(cs))
    return np.divide(inter, uni, out=np.zeros_like(inter), where=uni > 0)


def topk(r, k, id_offset=0):
    """(D float32, I int64) [nq, k]: the k best by a stable sort on (-float32 score, id); padding (-FLT_MAX, -1)."""
    s = r.astype(np.float32)
    order = np.argsort(-s, axis=1, kind="stable")[:, :k]
    D, I = np.full((s.shape[0], k), -FLT_MAX, np.float32), np.full((s.shape[0], k), -1, np.int64)
    D[:, :order.shape[1]], I[:, :order.shape[1]] = np.take_along_axis(s, order, axis=1), order + id_offset
    return D, I


def bands(r, edges, id_offset=0):
    """(counts, first) int64 [nq, len(edges) + 1]: band = number of edges with ratio >= edge, compared in float64."""
    band = (r[:, :, None] >= np.asarray(edges, np.float64)[None, None, :]).sum(2)
    nb = len(edges) + 1
    if r.shape[1] == 0:
        return np.zeros((r.shape[0], nb), np.int64), np.full((r.shape[0], nb), -1, np.int64)
    counts = np.stack([(band == b).sum(1) for b in range(nb)], 1).astype(np.int64)
    first = np.stack([np.where((band == b).any(1), (band == b).argmax(1) + id_offset, -1) for b in range(nb)], 1).astype(np.int64)
    return counts, first


def mine(r, lo=0.2, hi=0.8):
    """The mining rule of fine_tune_ours.py:199-227 for every query: (ids [nq, 3] as pos, half, neg; -1 none), (scores, nan
    none), keep = all three found."""
    ids, sc = np.full((r.shape[0], 3), -1, np.int64), np.full((r.shape[0], 3), np.nan)
    for f in range(r.shape[0]):
        for i, s in enumerate(r[f]):
            slot = 0 if s >= hi else 1 if s >= lo else 2
            if ids[f, slot] < 0:
                ids[f, slot], sc[f, slot] = i, s
            if (ids[f] >= 0).all():
                break
    return ids, sc, (ids >= 0).all(1)


def recall(I, r, thres):
    """(mean, skipped) of jaccard.neighbourhood_recall for ids without an offset (-1: missing)."""
    vals, skipped = [], 0
    for f in range(r.shape[0]):
        den = int((r[f] > thres).sum())
        if den == 0:
            skipped += 1
            continue
        vals.append(sum(1 for j in I[f] if j >= 0 and r[f, j] > thres) / den)
    return (float(np.mean(np.asarray(vals, np.float64))) if vals else float("nan")), skipped
