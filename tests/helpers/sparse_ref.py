"""numpy float64 oracle of the sparse session index (DESIGN.md "sparse session index"): session-vector weights, canonical
scores and the (score desc, id asc) top-k.  Plain loops and sequential sums -- the order of every sum is the contract's."""
import numpy as np

FLT_MAX = np.float32(3.4028234663852886e38)


def vectors(actions, mode="binary", lammy=None):
    """(ptr int64 [S + 1], items int32, weights float32) of an ActionTable: items ascending per session; weights in
    float64, rounded once."""
    ptr, items, weights = [0], [], []
    for s in range(actions.num_sessions):
        a, b = int(actions.sess_ptr[s]), int(actions.sess_ptr[s + 1])
        seq = [int(actions.item_id[t]) for t in range(a, b) if not actions.is_search[t]]
        L = len(seq)
        assert L <= 64
        u = {}
        for i, it in enumerate(seq):                                  # action order
            w = np.exp(np.float64(i - L) / np.float64(lammy)) if mode == "stan" else np.float64(1.0)
            u[it] = (u.get(it, np.float64(0.0)) + w) if mode == "stan" else w
        ids = sorted(u)
        if mode == "stan":
            ss = np.float64(0.0)
            for it in ids:                                            # ascending item order
                ss = ss + u[it] * u[it]
            w = [u[it] / np.sqrt(ss) for it in ids]
        else:
            w = [np.float64(1.0) / np.sqrt(np.float64(len(ids)))] * len(ids) if ids else []
        items += ids
        weights += w
        ptr.append(len(items))
    return np.asarray(ptr, np.int64), np.asarray(items, np.int32), np.asarray(weights, np.float64).astype(np.float32)


def scores(q, c, n_items):
    """Canonical float32 scores [nq, n] of CSR triples q against c: per query, its items ascending; per item, every row
    holding it gets (double)wq * (double)wc added to its float64 sum (a row holds an item once, so each row's sum runs
    in ascending item order)."""
    qp, qi, qw = q
    cp, ci, cw = c
    n = len(cp) - 1
    rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(cp))
    order = np.argsort(ci, kind="stable")                            # postings: rows of every item
    post_rows, post_w = rows[order], cw[order].astype(np.float64)
    start = np.searchsorted(ci[order], np.arange(n_items + 1))
    out = np.empty((len(qp) - 1, n), np.float32)
    for f in range(len(qp) - 1):
        acc = np.zeros(n, np.float64)
        assert np.all(np.diff(qi[qp[f]:qp[f + 1]]) > 0)
        for p in range(qp[f], qp[f + 1]):
            lo, hi = start[qi[p]], start[qi[p] + 1]
            acc[post_rows[lo:hi]] += np.float64(qw[p]) * post_w[lo:hi]
        out[f] = acc.astype(np.float32)
    return out


def topk(s, k, id_offset=0):
    """(D float32 [nq, k], I int64 [nq, k]) by (score desc, id asc), ids = row + id_offset, padding (-FLT_MAX, -1)."""
    nq, n = s.shape
    D = np.full((nq, k), -FLT_MAX, np.float32)
    I = np.full((nq, k), -1, np.int64)
    kk = min(k, n)
    for f in range(nq):
        if kk < n:
            t = np.partition(s[f], n - kk)[n - kk]                   # the kk-th best value
            cand = np.flatnonzero(s[f] >= t)
        else:
            cand = np.arange(n)
        o = cand[np.lexsort((cand, -s[f, cand].astype(np.float64)))][:kk]
        D[f, :kk], I[f, :kk] = s[f, o], o + id_offset
    return D, I


def search(q, c, n_items, k, id_offset=0):
    return topk(scores(q, c, n_items), k, id_offset)
