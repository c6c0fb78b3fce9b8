"""numpy restatement of include/sss_ptype.h: the type bags, the score of record -- integer arithmetic, one np.sqrt and one
division, both correctly rounded in float64 -- and, through the matrix of those scores, the (float32 score desc, id asc)
top-k, the bands and the mining loop, which are jaccard_ref's (they read nothing but the matrix)."""
import numpy as np

from jaccard_ref import FLT_MAX, bands, mine, recall, topk  # noqa: F401  (the restatements over a score matrix)


def bags(actions, item_type):
    """(ptr int64 [S + 1], types int32 ascending per session, counts float32) of an ActionTable: every non-search action
    whose item has a type (item_type[item] >= 0) adds one to its type's count."""
    ptr, types, counts = [0], [], []
    for s in range(actions.num_sessions):
        a, b = int(actions.sess_ptr[s]), int(actions.sess_ptr[s + 1])
        seen = {}
        for t in range(a, b):
            if not actions.is_search[t] and item_type[int(actions.item_id[t])] >= 0:
                ty = int(item_type[int(actions.item_id[t])])
                seen[ty] = seen.get(ty, 0) + 1
        types += sorted(seen)
        counts += [seen[ty] for ty in sorted(seen)]
        ptr.append(len(types))
    return np.asarray(ptr, np.int64), np.asarray(types, np.int32), np.asarray(counts, np.float32)


def triple(rows):
    """CSR triple of bags given as dicts {type: count} (or lists of (type, count))."""
    rows = [sorted(dict(r).items()) for r in rows]
    ptr = np.zeros(len(rows) + 1, np.int64)
    np.cumsum([len(r) for r in rows], out=ptr[1:])
    flat = [e for r in rows for e in r]
    return ptr, np.asarray([e[0] for e in flat], np.int32), np.asarray([e[1] for e in flat], np.float32)


def dense(b, n_types):
    """int64 [rows, n_types] count matrix of a bag triple."""
    ptr, types, counts = b
    m = np.zeros((len(ptr) - 1, n_types), np.int64)
    rows = np.repeat(np.arange(len(ptr) - 1), np.diff(ptr))
    lo, hi = int(ptr[0]), int(ptr[-1])
    m[rows, types[lo:hi]] = counts[lo:hi].astype(np.int64)
    return m


def scores(q, c, n_types=None):
    """The float64 score of record of every (query, corpus) pair: dot == 0 ? 0 : dot / sqrt(nq2 * nc2), the three integers
    exact in int64 and their float64 conversions exact (nq2 * nc2 <= 2^52)."""
    if n_types is None:
        n_types = int(max(q[1].max(initial=0), c[1].max(initial=0))) + 1
    Q, C = dense(q, n_types), dense(c, n_types)
    dot = Q @ C.T
    prod = (Q * Q).sum(1)[:, None] * (C * C).sum(1)[None, :]
    assert prod.max(initial=0) <= 2 ** 52 and dot.max(initial=0) < 2 ** 31
    root = np.sqrt(prod.astype(np.float64))
    return np.divide(dot.astype(np.float64), root, out=np.zeros(dot.shape, np.float64), where=dot != 0)


def ulp_distance(a, b):
    """Distance in units of the last place between non-negative float64 arrays (adjacent doubles are adjacent integers)."""
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    assert (a >= 0).all() and (b >= 0).all()
    return np.abs(a.view(np.int64) - b.view(np.int64))


def near_edge(s, edges, ulps):
    """Pairs whose score lies within `ulps` units of the last place of an edge."""
    near = np.zeros(s.shape, bool)
    for e in edges:
        near |= ulp_distance(s, np.full(s.shape, e)) <= ulps
    return near
