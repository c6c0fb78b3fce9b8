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


# ---------------------------------------------------------------------------------------------- variants and generators
# What follows serves tests/test_sparse_edges_*.py: restatements of `scores` that break the contract on purpose (so a test
# can show that its inputs tell them apart), a per-pair oracle that needs no table over the vocabulary, and the corpora.
def scores_variant(q, c, n_items, descending=False, acc=np.float64):
    """`scores` with the query's items walked in descending order and / or the running sum kept in `acc` (float32: the
    float64 sum of the running float32 value and the exact product, rounded after every step).  With the defaults it is
    `scores`."""
    qp, qi, qw = q
    cp, ci, cw = c
    n = len(cp) - 1
    rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(cp))
    order = np.argsort(ci, kind="stable")
    post_rows, post_w = rows[order], cw[order].astype(np.float64)
    start = np.searchsorted(ci[order], np.arange(n_items + 1))
    out = np.empty((len(qp) - 1, n), np.float32)
    for f in range(len(qp) - 1):
        a = np.zeros(n, acc)
        walk = range(qp[f], qp[f + 1])
        for p in (reversed(walk) if descending else walk):
            lo, hi = start[qi[p]], start[qi[p] + 1]
            r = post_rows[lo:hi]
            a[r] = (a[r].astype(np.float64) + np.float64(qw[p]) * post_w[lo:hi]).astype(acc)
        out[f] = a.astype(np.float32)
    return out


def scores_descending(q, c, n_items):
    return scores_variant(q, c, n_items, descending=True)


def scores_float32(q, c, n_items):
    return scores_variant(q, c, n_items, acc=np.float32)


def scores_pairs(q, c):
    """Canonical scores by the definition alone, pair by pair: the shared items of (query, row) ascending, one float64
    sum.  Slow; needs no table over the vocabulary, so it serves item ids up to 2^31 - 2."""
    qp, qi, qw = q
    cp, ci, cw = c
    out = np.empty((len(qp) - 1, len(cp) - 1), np.float32)
    for f in range(len(qp) - 1):
        a = qi[qp[f]:qp[f + 1]]
        for r in range(len(cp) - 1):
            b = ci[cp[r]:cp[r + 1]]
            _, ia, ib = np.intersect1d(a, b, assume_unique=True, return_indices=True)     # ascending
            s = np.float64(0.0)
            for x, y in zip(ia, ib):
                s = s + np.float64(qw[qp[f] + x]) * np.float64(cw[cp[r] + y])
            out[f, r] = np.float32(s)
    return out


def triple(rows):
    """CSR triple of rows given as [(items ascending, weights)]."""
    ptr = np.zeros(len(rows) + 1, np.int64)
    np.cumsum([len(r[0]) for r in rows], out=ptr[1:])
    items = np.concatenate([np.asarray(r[0], np.int64) for r in rows] + [np.zeros(0, np.int64)]).astype(np.int32)
    weights = np.concatenate([np.asarray(r[1], np.float32) for r in rows] + [np.zeros(0, np.float32)]).astype(np.float32)
    return ptr, items, weights


def rows_of(t, lo=0, hi=None):
    """Rows lo..hi of a triple as a triple of their own (ptr from 0, only their entries)."""
    hi = len(t[0]) - 1 if hi is None else hi
    return t[0][lo:hi + 1] - t[0][lo], t[1][t[0][lo]:t[0][hi]].copy(), t[2][t[0][lo]:t[0][hi]].copy()


def wave_kinds(ptr, limit=16):
    """Per 64 rows, as k_sparse_scores groups them (256 rows a block, 64 a wave, the last wave padded with inactive
    lanes): (longest row, number of rows longer than `limit`, their lanes, active lanes)."""
    ln = np.diff(ptr)
    out = []
    for w in range(0, len(ln), 64):
        seg = ln[w:w + 64]
        out.append((int(seg.max()), int((seg > limit).sum()), np.flatnonzero(seg > limit).tolist(), len(seg)))
    return out


EDGE_ITEMS = 110            # vocabulary of the edge corpora; rows draw from [EDGE_LO, EDGE_HI), queries from all of it
EDGE_LO, EDGE_HI = 4, 104
SHORT = (0, 1, 2, 15, 16)
LONG = (17, 18, 31, 32, 33, 63, 64, 65, 94)


def _row(rng, m, lo, hi, binary):
    it = np.sort(rng.choice(np.arange(lo, hi), m, replace=False))
    if binary:
        return it, np.full(m, np.float32(1.0 / np.sqrt(np.float64(max(m, 1)))), np.float32)
    return it, (rng.standard_normal(m) * np.exp2(rng.integers(-3, 4, m))).astype(np.float32)


def edge_lengths(rng):
    """Row lengths of the edge corpus, wave by wave (n = 933 = 3 * 256 + 2 * 64 + 37):
      block 0   four short waves; the second one's longest row is exactly 16
      block 1   four long waves; the first one has long rows only
      block 2   short waves with exactly one long row at lane 0 / lane 63 / lane 29, then a short wave
      block 3   a wave whose longest row is 16 beside one whose longest is 17, then 37 rows, the last one long"""
    short = lambda k: rng.choice(SHORT, k)
    waves = [short(64), np.r_[short(63), 16], short(64), short(64)]
    waves += [rng.choice(LONG, 64)] + [rng.choice(SHORT + LONG, 64) for _ in range(3)]
    for w in waves[5:8]:
        w[rng.integers(0, 64)] = 94
    for lane, m in ((0, 33), (63, 17), (29, 94)):
        w = short(64)
        w[lane] = m
        waves.append(w)
    waves.append(short(64))
    w16 = rng.choice(SHORT[:4], 64); w16[7] = 16
    w17 = rng.choice(SHORT, 64); w17[40] = 17
    tail = short(37); tail[-1] = 65
    waves += [w16, w17, tail]
    return np.concatenate(waves).astype(np.int64)


def edge_corpus(seed=0, lengths=None):
    """The edge corpus: rows of the given lengths over [EDGE_LO, EDGE_HI), every other row with binary weights (ties),
    the rest with signed ones."""
    rng = np.random.default_rng(seed)
    lengths = edge_lengths(rng) if lengths is None else lengths
    return triple([_row(rng, int(m), EDGE_LO, EDGE_HI, r % 2 == 0) for r, m in enumerate(lengths)])


def edge_queries(c, seed=1, nq=40):
    """Queries of lengths {0, 1, 2, 3, 9, 16, 17, 40, 94} over the whole vocabulary; the first five are: all items
    below every row item, all above (the walk ends on the sentinel), equal to the longest row, equal to a short row,
    empty."""
    rng = np.random.default_rng(seed)
    ln = np.diff(c[0])
    long_row, short_row = int(np.argmax(ln)), int(np.flatnonzero(ln == 2)[0])
    same = lambda r: (c[1][c[0][r]:c[0][r + 1]].astype(np.int64), c[2][c[0][r]:c[0][r + 1]])
    rows = [_row(rng, EDGE_LO, 0, EDGE_LO, False), _row(rng, EDGE_ITEMS - EDGE_HI, EDGE_HI, EDGE_ITEMS, False),
            same(long_row), same(short_row), _row(rng, 0, 0, 1, False)]
    lens = (0, 1, 2, 3, 9, 16, 17, 40, 94)
    rows += [_row(rng, lens[i % len(lens)], 0, EDGE_ITEMS, i % 3 == 0) for i in range(nq - len(rows))]
    return triple(rows)


def _mant(rng, size, e_lo, e_hi):
    """m * 2^e as float32: m in [1, 2), e in e_lo..e_hi."""
    return ((1.0 + rng.random(size)) * np.exp2(rng.integers(e_lo, e_hi + 1, size).astype(np.float64))).astype(np.float32)


def sum_order_batch(seed=5, n=700, nq=24, n_items=96, hot=(30, 60)):
    """(q, c, n_items) on which the order and the precision of the sum show.  Every query holds both hot items with one
    weight g = m * 2^(-5..5); about half of the rows with two or more items hold both, +B on the first and -B on the
    second, B = m * 2^(90..100); every other weight is +-m * 2^(-20..20).  Ascending, the terms ahead of the second hot
    item are absorbed by g * B and cancelled with it, so the score is the sum of the terms behind it; descending, of
    the terms ahead of the first; a float32 sum loses the low bits that float64 keeps.  Every score is finite."""
    rng = np.random.default_rng(seed)
    rest = np.setdiff1d(np.arange(n_items), hot)

    def signed(m):
        return _mant(rng, m, -20, 20) * rng.choice(np.float32([-1, 1]), m)

    def make(m, with_hot, hot_w):
        if with_hot:
            it = np.sort(np.r_[rng.choice(rest, m - 2, replace=False), hot])
        else:
            it = np.sort(rng.choice(np.arange(n_items), m, replace=False))
        w = signed(m)
        if with_hot:
            w[it == hot[0]], w[it == hot[1]] = hot_w
        return it, w

    lens = rng.choice(SHORT + LONG, n)
    rows = []
    for m in lens:
        B = _mant(rng, 1, 90, 100)[0]
        rows.append(make(int(m), m >= 2 and rng.random() < 0.5, (B, -B)))
    qlens = (2, 3, 9, 16, 17, 40, 94)
    qs = []
    for f in range(nq):
        g = _mant(rng, 1, -5, 5)[0]
        qs.append(make(qlens[f % len(qlens)], True, (g, g)))
    return triple(qs), triple(rows), n_items
