"""The string scores of record (include/ext/sss_seqsim.h) in plain Python: the documented
definitions of ``Levenshtein.ratio`` / ``seqratio`` restated, ``get_string_match`` and the reference's loops over a result
``I`` (``get_query_metric``, ``get_ave_score``, ``get_recall``).  Strings are ``str`` (``len`` counts code points),
sequences are lists of ``str``.  Imports nothing from the package."""
import numpy as np

_INDEL = {}


def lcs(a, b):
    """The longest common subsequence, row by row."""
    prev = [0] * (len(b) + 1)
    for ca in a:
        cur = [0]
        left = 0
        for j, cb in enumerate(b):
            left = prev[j] + 1 if ca == cb else (left if left > prev[j + 1] else prev[j + 1])
            cur.append(left)
        prev = cur
    return prev[-1]


def indel(a, b):
    """Insert and delete cost 1, a substitution 2: ``len(a) + len(b) - 2 LCS``."""
    key = (a, b) if a <= b else (b, a)
    if key not in _INDEL:
        _INDEL[key] = len(a) + len(b) - 2 * lcs(a, b)
    return _INDEL[key]


def ratio(a, b):
    L = len(a) + len(b)
    return 1.0 if L == 0 else (L - indel(a, b)) / L


def ratio_match(a, b):
    """``ratio(a, b) > 0.9``, decided in integers."""
    L = len(a) + len(b)
    return L == 0 or L > 10 * indel(a, b)


def cost(a, b):
    L = len(a) + len(b)
    return 0.0 if L == 0 else (2.0 / L) * indel(a, b)            # the division rounded first, the product second


def seqdist(A, B):
    n1, n2 = len(A), len(B)
    T = [[float(j) for j in range(n2 + 1)]] + [[float(i)] + [0.0] * n2 for i in range(1, n1 + 1)]
    for i in range(1, n1 + 1):
        for j in range(1, n2 + 1):
            T[i][j] = min(T[i - 1][j] + 1.0, T[i][j - 1] + 1.0, T[i - 1][j - 1] + cost(A[i - 1], B[j - 1]))
    return T[n1][n2]


def seqratio(A, B):
    n = len(A) + len(B)
    return 1.0 if n == 0 else (n - seqdist(A, B)) / n


def strip_common(A, B):
    """The two lists without their common prefix and suffix of equal strings (what the library does first)."""
    A, B = list(A), list(B)
    while A and B and A[0] == B[0]:
        A, B = A[1:], B[1:]
    while A and B and A[-1] == B[-1]:
        A, B = A[:-1], B[:-1]
    return A, B


def string_match(A, B):
    """``get_string_match``: how many strings of A match some string of B, and of B some of A (positions, not sets)."""
    am, bm = [0] * len(A), [0] * len(B)
    for i, a in enumerate(A):
        for j, b in enumerate(B):
            if ratio_match(a, b):
                am[i] = bm[j] = 1
    return sum(am), sum(bm)


def lcs_words(a, b):
    """LCS by the bit-parallel recurrence V' = (V + (V & M)) | (V & ~M) over 64-bit words with the carry passed from word
    to word, as the kernel runs it: the zero bits of V.  ``a`` is the string in words."""
    nw = (len(a) + 63) // 64
    full = (1 << 64) - 1
    V = [full] * nw
    for c in b:
        carry = 0
        for w in range(nw):
            M = sum(1 << l for l, ch in enumerate(a[64 * w:64 * w + 64]) if ch == c)
            s = V[w] + (V[w] & M) + carry
            carry = s >> 64
            V[w] = (s & full) | (V[w] & ~M & full)
    return sum(bin(~v & full).count("1") for v in V)


def near_duplicates(rng, n, alphabet="abcdefg ", lo=0, hi=24):
    """``n`` strings: a few random bases and edits of them, so that many pairs sit near the 0.9 match edge."""
    out = []
    while len(out) < n:
        if out and rng.random() < 0.7:
            s = list(rng.choice(out))
            for _ in range(rng.randint(0, 3)):
                k = rng.randint(0, len(s))
                if s and rng.random() < 0.5:
                    del s[min(k, len(s) - 1)]
                else:
                    s.insert(k, rng.choice(alphabet))
            out.append("".join(s))
        else:
            out.append("".join(rng.choice(alphabet) for _ in range(rng.randint(lo, hi))))
    return out


# ------------------------------------------------------------------------------------------------ over a result I
def pair_scores(I, Q, C, id_offset=0):
    """``(ratio, qmatch, cmatch, clen)`` as sss_seq_pair_scores writes them: -1 is a missing neighbour."""
    I = np.asarray(I)
    ratio_ = np.full(I.shape, np.nan)
    qm, cm, cl = np.zeros(I.shape, np.int32), np.zeros(I.shape, np.int32), np.full(I.shape, -1, np.int32)
    memo = {}
    for i in range(I.shape[0]):
        for j in range(I.shape[1]):
            if I[i, j] == -1:
                continue
            r = int(I[i, j]) - id_offset
            key = (tuple(Q[i]), r)
            if key not in memo:
                memo[key] = (seqratio(Q[i], C[r]),) + string_match(Q[i], C[r])
            ratio_[i, j], qm[i, j], cm[i, j] = memo[key]
            cl[i, j] = len(C[r])
    return ratio_, qm, cm, cl


def query_metric_sums(qm, cm, cl, qlen):
    """sss_seq_query_metric: float64 sums in ascending j."""
    out = np.zeros((qm.shape[0], 2))
    for i in range(qm.shape[0]):
        for j in range(qm.shape[1]):
            if cl[i, j] < 0:
                continue
            if qlen[i] + cl[i, j]:
                out[i, 0] += float(qm[i, j] + cm[i, j]) / float(qlen[i] + cl[i, j])
            if qlen[i]:
                out[i, 1] += float(qm[i, j]) / float(qlen[i])
    return out


MODES, METRICS = ("all", "cur", "future"), ("score", "recall")


def get_query_metric(I, parts, C, mode, metric):
    """The reference's loop; ``parts``: {'cur' | 'future' | 'all': list of lists}.  A missing neighbour adds no value."""
    if mode not in MODES:
        raise RuntimeError("unrecognized mode", mode)
    vals = []
    for i, query in enumerate(parts[mode]):
        if len(query) == 0:
            continue
        for d in np.asarray(I)[i]:
            if d == -1:
                continue
            session = C[int(d)]
            qm, sm = string_match(query, session)
            if metric == "score":
                vals.append(0 if len(query) + len(session) == 0 else float(qm + sm) / (len(query) + len(session)))
            else:
                vals.append(float(qm) / len(query))
    return float(np.mean(vals)) if vals else float("nan")


def get_score(A, B, sim_type):
    if sim_type == "all_query_score":
        return 0 if len(A) == 0 or len(B) == 0 else seqratio(A, B)
    assert sim_type == "all_product_title_score"
    return seqratio(A, B)


def score_matrix(I, Q, C, sim_type):
    """The reference's ``gt``: float32, a missing neighbour 0."""
    I = np.asarray(I)
    gt = np.zeros(I.shape, np.float32)
    for i in range(I.shape[0]):
        for j in range(I.shape[1]):
            if I[i, j] != -1:
                gt[i, j] = get_score(Q[i], C[int(I[i, j])], sim_type)
    return gt


def get_ave_score(I, Q, C, sim_type):
    """The float64 mean of the float32 pair scores (their sum is exact in float64 at any order: 24-bit values in [0, 1])."""
    gt = score_matrix(I, Q, C, sim_type)
    return float(gt.astype(np.float64).sum()) / gt.size


def get_recall(Q, C, I, sim_type, thres):
    gt = score_matrix(I, Q, C, sim_type)
    return float(np.mean(np.sum(gt > np.float32(thres), axis=1))) / float(gt.shape[1])
