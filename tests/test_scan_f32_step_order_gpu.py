"""The half-step skew of the f32 list scan for 512-byte rows (csrc/scan_kernel.h, "F32S", the half-step skew): each
accumulator of a 64-row step is decided under the other accumulator's MFMAs, across the step boundary, and the hot loop
has one exit per half.  None of it may change a result.

Every case goes through ``FlatIndex(128, metric, dtype="f32", scan="f32")`` and is compared with ``array_equal`` -- no
tolerance -- against the oracle: ``search_ref.search_exact`` (score descending, then id ascending) for the inner product;
for L2 what the L2 tests of the suite use, ``topk_from_scores(canonical_l2(q, c), k, largest=False)`` (``search_exact``
scores inner products only; the values are canonical_l2's own, computed in row blocks).  Both metrics, k = 1, 10, 14
(bootstrap tile, K2 = 8, 12, 16) and k = 20 (no bootstrap: every step is live).  After each search
``sss_scan_boot_expired(1)`` must be 0.

Shapes (``make_plan``, csrc/scan.hip):

* ``tiles64_a``: nq 256 (one query group), n = 192 * 64 + 1: 192 splits of two 64-row tiles (one step a tile: every step
  ends with a hand-over), the last tile holds ONE row -- only acc0 has a real row in the last step.
* ``tiles64_b``: nq 256, n = 552 * 64 + 33: 256 splits of three 64-row tiles, the last tile holds 33 rows -- acc1 has
  exactly one.
* ``tiles128``: nq 1024 (four groups -> 64 splits), n = 64 * 128 * 48 + 128 + 33: 128-row tiles (two steps a tile), 49 a
  split, the last split shorter, one split empty, the last step ragged inside acc1.  64 queries go to the oracle.

The background rows are random unit rows scaled by 0.5; planted rows are exact copies of chosen (unit) queries, so they
pass whatever the threshold is, and equal copies of one query tie: the order among them is by id.  They sit where the
new control flow can go wrong (``_plant``): step-local rows 0, 31, 32, 63; both halves of one step for one query; two
rows of one lane in one step (the pending slot); 18 rows of one lane in one step (more than the 16 of a lane list:
``maxlast``); the last step of a tile and the first of the next (across the hand-over); a split's first tile (scanned
max-only first and live as the last iteration); the corpus's last, ragged step; the very last step of a split."""
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

from oracle import search_ref as sr

D_ = 128
KS = (1, 10, 14, 20)
# name -> (nq, n, tile rows, tiles per split, splits with tiles)
SHAPES = {
    "tiles64_a": (256, 192 * 64 + 1, 64, 2, 97),
    "tiles64_b": (256, 552 * 64 + 33, 64, 3, 185),
    "tiles128": (1024, 64 * 128 * 48 + 128 + 33, 128, 49, 63),
}
_cache = {}


def _unit(rng, n, d):
    v = rng.standard_normal((n, d), dtype=np.float32)
    return (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(np.float32)


def _plant(c, q, nq, n, tr, tps, active):
    """Copies of chosen queries at the rows named in the module docstring; returns {query: planted rows}."""
    span = tr * tps                                  # rows of a full split
    planted = {}

    def put(qi, rows):
        for row in rows:
            assert 0 <= row < n and not any(row in v for v in planted.values()), row
            c[row] = q[qi]
        planted.setdefault(qi, []).extend(rows)

    qs = iter([w * 32 + lane for lane in (0, 1, 13, 30, 31, 7, 18) for w in range(8)])       # every wave of a group
    mid = 3 * span + (tr if tps > 2 else 0)          # first row of a middle tile of split 3 (two-tile splits: its first)
    put(next(qs), [mid + 0, mid + 31, mid + 32, mid + 63])                      # the corners of both halves of a step
    put(next(qs), [mid + 5, mid + 37])                                          # both halves, the same lane
    put(next(qs), [mid + 8, mid + 9])                                           # two rows of one lane (h = 0) of acc0
    put(next(qs), [mid + 44, mid + 47])                                         # ... and of acc1 (h = 1)
    lane_rows = [b + j for b in (0, 8, 16, 24) for j in range(4)] + [32, 33]     # 16 of acc0 + 2 of acc1, lane h = 0
    put(next(qs), [5 * span + r for r in lane_rows])                            # 18 rows of one lane, a split's first step
    put(next(qs), [7 * span + (tps - 1) * tr + r + 4 for r in lane_rows])       # ... (h = 1) a split's last tile
    put(next(qs), [9 * span + tr - 1, 9 * span + tr])                           # last row of a tile, first of the next
    put(next(qs), [9 * span + tr - 33, 9 * span + tr + 32])                     # ... acc0 of its last step, acc1 of the next's first
    put(next(qs), [11 * span + 0, 11 * span + 33])                              # a split's first tile
    put(next(qs), [11 * span + span - 1, 11 * span + span - 64])                # the very last step of a split
    put(next(qs), [12 * span + span - 32, 12 * span + span - 33])               # ... its acc1 / acc0 boundary
    put(next(qs), [n - 1])                                                      # the corpus's last row (ragged step)
    if n % 64 > 1:
        put(next(qs), [n - (n % 64), n - 2])                                    # ... the ragged step's first row, its acc0
    pen = (active - 2) * span                        # the last FULL split (the one behind it ends with the ragged step)
    put(next(qs), [pen, pen + span - 1])
    if nq > 256:                                     # the other query groups: a row in both halves of one step
        for g in range(1, nq // 256):
            put(g * 256 + 37 * g, [13 * span + 64 * g + 2 * g, 13 * span + 64 * g + 40 + g])
    return planted


def _data(shape):
    if shape not in _cache:
        nq, n, tr, tps, active = SHAPES[shape]
        rng = np.random.default_rng([20261020, nq, n])
        q = _unit(rng, nq, D_)
        c = _unit(rng, n, D_)
        c *= np.float32(0.5)
        planted = _plant(c, q, nq, n, tr, tps, active)
        chosen = sorted(planted)
        rest = [i for i in (np.arange(0, nq, max(1, nq // 64)) + 3) % nq if i not in planted]
        sel = np.array(sorted(chosen + rest[:max(0, 64 - len(chosen))]), np.int64)
        assert len(sel) == 64 and set(chosen) <= set(sel.tolist())
        _cache[shape] = (c, q, sel, planted)
    return _cache[shape]


def _l2_dist(q, c):
    """canonical_l2 in row blocks (it is elementwise in (query, row): the values are its own), blocks side by side."""
    key = ("l2", id(c), q.shape[0])
    if key not in _cache:
        blocks = [(lo, min(lo + 4096, c.shape[0])) for lo in range(0, c.shape[0], 4096)]
        with ThreadPoolExecutor(8) as pool:
            parts = list(pool.map(lambda b: sr.canonical_l2(q, c[b[0]:b[1]]), blocks))
        _cache[key] = np.concatenate(parts, axis=1)
    return _cache[key]


def _index(cuda, metric, shape):
    key = ("index", metric, shape)
    if key not in _cache:
        from sessionsimilaritysearch_amd.index import FlatIndex
        idx = FlatIndex(D_, metric, cuda, dtype="f32", scan="f32")
        idx.add(_data(shape)[0])
        _cache[key] = idx
    return _cache[key]


@pytest.mark.gpu
@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("shape", list(SHAPES))
@pytest.mark.parametrize("metric", ["ip", "l2"])
def test_f32_step_order(cuda, metric, shape, k):
    from sessionsimilaritysearch_amd import _lib
    c, q, sel, planted = _data(shape)
    idx = _index(cuda, metric, shape)
    _lib.lib().sss_scan_boot_expired(1)
    D, I = idx.search(q, k)
    assert idx.last_scan == "f32"
    assert _lib.lib().sss_scan_boot_expired(1) == 0
    if metric == "ip":
        Dr, Ir = sr.search_exact(q[sel], c, k)
    else:
        key = ("l2top", shape)                       # one sort serves every k: the best k are the first k of the best 20
        if key not in _cache:
            _cache[key] = sr.topk_from_scores(_l2_dist(q[sel], c), max(KS), largest=False)
        Dr, Ir = (a[:, :k] for a in _cache[key])
    # the planted rows are what the test says they are: the best min(k, planted) of a chosen query, in id order
    for qi, rows in planted.items():
        want = sorted(rows)[:k]
        assert Ir[np.searchsorted(sel, qi), :len(want)].tolist() == want, (qi, want)
    bad = np.argwhere(I[sel] != Ir)
    assert bad.size == 0, (len(bad), [(int(sel[a]), int(b), int(I[sel[a], b]), int(Ir[a, b])) for a, b in bad[:8]])
    assert np.array_equal(D[sel], Dr), int((D[sel] != Dr).sum())
