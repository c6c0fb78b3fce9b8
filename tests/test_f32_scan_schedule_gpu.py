"""The f32 list scan's own step order for 512-byte rows (csrc/scan_kernel.h, "F32S"): fragments carried over the step
boundary, the next tile's DMA one piece per k-group, the tile hand-over (wait + barrier) in front of the LAST k-group of a
tile's last step, half the max tree under the other accumulator's last MFMAs.  None of it may change a result.

Every case searches ``FlatIndex(d, metric, scan="f32")`` at k = 10 three times in the process -- the three results must be
equal -- and compares ids and scores with ``array_equal`` against the oracle on a query subset that covers every (wave,
lane) slot of one workgroup (queries 0 .. 255) plus the first query of every other query group.  The oracle is
``search_ref.search_exact`` for the inner product and, for L2, what the L2 tests of the suite use:
``topk_from_scores(canonical_l2(q, c), 10, largest=False)`` (``search_exact`` scores inner products only).

Shapes (``make_plan``, csrc/scan.hip: 128-row tiles of 512-byte rows from 48 tiles a split; S = (256 / query groups)
splits, at least 8; the bootstrap needs 16 active splits):

* nq 8192 (32 groups -> 8 splits), n = 49152 + 77: 128-row tiles, 49 a split, the last split shorter, the last tile
  ragged inside its second sub-step; no threshold / bootstrap (8 splits).  n = 49152: no ragged tile, 48 a split.
* nq 2048 (8 groups -> 32 splits), n = 32 * 48 * 128 + 77: 128-row tiles WITH the bootstrap tile (whose end keeps the old
  order: publish, wait, barrier, poll) and the threshold refreshes -- the headline's configuration at the smallest size
  that reaches it.
* nq 256 (1 group -> 256 splits), n = 256 * 64 * 3 + 5: 64-row tiles (one step per tile: every step ends with a
  hand-over), 3-4 a split, bootstrap; n = 16384: one-tile splits (the bootstrap tile and its live repeat, nothing else).

d = 64 and d = 256 keep the shared step order and have no case here."""
import numpy as np
import pytest

from oracle import search_ref as sr

K = 10
_cache = {}


def _unit(rng, n, d):
    v = rng.standard_normal((n, d)).astype(np.float32)
    return (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(np.float32)


def _data(nq, n, d=128):
    key = ("data", nq, n, d)
    if key not in _cache:
        rng = np.random.default_rng([20261019, nq, n, d])
        _cache[key] = (_unit(rng, n, d), _unit(rng, nq, d))
    return _cache[key]


def _subset(nq):
    """Every (wave, lane) slot of workgroup 0, and one query of every other query group (256 queries a group)."""
    return np.concatenate([np.arange(min(256, nq)), np.arange(256, nq, 256)])


def _oracle(metric, q, c):
    if metric == "ip":
        return sr.search_exact(q, c, K)
    # canonical_l2 is elementwise in (query, row): row blocks keep its temporaries in cache, the values are its own
    dist = np.concatenate([sr.canonical_l2(q, c[lo:lo + 4096]) for lo in range(0, c.shape[0], 4096)], axis=1)
    return sr.topk_from_scores(dist, K, largest=False)


def _search3(cuda, metric, c, q):
    from sessionsimilaritysearch_amd.index import FlatIndex
    idx = FlatIndex(c.shape[1], metric, cuda, scan="f32")
    idx.add(c)
    runs = [idx.search(q, K) for _ in range(3)]
    assert idx.last_scan == "f32"
    for D, I in runs[1:]:
        assert np.array_equal(I, runs[0][1]) and np.array_equal(D, runs[0][0]), "the same search gave two results"
    return runs[0]


def _check(cuda, metric, nq, n):
    c, q = _data(nq, n)
    D, I = _search3(cuda, metric, c, q)
    sel = _subset(nq)
    Dr, Ir = _oracle(metric, q[sel], c)
    assert np.array_equal(I[sel], Ir), int((I[sel] != Ir).sum())
    assert np.array_equal(D[sel], Dr), int((D[sel] != Dr).sum())


SHAPES = {
    "tiles128_ragged": (8192, 49152 + 77),
    "tiles128_full": (8192, 49152),
    "tiles128_bootstrap": (2048, 32 * 48 * 128 + 77),
    "tiles64": (256, 256 * 64 * 3 + 5),
    "tiles64_one_tile_splits": (256, 16384),
}


@pytest.mark.gpu
@pytest.mark.parametrize("shape", list(SHAPES))
def test_f32_schedule_inner_product(cuda, shape):
    _check(cuda, "ip", *SHAPES[shape])


@pytest.mark.gpu
@pytest.mark.parametrize("shape", ["tiles128_ragged", "tiles64"])
def test_f32_schedule_l2(cuda, shape):
    """MET = 1: the next tile's bias fetch sits next to the moved wait."""
    _check(cuda, "l2", *SHAPES[shape])


@pytest.mark.gpu
def test_f32_schedule_planted_rows(cuda):
    """Background: random unit rows scaled by 0.5 (scores below 0.5).  For 64 queries, ten planted rows q (1 - j 2^-10),
    j = 0 .. 9 (scores 1 - j 2^-10 up to rounding, all above 0.99), at tile-relative positions 0, 31, 32, 63, 64, 127 of the
    first tile of every split, of middle tiles, of the last full tile of every split and (positions below 77) of the
    ragged tail: the ten ids of a query are the planted ones, in the order of j.  A fragment read from a buffer handed over
    too early, or a tile whose DMA piece went astray, scores some other row in a planted row's place."""
    nq, n = SHAPES["tiles128_ragged"]
    c, q = _data(nq, n)
    c = (c * np.float32(0.5)).astype(np.float32)
    tiles_per_split, total = 49, (n + 127) // 128          # 8 splits of 49 tiles (the last one 42: tiles 343 .. 384)
    pos = (0, 31, 32, 63, 64, 127)
    first = [s * tiles_per_split for s in range(8)]
    last_full = [min((s + 1) * tiles_per_split, total - 1) - 1 for s in range(8)]
    slots = [(t, p) for t in first + last_full for p in pos] + [(total - 1, p) for p in pos if (total - 1) * 128 + p < n]
    middle = [s * tiles_per_split + m for m in (1, 2, 3, 12, 13, 23, 24, 25, 30, 36, 38, 39) for s in range(8)]
    slots += [(t, p) for t in middle for p in pos]
    chosen = np.arange(64) * 4                               # eight queries of every wave of workgroup 0
    assert len(slots) >= 10 * len(chosen) and len(set(slots)) == len(slots)
    # the 96 + 5 slots of first / last full / ragged tiles first, then middle tiles, dealt round robin over the queries
    want = np.empty((len(chosen), K), np.int64)
    for s_i, slot in enumerate(slots[:10 * len(chosen)]):
        qi, j = s_i % len(chosen), s_i // len(chosen)
        row = slot[0] * 128 + slot[1]
        c[row] = (q[chosen[qi]] * np.float32(1 - j * 2.0 ** -10)).astype(np.float32)
        want[qi, j] = row
    D, I = _search3(cuda, "ip", c, q)
    assert np.array_equal(I[chosen], want), np.argwhere(I[chosen] != want)[:8].tolist()
    Dr, Ir = sr.search_exact(q[chosen], c, K)
    assert np.array_equal(Ir, want)
    assert np.array_equal(D[chosen], Dr)
