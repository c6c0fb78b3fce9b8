"""tests/helpers/kept_rows.py is what it claims, for every corpus tests/test_kept_rows_gpu.py uses -- without a device.

1. Construction: against the oracle's canonical scores (and squared distances for the L2 configurations) every query j
   has exactly P_j rows above its radius r_j, exactly T_j rows AT it, no other row within 0.2 below it (0.4 above, in
   distances: d = 2 - 2 s on unit vectors), and every row outside its group scores ~0.  With the scans' error bounds at
   unit norm at least two orders of magnitude below 0.2, "the scan keeps M_j = P_j + T_j rows" is then a fact about the
   inputs.
2. Constants: the copies of THR_CAP, SA_ROWS_SMALL, SA_ROWS_FULL and two_launch_lds' 2048 the tests build their groups
   from equal the sources', and the groups are the ones meant: a capacity change cannot silently move the tests off the
   edges."""
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import kept_rows as kr  # noqa: E402

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "sessionsimilaritysearch_amd", "csrc")

# every (d, dtype, groups, metrics) of the GPU file: a corpus is shared by the configurations of one (d, dtype)
CORPORA = {}
for _name, _d, _dtype, _metric, _scan, _pad, _rung in kr.RANGE_CONFIGS:
    CORPORA.setdefault((_d, _dtype, "range"), set()).add(_metric)
for _name, _d, _dtype, _metric, _scan, _pad, _rung in kr.RUNG_CONFIGS:
    for _k in (10, 100):
        CORPORA.setdefault((_d, _dtype, ("rung", _k)), set()).add(_metric)
CORPORA[(128, "f32", "neighbours")] = {"ip"}


def _id(key):
    d, dtype, which = key
    return f"{dtype}-{d}-{which if isinstance(which, str) else 'rung%d' % which[1]}"


@pytest.mark.parametrize("key", sorted(CORPORA, key=_id), ids=_id)
def test_construction(key):
    d, dtype, which = key
    c = kr.corpus(d, dtype, which)
    nq, n = c.nq, c.c.shape[0]
    assert nq <= 20 and n <= 70_000 and c.q.shape == (nq, d) and c.M.sum() + 3000 == n
    assert np.array_equal(kr.round_to(c.c, dtype), c.c) and np.array_equal(kr.round_to(c.q, dtype), c.q)
    own = c.owner[None, :] == np.arange(nq)[:, None]
    for j in range(nq):                                             # the helper's bookkeeping is the groups asked for
        assert (own[j] & ~c.at_radius).sum() == c.P[j] and (own[j] & c.at_radius).sum() == c.T[j]
        if c.T[j]:
            copies = c.c[own[j] & c.at_radius]
            assert (copies == copies[0]).all()
    stray_ip, stray_l2 = kr.stray_bounds(dtype)
    s = c.scores("ip")
    r = c.r[:, None]
    assert np.array_equal((s > r).sum(1), c.P) and np.array_equal(s > r, own & ~c.at_radius[None, :])
    assert np.array_equal((s == r).sum(1), c.T) and np.array_equal(s == r, own & c.at_radius[None, :])
    assert not ((s < r) & (s >= r - kr.GAP)).any()
    assert np.abs(s[~own]).max() < stray_ip, (np.abs(s[~own]).max(), stray_ip)
    assert (np.abs(c.r - 0.5) < 2 * stray_ip + 2.0 ** -24).all() and (c.r[c.T == 0] == np.float32(0.5)).all()
    print(f"{_id(key)}: n={n} nq={nq}: stray |score| max {np.abs(s[~own]).max():.3g} (bound {stray_ip:.3g})")
    if "l2" in CORPORA[key]:
        dist = c.scores("l2")
        r = c.r_l2[:, None]
        assert np.array_equal(dist < r, own & ~c.at_radius[None, :])
        assert np.array_equal(dist == r, own & c.at_radius[None, :])
        assert not ((dist > r) & (dist <= r + 2 * kr.GAP)).any()
        assert np.abs(dist[~own] - 2.0).max() < stray_l2, (np.abs(dist[~own] - 2.0).max(), stray_l2)
        assert (c.r_l2[c.T == 0] == np.float32(1.0)).all()
    # the rung's input: r_j is a valid bound of the k-th result, and where the k-th place lies inside the copies the
    # oracle's answer is the lowest ids of them
    ks = {"range": (), "neighbours": (10, 100)}[which] if isinstance(which, str) else (which[1],)
    for k in ks:
        assert (c.M >= k).all()
        for metric in sorted(CORPORA[key]):
            D, I = c.topk(k, metric)
            bound = c.r if metric == "ip" else c.r_l2
            assert (D[:, k - 1] >= bound).all() if metric == "ip" else (D[:, k - 1] <= bound).all()
            assert own[np.arange(nq)[:, None], I].all()             # every result is a row of the query's own group
            for j in np.flatnonzero(c.P < k):
                assert np.array_equal(I[j, c.P[j]:], np.flatnonzero(own[j] & c.at_radius)[:k - c.P[j]])
                assert (D[j, c.P[j]:] == bound[j]).all()


def _source(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def test_constants_equal_the_sources():
    thr, ip = _source("select_thr.hip"), _source("ip_topk.hip")
    assert int(re.search(r"constexpr int THR_CAP = (\d+);", ip).group(1)) == kr.THR_CAP
    assert int(re.search(r"constexpr int SA_ROWS_SMALL = (\d+);", thr).group(1)) == kr.SA_ROWS_SMALL
    assert int(re.search(r"constexpr int SA_ROWS_FULL = (\d+);", thr).group(1)) == kr.SA_ROWS_FULL
    body = re.search(r"static int two_launch_lds\(.*?\n}", thr, re.S).group(0)
    m = re.search(r"s\.small = s\.cap_pow2 < (\d+) \? s\.cap_pow2 : (\d+);", body)
    assert int(m.group(1)) == int(m.group(2)) == kr.TWO_LAUNCH_SMALL
    # the switches inside the kernels that the groups are built around, as the sources spell them
    assert "if ((int)M > 2 * k + 64) {" in thr and "if (keep > 2 * Ks) {" in thr
    assert re.search(r"int Ks = 64;\s*while \(Ks < k\) Ks <<= 1;", thr)
    assert "a.k > 64" in thr                                          # the first k_select_all launch: 256-row groups above k = 64
    assert f"s.rb < {kr.STAGED_ROW_BYTES} ? 0" in thr                 # rows from 1024 bytes on are staged
    assert kr.sort_width(10) == 64 and kr.sort_width(64) == 64 and kr.sort_width(65) == 128 and kr.sort_width(100) == 128


def test_groups_are_the_edges_meant():
    assert kr.range_groups() == ((0, 0), (1, 0), (0, 1), (0, 3000), (127, 0), (128, 0), (129, 0), (2047, 0), (2048, 0),
                                 (2049, 0), (2000, 48), (2000, 49), (8191, 0), (8192, 0), (8193, 0), (8000, 192), (8000, 193),
                                 (100, 9000))
    assert kr.rung_groups(10) == ((10, 0), (7, 3), (7, 40), (84, 0), (85, 0), (7, 121), (7, 122), (2047, 0), (2048, 0),
                                  (2049, 0), (7, 2041), (7, 2042), (8192, 0), (8193, 0), (7, 8185), (7, 8186))
    assert kr.rung_groups(100) == ((100, 0), (97, 3), (97, 40), (264, 0), (265, 0), (97, 159), (97, 160), (2047, 0),
                                   (2048, 0), (2049, 0), (97, 1951), (97, 1952), (8192, 0), (8193, 0), (97, 8095), (97, 8096))
    for groups in (kr.range_groups(), kr.rung_groups(10), kr.rung_groups(100), kr.NEIGHBOUR_GROUPS):
        assert len(groups) <= 20
    m = [p + t for p, t in kr.range_groups()]
    assert sum(x > kr.THR_CAP for x in m) == 3 and sum(x == kr.THR_CAP for x in m) == 2
    # the stored row sizes the configurations are listed for: both sides of the staging switch, per element size
    sizes = {name: d * kr.ELEM_BYTES[dtype] for name, d, dtype, *_ in kr.RUNG_CONFIGS}
    assert sizes == {"f32-128-f16": 512, "f32-128-split": 512, "f32-128-f32": 512, "f32-64": 256, "f32-256-f32": 1024,
                     "f32-512": 2048, "bf16-128": 256, "bf16-512": 1024, "f16-128": 256, "l2-128": 512, "l2-256": 1024,
                     "pad-200-f16": 800}
