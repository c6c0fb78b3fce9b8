"""The inputs of tests/test_l2_long_bound_gpu.py are what they claim to be -- numpy and the oracle only, no device.  Each of
them exists to make ONE term of the long-row L2 scan's per-row error bound decide
(sessionsimilaritysearch_amd/csrc/select_thr.hip: THE PER-ROW BOUND); an input that missed its regime would leave the
GPU test green and the term untested."""
import os
import sys

import numpy as np
import pytest

from sessionsimilaritysearch_amd import _lib

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import l2_long_ref as lr  # noqa: E402

F32_MIN_NORMAL = 2.0 ** -126


def _bias(c):
    """float32 -|c|^2 / 2 from a float64 sum: what ``sss_l2_row_bias`` stores."""
    return (-0.5 * (c.astype(np.float64) ** 2).sum(1)).astype(np.float32)


def test_f16_shift_restatement_is_the_library_s():
    L = _lib.lib()
    for amax in (0.0, 2.0 ** -140, 2.0 ** -70, 0.999, 1.0, 2.9, 3.0, 4.0, 100.7, 2.0 ** 60, 3.0e38, float("inf"), float("nan")):
        assert lr.f16_shift(amax) == L.sss_f16_shift(amax), amax


@pytest.mark.parametrize("exp", lr.DWARF_EXPONENTS)
def test_dwarfs_lose_their_image_and_the_bias_alone_misorders_them(exp):
    c, q, info = lr.dwarfs_under_giants(exp)
    shift = _lib.lib().sss_f16_shift(float(np.abs(c).max()))
    assert shift == info["shift"] == 11 and np.abs(c).max() == np.float32(3.0)
    dwarf = np.setdiff1d(np.arange(c.shape[0]), info["giants"])
    assert dwarf.size == c.shape[0] - lr.GIANTS
    norms = np.linalg.norm(c[dwarf].astype(np.float64), axis=1)
    ratio = lr.f16_residual_norms(c[dwarf], shift) / (2.0 ** -11 * norms)
    print(f"dwarfs 2^{exp}: f16 residual / (2^-11 |c|): min {ratio.min():.1f}, median {np.median(ratio):.1f}")
    if exp == -39:                                  # flushed: the image of every dwarf is zero, the residual the row itself
        assert not np.ldexp(c[dwarf], shift).astype(np.float16).any() and ratio.min() >= 2047
    elif exp == -31:                                # 0 to 4 bits of an element survive
        assert ratio.min() >= 16
    else:
        # -27: scaled by 2^11 the element r.m.s. is 2^-18 to 2^-16 against the subnormal spacing 2^-24: 6 to 8 bits survive.
        # The rounding error is uniform in +-2^-25 (r.m.s. 2^-25 / sqrt 3), so residual / (2^-11 |c|) is 2^-14.8 / r.m.s. =
        # 2.3 to 9: beyond what the normal range allows, but 16-fold cannot be reached at this scale (2^-31 carries that)
        assert ratio.min() > 1 and ratio.max() < 16
    # the giants are ordinary f16 rows
    g = info["giants"]
    assert (lr.f16_residual_norms(c[g], shift) <= 2.0 ** -11 * np.linalg.norm(c[g].astype(np.float64), axis=1)).all()
    # bias alone (all the scan sees of a flushed row) against the truth, per query
    Dr, Ir = lr._oracle(q, c, 10)
    by_bias = np.lexsort((np.arange(c.shape[0]), -_bias(c).astype(np.float64)))[:10]
    for i in range(q.shape[0]):
        assert set(Ir[i].tolist()) <= set(info["clusters"][i].tolist()), i          # the neighbours are the query's own cluster
        assert Ir[i].tolist() != by_bias.tolist() and set(Ir[i].tolist()) != set(by_bias.tolist()), i
        # ... and inside the cluster the smallest norms are not the nearest rows either
        own = info["clusters"][i]
        smallest = own[np.argsort(np.linalg.norm(c[own].astype(np.float64), axis=1))[:10]]
        assert set(smallest.tolist()) != set(Ir[i].tolist()), i


def test_subnormal_bias_rows_are_subnormal_and_the_zero_query_finds_the_zero_rows():
    c, q, info = lr.subnormal_bias()
    b = _bias(c)
    tiny, zbias, zero = info["tiny"], info["zero_bias"], info["zero"]
    assert tiny.size == lr.TINY_ROWS and zero.size == lr.ZERO_ROWS and zbias.size == lr.ZERO_BIAS_ROWS
    assert (np.abs(b[tiny]) < F32_MIN_NORMAL).all() and (b[tiny] != 0).all()
    assert (b[zbias] == 0).all() and (b[zero] == 0).all() and not c[zero].any() and c[zbias].any(axis=1).all()
    assert ((c[zbias].astype(np.float64) ** 2).sum(1).astype(np.float32) == np.float32(2.0 ** -149)).all()
    rest = np.setdiff1d(np.arange(c.shape[0]), np.concatenate([tiny, zbias, zero]))
    assert (np.abs(b[rest]) > 2.0 ** -7).all()                                        # the background: norms from 1/4
    cmax = np.linalg.norm(c.astype(np.float64), axis=1).max()
    assert 2.0 ** -60 <= cmax <= 2.0 ** 60                                            # the route guard
    assert not q[0].any() and q[1:].any(axis=1).all() and np.abs(q).max() < 2.0 ** -60
    Dr, Ir = lr._oracle(q, c, 10)
    assert Ir[0].tolist() == zero.tolist() and (Dr[0] == 0).all()
    assert (Dr[1:] < F32_MIN_NORMAL).all() and (Dr[1:, -1] > 0).all()                 # float32 subnormal distances (or 0) ...
    D100, _ = lr._oracle(q[1:], c, 100)
    ties = sum(int((np.diff(row) == 0).sum()) for row in D100)
    print(f"subnormal bias: exact ties among the first 100 distances of {q.shape[0] - 1} queries: {ties}")
    assert ties >= q.shape[0] - 1                                                     # ... with exact ties: ids ascending decide


@pytest.mark.parametrize("norm", [0.25, 4.0])
@pytest.mark.parametrize("m", [40, 600])
def test_near_tie_clusters_are_strictly_inside_the_window(m, norm):
    c, q, info = lr.near_ties(m, norm)
    cluster = np.concatenate([[info["base"]], info["copies"]])
    assert info["copies"].size == m and np.unique(cluster).size == m + 1
    exact = lr.exact_l2(q[0], c[cluster])
    limit = 2.0 ** -13 * np.linalg.norm(q[0].astype(np.float64)) * np.linalg.norm(c[cluster].astype(np.float64), axis=1).min()
    assert 0 < exact.max() - exact.min() < limit
    assert exact.max() - exact.min() > limit / 4                                      # (and not vanishingly small)
    assert abs(np.linalg.norm(c[info["base"]].astype(np.float64)) / norm - 1) < 1e-6
    D, I = lr._oracle(q[:1], c, m + 1)
    assert set(I[0].tolist()) == set(cluster.tolist())                                # the cluster IS the neighbourhood
    assert np.unique(D[0]).size > min(m, 100) // 2                                    # many distinct float32 distances
    tiles = np.unique(info["copies"] // 256)
    assert tiles.size > min(m, 78) // 2                                               # scattered over the tiles


def test_worst_rounding_rows_round_down_to_the_query_and_are_the_neighbours():
    c, q, info = lr.worst_rounding()
    shift = _lib.lib().sss_f16_shift(float(np.abs(c).max()))
    img = np.ldexp(c, shift).astype(np.float16).astype(np.float64)
    q0 = q[0].astype(np.float64)
    assert np.array_equal(np.ldexp(q[0], lr.f16_shift(np.abs(q[0]).max())).astype(np.float16).astype(np.float64),
                          np.ldexp(q0, lr.f16_shift(np.abs(q[0]).max())))            # the query's own image is exact
    assert np.array_equal(img[info["exact"]], np.ldexp(c[info["exact"]].astype(np.float64), shift))       # exact rows: exact
    assert (img[info["rounded"]] == np.ldexp(q0, shift)[None, :]).all()                # rounded rows: the query itself
    qq = float(q0 @ q0)
    scan_err = 2.0 * ((c[info["rounded"]].astype(np.float64) - q0[None, :]) @ q0)      # what the scan's score misses
    d_exact, d_rounded = lr.exact_l2(q[0], c[info["exact"]]), lr.exact_l2(q[0], c[info["rounded"]])
    print(f"worst rounding: scan error / |q|^2 = 2^{np.log2(scan_err.min() / qq):.2f}, exact rows at 2^{np.log2(d_exact.min() / qq):.2f},"
          f" rounded rows at 2^{np.log2(d_rounded.max() / qq):.2f}")
    assert scan_err.min() > 0.5 * 2.0 ** -10 * qq                                      # more than half of 2 2^-11 |q||c| ...
    assert scan_err.max() < 2.04 * 2.0 ** -11 * qq                                     # ... and inside the bound's leading term
    assert d_rounded.max() < d_exact.min() and d_exact.max() < scan_err.min() / 4      # true order against the scan's order
    _, I = lr._oracle(q[:1], c, 10)
    assert set(I[0].tolist()) <= set(info["rounded"].tolist())


def test_wide_norms_span_twenty_octaves_and_the_aimed_queries_hit():
    c, q, info = lr.wide_norms()
    norms = np.linalg.norm(c.astype(np.float64), axis=1)
    assert norms.min() < 2.0 ** -9.9 and norms.max() > 2.0 ** 9.9
    _, I = lr._oracle(q, c, 1)
    aimed = np.concatenate([info["small"], info["large"]])
    assert I[:aimed.size, 0].tolist() == aimed.tolist()
    assert norms[info["small"]].max() < 2.0 ** -9 and norms[info["large"]].min() > 2.0 ** 9


def test_identical_nearest_groups_are_alone_in_reach_of_their_query():
    for m in (2047, 8193):
        c, q, info = lr.identical_nearest(m, 20_000, 320, 17, 300 + m)
        d = lr.exact_l2(q[0], c)
        others = np.setdiff1d(np.arange(c.shape[0]), info["group"])
        assert info["group"].size == m and d[info["group"]].max() < 1e-3 and d[others].min() > 9
        assert np.unique(c[info["group"]], axis=0).shape[0] == 1
