"""The inputs of tests/test_l2_scan_bound_gpu.py are what they claim to be -- numpy, the oracle and ``sss_f16_shift`` only, no
device.  Each of them exists to make one term of the short-row L2 scans' error bound (``select_dev.h: err_bound_l2``, DESIGN
3), one of its ``+inf`` exits or the routing guard decide; an input that missed its regime would leave the GPU test green
and the term untested.  Where the GPU file asserts "no fallbacks" or caps them, the proof that the input deserves it is
here: the exact-distance gap between rank k and the first row beyond the select's second chance exceeds four times the
documented ``B_l2`` (``l2_scan_ref.proof_margin`` > 1) for every such query."""
import os
import sys

import numpy as np
import pytest

from sessionsimilaritysearch_amd import _lib

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import l2_scan_ref as r  # noqa: E402

KERNEL_IDS = [f"{s}{d}" for s, d in r.KERNELS]
SCANS = [s for s, _ in r.KERNELS_128]


def _lib_shift(amax):
    return int(_lib.lib().sss_f16_shift(float(amax)))


def _bias(c):
    """float32 -|c|^2 / 2 from a float64 sum: what ``sss_l2_row_bias`` stores."""
    return (-0.5 * (c.astype(np.float64) ** 2).sum(1)).astype(np.float32)


def test_image_restatements():
    """The helper's f16 shift is the library's; its bf16 split is two roundings to 8 significant bits."""
    for amax in (0.0, 2.0 ** -140, 2.0 ** -101, 2.0 ** -75, 0.3 * 2.0 ** -55, 0.999, 1.0, 3.0, 2.0 ** 55, 3.0e38, float("inf")):
        assert r.f16_shift(amax) == _lib_shift(amax), amax
    x = np.random.default_rng(1).standard_normal(4096).astype(np.float32)
    hi, lo = r.split_image(x)
    assert (hi.view(np.uint32) & 0xFFFF == 0).all() and (lo.view(np.uint32) & 0xFFFF == 0).all()
    assert (np.abs(x - hi) <= 2.0 ** -8 * np.abs(x)).all()
    assert (np.abs(x.astype(np.float64) - hi - lo) <= 2.0 ** -16 * np.abs(x)).all()


# ------------------------------------------------------------------------------------------------ 1. both sides scaled
def test_scaling_both_sides_scales_the_oracle_exactly():
    """One oracle call per corpus serves every scale: ids unchanged, D = ldexp(D0, 2 s), at both ends of the scale set."""
    c, q = r.gauss(128)
    D0, I0 = r.answer(("gauss", 128), q, c)
    for s in (r.GAUSS_SCALES[0], r.GAUSS_SCALES[-1]):
        D, I = r.oracle(r.ldexp32(q[:8], s), r.ldexp32(c, s), r.K)
        assert np.array_equal(I, I0[:8]) and np.array_equal(D, r.ldexp32(D0[:8], 2 * s))
        assert (D >= r.F32_MIN_NORMAL).all() and np.isfinite(D).all()


@pytest.mark.parametrize("scan,d", r.KERNELS, ids=KERNEL_IDS)
def test_gauss_stays_inside_the_guard_and_deserves_no_fallback(scan, d):
    """Every scale keeps the largest norm inside the guard.  The documented bound proves every query (margin > 1) at every
    scale but the two of GAUSS_NO_PROOF, whose reasons are derived here: the bound's floors (split) and sigma (f16)."""
    c, q = r.gauss(d)
    assert c.shape[0] > r.RUNG_CAPACITY
    gaps = r.rank_gaps(q, c)
    for s in r.GAUSS_SCALES:
        qs, cs = r.ldexp32(q, s), r.ldexp32(c, s)
        assert r.in_guard(cs), s
        B = r.b_l2(scan, qs, cs)
        margin = np.ldexp(gaps, 2 * s) / (4.0 * B)
        print(f"gauss {scan} d={d} s={s}: margin min {margin.min():.3g}, B / scaled B(0) {np.median(B / np.ldexp(r.b_l2(scan, q, c), 2 * s)):.4g}")
        why = r.GAUSS_NO_PROOF.get((scan, s))
        if why is None:
            assert margin.min() > 1, (s, margin.min())
        elif why == "inf":
            shift = _lib_shift(np.abs(cs).max()) + np.array([_lib_shift(a) for a in np.abs(qs).max(1)])
            assert (shift > 120).all() and np.isinf(B).all()                     # sigma beyond 2^120 for EVERY query
        else:
            assert np.isfinite(B).all() and margin.max() < 1                      # the floors: finite, and no query has the room


@pytest.mark.parametrize("scan,d", r.KERNELS, ids=KERNEL_IDS)
def test_near_copies_straddle_rank_k_inside_the_window(scan, d):
    c, q, base = r.near(d, scan == "f16")
    D, I = r.answer(("near", d, scan == "f16"), q, c, 41)
    B = r.b_l2(scan, q, c)
    spread = (D[:, 39] - D[:, 0]).astype(np.float64)
    print(f"near {scan} d={d}: spread of the 40 copies / B_l2: max {(spread / B).max():.3g}")
    assert (base[I[:, :40]] == base[I[:, :1]]).all() and (base[I[:, 40]] != base[I[:, 0]]).all()     # the 40 nearest: ONE base row's copies
    assert (spread > 0).all() and (spread < B).all()                              # ... all inside the window, rank 10 among them
    for s in r.NEAR_SCALES:
        assert r.in_guard(r.ldexp32(c, s)), s


# ------------------------------------------------------------------------------------------------ 2. one side scaled
@pytest.mark.parametrize("side,s", r.ONE_SIDE, ids=[f"{a}{s}" for a, s in r.ONE_SIDE])
def test_one_side_scaled_degenerates_to_mass_ties(side, s):
    """Unit rows against unit queries 2^40 and more apart: every distance is |larger side|^2 to within 2^-38, so a query's n
    float32 distances take a handful of values and its answer is exact ties in id order."""
    c, q = r.one_side(side, s)
    dist = r.sr.canonical_l2(q[:4], c)
    values = [np.unique(row).size for row in dist]
    D, I = r.answer(("one_side", side, s), q, c)
    ties = (np.diff(D, axis=1) == 0).sum(1)
    print(f"one side {side} x 2^{s}: distinct float32 distances per query {values}, exact ties among a query's 10 results: "
          f"{ties.min()} .. {ties.max()} of 9")
    assert max(values) <= 8 and np.isfinite(D).all() and (D >= r.F32_MIN_NORMAL).all()
    assert ties.min() >= 6
    big = max(r.norms(c).max(), r.norms(q).max()) ** 2
    assert np.abs(dist.astype(np.float64) / big - 1).max() < 2.0 ** -20            # (unit rows: |x|^2 = 1 to a few float32 ulps)
    assert r.in_guard(c) == (side == "q" or s in (-40, 40, 59))                    # what the route must follow


# ------------------------------------------------------------------------------------------------ 3. +inf exits, guard
@pytest.mark.parametrize("d", [128, 512])
def test_sigma_beyond_2_120_for_every_query(d):
    c, q = r.unit(d)
    ce, qe = r.INF_EXITS["sigma"]
    cs, qs = r.ldexp32(c, ce), r.ldexp32(q, qe)
    shift = _lib_shift(np.abs(cs).max()) + np.array([_lib_shift(a) for a in np.abs(qs).max(1)])
    assert (shift > 120).all() and r.in_guard(cs)
    half = 0.5 * r.norms(cs).max() ** 2
    assert (half * np.ldexp(1.0, shift) < 1e36).all()                             # this exit alone
    assert np.isinf(r.b_l2("f16", qs, cs)).all()
    D, _ = r.answer(("inf", "sigma", d), qs, cs)
    assert (D >= r.F32_MIN_NORMAL).all()


@pytest.mark.parametrize("d", [128, 512])
def test_scaled_bias_beyond_1e36_for_every_query(d):
    c, q = r.unit(d)
    ce, qe = r.INF_EXITS["bias"]
    cs, qs = r.ldexp32(c, ce), r.ldexp32(q, qe)
    shift = _lib_shift(np.abs(cs).max()) + np.array([_lib_shift(a) for a in np.abs(qs).max(1)])
    assert (np.abs(shift) < 120).all() and r.in_guard(cs)                         # sigma itself is in range
    half = 0.5 * r.norms(cs).min() ** 2
    assert (half * np.ldexp(1.0, shift) >= 1e36).all()
    assert np.isinf(r.b_l2("f16", qs, cs)).all()


@pytest.mark.parametrize("d", [64, 128, 256, 512])
def test_query_norm_whose_square_overflows_float32(d):
    """Queries x 2^70: every canonical distance is +inf, the oracle answers ids 0 .. k-1.  The documented bound stays
    finite (|q|^2 is summed in float64), so the GPU case claims nothing about WHICH stage resolves the query."""
    c, q = r.unit(d)
    qs = r.ldexp32(q, 70)
    assert ((qs.astype(np.float64) ** 2).sum(1) > 3.5e38).all() and np.isfinite(qs).all()
    with np.errstate(over="ignore"):
        D, I = r.answer(("inf", "qnorm", d), qs, c)
    assert np.isposinf(D).all() and np.array_equal(I, np.tile(np.arange(r.K), (q.shape[0], 1)))
    for scan in SCANS:
        assert np.isfinite(r.b_l2(scan, qs, c)).all()


@pytest.mark.parametrize("d", [64, 128, 256, 512])
def test_guard_edges_are_one_octave_clear_of_the_guard(d):
    c, _ = r.unit(d)
    for s in r.GUARD_EDGES:
        cmax = r.norms(r.ldexp32(c, s)).max()
        assert abs(cmax / 2.0 ** s - 1) < 1e-6
        assert r.in_guard(r.ldexp32(c, s)) == (abs(s) < 60)
    # the index that crosses the edge by `add`: inside with its first rows, outside with all of them
    assert r.in_guard(r.ldexp32(c[:4000], 59)) and not r.in_guard(np.concatenate([r.ldexp32(c[:4000], 59), r.ldexp32(c[4000:], 61)]))


# ------------------------------------------------------------------------------------------------ 4. small rows, large cmax
def test_small_rows_under_a_large_cmax():
    c, q, info = r.small_rows()
    giants, tiny, zero = info["giants"], info["tiny"], info["zero"]
    shift = _lib_shift(np.abs(c).max())
    assert np.abs(c).max() == np.float32(3.0) and shift == 11 and r.in_guard(c)
    cmax = r.norms(c).max()
    assert int(np.argmax(r.norms(c))) in set(giants.tolist()) and 6 < cmax < 12
    b = _bias(c)
    assert (np.abs(b[tiny]) < r.F32_MIN_NORMAL).all() and (b[tiny] != 0).all()     # subnormal float32 bias
    assert not c[zero].any() and (b[zero] == 0).all() and zero.size == r.ZERO_ROWS
    D, I = r.answer("small_rows", q, c, 100)
    assert not q[0].any() and I[0, :10].tolist() == zero.tolist() and (D[0, :10] == 0).all() and D[0, 10] > 0
    small = set(tiny.tolist()) | set(zero.tolist())
    ties = 0
    for i in range(1, 1 + r.PER_KIND):                                             # queries at the tiny rows' scale
        assert np.abs(q[i]).max() < 2.0 ** -60 and set(I[i].tolist()) <= small
        assert 0 < D[i, 9] < r.F32_MIN_NORMAL                                      # subnormal float32 distances ...
        ties += int((np.diff(D[i]) == 0).sum())
    print(f"small rows: exact ties among the first 100 distances of the {r.PER_KIND} tiny queries: {ties}")
    assert ties >= 4 * r.PER_KIND                                                  # ... with exact ties: ids ascending decide
    by_bias = np.lexsort((np.arange(c.shape[0]), -b.astype(np.float64)))[:10]
    for j, exp in enumerate(r.DWARF_EXPONENTS):
        rows, own = info["clusters"][exp]
        ratio = r.f16_residual_norms(c[rows], shift) / (2.0 ** -11 * r.norms(c[rows]))
        print(f"small rows: dwarfs 2^{exp}: f16 residual / (2^-11 |c|): min {ratio.min():.1f}, median {np.median(ratio):.1f}, max {ratio.max():.1f}")
        if exp == -39:                                                             # flushed: the image is zero, the residual the row
            assert not np.ldexp(c[rows], shift).astype(np.float16).any() and ratio.min() >= 2047
        else:                                                                      # f16 subnormals: beyond what the normal range allows
            assert ratio.min() > 1 and ratio.max() < 16
        for i in range(r.PER_KIND):
            qi = 1 + r.PER_KIND * (1 + j) + i
            assert set(I[qi, :10].tolist()) <= set(own[i].tolist()), qi            # the neighbours are the query's own cluster
            assert set(I[qi, :10].tolist()) != set(by_bias.tolist())               # the bias alone (all a flushed row shows) misorders
            nearest_by_norm = own[i][np.argsort(r.norms(c[own[i]]))[:10]]
            assert set(nearest_by_norm.tolist()) != set(I[qi, :10].tolist()), qi
    g = r.f16_residual_norms(c[giants], shift)
    assert (g <= 2.0 ** -11 * r.norms(c[giants])).all()                            # the giants are ordinary f16 rows


# ------------------------------------------------------------------------------------------------ 5. aligned rounding
def _aligned_case(name):
    """(c, q, info, img): the input and its scan image in the rows' own units (float64), restated on the host."""
    if name == "f16":
        c, q, info = r.worst_f16()
        return c, q, info, r.f16_image(c, _lib_shift(np.abs(c).max()))
    c, q, info = r.worst_split()
    hi, lo = r.split_image(c)
    return c, q, info, hi.astype(np.float64) + lo.astype(np.float64)


@pytest.mark.parametrize("name,lead,share_min", [("f16", 2.0 ** -11, 0.75), ("split", 2.0 ** -16, 0.38)])
def test_aligned_rounding_hides_the_neighbours_behind_the_decoys(name, lead, share_min):
    """Scored on the restated image in float64, all 200 decoys precede all 30 true neighbours.  The aligned residual
    q.(c - image) reaches 0.79 .. 0.80 of the documented leading term 2^-11 |q||c| for f16 and 0.40 of 2^-16 |q||c| for
    split (measured here, asserted from 0.75 and 0.38).  For f16 the score error takes more than 0.85 of the whole B_l2 of
    the query: a bound that lost its factor 2, or its c_resid |q| term, would not cover it."""
    c, q, info, img = _aligned_case(name)
    decoys, aligned = info["decoys"], info["aligned"]
    assert decoys.size >= 200 and aligned.size == 30 and c.shape[0] > r.RUNG_CAPACITY
    q0, c64 = q[0].astype(np.float64), c.astype(np.float64)
    if name == "f16":                                                              # the query's own image is exact
        sh = _lib_shift(np.abs(q[0]).max())
        assert np.array_equal(r.f16_image(q[:1], sh)[0], q0)
    else:
        qh, ql = r.split_image(q[:1])
        assert np.array_equal(qh[0].astype(np.float64), q0) and not ql.any()
    assert np.array_equal(img[decoys], c64[decoys])                                # decoys: exact in the image
    residual = (c64[aligned] - img[aligned]) @ q0                                  # what the scan's q.c misses
    assert ((c64[aligned] - img[aligned]) > 0).all() and (q0 > 0).all()            # every element rounds against the query
    share = residual / (lead * np.linalg.norm(q0) * np.linalg.norm(c64[aligned], axis=1))
    scan_dist = (c64 ** 2).sum(1) - 2.0 * (img @ q0) + q0 @ q0                     # the scan's view of every row
    B = r.b_l2(name, q[:1], c)[0]
    print(f"aligned {name}: share of the leading term {share.min():.3f} .. {share.max():.3f}; score error / B_l2 "
          f"{2 * residual.min() / B:.3f} .. {2 * residual.max() / B:.3f}")
    assert share.min() >= share_min and share.max() <= 1
    assert scan_dist[decoys].max() < scan_dist[aligned].min()                      # the scan's order: decoys first ...
    first = np.argsort(scan_dist, kind="stable")[:decoys.size]
    assert set(first.tolist()) == set(decoys.tolist())                             # ... ahead of everything else too
    d_al, d_de = r.exact_l2(q[0], c[aligned]), r.exact_l2(q[0], c[decoys])
    assert d_al.max() < d_de.min() and np.unique(d_de).size == 1                   # the truth: neighbours first, decoys tie
    assert 2 * residual.max() < B                                                  # the documented bound covers the error ...
    if name == "f16":
        assert 2 * residual.min() > 0.85 * B                                       # ... with nothing to spare
        res = r.f16_residual_norms(c, _lib_shift(np.abs(c).max()))
        assert int(np.argmax(res)) in set(aligned.tolist())                        # c_resid comes from the aligned rows
    D, I = r.answer(("aligned", name), q, c, 100)
    assert set(I[0, :30].tolist()) == set(aligned.tolist()) and set(I[0, 30:].tolist()) <= set(decoys.tolist())
    assert (D[0, 30:] == D[0, 30]).all()
    margin = r.proof_margin(name, q[1:], c)
    print(f"aligned {name}: background margin min {margin.min():.2f}")
    assert margin.min() > 1


@pytest.mark.parametrize("norm", r.ULP_NORMS)
def test_ulp_copies_straddle_rank_k_far_inside_the_window(norm):
    c, q, info = r.ulp_copies(norm)
    cluster = np.concatenate([[info["base"]], info["copies"]])
    assert np.unique(cluster).size == r.ULP_COPIES + 1 >= 41 and c.shape[0] > r.RUNG_CAPACITY
    t = info["coordinate"]
    steps = np.abs(c[info["copies"], t].view(np.int32).astype(np.int64) - int(c[info["base"], t:t + 1].view(np.int32)[0]))
    assert steps.tolist() == list(range(1, r.ULP_COPIES + 1))                      # one float32 ulp apart, in one coordinate
    assert (np.delete(c[info["copies"]], t, axis=1) == np.delete(c[info["base"]], t)[None, :]).all()
    assert abs(r.norms(c[cluster]).max() / norm - 1) < 1e-5 and r.in_guard(c)
    exact = r.exact_l2(q[0], c[cluster])
    assert (np.diff(exact) > 0).all()                                              # every step leads away from the query
    D, I = r.answer(("ulp", norm), q, c, 41)
    assert set(I[0].tolist()) == set(cluster.tolist()) and np.unique(D[0]).size > 20
    B = r.b_l2("f32", q[:1], c)[0]
    assert exact[-1] - exact[0] < B / 100
    margin = r.proof_margin("f32", q[1:], c)
    print(f"ulp copies at norm {norm}: span / B_l2 {(exact[-1] - exact[0]) / B:.2e}, background margin min {margin.min():.1f}")
    assert margin.min() > 1
