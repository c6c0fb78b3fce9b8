"""CPU side of scoring a search result (include/sss_eval.h, sessionsimilaritysearch_amd/evaluation.py): the header against
its ctypes binding, argument validation without a device, the numpy restatement (tests/helpers/eval_ref.py) against what
the reference's own metric functions returned (tests/golden/eval_metrics.npz), and ActionTable.split / concat.

Bounds against the reference's recorded values (absolute; every term and every mean lies in [0, 1]), u = 2^-53:
  GAMMA(n) = n u / (1 - n u)  a float64 mean of the same n rounded pair terms taken in two orders.  A sum of non-negative
                              terms in which no term passes through more than m additions has relative error <= gamma_m.
                              Here: K - 1 additions per query, nq' - 1 over the queries and two divisions, K + nq' <= n / 2
                              for n = nq' K; numpy's pairwise mean of the reference passes a term through fewer than
                              n / 2 additions as well.  Two values within gamma_(n/2) of the exact mean differ by at
                              most 2 gamma_(n/2) <= gamma_n.
  GAMMA(2 K)                  average precision: sklearn sums (recall step) * precision over the ranks, this contract
                              sums t / (j + 1) over the hits -- 2 K roundings cover either; the mean over the queries
                              is held to the same bound.
  AVE_TOL(n)                  get_ave_score is numpy's float32 pairwise mean of n float32 pair scores:
                              (ceil(log2 n) + 2) 2^-24 bounds its distance from their exact mean (one rounding per
                              level of the pairwise tree, the division and the result's own rounding); the float64 mean
                              here is exact to far below that.
  get_recall                  counts: integers, the two means are of the same nq integers -- GAMMA(nq)."""
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
from abi import declared  # noqa: E402
import eval_ref as ev  # noqa: E402
import sparse_ref as sp  # noqa: E402

from sessionsimilaritysearch_amd import _lib  # noqa: E402
from sessionsimilaritysearch_amd.sessions import ActionTable, synthetic_actions  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "eval_metrics.npz")
U = 2.0 ** -53


def GAMMA(n):
    return n * U / (1 - n * U)


def AVE_TOL(n):
    return (math.ceil(math.log2(n)) + 2) * 2.0 ** -24


def golden():
    g = np.load(GOLDEN)
    tab = {t: ActionTable(g[f"{t}_sess_ptr"], g[f"{t}_is_search"], g[f"{t}_item_id"], np.zeros_like(g[f"{t}_item_id"]))
           for t in ("corpus", "query", "seq", "tar")}
    return g, tab


def host_parts(tab):
    return {"cur": sp.vectors(tab["seq"], "binary")[:2], "future": sp.vectors(tab["tar"], "binary")[:2],
            "all": sp.vectors(ActionTable.concat(tab["seq"], tab["tar"]), "binary")[:2]}


def check_against_reference(g, parts, value):
    """`value(key, thres)` -> this project's figure; every one within its bound of the reference's recorded value.
    Returns the largest |difference| / bound seen (printed by the callers)."""
    nq, K = g["I"].shape
    worst = 0.0

    def close(key, got, want, tol):
        nonlocal worst
        d = abs(got - want)
        print(f"{key}: |ours - reference| = {d:.3e}, bound {tol:.3e}")
        worst = max(worst, d / tol)
        assert d <= tol, (key, got, want, d, tol)
    for p in ev.PARTS:
        n_kept = int((np.diff(parts[p][0]) > 0).sum()) * K
        close(f"{p}_jaccard", value(f"{p}_jaccard", None), float(g[f"ref_{p}_jaccard"]), GAMMA(nq * K if p == "all" else n_kept))
        close(f"{p}_recall", value(f"{p}_recall", None), float(g[f"ref_{p}_recall"]), GAMMA(n_kept))
        close(f"{p}_map", value(f"{p}_map", None), float(g[f"ref_{p}_map"]), GAMMA(2 * K))
    for sim in ev.SIM_PART:
        close(f"ave_{sim}", value(f"ave_{sim}", None), float(g[f"ref_ave_{sim}"]), AVE_TOL(nq * K))
        for t, want in zip(g["thres"], g[f"ref_recall_{sim}"]):
            close(f"recall_{sim} > {t}", value(f"recall_{sim}", float(t)), float(want), GAMMA(nq))
    return worst


def test_helper_reproduces_the_reference_values():
    g, tab = golden()
    parts, corpus = host_parts(tab), sp.vectors(tab["corpus"], "binary")[:2]
    nq, K = g["I"].shape
    assert (nq, K) == (48, 20) and len(corpus[0]) - 1 == 400 and g["I"].min() >= 0 and g["I"].max() < 400
    # what the generator asserted of the fixture, seen through the helper
    assert (np.diff(parts["all"][0]) > 0).all() and (np.diff(parts["cur"][0]) == 0).any() and (np.diff(parts["future"][0]) == 0).any()
    assert (np.diff(corpus[0])[g["I"]] == 0).any()
    inter, _, err = ev.overlap(parts["all"], corpus, g["I"])
    assert err == 0 and (inter > 0).all(axis=1).any() and (inter == 0).all(axis=1).any()
    cache = {}

    def value(key, thres):
        if thres not in cache:
            cache[thres] = ev.evaluate(g["I"], parts, corpus, thres)
        return cache[thres][key]
    check_against_reference(g, parts, value)
    # strict >: 0.25 and 0.5 are pair scores, and counting them would change the figure
    for sim, p in ev.SIM_PART.items():
        a, c, _ = ev.overlap(parts[p], corpus, g["I"])
        s = a / np.maximum(np.diff(parts[p][0])[:, None] + c - a, 1)
        assert (s == 0.25).any() and (s == 0.5).any()


def test_helper_canonical_loop_by_hand():
    inter = np.array([[1, 0, 2, 0], [0, 0, 0, 0], [0, 0, 0, 0]], np.int32)
    csize = np.array([[2, 3, 2, -1], [0, 4, -1, 0], [-1, -1, -1, -1]], np.int32)
    out, flags = ev.metrics(inter, csize, np.array([3, 0, 5]), np.float32(0.25))
    assert out[0].tolist() == [1 / 4 + 0 + 2 / 3, 1 / 3 + 0 + 2 / 3, (1 / 1 + 2 / 3) / 2, 1.0]       # 0.25 is not > 0.25
    assert out[1].tolist() == [0, 0, 0, 0] and out[2].tolist() == [0, 0, 0, 0]
    assert flags.tolist() == [0, 3, 0]
    q, c = ev.sets_of([[1, 5, 9], []]), ev.sets_of([[5, 9], [], [0, 1, 2, 3]])
    a, cs, err = ev.overlap(q, c, np.array([[10, 12, -1], [11, 13, 9]]), id_offset=10)
    assert a.tolist() == [[2, 1, 0], [0, 0, 0]] and cs.tolist() == [[2, 4, -1], [0, -1, -1]] and err == 1


# ------------------------------------------------------------------------------------------------ the C ABI
def test_eval_header_and_binding_declare_the_same_entry_points():
    names = declared("sss_eval.h")
    assert names == _lib.symbols("sss_eval.h") == ["sss_item_overlap", "sss_overlap_metrics"]
    L = _lib.lib()
    for n in names:
        assert getattr(L, n).argtypes == _lib.HEADERS["sss_eval.h"][n][1] and getattr(L, n).restype is _lib.HEADERS["sss_eval.h"][n][0]
    others = {"sss.h": _lib.exported_symbols(), "sss_sparse.h": _lib.symbols("sss_sparse.h"), "sss_l2.h": _lib.symbols("sss_l2.h"),
              "sss_pad.h": _lib.symbols("sss_pad.h"), "sss_graph.h": _lib.symbols("sss_graph.h")}
    for header, bound in others.items():
        assert declared(header) == bound and not set(names) & set(bound), header
    assert len(others["sss.h"]) == 60
    text = open(os.path.join(ROOT, "include", "sss_eval.h")).read()
    assert "CALLER-OWNED DEVICE" in text and "-3 HIP error" in text


_P = 1 << 20                                                          # a non-null address; never dereferenced


def _overlap(L, **kw):
    a = dict(qp=_P, qi=_P, nq=4, cp=_P, ci=_P, n=100, I=_P, K=10, off=0, inter=_P, csize=_P, err=_P)
    a.update(kw)
    return L.sss_item_overlap(*[a[x] for x in ("qp", "qi", "nq", "cp", "ci", "n", "I", "K", "off", "inter", "csize", "err")], 0)


def _metrics(L, **kw):
    a = dict(inter=_P, csize=_P, qsize=_P, nq=4, K=10, thr=0.5, out=_P, flags=_P)
    a.update(kw)
    return L.sss_overlap_metrics(*[a[x] for x in ("inter", "csize", "qsize", "nq", "K", "thr", "out", "flags")], 0)


def test_eval_entry_points_validate_before_any_launch():
    """Every bad argument is -1 on a machine without a device: a call that skipped the check would reach the HIP runtime
    (-3) with addresses that are not memory."""
    L = _lib.lib()
    for bad in (dict(K=0), dict(K=1025), dict(K=-1), dict(nq=0), dict(nq=-5), dict(nq=1 << 31), dict(n=0), dict(n=1 << 31)):
        assert _overlap(L, **bad) == -1 and b"item_overlap" in L.sss_last_error(), bad
    for name in ("qp", "qi", "cp", "ci", "I", "inter", "csize", "err"):
        assert _overlap(L, **{name: 0}) == -1 and b"null" in L.sss_last_error(), name
    for bad in (dict(K=0), dict(K=1025), dict(nq=0), dict(nq=1 << 31)):
        assert _metrics(L, **bad) == -1 and b"overlap_metrics" in L.sss_last_error(), bad
    for name in ("inter", "csize", "qsize", "out", "flags"):
        assert _metrics(L, **{name: 0}) == -1 and b"null" in L.sss_last_error(), name


def test_python_surface_without_a_device():
    import sessionsimilaritysearch_amd as pkg
    from sessionsimilaritysearch_amd import evaluation
    for name in ("QueryParts", "query_parts", "item_overlap", "evaluate", "get_cur_jaccard", "get_future_jaccard", "get_all_jaccard",
                 "get_cur_recall", "get_all_recall", "get_future_recall", "get_future_map", "get_cur_map", "get_all_map",
                 "get_ave_score", "get_recall"):
        assert getattr(pkg, name) is getattr(evaluation, name) and name in pkg.__all__
        assert getattr(evaluation, name).__name__ == name and getattr(evaluation, name).__doc__
    with pytest.raises(ValueError, match="sim_type"):
        evaluation.get_ave_score(None, None, None, "all_query_score")
    with pytest.raises(TypeError, match="QueryParts"):
        evaluation.get_cur_jaccard(np.zeros((1, 1), np.int64), ([], []), None)


# ------------------------------------------------------------------------------------------------ split / concat
def table(sessions):
    """ActionTable of sessions given as lists of item ids, None = a search (its token: the action's index + 1)."""
    flat = [a for s in sessions for a in s]
    return ActionTable(np.r_[0, np.cumsum([len(s) for s in sessions], dtype=np.int64)].astype(np.int64),
                       np.array([a is None for a in flat], bool), np.array([0 if a is None else a for a in flat], np.int64),
                       np.array([i + 1 if a is None else 0 for i, a in enumerate(flat)], np.int64))


def rows(t):
    return [list(zip(t.is_search[a:b].tolist(), t.item_id[a:b].tolist(), t.query_tok[a:b].tolist()))
            for a, b in zip(t.sess_ptr[:-1], t.sess_ptr[1:])]


def test_split_and_concat_on_the_fixture():
    """split(1, 2) is the (seq, tar) cut the fixture's raw sessions were given; concat undoes it."""
    g, tab = golden()
    seq, tar = tab["query"].split(1, 2)
    for got, want in ((seq, tab["seq"]), (tar, tab["tar"]), (ActionTable.concat(seq, tar), tab["query"])):
        assert np.array_equal(got.sess_ptr, want.sess_ptr) and np.array_equal(got.is_search, want.is_search)
        assert np.array_equal(got.item_id, want.item_id) and got.sess_ptr.dtype == np.int64


@pytest.mark.parametrize("num,den", [(1, 2), (1, 3), (2, 3), (1, 1), (1, 100)])
def test_split_and_concat_edges(num, den):
    """A 1-action session (seq takes it, tar is empty), an empty session, a cut that leaves every tar empty (1, 1), one
    that leaves one action in every seq (1, 100); searches at both ends."""
    t = table([[7], [], [None, 3, 3, None, 9], [None], [4, 5], [1, 2, 3, None, 5, 6, 7]])
    seq, tar = t.split(num, den)
    pre = t.prefix(num, den)
    assert rows(seq) == rows(pre) and np.array_equal(seq.sess_ptr, pre.sess_ptr)
    full = rows(t)
    assert [a + b for a, b in zip(rows(seq), rows(tar))] == full
    assert rows(seq)[0] == full[0] and rows(tar)[0] == [] and rows(seq)[1] == rows(tar)[1] == []
    if (num, den) == (1, 1):
        assert int(tar.sess_ptr[-1]) == 0 and tar.is_search.shape == (0,) and tar.num_sessions == t.num_sessions
    if (num, den) == (1, 100):
        assert np.diff(seq.sess_ptr).tolist() == [1, 0, 1, 1, 1, 1]
    back = ActionTable.concat(seq, tar)
    assert rows(back) == full and np.array_equal(back.sess_ptr, t.sess_ptr)
    assert back.is_search.dtype == t.is_search.dtype and back.item_id.dtype == np.int64
    # concat is session-wise, not table-wise: b's actions follow a's inside every session
    assert rows(ActionTable.concat(tar, seq)) == [b + a for a, b in zip(rows(seq), rows(tar))]
    # slices of a larger table (sess_ptr[0] != 0 is not a form ActionTable takes; slice() rebases it)
    assert rows(ActionTable.concat(t.slice(2, 5), t.slice(0, 3))) == [a + b for a, b in zip(full[2:5], full[0:3])]
    with pytest.raises(ValueError):
        ActionTable.concat(t, t.slice(0, 2))


def test_split_on_synthetic_sessions():
    t = synthetic_actions(300, 4, 50, 9)
    seq, tar = t.split(1, 2)
    ln = np.diff(t.sess_ptr)
    assert np.array_equal(np.diff(seq.sess_ptr), -(-ln // 2)) and np.array_equal(np.diff(tar.sess_ptr), ln // 2)
    assert rows(ActionTable.concat(seq, tar)) == rows(t)
