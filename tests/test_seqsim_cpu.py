"""CPU side of the string metrics (include/ext/sss_seqsim.h, sessionsimilaritysearch_amd/strings.py): the restatement of
the score of record (tests/helpers/seqsim_ref.py) on the two values the library's documentation prints -- the only pins
there are -- and on the properties the contract leans on; the ext header against its binding and its snapshot
(tests/golden/abi_signatures_ext.json); argument validation without a device; the Python surface."""
import json
import os
import random
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import abi  # noqa: E402
import seqsim_ref as ref  # noqa: E402

from sessionsimilaritysearch_amd import _lib  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = "sss_seqsim.h"
SNAPSHOT = os.path.join(ROOT, "tests", "golden", "abi_signatures_ext.json")


def sequences(rng, vocab, n, hi=6):
    return [[rng.choice(vocab) for _ in range(rng.randint(0, hi))] for _ in range(n)]


# ------------------------------------------------------------------------------------------------ the score of record
def test_the_two_documented_values():
    assert ref.seqratio(["newspaper", "litter bin", "tinny", "antelope"], ["caribou", "sausage", "gorn", "woody"]) == 0.21517857142857144
    assert ref.ratio("Hello world!", "Holly grail!") == 0.5833333333333334
    assert ref.indel("Hello world!", "Holly grail!") == 10 and ref.indel("", "") == 0 and ref.indel("abc", "") == 3
    assert ref.ratio("", "") == 1.0 and ref.seqratio([], []) == 1.0 and ref.seqratio(["a"], []) == 0.0
    assert ref.seqratio([""], [""]) == 1.0 and ref.seqratio(["ab", "ab"], ["ab"]) == (3 - 1.0) / 3


def test_seqratio_is_symmetric_and_stripping_common_ends_changes_nothing():
    rng = random.Random(11)
    vocab = ref.near_duplicates(rng, 40)
    for _ in range(400):
        A, B = sequences(rng, vocab, 2)
        if rng.random() < 0.5:                                       # a common prefix and suffix to strip
            pre, post = sequences(rng, vocab, 2, hi=2)
            A, B = pre + A + post, pre + B + post
        s = ref.seqratio(A, B)
        assert s == ref.seqratio(B, A)
        sa, sb = ref.strip_common(A, B)
        n, m = len(A) + len(B), len(sa) + len(sb)
        # the stripped pairs cost 0.0 each, and T + 0.0 is T: the distance is the stripped lists' distance, bit for bit
        assert ref.seqdist(A, B) == ref.seqdist(sa, sb)
        assert s == ((n - ref.seqdist(sa, sb)) / n if n else 1.0) and (m or s == 1.0)


def test_integer_match_rule_equals_both_float_forms():
    for L in range(1, 3000):
        d = np.arange(0, L + 1, dtype=np.int64)
        rule = L > 10 * d
        assert np.array_equal(rule, (L - d).astype(np.float64) / float(L) > 0.9)
        assert np.array_equal(rule, 1.0 - d.astype(np.float64) / float(L) > 0.9)
    assert ref.ratio_match("", "") and not ref.ratio_match("a", "")
    assert ref.ratio_match("abcdef", "abcde")                       # L = 11 = 10 d + 1: a match
    assert not ref.ratio_match("abcdefghijk", "abcdefghi")          # L = 20 = 10 d: none (L and d have one parity)


def test_the_cost_rounds_the_division_first():
    rng = random.Random(5)
    differ = 0
    for _ in range(3000):
        L = rng.randint(1, 2048)
        d = rng.randint(0, L)
        differ += (2.0 / L) * d != (2.0 * d) / L
    assert differ > 0                                               # the two forms are not interchangeable
    assert ref.cost("abc", "abd") == (2.0 / 6) * 2 and ref.cost("", "") == 0.0


def test_word_carried_bit_parallel_lcs_equals_the_table():
    """The recurrence the kernel runs, restated with Python integers cut into 64-bit words, against the row-by-row LCS:
    at the word edges, with carries that run through whole words (a long common run), with no match at all."""
    rng = random.Random(3)
    cases = [("", ""), ("a", ""), ("", "a"), ("a" * 64, "a" * 64), ("a" * 65, "a" * 64), ("a" * 129, "b" * 70), ("ab" * 64, "ba" * 64),
             ("x" * 63 + "y" * 66, "y" * 66 + "x" * 63)]
    for la in (1, 63, 64, 65, 127, 128, 129, 200):
        for lb in (1, 64, 90):
            a = "".join(rng.choice("abc") for _ in range(la))
            cases.append((a, "".join(rng.choice("abc") for _ in range(lb))))
            cases.append((a, a[:la // 2] + "c" + a[la // 2 + 1:]))
    for a, b in cases:
        assert ref.lcs_words(a, b) == ref.lcs(a, b) == ref.lcs(b, a), (a, b)


def test_helper_loops_by_hand():
    Q = [["red shoe", "red shoes"], [], ["x"]]
    C = [["red shoes", "blue"], [], ["red shoe", "red shoe", "red shoes"]]
    I = np.array([[0, 2, -1], [1, 0, 2], [1, -1, 0]])
    r, qm, cm, cl = ref.pair_scores(I, Q, C)
    assert ref.ratio_match("red shoe", "red shoes") and qm[0].tolist() == [2, 2, 0] and cm[0].tolist() == [1, 3, 0]
    assert cl.tolist() == [[2, 3, -1], [0, 2, 3], [0, -1, 2]] and np.isnan(r[0, 2]) and r[1, 0] == 1.0 and r[1, 1] == 0.0
    sums = ref.query_metric_sums(qm, cm, cl, [2, 0, 1])
    assert sums[0].tolist() == [3 / 4 + 5 / 5, 2 / 2 + 2 / 2] and sums[1].tolist() == [0.0, 0.0]
    parts = {"all": Q, "cur": Q, "future": [[], [], []]}
    assert ref.get_query_metric(I, parts, C, "all", "score") == float(np.mean([3 / 4, 5 / 5, 0 / 1, 0 / 3]))
    assert ref.get_query_metric(I, parts, C, "cur", "recall") == float(np.mean([1.0, 1.0, 0.0, 0.0]))
    assert np.isnan(ref.get_query_metric(I, parts, C, "future", "score"))
    with pytest.raises(RuntimeError):
        ref.get_query_metric(I, parts, C, "past", "score")
    # an empty list scores 0 under 'all_query_score' and is an ordinary seqratio under the title kind
    assert ref.score_matrix(I, Q, C, "all_query_score")[1].tolist() == [0.0, 0.0, 0.0]
    assert ref.score_matrix(I, Q, C, "all_product_title_score")[1].tolist() == [1.0, 0.0, 0.0]


# ------------------------------------------------------------------------------------------------ the C ABI
def test_ext_header_is_declared_exported_bound_and_equals_its_snapshot():
    names = abi.declared(os.path.join("ext", HEADER))
    assert names == sorted(_lib.EXT_HEADERS[HEADER]) == ["sss_seq_pair_scores", "sss_seq_query_metric"]
    assert sorted(_lib.EXT_HEADERS) == sorted(f for f in os.listdir(os.path.join(ROOT, "include", "ext")) if f.endswith(".h"))
    assert len(_lib.HEADERS) == 12 and len(_lib.PARAMS) == 98 and not set(_lib.EXT_PARAMS) & set(_lib.PARAMS)
    with open(SNAPSHOT) as f:
        snap = json.load(f)
    assert {h: {n: abi.signature(*sig) for n, sig in t.items()} for h, t in _lib.EXT_HEADERS.items()} == snap["functions"]
    assert {n: list(p) for n, p in _lib.EXT_PARAMS.items()} == snap["params"]
    L = _lib.lib()
    for n, sig in snap["functions"][HEADER].items():
        fn = getattr(L, n)                                           # exported by libsss.so
        assert abi.signature(fn.restype, fn.argtypes) == sig and len(_lib.EXT_PARAMS[n]) == len(sig[1]), n
    assert snap["functions"][HEADER]["sss_seq_query_metric"] == ["c_int", ["c_void_p"] * 4 + ["c_int64", "c_int", "c_void_p", "c_void_p"]]
    text = open(os.path.join(ROOT, "include", "ext", HEADER)).read()
    assert "CALLER-OWNED DEVICE" in text and "-3 HIP error" in text
    assert _lib.header_constant("ext/" + HEADER, "SSS_SEQ_MAX_STRINGS") == 64
    assert _lib.header_constant("ext/" + HEADER, "SSS_STR_MAX_CHARS") == 1024


_P = 1 << 20                                                          # a non-null address; never dereferenced
_PAIR = ("sp", "sc", "ns", "qp", "qi", "nq", "cp", "ci", "n", "I", "K", "off", "ratio", "qm", "cm", "cl", "err")
_METRIC = ("qm", "cm", "cl", "ql", "nq", "K", "out")


def _pair(L, **kw):
    a = dict(sp=_P, sc=_P, ns=50, qp=_P, qi=_P, nq=4, cp=_P, ci=_P, n=100, I=_P, K=10, off=0, ratio=_P, qm=_P, cm=_P, cl=_P, err=_P)
    a.update(kw)
    return L.sss_seq_pair_scores(*[a[x] for x in _PAIR], 0)


def _metric(L, **kw):
    a = dict(qm=_P, cm=_P, cl=_P, ql=_P, nq=4, K=10, out=_P)
    a.update(kw)
    return L.sss_seq_query_metric(*[a[x] for x in _METRIC], 0)


def test_ext_entry_points_validate_before_any_launch():
    """Every bad argument is -1 on a machine without a device: a call that skipped the check would reach the HIP runtime
    (-3) with addresses that are not memory."""
    L = _lib.lib()
    for bad in (dict(K=0), dict(K=1025), dict(K=-1), dict(nq=0), dict(nq=-5), dict(nq=1 << 31), dict(nq=1 << 28, K=8), dict(n=0),
                dict(n=1 << 31), dict(ns=0), dict(ns=1 << 31)):
        assert _pair(L, **bad) == -1 and b"seq_pair_scores" in L.sss_last_error(), bad
    for name in _PAIR:
        if name not in ("ns", "nq", "n", "K", "off"):
            assert _pair(L, **{name: 0}) == -1 and b"null" in L.sss_last_error(), name
    for bad in (dict(K=0), dict(K=1025), dict(nq=0), dict(nq=-1), dict(nq=1 << 31)):
        assert _metric(L, **bad) == -1 and b"seq_query_metric" in L.sss_last_error(), bad
    for name in ("qm", "cm", "cl", "ql", "out"):
        assert _metric(L, **{name: 0}) == -1 and b"null" in L.sss_last_error(), name


# ------------------------------------------------------------------------------------------------ the Python surface
def test_python_surface_without_a_device():
    import sessionsimilaritysearch_amd as pkg
    from sessionsimilaritysearch_amd import evaluation, strings
    for name in ("StringTable", "StringSequences", "SequenceParts", "query_sequences", "title_sequences", "sequence_parts",
                 "seq_pair_scores", "seq_query_metric", "get_query_metric"):
        assert getattr(pkg, name) is getattr(strings, name) and name in pkg.__all__
        assert getattr(strings, name).__name__ == name and getattr(strings, name).__doc__
    assert (strings.MAX_STRINGS, strings.MAX_CHARS, strings.MAX_K) == (64, 1024, 1024)
    # the limits raise when the table or the sequence set is built, before anything touches a device
    with pytest.raises(_lib.SssError, match="more than 1024 code points"):
        strings.StringTable(["ok", "x" * 1025])
    with pytest.raises(TypeError):
        strings.StringTable(["ok", 3])
    with pytest.raises(_lib.SssError, match="more than 64 strings"):
        strings.check_sequences([0, 1, 66], np.zeros(66, np.int64), 5)
    ptr, ids = strings.check_sequences([0, 0, 64], np.arange(64) % 5, 5)           # 64 is inside the limit; repeats are kept
    assert ptr.dtype == np.int64 and ids.tolist() == (np.arange(64) % 5).tolist()
    for bad in (([0, 2], [0, 5]), ([0, 2], [0, -1]), ([1, 2], [0, 0]), ([0, 3], [0, 0]), ([0, 2, 1, 2], [0, 0])):
        with pytest.raises(ValueError):
            strings.check_sequences(*bad, 5)
    with pytest.raises(TypeError, match="StringTable"):
        strings.StringSequences([0], [], None)
    # with anything but StringSequences on both sides the string kinds stay the ValueError they were
    for kind in ("all_query_score", "all_product_title_score"):
        with pytest.raises(ValueError, match="sim_type"):
            evaluation.get_ave_score(None, None, None, kind)
        with pytest.raises(ValueError, match="sim_type"):
            evaluation.get_recall(None, None, np.zeros((1, 1), np.int64), kind, 0.5)
    with pytest.raises(RuntimeError, match="unrecognized mode"):
        strings.get_query_metric(None, None, None, "past", "score")
    assert "out of scope" not in evaluation.__doc__ and "all_query_score" in evaluation.__doc__
