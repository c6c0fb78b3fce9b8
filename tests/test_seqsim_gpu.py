"""The string metrics on the device (csrc/seqsim.hip, include/ext/sss_seqsim.h, strings.py) against the plain-Python
restatement of the score of record (tests/helpers/seqsim_ref.py).  Every comparison is ``==``, NaN matched by position:
the contract fixes every rounding, so there is no tolerance to state."""
import os
import random
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import seqsim_ref as ref  # noqa: E402

from sessionsimilaritysearch_amd import _lib, evaluation, strings  # noqa: E402
from sessionsimilaritysearch_amd.sessions import ActionTable  # noqa: E402

pytestmark = pytest.mark.gpu


def seqs_of(rows, table):
    """``StringSequences`` of rows given as lists of string ids."""
    ptr = np.r_[0, np.cumsum([len(r) for r in rows], dtype=np.int64)].astype(np.int64)
    return strings.StringSequences(ptr, np.array([k for r in rows for k in r], np.int64), table)


def strs_of(rows, vocab):
    return [[vocab[k] for k in r] for r in rows]


def same(got, want):
    return got.dtype == want.dtype and got.shape == want.shape and np.array_equal(got, want, equal_nan=True)


def check_pairs(I, qrows, crows, vocab, table, id_offset=0):
    """The four device outputs equal the restatement's; returns them (numpy)."""
    got = [t.cpu().numpy() for t in strings.seq_pair_scores(I, seqs_of(qrows, table), seqs_of(crows, table), id_offset)]
    want = ref.pair_scores(I, strs_of(qrows, vocab), strs_of(crows, vocab), id_offset)
    for name, g, w in zip(("ratio", "qmatch", "cmatch", "clen"), got, want):
        assert same(g, w), (name, np.argwhere(~((g == w) | ((g != g) & (w != w))))[:5])
    return got


def edit(rng, s, alphabet):
    k = rng.randrange(len(s))
    return s[:k] + rng.choice(alphabet) + s[k + 1:] if rng.random() < 0.5 else s[:k] + s[k + 1:]


def test_string_lengths_code_points_and_equal_content_under_two_ids(cuda):
    """One string per sequence, every pair of the vocabulary: lengths 0, 1, 63, 64, 65, 128, 129 and 1024 (the word edges
    of the bit-parallel LCS and the limit), each beside an edit of itself, code points above 0xFFFF that differ only there,
    and the longest strings' content again under second ids."""
    rng = random.Random(1)
    vocab = [""]
    for ln in (1, 63, 64, 65, 128, 129):
        s = "".join(rng.choice("ab") for _ in range(ln))
        vocab += [s, edit(rng, s, "abc")]
    big = "".join(rng.choice("abcd") for _ in range(1024))
    vocab += [big, edit(rng, big, "abcd"), "\U0001F600 shoes \U00010000", "\U0001F601 shoes \U00010000", "\uffff shoes \U00010000"]
    vocab += [vocab[11], big]                                        # the same content under two ids
    assert max(map(len, vocab)) == 1024 and len(vocab) == 20
    table = strings.StringTable(vocab, cuda)
    assert len(table) == 20 and table.device == cuda and table.chars.dtype == torch.int32 and int(table.chars.max()) == 0x1F601
    rows = [[k] for k in range(len(vocab))]
    I = np.tile(np.arange(len(vocab)), (len(vocab), 1))
    ratio, qm, cm, cl = check_pairs(I, rows, rows, vocab, table)
    assert (np.diag(ratio) == 1.0).all() and ratio[18, 11] == 1.0 and ratio[19, 13] == 1.0 and qm[19, 13] == 1 and (cl == 1).all()
    assert ratio[15, 16] < 1.0 and ratio[0, 0] == 1.0 and qm[0, 0] == 1 and qm[0, 1] == 0


def test_pairs_on_the_match_edge(cuda):
    """L == 10 d is no match, L == 10 d + 1 is one, two empty strings match; the counts are over positions."""
    vocab = ["abcdefghijk", "abcdefghi", "abcdef", "abcde", "", "x" * 50 + "y" * 5, "x" * 50 + "y" * 4 + "z", "x" * 45]
    table = strings.StringTable(vocab, cuda)
    assert [ref.ratio_match(vocab[a], vocab[b]) for a, b in ((0, 1), (2, 3), (4, 4), (5, 6), (5, 7))] == [False, True, True, True, False]
    assert ref.indel(vocab[5], vocab[6]) == 2 and ref.indel(vocab[5], vocab[7]) == 10       # L = 110 > 10 d = 20; L = 100 = 10 d
    qrows = [[0], [2], [4], [5], [0, 2, 2, 4], [5, 5]]
    crows = [[1], [3], [4], [6], [7], [3, 1, 3, 4, 4], [7, 6]]
    I = np.tile(np.arange(len(crows)), (len(qrows), 1))
    _, qm, cm, _ = check_pairs(I, qrows, crows, vocab, table)
    assert [qm[0, 0], qm[1, 1], qm[2, 2], qm[3, 3], qm[3, 4]] == [0, 1, 1, 1, 0]
    assert qm[4, 5] == 3 and cm[4, 5] == 4                           # "abcdef" twice and "" match; "abcde" twice and "" twice


def test_sequence_lengths_repeats_and_empty_lists(cuda):
    """Sequences of 0, 1, 2, 63 and 64 strings (one lane per row of T: the last lane, and the row without a left
    neighbour), a string repeated inside a sequence, two empty lists (1.0) and one (0.0)."""
    rng = random.Random(2)
    vocab = ref.near_duplicates(rng, 30, hi=12)
    table = strings.StringTable(vocab, cuda)
    rows = [[], [3], [3, 3], [rng.randrange(30) for _ in range(63)], [rng.randrange(30) for _ in range(64)], [7] * 64,
            [rng.randrange(30) for _ in range(64)], [5, 9, 5, 5, 9], []]
    I = np.tile(np.arange(len(rows)), (len(rows), 1))
    ratio, qm, cm, cl = check_pairs(I, rows, rows, vocab, table)
    assert ratio[0, 0] == 1.0 and ratio[0, 8] == 1.0 and ratio[0, 1] == 0.0 and ratio[4, 0] == 0.0 and cl[0].tolist() == [0, 1, 2, 63, 64, 64, 64, 5, 0]
    assert ratio[5, 5] == 1.0 and qm[5, 5] == 64 and qm[2, 1] == 2 and cm[2, 1] == 1 and 0.0 < ratio[4, 6] < 1.0
    # the per-query sums, in ascending j
    qlen = seqs_of(rows, table).lengths
    sums = strings.seq_query_metric(*[torch.from_numpy(x).to(cuda) for x in (qm, cm, cl)], qlen).cpu().numpy()
    assert same(sums, ref.query_metric_sums(qm, cm, cl, [len(r) for r in rows]))
    assert sums[0, 1] == 0.0 and sums[5, 0] > 0.0


@pytest.mark.parametrize("K", [1, 1024])
def test_k_1_and_1024_missing_neighbours_and_an_id_offset(cuda, K):
    rng = random.Random(K)
    vocab = ref.near_duplicates(rng, 25, hi=10)
    table = strings.StringTable(vocab, cuda)
    crows = [[rng.randrange(25) for _ in range(rng.randint(0, 5))] for _ in range(40)]
    qrows = [[rng.randrange(25) for _ in range(rng.randint(0, 4))] for _ in range(5)]
    I = np.array([[rng.randrange(40) + 1000 for _ in range(K)] for _ in qrows], np.int64)
    I[rng.randrange(5), rng.randrange(K)] = -1
    I[4, K - 1] = -1
    ratio, qm, cm, cl = check_pairs(I, qrows, crows, vocab, table, id_offset=1000)
    assert np.isnan(ratio[4, K - 1]) and cl[4, K - 1] == -1 and qm[4, K - 1] == 0 and np.isnan(ratio).sum() <= 2
    sums = strings.seq_query_metric(*[torch.from_numpy(x).to(cuda) for x in (qm, cm, cl)], seqs_of(qrows, table).lengths)
    assert same(sums.cpu().numpy(), ref.query_metric_sums(qm, cm, cl, [len(r) for r in qrows]))


def test_an_id_outside_the_corpus_raises(cuda):
    vocab = ["a", "b"]
    table = strings.StringTable(vocab, cuda)
    q, c = seqs_of([[0], [1]], table), seqs_of([[0], [1], [0, 1]], table)
    for bad in (3, -2, 1 << 40):
        with pytest.raises(_lib.SssError, match="outside"):
            strings.seq_pair_scores(np.array([[0, 1], [bad, 2]]), q, c)
    with pytest.raises(_lib.SssError, match="outside"):
        strings.seq_pair_scores(np.array([[0], [1]]), q, c, id_offset=1)
    with pytest.raises(ValueError):
        strings.seq_pair_scores(np.zeros((3, 1), np.int64), q, c)
    with pytest.raises(_lib.SssError, match="different string tables"):
        strings.seq_pair_scores(np.zeros((2, 1), np.int64), q, seqs_of([[0]], strings.StringTable(vocab, cuda)))


def test_the_kernel_never_truncates(cuda):
    """Past Python's checks, through the C ABI: a sequence of 65 strings, a string of 1025 code points and a string id
    outside the table make their pairs missing and OR 2 into err; the other pairs of the launch are scored."""
    t64 = lambda x: torch.tensor(x, dtype=torch.int64, device=cuda)
    t32 = lambda x: torch.tensor(x, dtype=torch.int32, device=cuda)
    sptr, chars = t64([0, 1, 2, 1027]), t32([97, 98] + [99] * 1025)             # "a", "b", "c" * 1025
    qptr, qids = t64([0, 1, 66, 67, 68]), t32([0] + [1] * 65 + [2] + [3])      # fine | 65 strings | the long string | id 3
    cptr, cids = t64([0, 2]), t32([0, 1])
    I = t64([[0], [0], [0], [0]])
    ratio = torch.zeros((4, 1), dtype=torch.float64, device=cuda)
    qm, cm, cl = (torch.full((4, 1), 7, dtype=torch.int32, device=cuda) for _ in range(3))
    err = t32([5])
    rc = _lib.lib().sss_seq_pair_scores(sptr.data_ptr(), chars.data_ptr(), 3, qptr.data_ptr(), qids.data_ptr(), 4, cptr.data_ptr(),
                                        cids.data_ptr(), 1, I.data_ptr(), 1, 0, ratio.data_ptr(), qm.data_ptr(), cm.data_ptr(),
                                        cl.data_ptr(), err.data_ptr(), 0)
    _lib.check(rc, "sss_seq_pair_scores")
    torch.cuda.synchronize(cuda)
    assert int(err.item()) == 2
    assert cl[:, 0].tolist() == [2, -1, -1, -1] and qm[:, 0].tolist() == [1, 0, 0, 0] and cm[:, 0].tolist() == [1, 0, 0, 0]
    r = ratio[:, 0].cpu().numpy()
    assert r[0] == ref.seqratio(["a"], ["a", "b"]) and np.isnan(r[1:]).all()


# ------------------------------------------------------------------------------------------------ the seeded fuzz
NQ, K, NC, NONE_ID = 64, 16, 200, 58


def fuzz_table(rng, n, vocab_ids, n_items):
    """``n`` sessions of 0-9 actions: a search with a query token out of ``vocab_ids`` (NONE_ID: the reference's None), or
    a click on an item; returned with the sessions as Python lists of (is_search, item, token)."""
    sess = [[(True, 0, rng.choice(vocab_ids)) if rng.random() < 0.45 else (False, rng.randrange(n_items), 0)
             for _ in range(rng.randint(0, 9))] for _ in range(n)]
    flat = [a for s in sess for a in s]
    ptr = np.r_[0, np.cumsum([len(s) for s in sess], dtype=np.int64)].astype(np.int64)
    return ActionTable(ptr, np.array([a[0] for a in flat], bool), np.array([a[1] for a in flat], np.int64),
                       np.array([a[2] for a in flat], np.int64)), sess


def lists_of(t: ActionTable):
    return [list(zip(t.is_search[a:b].tolist(), t.item_id[a:b].tolist(), t.query_tok[a:b].tolist()))
            for a, b in zip(t.sess_ptr[:-1], t.sess_ptr[1:])]


def fuzz_host():
    """64 queries, K = 16, 200 corpus sessions over a 60-string vocabulary of near-duplicates (id 58 stands for None, id 59
    is ''): the action tables, and both sides as the reference's lists of str."""
    rng = random.Random(7)
    vocab = ref.near_duplicates(rng, 59, alphabet="abcde ", lo=3, hi=20) + [""]
    n_items = 40
    item_title = np.array([rng.randrange(58) if rng.random() < 0.85 else -1 for _ in range(n_items)], np.int64)
    corpus, _ = fuzz_table(rng, NC, list(range(59)), n_items)
    query, _ = fuzz_table(rng, NQ, list(range(59)), n_items)
    seq, tar = query.split(1, 2)

    def queries(t):
        return [[vocab[tok] for s, _, tok in sess if s and tok != NONE_ID] for sess in lists_of(t)]

    def titles(t):
        return [[vocab[item_title[it]] if item_title[it] >= 0 else "" for s, it, _ in sess if not s] for sess in lists_of(t)]
    both = ActionTable.concat(seq, tar)
    I = np.array([[rng.randrange(NC) for _ in range(K)] for _ in range(NQ)], np.int64)
    for _ in range(20):
        I[rng.randrange(NQ), rng.randrange(K)] = -1
    host = {"parts": {"cur": queries(seq), "future": queries(tar), "all": queries(both)}, "corpus_q": queries(corpus),
            "all_t": titles(both), "corpus_t": titles(corpus)}
    # what the fixture has to contain for the tests below to mean something
    assert any(len(q) == 0 for q in host["parts"]["all"]) and any(len(c) == 0 for c in host["corpus_q"])
    assert any("" in t for t in host["corpus_t"]) and any(len(set(t)) < len(t) for t in host["corpus_t"])
    return I, host, vocab, item_title, (seq, tar, both, corpus)


@pytest.fixture(scope="module")
def fuzz(cuda):
    """``fuzz_host`` with both sides built on the device by the package's own builders."""
    I, host, vocab, item_title, (seq, tar, both, corpus) = fuzz_host()
    table = strings.StringTable(vocab, cuda)
    dev = {"parts": strings.sequence_parts(seq, tar, table, none_id=NONE_ID), "corpus_q": strings.query_sequences(corpus, table, NONE_ID),
           "all_t": strings.title_sequences(both, item_title, table), "corpus_t": strings.title_sequences(corpus, item_title, table),
           "vocab": vocab}
    return I, host, dev


def test_fuzz_builders_give_the_reference_lists(fuzz, cuda):
    I, host, dev = fuzz
    vocab = dev["vocab"]

    def lists(seqs):
        ptr, ids = seqs.ptr.cpu().numpy(), seqs.ids.cpu().numpy()
        return [[vocab[k] for k in ids[a:b]] for a, b in zip(ptr[:-1], ptr[1:])]
    for name in ("cur", "future", "all"):
        assert lists(getattr(dev["parts"], name)) == host["parts"][name], name
    assert lists(dev["corpus_q"]) == host["corpus_q"] and lists(dev["corpus_t"]) == host["corpus_t"] and lists(dev["all_t"]) == host["all_t"]
    assert len(dev["corpus_q"]) == NC and len(dev["parts"].all) == NQ and dev["all_t"].ids.device == cuda


def test_fuzz_pair_scores(fuzz):
    I, host, dev = fuzz
    for q, c in (("all_q", "corpus_q"), ("all_t", "corpus_t")):
        dq, hq = (dev["parts"].all, host["parts"]["all"]) if q == "all_q" else (dev[q], host[q])
        got = [t.cpu().numpy() for t in strings.seq_pair_scores(I, dq, dev[c])]
        for name, g, w in zip(("ratio", "qmatch", "cmatch", "clen"), got, ref.pair_scores(I, hq, host[c])):
            assert same(g, w), (q, name)
        assert (got[1] > 0).any() and ((got[0] > 0) & (got[0] < 1)).any() and np.isnan(got[0]).sum() >= 10


@pytest.mark.parametrize("mode", ref.MODES)
@pytest.mark.parametrize("metric", ref.METRICS)
def test_fuzz_get_query_metric(fuzz, mode, metric):
    I, host, dev = fuzz
    got = strings.get_query_metric(I, dev["parts"], dev["corpus_q"], mode, metric)
    want = ref.get_query_metric(I, host["parts"], host["corpus_q"], mode, metric)
    print(f"get_query_metric({mode}, {metric}) = {got!r}, restatement {want!r}")
    assert got == want and 0.0 < got < 1.0


@pytest.mark.parametrize("kind", ["all_query_score", "all_product_title_score"])
def test_fuzz_get_ave_score_and_get_recall(fuzz, kind):
    I, host, dev = fuzz
    dq, dc, hq, hc = ((dev["parts"].all, dev["corpus_q"], host["parts"]["all"], host["corpus_q"]) if kind == "all_query_score" else
                      (dev["all_t"], dev["corpus_t"], host["all_t"], host["corpus_t"]))
    got, want = evaluation.get_ave_score(I, dq, dc, kind), ref.get_ave_score(I, hq, hc, kind)
    print(f"get_ave_score({kind}) = {got!r}, restatement {want!r}")
    assert got == want and 0.0 < got < 1.0
    got, want = evaluation.get_recall(dq, dc, I, kind, 0.5), ref.get_recall(hq, hc, I, kind, 0.5)
    print(f"get_recall({kind}, 0.5) = {got!r}, restatement {want!r}")
    assert got == want and 0.0 < got < 1.0
    if kind == "all_query_score":                                    # the empty-list rule is what separates the kinds
        empty_both = [(i, j) for i in range(NQ) for j in range(K) if I[i, j] >= 0 and not hq[i] and not hc[I[i, j]]]
        assert empty_both and ref.get_ave_score(I, hq, hc, "all_product_title_score") > want
