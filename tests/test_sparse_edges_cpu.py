"""CPU side of tests/test_sparse_edges_gpu.py: that the inputs of those tests can tell a wrong kernel from a right one
(conditions on the inputs, checked against the numpy oracle alone), and SessionVectors.check() on host tensors.

The thresholds (10 % of all pairs, and of the pairs of rows longer than 16 entries) are floors on how many scores of the
committed sum-order batch change when the sum runs in descending item order or in float32; the generator's docstring
(tests/helpers/sparse_ref.py: sum_order_batch) says why they change at all."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import sparse_ref as ref  # noqa: E402

from sessionsimilaritysearch_amd.sparse import SessionVectors  # noqa: E402


def test_sum_order_batch_tells_the_orders_and_precisions_apart():
    q, c, n_items = ref.sum_order_batch()
    assert len(c[0]) - 1 == 700 and len(q[0]) - 1 == 24
    s = ref.scores(q, c, n_items)
    assert np.array_equal(s, ref.scores_variant(q, c, n_items)) and np.array_equal(s, ref.scores_pairs(q, c))
    long_rows = np.diff(c[0]) > 16
    assert np.isfinite(s).all() and 100 < long_rows.sum() < 600
    for name, other in (("descending", ref.scores_descending(q, c, n_items)), ("float32", ref.scores_float32(q, c, n_items))):
        differ = s != other
        print(f"{name}: differs on {differ.mean():.3f} of all pairs, {differ[:, long_rows].mean():.3f} of the long rows' pairs")
        assert differ.mean() >= 0.10 and differ[:, long_rows].mean() >= 0.10, name
    # the top-k sees negative, zero and positive scores; the empty rows alone (one length in 14, 50 of 700 expected) tie
    # at zero in every query, and most queries have such ties by the hundred
    zeros = (s == 0).sum(axis=1)
    print(f"negative {(s < 0).mean():.3f}, zero {(s == 0).mean():.3f}, positive {(s > 0).mean():.3f}, zeros per query {zeros.min()}..{zeros.max()}")
    assert (s < 0).mean() >= 0.10 and (s > 0).mean() >= 0.10
    assert (np.diff(c[0]) == 0).sum() >= 40 and (zeros >= (np.diff(c[0]) == 0).sum()).all() and np.median(zeros) >= 100


def test_edge_corpus_has_every_kind_of_wave_and_the_oracles_agree():
    c = ref.edge_corpus()
    q = ref.edge_queries(c)
    kinds = ref.wave_kinds(c[0])
    n = len(c[0]) - 1
    assert n == 933 and n % 256 and n % 64 and len(q[0]) - 1 == 40
    assert set(np.diff(c[0]).tolist()) == set(ref.SHORT + ref.LONG) and set(np.diff(q[0]).tolist()) >= {0, 1, 2, 3, 9, 16, 17, 40, 94}
    assert any(k[1] == 0 for k in kinds) and any(k[1] == k[3] == 64 for k in kinds) and any(0 < k[1] < k[3] for k in kinds)
    s = ref.scores(q, c, ref.EDGE_ITEMS)
    assert np.array_equal(s, ref.scores_pairs(q, c))                  # two statements of the contract, one result
    assert (s[0] == 0).all() and (s[1] == 0).all() and (s[4] == 0).all()          # below every row, above every row, empty
    r = int(np.argmax(np.diff(c[0])))
    w = c[2][c[0][r]:c[0][r + 1]].astype(np.float64)
    assert s[2, r] == np.float32(np.cumsum(w * w)[-1])               # the query equal to a row: its own squared norm


def test_check_limits_are_n_items_minus_one_and_n_items():
    def mk(items):
        return SessionVectors(torch.tensor([0, len(items)]), torch.tensor(items, dtype=torch.int32), torch.ones(len(items)))
    for n_items in (1, 10, 2 ** 31 - 1):
        assert mk([n_items - 1]).check(n_items) is not None
        if n_items > 1:
            assert mk([0, n_items - 1]).check(n_items) is not None
        with pytest.raises(ValueError):
            mk([n_items]).check(n_items)
        with pytest.raises(ValueError):
            mk([0, n_items]).check(n_items)
    assert mk([2 ** 31 - 2]).check() is not None                      # the default vocabulary: any id below the scorer's sentinel
    with pytest.raises(ValueError):
        mk([2 ** 31 - 1]).check()


BAD = {"an unsorted row": ([0, 2], [3, 1]), "a duplicate item in a row": ([0, 3], [1, 4, 4]), "a decreasing ptr": ([0, 2, 1], [1, 3]),
       "ptr[-1] > len(items)": ([0, 3], [1, 2]), "a negative id": ([0, 2], [-1, 3])}


@pytest.mark.parametrize("what", sorted(BAD))
def test_check_with_the_default_argument_checks(what):
    ptr, items = BAD[what]
    v = SessionVectors(torch.tensor(ptr), torch.tensor(items, dtype=torch.int32), torch.ones(len(items)))
    with pytest.raises(ValueError):
        v.check()
    with pytest.raises(ValueError):                                   # and a failed check is not remembered as a passed one
        v.check()
    with pytest.raises(ValueError):
        v.check(10)


def test_check_runs_once_per_n_items(monkeypatch):
    """Every real check starts with require_contiguous(); a remembered one returns before it."""
    calls = []
    real = SessionVectors.require_contiguous
    monkeypatch.setattr(SessionVectors, "require_contiguous", lambda self: (calls.append(1), real(self))[1])
    v = SessionVectors(torch.tensor([0, 2, 2, 5]), torch.tensor([1, 3, 0, 2, 9], dtype=torch.int32), torch.ones(5))
    assert not hasattr(v, "_checked")
    assert v.check() is v and len(calls) == 1 and v._checked == (None,)
    assert v.check() is v and v.check(None) is v and len(calls) == 1
    assert v.check(10) is v and len(calls) == 2 and v._checked == (10,)
    assert v.check(10) is v and len(calls) == 2
    assert v.check() is v and len(calls) == 3 and v._checked == (None,)          # one memo: the last n_items
    with pytest.raises(ValueError):
        v.check(9)                                                    # item 9 is outside [0, 9)
    assert len(calls) == 4 and v._checked == (None,)
