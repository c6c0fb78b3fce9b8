"""Scoring a search result on the device: item-overlap Jaccard, recall and MAP of ``I`` against the sessions themselves.

After ``D, I = index.search(...)`` the reference's ``main2`` scores ``I`` with Python sets, one (query, neighbour) pair at
a time (``test_amazon_filterd.py:669-740``: ``get_cur / future / all_jaccard`` :286-343, ``get_cur / all /
future_recall`` :345-382, ``get_future_map`` :226-244, ``get_recall`` :443-450; ``fine_tune_ours.py``: ``get_score`` /
``get_ave_score`` :42-97).  All of them are means of one primitive, ``|items(query i) & items(neighbour I[i, j])|``.  Here
the item sets are ``SessionVectors`` (``sparse.session_vectors(actions, "binary")``; the weights are ignored), the
primitive is one kernel launch per query part (``item_overlap``; C ABI: ``include/sss_eval.h``), the per-query sums a
second one, and the means over queries are taken in numpy float64 from ``nq`` doubles.  The functions below keep the
reference's names and argument order, with ``test_data`` a ``QueryParts`` and ``train_data`` the corpus
``SessionVectors``; ``evaluate`` returns all of them from three overlap launches.  No CPU fallback.

Deviations from the reference (DESIGN.md "Scoring a result"): an id of -1 in ``I`` is a missing neighbour (it scores 0
and is never a hit, but keeps its rank; the reference would wrap to the last session), and ``get_cur_map`` /
``get_all_map`` apply ``get_future_map``'s rule to the ``cur`` / ``all`` item sets (the reference's two index an older
dataset layout).  ``get_ave_score`` / ``get_recall`` also take ``'all_product_type_score'``, the kind the reference is
configured with, over type bags (``product_types.type_bags``; score of record: ``include/sss_ptype.h``), and the two string kinds ``'all_query_score'`` / ``'all_product_title_score'`` over
``strings.StringSequences`` (``Levenshtein.seqratio``; score of record: ``include/ext/sss_seqsim.h``).
"""
from __future__ import annotations

from typing import NamedTuple

import numpy as np
import torch

from . import _lib
from .sessions import ActionTable
from .sparse import SessionVectors, _ptr_of, session_vectors
from .strings import StringSequences, seq_pair_scores

MAX_K = 1024
PARTS = ("cur", "future", "all")
_SIM_PART = {"cur_jaccard": "cur", "all_jaccard": "all"}
PRODUCT_TYPE = "all_product_type_score"
QUERY_SCORE, TITLE_SCORE = "all_query_score", "all_product_title_score"


class QueryParts(NamedTuple):
    """The three query-side item sets of a ``(seq, tar)`` split: ``cur`` (the items of ``seq``), ``future`` (of ``tar``)
    and ``all`` (of ``seq[i] + tar[i]``), each a ``SessionVectors`` with one row per query."""
    cur: SessionVectors
    future: SessionVectors
    all: SessionVectors


def query_parts(seq: ActionTable, tar: ActionTable, device=None) -> QueryParts:
    """``QueryParts`` of the query sessions' ``(seq, tar)`` tables (``ActionTable.split``).  The 64-item-action limit of
    ``session_vectors`` holds for every part, ``all`` included, and is reported the same way."""
    return QueryParts(session_vectors(seq, "binary", device=device), session_vectors(tar, "binary", device=device),
                      session_vectors(ActionTable.concat(seq, tar), "binary", device=device))


def _sets(v, name) -> SessionVectors:
    if not isinstance(v, SessionVectors):
        raise TypeError(f"{name}: expected SessionVectors, got {type(v).__name__}")
    _lib.require_cuda(v.ptr, f"{name}.ptr", torch.int64)
    _lib.require_cuda(v.items, f"{name}.items", torch.int32)
    return v


def item_overlap(I, query_sets: SessionVectors, corpus_sets: SessionVectors, id_offset: int = 0):
    """``(inter, csize)``, CUDA int32 ``[nq, K]``: ``inter[i, j] = |Q_i & C_r|`` and ``csize[i, j] = |C_r|`` with
    ``r = I[i, j] - id_offset``.  ``I``: numpy or a CUDA int64 tensor ``[nq, K]``, K <= 1024.  ``I[i, j] == -1`` is a
    missing neighbour (``inter = 0, csize = -1``); any other id outside the corpus raises."""
    q, c = _sets(query_sets, "query_sets"), _sets(corpus_sets, "corpus_sets")
    dev = q.ptr.device
    if c.ptr.device != dev:
        raise _lib.SssError("item_overlap: the query and corpus sets live on different devices")
    if not isinstance(I, torch.Tensor):
        I = torch.from_numpy(np.ascontiguousarray(np.asarray(I), dtype=np.int64)).to(dev)
    _lib.require_cuda(I, "I", torch.int64)
    if I.dim() != 2 or I.shape[0] != len(q) or not 0 < I.shape[1] <= MAX_K:
        raise ValueError(f"I must be [{len(q)}, K] with 0 < K <= {MAX_K}, got {tuple(I.shape)}")
    nq, K = int(I.shape[0]), int(I.shape[1])
    inter = torch.empty((nq, K), dtype=torch.int32, device=dev)
    csize = torch.empty((nq, K), dtype=torch.int32, device=dev)
    if nq == 0:
        return inter, csize
    if len(c) == 0:
        raise ValueError("item_overlap: the corpus has no rows")
    err = torch.zeros(1, dtype=torch.int32, device=dev)
    rc = _lib.lib().sss_item_overlap(q.ptr.data_ptr(), _ptr_of(q.items), nq, c.ptr.data_ptr(), _ptr_of(c.items), len(c),
                                     I.data_ptr(), K, int(id_offset), inter.data_ptr(), csize.data_ptr(), err.data_ptr(),
                                     _lib.stream_ptr(dev))
    _lib.check(rc, "sss_item_overlap")
    if int(err.item()):
        raise _lib.SssError(f"item_overlap: I holds an id outside [{id_offset}, {id_offset + len(c)}) that is not the padding -1")
    return inter, csize


class PartScores(NamedTuple):
    """What one query part contributes: the overlaps on the device, and ``sss_overlap_metrics``'s per-query sums
    (``out`` float64 [nq, 4]: Jaccard sum, recall sum, average precision, pairs above ``thres``) and ``flags`` (bit 1: a
    pair with an empty union; bit 2: an empty query set) on the host."""
    inter: torch.Tensor
    csize: torch.Tensor
    qsize: torch.Tensor
    out: np.ndarray
    flags: np.ndarray


def part_scores(I, query_sets: SessionVectors, corpus_sets: SessionVectors, thres=None, id_offset: int = 0) -> PartScores:
    """One overlap launch and one reduction launch for one query part; ``nq`` rows of doubles and flags are copied."""
    inter, csize = item_overlap(I, query_sets, corpus_sets, id_offset)
    dev = inter.device
    nq, K = inter.shape
    qsize = (query_sets.ptr[1:] - query_sets.ptr[:-1]).to(torch.int32)
    out = torch.empty((nq, 4), dtype=torch.float64, device=dev)
    flags = torch.empty(nq, dtype=torch.int32, device=dev)
    if nq:
        thr = float("inf") if thres is None else float(thres)
        rc = _lib.lib().sss_overlap_metrics(inter.data_ptr(), csize.data_ptr(), qsize.data_ptr(), nq, K, thr, out.data_ptr(),
                                            flags.data_ptr(), _lib.stream_ptr(dev))
        _lib.check(rc, "sss_overlap_metrics")
    return PartScores(inter, csize, qsize, out.cpu().numpy(), flags.cpu().numpy())


def _mean(x) -> float:
    """numpy's float64 mean; of nothing it is nan, as the reference's ``np.mean([])``."""
    x = np.asarray(x, np.float64)
    return float(np.mean(x)) if x.size else float("nan")


def _jaccard(s: PartScores, skip_empty: bool) -> float:
    """Mean of the pair scores ``inter / union``.  ``skip_empty``: queries with an empty set are left out
    (``get_cur_jaccard`` / ``get_future_jaccard``); otherwise the union is divided by unguarded (``get_all_jaccard``)."""
    K = s.inter.shape[1]
    if skip_empty:
        return _mean(s.out[(s.flags & 2) == 0, 0]) / K
    if (s.flags & 1).any():
        raise ZeroDivisionError("division by zero: a (query, neighbour) pair has an empty union")
    return _mean(s.out[:, 0]) / K


def _recall(s: PartScores) -> float:
    return _mean(s.out[(s.flags & 2) == 0, 1]) / s.inter.shape[1]


def _map(s: PartScores) -> float:
    return _mean(s.out[:, 2])


def _ave_score(s: PartScores, sim_type: str) -> float:
    """``get_ave_score``: every pair score rounded to float32 first (the reference's ``np.zeros_like(I, dtype=np.float32)``),
    their mean in float64.  A missing neighbour scores 0; an empty union is 0 for 'cur_jaccard' and an error for
    'all_jaccard'."""
    if sim_type == "all_jaccard" and (s.flags & 1).any():
        raise ZeroDivisionError("division by zero: a (query, neighbour) pair has an empty union")
    union = s.qsize.to(torch.int64)[:, None] + s.csize - s.inter
    ok = (s.csize >= 0) & (union > 0)
    score = torch.where(ok, s.inter.double() / union.clamp(min=1).double(), torch.zeros((), dtype=torch.float64, device=union.device))
    return float(score.float().double().sum().item()) / score.numel() if score.numel() else float("nan")


def _above(s: PartScores, sim_type: str) -> float:
    """``get_recall``: the mean number of pair scores above ``thres`` (float32 comparison), over K."""
    if sim_type == "all_jaccard" and (s.flags & 1).any():
        raise ZeroDivisionError("division by zero: a (query, neighbour) pair has an empty union")
    return _mean(s.out[:, 3]) / s.inter.shape[1]


def _part(test_data: QueryParts, name: str) -> SessionVectors:
    if not isinstance(test_data, QueryParts):
        raise TypeError("test_data must be a QueryParts (evaluation.query_parts(seq, tar))")
    return getattr(test_data, name)


def _single(part, reduce):
    def fn(I, test_data, train_data):
        return reduce(part_scores(I, _part(test_data, part), train_data))
    return fn


get_cur_jaccard = _single("cur", lambda s: _jaccard(s, True))
get_future_jaccard = _single("future", lambda s: _jaccard(s, True))
get_all_jaccard = _single("all", lambda s: _jaccard(s, False))
get_cur_recall = _single("cur", _recall)
get_future_recall = _single("future", _recall)
get_all_recall = _single("all", _recall)
get_cur_map = _single("cur", _map)
get_future_map = _single("future", _map)
get_all_map = _single("all", _map)
for _name, _ref in (("get_cur_jaccard", "286-297"), ("get_future_jaccard", "331-343"), ("get_all_jaccard", "299-312"),
                    ("get_cur_recall", "345-356"), ("get_future_recall", "371-382"), ("get_all_recall", "358-369"),
                    ("get_cur_map", "266-284"), ("get_future_map", "226-244"), ("get_all_map", "246-264")):
    globals()[_name].__name__ = globals()[_name].__qualname__ = _name
    globals()[_name].__doc__ = (f"Drop-in for the reference's ``{_name}(I, test_data, train_data)`` (test_amazon_filterd.py:{_ref}): "
                                "``test_data`` a ``QueryParts``, ``train_data`` the corpus ``SessionVectors``; returns a float.")


def _sim_part(sim_type: str) -> str:
    if sim_type not in _SIM_PART:
        raise ValueError(f"sim_type must be 'all_jaccard', 'cur_jaccard', '{PRODUCT_TYPE}' or, over StringSequences, "
                         f"'{QUERY_SCORE}' / '{TITLE_SCORE}', got {sim_type!r}")
    return _SIM_PART[sim_type]


def _type_scores32(I, test_bags, train_bags) -> torch.Tensor:
    """float32 of the product-type score of record of every pair, a missing neighbour scoring 0: what the reference's
    ``gt = np.zeros_like(I, dtype=np.float32)`` holds."""
    from .product_types import bag_pair_scores
    return torch.nan_to_num(bag_pair_scores(I, test_bags, train_bags), nan=0.0).float()


def _is_string_kind(sim_type, test_data, train_data) -> bool:
    """A string kind over ``StringSequences`` on both sides; with anything else the kinds stay the ``ValueError`` of
    ``_sim_part``."""
    return sim_type in (QUERY_SCORE, TITLE_SCORE) and isinstance(test_data, StringSequences) and isinstance(train_data, StringSequences)


def _seq_scores32(I, test_seqs, train_seqs, sim_type) -> torch.Tensor:
    """float32 of ``seqratio`` of every pair, a missing neighbour scoring 0; 'all_query_score' scores 0 where either list
    is empty (fine_tune_ours.py:59-60), the title kind does not (two empty lists score 1.0)."""
    ratio, _, _, clen = seq_pair_scores(I, test_seqs, train_seqs)
    s = torch.nan_to_num(ratio, nan=0.0)
    if sim_type == QUERY_SCORE:
        s = torch.where((test_seqs.lengths[:, None] == 0) | (clen == 0), torch.zeros((), dtype=torch.float64, device=s.device), s)
    return s.float()


def _mean32(s: torch.Tensor) -> float:
    return float(s.double().sum().item()) / s.numel() if s.numel() else float("nan")


def _above32(s: torch.Tensor, thres) -> float:
    above = (s > torch.tensor(float(thres), dtype=torch.float32, device=s.device)).sum(1)
    return _mean(above.cpu().numpy()) / s.shape[1]


def get_ave_score(I, test_data, train_data, sim_type) -> float:
    """Drop-in for the reference's ``get_ave_score`` (fine_tune_ours.py:90-97) for the two item-set kinds of
    ``get_score``: 'all_jaccard' (raises ZeroDivisionError on an empty union, as the reference does) and 'cur_jaccard'
    (an empty union scores 0); and for 'all_product_type_score', the kind the reference is configured with: ``test_data`` is
    then the type bags of ``seq[i] + tar[i]`` (``product_types.type_bags(ActionTable.concat(seq, tar), ...)``) and
    ``train_data`` the corpus bags; and for 'all_query_score' / 'all_product_title_score' when both are
    ``strings.StringSequences`` (``query_sequences`` / ``title_sequences`` of ``ActionTable.concat(seq, tar)`` and of the
    corpus).  Every pair score is rounded to float32 first, their mean is taken in float64."""
    if sim_type == PRODUCT_TYPE:
        return _mean32(_type_scores32(I, test_data, train_data))
    if _is_string_kind(sim_type, test_data, train_data):
        return _mean32(_seq_scores32(I, test_data, train_data, sim_type))
    return _ave_score(part_scores(I, _part(test_data, _sim_part(sim_type)), train_data), sim_type)


def get_recall(test_data, train_data, I, sim_type, thres) -> float:
    """Drop-in for the reference's ``get_recall`` (test_amazon_filterd.py:443-450): the share of the K neighbours whose
    float32 pair score exceeds ``thres``, averaged over the queries.  'all_product_type_score' and the two string kinds: as
    ``get_ave_score``."""
    if sim_type == PRODUCT_TYPE:
        return _above32(_type_scores32(I, test_data, train_data), thres)
    if _is_string_kind(sim_type, test_data, train_data):
        return _above32(_seq_scores32(I, test_data, train_data, sim_type), thres)
    return _above(part_scores(I, _part(test_data, _sim_part(sim_type)), train_data, thres), sim_type)


def evaluate(I, test_data: QueryParts, train_data: SessionVectors, thres=None, id_offset: int = 0) -> dict:
    """Every metric above from one overlap launch per query part (three, not eleven): keys ``cur_jaccard``,
    ``future_jaccard``, ``all_jaccard``, ``cur_recall``, ``future_recall``, ``all_recall``, ``cur_map``, ``future_map``,
    ``all_map``, ``ave_all_jaccard``, ``ave_cur_jaccard`` and, with ``thres``, ``recall_all_jaccard`` /
    ``recall_cur_jaccard`` (``get_recall``)."""
    if not isinstance(I, torch.Tensor):
        I = torch.from_numpy(np.ascontiguousarray(np.asarray(I), dtype=np.int64)).to(_part(test_data, "cur").ptr.device)
    s = {p: part_scores(I, _part(test_data, p), train_data, thres, id_offset) for p in PARTS}
    res = {}
    for p in PARTS:
        res[f"{p}_jaccard"] = _jaccard(s[p], p != "all")
        res[f"{p}_recall"] = _recall(s[p])
        res[f"{p}_map"] = _map(s[p])
    for sim, p in _SIM_PART.items():
        res[f"ave_{sim}"] = _ave_score(s[p], sim)
        if thres is not None:
            res[f"recall_{sim}"] = _above(s[p], sim)
    return res
