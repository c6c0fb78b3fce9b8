"""Ground truth on the device: the exact item-set Jaccard of a query session against EVERY corpus session.

Everything else in the package ranks sessions under an embedding.  What the encoder is trained to approximate is the
reference's ``get_score`` (``fine_tune_ours.py:42-55``): here the Jaccard index of two sessions' item sets, over the items
of ``seq + tar`` (``'all_jaccard'``) or of ``seq`` (``'cur_jaccard'``) -- two of ``get_score``'s kinds; the kind the
reference is configured with, ``CFG.sim_type = 'all_product_type_score'``, is ``product_types.ProductTypeIndex``'s.
``JaccardIndex`` answers the three questions the reference could only put to a Python double loop: the true top-k neighbours (its commented-out loop,
``fine_tune_ours.py:899-907``), how many corpus sessions lie in each score band, and the first session of each band --
the fine-tuning triple mining of ``fine_tune_ours.py:187-235`` (``mine_triples``).  ``neighbourhood_recall`` is the ratio
``get_recall`` (``test_amazon_filterd.py:443-450``) approximates by dividing by K: the neighbours above a threshold that a
result ``I`` found, over those the whole corpus holds.

Item sets are ``SessionVectors`` (``sparse.session_vectors(actions, "binary")``, the parts of ``evaluation.query_parts``);
the weights are not read.  The contract -- the score of record, the order, the bands -- is stated once, in
``include/sss_jaccard.h``.  No CPU fallback.

Deviation from the reference: a pair of two empty sets scores 0, ``get_score('cur_jaccard')``'s rule; for ``'all_jaccard'``
the reference divides by zero there (``evaluation.get_ave_score`` raises for it; a search over a whole corpus cannot, one
search-only corpus session would fail every query).
"""
from __future__ import annotations

import ctypes
from typing import NamedTuple

import numpy as np
import torch

from . import _lib
from .evaluation import item_overlap
from .sparse import CsrIndex, SessionVectors, _ptr_of, device_vectors, query_pieces

MAX_EDGES = 7
MAX_QUERIES = 65535                  # per call of either entry point (include/sss_jaccard.h)


def check_edges(edges) -> np.ndarray:
    """``edges`` as a float64 array, or ValueError: 1..7 values, finite, strictly ascending."""
    e = np.atleast_1d(np.asarray(edges, np.float64))
    if e.ndim != 1 or not 1 <= e.size <= MAX_EDGES or not np.isfinite(e).all() or not (np.diff(e) > 0).all():
        raise ValueError(f"edges must be 1..{MAX_EDGES} finite, strictly ascending values, got {edges!r}")
    return np.ascontiguousarray(e)


def query_chunks(nq: int, per: int):
    """The (first query, queries) pieces of a batch of ``nq`` at ``per`` a call, never more than a call takes."""
    return query_pieces(nq, max(1, min(int(per), MAX_QUERIES)))


class BandIndex(CsrIndex):
    """What the two ground-truth indexes share (``JaccardIndex``, ``product_types.ProductTypeIndex``) beyond ``CsrIndex``:
    ``bands`` in query pieces.  A subclass gives ``_bands``, its one library call, and ``pair_scores(I, queries)``, numpy
    float64 ``[nq, K]`` with nan for a missing neighbour -- what ``mine_triples`` and ``neighbourhood_recall`` read."""

    def bands(self, sets, edges):
        """``(counts, first)``, device int64 ``[nq, len(edges) + 1]``: per query, the rows of every band and the lowest row
        + ``id_offset`` in it (-1: none).  The band of a row is the number of edges its float64 score reaches (``>=``);
        ``score > t`` is the edge ``nextafter(t, inf)``.  No host sync."""
        e = check_edges(edges)
        q = self._take(sets, "bands")
        nq, n, nb = len(q), self.ntotal, e.size + 1
        counts = torch.zeros((nq, nb), dtype=torch.int64, device=self.device)
        first = torch.full((nq, nb), -1, dtype=torch.int64, device=self.device)
        self.last_chunks = 0
        if n == 0:
            return counts, first
        L, st = _lib.lib(), _lib.stream_ptr(self.device)
        host_edges = (ctypes.c_double * e.size)(*e.tolist())

        def call(lo, m):
            self._bands(L, q, lo, m, n, ctypes.addressof(host_edges), e.size, counts.data_ptr() + 8 * lo * nb,
                        first.data_ptr() + 8 * lo * nb, st)
        self._each_piece(query_chunks(nq, MAX_QUERIES), call)
        return counts, first


class JaccardIndex(BandIndex):
    """Exact search under the item-set Jaccard: ``add(sets)``; ``search(sets, k) -> (D float32 [nq, k], I int64 [nq, k])``
    by (score desc, id asc), ids = row + ``id_offset``, padding (-FLT_MAX, -1) when ``ntotal < k``, rows scoring 0 ordinary
    results, k <= 1024; ``bands(sets, edges) -> (counts, first)`` over the float64 ``inter / uni``.  Scores, order and bands:
    ``include/sss_jaccard.h``."""
    weighted = False

    @property
    def sets(self) -> SessionVectors:
        """The corpus item sets (what ``evaluation.item_overlap`` takes); the weights are zeros, nothing reads them."""
        return SessionVectors(self._ptr, self._items, torch.zeros(self._items.numel(), dtype=torch.float32, device=self.device))

    def _take(self, v, what) -> SessionVectors:
        return device_vectors(v, what, weighted=False).check(self.n_items)

    def _topk(self, L, q, lo, m, n, k, d_ptr, i_ptr, st):
        ws = self._ws.get(L.sss_jaccard_topk_workspace_bytes(m, n))
        rc = L.sss_jaccard_topk(q.ptr.data_ptr() + 8 * lo, _ptr_of(q.items), m, self._ptr.data_ptr(), _ptr_of(self._items), n, k,
                                self.id_offset, d_ptr, i_ptr, ws.data_ptr(), ws.numel(), st)
        _lib.check(rc, "sss_jaccard_topk")

    def _bands(self, L, q, lo, m, n, edges_ptr, n_edges, counts_ptr, first_ptr, st):
        rc = L.sss_jaccard_bands(q.ptr.data_ptr() + 8 * lo, _ptr_of(q.items), m, self._ptr.data_ptr(), _ptr_of(self._items), n,
                                 edges_ptr, n_edges, self.id_offset, counts_ptr, first_ptr, st)
        _lib.check(rc, "sss_jaccard_bands")

    def search(self, sets, k: int):
        return self.search_device(self._take(sets, "search"), k)

    def pair_scores(self, I, sets):
        """``pair_scores(I, sets, self)``."""
        return pair_scores(I, sets, self)


def pair_scores(I, query_sets: SessionVectors, index: JaccardIndex):
    """Float64 ``inter / uni`` of every (query i, row ``I[i, j]``) pair, numpy ``[nq, K]``, from ``evaluation.item_overlap``;
    an empty union scores 0, a missing neighbour (-1) is nan."""
    inter, csize = item_overlap(I, query_sets, index.sets, index.id_offset)
    qsize = (query_sets.ptr[1:] - query_sets.ptr[:-1])[:, None]
    inter, csize = inter.to(torch.int64), csize.to(torch.int64)
    uni = qsize + csize - inter
    s = torch.where(uni > 0, inter.double() / uni.clamp(min=1).double(), torch.zeros((), dtype=torch.float64, device=uni.device))
    return torch.where(csize >= 0, s, torch.full((), float("nan"), dtype=torch.float64, device=uni.device)).cpu().numpy()


class Triples(NamedTuple):
    """``mine_triples``' result, numpy, one entry per query: the ids (-1: no such row) and float64 scores (nan: none) of the
    three picks, and ``keep``: all three exist."""
    pos: np.ndarray
    half: np.ndarray
    neg: np.ndarray
    pos_score: np.ndarray
    half_score: np.ndarray
    neg_score: np.ndarray
    keep: np.ndarray


def mine_triples(index: BandIndex, query_sets: SessionVectors, lo: float = 0.2, hi: float = 0.8) -> Triples:
    """The fine-tuning triple mining of the reference (``fine_tune_ours.py:187-235``) for a whole query batch: per query the
    FIRST corpus row scoring ``>= hi`` (``pos``), the first in ``[lo, hi)`` (``half``) and the first ``< lo`` (``neg``), with
    their scores, and ``keep`` where all three exist (the reference's ``cnt == 3``).  The rows are ``index.bands``' first
    rows of bands 2 / 1 / 0, the scores ``index.pair_scores``' float64 values (for a ``JaccardIndex`` ``inter / uni`` as the
    reference's Python computes them; for a ``ProductTypeIndex`` the score of record of ``include/sss_ptype.h``).  "First" is add
    order: the reference walks ``db_data`` as loaded, so a caller who wants other triples shuffles before ``add``."""
    _, first = index.bands(query_sets, (lo, hi))
    picks = first[:, [2, 1, 0]].contiguous()
    if picks.shape[0] == 0 or index.ntotal == 0:
        s = np.full(tuple(picks.shape), np.nan)
    else:
        s = index.pair_scores(picks, query_sets)
    p = picks.cpu().numpy()
    return Triples(p[:, 0], p[:, 1], p[:, 2], s[:, 0], s[:, 1], s[:, 2], (p >= 0).all(axis=1))


def neighbourhood_recall(I, index: BandIndex, query_sets: SessionVectors, thres: float):
    """``(mean, skipped)``: per query, the rows of ``I[i]`` scoring ``> thres`` over the corpus rows scoring ``> thres``,
    averaged over the queries that have such a row; the others are skipped and counted.  This is the ratio the reference's
    ``get_recall`` approximates by dividing by K (it could not count over the corpus).  Numerator: ``index.pair_scores``'
    float64 values (ids of -1 are missing and never count; ``I`` should not repeat an id); denominator:
    ``index.bands`` with the edge ``nextafter(thres, inf)``."""
    thres = float(thres)
    counts, _ = index.bands(query_sets, (np.nextafter(thres, np.inf),))
    den = counts[:, 1].cpu().numpy()
    if den.size == 0 or index.ntotal == 0:
        return float("nan"), int(den.size)
    s = index.pair_scores(I, query_sets)
    num = (s > thres).sum(axis=1)                        # nan > thres is False
    ok = den > 0
    return (float(np.mean(num[ok] / den[ok])) if ok.any() else float("nan")), int((~ok).sum())
