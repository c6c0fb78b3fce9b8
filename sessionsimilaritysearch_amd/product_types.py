"""Ground truth under the similarity the reference is configured with: the product-type cosine over the WHOLE corpus.

``config.py:61`` sets ``CFG.sim_type = 'all_product_type_score'``: the kind of ``get_score`` (``fine_tune_ours.py:66-85``)
that the fine-tuning triple mining (``:187-235``), the ground truth ``test()`` records (``:887``, ``:902``) and the first
figure ``main2`` prints after a search (``test_amazon_filterd.py:670``) all use.  It is the cosine of two sessions'
product-type count vectors: every non-search action whose item has a type (``get_item_type``,
``util_amazon_filtered.py:59-60``) adds one to its type's count; a session without a typed item is the zero vector and
scores 0 against everything.

``type_bags`` builds the count vectors of a whole ``ActionTable`` as ``SessionVectors`` (type ids ascending, counts as exact
float32), ``ProductTypeIndex`` is to them what ``jaccard.JaccardIndex`` is to item sets: exact top-k, band counts / first
rows, pair scores; ``jaccard.mine_triples`` and ``jaccard.neighbourhood_recall`` take either index.  The contract -- the
score of record, the order, the bands, the deviation from the reference's float64 arithmetic -- is stated once, in
``include/sss_ptype.h``.  No CPU fallback.
"""
from __future__ import annotations

import numpy as np
import torch

from . import _lib
from .index import _dev
from .jaccard import BandIndex, mine_triples, neighbourhood_recall, query_chunks  # noqa: F401  (the two functions: re-exported)
from .sessions import ActionTable
from .sparse import MAX_ITEMS, SessionVectors, _ptr_of, device_vectors, rows_of_sessions

MAX_K = 1024
MAX_NORM2 = 2 ** 26                  # a row's sum of squared counts (include/sss_ptype.h): dot < 2^31, nq2 * nc2 <= 2^52


def type_bags(actions: ActionTable, item_type, n_types: int | None = None, device=None) -> SessionVectors:
    """The type bags of all sessions of ``actions``: per session the distinct product types of its non-search actions,
    ascending, each with its count over ACTIONS (a type clicked through three items, or three times through one, counts 3).
    ``item_type``: int32 ``[n_items]`` (numpy or tensor), the type of every item, -1 for an item without one (the reference's
    ``action[4] is None``); ``n_types``: the type vocabulary (default ``max(item_type) + 1``).  Batched replacement of the
    reference's per-session ``get_item_type`` + counting loop; like ``sparse.session_vectors`` one host read sizes the output,
    and a session with more than 64 item actions, an item id outside ``[0, n_items)`` or a type id outside ``[-1, n_types)``
    raises ``SssError``."""
    ty = item_type if isinstance(item_type, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(np.asarray(item_type)))
    if ty.dim() != 1 or ty.numel() == 0 or ty.dtype not in (torch.int32, torch.int64):
        raise ValueError("item_type must be a non-empty one-dimensional integer array (one type id per item, -1: none)")
    if n_types is None:
        n_types = max(1, int(ty.max().item()) + 1)
    if not 0 < int(n_types) < 2 ** 31:
        raise ValueError("n_types must be in (0, 2^31)")
    n_types, n_items = int(n_types), int(ty.numel())
    dev = _dev(device)
    ty = ty.to(dev).clamp(-2, 2 ** 31 - 1).to(torch.int32).contiguous()       # an int64 id beyond int32 stays out of range
    args = (ty.data_ptr(), n_items, n_types)
    return rows_of_sessions(actions, dev, "sss_type_bags_count", args, "sss_type_bags_fill", args,
                            {1: f"type_bags: a session has more than {MAX_ITEMS} item actions",
                             2: f"type_bags: an item id lies outside [0, {n_items})",
                             4: f"type_bags: item_type holds a type id outside [-1, {n_types})"})


def check_bags(v, n_types: int | None = None, what: str = "bags") -> SessionVectors:
    """``v`` as a checked batch of type bags, or TypeError / SssError / ValueError: device ``SessionVectors``, well formed
    (``SessionVectors.check``), every count a positive integer and every row's sum of squared counts ``<= 2^26`` -- the
    range in which the score of record is exact integer arithmetic.  Device reductions and one host read, once per batch."""
    device_vectors(v, what, expected="SessionVectors (product_types.type_bags)")
    if n_types is not None or not getattr(v, "_checked", ()):                # checked against any vocabulary: well formed
        v.check(n_types)
    if getattr(v, "_bags_checked", False):
        return v
    lo, hi = int(v.ptr[0].item()), int(v.ptr[-1].item())
    if hi > lo:
        w = v.weights[lo:hi]
        whole = (w >= 1) & (w <= 8192) & (w == w.round())                      # 8192^2 = 2^26; nan compares False
        c = torch.where(whole, w, torch.zeros_like(w)).to(torch.int64)
        run = torch.zeros(hi - lo + 1, dtype=torch.int64, device=w.device)
        torch.cumsum(c * c, 0, out=run[1:])
        norm2 = run[v.ptr[1:] - lo] - run[v.ptr[:-1] - lo]
        if not bool((whole.all() & (norm2 <= MAX_NORM2).all()).item()):
            raise ValueError(f"{what}: the counts of a type bag are positive integers (exact float32) and every row's sum of "
                             f"squared counts is <= 2^26 (include/sss_ptype.h)")
    object.__setattr__(v, "_bags_checked", True)
    return v


def bag_pair_scores(I, query_bags: SessionVectors, corpus_bags: SessionVectors, id_offset: int = 0) -> torch.Tensor:
    """The float64 score of record of every (query i, row ``I[i, j] - id_offset``) pair, a CUDA tensor ``[nq, K]``; ``I``:
    numpy or a CUDA int64 tensor, K <= 1024.  ``I[i, j] == -1`` is a missing neighbour and scores nan; any other id outside
    the corpus raises (``evaluation.item_overlap``'s rules)."""
    q, c = check_bags(query_bags, None, "query_bags"), check_bags(corpus_bags, None, "corpus_bags")
    dev = q.ptr.device
    if c.ptr.device != dev:
        raise _lib.SssError("pair_scores: the query and corpus bags live on different devices")
    if not isinstance(I, torch.Tensor):
        I = torch.from_numpy(np.ascontiguousarray(np.asarray(I), dtype=np.int64)).to(dev)
    _lib.require_cuda(I, "I", torch.int64)
    if I.dim() != 2 or I.shape[0] != len(q) or not 0 < I.shape[1] <= MAX_K:
        raise ValueError(f"I must be [{len(q)}, K] with 0 < K <= {MAX_K}, got {tuple(I.shape)}")
    nq, K = int(I.shape[0]), int(I.shape[1])
    out = torch.empty((nq, K), dtype=torch.float64, device=dev)
    if nq == 0:
        return out
    if len(c) == 0:
        raise ValueError("pair_scores: the corpus has no rows")
    err = torch.zeros(1, dtype=torch.int32, device=dev)
    rc = _lib.lib().sss_ptype_pair_scores(q.ptr.data_ptr(), _ptr_of(q.items), _ptr_of(q.weights), nq, c.ptr.data_ptr(), _ptr_of(c.items),
                                          _ptr_of(c.weights), len(c), I.data_ptr(), K, int(id_offset), out.data_ptr(), err.data_ptr(),
                                          _lib.stream_ptr(dev))
    _lib.check(rc, "sss_ptype_pair_scores")
    if int(err.item()):
        raise _lib.SssError(f"pair_scores: I holds an id outside [{id_offset}, {id_offset + len(c)}) that is not the padding -1")
    return out


class ProductTypeIndex(BandIndex):
    """Exact search under the product-type cosine: ``add(bags)``; ``search(bags, k) -> (D float32 [nq, k], I int64 [nq, k])``
    by (float32 score desc, id asc), ids = row + ``id_offset``, padding (-FLT_MAX, -1) when ``ntotal < k``, rows scoring 0
    ordinary results, k <= 1024; ``bands(bags, edges) -> (counts, first)``; ``pair_scores(I, bags)`` numpy float64.  Scores,
    order and bands: ``include/sss_ptype.h``."""
    weighted = True

    def __init__(self, n_types: int, device=None):
        super().__init__(n_types, device)

    @property
    def n_types(self) -> int:
        return self.n_items

    @property
    def bags(self) -> SessionVectors:
        """The corpus bags."""
        v = SessionVectors(self._ptr, self._items, self._weights)
        object.__setattr__(v, "_checked", (self.n_items,))                  # rows enter through add(), which checked them
        object.__setattr__(v, "_bags_checked", True)
        return v

    def _take(self, v, what) -> SessionVectors:
        return check_bags(v, self.n_items, what)

    def _topk(self, L, q, lo, m, n, k, d_ptr, i_ptr, st):
        ws = self._ws.get(L.sss_ptype_topk_workspace_bytes(m, n))
        rc = L.sss_ptype_topk(q.ptr.data_ptr() + 8 * lo, _ptr_of(q.items), _ptr_of(q.weights), m, self._ptr.data_ptr(),
                              _ptr_of(self._items), _ptr_of(self._weights), n, k, self.id_offset, d_ptr, i_ptr, ws.data_ptr(),
                              ws.numel(), st)
        _lib.check(rc, "sss_ptype_topk")

    def _bands(self, L, q, lo, m, n, edges_ptr, n_edges, counts_ptr, first_ptr, st):
        rc = L.sss_ptype_bands(q.ptr.data_ptr() + 8 * lo, _ptr_of(q.items), _ptr_of(q.weights), m, self._ptr.data_ptr(),
                               _ptr_of(self._items), _ptr_of(self._weights), n, edges_ptr, n_edges, self.id_offset, counts_ptr,
                               first_ptr, st)
        _lib.check(rc, "sss_ptype_bands")

    def search(self, bags, k: int):
        return self.search_device(self._take(bags, "search"), k)

    def pair_scores(self, I, bags) -> np.ndarray:
        """The float64 score of record of every (query i, row ``I[i, j]``) pair, numpy ``[nq, K]``; nan for a missing
        neighbour (-1)."""
        return bag_pair_scores(I, self._take(bags, "pair_scores"), self.bags, self.id_offset).cpu().numpy()
