"""Sparse session index: the reference's SKNN / STAN item-vector baselines on the device.

In the reference (``test_amazon_filterd.py``) every corpus session becomes a unit vector over the item vocabulary
(``sequence_to_binary_vec`` :48-57), every query session a binary or time-decayed one (``sequence_to_stan_vec``
:37-46), and ``find_K_sparse_dense`` (:403-412) takes the top K of ``sparse_corpus . query`` per query in a Python
loop -- the ``'SKNN'`` / ``'STAN'`` branch of ``main2`` (:582-603).  The vocabulary has 391 572 items, so the vectors
stay sparse here: a batch of them is a CSR triple on the device (``SessionVectors``), built for a whole
``ActionTable`` at once by ``session_vectors`` and searched exactly by ``SparseSessionIndex`` (C ABI:
``include/sss_sparse.h``; contract: DESIGN.md "sparse session index").  No CPU fallback.
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np
import torch

from . import _lib
from ._device import Workspace, exhaustive_chunk
from .index import _dev
from .sessions import ActionTable

FLT_MAX = 3.4028234663852886e38
MAX_ITEMS = 64                      # item actions per session (include/sss_sparse.h)
_MODES = {"binary": 0, "stan": 1}


@dataclass
class SessionVectors:
    """CSR rows over the item vocabulary, on the device: ``ptr`` int64 [rows + 1], ``items`` int32 (ascending inside a
    row), ``weights`` float32 -- the values of record."""
    ptr: torch.Tensor
    items: torch.Tensor
    weights: torch.Tensor

    def __len__(self) -> int:
        return int(self.ptr.shape[0] - 1)

    def check(self, n_items: int | None = None):
        """Raise ValueError unless this is a well-formed batch: ``ptr`` non-decreasing inside ``items``, ``items`` and
        ``weights`` of one length, item ids strictly ascending inside every row (the search merges ascending lists; an
        unsorted row would silently score wrong) and inside ``[0, n_items)``.  Device reductions and one host read; the
        result is remembered per ``n_items`` (``_checked`` holds ``(n_items,)``, so "never checked" differs from
        "checked with None"), and a batch is checked once."""
        if getattr(self, "_checked", ()) == (n_items,):
            return self
        ptr, items = self.ptr, self.items
        if ptr.dim() != 1 or ptr.numel() < 1 or items.dim() != 1 or self.weights.shape != items.shape:
            raise ValueError("SessionVectors: ptr [rows + 1], items [nnz] and weights [nnz] are one-dimensional, items and weights alike")
        self.require_contiguous()
        lo, hi = int(ptr[0].item()), int(ptr[-1].item())
        bad = lo < 0 or hi > items.numel() or bool((ptr[1:] < ptr[:-1]).any().item())
        if not bad and hi - lo > 1:
            seg = items[lo:hi]
            rising = seg[1:] > seg[:-1]
            cut = ptr[1:-1]
            rising[(cut - lo - 1)[(cut > lo) & (cut < hi)]] = True    # a row's first entry follows another row's last
            bad = not bool(rising.all().item())
        if not bad and hi > lo:
            top = 2 ** 31 - 1 if n_items is None else n_items
            bad = int(items[lo:hi].min().item()) < 0 or int(items[lo:hi].max().item()) >= top
        if bad:
            raise ValueError("SessionVectors: ptr must be non-decreasing inside items, and the item ids of a row strictly "
                             f"ascending and inside [0, {n_items if n_items is not None else 2 ** 31 - 1})")
        object.__setattr__(self, "_checked", (n_items,))
        return self

    def require_contiguous(self):
        """Raise ValueError for a strided view (``ptr[::2]``): the C ABI reads all three through bare pointers.  No
        host sync."""
        for name in ("ptr", "items", "weights"):
            if not getattr(self, name).is_contiguous():
                raise ValueError(f"SessionVectors: {name} must be contiguous (got strides {tuple(getattr(self, name).stride())})")
        return self

    def to_numpy(self):
        return self.ptr.cpu().numpy(), self.items.cpu().numpy(), self.weights.cpu().numpy()


def _device_triple(ptr, items, weights, device) -> SessionVectors:
    """Host CSR arrays -> SessionVectors (items / weights keep one spare entry so that an empty batch still has an
    allocation behind its pointers)."""
    nnz = int(ptr[-1])
    it = torch.zeros(nnz + 1, dtype=torch.int32, device=device)
    w = torch.zeros(nnz + 1, dtype=torch.float32, device=device)
    it[:nnz] = torch.from_numpy(np.ascontiguousarray(items, dtype=np.int32)).to(device)
    w[:nnz] = torch.from_numpy(np.ascontiguousarray(weights, dtype=np.float32)).to(device)
    return SessionVectors(torch.from_numpy(np.ascontiguousarray(ptr, dtype=np.int64)).to(device), it[:nnz], w[:nnz])


def device_vectors(v, what: str, weighted: bool = True, expected: str = "SessionVectors") -> SessionVectors:
    """``v``, a ``SessionVectors`` of contiguous CUDA tensors of the C ABI's dtypes (the weights only when ``weighted``), or
    TypeError (it names ``expected``) / SssError.  What every index checks before ``SessionVectors.check``; no host sync."""
    if not isinstance(v, SessionVectors):
        raise TypeError(f"{what}: expected {expected}, got {type(v).__name__}")
    _lib.require_cuda(v.ptr, "ptr", torch.int64)
    _lib.require_cuda(v.items, "items", torch.int32)
    if weighted:
        _lib.require_cuda(v.weights, "weights", torch.float32)
    return v


def rows_of_sessions(actions: ActionTable, dev, count: str, count_args, fill: str, fill_args, messages) -> SessionVectors:
    """One CSR row per session of ``actions`` by a pair of builder entry points (``count`` / ``fill``, by name): the
    ``ActionTable`` staged on the device (``sess_ptr``, ``is_search``, ``item_id``; at least one entry, so an action-free
    table still has an allocation behind its pointers), then the two sweeps -- count, prefix sum, the one host read that
    sizes the output, fill -- and the err word: ``messages`` maps its bits to the ``SssError`` text, the lowest bit first.
    ``count_args`` / ``fill_args``: what each call takes between the session count and its outputs."""
    S = actions.num_sessions
    if S == 0:
        return SessionVectors(torch.zeros(1, dtype=torch.int64, device=dev), torch.zeros(0, dtype=torch.int32, device=dev),
                              torch.zeros(0, dtype=torch.float32, device=dev))
    L, st = _lib.lib(), _lib.stream_ptr(dev)
    sp = torch.from_numpy(np.ascontiguousarray(actions.sess_ptr, dtype=np.int64)).to(dev)
    T = max(1, int(actions.is_search.shape[0]))
    isr = torch.zeros(T, dtype=torch.uint8, device=dev)
    item = torch.zeros(T, dtype=torch.int64, device=dev)
    isr[:actions.is_search.shape[0]] = torch.from_numpy(np.ascontiguousarray(actions.is_search, dtype=np.uint8)).to(dev)
    item[:actions.item_id.shape[0]] = torch.from_numpy(np.ascontiguousarray(actions.item_id, dtype=np.int64)).to(dev)
    head = (sp.data_ptr(), isr.data_ptr(), item.data_ptr(), S)
    counts = torch.empty(S, dtype=torch.int32, device=dev)
    err = torch.zeros(1, dtype=torch.int32, device=dev)
    _lib.check(getattr(L, count)(*head, *count_args, counts.data_ptr(), err.data_ptr(), st), count)
    ptr = torch.zeros(S + 1, dtype=torch.int64, device=dev)
    torch.cumsum(counts, 0, out=ptr[1:])
    nnz = int(ptr[-1].item())                            # the one host read: sizes the output
    items = torch.empty(nnz + 1, dtype=torch.int32, device=dev)
    weights = torch.empty(nnz + 1, dtype=torch.float32, device=dev)
    _lib.check(getattr(L, fill)(*head, *fill_args, ptr.data_ptr(), items.data_ptr(), weights.data_ptr(), err.data_ptr(), st), fill)
    flags = int(err.item())
    for bit, text in messages.items():
        if flags & bit:
            raise _lib.SssError(text)
    return SessionVectors(ptr, items[:nnz], weights[:nnz])


def session_vectors(actions: ActionTable, mode: str = "binary", lammy=None, device=None, n_items: int | None = None) -> SessionVectors:
    """All sessions of ``actions`` as sparse vectors: ``mode="binary"`` (SKNN queries and every corpus row,
    ``sequence_to_binary_vec`` + ``normalize``) or ``mode="stan"`` (``sequence_to_stan_vec``; ``lammy`` is required --
    the reference's ``CFG.STAN_lammy`` is commented out, there is no default).  Batched replacement of the reference's
    per-session ``sequence_to_*_vec`` calls.  ``n_items``: the vocabulary the ids are checked against (default: any
    non-negative int32)."""
    if mode not in _MODES:
        raise ValueError(f"mode must be 'binary' or 'stan', got {mode!r}")
    if mode == "stan" and (lammy is None or not np.isfinite(lammy) or lammy <= 0):
        raise ValueError("mode='stan' needs a finite lammy > 0")
    vocab = int(n_items) if n_items is not None else 2 ** 31 - 1
    return rows_of_sessions(actions, _dev(device), "sss_session_vectors_count", (vocab,), "sss_session_vectors_fill",
                            (vocab, _MODES[mode], float(lammy) if mode == "stan" else 0.0),
                            {1: f"session_vectors: a session has more than {MAX_ITEMS} item actions",
                             2: f"session_vectors: an item id lies outside [0, {vocab})"})


def dense_to_vectors(x: np.ndarray, device=None) -> SessionVectors:
    """Dense [rows, n_items] host rows -> SessionVectors of their non-zero entries (values rounded to float32)."""
    x = np.asarray(x)
    if x.ndim != 2:
        raise ValueError(f"expected [rows, n_items], got {x.shape}")
    r, c = np.nonzero(x)                                 # row-major: items ascending inside a row
    ptr = np.zeros(x.shape[0] + 1, np.int64)
    np.cumsum(np.bincount(r, minlength=x.shape[0]), out=ptr[1:])
    return _device_triple(ptr, c, x[r, c], _dev(device))


def csr_to_vectors(m, device=None) -> SessionVectors:
    """A scipy CSR matrix [rows, n_items] -> SessionVectors (duplicates summed, indices sorted, explicit zeros kept out)."""
    m = m.tocsr().copy()
    m.sum_duplicates()
    m.eliminate_zeros()
    m.sort_indices()
    return _device_triple(m.indptr, m.indices, m.data, _dev(device))


def query_pieces(nq: int, per: int):
    """The (first query, queries) pieces of a batch of ``nq`` at ``per`` a call."""
    return [(lo, min(per, nq - lo)) for lo in range(0, nq, per)]


class CsrIndex:
    """What the exact indexes over CSR rows share (``SparseSessionIndex``, ``jaccard.JaccardIndex``,
    ``product_types.ProductTypeIndex``): the corpus on the device, with a weights column when ``weighted``, and the top-k
    call in query pieces under the exhaustive score budget.  A subclass gives ``_take(v, what) -> SessionVectors`` (checked)
    and ``_topk``, its one library call."""
    weighted = True

    def __init__(self, n_items: int, device=None):
        if not 0 < int(n_items) < 2 ** 31:
            raise ValueError("n_items must be in (0, 2^31)")
        self.n_items = int(n_items)
        self.device = _dev(device)
        self.id_offset = 0
        self._ptr = torch.zeros(1, dtype=torch.int64, device=self.device)
        self._items = torch.zeros(1, dtype=torch.int32, device=self.device)[:0]      # never NULL
        self._weights = torch.zeros(1, dtype=torch.float32, device=self.device)[:0] if self.weighted else None
        self._ws = Workspace(self.device)
        self.last_chunks = 0                             # query pieces of the last search (or bands)

    @property
    def ntotal(self) -> int:
        return int(self._ptr.shape[0] - 1)

    def add(self, vectors):
        v = self._take(vectors, "add")
        if len(v) == 0:
            return self
        lo, hi = int(v.ptr[0].item()), int(v.ptr[-1].item())         # the entries these rows own (v may be a slice of a larger batch)
        nnz_old, nnz = int(self._items.numel()), hi - lo

        def grown(old, new):                             # one spare entry: zero entries still have an allocation behind them
            t = torch.zeros(nnz_old + nnz + 1, dtype=old.dtype, device=self.device)
            t[:nnz_old] = old; t[nnz_old:nnz_old + nnz] = new[lo:hi].to(self.device)
            return t[:nnz_old + nnz]
        self._ptr = torch.cat([self._ptr, v.ptr[1:].to(self.device) - lo + nnz_old])
        self._items = grown(self._items, v.items)
        if self.weighted:
            self._weights = grown(self._weights, v.weights)
        return self

    def _pieces(self, nq, n):
        return query_pieces(nq, exhaustive_chunk(n, 4))                  # at most the 65535 queries a call takes

    def _each_piece(self, pieces, call):
        """``call(lo, m)`` per piece of the query batch, counted in ``last_chunks``."""
        self.last_chunks = 0
        for lo, m in pieces:
            call(lo, m)
            self.last_chunks += 1

    def search_device(self, q: SessionVectors, k: int, D: torch.Tensor | None = None, I: torch.Tensor | None = None):
        """``search`` for device vectors, into ``D`` / ``I`` when given; no host sync.  Queries go in pieces under the
        exhaustive score budget."""
        k = int(k)
        if not 0 < k <= 1024:
            raise ValueError("k must be in 1..1024")
        nq, n = len(q.require_contiguous()), self.ntotal
        if D is None:
            D = torch.empty((nq, k), dtype=torch.float32, device=self.device)
            I = torch.empty((nq, k), dtype=torch.int64, device=self.device)
        elif (I is None or tuple(D.shape) != (nq, k) or tuple(I.shape) != (nq, k) or D.dtype != torch.float32
              or I.dtype != torch.int64 or not D.is_contiguous() or not I.is_contiguous()):
            raise ValueError(f"D / I must be contiguous float32 / int64 [{nq}, {k}] tensors")
        self.last_chunks = 0
        if n == 0:
            D.fill_(-FLT_MAX); I.fill_(-1)
            return D, I
        if nq == 0:
            return D, I
        L, st = _lib.lib(), _lib.stream_ptr(self.device)

        def call(lo, m):
            self._topk(L, q, lo, m, n, k, D.data_ptr() + 4 * lo * k, I.data_ptr() + 8 * lo * k, st)
        self._each_piece(self._pieces(nq, n), call)
        return D, I


class SparseSessionIndex(CsrIndex):
    """Exact top-k over sparse session vectors: ``add(vectors)``, ``search(vectors, k) -> (D float32 [nq, k], I int64
    [nq, k])`` by (score desc, id asc), ids = row + ``id_offset``, padding (-FLT_MAX, -1) when ``ntotal < k``.  The score
    is the float64 sum of the products of the stored float32 weights over the shared items in ascending item order,
    rounded once to float32; rows scoring 0 are ordinary results.  k <= 1024."""

    @property
    def vectors(self) -> SessionVectors:
        return SessionVectors(self._ptr, self._items, self._weights)

    def _take(self, v, what) -> SessionVectors:
        if isinstance(v, np.ndarray):
            if v.ndim != 2 or v.shape[1] != self.n_items:
                raise ValueError(f"{what}: expected [rows, {self.n_items}], got {v.shape}")
            return dense_to_vectors(v, self.device)
        return device_vectors(v, what, expected="SessionVectors or a dense [rows, n_items] numpy array").check(self.n_items)

    def _topk(self, L, q, lo, m, n, k, d_ptr, i_ptr, st):
        # items / weights of an all-empty batch: zero entries, but sliced from a one-entry allocation (never NULL)
        ws = self._ws.get(L.sss_sparse_topk_workspace_bytes(m, n))
        rc = L.sss_sparse_topk(q.ptr.data_ptr() + 8 * lo, _ptr_of(q.items), _ptr_of(q.weights), m, self._ptr.data_ptr(),
                               _ptr_of(self._items), _ptr_of(self._weights), n, k, self.id_offset, d_ptr, i_ptr, ws.data_ptr(),
                               ws.numel(), st)
        _lib.check(rc, "sss_sparse_topk")

    def search(self, vectors, k: int):
        """Device ``SessionVectors`` -> device tensors; a dense [nq, n_items] numpy query -> numpy arrays."""
        q = self._take(vectors, "search")
        D, I = self.search_device(q, k)
        if isinstance(vectors, np.ndarray):
            return D.cpu().numpy(), I.cpu().numpy()
        return D, I


_SPARE = {}


def _ptr_of(t: torch.Tensor) -> int:
    """data_ptr of a tensor that may have zero entries: then of the allocation it was sliced from, or, where it has none
    (``torch.zeros(0)``), of a spare word on its device -- the C ABI takes no NULL, and reads nothing through a pointer
    whose rows are all empty."""
    if t.numel():
        return t.data_ptr()
    p = t.untyped_storage().data_ptr()
    if p:
        return p + t.storage_offset() * t.element_size()
    if t.device not in _SPARE:
        _SPARE[t.device] = torch.zeros(2, dtype=torch.int64, device=t.device)
    return _SPARE[t.device].data_ptr()


def find_K_sparse_dense(sparse_data, dense_query, K):
    """Drop-in for the reference's ``find_K_sparse_dense`` (test_amazon_filterd.py:403-412): ``sparse_data`` is a
    ``SparseSessionIndex`` or a scipy CSR matrix [n, n_items] (indexed on the fly), ``dense_query`` a dense
    [nq, n_items] array.  Returns (D float64 [nq, K], I int32 [nq, K]) like the reference; the values are this index's
    float32 scores and equal scores are ordered by ascending id (the reference's argsort order among ties is arbitrary)."""
    dense_query = np.asarray(dense_query)
    if isinstance(sparse_data, SparseSessionIndex):
        index = sparse_data
    else:
        index = SparseSessionIndex(sparse_data.shape[1])
        index.add(csr_to_vectors(sparse_data, index.device))
    D, I = index.search(dense_query, K)
    return D.astype(np.float64), I.astype(np.int32)
