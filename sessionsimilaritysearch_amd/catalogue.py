"""Catalogue heads: the trained model's own item prediction over the whole catalogue, and the loss its checkpoints are
selected by, at inference time.

In the reference these are four functions over ``sigmoid(rep @ asin_embedding.weight.T)``, a ``[B, V]`` matrix with
V = 391 572 items: ``get_next_product_asin_accuracy`` / ``get_next_product_asin_loss``
(``train_subsession_embedding.py:318-339, 271-302``) and ``get_all_product_asin_accuracy`` / ``get_all_product_asin_loss``
(``train_session_embedding.py:87-119, 122-``).  The validation loop of ``pretrain_filtered_amazon.py`` (:580-610) saves the
checkpoint with the lowest ``get_next_product_asin_loss``; ``test_amazon_filterd.py:126-133`` prints
``get_next_product_asin_accuracy(..., 20)`` as "Model Predict, Recall".  Here ``CatalogueHead`` keeps the item table on the
device and answers both without the ``[B, V]`` matrix: ``predict`` is the exact inner-product top-K of a ``FlatIndex`` over
the table, ``accuracy`` counts its hits against the target sets on the device, and ``bce`` is one fused GEMM + loss pass
(``sss_catalogue_bce``; C ABI and contract: ``include/heads/sss_catalogue.h``).  Targets are
``SessionVectors`` (``evaluation.query_parts(seq, tar).future`` for the next-product pair, ``.cur`` / ``.all`` for the
all-product pair; the weights are ignored).  Forward only, heads in eval mode.  No CPU fallback.
"""
from __future__ import annotations

from typing import NamedTuple

import numpy as np
import torch

from . import _lib
from ._device import Workspace
from .index import FlatIndex, _as_device_f32, _dev
from .sparse import SessionVectors, _ptr_of, device_vectors

HEADER = "heads/sss_catalogue.h"
MAX_K = 1024
N_NEG = 1000                        # the reference keeps a negative with probability 1000 / V


class CatalogueLoss(NamedTuple):
    """``loss`` = (sum of ``sums``) / (sum of ``counts``) in float64; ``sums`` float64 [B, 2] (positive part, negative part
    per row) and ``counts`` int64 [B, 2] (targets, kept negatives per row), on the host."""
    loss: float
    sums: np.ndarray
    counts: np.ndarray


def keep_threshold(n_neg, n_items: int) -> int:
    """``floor(min(1, n_neg / n_items) * 2^32)``: a negative is kept iff its 32-bit hash is below this (2^32: all are)."""
    if n_neg == "all":
        return 1 << 32
    if isinstance(n_neg, bool) or not isinstance(n_neg, (int, np.integer)) or n_neg < 0:
        raise ValueError(f"n_neg must be a non-negative integer or 'all', got {n_neg!r}")
    return (1 << 32) if n_neg >= n_items else (int(n_neg) << 32) // int(n_items)


def accuracy_of_hits(hit: np.ndarray, size: np.ndarray, K: int, skip_empty: bool):
    """``(precision, recall)`` from the per-row hit counts and target-set sizes: the float64 quotients ``hit / K`` and
    ``hit / size`` (numpy on the host: IEEE divisions, as the reference's Python floats) and numpy's mean of each."""
    empty = size == 0
    if not skip_empty and empty.any():
        raise ZeroDivisionError("float division by zero: a row has no targets")
    hit, size = hit[~empty].astype(np.float64), size[~empty].astype(np.float64)
    if not hit.shape[0]:
        return float("nan"), float("nan")
    return float(np.mean(hit / float(K))), float(np.mean(hit / size))


class CatalogueHead:
    """The item table ``target_asin_embedding.weight`` ``[V, d]`` (float32, ``d % 4 == 0``) on the device, with an optional
    ``variants.MLPHead`` (the reference's ``next_product_head`` / ``all_product_head``) run in front of every call.

    It keeps one zero-extended ``[V, Kp]`` image, ``Kp = ceil32(d)``, for the loss pass -- exact zero columns leave every fma
    chain unchanged, the argument ``FlatIndex(pad_scan=True)`` and ``use_id_embedding`` already rest on -- and, for
    prediction, a ``FlatIndex(d, pad_scan=True)`` over the same rows (d = 200, the reference's width, has no scan of its
    own), built on first use."""

    def __init__(self, item_table, head=None, device=None):
        self.device = _dev(device)
        t = _as_device_f32(item_table.detach() if isinstance(item_table, torch.Tensor) else item_table, self.device)   # (a Parameter)
        if t.dim() != 2 or t.shape[0] < 1 or t.shape[1] < 4 or t.shape[1] % 4:
            raise ValueError(f"item_table must be [V >= 1, d] with d % 4 == 0, got {tuple(t.shape)}")
        if t.shape[0] >= 2 ** 31:
            raise ValueError("item_table must have fewer than 2^31 rows")
        self.n_items, self.d = int(t.shape[0]), int(t.shape[1])
        self.kp = _lib.pad32(self.d)
        self.head = head
        if head is not None and head.n_out != self.d:
            raise ValueError(f"head gives {head.n_out} columns, the item table has {self.d}")
        self._rows = t
        if self.kp == self.d:
            self._image = t
        else:
            self._image = torch.zeros((self.n_items, self.kp), dtype=torch.float32, device=self.device)
            self._image[:, :self.d] = t
        self._index_box = [None]                        # shared with the views of with_head
        self._ws = Workspace(self.device)

    @property
    def index(self) -> FlatIndex:
        """The exact inner-product index over the table (built on first use; it adopts the rows, no copy)."""
        if self._index_box[0] is None:
            self._index_box[0] = FlatIndex(self.d, "ip", self.device, pad_scan=True).adopt(self._rows)
        return self._index_box[0]

    def with_head(self, head) -> "CatalogueHead":
        """The same table, index and workspace behind another head (or none): nothing is copied."""
        if head is not None and head.n_out != self.d:
            raise ValueError(f"head gives {head.n_out} columns, the item table has {self.d}")
        view = CatalogueHead.__new__(CatalogueHead)
        view.__dict__.update(self.__dict__)
        view.head = head
        return view

    def rep(self, emb) -> torch.Tensor:
        """``head.forward(emb)``, the reference's ``product_head(graph_embedding)`` in eval mode, or ``emb`` itself where there
        is no head: contiguous float32 ``[B, d]`` on the device."""
        x = _as_device_f32(emb.detach() if isinstance(emb, torch.Tensor) else emb, self.device)
        if x.dim() != 2:
            raise ValueError(f"expected [B, width], got {tuple(x.shape)}")
        if self.head is not None:
            x = self.head.forward(x)
        if x.shape[1] != self.d:
            raise ValueError(f"expected [B, {self.d}], got {tuple(x.shape)}")
        return x.contiguous()

    # ------------------------------------------------------------------------------------------ prediction
    @torch.no_grad()
    def predict(self, emb, K: int):
        """``(D float32 [B, K], I int64 [B, K])``, device tensors: the K items with the largest logit ``rep . table[i]`` per
        row, ordered by (logit descending, id ascending), scores as ``FlatIndex`` defines them.  Sigmoid and clip are
        monotone, so this is a valid ``torch.topk`` of the reference's clipped ``val`` -- and among the orders ``topk`` may
        return where values tie (everything the clip saturates ties) it is the only deterministic one."""
        K = int(K)
        if not 0 < K <= MAX_K:
            raise ValueError(f"K must be in 1..{MAX_K}")
        return self.index.search_device(self.rep(emb), K)

    def _targets(self, targets, B: int) -> SessionVectors:
        v = device_vectors(targets, "targets", weighted=False).check(self.n_items)
        if len(v) != B:
            raise ValueError(f"targets has {len(v)} rows, the batch {B}")
        if v.ptr.device != self.device:
            raise _lib.SssError("targets live on another device than the catalogue")
        return v

    @torch.no_grad()
    def hits(self, I: torch.Tensor, targets: SessionVectors) -> torch.Tensor:
        """int32 [B] on the device: the distinct ids of ``I[b]`` that are targets of row b (``sss_catalogue_hits``)."""
        _lib.require_cuda(I, "I", torch.int64)
        if I.dim() != 2 or not 0 < I.shape[1] <= MAX_K:
            raise ValueError(f"I must be [B, K] with 0 < K <= {MAX_K}, got {tuple(I.shape)}")
        B, K = int(I.shape[0]), int(I.shape[1])
        v = self._targets(targets, B)
        out = torch.empty(B, dtype=torch.int32, device=self.device)
        rc = _lib.lib().sss_catalogue_hits(I.data_ptr(), B, K, v.ptr.data_ptr(), _ptr_of(v.items), out.data_ptr(),
                                           _lib.stream_ptr(self.device))
        _lib.check(rc, "sss_catalogue_hits")
        return out

    @torch.no_grad()
    def accuracy(self, emb, targets: SessionVectors, K: int, skip_empty: bool = True):
        """``(precision, recall)`` of the top-K prediction: per row ``hit / K`` and ``hit / |targets|``, from the device's hit
        counts (one read-back of B integers; the quotients and their means are numpy's, no host loop over sessions).
        ``skip_empty=True`` leaves rows without targets out of both means (``get_next_product_asin_accuracy``); ``False``
        divides unguarded (``get_all_product_asin_accuracy``: ZeroDivisionError on an empty row, as the reference).  No rows:
        (nan, nan)."""
        _, I = self.predict(emb, K)
        hit = self.hits(I, targets)
        size = targets.ptr[1:] - targets.ptr[:-1]
        return accuracy_of_hits(hit.cpu().numpy(), size.cpu().numpy(), int(K), skip_empty)

    # ------------------------------------------------------------------------------------------ the loss
    @torch.no_grad()
    def bce_device(self, rep: torch.Tensor, targets: SessionVectors, n_neg=N_NEG, seed: int = 0, row_offset: int = 0):
        """``(sums float64 [B, 2], counts int64 [B, 2])`` on the device for representations ``rep [B, d]`` (the head is NOT
        run): one ``sss_catalogue_bce`` call, no host sync."""
        _lib.require_cuda(rep, "rep", torch.float32)
        if rep.dim() != 2 or rep.shape[1] != self.d:
            raise ValueError(f"rep must be [B, {self.d}], got {tuple(rep.shape)}")
        B = int(rep.shape[0])
        v = self._targets(targets, B)
        if not 0 <= int(seed) < 1 << 64 or int(row_offset) < 0:
            raise ValueError("seed must be in [0, 2^64) and row_offset >= 0")
        thr = keep_threshold(n_neg, self.n_items)
        mode, thr = (1, 0) if thr >> 32 else (0, thr)
        if self.kp != self.d:
            x = torch.zeros((B, self.kp), dtype=torch.float32, device=self.device)
            x[:, :self.d] = rep
        else:
            x = rep
        sums = torch.empty((B, 2), dtype=torch.float64, device=self.device)
        counts = torch.empty((B, 2), dtype=torch.int64, device=self.device)
        if B == 0:
            return sums, counts
        L = _lib.lib()
        ws = self._ws.get(L.sss_catalogue_bce_workspace_bytes(B, self.n_items))
        rc = L.sss_catalogue_bce(x.data_ptr(), self._image.data_ptr(), self._image.stride(0), self.kp, v.ptr.data_ptr(),
                                 _ptr_of(v.items), B, self.n_items, mode, thr, int(seed), int(row_offset), sums.data_ptr(),
                                 counts.data_ptr(), ws.data_ptr(), ws.numel(), _lib.stream_ptr(self.device))
        _lib.check(rc, "sss_catalogue_bce")
        return sums, counts

    def bce(self, emb, targets: SessionVectors, n_neg=N_NEG, seed: int = 0, row_offset: int = 0) -> CatalogueLoss:
        """The reference's loss ``mean(loss_mat[neg_mask | y])`` of a batch: every target pair, and of the other items
        ``n_neg`` in expectation per row (``"all"``: every one), chosen by a stateless hash of ``(seed, row_offset + b,
        item)`` in place of ``torch.rand([B, V])``.  ``loss`` = (sum of sums) / (sum of counts), added up on the host in
        float64 in ascending row order from the ``[B, 2]`` arrays (one small read-back, the reference's ``.item()``).  Raises
        ``AssertionError``, the reference's failure, when a sum is NaN or no element is kept."""
        sums, counts = self.bce_device(self.rep(emb), targets, n_neg, seed, row_offset)
        sums, counts = sums.cpu().numpy(), counts.cpu().numpy()
        total, kept = 0.0, 0
        for s, c in zip(sums.reshape(-1).tolist(), counts.reshape(-1).tolist()):
            total += s
            kept += c
        if np.isnan(total):                              # (raised, not asserted: python -O must not drop the check)
            raise AssertionError("catalogue bce: a loss term is NaN")
        if kept <= 0:
            raise AssertionError("catalogue bce: no element is kept")
        return CatalogueLoss(total / kept, sums, counts)


def _catalogue(catalogue, head) -> CatalogueHead:
    if not isinstance(catalogue, CatalogueHead):
        raise TypeError(f"catalogue must be a CatalogueHead, got {type(catalogue).__name__}")
    if head is None or head is catalogue.head:            # (None: the catalogue's own head, if it has one)
        return catalogue
    return catalogue.with_head(head)


def get_next_product_asin_accuracy(graph_embedding, product_head, targets, catalogue, K):
    """Drop-in for the reference's ``get_next_product_asin_accuracy(graph_embedding, product_head, data, asin_embedding, K)``
    (train_subsession_embedding.py:318-339): ``targets`` = ``query_parts(seq, tar).future`` in place of ``data``,
    ``catalogue`` a ``CatalogueHead`` in place of ``asin_embedding``; rows without targets are skipped."""
    return _catalogue(catalogue, product_head).accuracy(graph_embedding, targets, K, skip_empty=True)


def get_all_product_asin_accuracy(graph_embedding, product_head, targets, catalogue, K):
    """Drop-in for ``get_all_product_asin_accuracy`` (train_session_embedding.py:87-119): ``targets`` = ``.cur`` / ``.all``;
    a row without targets raises ZeroDivisionError, as the reference."""
    return _catalogue(catalogue, product_head).accuracy(graph_embedding, targets, K, skip_empty=False)


def get_next_product_asin_loss(graph_embedding, product_head, targets, catalogue, device=None, n_neg=N_NEG, seed=0, row_offset=0):
    """Drop-in for ``get_next_product_asin_loss(graph_embedding, product_head, data, asin_embedding, device)``
    (train_subsession_embedding.py:271-302), returning a float (``device`` is accepted and ignored: the catalogue has one)."""
    return _catalogue(catalogue, product_head).bce(graph_embedding, targets, n_neg, seed, row_offset).loss


def get_all_product_asin_loss(graph_embedding, product_head, targets, catalogue, device=None, n_neg=N_NEG, seed=0, row_offset=0):
    """Drop-in for ``get_all_product_asin_loss`` (train_session_embedding.py:122-): the same loss over ``.cur`` / ``.all``."""
    return _catalogue(catalogue, product_head).bce(graph_embedding, targets, n_neg, seed, row_offset).loss
