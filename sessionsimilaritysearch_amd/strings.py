"""The string metrics of a search result, on the device: ``Levenshtein.seqratio`` between the query strings (or the item
titles) of two sessions, and ``get_string_match``'s counts under ``get_query_metric``.

After a search the reference's ``main2`` prints ``get_ave_score(I, ..., 'all_query_score')`` and ``...
'all_product_title_score')`` (``test_amazon_filterd.py:672-673``; ``fine_tune_ours.py: get_score`` :56-65) and calls
``get_query_metric`` six times (``:416-441``, ``:741-757``): per (query, neighbour) pair a ``seqratio`` over two lists of
strings, which needs an edit distance for every pair of strings of the two lists.  Here the strings are a ``StringTable``
(code points on the device), the lists ``StringSequences`` (string ids in action order, repeats kept), and every pair of a
result ``I`` is one workgroup of one launch (``seq_pair_scores``; C ABI and the score of record:
``include/ext/sss_seqsim.h``).  ``evaluation.get_ave_score`` / ``get_recall`` take the two string
kinds over ``StringSequences``.  ``Levenshtein`` itself is not a dependency: the score of record is a restatement of its
documented definitions.  No CPU fallback.
"""
from __future__ import annotations

from typing import NamedTuple

import numpy as np
import torch

from . import _lib
from .index import _dev
from .sessions import ActionTable
from .sparse import _ptr_of

HEADER = "ext/sss_seqsim.h"
MAX_STRINGS = _lib.header_constant(HEADER, "SSS_SEQ_MAX_STRINGS")      # strings per sequence
MAX_CHARS = _lib.header_constant(HEADER, "SSS_STR_MAX_CHARS")          # code points per string
MAX_K = 1024


class StringTable:
    """``StringTable(strings, device=None)``: a list of ``str`` as code points on the device -- ``ptr`` int64
    ``[len + 1]`` and ``chars`` int32, string ``u`` being ``chars[ptr[u]:ptr[u + 1]]``.  A sequence names a string by its
    index here; equal strings under two indexes are allowed (they score as equal strings do).  ``len()`` is the number of
    strings, ``.device`` where they live, ``.lengths`` their lengths (host int64).  A string of more than 1024 code points
    raises ``SssError`` before anything is copied, the way ``session_vectors`` reports its 64-action limit: the kernel
    never truncates."""

    def __init__(self, strings, device=None):
        strings = list(strings)
        if not strings or not all(isinstance(s, str) for s in strings):
            raise TypeError("StringTable: expected a non-empty list of str")
        if len(strings) >= 2 ** 31:
            raise ValueError("StringTable: at most 2^31 - 1 strings")
        self.lengths = np.fromiter((len(s) for s in strings), np.int64, len(strings))
        if int(self.lengths.max()) > MAX_CHARS:
            raise _lib.SssError(f"StringTable: a string has more than {MAX_CHARS} code points (string {int(self.lengths.argmax())})")
        ptr = np.zeros(len(strings) + 1, np.int64)
        np.cumsum(self.lengths, out=ptr[1:])
        chars = np.frombuffer("".join(strings).encode("utf-32-le", "surrogatepass"), dtype="<i4")
        assert chars.shape[0] == int(ptr[-1])
        empty = np.flatnonzero(self.lengths == 0)
        self.empty_id = int(empty[0]) if empty.size else None       # the id of '', what an item without a title maps to
        dev = _dev(device)
        self.ptr = torch.from_numpy(ptr).to(dev)
        spare = torch.zeros(chars.shape[0] + 1, dtype=torch.int32, device=dev)   # an allocation even when all are ''
        spare[:chars.shape[0]] = torch.from_numpy(chars.astype(np.int32)).to(dev)
        self.chars = spare[:chars.shape[0]]

    def __len__(self) -> int:
        return int(self.lengths.shape[0])

    @property
    def device(self):
        return self.ptr.device


def check_sequences(ptr, ids, n_strings: int):
    """``(ptr, ids)`` as int64 host arrays, checked for ``StringSequences`` against a table of ``n_strings``: ValueError for
    a malformed ``ptr`` or an id outside the table, ``SssError`` for a row of more than 64 strings."""
    ptr, ids = np.asarray(ptr), np.asarray(ids)
    if ptr.ndim != 1 or ptr.size < 1 or ids.ndim != 1 or not np.issubdtype(ptr.dtype, np.integer) or \
            not (ids.size == 0 or np.issubdtype(ids.dtype, np.integer)):
        raise ValueError("StringSequences: ptr [rows + 1] and ids [entries] are one-dimensional integer arrays")
    ptr, ids = ptr.astype(np.int64), ids.astype(np.int64)
    ln = np.diff(ptr)
    if int(ptr[0]) != 0 or int(ptr[-1]) != ids.size or (ln < 0).any():
        raise ValueError("StringSequences: ptr must start at 0, never decrease and end at len(ids)")
    if ids.size and (int(ids.min()) < 0 or int(ids.max()) >= n_strings):
        raise ValueError(f"StringSequences: a string id lies outside [0, {n_strings})")
    if ln.size and int(ln.max()) > MAX_STRINGS:
        raise _lib.SssError(f"StringSequences: a session has more than {MAX_STRINGS} strings (row {int(ln.argmax())})")
    return ptr, ids


class StringSequences:
    """``StringSequences(ptr, ids, table)``: one row per session, ``ids[ptr[s]:ptr[s + 1]]`` the string ids of session
    ``s`` in action order (a sequence, not a set: repeats are kept).  ``ptr`` / ``ids``: host integer arrays; they are
    checked here -- ``ptr`` from 0, non-decreasing, ending at ``len(ids)``; ids inside the table; a row of more than 64
    strings raises ``SssError`` -- and then copied to the table's device (``.ptr`` int64, ``.ids`` int32, ``.lengths``
    int32).  ``.table`` is the ``StringTable`` the ids index."""

    def __init__(self, ptr, ids, table: StringTable):
        if not isinstance(table, StringTable):
            raise TypeError(f"StringSequences: table must be a StringTable, got {type(table).__name__}")
        ptr, ids = check_sequences(ptr, ids, len(table))
        ln = np.diff(ptr)
        dev = table.device
        self.table = table
        self.ptr = torch.from_numpy(ptr).to(dev)
        spare = torch.zeros(ids.size + 1, dtype=torch.int32, device=dev)
        spare[:ids.size] = torch.from_numpy(ids.astype(np.int32)).to(dev)
        self.ids = spare[:ids.size]
        self.lengths = torch.from_numpy(ln.astype(np.int32)).to(dev)

    def __len__(self) -> int:
        return int(self.ptr.shape[0] - 1)


def _rows(actions: ActionTable, keep, ids, table) -> StringSequences:
    """The kept actions' ids, sessions keeping their place (``ActionTable.clicks_only``'s prefix-sum cut)."""
    ptr = np.r_[0, np.cumsum(keep, dtype=np.int64)][np.asarray(actions.sess_ptr, np.int64) - int(actions.sess_ptr[0])]
    return StringSequences(ptr, ids[keep], table)


def _window(actions: ActionTable, x):
    return np.asarray(x)[int(actions.sess_ptr[0]):int(actions.sess_ptr[-1])]


def query_sequences(actions: ActionTable, table: StringTable, none_id=None) -> StringSequences:
    """The query strings of every session: ``query_tok`` of each search action, in order, as an id of ``table`` -- the
    reference's ``get_query(sess, pad=False)`` (``util_amazon_filtered.py:232-236``).  Search actions whose token is
    ``none_id`` are dropped: its ``action[2] is not None``.  Host numpy over the ``ActionTable``; no kernel."""
    srch = _window(actions, actions.is_search).astype(bool)
    tok = _window(actions, actions.query_tok).astype(np.int64)
    keep = srch if none_id is None else srch & (tok != int(none_id))
    return _rows(actions, keep, tok, table)


def title_sequences(actions: ActionTable, item_title, table: StringTable) -> StringSequences:
    """The item titles of every session: ``item_title[item_id]`` of each non-search action, in order, as an id of ``table``
    -- the reference's ``get_session_item_title`` (``util_amazon_filtered.py:36-37``).  ``item_title``: integer
    ``[n_items]``, -1 for an item without a title, which maps to the id of ``''`` (the table must then hold it).  Host numpy
    over the ``ActionTable``; no kernel."""
    title = np.asarray(item_title)
    if title.ndim != 1 or title.size == 0 or not np.issubdtype(title.dtype, np.integer):
        raise ValueError("item_title must be a non-empty one-dimensional integer array (one string id per item, -1: none)")
    keep = ~_window(actions, actions.is_search).astype(bool)
    item = _window(actions, actions.item_id).astype(np.int64)
    if keep.any() and (int(item[keep].min()) < 0 or int(item[keep].max()) >= title.size):
        raise ValueError(f"title_sequences: an item id lies outside [0, {title.size})")
    ids = title.astype(np.int64)[np.where(keep, item, 0)]
    if (ids[keep] < 0).any():
        if table.empty_id is None:
            raise ValueError("title_sequences: an item has no title and the table does not hold ''")
        ids = np.where(ids < 0, table.empty_id, ids)
    return _rows(actions, keep, ids, table)


class SequenceParts(NamedTuple):
    """The three query-side string lists of a ``(seq, tar)`` split: ``cur`` (of ``seq``), ``future`` (of ``tar``) and
    ``all`` (of ``seq[i] + tar[i]``), each a ``StringSequences`` with one row per query."""
    cur: StringSequences
    future: StringSequences
    all: StringSequences


def sequence_parts(seq: ActionTable, tar: ActionTable, table: StringTable, none_id=None) -> SequenceParts:
    """``SequenceParts`` of the query sessions' ``(seq, tar)`` tables (``ActionTable.split``): ``query_sequences`` of each
    part.  The 64-string limit holds for every part, ``all`` included."""
    return SequenceParts(query_sequences(seq, table, none_id), query_sequences(tar, table, none_id),
                         query_sequences(ActionTable.concat(seq, tar), table, none_id))


def _sequences(v, name) -> StringSequences:
    if not isinstance(v, StringSequences):
        raise TypeError(f"{name}: expected StringSequences, got {type(v).__name__}")
    return v


def seq_pair_scores(I, q: StringSequences, c: StringSequences, id_offset: int = 0):
    """``(ratio, qmatch, cmatch, clen)``, CUDA tensors ``[nq, K]`` (float64, then int32), for every pair of query ``i`` and
    row ``r = I[i, j] - id_offset`` of ``c``: ``ratio = seqratio(Q_i, C_r)``; ``qmatch`` / ``cmatch`` the strings of ``Q_i``
    / ``C_r`` that ``get_string_match`` marks (``Levenshtein.ratio > 0.9`` against some string of the other list);
    ``clen = len(C_r)``.  ``I``: numpy or a CUDA int64 tensor, K <= 1024.  ``I[i, j] == -1`` is a missing neighbour
    (``ratio`` nan, counts 0, ``clen`` -1); any other id outside ``c`` raises.  Both sides index one ``StringTable``."""
    q, c = _sequences(q, "q"), _sequences(c, "c")
    if q.table is not c.table:
        raise _lib.SssError("seq_pair_scores: the query and corpus sequences index different string tables")
    t, dev = q.table, q.table.device
    if not isinstance(I, torch.Tensor):
        I = torch.from_numpy(np.ascontiguousarray(np.asarray(I), dtype=np.int64)).to(dev)
    _lib.require_cuda(I, "I", torch.int64)
    if I.dim() != 2 or I.shape[0] != len(q) or not 0 < I.shape[1] <= MAX_K:
        raise ValueError(f"I must be [{len(q)}, K] with 0 < K <= {MAX_K}, got {tuple(I.shape)}")
    nq, K = int(I.shape[0]), int(I.shape[1])
    ratio = torch.empty((nq, K), dtype=torch.float64, device=dev)
    qmatch, cmatch, clen = (torch.empty((nq, K), dtype=torch.int32, device=dev) for _ in range(3))
    if nq == 0:
        return ratio, qmatch, cmatch, clen
    if len(c) == 0:
        raise ValueError("seq_pair_scores: the corpus has no rows")
    err = torch.zeros(1, dtype=torch.int32, device=dev)
    rc = _lib.lib().sss_seq_pair_scores(t.ptr.data_ptr(), _ptr_of(t.chars), len(t), q.ptr.data_ptr(), _ptr_of(q.ids), nq,
                                        c.ptr.data_ptr(), _ptr_of(c.ids), len(c), I.data_ptr(), K, int(id_offset), ratio.data_ptr(),
                                        qmatch.data_ptr(), cmatch.data_ptr(), clen.data_ptr(), err.data_ptr(), _lib.stream_ptr(dev))
    _lib.check(rc, "sss_seq_pair_scores")
    flags = int(err.item())
    if flags & 1:
        raise _lib.SssError(f"seq_pair_scores: I holds an id outside [{id_offset}, {id_offset + len(c)}) that is not the padding -1")
    if flags & 2:
        raise _lib.SssError(f"seq_pair_scores: a sequence of more than {MAX_STRINGS} strings, a string of more than {MAX_CHARS} "
                            "code points or a string id outside the table")
    return ratio, qmatch, cmatch, clen


def seq_query_metric(qmatch, cmatch, clen, qlen) -> torch.Tensor:
    """``sss_seq_query_metric``: per query the float64 sums over ascending ``j`` of ``(qmatch + cmatch) / (qlen + clen)``
    (column 0; an empty pair adds 0) and of ``qmatch / qlen`` (column 1; 0 for an empty query), missing neighbours adding
    nothing.  CUDA float64 ``[nq, 2]`` from ``seq_pair_scores``' int32 outputs and ``StringSequences.lengths``."""
    for name, t in (("qmatch", qmatch), ("cmatch", cmatch), ("clen", clen), ("qlen", qlen)):
        _lib.require_cuda(t, name, torch.int32)
    if qmatch.dim() != 2 or cmatch.shape != qmatch.shape or clen.shape != qmatch.shape or qlen.shape != qmatch.shape[:1] or \
            not 0 < qmatch.shape[1] <= MAX_K:
        raise ValueError(f"qmatch, cmatch and clen must be [nq, K] with 0 < K <= {MAX_K} and qlen [nq]")
    nq, K = int(qmatch.shape[0]), int(qmatch.shape[1])
    out = torch.empty((nq, 2), dtype=torch.float64, device=qmatch.device)
    if nq:
        rc = _lib.lib().sss_seq_query_metric(qmatch.data_ptr(), cmatch.data_ptr(), clen.data_ptr(), qlen.data_ptr(), nq, K,
                                             out.data_ptr(), _lib.stream_ptr(qmatch.device))
        _lib.check(rc, "sss_seq_query_metric")
    return out


def get_query_metric(I, test_data, train_data, mode, metric) -> float:
    """Drop-in for the reference's ``get_query_metric(I, test_data, train_data, mode, metric)``
    (test_amazon_filterd.py:416-441).  ``test_data``: a ``SequenceParts`` (``sequence_parts(seq, tar, table)``);
    ``train_data``: the corpus ``StringSequences`` (``query_sequences``); ``mode``: 'all', 'cur' or 'future' (anything else
    raises ``RuntimeError``, as upstream); ``metric``: 'score' -- ``(query matches + session matches) / (len(query) +
    len(session))`` per pair -- or 'recall' -- ``query matches / len(query)``.  Queries with an empty list are skipped and a
    missing neighbour (-1) adds no value; the mean is numpy's float64 mean over the pair values in ``(i, j)`` order."""
    if mode not in ("all", "cur", "future"):
        raise RuntimeError("unrecognized mode", mode)
    if metric not in ("score", "recall"):
        raise ValueError(f"metric must be 'score' or 'recall', got {metric!r}")
    if not isinstance(test_data, SequenceParts):
        raise TypeError("test_data must be a SequenceParts (strings.sequence_parts(seq, tar, table))")
    q = getattr(test_data, mode)
    _, qm, cm, cl = seq_pair_scores(I, q, _sequences(train_data, "train_data"))
    ql = q.lengths[:, None].expand_as(cl)
    if metric == "score":
        den = ql + cl
        val = torch.where(den == 0, torch.zeros((), dtype=torch.float64, device=cl.device), (qm + cm).double() / den.clamp(min=1).double())
    else:
        val = qm.double() / ql.clamp(min=1).double()
    vals = val[(ql > 0) & (cl >= 0)].cpu().numpy()                   # row-major: (i, j) order
    return float(np.mean(vals)) if vals.size else float("nan")
