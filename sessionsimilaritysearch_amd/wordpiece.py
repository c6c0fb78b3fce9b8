"""The BERT WordPiece tokenizer on the device: a ``StringTable`` in, ``(input_ids, token_type_ids, attention_mask)`` out.

The reference feeds every query node and every product title through ``tokenizer(strings, padding='max_length',
max_length=20, truncation=True)`` inside ``sequence_to_graph`` (``util_amazon_filtered.py:19-20, 120-121``).  Here the
strings are already code points on the device (``strings.StringTable``), and ``WordPieceTokenizer`` turns them into the
integers ``BertNodeEncoder`` / ``NodeTextTransformer`` take in one launch (``sss_wordpiece_encode``; C ABI, the table
formats and the score of record: ``include/tok/sss_wordpiece.h``).  ``transformers`` /
``tokenizers`` are not dependencies: the definition below is a restatement, pinned against the real tokenizer by
tests/test_wordpiece_cpu.py.  No CPU fallback: ``__call__`` and ``encode_table`` need the device.

THE SCORE OF RECORD (single sentences; an integer result, bit-exact):

1. The per-code-point map (built here from ``unicodedata``; 0 to 3 mapped characters each, with a class: other, space or
   punctuation).  U+0000, U+FFFD and the categories Cc / Cf / Co are dropped, except ``\\t \\n \\r``, which become a space;
   Zs (and Zl / Zp) becomes a space; otherwise NFD with its Mn dropped (under ``strip_accents``; ``None`` follows
   ``do_lower_case``), then each remaining code point through Python's single-character ``str.lower()`` (under
   ``do_lower_case``).  A code point of HF's CJK ranges gets a space on either side of its mapped form (so the compatibility
   ideographs U+F900-FAFF and U+2F800-2FA1F are decomposed and still spaced) unless ``tokenize_chinese_chars`` is off.
   Unassigned code points are kept as "other".  Punctuation is the ASCII ranges 33-47, 58-64, 91-96, 123-126 and every
   category P*.  No rule looks at a neighbour: no final sigma, no canonical reordering of surviving marks.
2. Words are maximal runs of "other" characters; every punctuation character is a word of its own.
3. WordPiece per word: a word of more than ``max_input_chars_per_word`` mapped characters is one ``[UNK]``; otherwise
   greedy, longest piece first, ``##`` on continuation pieces; a position without a piece makes the whole word one ``[UNK]``.
4. ``[CLS]``, the first ``T - 2`` pieces, ``[SEP]``, ``[PAD]`` up to ``T``; ``attention_mask`` 1 on the real positions;
   ``token_type_ids`` all 0.

DIFFERENCES FROM HF: the literal text of a special token inside a string is ordinary text here (``"[SEP] a"`` gives ``[``,
``sep``, ``]``, ``a``); sentence pairs are not supported; every ``padding`` / ``truncation`` mode other than
``'max_length'`` / ``True`` raises ``ValueError``; and a few hundred code points above U+0700 whose Unicode category this
Python's tables and the ones HF's Rust crate carries disagree on (tests/golden/wordpiece_charmap_diff.json lists them).
"""
from __future__ import annotations

import functools
import os
import unicodedata
from typing import NamedTuple

import numpy as np

from . import _lib

HEADER = "tok/sss_wordpiece.h"
PAGES = _lib.header_constant(HEADER, "SSS_WP_PAGES")
CONT = _lib.header_constant(HEADER, "SSS_WP_CONT")
MAX_T = _lib.header_constant(HEADER, "SSS_WP_MAX_T")
ERR_CODEPOINT = _lib.header_constant(HEADER, "SSS_WP_ERR_CODEPOINT")
ERR_LENGTH = _lib.header_constant(HEADER, "SSS_WP_ERR_LENGTH")
MAX_CHARS = _lib.header_constant("ext/sss_seqsim.h", "SSS_STR_MAX_CHARS")
OTHER, SPACE, PUNCT = 0, 1, 2
CP_MASK = 0x1FFFFF
_SPACE_CHAR = 0x20 | (SPACE << 24)
# HF's is_chinese_char (tokenizers' BertNormalizer)
CJK_RANGES = ((0x4E00, 0x9FFF), (0x3400, 0x4DBF), (0x20000, 0x2A6DF), (0x2A700, 0x2B73F), (0x2B740, 0x2B81F),
              (0x2B920, 0x2CEAF), (0xF900, 0xFAFF), (0x2F800, 0x2FA1F))


# ------------------------------------------------------------------------------------------------ the character map
def _class_of(ch: str) -> int:
    cp = ord(ch)
    if cp == 0x20:
        return SPACE
    if 33 <= cp <= 47 or 58 <= cp <= 64 or 91 <= cp <= 96 or 123 <= cp <= 126:
        return PUNCT
    cat = unicodedata.category(ch)
    if cat in ("Zl", "Zp"):
        return SPACE
    return PUNCT if cat[0] == "P" else OTHER


def map_code_point(cp: int, lower: bool, strip: bool):
    """Step 1 without the CJK spaces: the ``(code point, class)`` pairs one input code point becomes."""
    if cp in (0x09, 0x0A, 0x0D):
        return ((0x20, SPACE),)
    ch = chr(cp)
    cat = unicodedata.category(ch)
    if cp == 0 or cp == 0xFFFD or cat in ("Cc", "Cf", "Co"):
        return ()
    if cat in ("Zs", "Zl", "Zp"):
        return ((0x20, SPACE),)
    if cat in ("Cn", "Cs"):                                 # unassigned (and lone surrogates): kept as they are
        return ((cp, OTHER),)
    out = ch
    if strip:
        out = "".join(c for c in unicodedata.normalize("NFD", out) if unicodedata.category(c) != "Mn")
    if lower:
        out = "".join(c.lower() for c in out)
    return tuple((ord(c), _class_of(c)) for c in out)


def is_cjk(cp: int) -> bool:
    return any(lo <= cp <= hi for lo, hi in CJK_RANGES)


@functools.lru_cache(maxsize=8)
def build_char_map(lower: bool, strip: bool, cjk: bool):
    """``(map_page int32 [4352], map_entry int32 [n_pages * 256], map_ext int32)`` in the format of
    include/tok/sss_wordpiece.h.  Entries of one-to-one mappings hold the DIFFERENCE of the code points, so every page of
    unchanged (or of dropped) code points is the same page and is stored once."""
    pages, page_of, entries_of = [], np.zeros(PAGES, np.int32), {}
    ext, ext_at = [], {}
    for p in range(PAGES):
        entries = []
        for cp in range(p << 8, (p + 1) << 8):
            out = map_code_point(cp, lower, strip)
            spaced = cjk and is_cjk(cp)
            if len(out) <= 1 and not (spaced and not out):
                e = (len(out) << 28) | (int(spaced) << 26)
                if out:
                    e |= ((out[0][0] - cp) & CP_MASK) | (out[0][1] << 24)
            else:
                if spaced:
                    out = ((0x20, SPACE),) + out + ((0x20, SPACE),)
                if not 2 <= len(out) <= 3:
                    raise ValueError(f"U+{cp:04X} maps to {len(out)} characters: the map holds at most 3")
                if out not in ext_at:
                    ext_at[out] = len(ext)
                    ext += [c | (cls << 24) for c, cls in out]
                e = (len(out) << 28) | ext_at[out]
            entries.append(e)
        key = tuple(entries)
        if key not in entries_of:
            entries_of[key] = len(pages)
            pages.append(entries)
        page_of[p] = entries_of[key]
    if len(ext) >= 1 << 24:
        raise ValueError("the character map's expansion store is too large")
    return page_of, np.asarray(pages, np.int32).reshape(-1), np.asarray(ext, np.int32)


def map_chars(text, char_map, strict: bool = True):
    """The packed mapped characters (code point | class << 24) of ``text`` -- a ``str`` or a sequence of code points --,
    read out of the TABLES the way the kernel reads them (for checking a map without a device)."""
    page_of, entry, ext = char_map
    out = []
    for cp in (map(ord, text) if isinstance(text, str) else text):
        e = int(entry[int(page_of[cp >> 8]) * 256 + (cp & 255)])
        n = (e >> 28) & 3
        if n >= 2:
            out += [int(c) for c in ext[(e & 0xFFFFFF):(e & 0xFFFFFF) + n]]
            continue
        spaced = (e >> 26) & 1
        out += [_SPACE_CHAR] * spaced
        if n:
            out.append(((cp + (e & CP_MASK)) & CP_MASK) | (e & (3 << 24)))
        out += [_SPACE_CHAR] * spaced
    return out


# ------------------------------------------------------------------------------------------------ the vocabulary table
def key_hash(key) -> int:
    """THE KEY HASH of include/tok/sss_wordpiece.h, in Python integers."""
    h = 2166136261
    for k in key:
        h = ((h ^ k) * 16777619) & 0xFFFFFFFF
    h ^= h >> 15
    h = (h * 0x2C1B3C6D) & 0xFFFFFFFF
    return h ^ (h >> 12)


def piece_key(token: str):
    """A token's key: its code points without the ``##`` of a continuation piece, ``CONT`` OR-ed into the first."""
    if token.startswith("##") and len(token) > 2:
        cps = [ord(c) for c in token[2:]]
        cps[0] |= CONT
        return tuple(cps)
    return tuple(ord(c) for c in token)


def next_pow2(n: int) -> int:
    return 1 << max(int(n) - 1, 0).bit_length()


def build_vocab_table(tokens, table_slots: int):
    """``(slots int32 [table_slots, 2], piece_ptr int32 [V + 1], piece_chars int32, max_piece_len)``: tokens inserted in id
    order by linear probing from ``key_hash & (table_slots - 1)``."""
    V = len(tokens)
    if table_slots & (table_slots - 1) or table_slots <= V or table_slots > 1 << 30:
        raise ValueError(f"table_slots must be a power of two greater than the vocabulary's {V} and at most 2^30, got {table_slots}")
    keys = [piece_key(t) for t in tokens]
    ptr = np.zeros(V + 1, np.int64)
    np.cumsum([len(k) for k in keys], out=ptr[1:])
    if int(ptr[-1]) >= 2 ** 31:
        raise ValueError("the vocabulary's pieces hold 2^31 code points or more")
    chars = np.fromiter((c for k in keys for c in k), np.int32, int(ptr[-1]))
    slots = np.full((table_slots, 2), -1, np.int32)
    mask = table_slots - 1
    for t, k in enumerate(keys):
        h = key_hash(k)
        s = h & mask
        while slots[s, 0] >= 0:
            s = (s + 1) & mask
        slots[s] = (t, np.uint32(h).astype(np.int32))
    longest = max((len(k) for k in keys), default=1)
    return slots, ptr.astype(np.int32), chars, max(longest, 1)


def table_lookup(key, slots, piece_ptr, piece_chars) -> int:
    """The id stored under ``key``, or -1: the kernel's probe sequence on the host tables."""
    mask = slots.shape[0] - 1
    h = key_hash(key)
    hs = int(np.uint32(h).astype(np.int32))
    s = h & mask
    for _ in range(slots.shape[0]):
        t = int(slots[s, 0])
        if t < 0:
            return -1
        if int(slots[s, 1]) == hs and tuple(int(c) for c in piece_chars[piece_ptr[t]:piece_ptr[t + 1]]) == tuple(key):
            return t
        s = (s + 1) & mask
    return -1


def load_vocab(vocab):
    """The tokens in id order, from a ``{token: id}`` dict, a list in id order or the path of a ``vocab.txt``."""
    if isinstance(vocab, (str, os.PathLike)):
        with open(vocab, encoding="utf-8") as f:
            vocab = [line.rstrip("\n") for line in f]
        while vocab and vocab[-1] == "":
            vocab.pop()
    if isinstance(vocab, dict):
        ids = sorted(vocab.values())
        if not all(isinstance(i, (int, np.integer)) and not isinstance(i, bool) for i in ids) or ids != list(range(len(ids))):
            raise ValueError("vocab: the ids must be 0 .. V - 1, each used once")
        tokens = [None] * len(ids)
        for t, i in vocab.items():
            tokens[int(i)] = t
    else:
        tokens = list(vocab)
    if not tokens or not all(isinstance(t, str) for t in tokens):
        raise ValueError("vocab: expected a non-empty {token: id} dict, list of str or vocab.txt path")
    if len(set(tokens)) != len(tokens):
        seen, dup = set(), None
        for t in tokens:
            if t in seen:
                dup = t
                break
            seen.add(t)
        raise ValueError(f"vocab: the token {dup!r} appears twice")
    return tokens


# ------------------------------------------------------------------------------------------------ results
class Tokens(NamedTuple):
    """int64 ``[n, T]`` device tensors, as a tuple, by attribute or by name (``tokens['input_ids']``; ``**tokens`` works)."""
    input_ids: "object"
    token_type_ids: "object"
    attention_mask: "object"

    def __getitem__(self, key):
        return getattr(self, key) if isinstance(key, str) else tuple.__getitem__(self, key)

    def keys(self):
        return self._fields


def _tokens(ids, n_tok) -> Tokens:
    import torch
    T = ids.shape[1]
    mask = (torch.arange(T, device=ids.device)[None, :] < n_tok[:, None]).to(torch.int64)
    return Tokens(ids.to(torch.int64), torch.zeros_like(mask), mask)


class TokenTable:
    """Every string of a ``StringTable`` encoded once: ``ids`` int32 ``[n, T]``, ``n_tok`` int32 ``[n]`` on the device;
    ``empty_id`` is the table's id of ``''`` (what a ``None`` query or an item without a title maps to)."""

    def __init__(self, ids, n_tok, empty_id=None):
        self.ids, self.n_tok, self.empty_id = ids, n_tok, empty_id
        self.max_length = int(ids.shape[1])

    def __len__(self) -> int:
        return int(self.ids.shape[0])

    def rows(self, string_ids) -> Tokens:
        """``Tokens`` of the strings ``string_ids`` (any integer array or tensor, any shape flattened to one dimension):
        ``rows(batch['query'].x)`` is the reference's ``get_query_node_tokens``, ``rows(item_title[batch['product'].x])`` its
        title tokens.  An id outside the table raises ``IndexError``."""
        import torch
        idx = torch.as_tensor(np.asarray(string_ids) if not isinstance(string_ids, torch.Tensor) else string_ids)
        idx = idx.to(self.ids.device, torch.int64).reshape(-1)
        if idx.numel() and (int(idx.min()) < 0 or int(idx.max()) >= len(self)):
            raise IndexError(f"TokenTable.rows: a string id lies outside [0, {len(self)})")
        return _tokens(self.ids.index_select(0, idx), self.n_tok.index_select(0, idx))


# ------------------------------------------------------------------------------------------------ the tokenizer
class WordPieceTokenizer:
    """``WordPieceTokenizer(vocab, do_lower_case=True, tokenize_chinese_chars=True, strip_accents=None, ...)``: the
    definition in the module docstring over ``vocab`` (a ``{token: id}`` dict with ids 0 .. V - 1, a list in id order or a
    ``vocab.txt`` path; a duplicate token or a missing special token raises ``ValueError``).  Construction builds the
    character map and the hash table on the host and touches no device; they are uploaded on first use.  ``table_slots``: the
    hash table's size, a power of two greater than V (default: the power of two at or above 2 V)."""

    def __init__(self, vocab, do_lower_case=True, tokenize_chinese_chars=True, strip_accents=None, unk_token="[UNK]",
                 cls_token="[CLS]", sep_token="[SEP]", pad_token="[PAD]", max_input_chars_per_word=100, device=None,
                 table_slots=None):
        self.tokens = load_vocab(vocab)
        self.vocab = {t: i for i, t in enumerate(self.tokens)}
        for name, tok in (("unk_token", unk_token), ("cls_token", cls_token), ("sep_token", sep_token), ("pad_token", pad_token)):
            if tok not in self.vocab:
                raise ValueError(f"vocab: the {name} {tok!r} is not in the vocabulary")
        self.unk_id, self.cls_id, self.sep_id, self.pad_id = (self.vocab[t] for t in (unk_token, cls_token, sep_token, pad_token))
        self.do_lower_case = bool(do_lower_case)
        self.strip_accents = self.do_lower_case if strip_accents is None else bool(strip_accents)
        self.tokenize_chinese_chars = bool(tokenize_chinese_chars)
        self.max_input_chars_per_word = int(max_input_chars_per_word)
        if self.max_input_chars_per_word < 1:
            raise ValueError("max_input_chars_per_word must be at least 1")
        self.table_slots = next_pow2(2 * len(self.tokens)) if table_slots is None else int(table_slots)
        self.char_map = build_char_map(self.do_lower_case, self.strip_accents, self.tokenize_chinese_chars)
        self.slots, self.piece_ptr, self.piece_chars, self.max_piece_len = build_vocab_table(self.tokens, self.table_slots)
        self._device_arg = device
        self._dev_tables = None

    @classmethod
    def from_transformers(cls, tok, **kw):
        """From a live HF BERT tokenizer: ``tok.get_vocab()``, its special tokens, and the options of its normalizer
        (``lowercase`` / ``strip_accents`` / ``handle_chinese_chars``) or, on a slow tokenizer, of ``tok`` itself."""
        norm = getattr(getattr(tok, "backend_tokenizer", None), "normalizer", None)
        if norm is not None and hasattr(norm, "lowercase"):
            lower, strip, cjk = norm.lowercase, norm.strip_accents, norm.handle_chinese_chars
        else:
            basic = getattr(tok, "basic_tokenizer", tok)
            lower, strip = getattr(basic, "do_lower_case", True), getattr(basic, "strip_accents", None)
            cjk = getattr(basic, "tokenize_chinese_chars", True)
        return cls(tok.get_vocab(), do_lower_case=lower, tokenize_chinese_chars=cjk, strip_accents=strip, unk_token=tok.unk_token,
                   cls_token=tok.cls_token, sep_token=tok.sep_token, pad_token=tok.pad_token, **kw)

    # -------------------------------------------------------------------------------------------- the tables on the host
    def lookup(self, piece: str, continuation: bool = False) -> int:
        """The id of ``piece`` as a word-initial or a continuation piece, or -1, through the hash table."""
        key = [ord(c) for c in piece]
        if continuation and key:
            key[0] |= CONT
        return table_lookup(tuple(key), self.slots, self.piece_ptr, self.piece_chars)

    def host_encode(self, text, T: int):
        """``(ids, n_tok)`` of one string, walking the TABLES the way the kernel walks them (the map's pages, the incremental
        hash, the probe sequence).  For holding the tables to the definition without a device; ``__call__`` never comes here."""
        m = map_chars(text, self.char_map)
        words, j = [], 0
        while j < len(m):
            c = (m[j] >> 24) & 3
            if c == SPACE:
                j += 1
                continue
            e = j + 1
            while c == OTHER and e < len(m) and (m[e] >> 24) & 3 == OTHER:
                e += 1
            words.append((j, e))
            j = e
        pieces = []
        for s, e in words[:max(T - 2, 0)]:
            got, p = [], s
            if e - s > self.max_input_chars_per_word:
                got = None
            while got is not None and p < e:
                best, best_end, key = -1, p, []
                for q in range(p, min(e, p + self.max_piece_len)):
                    key.append((m[q] & CP_MASK) | (CONT if q == p and p > s else 0))
                    t = table_lookup(tuple(key), self.slots, self.piece_ptr, self.piece_chars)
                    if t >= 0:
                        best, best_end = t, q + 1
                if best < 0:
                    got = None
                else:
                    got.append(best)
                    p = best_end
            pieces += [self.unk_id] if got is None else got
        pieces = pieces[:max(T - 2, 0)]
        ids = [self.cls_id] + pieces + [self.sep_id]
        return ids + [self.pad_id] * (T - len(ids)), len(ids)

    # -------------------------------------------------------------------------------------------- the device
    def _tables(self, device):
        import torch
        if self._dev_tables is None or self._dev_tables[0] != device:
            up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device)
            spare = lambda a: up(np.concatenate([a, np.zeros(1, a.dtype)]))      # an allocation even when empty
            self._dev_tables = (device, up(self.char_map[0]), up(self.char_map[1]), spare(self.char_map[2]), up(self.slots),
                                up(self.piece_ptr), spare(self.piece_chars))
        return self._dev_tables[1:]

    @staticmethod
    def _check_length(max_length) -> int:
        if isinstance(max_length, bool) or not isinstance(max_length, (int, np.integer)) or not 2 <= max_length <= MAX_T:
            raise ValueError(f"max_length must be an integer in 2..{MAX_T}, got {max_length!r}")
        return int(max_length)

    def encode_device(self, table, max_length: int = 20):
        """``(ids int32 [n, T], n_tok int32 [n], err int32 [1])`` on the table's device: one ``sss_wordpiece_encode`` call, no
        host sync.  ``err`` holds ``ERR_CODEPOINT`` / ``ERR_LENGTH`` bits; a row they concern is ``[CLS] [SEP]`` + padding."""
        import torch

        from .index import _dev
        from .sparse import _ptr_of
        from .strings import StringTable
        if not isinstance(table, StringTable):
            raise TypeError(f"expected a StringTable, got {type(table).__name__}")
        T = self._check_length(max_length)
        dev = table.device
        if self._device_arg is not None and _dev(self._device_arg) != dev:
            raise _lib.SssError("the string table lives on another device than the tokenizer")
        n = len(table)
        page, entry, ext, slots, pptr, pchars = self._tables(dev)
        ids = torch.empty((n, T), dtype=torch.int32, device=dev)
        n_tok = torch.empty(n, dtype=torch.int32, device=dev)
        err = torch.zeros(1, dtype=torch.int32, device=dev)
        rc = _lib.lib().sss_wordpiece_encode(
            table.ptr.data_ptr(), _ptr_of(table.chars), n, int(table.chars.shape[0]), page.data_ptr(), entry.data_ptr(),
            int(entry.shape[0]) // 256, ext.data_ptr(), int(ext.shape[0]) - 1, slots.data_ptr(), self.table_slots, pptr.data_ptr(),
            pchars.data_ptr(), len(self.tokens), self.max_piece_len, self.max_input_chars_per_word, self.unk_id, self.cls_id,
            self.sep_id, self.pad_id, T, ids.data_ptr(), n_tok.data_ptr(), err.data_ptr(), _lib.stream_ptr(dev))
        _lib.check(rc, "sss_wordpiece_encode")
        return ids, n_tok, err

    def encode_table(self, table, max_length: int = 20) -> TokenTable:
        """Every string of ``table`` encoded once, as a ``TokenTable`` (one launch and one read-back of the error word: a code
        point outside [0, 0x10FFFF] or a string of more than 1024 code points raises ``SssError``)."""
        ids, n_tok, err = self.encode_device(table, max_length)
        flags = int(err.item())
        if flags & ERR_CODEPOINT:
            raise _lib.SssError("WordPieceTokenizer: a string holds a code point outside [0, 0x10FFFF]")
        if flags & ERR_LENGTH:
            raise _lib.SssError(f"WordPieceTokenizer: a string has more than {MAX_CHARS} code points or leaves the table's chars")
        return TokenTable(ids, n_tok, table.empty_id)

    def __call__(self, strings, max_length: int = 20, padding="max_length", truncation=True) -> Tokens:
        """``Tokens(input_ids, token_type_ids, attention_mask)``, int64 ``[n, max_length]`` on the device, of a list of ``str``
        (or one ``str``, or a ``StringTable``).  Only ``padding='max_length'`` and ``truncation=True`` exist here."""
        from .strings import StringTable
        if padding != "max_length" or truncation is not True:
            raise ValueError(f"only padding='max_length' and truncation=True are supported, got padding={padding!r}, "
                             f"truncation={truncation!r}")
        self._check_length(max_length)
        if isinstance(strings, str):
            strings = [strings]
        if isinstance(strings, (tuple, list)) and strings and isinstance(strings[0], (tuple, list)):
            raise ValueError("sentence pairs are not supported")
        table = strings if isinstance(strings, StringTable) else StringTable(strings, self._device_arg)
        t = self.encode_table(table, max_length)
        return _tokens(t.ids, t.n_tok)
