"""CPU side of the WordPiece tokenizer (include/tok/sss_wordpiece.h, csrc/wordpiece.hip, wordpiece.py): the restatement
(tests/wordpiece_ref.py) against the recorded run of the Hugging Face BertTokenizer (tests/golden/wordpiece_cases.json,
make_golden_wordpiece.py) and, code point by code point, against the installed normalizer and pre-tokenizer; the pinned
divergences; the host-built tables; the tok header against its binding and its snapshot; argument validation without a
device."""
import json
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [HERE, os.path.join(HERE, "helpers"), os.path.join(HERE, "golden")]
import abi  # noqa: E402
import make_golden_abi_tok as tok_abi  # noqa: E402
import make_golden_wordpiece as gold  # noqa: E402
import wordpiece_ref as wr  # noqa: E402

from sessionsimilaritysearch_amd import _lib, wordpiece as wp  # noqa: E402

ROOT = os.path.dirname(HERE)
HEADER = "sss_wordpiece.h"
NAME = "sss_wordpiece_encode"


@pytest.fixture(scope="module")
def fixture():
    z = gold.load_cases()
    z["vocab_ids"] = {t: i for i, t in enumerate(z["vocab"])}
    return z


# ------------------------------------------------------------------------------------------------ the definition
def test_the_restatement_equals_the_recorded_bert_tokenizer_on_every_row(fixture):
    """Exact on every row of every case: no row is left out."""
    names = []
    for case in fixture["cases"]:
        assert case["T"] == 20 and len(case["strings"]) == len(case["ids"]) == len(case["n_tok"])
        for s, ids, n_tok in zip(case["strings"], case["ids"], case["n_tok"]):
            assert wr.encode(s, fixture["vocab_ids"], case["T"], **case["options"]) == (ids, n_tok), (case["name"], s)
        names.append(case["name"])
    assert names == ["default", "cased", "lower_keep_accents", "no_cjk_spaces"]
    opts = {c["name"]: c["options"] for c in fixture["cases"]}
    assert opts["cased"]["do_lower_case"] is False and opts["lower_keep_accents"] == dict(
        do_lower_case=True, tokenize_chinese_chars=True, strip_accents=False) and opts["no_cjk_spaces"]["tokenize_chinese_chars"] is False
    assert sum(len(c["strings"]) for c in fixture["cases"]) >= 3000


def test_the_fixture_holds_the_cases_it_is_meant_to(fixture):
    default = fixture["cases"][0]
    strings = default["strings"]
    for s in wr.edge_strings(default["T"]):
        assert s in strings
    unk = fixture["vocab_ids"]["[UNK]"]
    n_tok = default["n_tok"]
    assert {2, 17, 18, 19, 20} <= set(n_tok)                            # empty, and around the truncation point
    assert any(unk in r for r in default["ids"]) and any(unk not in r and k > 2 for r, k in zip(default["ids"], n_tok))
    with open(gold.DIFF) as f:
        d = json.load(f)
    banned = set(d["normalisation"]) | set(d["splitting"])
    for case in fixture["cases"]:
        for s in case["strings"]:
            assert not banned & set(map(ord, s)) and not any(sp.lower() in s.lower() for sp in wr.SPECIALS)


def test_the_code_point_sweep_equals_the_recorded_difference_list():
    """All 1 112 064 scalar values through the installed BertNormalizer and BertPreTokenizer: the code points where the
    restatement's map or its word splitting differs are exactly the recorded ones (categories that differ between this
    Python's Unicode tables and the tokenizers crate's)."""
    pytest.importorskip("tokenizers", reason="the sweep compares against the installed tokenizers package")
    with open(gold.DIFF) as f:
        d = json.load(f)
    union = sorted(set(d["normalisation"]) | set(d["splitting"]))
    assert len(union) <= 600 and min(union) >= 0x700 and not any(0x4E00 <= c <= 0x9FFF for c in union)
    norm, split = gold.sweep()
    print(f"{len(norm)} normalisation + {len(split)} splitting differences, {len(set(norm) | set(split))} code points")
    assert norm == d["normalisation"] and split == d["splitting"]


def test_pinned_divergences_from_hf(fixture):
    vocab = fixture["vocab_ids"]
    t = wp.WordPieceTokenizer(vocab)
    ids, n = wr.encode("[SEP] a", vocab, 20)
    assert wr.words("[SEP] a") == ["[", "sep", "]", "a"]
    assert ids[1] == vocab["["] and ids[n - 3] == vocab["]"] and ids[n - 2] == vocab["a"] and ids[n - 1] == vocab["[SEP]"]
    assert n >= 6 and vocab["[SEP]"] not in ids[:n - 1]                 # (HF gives [CLS] [SEP] a [SEP]: n = 4)
    assert t.host_encode("[SEP] a", 20) == (ids, n)
    for kw in (dict(padding=True), dict(padding="longest"), dict(padding=False), dict(truncation=False),
               dict(truncation="only_first"), dict(max_length=1), dict(max_length=65), dict(max_length=20.0)):
        with pytest.raises(ValueError):
            t(["a"], **kw)                                              # (raised before any device is touched)
    with pytest.raises(ValueError, match="pairs"):
        t([("a", "b")])


def test_bad_vocabularies_raise(tmp_path):
    ok = ["[PAD]", "[UNK]", "[CLS]", "[SEP]", "a", "##a"]
    assert wp.WordPieceTokenizer(ok).vocab == {t: i for i, t in enumerate(ok)}
    assert wp.WordPieceTokenizer({t: i for i, t in enumerate(ok)}).tokens == ok
    path = tmp_path / "vocab.txt"
    path.write_text("\n".join(ok) + "\n", encoding="utf-8")
    assert wp.WordPieceTokenizer(str(path)).tokens == ok
    with pytest.raises(ValueError, match="twice"):
        wp.WordPieceTokenizer(ok + ["a"])
    with pytest.raises(ValueError, match="0 .. V - 1"):
        wp.WordPieceTokenizer({**{t: i for i, t in enumerate(ok)}, "b": 7})
    with pytest.raises(ValueError, match="0 .. V - 1"):
        wp.WordPieceTokenizer({**{t: i for i, t in enumerate(ok)}, "b": 5})
    for missing in ("[PAD]", "[UNK]", "[CLS]", "[SEP]"):
        with pytest.raises(ValueError, match="not in the vocabulary"):
            wp.WordPieceTokenizer([t for t in ok if t != missing])
    for slots in (6, 7, 12, 4):                                         # not a power of two, or not above V
        with pytest.raises(ValueError, match="table_slots"):
            wp.WordPieceTokenizer(ok, table_slots=slots)
    assert wp.WordPieceTokenizer(ok, table_slots=8).table_slots == 8 and wp.WordPieceTokenizer(ok).table_slots == 16


def test_from_transformers_reads_vocabulary_and_options(fixture):
    transformers = pytest.importorskip("transformers", reason="from_transformers reads a live HF tokenizer")
    for case in fixture["cases"]:
        hf = transformers.BertTokenizer(vocab=fixture["vocab_ids"], **case["options"])
        t = wp.WordPieceTokenizer.from_transformers(hf)
        lower, strip, cjk = wr.resolve(**case["options"])
        assert (t.do_lower_case, t.strip_accents, t.tokenize_chinese_chars) == (lower, strip, cjk) and t.vocab == fixture["vocab_ids"]
        assert (t.unk_id, t.cls_id, t.sep_id, t.pad_id) == tuple(fixture["vocab_ids"][s] for s in ("[UNK]", "[CLS]", "[SEP]", "[PAD]"))


# ------------------------------------------------------------------------------------------------ the tables
@pytest.mark.parametrize("options", [dict(), dict(do_lower_case=False), dict(strip_accents=False), dict(tokenize_chinese_chars=False)])
def test_character_map_pages_hold_the_definition(options):
    """Every code point read out of the paged tables (the kernel's decoding) equals the restatement; equal pages are shared."""
    lower, strip, cjk = wr.resolve(**options)
    cmap = wp.build_char_map(lower, strip, cjk)
    page_of, entry, ext = cmap
    assert page_of.shape == (wp.PAGES,) and page_of.dtype == entry.dtype == ext.dtype == np.int32
    n_pages = entry.shape[0] // 256
    assert entry.shape[0] == n_pages * 256 and set(page_of.tolist()) == set(range(n_pages)) and n_pages < 400
    assert len({tuple(entry[p * 256:(p + 1) * 256].tolist()) for p in range(n_pages)}) == n_pages      # no page stored twice
    assert page_of[0x4E] == page_of[0x9F] and page_of[0xE0] == page_of[0xF0000 >> 8]    # ideographs; private use: shared pages
    for cp in range(0x110000):
        want = [c | (cls << 24) for c, cls in wr.map_code_point(cp, lower, strip, cjk)]
        if wp.map_chars([cp], cmap) != want:
            raise AssertionError((hex(cp), wp.map_chars([cp], cmap), want))
        assert len(want) <= 3


def test_the_hash_table_finds_every_token_and_misses_every_absent_probe(fixture):
    tokens = fixture["vocab"]
    V = len(tokens)
    slots_n = wp.next_pow2(V + 1)
    assert slots_n > V and slots_n & (slots_n - 1) == 0 and slots_n // 2 <= V
    t = wp.WordPieceTokenizer(tokens, table_slots=slots_n)
    assert t.slots.shape == (slots_n, 2) and int((t.slots[:, 0] >= 0).sum()) == V and t.max_piece_len == 6
    for i, tok in enumerate(tokens):
        cont = tok.startswith("##") and len(tok) > 2
        assert t.lookup(tok[2:] if cont else tok, cont) == i, tok
        assert wp.key_hash(wp.piece_key(tok)) == int(np.uint32(t.slots[t.slots[:, 0] == i][0, 1]))
    vocab = fixture["vocab_ids"]
    rng = np.random.default_rng(5)
    misses = 0
    for _ in range(4000):
        w = "".join(rng.choice(list("abcdefghijzq한"), size=int(rng.integers(1, 8))))
        for cont in (False, True):
            want = vocab.get(("##" if cont else "") + w, -1)
            assert t.lookup(w, cont) == want
            misses += want < 0
    assert misses > 4000
    assert t.lookup("only") >= 0 and t.lookup("only", True) == -1 and t.lookup("cont") == -1 and t.lookup("cont", True) >= 0
    # the tight table and the default one encode alike (probe chains change no result)
    roomy = wp.WordPieceTokenizer(tokens)
    assert roomy.table_slots == wp.next_pow2(2 * V)
    for s in fixture["cases"][0]["strings"][:300] + wr.edge_strings(20):
        assert t.host_encode(s, 20) == roomy.host_encode(s, 20) == wr.encode(s, vocab, 20)
    # the header's hash, written out once more
    h = 2166136261
    for k in (ord("a") | wp.CONT, ord("b")):
        h = ((h ^ k) * 16777619) % 2 ** 32
    h ^= h >> 15
    h = h * 0x2C1B3C6D % 2 ** 32
    assert wp.key_hash(wp.piece_key("##ab")) == h ^ (h >> 12)


def test_the_host_walk_of_the_tables_equals_the_fixture(fixture):
    for case in fixture["cases"]:
        t = wp.WordPieceTokenizer(fixture["vocab"], **case["options"])
        for s, ids, n_tok in zip(case["strings"], case["ids"], case["n_tok"]):
            assert t.host_encode(s, case["T"]) == (ids, n_tok), (case["name"], s)


# ------------------------------------------------------------------------------------------------ ABI and rejections
def test_tok_header_is_declared_bound_and_equals_its_snapshot():
    assert abi.declared(os.path.join("tok", HEADER)) == sorted(_lib.TOK_HEADERS[HEADER]) == [NAME]
    assert sorted(_lib.TOK_HEADERS) == sorted(f for f in os.listdir(os.path.join(ROOT, "include", "tok")) if f.endswith(".h")) == [HEADER]
    with open(tok_abi.SNAPSHOT) as f:
        snap = json.load(f)
    assert tok_abi.record(_lib) == snap
    fn = getattr(_lib.lib(), NAME)
    assert tok_abi.signature(fn.restype, fn.argtypes) == snap["functions"][HEADER][NAME]
    assert NAME not in _lib.exported_symbols() and len(_lib.exported_symbols()) == 60
    text = open(os.path.join(ROOT, "include", "tok", HEADER)).read()
    for words in ("CALLER-OWNED DEVICE", "2166136261", "16777619", "0x2C1B3C6D", "THE SCORE OF RECORD", "a hash collision costs a probe"):
        assert words in text, words
    assert (wp.PAGES, wp.CONT, wp.MAX_T, wp.ERR_CODEPOINT, wp.ERR_LENGTH, wp.MAX_CHARS) == (4352, 1 << 21, 64, 1, 2, 1024)


def test_the_five_binding_tables_are_disjoint_and_the_older_four_unchanged():
    tables = [_lib.PARAMS, _lib.EXT_PARAMS, _lib.LOWP_PARAMS, _lib.HEADS_PARAMS, _lib.TOK_PARAMS]
    names = [n for t in tables for n in t]
    assert len(names) == len(set(names))
    assert len(_lib.HEADERS) == 12 and len(_lib.PARAMS) == 98
    assert sorted(_lib.EXT_HEADERS) == ["sss_seqsim.h"] and sorted(_lib.LOWP_HEADERS) == ["sss_linear_bf16.h"]
    assert sorted(_lib.HEADS_HEADERS) == ["sss_catalogue.h"] and sorted(_lib.TOK_PARAMS) == [NAME]
    for maker, table in (("make_golden_abi_ext", "abi_signatures_ext.json"), ("make_golden_abi_lowp", "abi_signatures_lowp.json"),
                         ("make_golden_abi_heads", "abi_signatures_heads.json")):
        mod = __import__(maker)
        with open(os.path.join(ROOT, "tests", "golden", table)) as f:
            assert mod.record(_lib) == json.load(f)


_P = 1 << 20                                                          # a non-null, aligned address; never dereferenced


def _encode(**kw):
    a = dict(str_ptr=_P, str_chars=_P, n=5, n_chars=100, map_page=_P, map_entry=_P, n_pages=150, map_ext=_P, n_ext=10, slots=_P,
             table_slots=8192, piece_ptr=_P, piece_chars=_P, vocab_size=3000, max_piece_len=6, max_word_chars=100, unk_id=1, cls_id=2,
             sep_id=3, pad_id=0, T=20, ids=_P, n_tok=_P, err=_P, stream=0)
    a.update(kw)
    L = _lib.lib()
    return getattr(L, NAME)(*[a[p] for p in _lib.TOK_PARAMS[NAME]]), L.sss_last_error() or b""


def test_arguments_are_rejected_before_any_launch():
    """No address given here is memory: a call that launched would fault.  Every rejection names what is wrong."""
    for kw, words in ((dict(n=-1), b"0 <= n"), (dict(n=1 << 31), b"0 <= n"), (dict(n_chars=-1), b"n_chars"),
                      (dict(T=1), b"2 <= T <= 64"), (dict(T=65), b"2 <= T <= 64"), (dict(T=0), b"2 <= T <= 64"),
                      (dict(n_pages=0), b"n_pages"), (dict(n_pages=4353), b"n_pages"), (dict(n_ext=-1), b"n_ext"),
                      (dict(n_ext=1 << 24), b"n_ext"),
                      (dict(table_slots=8191), b"power of two"), (dict(table_slots=2048), b"power of two"),
                      (dict(table_slots=4096, vocab_size=4096), b"power of two"), (dict(table_slots=1 << 31), b"power of two"),
                      (dict(vocab_size=0), b"vocab_size"), (dict(max_piece_len=0), b"max_piece_len"),
                      (dict(max_word_chars=0), b"max_word_chars"),
                      (dict(unk_id=-1), b"special id"), (dict(cls_id=3000), b"special id"), (dict(sep_id=-5), b"special id"),
                      (dict(pad_id=1 << 20), b"special id"),
                      *[(dict([(p, 0)]), b"null") for p in ("str_ptr", "str_chars", "map_page", "map_entry", "map_ext", "slots",
                                                            "piece_ptr", "piece_chars", "ids", "n_tok", "err")],
                      (dict(slots=_P + 4), b"aligned")):
        rc, msg = _encode(**kw)
        assert rc == -1 and msg.startswith(b"wordpiece_encode:") and words in msg, (kw, rc, msg)
    assert _encode(n=0)[0] == 0                                         # an empty table touches nothing
    assert _encode(n=0, T=1)[0] == -1                                   # but its shapes are still checked


def test_the_package_exports_the_tokenizer():
    import sessionsimilaritysearch_amd as pkg
    for name in ("WordPieceTokenizer", "TokenTable", "Tokens"):
        assert getattr(pkg, name) is getattr(wp, name) and name in pkg.__all__
    t = wp.Tokens(1, 2, 3)
    assert t["input_ids"] == t[0] == t.input_ids == 1 and t["attention_mask"] == 3 and dict(**t) == t._asdict()
