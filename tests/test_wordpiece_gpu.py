"""GPU side of the WordPiece tokenizer: sss_wordpiece_encode through wordpiece.WordPieceTokenizer against the plain-Python
restatement (tests/wordpiece_ref.py) bit for bit -- ids, n_tok and the mask -- on the fixture's random strings and on the
shapes the kernel can go wrong at (wordpiece_ref.edge_strings), at T = 2, 3, 8, 20, 64, with the default table and the
tightest one; against the recorded Hugging Face rows under the other option sets; the error word; and the wiring into the
graph builder's string ids and BertNodeEncoder."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [HERE, os.path.join(HERE, "helpers"), os.path.join(HERE, "golden")]
import bert_ref as br  # noqa: E402
import make_golden_wordpiece as gold  # noqa: E402
import wordpiece_ref as wr  # noqa: E402

from sessionsimilaritysearch_amd import wordpiece as wp  # noqa: E402
from sessionsimilaritysearch_amd.strings import StringTable  # noqa: E402

pytestmark = pytest.mark.gpu
_CACHE = {}


def fixture():
    if "fixture" not in _CACHE:
        z = gold.load_cases()
        z["vocab_ids"] = {t: i for i, t in enumerate(z["vocab"])}
        _CACHE["fixture"] = z
    return _CACHE["fixture"]


def tokenizer(name="default", **kw):
    """One tokenizer per option set and table size, built once."""
    key = ("tok", name, tuple(sorted(kw.items())))
    if key not in _CACHE:
        z = fixture()
        options = next(c["options"] for c in z["cases"] if c["name"] == name)
        _CACHE[key] = wp.WordPieceTokenizer(z["vocab"], **options, **kw)
    return _CACHE[key]


def inputs(T):
    """The fixture's random strings and the edge strings for ``T`` -- a count that is no multiple of the four strings of a
    workgroup -- with the restatement's rows, computed once."""
    if ("inputs", T) not in _CACHE:
        z = fixture()
        strings = z["cases"][0]["strings"][:2000] + wr.edge_strings(T)
        if len(strings) % 4 == 0:
            strings.append("ab")
        ids, n_tok = wr.encode_batch(strings, z["vocab_ids"], T)
        _CACHE[("inputs", T)] = (strings, np.asarray(ids, np.int64), np.asarray(n_tok, np.int64))
    return _CACHE[("inputs", T)]


def run(tok, strings, T, cuda):
    table = strings if isinstance(strings, StringTable) else StringTable(strings, cuda)
    ids, n_tok, err = tok.encode_device(table, T)
    assert ids.dtype == n_tok.dtype == err.dtype == torch.int32 and ids.shape == (len(table), T) and n_tok.shape == (len(table),)
    return ids.cpu().numpy().astype(np.int64), n_tok.cpu().numpy().astype(np.int64), int(err.item())


def same(got, want, strings):
    bad = np.flatnonzero((got[0] != want[0]).any(1) | (got[1] != want[1]))
    assert bad.size == 0, (len(bad), repr(strings[bad[0]][:60]), got[0][bad[0]].tolist(), want[0][bad[0]].tolist())


@pytest.mark.parametrize("T", [2, 3, 8, 20, 64])
def test_device_equals_the_restatement(cuda, T):
    strings, ids, n_tok = inputs(T)
    assert len(strings) % 4 and len(strings) > 2000
    got = run(tokenizer(), strings, T, cuda)
    assert got[2] == 0
    same(got, (ids, n_tok), strings)
    # the public call: int64, the mask out of n_tok, all-zero types; readable by name
    tokens = tokenizer()(strings[:301], max_length=T)
    assert all(t.dtype == torch.int64 and t.shape == (301, T) and t.device.type == "cuda" for t in tokens)
    assert np.array_equal(tokens["input_ids"].cpu().numpy(), ids[:301])
    assert tokens.attention_mask.cpu().numpy().tolist() == wr.mask_of(n_tok[:301].tolist(), T)
    assert not tokens.token_type_ids.any()
    # one string
    one = run(tokenizer(), [strings[7]], T, cuda)
    same(one, (ids[7:8], n_tok[7:8]), strings[7:8])


def test_the_tightest_table_gives_the_same_rows(cuda):
    """table_slots = next_pow2(V + 1): the longest probe chains a legal table has."""
    strings, ids, n_tok = inputs(20)
    V = len(fixture()["vocab"])
    tight = tokenizer(table_slots=wp.next_pow2(V + 1))
    assert tight.table_slots == 4096 and tight.table_slots // 2 <= V < tight.table_slots and tokenizer().table_slots == 8192
    same(run(tight, strings, 20, cuda), (ids, n_tok), strings)


@pytest.mark.parametrize("name", ["default", "cased", "lower_keep_accents", "no_cjk_spaces"])
def test_device_equals_the_recorded_bert_tokenizer(cuda, name):
    case = next(c for c in fixture()["cases"] if c["name"] == name)
    got = run(tokenizer(name), case["strings"], case["T"], cuda)
    assert got[2] == 0
    same(got, (np.asarray(case["ids"], np.int64), np.asarray(case["n_tok"], np.int64)), case["strings"])


def test_bad_code_points_and_lengths_set_the_error_word_and_nothing_else(cuda):
    strings, ids, n_tok = inputs(20)
    strings, ids, n_tok = strings[:203], ids[:203].copy(), n_tok[:203].copy()
    tok, vocab = tokenizer(), fixture()["vocab_ids"]
    empty = [vocab["[CLS]"], vocab["[SEP]"]] + [vocab["[PAD]"]] * 18
    table = StringTable(strings, cuda)
    ptr = table.ptr.cpu().numpy()
    rows = [r for r in range(203) if ptr[r + 1] - ptr[r] >= 3 and n_tok[r] > 2][:2]
    table.chars[int(ptr[rows[0]]) + 1] = -1
    table.chars[int(ptr[rows[1] + 1]) - 1] = 0x110000
    got = run(tok, table, 20, cuda)
    assert got[2] == wp.ERR_CODEPOINT
    for r in rows:
        ids[r], n_tok[r] = empty, 2
    same(got, (ids, n_tok), strings)
    with pytest.raises(wp._lib.SssError, match="code point"):
        tok.encode_table(table)
    table.chars[int(ptr[rows[0]]) + 1] = 0x10FFFF                       # the last scalar value: legal (unassigned, "other")
    table.chars[int(ptr[rows[1] + 1]) - 1] = 0
    assert run(tok, table, 20, cuda)[2] == 0
    # a row of more than 1024 code points (made by moving a row boundary): bit 1, and only that row
    long_table = StringTable(["b" * 1000, "x" * 1000, "only"], cuda)
    long_table.ptr[1] = 1030
    got = run(tok, long_table, 20, cuda)
    want = wr.encode_batch(["", "x" * 970, "only"], vocab, 20)
    assert got[2] == wp.ERR_LENGTH
    same(got, (np.asarray(want[0]), np.asarray(want[1])), ["", "x" * 970, "only"])
    with pytest.raises(wp._lib.SssError, match="1024"):
        tok.encode_table(long_table)


def test_token_table_rows_wire_the_graph_builder_to_the_bert_encoder(cuda):
    """``encode_table`` + ``rows(batch['query'].x)`` equals tokenizing the gathered strings directly, and through a small
    BertNodeEncoder it gives the bits the encoder gives on the restatement's ids."""
    from sessionsimilaritysearch_amd import sessions as S
    from sessionsimilaritysearch_amd.text import BertNodeEncoder
    z, tok, T = fixture(), tokenizer(), 20
    strings = [""] + [s for s in z["cases"][0]["strings"][:400] if s][:128]            # id 0: the empty root query
    table = StringTable(strings, cuda)
    assert table.empty_id == 0
    tt = tok.encode_table(table, T)
    assert len(tt) == len(strings) and tt.max_length == T and tt.empty_id == 0
    batch = S.build_batch(S.synthetic_actions(40, 3, 500, len(strings)))
    x = np.asarray(batch["query"].x)
    assert x.size > 40 and (x == 0).any() and x.max() < len(strings)
    rows = tt.rows(torch.from_numpy(x).to(cuda))
    direct = tok([strings[i] for i in x], max_length=T)
    want_ids, want_n = wr.encode_batch([strings[i] for i in x], z["vocab_ids"], T)
    for a, b in zip(rows, direct):
        assert torch.equal(a, b)
    assert np.array_equal(rows.input_ids.cpu().numpy(), np.asarray(want_ids))
    assert rows.attention_mask.cpu().numpy().tolist() == wr.mask_of(want_n, T)
    assert torch.equal(tt.rows(x).input_ids, rows.input_ids)              # host ids are taken too
    with pytest.raises(IndexError):
        tt.rows([len(strings)])
    heads = 4
    w = br.seeded_weights(3, len(z["vocab"]), 64, heads, 128, 1, 32)
    enc = BertNodeEncoder(w, heads, device=cuda)
    out = enc(*rows)
    ref = enc(np.asarray(want_ids, np.int64), np.zeros((x.size, T), np.int64), np.asarray(wr.mask_of(want_n, T), np.int64))
    assert out.shape[0] == x.size and torch.equal(out, ref)
