"""Writes tests/golden/wordpiece_cases.json (with wordpiece_cases.npz) and tests/golden/wordpiece_charmap_diff.json from the installed Hugging Face
BERT tokenizer:
    python tests/golden/make_golden_wordpiece.py

wordpiece_cases.json + wordpiece_cases.npz: a vocabulary (tests/wordpiece_ref.py: ``make_vocab``), and per case the
tokenizer's options, ``T``, the input strings and what ``BertTokenizer(vocab=..., **options)(strings, padding='max_length',
max_length=T, truncation=True)`` returned: ``ids`` (the rows of ``input_ids``) and ``n_tok`` (the number of ones of each
``attention_mask`` row; the generator asserts that every mask is that many ones followed by zeros and that
``token_type_ids`` is all zero, so nothing is lost).  The .json holds the versions and, per case, its name, options, ``T``
and row count; the bulk lies beside it in the compressed .npz, cases concatenated in the .json's order -- ``chars`` /
``ptr`` (the input strings as code points, string ``u`` being ``chars[ptr[u]:ptr[u + 1]]``), ``ids`` int16 [rows, T],
``n_tok`` int8 [rows], ``vocab_chars`` / ``vocab_ptr`` (the tokens in id order, the same way).  ``load_cases()`` puts the two
back together.  The inputs are random strings over ``wordpiece_ref.ALPHABET`` and ``wordpiece_ref.edge_strings``.  The
generator asserts that no input holds the text of a special token or a code point of the difference list, so the tests
compare EVERY row with no exception.

wordpiece_charmap_diff.json: the code points at which the restatement's character map or word splitting differs from
``BertNormalizer.normalize_str`` / ``BertPreTokenizer.pre_tokenize_str`` (``sweep`` below, all 1 112 064 scalar values under
the default options).  They are code points whose Unicode category this Python's tables and the ones the tokenizers crate
carries disagree on.  tests/test_wordpiece_cpu.py re-runs the sweep and holds it to the file.
"""
import json
import os
import random
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE)]

import wordpiece_ref as wr  # noqa: E402

CASES = os.path.join(HERE, "wordpiece_cases.json")
CASES_NPZ = os.path.join(HERE, "wordpiece_cases.npz")
DIFF = os.path.join(HERE, "wordpiece_charmap_diff.json")
T = 20
# name -> (the options, random strings, edge strings?)
OPTION_SETS = {"default": (dict(do_lower_case=True, tokenize_chinese_chars=True, strip_accents=None), 2000, True),
               "cased": (dict(do_lower_case=False, tokenize_chinese_chars=True, strip_accents=None), 400, False),
               "lower_keep_accents": (dict(do_lower_case=True, tokenize_chinese_chars=True, strip_accents=False), 400, False),
               "no_cjk_spaces": (dict(do_lower_case=True, tokenize_chinese_chars=False, strip_accents=None), 400, False)}


def _pack(strings):
    """``(chars int32, ptr int64)`` of a list of str."""
    import numpy as np
    ptr = np.zeros(len(strings) + 1, np.int64)
    np.cumsum([len(s) for s in strings], out=ptr[1:])
    return np.frombuffer("".join(strings).encode("utf-32-le", "surrogatepass"), dtype="<i4").astype(np.int32), ptr


def _unpack(chars, ptr):
    text = chars.astype("<i4").tobytes().decode("utf-32-le", "surrogatepass")
    return [text[int(a):int(b)] for a, b in zip(ptr[:-1], ptr[1:])]


def load_cases():
    """The fixture as one dict: ``vocab`` (tokens in id order), the versions, and ``cases``: per case ``name``, ``options``,
    ``T``, ``strings``, ``ids`` (lists of ``T`` ints) and ``n_tok``."""
    import numpy as np
    with open(CASES) as f:
        z = json.load(f)
    with np.load(CASES_NPZ) as a:
        strings, ids, n_tok = _unpack(a["chars"], a["ptr"]), a["ids"].astype(np.int64).tolist(), a["n_tok"].astype(np.int64).tolist()
        z["vocab"] = _unpack(a["vocab_chars"], a["vocab_ptr"])
    at = 0
    for case in z["cases"]:
        rows = case.pop("rows")
        case.update(strings=strings[at:at + rows], ids=ids[at:at + rows], n_tok=n_tok[at:at + rows])
        assert len(case["strings"]) == rows and all(len(r) == case["T"] for r in case["ids"])
        at += rows
    assert at == len(strings) == len(ids) == len(n_tok)
    return z


def sweep():
    """``(normalisation differences, word-splitting differences)``: sorted code points, under the default options.  The
    splitting is compared on the restatement's own mapped text between two letters, so it isolates the classes."""
    from tokenizers.normalizers import BertNormalizer
    from tokenizers.pre_tokenizers import BertPreTokenizer
    nz = BertNormalizer(clean_text=True, handle_chinese_chars=True, strip_accents=True, lowercase=True)
    pre = BertPreTokenizer()
    norm, split = [], []
    for cp in range(0x110000):
        if 0xD800 <= cp <= 0xDFFF:
            continue
        ch = chr(cp)
        mine = wr.normalize(ch)
        if nz.normalize_str(ch) != mine:
            norm.append(cp)
        text = "a" + mine + "b"
        if [w for w, _ in pre.pre_tokenize_str(text)] != wr.words(text, False, False, False):
            split.append(cp)
    return norm, split


def main():
    import tokenizers
    import transformers
    from transformers import BertTokenizer
    norm, split = sweep()
    diff = sorted(set(norm) | set(split))
    with open(DIFF, "w") as f:
        json.dump({"unidata_version": __import__("unicodedata").unidata_version, "tokenizers": tokenizers.__version__,
                   "normalisation": norm, "splitting": split}, f, separators=(",", ":"))
        f.write("\n")
    print(f"{len(norm)} normalisation and {len(split)} splitting differences, {len(diff)} code points, lowest U+{diff[0]:04X}")
    rng = random.Random(7)
    tokens = wr.make_vocab(rng)
    vocab = {t: i for i, t in enumerate(tokens)}
    banned = set(diff)
    cases = []
    for name, (options, n_random, edges) in OPTION_SETS.items():
        strings = wr.random_strings(rng, n_random) + (wr.edge_strings(T) if edges else [])
        for s in strings:
            assert not any(sp.lower() in s.lower() for sp in wr.SPECIALS), s
            assert not banned & set(map(ord, s)), s
        hf = BertTokenizer(vocab=vocab, **options)
        assert hf.get_vocab() == vocab
        out = hf(strings, padding="max_length", max_length=T, truncation=True)
        n_tok = [sum(m) for m in out["attention_mask"]]
        assert all(m == [1] * k + [0] * (T - k) for m, k in zip(out["attention_mask"], n_tok))
        assert all(not any(t) for t in out["token_type_ids"])
        cases.append({"name": name, "options": options, "T": T, "strings": strings, "ids": out["input_ids"], "n_tok": n_tok})
        print(name, len(strings), "strings, mean tokens", sum(n_tok) / len(n_tok), "[UNK] share",
              sum(r.count(vocab["[UNK]"]) for r in out["input_ids"]) / sum(n_tok))
    import numpy as np
    chars, ptr = _pack([s for c in cases for s in c["strings"]])
    vocab_chars, vocab_ptr = _pack(tokens)
    np.savez_compressed(CASES_NPZ, chars=chars, ptr=ptr, vocab_chars=vocab_chars, vocab_ptr=vocab_ptr,
                        ids=np.asarray([r for c in cases for r in c["ids"]], np.int16),
                        n_tok=np.asarray([k for c in cases for k in c["n_tok"]], np.int8))
    with open(CASES, "w") as f:
        json.dump({"transformers": transformers.__version__, "tokenizers": tokenizers.__version__, "data": os.path.basename(CASES_NPZ),
                   "cases": [{"name": c["name"], "options": c["options"], "T": c["T"], "rows": len(c["strings"])} for c in cases]},
                  f, indent=1)
        f.write("\n")
    back = load_cases()
    assert back["vocab"] == tokens and [(c["strings"], c["ids"], c["n_tok"]) for c in back["cases"]] == \
        [(c["strings"], c["ids"], c["n_tok"]) for c in cases]
    print("wrote", CASES, os.path.getsize(CASES), "bytes,", CASES_NPZ, os.path.getsize(CASES_NPZ), "bytes and", DIFF, os.path.getsize(DIFF), "bytes")


if __name__ == "__main__":
    main()
