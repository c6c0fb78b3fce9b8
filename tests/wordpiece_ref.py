"""The WordPiece score of record in plain Python: what ``sessionsimilaritysearch_amd.wordpiece`` and csrc/wordpiece.hip are held
to, bit for bit (tests/test_wordpiece_cpu.py, tests/test_wordpiece_gpu.py).  It restates include/tok/sss_wordpiece.h with
``unicodedata`` and a dict, shares no code with the package, and is itself held to a recorded run of the Hugging Face
``BertTokenizer`` (tests/golden/wordpiece_cases.json) and, code point by code point, to its normalizer and pre-tokenizer.

Single sentences only; ``padding='max_length'``, ``truncation=True``.  The literal text of a special token inside a string
is ordinary text here (``"[SEP] a"`` gives ``[ sep ] a``).
"""
import unicodedata

OTHER, SPACE, PUNCT = 0, 1, 2
# the ranges of HF's ``_is_chinese_char`` / ``is_chinese_char``
CJK = ((0x4E00, 0x9FFF), (0x3400, 0x4DBF), (0x20000, 0x2A6DF), (0x2A700, 0x2B73F), (0x2B740, 0x2B81F), (0x2B920, 0x2CEAF),
       (0xF900, 0xFAFF), (0x2F800, 0x2FA1F))


def is_cjk(cp):
    return any(lo <= cp <= hi for lo, hi in CJK)


def char_class(cp):
    """The class of one MAPPED code point."""
    if cp == 0x20:
        return SPACE
    if 33 <= cp <= 47 or 58 <= cp <= 64 or 91 <= cp <= 96 or 123 <= cp <= 126:
        return PUNCT
    cat = unicodedata.category(chr(cp))
    if cat in ("Zl", "Zp"):
        return SPACE
    return PUNCT if cat.startswith("P") else OTHER


def resolve(do_lower_case=True, tokenize_chinese_chars=True, strip_accents=None):
    """``(lower, strip, cjk)``: ``strip_accents=None`` follows ``do_lower_case``."""
    return bool(do_lower_case), bool(do_lower_case if strip_accents is None else strip_accents), bool(tokenize_chinese_chars)


def map_code_point(cp, lower, strip, cjk):
    """Step 1 for one input code point: the list of ``(mapped code point, class)`` it becomes (0 to 3 of them)."""
    ch = chr(cp)
    if cp in (0x09, 0x0A, 0x0D):
        return [(0x20, SPACE)]
    cat = unicodedata.category(ch)
    if cp == 0 or cp == 0xFFFD or cat in ("Cc", "Cf", "Co"):
        return []
    if cat in ("Zs", "Zl", "Zp"):                            # (HF's clean_text turns every white space into U+0020)
        return [(0x20, SPACE)]
    out = ch
    if strip:
        out = "".join(c for c in unicodedata.normalize("NFD", out) if unicodedata.category(c) != "Mn")
    if lower:
        out = "".join(c.lower() for c in out)
    res = [(ord(c), char_class(ord(c))) for c in out]
    if cjk and is_cjk(cp):
        res = [(0x20, SPACE)] + res + [(0x20, SPACE)]
    return res


def normalize(text, lower=True, strip=True, cjk=True):
    """The mapped text of a string (what HF's ``BertNormalizer.normalize_str`` gives)."""
    return "".join(chr(c) for cp in map(ord, text) for c, _ in map_code_point(cp, lower, strip, cjk))


def words(text, lower=True, strip=True, cjk=True):
    """Step 2: maximal runs of "other" characters; every punctuation character a word of its own."""
    out, cur = [], []
    for cp in map(ord, text):
        for c, cls in map_code_point(cp, lower, strip, cjk):
            if cls == OTHER:
                cur.append(chr(c))
                continue
            if cur:
                out.append("".join(cur))
                cur = []
            if cls == PUNCT:
                out.append(chr(c))
    if cur:
        out.append("".join(cur))
    return out


def wordpiece(word, vocab, unk_id, max_input_chars_per_word=100):
    """Step 3: the ids of one word -- greedy, longest piece first, ``##`` on continuation pieces; one ``unk_id`` for a word
    of more than ``max_input_chars_per_word`` characters or with a position no piece starts at."""
    if len(word) > max_input_chars_per_word:
        return [unk_id]
    ids, start = [], 0
    while start < len(word):
        end = len(word)
        while end > start:
            piece = ("##" if start else "") + word[start:end]
            if piece in vocab:
                break
            end -= 1
        if end == start:
            return [unk_id]
        ids.append(vocab[piece])
        start = end
    return ids


def encode(text, vocab, T, do_lower_case=True, tokenize_chinese_chars=True, strip_accents=None, unk_token="[UNK]",
           cls_token="[CLS]", sep_token="[SEP]", pad_token="[PAD]", max_input_chars_per_word=100):
    """Step 4: ``(ids, n_tok)`` -- ``[CLS]``, the first ``T - 2`` pieces, ``[SEP]``, ``[PAD]`` up to ``T``; ``n_tok`` counts
    the attended positions."""
    lower, strip, cjk = resolve(do_lower_case, tokenize_chinese_chars, strip_accents)
    pieces = []
    for w in words(text, lower, strip, cjk):
        if len(pieces) >= T - 2:
            break
        pieces += wordpiece(w, vocab, vocab[unk_token], max_input_chars_per_word)
    pieces = pieces[:max(T - 2, 0)]
    ids = [vocab[cls_token]] + pieces + [vocab[sep_token]]
    return ids + [vocab[pad_token]] * (T - len(ids)), len(ids)


def encode_batch(texts, vocab, T, **options):
    """``(ids [n][T], n_tok [n])`` as lists."""
    rows = [encode(t, vocab, T, **options) for t in texts]
    return [r[0] for r in rows], [r[1] for r in rows]


def mask_of(n_tok, T):
    return [[1] * n + [0] * (T - n) for n in n_tok]


# ------------------------------------------------------------------------------------------------ the shared test inputs
# The alphabet of the random strings: ASCII, punctuation, accents, the case-mapping oddities, Cyrillic, CJK, Hangul, an
# emoji, and the characters that vanish or turn into spaces.
ALPHABET = (list("abcdefghijklmnoprstuwyABCDEFRST") + [" "] * 5 + list(".,!-'()[]#") + list("éèüñçÅøßİıΣσςΩж") +
            list("世界語한글가") + ["\t", "\n", "\u00a0", "\u200b", "\x00", "\ufffd", "\u0301", "\u3000", "\U0001F600", "\u2028",
                             "\x85", "\x0b"])
# explicit vocabulary entries the edge strings rely on ("z" and "q" are in no piece)
EDGE_TOKENS = [".", "!", "x", "##x", "only", "##cont", "a", "##b", "##a", "ab", "##abab", "世", "界"]
SPECIALS = ["[PAD]", "[UNK]", "[CLS]", "[SEP]", "[MASK]"]


def make_vocab(rng, n_random=2600):
    """The test vocabulary, in id order: the special tokens, ``EDGE_TOKENS``, four fifths of the mapped alphabet as
    word-initial and (independently) as continuation pieces, and random pieces of 2 to 6 letters."""
    tokens, seen = [], set()

    def add(t):
        if t not in seen:
            seen.add(t)
            tokens.append(t)
    for t in SPECIALS + EDGE_TOKENS:
        add(t)
    text = "".join(ALPHABET)                                 # (mapped with and without lower-casing and accent stripping)
    mapped = sorted((set(normalize(text)) | set(normalize(text, False, False)) | set(normalize(text, True, False))) - set(" zq"))
    for c in mapped:
        for prefix in ("", "##"):
            if rng.random() < 0.8:
                add(prefix + c)
    for _ in range(n_random):
        w = "".join(rng.choice("abcdefghijklmnoprstuwyeusσж한") for _ in range(rng.randint(2, 6)))
        if "only" not in w and "cont" not in w:
            add(rng.choice(["", "##"]) + w)
    assert "cont" not in seen and "##only" not in seen and not any("z" in t or "q" in t for t in tokens)
    return tokens


def random_strings(rng, n, max_symbols=60):
    return ["".join(rng.choice(ALPHABET) for _ in range(rng.randint(0, max_symbols))) for _ in range(n)]


def edge_strings(T):
    """The shapes a tokenizer kernel can go wrong at, for an output width ``T`` (every string at most 1024 code points)."""
    hangul = "한"                                        # one syllable: three mapped characters (its jamo)
    out = ["", " ", "   \t\n ", " " * 1020 + "only",         # empty; only spaces; a full-length run of spaces, then a word
           "x" * 100, "x" * 101, "a " + "x" * 100 + " b", "a " + "x" * 101 + " b",   # the word-length limit, at and over
           hangul * 33, hangul * 34,                         # 99 and 102 mapped characters
           "abz", "ab abz ab", "xxxxz xx",                   # first pieces match, the last position does not: one [UNK]
           "only", "onlyonly", "xonly", "cont", "xcont", "contx",   # a piece only without "##", one only with it
           "!" * 63, "!" * 65, ". " * 63, hangul * 1024, "!" * 1024, ("x" * 99 + " ") * 10,
           "世界ab世x界", "ab世", "世ab", "\uf900a", "a\U0002f800b",   # CJK next to Latin; compatibility ideographs
           "[SEP", "a[b]c", "##x x##", "\u00e9\u0301e\u0301", "\u0130I\u0131i \u0391\u03a3 \u03b1\u03c2"]
    for k in (T - 3, T - 2, T - 1):                          # exactly T - 3, T - 2 and T - 1 pieces
        if k >= 0:
            out += ["." * k, ". " * k, "." * max(k - 1, 0) + " only", "." * max(k - 2, 0) + "ababx"]
    word = "ababababababab"
    for k in range(1, 17):                                   # a mapped length one short of, at and one past each 64-chunk
        for d in (-1, 0, 1):
            n = 64 * k + d
            if n <= 1024:
                s = ((word + " ") * 70)[:n]
                out.append(s)
    for k in (1, 8, 21):                                     # ... with three mapped characters per code point
        out += [hangul * k + " x", "x" + hangul * k, "世" * k + "x"]
    for vanishing in ("\x00", "\ufffd", "\u200b", "\u0301"):   # characters that vanish at a chunk's first and last lane
        s = list("ab x. " * 40)[:200]
        for at in (0, 63, 64, 127, 128, 199):
            s[at] = vanishing
        out.append("".join(s))
    return out
