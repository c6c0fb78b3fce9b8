"""Dev helper: the device WordPiece tokenizer (sessionsimilaritysearch_amd/wordpiece.py) against the installed Hugging Face
fast tokenizer on the host, over a synthetic vocabulary of 30 522 pieces and two kinds of strings at T = 20: ``--n``
query-like strings of 2-6 words and ``--n`` title-like strings of 8-30 words (default 1 000 000 each).  Both run in the
same job, alternating, ``--reps`` times; the host tokenizer gets ``--threads`` threads (RAYON_NUM_THREADS).  Prints one JSON
line, per kind:
  device_ms / device_strings_per_s   sss_wordpiece_encode alone over the whole table (hipEvent median after warm-up), and
                                     device_bytes_per_s: (the code points and offsets read + the ids and counts written) / time
  encode_table_wall_ms               WordPieceTokenizer.encode_table: the launch and the read-back of the error word
  hf_backend_ms / hf_backend_strings_per_s   tokenizers' encode_batch with truncation and padding enabled (the Rust thread pool alone)
  hf_call_ms / hf_call_strings_per_s         BertTokenizer(strings, padding='max_length', max_length=20, truncation=True,
                                             return_tensors='np'): the reference's call
  equals_hf                          the device rows of the first --check strings equal the host tokenizer's
The host-side cost of building the StringTable (and the tokenizer's tables) is reported once, as *_build_s."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def lexicon(rng, n):
    return ["".join(chr(97 + int(c)) for c in rng.integers(0, 26, int(rng.integers(2, 11)))) for _ in range(n)]


def vocabulary(rng, lex, size=30522):
    """Special tokens, every ASCII letter, digit and punctuation mark in both forms, the ``size // 4`` most frequent words
    of the lexicon whole, and random pieces of 2-6 letters (half of them continuation pieces) up to ``size``."""
    tokens, seen = [], set()

    def add(t):
        if t not in seen and len(tokens) < size:
            seen.add(t)
            tokens.append(t)
    for t in ("[PAD]", "[UNK]", "[CLS]", "[SEP]", "[MASK]"):
        add(t)
    for c in map(chr, range(33, 127)):
        if not c.isupper():
            add(c)
            add("##" + c)
    for w in lex[:size // 4]:
        add(w)
    while len(tokens) < size:
        w = "".join(chr(97 + int(c)) for c in rng.integers(0, 26, int(rng.integers(2, 7))))
        add(w if rng.random() < 0.5 else "##" + w)
    return tokens


def sentences(rng, lex, n, lo, hi):
    """``n`` strings of ``lo`` to ``hi`` words, words drawn Zipf-like from the lexicon, one in twelve capitalised, one in
    fifteen followed by a comma."""
    import numpy as np
    counts = rng.integers(lo, hi + 1, n)
    picks = np.minimum(rng.zipf(1.3, int(counts.sum())) - 1, len(lex) - 1)
    style = rng.integers(0, 60, picks.shape[0])
    words = [lex[p].capitalize() if s % 12 == 0 else lex[p] + "," if s % 15 == 1 else lex[p] for p, s in zip(picks.tolist(), style.tolist())]
    out, at = [], 0
    for c in counts.tolist():
        out.append(" ".join(words[at:at + c]))
        at += c
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1000000, help="strings of each kind")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--check", type=int, default=20000)
    ap.add_argument("--max-length", type=int, default=20)
    a = ap.parse_args()
    os.environ["RAYON_NUM_THREADS"] = str(a.threads)
    os.environ["TOKENIZERS_PARALLELISM"] = "true"
    import numpy as np
    import torch
    from transformers import BertTokenizer

    from sessionsimilaritysearch_amd import _lib
    from sessionsimilaritysearch_amd.strings import StringTable
    from sessionsimilaritysearch_amd.wordpiece import WordPieceTokenizer

    dev, T = torch.device("cuda", 0), a.max_length
    rng = np.random.default_rng(11)
    lex = lexicon(rng, 60000)
    tokens = vocabulary(rng, lex)
    t0 = time.perf_counter()
    tok = WordPieceTokenizer(tokens)
    out = {"n": a.n, "T": T, "reps": a.reps, "threads": a.threads, "vocab": len(tokens), "table_slots": tok.table_slots,
           "max_piece_len": tok.max_piece_len, "tokenizer_build_s": time.perf_counter() - t0}
    hf = BertTokenizer(vocab={t: i for i, t in enumerate(tokens)}, do_lower_case=True)
    backend = hf.backend_tokenizer
    backend.enable_truncation(max_length=T)
    backend.enable_padding(length=T, pad_id=tok.pad_id, pad_token="[PAD]")
    kinds = {"query": sentences(rng, lex, a.n, 2, 6), "title": sentences(rng, lex, a.n, 8, 30)}
    for kind, strings in kinds.items():
        t0 = time.perf_counter()
        table = StringTable(strings, dev)
        torch.cuda.synchronize()
        r = {"string_table_build_s": time.perf_counter() - t0, "chars": int(table.chars.numel()),
             "mean_chars": float(table.lengths.mean())}
        tok.encode_table(table, T)                                      # warm-up: uploads the tables
        dev_ms, wall_ms, backend_ms, call_ms = [], [], [], []
        for _ in range(a.reps):                                         # alternating: device, host, device, host, ...
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            ids, n_tok, err = tok.encode_device(table, T)
            e1.record()
            e1.synchronize()
            dev_ms.append(e0.elapsed_time(e1))
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            tt = tok.encode_table(table, T)
            torch.cuda.synchronize()
            wall_ms.append((time.perf_counter() - t0) * 1e3)
            t0 = time.perf_counter()
            enc = backend.encode_batch(strings)
            backend_ms.append((time.perf_counter() - t0) * 1e3)
            t0 = time.perf_counter()
            called = hf(strings, padding="max_length", max_length=T, truncation=True, return_tensors="np")
            call_ms.append((time.perf_counter() - t0) * 1e3)
            print(f"{kind}: device {dev_ms[-1]:.2f} ms, hf backend {backend_ms[-1]:.0f} ms, hf call {call_ms[-1]:.0f} ms",
                  file=sys.stderr, flush=True)
        moved = 4 * r["chars"] + 8 * (a.n + 1) + 4 * a.n * T + 4 * a.n
        d = float(np.median(dev_ms))
        r.update(device_ms=d, device_strings_per_s=a.n / (d * 1e-3), device_bytes_per_s=moved / (d * 1e-3),
                 encode_table_wall_ms=float(np.median(wall_ms)), hf_backend_ms=float(np.median(backend_ms)),
                 hf_backend_strings_per_s=a.n / (float(np.median(backend_ms)) * 1e-3), hf_call_ms=float(np.median(call_ms)),
                 hf_call_strings_per_s=a.n / (float(np.median(call_ms)) * 1e-3),
                 mean_tokens=float(tt.n_tok.double().mean().item()),
                 unk_share=float((tt.ids == tok.unk_id).sum().item() / tt.n_tok.sum().item()))
        k = min(a.check, a.n)
        got = tt.ids[:k].cpu().numpy()
        r["equals_hf"] = bool(np.array_equal(got, called["input_ids"][:k]) and
                              np.array_equal(got, np.asarray([e.ids for e in enc[:k]])) and
                              np.array_equal(tt.n_tok[:k].cpu().numpy(), called["attention_mask"][:k].sum(1)))
        out[kind] = r
        del table, enc, called, tt, ids
    print(json.dumps(out))
    if not all(out[k]["equals_hf"] for k in kinds):
        raise SystemExit("the device rows differ from the host tokenizer's")


if __name__ == "__main__":
    main()
