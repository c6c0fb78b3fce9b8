"""Dev helper: the string metrics of a search result (sessionsimilaritysearch_amd/strings.py) at nq = 1024, K = 100 over
synthetic sessions: query strings of 2-4 words, item titles of 5-30 words of which about 40 % are near-duplicates of
another title (one to three words changed), I seeded random ids.  Prints one JSON line, per kind ("query": the query
strings of a session; "title": its item titles):
  pair_scores_ms            sss_seq_pair_scores alone (hipEvent median after warm-up), with session pairs_per_s and
                            string_pairs_per_s (string pairs = sum of len(Q_i) * len(C_r): what the kernel computes an
                            edit distance for, equal ids included)
  query_metric_ms           sss_seq_query_metric on its outputs
  drop_in_wall_ms           get_ave_score of the kind (the launch, the float32 rounding, the mean; wall clock around a
                            synchronise, median)
  host_restatement_ms       tests/helpers/seqsim_ref.pair_scores (plain Python, the score of record) on the first
                            --host-queries queries x --host-k neighbours, scaled to the batch; host_pairs_timed says how
                            many session pairs were timed"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import seqsim_ref  # noqa: E402
from sessionsimilaritysearch_amd import _lib, evaluation, strings  # noqa: E402
from sessionsimilaritysearch_amd.sessions import ActionTable, synthetic_actions  # noqa: E402


def event_median_ms(fn, warmup, reps):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); fn(); b.record(); b.synchronize()
        ts.append(a.elapsed_time(b))
    return float(np.median(ts))


def words(rng, n):
    return ["".join(chr(97 + int(c)) for c in rng.integers(0, 26, int(rng.integers(2, 10)))) for _ in range(n)]


def vocabulary(rng, n_query, n_title):
    """``n_query`` query strings of 2-4 words, then ``n_title`` titles of 5-30 words, about 40 % of them another title
    with one to three words replaced."""
    lex = words(rng, 3000)
    pick = lambda k: [lex[int(w)] for w in rng.integers(0, len(lex), k)]
    out = [" ".join(pick(int(rng.integers(2, 5)))) for _ in range(n_query)]
    titles = []
    for _ in range(n_title):
        if titles and rng.random() < 0.4:
            t = list(titles[int(rng.integers(0, len(titles)))])
            for _ in range(int(rng.integers(1, 4))):
                t[int(rng.integers(0, len(t)))] = pick(1)[0]
        else:
            t = pick(int(rng.integers(5, 31)))
        titles.append(t)
    return out + [" ".join(t) for t in titles]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=100000)
    ap.add_argument("--nq", type=int, default=1024)
    ap.add_argument("--k", type=int, default=100)
    ap.add_argument("--queries", type=int, default=4096, help="distinct query strings")
    ap.add_argument("--titles", type=int, default=20000, help="distinct item titles")
    ap.add_argument("--host-queries", type=int, default=4)
    ap.add_argument("--host-k", type=int, default=10)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(5)
    vocab = vocabulary(rng, a.queries, a.titles)
    table = strings.StringTable(vocab, dev)
    item_title = (a.queries + np.arange(a.titles)).astype(np.int64)              # item i carries title i
    corpus_actions = synthetic_actions(a.n, 1, a.titles + 1, a.queries + 1)      # ids clipped below into both vocabularies
    seq, tar = synthetic_actions(a.nq, 2, a.titles + 1, a.queries + 1).split(1, 2)
    both = ActionTable.concat(seq, tar)
    for t in (corpus_actions, both):
        t.item_id[:] = np.minimum(t.item_id, a.titles - 1)
        t.query_tok[:] = np.minimum(t.query_tok, a.queries - 1)
    sides = {"query": (strings.query_sequences(both, table), strings.query_sequences(corpus_actions, table), "all_query_score"),
             "title": (strings.title_sequences(both, item_title, table), strings.title_sequences(corpus_actions, item_title, table),
                       "all_product_title_score")}
    I = torch.from_numpy(np.random.default_rng(3).integers(0, a.n, (a.nq, a.k))).to(dev).contiguous()
    pairs = a.nq * a.k
    out = {"n": a.n, "nq": a.nq, "k": a.k, "reps": a.reps, "pairs": pairs, "strings": len(table), "chars": int(table.chars.numel()),
           "mean_chars": {"query": float(table.lengths[:a.queries].mean()), "title": float(table.lengths[a.queries:].mean())}}
    L, st = _lib.lib(), _lib.stream_ptr(dev)
    for kind, (q, c, sim_type) in sides.items():
        ratio = torch.empty((a.nq, a.k), dtype=torch.float64, device=dev)
        qm, cm, cl = (torch.empty((a.nq, a.k), dtype=torch.int32, device=dev) for _ in range(3))
        err, sums = torch.zeros(1, dtype=torch.int32, device=dev), torch.empty((a.nq, 2), dtype=torch.float64, device=dev)

        def scores():
            _lib.check(L.sss_seq_pair_scores(table.ptr.data_ptr(), table.chars.data_ptr(), len(table), q.ptr.data_ptr(), q.ids.data_ptr(),
                                             a.nq, c.ptr.data_ptr(), c.ids.data_ptr(), a.n, I.data_ptr(), a.k, 0, ratio.data_ptr(),
                                             qm.data_ptr(), cm.data_ptr(), cl.data_ptr(), err.data_ptr(), st), "sss_seq_pair_scores")

        def reduce():
            _lib.check(L.sss_seq_query_metric(qm.data_ptr(), cm.data_ptr(), cl.data_ptr(), q.lengths.data_ptr(), a.nq, a.k,
                                              sums.data_ptr(), st), "sss_seq_query_metric")
        r = {"pair_scores_ms": event_median_ms(scores, 2, a.reps), "query_metric_ms": event_median_ms(reduce, 2, a.reps)}
        assert int(err.item()) == 0
        string_pairs = int((q.lengths.long()[:, None] * cl.long()).sum().item())
        r.update(mean_query_strings=float(q.lengths.double().mean().item()), mean_corpus_strings=float(cl.double().mean().item()),
                 string_pairs=string_pairs, pairs_per_s=pairs / (r["pair_scores_ms"] * 1e-3),
                 string_pairs_per_s=string_pairs / (r["pair_scores_ms"] * 1e-3))
        walls = []
        for _ in range(a.reps + 1):
            torch.cuda.synchronize(); t0 = time.perf_counter(); ave = evaluation.get_ave_score(I, q, c, sim_type); torch.cuda.synchronize()
            walls.append((time.perf_counter() - t0) * 1e3)
        r.update(drop_in_wall_ms=float(np.median(walls[1:])), ave_score=ave)

        hq, hk = min(a.host_queries, a.nq), min(a.host_k, a.k)
        lists = lambda s, rows: {int(x): [vocab[k] for k in s.ids[int(s.ptr[x]):int(s.ptr[x + 1])].tolist()] for x in rows}
        host_I = I[:hq, :hk].cpu().numpy()
        host_q, host_c = lists(q, range(hq)), lists(c, np.unique(host_I))
        t0 = time.perf_counter()
        want = seqsim_ref.pair_scores(host_I, host_q, host_c)[0]
        r["host_restatement_ms"] = (time.perf_counter() - t0) * 1e3 / (hq * hk) * pairs
        r["host_pairs_timed"] = hq * hk
        r["host_equals_device"] = bool(np.array_equal(want, ratio[:hq, :hk].cpu().numpy(), equal_nan=True))
        out[kind] = r
    print(json.dumps(out))
    if not all(out[k]["host_equals_device"] for k in sides):
        raise SystemExit("the device scores differ from the restatement")


if __name__ == "__main__":
    main()
