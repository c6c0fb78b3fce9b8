"""Dev helper: the native session-graph builder (csrc/graphbuild.hip through SessionEncoder.prepare_actions) on
synthetic_actions(1M sessions): the default mode and ignore_query=True.  The action table is uploaded once, outside the
timed region -- a call is the two kernel sweeps, the scans, the id-bound reductions, the one read-back of the totals and
the output allocations.  Prints one JSON line, per mode:
  prepare_actions_ms   hipEvent median over --reps calls after --warmup
  min_ms, max_ms       the spread inside the run
--root PATH times the package of another checkout (built there) with the same loop, so that two commits can be run
alternately on one card: `--root <parent checkout> --modes default`, then this one, and again."""
import argparse
import json
import os
import sys
import types

import numpy as np
import torch


def event_times_ms(fn, warmup, reps):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); fn(); b.record(); b.synchronize()
        ts.append(a.elapsed_time(b))
    return ts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1000000)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--modes", default="default,ignore_query")
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    a = ap.parse_args()
    if a.reps < 10:
        raise SystemExit("--reps must be at least 10")
    sys.path.insert(0, os.path.abspath(a.root))
    from sessionsimilaritysearch_amd.encoder import EncoderConfig, SessionEncoder, init_weights
    from sessionsimilaritysearch_amd.sessions import synthetic_actions

    dev = torch.device("cuda", 0)
    cfg = EncoderConfig(d_in=32, h=32, n_layers=1, d_out=96)
    enc = SessionEncoder(cfg, init_weights(cfg, 1, tables=False), dev)
    acts = synthetic_actions(a.n, a.seed)
    table = types.SimpleNamespace(**{k: torch.from_numpy(getattr(acts, k)).to(dev)
                                     for k in ("sess_ptr", "is_search", "item_id", "query_tok")})
    out = {"n_sessions": a.n, "n_actions": int(acts.sess_ptr[-1]), "reps": a.reps, "warmup": a.warmup,
           "root": os.path.abspath(a.root)}
    for mode in a.modes.split(","):
        kw = {"ignore_query": True} if mode == "ignore_query" else {}
        pb = enc.prepare_actions(table, **kw)
        ts = event_times_ms(lambda: enc.prepare_actions(table, **kw), a.warmup, a.reps)
        out[mode] = {"prepare_actions_ms": float(np.median(ts)), "min_ms": float(min(ts)), "max_ms": float(max(ts)),
                     "Nq": pb.Nq, "Np": pb.Np, "n_clicks": pb.n_clicks}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
