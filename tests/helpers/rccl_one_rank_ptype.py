"""Child process of tests/test_type_score_gpu.py: ShardedProductTypeIndex's exchange route on a ONE-rank RCCL group ("nccl"
on ROCm), started as a fresh process so that the process group exists before anything else of it touches the GPU.  search
(all-gather of the pack, k_topk_merge) and bands (all-reduce SUM of the counts, MIN of the first rows) with
force_collectives=True and an id_offset, each array_equal to the unsharded index's own answer and to the numpy helper.
Prints one JSON line; exit code 0 = every check passed."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [ROOT, HERE]

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402

OFF = 1000
N_ITEMS, N_TYPES = 60, 9


def main():
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ.setdefault("MASTER_PORT", sys.argv[1] if len(sys.argv) > 1 else "29536")
    dev = torch.device("cuda", 0)
    dist.init_process_group("nccl", world_size=1, rank=0, device_id=dev)
    torch.cuda.set_device(dev)
    import type_score_ref as tr
    from sessionsimilaritysearch_amd import sparse
    from sessionsimilaritysearch_amd.distributed import ProductTypeEngine, ShardedProductTypeIndex
    from sessionsimilaritysearch_amd.product_types import ProductTypeIndex
    from sessionsimilaritysearch_amd.sessions import synthetic_actions

    item_type = (np.random.default_rng(9).integers(0, N_TYPES + 1, N_ITEMS) - 1).astype(np.int32)      # -1: an item without a type
    c = tr.bags(synthetic_actions(3000, 5, N_ITEMS, 9), item_type)
    q = tr.bags(synthetic_actions(33, 6, N_ITEMS, 9), item_type)
    s = tr.scores(q, c, N_TYPES)
    index = ProductTypeIndex(N_TYPES, dev).add(sparse._device_triple(*c, dev))
    index.id_offset = OFF
    qd = sparse._device_triple(*q, dev)
    sh = ShardedProductTypeIndex(ProductTypeEngine(index), dev, force_collectives=True)
    same = lambda got, want: bool(all(np.array_equal(g.cpu().numpy(), w.cpu().numpy() if isinstance(w, torch.Tensor) else w)
                                      for g, w in zip(got, want)))
    checks = {"exchange": sh.exchange}
    for k in (10, 1024):
        want = tuple(t.clone() for t in index.search(qd, k))
        got = sh.search(qd, k)
        checks[f"search{k}_vs_unsharded"], checks[f"search{k}_vs_helper"] = same(got, want), same(got, tr.topk(s, k, OFF))
    for edges in ((0.2, 0.8), (0.0,), (0.1, 0.2, 0.3, 0.4, 0.5, 0.8, 1.0)):
        got = sh.bands(qd, edges)
        checks[f"bands{len(edges)}_vs_unsharded"] = same(got, index.bands(qd, edges))
        checks[f"bands{len(edges)}_vs_helper"] = same(got, tr.bands(s, edges, OFF))
    checks["an_empty_band_and_a_full_one"] = bool((tr.bands(s, (0.0,))[1][:, 0] == -1).all() and (tr.bands(s, (0.2, 0.8))[0] > 0).all(1).any())
    torch.cuda.synchronize()
    out = {"backend": dist.get_backend(), "world": dist.get_world_size(), "checks": checks}
    out["ok"] = bool(all(checks.values()) and out["backend"] == "nccl")
    print(json.dumps(out), flush=True)
    dist.destroy_process_group()
    return 0 if out["ok"] else 1


if __name__ == "__main__":
    sys.exit(main())
