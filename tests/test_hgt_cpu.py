"""CPU side of the HGT encoder (include/sss_hgt.h, variants.HGT): the two restatements of tests/helpers/hgt_ref.py against
each other, hgt_fold_weights against the unfolded restatement, the header against its ctypes binding, and the argument
checks of both entry points, which return before any device work."""
import ctypes
import math
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
from abi import declared  # noqa: E402
import hgt_ref as hr  # noqa: E402

from sessionsimilaritysearch_amd import _lib  # noqa: E402
from sessionsimilaritysearch_amd import sessions as S  # noqa: E402
from sessionsimilaritysearch_amd.sessions import EDGE_PP, EDGE_PQ, EDGE_QP  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def synthetic_graph(n_sessions, seed):
    """(Nq, Np, edges) of a seeded batch of synthetic sessions."""
    b = S.build_batch(S.synthetic_actions(n_sessions, seed, 500, 65)).to_numpy()
    ei = b.edge_index_dict
    return len(b["query"].x), len(b["product"].x), {"qp": ei[EDGE_QP], "pq": ei[EDGE_PQ], "pp": ei[EDGE_PP]}


def hand_graphs():
    """Hand-made graphs: an empty pp edge set with duplicate qp edges; a query with no clicks (no pq edge reaches query 2)
    beside targets of in-degree 1, duplicate pp edges and a product nothing points at (product 4)."""
    e = lambda *pairs: np.asarray(pairs, dtype=np.int64).reshape(-1, 2).T
    yield 2, 3, {"qp": e((0, 0), (0, 0), (1, 0), (1, 2)), "pq": e((0, 0), (2, 1), (1, 1)), "pp": e()}
    yield 3, 5, {"qp": e((0, 0), (1, 1), (0, 2), (1, 2), (1, 2)), "pq": e((0, 0), (1, 0), (2, 1)),
                 "pp": e((0, 1), (0, 1), (1, 3), (2, 3), (3, 0))}


def _inputs(g, nq, np_, d):
    return torch.randn((nq, d), generator=g, dtype=torch.float64), torch.randn((np_, d), generator=g, dtype=torch.float64)


def test_the_two_restatements_agree_in_float64():
    g = torch.Generator().manual_seed(5)
    graphs = [synthetic_graph(12, 11)] + list(hand_graphs())
    for (nq, np_, edges), (h, heads) in zip(graphs, ((32, 4), (24, 2), (16, 8))):
        w = {k: v.double() for k, v in hr.make_weights(g, 20, 20, h, heads, 2).items()}
        xq, xp = _inputs(g, nq, np_, 20)
        a = hr.hgt_torch(xq, xp, edges, w, heads, 2)
        b = hr.hgt_loops(xq.numpy(), xp.numpy(), edges, w, heads, 2)
        for t in hr.TYPES:
            assert a[t].shape == (xq.shape[0] if t == "query" else xp.shape[0], 3 * h)
            assert np.abs(a[t].numpy() - b[t]).max() < 1e-12, (t, h, heads)
    # the hand graphs hold what they are for
    (_, _, e0), (_, _, e1) = hand_graphs()
    assert e0["pp"].shape == (2, 0) and 2 not in e1["pq"][1] and 4 not in np.concatenate([e1["qp"][1], e1["pp"][1]])
    assert (np.bincount(e1["qp"][1], minlength=5)[:2] == 1).all() and (e1["pp"][:, 0] == e1["pp"][:, 1]).all()


@pytest.mark.parametrize("heads", [1, 2, 4, 8])
def test_fold_weights_reproduces_the_unfolded_restatement(heads):
    """Applying the folded matrices gives k^e with the score scale p_rel / sqrt(D) in it, v^e, q, and sigmoid(skip) * a_lin
    with beta = 1 - sigmoid(skip), all to 1e-12 in float64; the K^e | V^e pair of an edge type is adjacent."""
    from sessionsimilaritysearch_amd.variants import HGT_BLOCKS, hgt_fold_weights
    g = torch.Generator().manual_seed(20 + heads)
    h, L = 32, 2
    D = h // heads
    w = {k: v.double() for k, v in hr.make_weights(g, 12, 20, h, heads, L).items()}
    nq, np_, edges = synthetic_graph(8, 13)
    f = hgt_fold_weights(w, heads, L)
    assert f["h"] == h and f["heads"] == heads and len(f["layers"]) == L
    assert HGT_BLOCKS == {"product": ("q", "pq.k", "pq.v", "pp.k", "pp.v"), "query": ("q", "qp.k", "qp.v")}
    x = {"query": torch.randn((nq, h), generator=g, dtype=torch.float64), "product": torch.randn((np_, h), generator=g, dtype=torch.float64)}
    for l in range(L):
        parts = {}
        new = hr.hgt_conv_torch(x, edges, w, l, heads, parts)
        for t in hr.TYPES:
            lay = f["layers"][l][t]
            assert lay["w"].dtype == torch.float64 and lay["w"].shape == (len(HGT_BLOCKS[t]) * h, h)
            y = x[t] @ lay["w"].T + lay["b"]
            for i, blk in enumerate(HGT_BLOCKS[t]):
                got = y[:, i * h:(i + 1) * h].reshape(-1, heads, D)
                if blk == "q":
                    want = (x[t] @ w[f"hgt.{l}.{t}.q.w"].T + w[f"hgt.{l}.{t}.q.b"]).view(-1, heads, D)
                else:
                    e, kind = blk.split(".")
                    want = parts[f"{kind}.{e}"]
                    if kind == "k":
                        want = want * (w[f"hgt.{l}.{e}.p_rel"] / math.sqrt(D)).view(1, heads, 1)
                assert (got - want).abs().max() < 1e-12, (l, t, blk)
            sig = torch.sigmoid(w[f"hgt.{l}.{t}.skip"].reshape(()))
            agg = torch.nn.functional.gelu(parts[f"agg.{t}"])
            y = agg @ lay["a_w"].T + lay["a_b"] + lay["beta"] * x[t]
            assert abs(lay["beta"] - float(1 - sig)) < 1e-15 and (y - new[t]).abs().max() < 1e-12, (l, t)
        # the folded k gives the restatement's logits as plain dot products
        for e, s, t in hr.EDGES:
            blocks, src = HGT_BLOCKS[s], f["layers"][l][s]
            i = blocks.index(e + ".k")
            assert blocks[i + 1] == e + ".v"
            k = (x[s] @ src["w"].T + src["b"])[:, i * h:(i + 1) * h].reshape(-1, heads, D)
            q = (x[t] @ f["layers"][l][t]["w"].T + f["layers"][l][t]["b"])[:, :h].reshape(-1, heads, D)
            alpha = (q[torch.as_tensor(edges[e][1])] * k[torch.as_tensor(edges[e][0])]).sum(-1)
            assert (alpha - parts[f"alpha.{e}"]).abs().max() < 1e-12, (l, e)
        x = new
    with pytest.raises(ValueError):
        hgt_fold_weights(w, 3, L)


def test_package_exports_the_hgt_encoder():
    import sessionsimilaritysearch_amd as pkg
    from sessionsimilaritysearch_amd import variants
    assert pkg.HGT is variants.HGT and pkg.hgt_fold_weights is variants.hgt_fold_weights
    assert {"HGT", "hgt_fold_weights"} <= set(pkg.__all__)


# ------------------------------------------------------------------------------------------------ the C ABI
def test_hgt_header_and_binding_declare_the_same_entry_points():
    names = declared("sss_hgt.h")
    assert names == _lib.symbols("sss_hgt.h") == ["sss_hgt_aggregate", "sss_hgt_skip"]
    L = _lib.lib()
    for n in names:
        assert getattr(L, n).argtypes == _lib.HEADERS["sss_hgt.h"][n][1] and getattr(L, n).restype is ctypes.c_int
    for header, table in _lib.HEADERS.items():
        if header != "sss_hgt.h":
            assert not set(names) & set(table) and not set(names) & set(declared(header)), header
    assert declared("sss.h") == _lib.exported_symbols()
    text = open(os.path.join(ROOT, "include", "sss_hgt.h")).read()
    for phrase in ("CALLER-OWNED DEVICE", "nothing is allocated", "no host synchronisation", "enqueued on `stream`",
                   "-1 bad argument", "-3 HIP error"):
        assert phrase in text, phrase
    # the structs mirror the header field for field (names in order)
    body = lambda name: re.search(r"typedef struct \{([^}]*)\} " + name + ";", re.sub(r"/\*.*?\*/", "", text, flags=re.S), re.S).group(1)
    fields = lambda name: re.findall(r"(\w+)(?:\[\d+\])?\s*;", body(name))
    assert fields("sss_hgt_slot") == [n for n, _ in _lib.HgtSlot._fields_]
    assert fields("sss_hgt_args") == [n for n, _ in _lib.HgtArgs._fields_]


_P = 1 << 20                                                          # a non-null, 16-byte aligned address; never dereferenced


def _aggregate(L, **kw):
    a = dict(q=_P, ld_q=128, out=_P, ld_out=128, n_slots=1, n_dst=7, heads=4, head_dim=32, gelu=1, k=_P, ld_k=128, v=_P, ld_v=128,
             rowptr=_P, col=_P)
    a.update(kw)
    slot = _lib.HgtSlot(k=a["k"], ld_k=a["ld_k"], v=a["v"], ld_v=a["ld_v"], rowptr=a["rowptr"], col=a["col"])
    args = _lib.HgtArgs(q=a["q"], ld_q=a["ld_q"], n_slots=a["n_slots"], n_dst=a["n_dst"], heads=a["heads"], head_dim=a["head_dim"],
                        gelu=a["gelu"], out=a["out"], ld_out=a["ld_out"])
    args.slot[0], args.slot[1] = slot, slot
    return L.sss_hgt_aggregate(ctypes.byref(args), 0)


def test_argument_checks_return_before_any_device_work():
    """No address given here is memory: a call that launched would fault."""
    L = _lib.lib()
    bad = [dict(heads=3), dict(heads=0), dict(heads=16), dict(head_dim=30), dict(head_dim=0), dict(heads=8, head_dim=260),
           dict(heads=1, head_dim=2052), dict(n_slots=0), dict(n_slots=3), dict(n_dst=-1), dict(n_dst=1 << 31), dict(ld_q=126),
           dict(ld_q=124), dict(ld_k=130), dict(ld_v=64), dict(ld_out=120), dict(q=0), dict(out=0), dict(k=0), dict(v=_P + 4),
           dict(rowptr=0), dict(col=0)]
    for kw in bad:
        assert _aggregate(L, **kw) == -1 and L.sss_last_error().startswith(b"hgt_aggregate:"), kw
    assert L.sss_hgt_aggregate(None, 0) == -1 and L.sss_last_error().startswith(b"hgt_aggregate:")
    assert _aggregate(L, n_dst=0) == 0 and _aggregate(L, n_dst=0, n_slots=2, heads=8, head_dim=256, ld_q=2048, ld_k=2048,
                                                      ld_v=2048, ld_out=2048) == 0
    assert _aggregate(L, n_dst=0, heads=3) == -1                       # an empty batch's scalars are still checked
    assert _aggregate(L, n_dst=0, q=0, out=0, k=0, v=0, rowptr=0, col=0) == 0      # and it has no buffers
    skip = lambda **kw: L.sss_hgt_skip(*(dict(y=_P, ld_y=64, x=_P + 256, ld_x=64, beta=0.5, n=5, h=64, st=0) | kw).values())
    for kw in (dict(h=0), dict(h=30), dict(n=-1), dict(n=1 << 31), dict(ld_y=60), dict(ld_x=66), dict(y=0), dict(x=0), dict(x=_P + 8)):
        assert skip(**kw) == -1 and L.sss_last_error().startswith(b"hgt_skip:"), kw
    assert skip(n=0) == 0 and skip(n=0, y=0, x=0) == 0 and skip(n=0, h=30) == -1
