"""ignore_query and last_click_mask on the host: `sessions.build_batch(actions, ignore_query=True)`, `ActionTable.clicks_only()`
and `data['product'].last_click_mask`, held with array_equal to what the reference's own sequence_to_graph returned
(tests/golden/reference_graph.npz: record 2i run with ignore_query=False, record 2i+1 with ignore_query=True, every
record with its mask `p_last`); and the header / ctypes table of the `_ex` builder entry points (include/sss_graph.h).
The subset collation of the fixture is test code (numpy offsets), as in tests/helpers/graph_np.py."""
import itertools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
from abi import declared  # noqa: E402
import graph_np as G  # noqa: E402
from sessionsimilaritysearch_amd import _lib  # noqa: E402
from sessionsimilaritysearch_amd import sessions as S  # noqa: E402

NODE_KEYS = {"product": ("x", "batch", "cnt", "pos_emb_id", "last_click_mask"), "query": ("x", "batch", "pos_emb_id")}


def records_table(z, recs):
    """The INPUT sessions of the fixture records `recs`, in that order, as one ActionTable."""
    sp = z["sess_ptr"]
    idx = np.concatenate([np.arange(sp[r], sp[r + 1]) for r in recs] + [np.zeros(0, np.int64)]).astype(np.int64)
    ptr = np.r_[0, np.cumsum([sp[r + 1] - sp[r] for r in recs])].astype(np.int64)
    return S.ActionTable(ptr, z["is_search"][idx].astype(bool), z["item_id"][idx].astype(np.int64),
                         z["query_tok"][idx].astype(np.int64))


def collate_records(z, recs):
    """The reference's OUTPUTS of the records `recs`, relabelled to first-occurrence order and concatenated with numpy
    offsets (G.collate_fixture for a subset).  q_x: the root's 0, then the record's own search tokens."""
    gs = [G.relabel_first_occurrence(G.fixture_graph(z, r)) for r in recs]
    nq, n_p = np.array([len(g["q_pos"]) for g in gs]), np.array([len(g["p_x"]) for g in gs])
    qo, po = np.r_[0, np.cumsum(nq)], np.r_[0, np.cumsum(n_p)]
    cat = lambda f: np.concatenate([f(i, g) for i, g in enumerate(gs)]).astype(np.int64)
    sp = z["sess_ptr"]
    o = dict(
        q_x=cat(lambda i, g: np.r_[0, z["query_tok"][sp[recs[i]]:sp[recs[i] + 1]][z["is_search"][sp[recs[i]]:sp[recs[i] + 1]]]]),
        q_pos=cat(lambda i, g: g["q_pos"]), q_batch=np.repeat(np.arange(len(gs)), nq),
        p_x=cat(lambda i, g: g["p_x"]), p_cnt=cat(lambda i, g: g["p_cnt"]), p_pos=cat(lambda i, g: g["p_pos"]),
        p_batch=np.repeat(np.arange(len(gs)), n_p),
        qp0=cat(lambda i, g: g["qp"][0] + qo[i]), qp1=cat(lambda i, g: g["qp"][1] + po[i]),
        pp0=cat(lambda i, g: g["pp"][0] + po[i]), pp1=cat(lambda i, g: g["pp"][1] + po[i]))
    o["pp_w"] = np.concatenate([g["pp_w"] for g in gs]).astype(np.float32)
    o["p_last"] = np.concatenate([g["p_last"] for g in gs]).astype(np.float32)
    return o


def table(sessions):
    flat = [a for s in sessions for a in s]
    return S.ActionTable(np.r_[0, np.cumsum([len(s) for s in sessions], dtype=np.int64)].astype(np.int64),
                         np.array([a[0] for a in flat], bool), np.array([a[1] for a in flat], np.int64),
                         np.array([a[2] for a in flat], np.int64))


def assert_batches_equal(a, b):
    assert a.num_graphs == b.num_graphs
    for t, keys in NODE_KEYS.items():
        assert sorted(a[t].keys()) == sorted(b[t].keys()) == sorted(keys)
        for k in keys:
            x, y = getattr(a[t], k), getattr(b[t], k)
            assert x.dtype == y.dtype and np.array_equal(x, y), (t, k)
    for e in (S.EDGE_QP, S.EDGE_PQ, S.EDGE_PP):
        assert np.array_equal(a.edge_index_dict[e], b.edge_index_dict[e]), e
    assert a.edge_weight_dict[S.EDGE_QP] is None and a.edge_weight_dict[S.EDGE_PQ] is None
    assert np.array_equal(a.edge_weight_dict[S.EDGE_PP], b.edge_weight_dict[S.EDGE_PP])


@pytest.fixture(scope="module")
def z():
    return G.load_fixture()


def test_host_builder_ignore_query_equals_the_reference_run(z):
    """The unfiltered sessions (even records) with ignore_query=True == the reference's run of them with ignore_query=True
    (odd records): lengths, position ids, the one query node per graph, edges, transitions and the mask."""
    R = len(z["sess_ptr"]) - 1
    even, odd = list(range(0, R, 2)), list(range(1, R, 2))
    ref = collate_records(z, odd)
    b = S.build_batch(records_table(z, even), ignore_query=True)
    got = G.batch_to_collated(b)
    for k in G.COLLATED_KEYS:
        assert got[k].dtype == ref[k].dtype and np.array_equal(got[k], ref[k]), k
    assert b.num_graphs == len(even) == 330
    assert len(got["q_x"]) == 330 and not got["q_x"].any() and np.array_equal(got["q_batch"], np.arange(330))
    mask = b["product"].last_click_mask
    assert mask.dtype == np.float32 and np.array_equal(mask, ref["p_last"])
    assert np.array_equal(b.edge_index_dict[S.EDGE_PQ], np.stack([ref["qp1"], ref["qp0"]]))
    assert z["is_search"][np.concatenate([np.arange(z["sess_ptr"][r], z["sess_ptr"][r + 1]) for r in even])].sum() > 100


def test_host_mask_equals_the_reference_mask(z):
    """ignore_query=False, all 660 records in one batch: last_click_mask == the reference's, relabelled and concatenated."""
    R = len(z["sess_ptr"]) - 1
    b = S.build_batch(S.ActionTable(z["sess_ptr"], z["is_search"], z["item_id"], z["query_tok"]))
    mask = b["product"].last_click_mask
    ref = G.collate_fixture(z)["p_last"]
    assert mask.dtype == np.float32 and mask.shape == b["product"].x.shape and np.array_equal(mask, ref)
    first = np.r_[0, np.cumsum(np.bincount(b["product"].batch, minlength=R))][:-1]     # node 0 of every graph
    assert np.array_equal(np.add.reduceat(mask, first), np.ones(R, np.float32))       # exactly one 1 per graph
    assert int(np.sum(mask[first] == 0.0)) > 50                                        # ... and not always at node 0


def every_small_session():
    act = lambda sym, t: (True, 0, 1 + t) if sym == 0 else (False, sym, 0)
    return [[act(sym, t) for t, sym in enumerate(p)] for n in range(7) for p in itertools.product(range(4), repeat=n)]


@pytest.mark.parametrize("kind", ["fixture", "every small structure", "search-only"])
def test_ignore_query_is_filtering_on_the_host(z, kind):
    """build_batch(t, ignore_query=True) == build_batch(t.clicks_only()) on every key; clicks_only itself against what
    it must return, stated independently per kind."""
    if kind == "fixture":
        R = len(z["sess_ptr"]) - 1
        t = records_table(z, range(R))
        want = records_table(z, [r | 1 for r in range(R)])          # the reference's own filtered sessions (odd records)
    elif kind == "every small structure":
        sessions = every_small_session()
        assert len(sessions) == 5461
        t, want = table(sessions), table([[a for a in s if not a[0]] for s in sessions])
    else:
        sessions = [[(True, 0, 1 + (i + t) % 7) for t in range(n)] for i, n in enumerate((1, 3, 0, 64, 2))]
        t, want = table(sessions), table([[] for _ in sessions])
    c = t.clicks_only()
    for k in ("sess_ptr", "is_search", "item_id", "query_tok"):
        assert getattr(c, k).dtype == getattr(want, k).dtype and np.array_equal(getattr(c, k), getattr(want, k)), k
    assert not c.is_search.any() and c.num_sessions == t.num_sessions
    a, b = S.build_batch(t, ignore_query=True), S.build_batch(c)
    assert_batches_equal(a, b)
    assert a["query"].x.shape[0] == t.num_sessions and not a["query"].x.any()
    if kind == "search-only":
        n = t.num_sessions
        assert np.array_equal(a["product"].last_click_mask, np.ones(n, np.float32)) and not a["product"].x.any()
        assert a.edge_index_dict[S.EDGE_QP].shape == (2, 0) and a.edge_index_dict[S.EDGE_PP].shape == (2, 0)
        assert not a["query"].pos_emb_id.any() and not a["product"].pos_emb_id.any()


def test_graph_header_library_and_ctypes_binding_name_the_same_entry_points():
    names = declared("sss_graph.h")
    assert names == _lib.symbols("sss_graph.h") == ["sss_graph_counts_ex", "sss_graph_fill_ex"]
    L = _lib.lib()
    for n in names:
        assert getattr(L, n).argtypes == _lib.HEADERS["sss_graph.h"][n][1]
    others = set(_lib.exported_symbols()) | set(_lib.symbols("sss_sparse.h")) | set(_lib.symbols("sss_l2.h")) | set(_lib.symbols("sss_pad.h"))
    assert not set(names) & others
    assert declared("sss.h") == _lib.exported_symbols() and len(_lib.exported_symbols()) == 60
    # argument rules, checked before anything is launched (addresses that are never dereferenced)
    A = 1 << 20
    for flags in (2, 3, 4, -1, 1 << 16):
        assert L.sss_graph_counts_ex(A, A, A, 8, flags, A, A, A, 0) == -1
        assert L.sss_last_error().startswith(b"graph_counts_ex:")
        assert L.sss_graph_fill_ex(A, A, A, A, 8, flags, A, A, A, A, 0) == -1
        assert L.sss_last_error().startswith(b"graph_fill_ex:")
    for flags in (0, 1):
        for kw in (dict(n=0), dict(n=-3), dict(sp=0), dict(bases=0), dict(scratch=0), dict(err=0)):
            a = {**dict(sp=A, n=8, bases=A, scratch=A, err=A), **kw}
            assert L.sss_graph_counts_ex(a["sp"], A, A, a["n"], flags, a["bases"], a["scratch"], a["err"], 0) == -1, kw
            assert L.sss_last_error().startswith(b"graph_counts_ex:")
        for kw in (dict(n=0), dict(sp=0), dict(bases=0), dict(out=0)):
            a = {**dict(sp=A, n=8, bases=A, out=A), **kw}
            assert L.sss_graph_fill_ex(a["sp"], A, A, A, a["n"], flags, a["bases"], a["out"], 0, 0, 0) == -1, kw
            assert L.sss_last_error().startswith(b"graph_fill_ex:")
