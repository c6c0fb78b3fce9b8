"""Session-graph construction pinned to the reference.

tests/golden/reference_graph.npz holds what the reference's OWN `sequence_to_graph` (util_amazon_filtered.py:98-230)
returned for 330 sessions, each with ignore_query False and True (tests/golden/make_golden_graph.py: the function
bodies compiled out of the file's syntax tree; the container / tokenizer stand-ins supply no arithmetic).  Held to it
with `==`: the per-session oracle `oracle/graph_ref.py`, then `graph_ref.collate` and the vectorised host builder
`sessions.build_batch` over the whole table.  The one documented difference is the numbering of a session's products
(`list(set())` order upstream, first-occurrence order here); the relabelling is test code (tests/helpers/graph_np.py).
NOT pinned: `q_x` (the reference's query nodes carry token tensors, no id) and the token tensors themselves.
"""
import importlib.util
import itertools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import graph_np as G  # noqa: E402
from oracle import graph_ref  # noqa: E402
from sessionsimilaritysearch_amd import sessions as S  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))


def _generator():
    spec = importlib.util.spec_from_file_location("make_golden_graph", os.path.join(HERE, "golden", "make_golden_graph.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def fx():
    z = G.load_fixture()
    R = len(z["sess_ptr"]) - 1
    return dict(z=z, R=R, sessions=G.fixture_sessions(z), raw=[G.fixture_graph(z, r) for r in range(R)])


def test_fixture_holds_the_cases_it_names(fx):
    z, R, sessions = fx["z"], fx["R"], fx["sessions"]
    assert R == 660 and np.array_equal(z["ignore_query"], np.arange(R) % 2 == 1)
    ln = np.diff(z["sess_ptr"])
    assert set(ln[0::2].tolist()) >= {0, 1, 2, 3, 5, 8, 19, 20, 63, 64}
    assert z["item_id"].max() > 2 ** 16 and z["item_id"].max() < 391572 and z["item_id"].min() == 0
    for r in range(1, R, 2):                                  # ignore_query: the reference kept the clicks, in order
        assert not any(a[0] for a in sessions[r])
        assert [a[1] for a in sessions[r]] == [a[1] for a in sessions[r - 1] if not a[0]]
    hand = sessions[0:2 * int(z["n_hand"]):2]
    T, F = True, False
    assert hand[0] == [] and hand[1] == [(T, 0, 3)] and hand[2] == [(F, 11, 0)]
    assert [a[0] for a in hand[3]] == [F] * 4 and [a[0] for a in hand[4]] == [T] * 3
    assert [a[1] for a in hand[5]] == [11] * 4 and [a[1] for a in hand[6]] == [11, 5, 11, 5]
    assert [a[:2] for a in hand[7]] == [(F, 11), (T, 0), (F, 11)]
    assert len(hand[8]) == 64 and not hand[8][63][0] and len(hand[9]) == 64 and hand[9][63][0]
    # a search-only session under ignore_query is a zero-action session
    assert sessions[2 * 4 + 1] == [] and sessions[3] == []
    # the relabelling is exercised: some record's products are NOT in first-occurrence order upstream
    moved = sum(not np.array_equal(G.relabel_first_occurrence(g)["p_x"], g["p_x"]) for g in fx["raw"])
    assert moved > 50


def test_session_oracle_equals_the_reference_run(fx):
    """oracle/graph_ref.session_to_graph == the reference's sequence_to_graph, record by record: distinct items and
    their counts, the grouped position ids, query positions, click edges (both directions), de-duplicated
    transitions in first-seen order and their weights; the query mask is 0 for the root and 1 for every search."""
    for r, (seq, raw) in enumerate(zip(fx["sessions"], fx["raw"])):
        ref = G.relabel_first_occurrence(raw)
        got = graph_ref.session_to_graph(seq)
        assert got["p_x"] == ref["p_x"].tolist(), r
        assert got["p_cnt"] == ref["p_cnt"].tolist(), r
        assert got["p_pos"] == ref["p_pos"].tolist(), r
        assert got["q_pos"] == ref["q_pos"].tolist(), r
        assert len(got["q_x"]) == len(ref["q_pos"]), r
        assert ref["q_mask"].tolist() == [0.0] + [1.0] * (len(got["q_x"]) - 1), r
        assert [list(got["qp"][0]), list(got["qp"][1])] == ref["qp"].tolist(), r
        assert [list(got["qp"][1]), list(got["qp"][0])] == ref["pq"].tolist(), r
        assert [list(got["pp"][0]), list(got["pp"][1])] == ref["pp"].tolist(), r
        assert ref["pp_w"].dtype == np.float32 and [float(v) for v in got["pp_w"]] == ref["pp_w"].tolist(), r


def test_hand_written_sessions_known_answers(fx):
    """The reference's outputs for the hand-written sessions, read off the fixture (ignore_query False)."""
    ref = [G.relabel_first_occurrence(fx["raw"][2 * i]) for i in range(int(fx["z"]["n_hand"]))]
    for i in (0, 1, 4):                                       # no click: the unknown-item node, one position id 0
        assert ref[i]["p_x"].tolist() == [0] and ref[i]["p_cnt"].tolist() == [1] and ref[i]["p_pos"].tolist() == [0]
        assert ref[i]["qp"].shape == (2, 0) and ref[i]["pp"].shape == (2, 0) and ref[i]["p_last"].tolist() == [1.0]
    assert ref[0]["q_pos"].tolist() == [0] and ref[1]["q_pos"].tolist() == [1, 0] and ref[4]["q_pos"].tolist() == [3, 2, 1, 0]
    assert ref[5]["pp"].tolist() == [[0], [0]] and ref[5]["pp_w"].tolist() == [3.0] and ref[5]["p_pos"].tolist() == [4, 3, 2, 1]
    assert ref[6]["pp"].tolist() == [[0, 1], [1, 0]] and ref[6]["pp_w"].tolist() == [2.0, 1.0]
    assert ref[6]["p_pos"].tolist() == [4, 2, 3, 1] and ref[6]["p_last"].tolist() == [0.0, 1.0]
    assert ref[7]["qp"].tolist() == [[0, 1], [0, 0]] and ref[7]["pp"].tolist() == [[0], [0]] and ref[7]["pp_w"].tolist() == [1.0]


def test_last_click_equals_the_reference_mask(fx):
    """`last_click` of the oracle = the one position the reference's last_click_mask sets (:203-216): the target of
    the last transition, node 0 when the session has fewer than two clicks."""
    two_hot = 0
    for r, (seq, raw) in enumerate(zip(fx["sessions"], fx["raw"])):
        ref = G.relabel_first_occurrence(raw)
        got = graph_ref.session_to_graph(seq)
        mask = np.zeros(len(got["p_x"]), np.float32)
        mask[got["last_click"]] = 1.0
        assert np.array_equal(mask, ref["p_last"]), r
        two_hot += got["last_click"] != 0
    assert two_hot > 50


def test_batched_builders_equal_the_collated_reference_run(fx):
    """graph_ref.collate and sessions.build_batch over the WHOLE fixture table (660 sessions in one batch, zero-action
    sessions among them) == the reference-run graphs collated here with plain numpy offsets."""
    z = fx["z"]
    ref = G.collate_fixture(z)
    o = graph_ref.collate([graph_ref.session_to_graph(s) for s in fx["sessions"]])
    acts = S.ActionTable(z["sess_ptr"], z["is_search"], z["item_id"], z["query_tok"])
    b = G.batch_to_collated(S.build_batch(acts))
    for k in G.COLLATED_KEYS:
        assert o[k].dtype == ref[k].dtype and np.array_equal(o[k], ref[k]), "collate " + k
        assert b[k].dtype == ref[k].dtype and np.array_equal(b[k], ref[k]), "build_batch " + k
    bb = S.build_batch(acts)
    assert np.array_equal(bb.edge_index_dict[S.EDGE_PQ], np.stack([ref["qp1"], ref["qp0"]]))
    assert bb.num_graphs == fx["R"]


@pytest.mark.parametrize("where", ["front", "middle", "end", "all three", "only"])
def test_zero_action_sessions_pass_through_build_batch(where):
    """A zero-action session (what a search-only session becomes under the deployed ignore_query=True) is a root query
    node + the unknown-item node with position id 0 and no edge, wherever it sits in the batch."""
    rng = np.random.default_rng(5)
    body = [[(bool(rng.random() < 0.3), int(rng.integers(1, 5)), int(rng.integers(1, 9))) for _ in range(n)]
            for n in (3, 1, 7, 2)]
    body = [[(s, 0 if s else it, tok if s else 0) for s, it, tok in seq] for seq in body]
    sessions = {"front": [[], []] + body, "middle": body[:2] + [[]] + body[2:], "end": body + [[]],
                "all three": [[]] + body[:2] + [[], []] + body[2:] + [[]], "only": [[], [], []]}[where]
    flat = [a for s in sessions for a in s]
    acts = S.ActionTable(np.r_[0, np.cumsum([len(s) for s in sessions])].astype(np.int64),
                         np.array([a[0] for a in flat], bool), np.array([a[1] for a in flat], np.int64),
                         np.array([a[2] for a in flat], np.int64))
    o = graph_ref.collate([graph_ref.session_to_graph(s) for s in sessions])
    b = G.batch_to_collated(S.build_batch(acts))
    for k in G.COLLATED_KEYS:
        assert np.array_equal(b[k], o[k]) and b[k].dtype == o[k].dtype, k
    for g, s in enumerate(sessions):
        if not s:
            assert o["q_pos"][o["q_batch"] == g].tolist() == [0] and o["p_x"][o["p_batch"] == g].tolist() == [0]


def test_every_small_structure_through_build_batch():
    """All sessions of length 0..6 over {search, item 1, item 2, item 3} (5 461 in one batch): the vectorised host
    builder against the per-session oracle.  The GPU suite runs the same table through the native builder."""
    act = lambda sym, t: (True, 0, 1 + t) if sym == 0 else (False, sym, 0)
    sessions = [[act(sym, t) for t, sym in enumerate(p)] for n in range(7) for p in itertools.product(range(4), repeat=n)]
    flat = [a for s in sessions for a in s]
    acts = S.ActionTable(np.r_[0, np.cumsum([len(s) for s in sessions])].astype(np.int64),
                         np.array([a[0] for a in flat], bool), np.array([a[1] for a in flat], np.int64),
                         np.array([a[2] for a in flat], np.int64))
    assert acts.num_sessions == 5461
    o = graph_ref.collate([graph_ref.session_to_graph(s) for s in sessions])
    b = G.batch_to_collated(S.build_batch(acts))
    for k in G.COLLATED_KEYS:
        assert np.array_equal(b[k], o[k]), k


_GEN = _generator()


@pytest.mark.skipif(not os.path.isfile(os.path.join(_GEN.REF, "util_amazon_filtered.py")),
                    reason="the reference tree is only present in the build container")
def test_regenerating_the_fixture_reproduces_the_committed_arrays(tmp_path, fx):
    _GEN.main(str(tmp_path))
    new = G.load_fixture(str(tmp_path / "reference_graph.npz"))
    assert sorted(new) == sorted(fx["z"])
    for k, v in fx["z"].items():
        assert new[k].dtype == v.dtype and np.array_equal(new[k], v), k
