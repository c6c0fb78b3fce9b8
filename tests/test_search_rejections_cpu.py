"""The scanning search entry points reject what they rejected, in the same order, with the same words.

tests/golden/search_rejections.json (make_golden_search_rejections.py, written from the library of the commit before the
search host code moved to one call record) holds, for each of the eleven entry points, a base call that is valid except for
a workspace of 0 bytes, its single faults, and the (return code, message) of every fault alone and of every two at once;
and the sizes the families' sizing functions return on a grid of shapes.  Both are replayed against the built library.

Every call is made with addresses that are no memory.  A regression that let one through would launch on them, so the
module skips itself where a HIP device is visible: its place is the build machine, where such a call ends in the runtime.
"""
import importlib.util
import itertools
import json
import os

import pytest

from sessionsimilaritysearch_amd import _lib

HERE = os.path.dirname(os.path.abspath(__file__))


def _generator():
    spec = importlib.util.spec_from_file_location("make_golden_search_rejections",
                                                  os.path.join(HERE, "golden", "make_golden_search_rejections.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


GEN = _generator()
with open(GEN.FIXTURE) as _f:
    GOLDEN = json.load(_f)


def _device_visible():
    import torch
    return torch.cuda.is_available()


pytestmark = pytest.mark.skipif(_device_visible(), reason="calls with made-up addresses: never where a call let through would launch")


def test_the_fixture_covers_the_eleven_entry_points_and_their_sizing_functions():
    assert list(GOLDEN["entry_points"]) == list(GEN.ENTRY_POINTS) and len(GEN.ENTRY_POINTS) == 11
    assert list(GOLDEN["sizes"]) == GEN.SIZING
    for name, entry in GOLDEN["entry_points"].items():
        assert list(entry["base"]) == list(_lib.PARAMS[name]), name
        assert entry["base"]["workspace_bytes"] == 0, name
        assert len(entry["results"]) == sum(1 for _ in GEN.cases(entry)) > len(entry["faults"]), name
    assert all(rc in (-1, -2) for rc, _ in GOLDEN["messages"])


@pytest.mark.parametrize("name", list(GEN.ENTRY_POINTS))
def test_every_rejection_is_the_recorded_one(name):
    entry = GOLDEN["entry_points"][name]
    wrong = []
    for over, want in zip(GEN.cases(entry), entry["results"]):
        got = GEN.answer(_lib, name, entry["base"] | over)
        if got != GOLDEN["messages"][want]:
            wrong.append((over, got, GOLDEN["messages"][want]))
    assert not wrong, f"{len(wrong)} of {len(entry['results'])} cases differ; the first: {wrong[:3]}"


@pytest.mark.parametrize("fn", GEN.SIZING)
def test_sizing_functions_return_the_recorded_bytes(fn):
    rec = GOLDEN["sizes"][fn]
    assert [p for p, _ in rec["axes"]] == list(_lib.PARAMS[fn])
    call = getattr(_lib.lib(), fn)
    got = [call(*args) for args in itertools.product(*[v for _, v in rec["axes"]])]
    assert len(got) == len(rec["bytes"]) and any(rec["bytes"])
    wrong = [(args, g, w) for args, g, w in zip(itertools.product(*[v for _, v in rec["axes"]]), got, rec["bytes"]) if g != w]
    assert not wrong, wrong[:5]
