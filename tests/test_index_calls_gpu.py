"""Which entry points of libsss a ``FlatIndex`` calls, and in what order: one ``add`` and two ``search`` calls per scan
family, with the library object wrapped in a recorder.  The name sequences are literals taken from the index before its
call paths were folded into one, so a change of entry point, an extra image build or a rebuild on the second search
shows as a difference; every case's (D, I) also equals the oracle's exact result bit for bit."""
import contextlib
import functools

import numpy as np
import pytest
import torch

from oracle import search_ref as sr

pytestmark = pytest.mark.gpu


class Recorder:
    """Stands in for the ctypes library object: notes the name of every ``sss_*`` function called through it."""

    def __init__(self, lib):
        self._lib, self.names = lib, []

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if not name.startswith("sss_"):
            return fn

        def call(*args):
            self.names.append(name)
            return fn(*args)
        return call


@contextlib.contextmanager
def recording():
    from sessionsimilaritysearch_amd import _lib
    real = _lib.lib
    rec = Recorder(real())
    _lib.lib = lambda: rec
    try:
        yield rec
    finally:
        _lib.lib = real


# name: (d, metric, dtype, scan, pad_scan, k, rows)
CASES = {
    "f32-ip-128-auto": (128, "ip", "f32", "auto", False, 10, "random"),
    "f32-ip-128-split": (128, "ip", "f32", "split", False, 10, "random"),
    "f32-ip-128-f32": (128, "ip", "f32", "f32", False, 10, "random"),
    "f32-l2-128": (128, "l2", "f32", None, False, 10, "random"),
    "f32-ip-200-pad": (200, "ip", "f32", None, True, 10, "random"),
    "f32-l2-200-pad": (200, "l2", "f32", None, True, 10, "random"),
    "f32-ip-320-long": (320, "ip", "f32", None, False, 10, "random"),
    "f32-l2-320-long": (320, "l2", "f32", None, False, 10, "random"),
    "bf16-ip-256": (256, "ip", "bf16", None, False, 10, "random"),
    "f16-ip-256": (256, "ip", "f16", None, False, 10, "random"),
    "i8-ip-256": (256, "ip", "i8", None, False, 10, "random"),
    "f32-ip-96-exhaustive": (96, "ip", "f32", None, False, 10, "random"),
    "f32-ip-128-k501": (128, "ip", "f32", None, False, 501, "random"),
    "rung-ip": (128, "ip", "f32", None, False, 10, "rung"),
    "rung-l2": (128, "l2", "f32", None, False, 10, "rung"),
    "ties-ip": (128, "ip", "f32", None, False, 10, "ties"),
    "ties-l2": (128, "l2", "f32", None, False, 10, "ties"),
    "overflow-ip": (128, "ip", "f32", None, False, 10, "overflow"),
    "overflow-l2": (128, "l2", "f32", None, False, 10, "overflow"),
}


@functools.lru_cache(maxsize=None)
def _data(d, dtype, rows):
    """(corpus, queries) as float32 arrays holding values the stored type represents exactly."""
    rng = np.random.default_rng(d + len(dtype) + len(rows))
    n = 10_000 if rows == "overflow" else 3000
    if dtype == "i8":
        return (rng.integers(-127, 128, (n, d)).astype(np.float32), rng.integers(-127, 128, (8, d)).astype(np.float32))
    c = sr.normalize(rng.standard_normal((n, d)).astype(np.float32)).astype(np.float32)
    q = sr.normalize(rng.standard_normal((8, d)).astype(np.float32)).astype(np.float32)
    if rows == "rung":                  # 20 identical rows and a query equal to them: a tie across rank 10 (which the
        # fused scan proves by itself: its candidate list holds all 20, so the recorded sequence has no rung call)
        c[:20] = c[0]
        q[3] = c[0]
    if rows == "ties":                  # 2000 identical rows: more than a fused scan keeps, so the query stays unproven;
        # fewer than the rung's capacity, so the rung resolves it
        c[:2000] = c[0]
        q[3] = c[0]
    if rows == "overflow":              # more tied rows than the rung's 8192 candidates
        c[1000:] = c[1000]
        q[3] = c[1000]
    if dtype != "f32":
        t = torch.bfloat16 if dtype == "bf16" else torch.float16
        c, q = (torch.from_numpy(x).to(t).float().numpy() for x in (c, q))
    return c, q


@functools.lru_cache(maxsize=None)
def _exact(d, metric, dtype, k, rows):
    c, q = _data(d, dtype, rows)
    if metric == "l2":
        return sr.topk_from_scores(sr.canonical_l2(q, c), k, largest=False)
    return sr.search_exact(q, c, k)


def run_case(name, device):
    """(names recorded during add, during the first search, during the second; the two results)."""
    from sessionsimilaritysearch_amd.index import FlatIndex
    d, metric, dtype, scan, pad, k, rows = CASES[name]
    c, q = _data(d, dtype, rows)
    idx = FlatIndex(d, metric, device, dtype=dtype, scan=scan, pad_scan=pad)
    seen, results = [], []
    with recording() as rec:
        for step in (lambda: idx.add(c), lambda: idx.search(q, k), lambda: idx.search(q, k)):
            del rec.names[:]
            out = step()
            seen.append(list(rec.names))
            results.append(out)
    return seen, results[1:]


# Recorded on commit 2253765 (the parent of the change that introduced routing.py and the one call path of index.py),
# by this file's recorder on an MI355X -- not from the code under test.
EXPECTED = {
    "bf16-ip-256": {
        "add": "sss_f32_to_bf16 sss_row_norm_max",
        "search": "sss_f32_to_bf16 sss_ip_topk_workspace_bytes sss_ip_topk_state_bytes sss_ip_topk",
        "again": "sss_f32_to_bf16 sss_ip_topk_workspace_bytes sss_ip_topk_state_bytes sss_ip_topk",
    },
    "f16-ip-256": {
        "add": "sss_row_norm_max",
        "search": "sss_ip_topk_workspace_bytes sss_ip_topk_state_bytes sss_ip_topk",
        "again": "sss_ip_topk_workspace_bytes sss_ip_topk_state_bytes sss_ip_topk",
    },
    "f32-ip-128-auto": {
        "add": "sss_row_norm_max",
        "search": ("sss_abs_max sss_f16_shift sss_scale_f16 sss_f16_resid_max sss_ip_topk_f16_workspace_bytes "
                  "sss_ip_topk_state_bytes sss_ip_topk_f16"),
        "again": "sss_ip_topk_f16_workspace_bytes sss_ip_topk_state_bytes sss_ip_topk_f16",
    },
    "f32-ip-128-f32": {
        "add": "sss_row_norm_max",
        "search": "sss_ip_topk_workspace_bytes sss_ip_topk_state_bytes sss_ip_topk",
        "again": "sss_ip_topk_workspace_bytes sss_ip_topk_state_bytes sss_ip_topk",
    },
    "f32-ip-128-k501": {
        "add": "sss_row_norm_max",
        "search": "sss_ip_topk_exhaustive_workspace_bytes sss_ip_topk_exhaustive",
        "again": "sss_ip_topk_exhaustive_workspace_bytes sss_ip_topk_exhaustive",
    },
    "f32-ip-128-split": {
        "add": "sss_row_norm_max",
        "search": "sss_split_bf16 sss_ip_topk_workspace_bytes sss_ip_topk_state_bytes sss_ip_topk_split",
        "again": "sss_ip_topk_workspace_bytes sss_ip_topk_state_bytes sss_ip_topk_split",
    },
    "f32-ip-200-pad": {
        "add": "sss_row_norm_max",
        "search": ("sss_abs_max sss_f16_shift sss_pad_scale_f16 sss_pad_f16_resid_max sss_pad_topk_workspace_bytes "
                  "sss_ip_topk_state_bytes sss_pad_rows_f32 sss_pad_topk"),
        "again": "sss_pad_topk_workspace_bytes sss_ip_topk_state_bytes sss_pad_rows_f32 sss_pad_topk",
    },
    "f32-ip-320-long": {
        "add": "sss_row_norm_max",
        "search": ("sss_abs_max sss_f16_shift sss_scale_f16 sss_f16_resid_max sss_ip_topk_long_workspace_bytes "
                  "sss_ip_topk_long"),
        "again": "sss_ip_topk_long_workspace_bytes sss_ip_topk_long",
    },
    "f32-ip-96-exhaustive": {
        "add": "sss_row_norm_max",
        "search": "sss_ip_topk_exhaustive_workspace_bytes sss_ip_topk_exhaustive",
        "again": "sss_ip_topk_exhaustive_workspace_bytes sss_ip_topk_exhaustive",
    },
    "f32-l2-128": {
        "add": "sss_row_norm_max",
        "search": ("sss_abs_max sss_f16_shift sss_scale_f16 sss_f16_resid_max sss_l2_row_bias "
                  "sss_l2_topk_workspace_bytes sss_ip_topk_state_bytes sss_l2_topk"),
        "again": "sss_l2_topk_workspace_bytes sss_ip_topk_state_bytes sss_l2_topk",
    },
    "f32-l2-200-pad": {
        "add": "sss_row_norm_max",
        "search": ("sss_abs_max sss_f16_shift sss_pad_scale_f16 sss_pad_f16_resid_max sss_l2_row_bias "
                  "sss_pad_topk_workspace_bytes sss_ip_topk_state_bytes sss_pad_rows_f32 sss_pad_topk"),
        "again": "sss_pad_topk_workspace_bytes sss_ip_topk_state_bytes sss_pad_rows_f32 sss_pad_topk",
    },
    "f32-l2-320-long": {
        "add": "sss_row_norm_max",
        "search": ("sss_abs_max sss_f16_shift sss_scale_f16 sss_f16_resid_max sss_l2_row_bias "
                  "sss_l2_topk_long_workspace_bytes sss_l2_topk_long"),
        "again": "sss_l2_topk_long_workspace_bytes sss_l2_topk_long",
    },
    "i8-ip-256": {
        "add": "sss_row_norm_max",
        "search": "sss_ip_topk_workspace_bytes sss_ip_topk_state_bytes sss_ip_topk",
        "again": "sss_ip_topk_workspace_bytes sss_ip_topk_state_bytes sss_ip_topk",
    },
    "overflow-ip": {
        "add": "sss_row_norm_max",
        "search": ("sss_abs_max sss_f16_shift sss_scale_f16 sss_f16_resid_max sss_ip_topk_f16_workspace_bytes "
                  "sss_ip_topk_state_bytes sss_ip_topk_f16 sss_ip_topk_threshold_workspace_bytes sss_ip_topk_threshold "
                  "sss_ip_topk_exhaustive_workspace_bytes sss_ip_topk_exhaustive_lb"),
        "again": ("sss_ip_topk_f16_workspace_bytes sss_ip_topk_state_bytes sss_ip_topk_f16 "
                  "sss_ip_topk_threshold_workspace_bytes sss_ip_topk_threshold sss_ip_topk_exhaustive_workspace_bytes "
                  "sss_ip_topk_exhaustive_lb"),
    },
    "overflow-l2": {
        "add": "sss_row_norm_max",
        "search": ("sss_abs_max sss_f16_shift sss_scale_f16 sss_f16_resid_max sss_l2_row_bias "
                  "sss_l2_topk_workspace_bytes sss_ip_topk_state_bytes sss_l2_topk "
                  "sss_l2_topk_threshold_workspace_bytes sss_l2_topk_threshold sss_ip_topk_exhaustive_workspace_bytes "
                  "sss_ip_topk_exhaustive"),
        "again": ("sss_l2_topk_workspace_bytes sss_ip_topk_state_bytes sss_l2_topk "
                  "sss_l2_topk_threshold_workspace_bytes sss_l2_topk_threshold sss_ip_topk_exhaustive_workspace_bytes "
                  "sss_ip_topk_exhaustive"),
    },
    "rung-ip": {
        "add": "sss_row_norm_max",
        "search": ("sss_abs_max sss_f16_shift sss_scale_f16 sss_f16_resid_max sss_ip_topk_f16_workspace_bytes "
                  "sss_ip_topk_state_bytes sss_ip_topk_f16"),
        "again": "sss_ip_topk_f16_workspace_bytes sss_ip_topk_state_bytes sss_ip_topk_f16",
    },
    "rung-l2": {
        "add": "sss_row_norm_max",
        "search": ("sss_abs_max sss_f16_shift sss_scale_f16 sss_f16_resid_max sss_l2_row_bias "
                  "sss_l2_topk_workspace_bytes sss_ip_topk_state_bytes sss_l2_topk"),
        "again": "sss_l2_topk_workspace_bytes sss_ip_topk_state_bytes sss_l2_topk",
    },
    "ties-ip": {
        "add": "sss_row_norm_max",
        "search": ("sss_abs_max sss_f16_shift sss_scale_f16 sss_f16_resid_max sss_ip_topk_f16_workspace_bytes "
                  "sss_ip_topk_state_bytes sss_ip_topk_f16 sss_ip_topk_threshold_workspace_bytes sss_ip_topk_threshold"),
        "again": ("sss_ip_topk_f16_workspace_bytes sss_ip_topk_state_bytes sss_ip_topk_f16 "
                  "sss_ip_topk_threshold_workspace_bytes sss_ip_topk_threshold"),
    },
    "ties-l2": {
        "add": "sss_row_norm_max",
        "search": ("sss_abs_max sss_f16_shift sss_scale_f16 sss_f16_resid_max sss_l2_row_bias "
                  "sss_l2_topk_workspace_bytes sss_ip_topk_state_bytes sss_l2_topk "
                  "sss_l2_topk_threshold_workspace_bytes sss_l2_topk_threshold"),
        "again": ("sss_l2_topk_workspace_bytes sss_ip_topk_state_bytes sss_l2_topk "
                  "sss_l2_topk_threshold_workspace_bytes sss_l2_topk_threshold"),
    },
}


@pytest.mark.parametrize("name", sorted(CASES))
def test_entry_points_called_and_results(cuda, name):
    d, metric, dtype, scan, pad, k, rows = CASES[name]
    seen, results = run_case(name, cuda)
    print(name, seen)
    assert [tuple(s) for s in seen] == [tuple(EXPECTED[name][step].split()) for step in ("add", "search", "again")]
    Dr, Ir = _exact(d, metric, dtype, k, rows)
    for D, I in results:
        assert np.array_equal(I, Ir) and np.array_equal(D, Dr)
