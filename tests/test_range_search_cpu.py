"""Range search C ABI without a device: the symbols are declared, exported and bound; workspace sizes are sane; bad
arguments and short workspaces are rejected on the host (return codes, sss_last_error) before any HIP call."""
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RANGE_SYMBOLS = {"sss_range_search_workspace_bytes", "sss_range_search_count", "sss_range_search_fill",
                 "sss_range_search_exhaustive_workspace_bytes", "sss_range_search_exhaustive_count",
                 "sss_range_search_exhaustive_fill"}
CAP = 8192              # rows a query's fused scan may keep


@pytest.fixture(scope="module")
def L():
    import sessionsimilaritysearch_amd as pkg
    return pkg.lib()


def test_range_symbols_declared_exported_and_bound(L):
    import sessionsimilaritysearch_amd as pkg
    hdr = open(os.path.join(ROOT, "include", "sss.h")).read()
    declared = set(re.findall(r"\b(sss_[a-z0-9_]+)\s*\(", hdr))
    assert RANGE_SYMBOLS <= declared
    assert RANGE_SYMBOLS <= set(pkg.exported_symbols())
    for name in RANGE_SYMBOLS:
        assert getattr(L, name).argtypes is not None


def test_range_workspace_sizes(L):
    # fused: every scan shape of the threshold rung, ~cap x 8 bytes per query, 256-byte granular
    for scan, d in ((0, 64), (0, 128), (0, 256), (1, 128), (1, 256), (1, 512), (2, 64), (2, 256), (3, 128), (3, 512)):
        for nq, n in ((1, 1), (7, 1_000_000), (4096, 1_000_000)):
            b = L.sss_range_search_workspace_bytes(nq, n, d, scan)
            assert b % 256 == 0 and nq * CAP * 8 <= b <= nq * (CAP * 8 + 16) + 1024, (scan, d, nq, n, b)
    for scan, d in ((0, 96), (0, 512), (1, 64), (3, 64), (0, 1600)):          # no scan of that row size
        assert L.sss_range_search_workspace_bytes(16, 100_000, d, scan) == 0
    assert L.sss_range_search_workspace_bytes(0, 100, 128, 0) == 0
    assert L.sss_range_search_workspace_bytes(4, 0, 128, 0) == 0
    # exhaustive: the scores of every selected query (4 n bytes each) plus the per-slab counters
    for nsel, n in ((1, 1), (8, 100_000), (256, 1_000_000)):
        b = L.sss_range_search_exhaustive_workspace_bytes(nsel, n)
        assert nsel * n * 4 <= b <= nsel * n * 4 + nsel * (n // 4096 + 8) * 4 + 1024, (nsel, n, b)
    assert L.sss_range_search_exhaustive_workspace_bytes(0, 10) == 0
    assert L.sss_range_search_exhaustive_workspace_bytes(3, 0) == 0


def test_range_fused_entry_points_reject_bad_arguments(L):
    P = 1 << 20                                     # a 256-byte aligned stand-in for device pointers: never dereferenced
    ws = L.sss_range_search_workspace_bytes(4, 100, 128, 3)

    def count(q=P, nq=4, corpus=P, dtype=0, image=P, scan=3, shift=0, resid=0.0, n=100, d=128, radius=P, cmax=1.0,
              counts=P, status=P, w=P, wb=ws):
        return L.sss_range_search_count(q, nq, corpus, dtype, image, scan, shift, resid, n, d, radius, cmax, counts, status,
                                        w, wb, 0)

    assert count(nq=0) == -1 and count(n=0) == -1
    assert count(image=0) == -1 and b"scan image" in L.sss_last_error()
    assert count(image=P + 8) == -1                                      # not 16-byte aligned
    assert count(dtype=2) == -1                                          # not a corpus dtype
    assert count(dtype=1) == -1                                          # f16 image of a bf16 index
    assert count(d=96) == -1 and count(scan=0, d=512) == -1              # no scan of that row size
    assert count(radius=0) == -1 and b"radius" in L.sss_last_error()
    assert count(counts=0) == -1 and count(status=0) == -1
    assert count(shift=999) == -1 and count(resid=-1.0) == -1
    assert count(w=P + 64) == -1                                         # workspace not 256-byte aligned
    assert count(wb=ws - 256) == -2 and b"workspace" in L.sss_last_error()
    assert count(w=0) == -2

    fb = 4 * CAP * 8                                                     # less than the fill needs (head + candidates)
    assert L.sss_range_search_fill(0, P, 0, P, P, P, ws, 0) == -1
    assert L.sss_range_search_fill(4, 0, 0, P, P, P, ws, 0) == -1 and b"lims" in L.sss_last_error()
    assert L.sss_range_search_fill(4, P, 0, P, P, P + 64, ws, 0) == -1
    assert L.sss_range_search_fill(4, P, 0, P, P, P, fb, 0) == -2
    assert L.sss_range_search_fill(4, P, 0, P, P, 0, ws, 0) == -2


def test_range_exhaustive_entry_points_reject_bad_arguments(L):
    P = 1 << 20
    ws = L.sss_range_search_exhaustive_workspace_bytes(4, 1000)

    def count(q=P, qsel=P, nsel=4, corpus=P, n=1000, d=96, dtype=0, metric=1, radius=P, counts=P, w=P, wb=ws):
        return L.sss_range_search_exhaustive_count(q, qsel, nsel, corpus, n, d, dtype, metric, radius, counts, w, wb, 0)

    assert count(nsel=0) == -1 and count(n=0) == -1 and count(nsel=65536) == -1
    assert count(d=6) == -1 and count(dtype=1, d=12) == -1 and count(dtype=3) == -1
    assert count(metric=2) == -1
    assert count(qsel=0) == -1 and count(radius=0) == -1 and count(counts=0) == -1
    assert count(w=P + 16) == -1
    assert count(wb=ws - 1) == -2 and b"workspace" in L.sss_last_error()

    def fill(qsel=P, nsel=4, n=1000, metric=0, radius=P, lims=P, w=P, wb=ws):
        return L.sss_range_search_exhaustive_fill(qsel, nsel, n, metric, radius, lims, 0, P, P, w, wb, 0)

    assert fill(nsel=0) == -1 and fill(metric=-1) == -1 and fill(radius=0) == -1
    assert fill(lims=0) == -1 and b"lims" in L.sss_last_error()
    assert fill(wb=16) == -2
