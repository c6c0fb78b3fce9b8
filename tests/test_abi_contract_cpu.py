"""CPU side of the C ABI contract tests (tests/test_abi_contract_gpu.py): every entry point declared in
include/sss.h is either covered there by a guarded call or exempt here with a reason, and sss_last_error is
thread-local."""
import ast
import os
import re
import sys
import threading

from sessionsimilaritysearch_amd import _lib

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
from abi import declared  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GPU_MODULE = os.path.join(ROOT, "tests", "test_abi_contract_gpu.py")

# Host-only helpers and diagnostics: nothing is written to device buffers the caller owns.
EXEMPT = {
    "sss_version": "host-only: returns the library version",
    "sss_last_error": "host-only: the thread-local message (tested here)",
    "sss_f16_shift": "host-only helper: the shift for a largest magnitude",
    "sss_profile_enable": "measurement aid: toggles the per-device event bracketing",
    "sss_profile_read": "measurement aid: reads the host-side timing counters",
    "sss_scan_boot_expired": "diagnostic counter; read (not asserted) by the concurrency test",
}
_EXEMPT_PATTERNS = (r".*_bytes", r".*_capacity", r"sss_graph_scratch_ints")   # sizing queries: host arithmetic only


def _gpu_module():
    tree = ast.parse(open(GPU_MODULE).read())
    table = next(ast.literal_eval(n.value) for n in tree.body
                 if isinstance(n, ast.Assign) and any(getattr(t, "id", None) == "COVERAGE" for t in n.targets))
    tests = {n.name for n in tree.body if isinstance(n, ast.FunctionDef) and n.name.startswith("test_")}
    return table, tests


def _exempt(name):
    return name in EXEMPT or any(re.fullmatch(p, name) for p in _EXEMPT_PATTERNS)


def test_every_entry_point_is_covered_or_exempt():
    names = declared("sss.h")
    assert len(names) > 50
    table, tests = _gpu_module()
    missing = [n for n in names if n not in table and not _exempt(n)]
    assert not missing, f"entry points of include/sss.h with no guarded test and no exemption: {missing}"
    both = [n for n in names if n in table and _exempt(n)]
    assert not both, f"covered and exempt at once: {both}"
    stale = sorted(set(table) - set(names)) + sorted(set(EXEMPT) - set(names))
    assert not stale, f"coverage / exemption entries for names the header does not declare: {stale}"
    unknown = sorted({t for t in table.values() if t not in tests})
    assert not unknown, f"coverage table names tests that do not exist: {unknown}"
    assert all(EXEMPT.values())


def test_header_and_ctypes_binding_declare_the_same_entry_points():
    assert declared("sss.h") == _lib.exported_symbols()


def test_last_error_is_thread_local():
    """Two threads fail two different argument checks (caught before any device work: null pointers only) and each
    reads back its own message."""
    L = _lib.lib()
    start, got = threading.Barrier(2), {}

    def fused_nq0():
        start.wait()
        rc = L.sss_ip_topk(0, 0, 0, 1000, 128, 10, 0, 0, 1.0, 0, 0, 0, 0, 0, 0, 0, 0, 0)
        start.wait()
        got["ip_topk"] = (rc, L.sss_last_error())

    def hamming_k0():
        start.wait()
        rc = L.sss_hamming_topk(0, 10, 0, 1000, 16, 0, 0, 0, 0, 0, 0, 0, 0)
        start.wait()
        got["hamming"] = (rc, L.sss_last_error())
    threads = [threading.Thread(target=fused_nq0), threading.Thread(target=hamming_k0)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert got["ip_topk"][0] == -1 and got["hamming"][0] == -1
    assert got["ip_topk"][1].startswith(b"ip_topk:"), got
    assert got["hamming"][1].startswith(b"hamming_topk:"), got
    assert got["ip_topk"][1] != got["hamming"][1]
