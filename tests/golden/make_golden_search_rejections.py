"""Writes tests/golden/search_rejections.json from the built libsss.so:  python tests/golden/make_golden_search_rejections.py

What the eleven scanning search entry points (sss_ip_topk, _split, _f16, sss_l2_topk, sss_pad_topk, the three
*_topk_threshold, sss_range_search_count, sss_ip_topk_long, sss_l2_topk_long) answer to a call they must reject: the return
code and the message of sss_last_error, byte for byte.  Per entry point a base call that is valid except for a workspace of
0 bytes, a list of single faults (a count at 0, n at the 2^31 limit, a pointer null or misaligned, a bad d / d_row /
d_scan / dtype / scan_dtype, shift 161 and residual -1 on an f16 image, k one past its limit, the state null, misaligned
and short, the workspace null, misaligned, one byte short and 0 bytes), every fault alone and every two of them at once:
the pairs pin the ORDER of the checks.  A "fault" an entry point accepts (a null pointer it does not require, a dtype it
pairs) is kept: the call then ends at the empty workspace, which pins that the value IS accepted.  All addresses are made
up and never dereferenced; no call reaches a device.  A case that is not rejected with -1 or -2 is refused, not recorded.

Also the sizes the families' *_workspace_bytes / sss_ip_topk_state_bytes return on a small grid of shapes.

Every message is stored once (``messages``: [rc, text]) and referred to by index.  tests/test_search_rejections_cpu.py
replays the file against the library it finds.  Provenance: the committed file was written from the library of the commit
BEFORE the search host code moved to one call record (csrc/scan.h: SearchCall), so that refactor is held to what the
positional code answered; regenerate it ON PURPOSE only, when a rule or a message is meant to change, and read the diff.
"""
import ctypes
import itertools
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(os.path.dirname(HERE))]

FIXTURE = os.path.join(HERE, "search_rejections.json")
A = 1 << 20                             # a 256-byte aligned address that is no memory

# entry point -> (what its base call differs in from BASE, the sizing call of its workspace, its largest k)
ENTRY_POINTS = {
    "sss_ip_topk": ({}, ("sss_ip_topk_workspace_bytes", {}), 500),
    "sss_ip_topk_split": ({}, ("sss_l2_topk_workspace_bytes", {"scan_dtype": 2}), 500),
    "sss_ip_topk_f16": ({}, ("sss_ip_topk_f16_workspace_bytes", {}), 500),
    "sss_l2_topk": ({}, ("sss_l2_topk_workspace_bytes", {}), 500),
    "sss_pad_topk": ({}, ("sss_pad_topk_workspace_bytes", {}), 500),
    "sss_ip_topk_threshold": ({}, ("sss_ip_topk_threshold_workspace_bytes", {}), 8192),
    "sss_l2_topk_threshold": ({}, ("sss_l2_topk_threshold_workspace_bytes", {}), 8192),
    "sss_pad_topk_threshold": ({}, ("sss_pad_topk_threshold_workspace_bytes", {}), 8192),
    "sss_range_search_count": ({}, ("sss_range_search_workspace_bytes", {}), None),
    "sss_ip_topk_long": ({"d": 1600}, ("sss_ip_topk_long_workspace_bytes", {}), 1024),
    "sss_l2_topk_long": ({"d": 1600}, ("sss_l2_topk_long_workspace_bytes", {}), 1024),
}
LONG = ("sss_ip_topk_long", "sss_l2_topk_long")
# these reject a null workspace whatever its size; the others would take a null workspace of enough bytes to the device
NULL_WORKSPACE_CHECKED = ("sss_pad_topk", "sss_pad_topk_threshold", "sss_l2_topk_threshold", "sss_range_search_count")
BASE = dict(q=A, nq=8, qsel=A, nsel=8, corpus=A, scan_image=A, dtype=0, scan_dtype=0, corpus_shift=0, corpus_resid_norm=0.0, bias=A,
            radius=A, n=1000, d=256, d_row=200, d_scan=256, k=10, id_offset=0, corpus_max_norm=1.0, D_out=A, I_out=A, status=A,
            counts=A, unproven_count=A, state=A, state_bytes=1 << 30, workspace=A, workspace_bytes=0, stream=0)

# the sizing functions and the grid each is recorded on (the product of its parameters' values below)
SIZING = ["sss_ip_topk_state_bytes", "sss_ip_topk_workspace_bytes", "sss_ip_topk_f16_workspace_bytes", "sss_l2_topk_workspace_bytes",
          "sss_pad_topk_workspace_bytes", "sss_ip_topk_threshold_workspace_bytes", "sss_l2_topk_threshold_workspace_bytes",
          "sss_pad_topk_threshold_workspace_bytes", "sss_range_search_workspace_bytes", "sss_ip_topk_long_workspace_bytes",
          "sss_l2_topk_long_workspace_bytes"]
GRID = dict(nq=[0, 1, 8, 300], nsel=[0, 1, 8, 300], n=[0, 1000, 70001], d=[64, 100, 128, 256, 1600, 4160], k=[1, 10, 500],
            dtype=[0, 1, 2, 3, 4, 5, 6], scan_dtype=[0, 1, 2, 3, 4, 5, 6], d_row=[60, 200, 202], d_scan=[64, 256, 512])


def base_of(name, params):
    return {p: ENTRY_POINTS[name][0].get(p, BASE[p]) for p in params}


def sizes_of(lib_module, name):
    """(workspace bytes, state bytes) the base call of ``name`` needs."""
    L = lib_module.lib()
    fn, fixed = ENTRY_POINTS[name][1]
    v = BASE | ENTRY_POINTS[name][0] | fixed
    return getattr(L, fn)(*[v[p] for p in lib_module.PARAMS[fn]]), L.sss_ip_topk_state_bytes(v["nq"])


def faults_of(name, params, argtypes, need, need_state):
    """[label, {parameter: value}] of every single fault of entry point ``name``."""
    F = [["workspace of 0 bytes", {}]]
    for p in ("nq", "nsel", "n", "k"):
        if p in params:
            F.append([f"{p} = 0", {p: 0}])
    F.append(["n at the limit", {"n": (1 << 31) - 1024}])
    F.append(["queries at the limit", {"nsel" if "nsel" in params else "nq": 1 << 31}])
    for p, t in zip(params, argtypes):
        if t is ctypes.c_void_p and p != "stream":
            F.append([f"{p} null", {p: 0}])
            F.append([f"{p} misaligned", {p: A + (16 if p == "workspace" else 4)}])
    if "d" in params:
        F += [[f"d = {d}", {"d": d}] for d in ((0, 100, 4160) if name in LONG else (0, 100, 512))]
    if "d_row" in params:
        F += [[f"d_row = {d}", {"d_row": d}] for d in (0, -4, 202, 260)] + [[f"d_scan = {d}", {"d_scan": d}] for d in (200, 512)]
    for p in ("dtype", "scan_dtype"):
        if p in params:
            F += [[f"{p} = {v}", {p: v}] for v in range(1, 8)]
    f16 = {"scan_dtype": 3} if "scan_dtype" in params else {}
    if "corpus_shift" in params:
        F += [["f16 image, shift 161", f16 | {"corpus_shift": 161}], ["f16 image, shift -161", f16 | {"corpus_shift": -161}],
              ["f16 image, residual -1", f16 | {"corpus_resid_norm": -1.0}]]
    if "k" in params:
        F.append(["k past its limit", {"k": ENTRY_POINTS[name][2] + 1}])
    if "state_bytes" in params:
        F.append(["state one byte short", {"state_bytes": need_state - 1}])
    F.append(["workspace one byte short", {"workspace_bytes": need - 1}])
    if name in NULL_WORKSPACE_CHECKED:
        F.append(["workspace null, its size right", {"workspace": 0, "workspace_bytes": need}])
    return F


def cases(entry):
    """The overrides of every case of one entry point's record, in the order of its ``results``: each fault alone, then
    every two faults that do not set one parameter to two values."""
    faults = [f for _, f in entry["faults"]]
    yield from faults
    for a, b in itertools.combinations(faults, 2):
        if all(a[p] == b[p] for p in set(a) & set(b)):
            yield a | b


def answer(lib_module, name, values):
    L = lib_module.lib()
    rc = lib_module.call(name, values)
    return [rc, L.sss_last_error().decode()]


def record(lib_module):
    L = lib_module.lib()
    messages, index = [], {}
    entries = {}
    for name in ENTRY_POINTS:
        params = lib_module.PARAMS[name]
        argtypes = next(t[name][1] for t in lib_module.HEADERS.values() if name in t)
        base = base_of(name, params)
        need, need_state = sizes_of(lib_module, name)
        if need <= 0:
            raise SystemExit(f"{name}: the base call's workspace size is {need}")
        entry = {"base": base, "faults": faults_of(name, params, argtypes, need, need_state), "results": []}
        for over in cases(entry):
            got = answer(lib_module, name, base | over)
            if got[0] not in (-1, -2):
                raise SystemExit(f"{name} {over}: returned {got[0]} ({got[1]!r}): not a rejection, not recorded")
            entry["results"].append(index.setdefault(tuple(got), len(index)))
        entries[name] = entry
    messages = [list(m) for m in index]
    sizes = {}
    for fn in SIZING:
        axes = [[p, GRID[p]] for p in lib_module.PARAMS[fn]]
        sizes[fn] = {"axes": axes, "bytes": [getattr(L, fn)(*args) for args in itertools.product(*[v for _, v in axes])]}
    return {"messages": messages, "entry_points": entries, "sizes": sizes}


def dump(rec, path=FIXTURE):
    """One line per message, per fault list and per result list."""
    js = lambda x: json.dumps(x, separators=(",", ":"))
    out = ['{"messages": [']
    out += [f' {js(m)}{"," if i + 1 < len(rec["messages"]) else ""}' for i, m in enumerate(rec["messages"])]
    out.append('],\n"entry_points": {')
    for i, (name, e) in enumerate(rec["entry_points"].items()):
        out += [f' {js(name)}: {{', f'  "base": {js(e["base"])},', f'  "faults": {js(e["faults"])},', f'  "results": {js(e["results"])}',
                ' }' + ("," if i + 1 < len(rec["entry_points"]) else "")]
    out.append('},\n"sizes": {')
    out += [f' {js(fn)}: {js(s)}{"," if i + 1 < len(rec["sizes"]) else ""}' for i, (fn, s) in enumerate(rec["sizes"].items())]
    out.append('}}')
    with open(path, "w") as f:
        f.write("\n".join(out) + "\n")


if __name__ == "__main__":
    from sessionsimilaritysearch_amd import _lib
    rec = record(_lib)
    dump(rec)
    print("wrote", FIXTURE, ":", sum(len(e["results"]) for e in rec["entry_points"].values()), "cases,", len(rec["messages"]), "messages")
