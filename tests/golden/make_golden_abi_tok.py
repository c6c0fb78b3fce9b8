"""Writes tests/golden/abi_signatures_tok.json from the binding ``_lib`` holds of include/tok/:
    python tests/golden/make_golden_abi_tok.py

The same record as tests/golden/abi_signatures.json (make_golden_abi.py), for the headers of include/tok/: per header and
entry point [restype, [argtypes]] in the type names of tests/helpers/abi.py plus ``c_uint32`` (``type_name`` below; a
``uint64_t`` is the ctypes class of ``size_t`` on this ABI and is spelled ``c_size_t``), and the parameter names.  No header
there declares a struct.  tests/test_wordpiece_cpu.py holds the reader and the loaded library to this file, so a header edit that
moves the ABI fails until the file is regenerated ON PURPOSE: run this, read the diff of the .json, and commit it with the
header.
"""
import ctypes
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), os.path.join(os.path.dirname(HERE), "helpers")]

import abi  # noqa: E402

SNAPSHOT = os.path.join(HERE, "abi_signatures_tok.json")


def type_name(t):
    return "c_uint32" if t is ctypes.c_uint32 else abi.type_name(t)


def signature(restype, argtypes):
    return [type_name(restype), [type_name(a) for a in argtypes]]


def record(lib_module):
    return {"functions": {h: {n: signature(*sig) for n, sig in sorted(table.items())}
                          for h, table in sorted(lib_module.TOK_HEADERS.items())},
            "params": {n: list(p) for n, p in sorted(lib_module.TOK_PARAMS.items())}}


def dump(rec, path=SNAPSHOT):
    """One entry point per line: a change of one signature is a one-line diff."""
    out = ['{"functions": {']
    for hi, (h, table) in enumerate(rec["functions"].items()):
        out.append(f' {json.dumps(h)}: {{')
        out += [f'  {json.dumps(n)}: {json.dumps(sig)}{"," if i + 1 < len(table) else ""}' for i, (n, sig) in enumerate(table.items())]
        out.append(' }' + ("," if hi + 1 < len(rec["functions"]) else ""))
    out.append('},\n"params": {')
    out += [f' {json.dumps(n)}: {json.dumps(p)}{"," if i + 1 < len(rec["params"]) else ""}' for i, (n, p) in enumerate(rec["params"].items())]
    out.append('}}')
    with open(path, "w") as f:
        f.write("\n".join(out) + "\n")


if __name__ == "__main__":
    from sessionsimilaritysearch_amd import _lib
    dump(record(_lib))
    print("wrote", SNAPSHOT)
