"""Writes tests/golden/abi_signatures.json from the binding ``_lib`` holds:  python tests/golden/make_golden_abi.py

For every header of include/ and every entry point, [restype, [argtypes]]; for every argument struct, its (field, type)
list and sizeof -- all as the type names of tests/helpers/abi.py.  tests/test_abi_snapshot_cpu.py holds the reader of
``_lib`` and the loaded library to this file, so a header edit that moves the ABI fails until the file is regenerated ON
PURPOSE: run this, read the diff of the .json, and commit it with the header.

Provenance: the committed file was first written by this script from the hand-typed signature tables and ``Structure``
field lists ``_lib`` held before it read the headers, so the derived binding is pinned to the one it replaced.
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), os.path.join(os.path.dirname(HERE), "helpers")]

import abi  # noqa: E402


def record(lib_module):
    return {"functions": {h: {n: abi.signature(*sig) for n, sig in sorted(table.items())}
                          for h, table in sorted(lib_module.HEADERS.items())},
            "structs": {n: abi.struct_record(cls) for n, cls in sorted(lib_module.STRUCTS.items())}}


def dump(rec, path=abi.SNAPSHOT):
    """One entry point per line: a change of one signature is a one-line diff."""
    out = ['{"functions": {']
    for hi, (h, table) in enumerate(rec["functions"].items()):
        out.append(f' {json.dumps(h)}: {{')
        out += [f'  {json.dumps(n)}: {json.dumps(sig)}{"," if i + 1 < len(table) else ""}' for i, (n, sig) in enumerate(table.items())]
        out.append(' }' + ("," if hi + 1 < len(rec["functions"]) else ""))
    out.append('},\n"structs": {')
    out += [f' {json.dumps(n)}: {json.dumps(s)}{"," if i + 1 < len(rec["structs"]) else ""}' for i, (n, s) in enumerate(rec["structs"].items())]
    out.append('}}')
    with open(path, "w") as f:
        f.write("\n".join(out) + "\n")


if __name__ == "__main__":
    from sessionsimilaritysearch_amd import _lib
    dump(record(_lib))
    print("wrote", abi.SNAPSHOT)
