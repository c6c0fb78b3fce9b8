"""What the C-ABI tests share: the entry-point names a header of include/ declares, read by a regex of its own (not by
``_lib``'s reader, which these tests check), and the type names tests/golden/abi_signatures.json is written in."""
import ctypes
import json
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
INCLUDE = os.path.join(ROOT, "include")
SNAPSHOT = os.path.join(ROOT, "tests", "golden", "abi_signatures.json")
_TYPE_NAMES = ("c_void_p", "c_char_p", "c_int", "c_int64", "c_size_t", "c_float", "c_double")   # c_int32 is c_int


def declared(header):
    """The sorted ``sss_*`` names followed by ``(`` in include/<header>, comments of both styles stripped."""
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(INCLUDE, header)).read(), flags=re.S)
    text = re.sub(r"//[^\n]*", "", text)
    return sorted(set(re.findall(r"\b(sss_\w+)\s*\(", text)))


def headers():
    return sorted(f for f in os.listdir(INCLUDE) if f.endswith(".h"))


def type_name(t):
    """A ctypes type as the snapshot spells it: ``c_int64``, or ``HgtSlot[2]`` for an array of a ``Structure``."""
    if issubclass(t, ctypes.Array):
        return f"{t._type_.__name__}[{t._length_}]"
    return next(n for n in _TYPE_NAMES if getattr(ctypes, n) is t)


def signature(restype, argtypes):
    return [type_name(restype), [type_name(a) for a in argtypes]]


def struct_record(cls):
    return {"fields": [[n, type_name(t)] for n, t in cls._fields_], "sizeof": ctypes.sizeof(cls)}


def snapshot():
    with open(SNAPSHOT) as f:
        return json.load(f)
