"""ctypes binding of libsss.so, read from the C ABI's own declarations: the headers of include/ are the one place where
an entry point's types and an argument struct's fields are written down (``HEADERS``, ``PARAMS`` and ``STRUCTS`` below
are what the reader makes of them).  The headers of include/ext/ are read the same way into tables of their own
(``EXT_HEADERS``, ``EXT_PARAMS``): families added since the listing of include/ was pinned; those of include/lowp/, the
reduced-precision entry points, into ``LOWP_HEADERS`` and ``LOWP_PARAMS``; those of include/heads/, the model's catalogue
heads, into ``HEADS_HEADERS`` and ``HEADS_PARAMS``; those of include/tok/, the tokenizer, into ``TOK_HEADERS`` and
``TOK_PARAMS``; ``lib()`` binds all five.

The product path has NO CPU fallback: if the HIP library is missing or a call fails, this
module raises.  ``build()`` compiles the library in-tree with hipcc for gfx950.
"""
from __future__ import annotations

import ctypes
import os
import re
import subprocess
from ctypes import c_char_p, c_double, c_float, c_int, c_int32, c_int64, c_size_t, c_uint32, c_uint64, c_void_p

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libsss.so")
CSRC = os.path.join(_HERE, "csrc")
INCLUDE = os.path.join(os.path.dirname(_HERE), "include")

_lib = None

# ---------------------------------------------------------------------------------------------- the header reader
# The headers are plain C in one style: no macros in declarations, these scalar types, and everything else a pointer.
_SCALARS = {"int": c_int, "int32_t": c_int32, "int64_t": c_int64, "size_t": c_size_t, "float": c_float, "double": c_double,
            "uint32_t": c_uint32, "uint64_t": c_uint64}
_DECLARATOR = re.compile(r"\s*(?:const\s+)?(\w+)\s*(\*?)\s*(\w+)\s*(?:\[(\d+)\])?\s*")
_STRUCT = re.compile(r"typedef\s+struct\s*\{(.*?)\}\s*(sss_\w+)\s*;", re.S)
_FUNCTION = re.compile(r"\b((?:const\s+)?\w+\s*\*?)\s*\b(sss_\w+)\s*\(([^()]*)\)\s*;")


def _declarator(text, where, structs=()):
    """``(name, ctypes type)`` of one parameter or struct field; ``structs``: the struct types a field may nest."""
    m = _DECLARATOR.fullmatch(text)
    if not m:
        raise ValueError(f"{where}: cannot read the declaration {text.strip()!r}")
    base, star, name, count = m.groups()
    if star:
        t = c_void_p
    elif base in _SCALARS:
        t = _SCALARS[base]
    elif base in structs:
        t = structs[base]
    else:
        raise ValueError(f"{where}: type {base!r} of {text.strip()!r} is not one this binding knows")
    return name, t * int(count) if count else t


def read_header(text, header):
    """What a header's text declares: ``({entry point: (restype, argtypes, parameter names)}, {struct: [field text]})``.
    Comments and preprocessor lines are dropped first; a type outside ``_SCALARS`` that is no pointer raises, naming the
    header and the declaration."""
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    text = re.sub(r"//[^\n]*", " ", text)
    text = re.sub(r"^[ \t]*#[^\n]*", " ", text, flags=re.M)
    structs = {name: [f for f in body.split(";") if f.strip()] for body, name in _STRUCT.findall(text)}
    functions = {}
    for ret, name, params in _FUNCTION.findall(_STRUCT.sub(" ", text)):
        where = f"{header}: {name}"
        ret = " ".join(ret.replace("*", " * ").split())
        if ret == "const char *":
            restype = c_char_p
        elif ret in _SCALARS:
            restype = _SCALARS[ret]
        else:
            raise ValueError(f"{where}: return type {ret!r} is not one this binding knows")
        args = [] if params.strip() == "void" else [_declarator(p, where) for p in params.split(",")]
        functions[name] = (restype, [t for _, t in args], tuple(n for n, _ in args))
    return functions, structs


def _read_include(directory=INCLUDE):
    headers, params, fields = {}, {}, {}
    for header in sorted(f for f in os.listdir(directory) if f.endswith(".h")):
        with open(os.path.join(directory, header)) as f:
            functions, structs = read_header(f.read(), header)
        headers[header] = {n: sig[:2] for n, sig in functions.items()}
        params.update({n: sig[2] for n, sig in functions.items()})
        fields.update({n: (header, body) for n, body in structs.items()})
    return headers, params, fields


# HEADERS: header of include/ -> {entry point: (restype, argtypes)}, what lib() binds; PARAMS: entry point -> its
# parameter names; STRUCTS: C struct name -> its ctypes.Structure below
HEADERS, PARAMS, _STRUCT_FIELDS = _read_include()
STRUCTS = {}
GRAPH_IGNORE_QUERY = 1      # SSS_GRAPH_IGNORE_QUERY of include/sss_graph.h
# the same two tables for include/ext/ (no header there declares a struct)
EXT_INCLUDE = os.path.join(INCLUDE, "ext")
EXT_HEADERS, EXT_PARAMS, _EXT_STRUCT_FIELDS = _read_include(EXT_INCLUDE)
if _EXT_STRUCT_FIELDS or set(EXT_PARAMS) & set(PARAMS):
    raise ValueError(f"include/ext/ declares a struct or repeats an entry point of include/: "
                     f"{sorted(_EXT_STRUCT_FIELDS) + sorted(set(EXT_PARAMS) & set(PARAMS))}")
# and for include/lowp/ (its entry points take the structs of include/ by pointer and declare none)
LOWP_INCLUDE = os.path.join(INCLUDE, "lowp")
LOWP_HEADERS, LOWP_PARAMS, _LOWP_STRUCT_FIELDS = _read_include(LOWP_INCLUDE)
if _LOWP_STRUCT_FIELDS or set(LOWP_PARAMS) & (set(PARAMS) | set(EXT_PARAMS)):
    raise ValueError(f"include/lowp/ declares a struct or repeats an entry point of include/ or include/ext/: "
                     f"{sorted(_LOWP_STRUCT_FIELDS) + sorted(set(LOWP_PARAMS) & (set(PARAMS) | set(EXT_PARAMS)))}")
# and for include/heads/ (sss_catalogue.h: no struct)
HEADS_INCLUDE = os.path.join(INCLUDE, "heads")
HEADS_HEADERS, HEADS_PARAMS, _HEADS_STRUCT_FIELDS = _read_include(HEADS_INCLUDE)
if _HEADS_STRUCT_FIELDS or set(HEADS_PARAMS) & (set(PARAMS) | set(EXT_PARAMS) | set(LOWP_PARAMS)):
    raise ValueError(f"include/heads/ declares a struct or repeats an entry point of include/, include/ext/ or include/lowp/: "
                     f"{sorted(_HEADS_STRUCT_FIELDS) + sorted(set(HEADS_PARAMS) & (set(PARAMS) | set(EXT_PARAMS) | set(LOWP_PARAMS)))}")
# and for include/tok/ (sss_wordpiece.h: no struct)
TOK_INCLUDE = os.path.join(INCLUDE, "tok")
TOK_HEADERS, TOK_PARAMS, _TOK_STRUCT_FIELDS = _read_include(TOK_INCLUDE)
_OLDER_PARAMS = set(PARAMS) | set(EXT_PARAMS) | set(LOWP_PARAMS) | set(HEADS_PARAMS)
if _TOK_STRUCT_FIELDS or set(TOK_PARAMS) & _OLDER_PARAMS:
    raise ValueError(f"include/tok/ declares a struct or repeats an entry point of an older include directory: "
                     f"{sorted(_TOK_STRUCT_FIELDS) + sorted(set(TOK_PARAMS) & _OLDER_PARAMS)}")


def header_constant(path, name):
    """The integer a header ``#define``s ``name`` as (``path`` below include/)."""
    with open(os.path.join(INCLUDE, path)) as f:
        m = re.search(rf"^[ \t]*#[ \t]*define[ \t]+{name}[ \t]+(-?\d+)\b", f.read(), flags=re.M)
    if not m:
        raise ValueError(f"include/{path} does not define {name} as an integer")
    return int(m.group(1))


def header_float(path, name):
    """The float32 value a header ``#define``s ``name`` as, written as a hexadecimal float literal with an ``f`` suffix."""
    with open(os.path.join(INCLUDE, path)) as f:
        m = re.search(rf"^[ \t]*#[ \t]*define[ \t]+{name}[ \t]+(-?0x[0-9a-fA-F.]+p[-+]?\d+)f\b", f.read(), flags=re.M)
    if not m:
        raise ValueError(f"include/{path} does not define {name} as a hexadecimal float32 literal")
    return float.fromhex(m.group(1))


def _c_struct(name):
    """Class decorator: the ``_fields_`` of struct ``name`` as its header declares them."""
    def bind(cls):
        header, body = _STRUCT_FIELDS[name]
        cls._fields_ = [_declarator(f, f"{header}: {name}", STRUCTS) for f in body]
        STRUCTS[name] = cls
        return cls
    return bind


@_c_struct("sss_linear_problem")
class LinearProblem(ctypes.Structure):
    """``sss_linear_problem`` of include/sss.h."""


def linear_problem(x, w, bias, y, n, m, act=0, post=None, ids=None, table=None, xcopy=None):
    """One problem of ``sss_linear_grouped``: ``y[:n, :m] = act(x w^T + bias)`` on 2-D device tensors (row strides are taken
    from them), ``post = (scale, shift)`` the second epilogue stage.  Gather mode: ``x = None``, ``ids`` / ``table`` the
    rows' source and ``xcopy`` (optional) where the gathered rows are also written."""
    ptr = lambda t: 0 if t is None else t.data_ptr()
    ld = lambda t: 0 if t is None else t.stride(0)
    return LinearProblem(x=ptr(x), ldx=ld(x), ids=ptr(ids), table=ptr(table), xcopy=ptr(xcopy), ld_xcopy=ld(xcopy),
                         w=w.data_ptr(), ldw=w.stride(0), bias=ptr(bias), y=y.data_ptr(), ldy=y.stride(0), n=n, m=m, act=act,
                         post_scale=0 if post is None else post[0].data_ptr(),
                         post_shift=0 if post is None else post[1].data_ptr())


def pad32(n):
    """``n`` rounded up to the multiple of 32 that the GEMM's K has to be."""
    return (n + 31) // 32 * 32


@_c_struct("sss_graph_out")
class GraphOut(ctypes.Structure):
    """``sss_graph_out`` of include/sss.h."""


@_c_struct("sss_layer_args")
class LayerArgs(ctypes.Structure):
    """``sss_layer_args`` of include/sss.h."""


@_c_struct("sss_hgt_slot")
class HgtSlot(ctypes.Structure):
    """``sss_hgt_slot`` of include/sss_hgt.h."""


@_c_struct("sss_hgt_args")
class HgtArgs(ctypes.Structure):
    """``sss_hgt_args`` of include/sss_hgt.h."""


@_c_struct("sss_seq_attention_args")
class SeqAttentionArgs(ctypes.Structure):
    """``sss_seq_attention_args`` of include/sss_text.h."""


if set(STRUCTS) != set(_STRUCT_FIELDS):
    raise ValueError(f"include/ declares structs with no ctypes.Structure here: {sorted(set(_STRUCT_FIELDS) - set(STRUCTS))}")


def symbols(header):
    """The entry points of include/<header>."""
    return sorted(HEADERS[header])


def exported_symbols():
    return symbols("sss.h")


def build(verbose: bool = False) -> str:
    """Compile libsss.so for gfx950 (hipcc cross-compiles without a GPU)."""
    cmd = ["make", "-C", CSRC, "-j4"]
    res = subprocess.run(cmd, capture_output=True, text=True)
    if res.returncode != 0:
        raise RuntimeError("building libsss.so failed:\n" + res.stdout[-4000:] + res.stderr[-4000:])
    if verbose:
        print(res.stdout)
    return LIB_PATH


def lib():
    """The loaded library; raises (never falls back) when it is absent."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                f"{LIB_PATH} is missing: the HIP extension is not built. Run "
                "`python -c 'import __graft_entry__ as g; g.build()'` (or `make -C "
                "sessionsimilaritysearch_amd/csrc`). There is no CPU fallback.")
        h = ctypes.CDLL(LIB_PATH)
        for table in (*HEADERS.values(), *EXT_HEADERS.values(), *LOWP_HEADERS.values(), *HEADS_HEADERS.values(),
                      *TOK_HEADERS.values()):
            for name, (res, args) in table.items():
                fn = getattr(h, name)      # AttributeError if the .so lacks a declared symbol
                fn.restype, fn.argtypes = res, args
        _lib = h
    return _lib


def call(name, values):
    """Entry point ``name`` with each argument taken from ``values`` under the name its header gives the parameter (a
    parameter ``values`` lacks: KeyError naming it).  For the once-per-search calls whose families differ in what they
    take; the per-launch paths call positionally."""
    return getattr(lib(), name)(*[values[p] for p in PARAMS[name]])


class SssError(RuntimeError):
    pass


def check(rc: int, what: str):
    if rc != 0:
        msg = lib().sss_last_error()
        raise SssError(f"{what} failed (rc={rc}): {msg.decode() if msg else ''}")


def stream_ptr(device=None):
    import torch
    return torch.cuda.current_stream(device).cuda_stream


def require_cuda(t, name, dtype=None):
    import torch
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise SssError(f"{name} must be a CUDA (HIP) tensor")
    if dtype is not None and t.dtype != dtype:
        raise SssError(f"{name} must have dtype {dtype}, got {t.dtype}")
    if not t.is_contiguous():
        raise SssError(f"{name} must be contiguous")
    return t
