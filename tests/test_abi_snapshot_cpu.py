"""The binding ``_lib`` reads from include/*.h: equal to tests/golden/abi_signatures.json (a header edit that moves the ABI
fails here until tests/golden/make_golden_abi.py regenerates the file on purpose), the reader on the edges of the headers'
style, and the parameter names ``FlatIndex`` calls the scan families by."""
import ctypes
import os
import sys

import pytest

from sessionsimilaritysearch_amd import _lib, index as ix

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import abi  # noqa: E402


def test_headers_are_the_directory_listing_and_every_name_is_declared_once():
    assert sorted(_lib.HEADERS) == abi.headers() and len(abi.headers()) == 12
    names = [n for table in _lib.HEADERS.values() for n in table]
    assert len(names) == len(set(names)) == len(_lib.PARAMS) == 98
    for header, table in _lib.HEADERS.items():
        assert sorted(table) == abi.declared(header) == _lib.symbols(header), header


def test_reader_and_loaded_library_equal_the_snapshot():
    snap = abi.snapshot()
    assert {h: {n: abi.signature(*sig) for n, sig in table.items()} for h, table in _lib.HEADERS.items()} == snap["functions"]
    assert {n: abi.struct_record(cls) for n, cls in _lib.STRUCTS.items()} == snap["structs"]
    L = _lib.lib()
    for header, table in snap["functions"].items():
        for name, sig in table.items():
            fn = getattr(L, name)
            assert abi.signature(fn.restype, fn.argtypes) == sig, name
            assert len(_lib.PARAMS[name]) == len(sig[1]), name
    assert [ctypes.sizeof(c) for c in (_lib.LinearProblem, _lib.LayerArgs, _lib.GraphOut, _lib.HgtSlot, _lib.HgtArgs,
                                       _lib.SeqAttentionArgs)] == [120, 256, 120, 48, 160, 80]


EDGES = """
/* a comment that declares nothing: int sss_fake(int x); */
#ifdef __cplusplus
extern "C" {
#endif
typedef struct { const float* k; int64_t ld_k; } sss_t_slot;
typedef struct {
    sss_t_slot slot[2];     /* the nested array */
    int32_t n; float* out;
} sss_t_args;
int sss_t_version(void);
const char* sss_t_error(void);   /* trailing */
size_t sss_t_bytes(int64_t nq,
                   int d,
                   float eps,
                   double lam);      // four lines
int sss_t_run(const uint16_t* image, const sss_t_args* args, int32_t* status, size_t bytes, void* stream);
"""


def test_reader_on_the_edges_of_the_header_style():
    functions, structs = _lib.read_header(EDGES, "edges.h")
    c = ctypes
    assert functions == {
        "sss_t_version": (c.c_int, [], ()),
        "sss_t_error": (c.c_char_p, [], ()),
        "sss_t_bytes": (c.c_size_t, [c.c_int64, c.c_int, c.c_float, c.c_double], ("nq", "d", "eps", "lam")),
        "sss_t_run": (c.c_int, [c.c_void_p, c.c_void_p, c.c_void_p, c.c_size_t, c.c_void_p], ("image", "args", "status", "bytes", "stream")),
    }
    assert list(structs) == ["sss_t_slot", "sss_t_args"]
    slot = [_lib._declarator(f, "edges.h") for f in structs["sss_t_slot"]]
    assert slot == [("k", c.c_void_p), ("ld_k", c.c_int64)]                         # two fields on one line

    class Slot(c.Structure):
        _fields_ = slot
    args = [_lib._declarator(f, "edges.h", {"sss_t_slot": Slot}) for f in structs["sss_t_args"]]
    assert [n for n, _ in args] == ["slot", "n", "out"] and args[1:] == [("n", c.c_int32), ("out", c.c_void_p)]
    assert issubclass(args[0][1], c.Array) and args[0][1]._type_ is Slot and args[0][1]._length_ == 2


@pytest.mark.parametrize("text, named", [
    ("int sss_t_f(long x);", ("edges.h", "sss_t_f", "long")),
    ("long sss_t_f(int x);", ("edges.h", "sss_t_f", "long")),
    ("int sss_t_f(unsigned int x);", ("edges.h", "sss_t_f", "unsigned int x")),
    ("int sss_t_f(sss_t_slot s);", ("edges.h", "sss_t_f", "sss_t_slot")),          # a struct by value is no parameter type
])
def test_reader_refuses_a_type_it_does_not_know(text, named):
    with pytest.raises(ValueError) as e:
        _lib.read_header(text, "edges.h")
    assert all(part in str(e.value) for part in named), str(e.value)
    with pytest.raises(ValueError, match="long"):
        _lib._declarator("long n", "edges.h: sss_t_args")


# the names FlatIndex._values / _call / search_fused / search_threshold key their values by
VOCABULARY = {"q", "nq", "nsel", "qsel", "corpus", "dtype", "scan_image", "scan_dtype", "corpus_shift", "corpus_resid_norm", "bias",
              "n", "d", "d_row", "d_scan", "k", "id_offset", "corpus_max_norm", "D_out", "I_out", "status", "unproven_count", "state",
              "state_bytes", "workspace", "workspace_bytes", "stream"}


@pytest.mark.parametrize("table", ["_TOPK", "_THRESHOLD"])
def test_scan_families_take_only_parameters_flatindex_names(table):
    families = getattr(ix, table)
    assert len(families) == {"_TOPK": 7, "_THRESHOLD": 3}[table]
    for family, name in families.items():
        sizer = ix._WORKSPACE_BYTES.get(name, name + "_workspace_bytes")
        assert set(_lib.PARAMS[name]) <= VOCABULARY, (family, sorted(set(_lib.PARAMS[name]) - VOCABULARY))
        assert set(_lib.PARAMS[sizer]) <= VOCABULARY, (family, sorted(set(_lib.PARAMS[sizer]) - VOCABULARY))
        assert ("state" in _lib.PARAMS[name]) == ("unproven_count" in _lib.PARAMS[name]) == (table == "_TOPK" and "long" not in family)
    assert ix._WORKSPACE_BYTES == {"sss_ip_topk_split": "sss_ip_topk_workspace_bytes"}


def test_call_by_name_names_the_parameter_it_lacks():
    with pytest.raises(KeyError, match="'amax'"):
        _lib.call("sss_f16_shift", {})
    assert _lib.call("sss_f16_shift", {"amax": 1.0, "unused": None}) == _lib.lib().sss_f16_shift(1.0)
