"""CPU side of the catalogue heads (include/heads/sss_catalogue.h, csrc/catalogue.hip, catalogue.py): the heads header against
its binding and its snapshot (tests/golden/abi_signatures_heads.json) with the three older listings unchanged; the header's
constants against their derivation; argument validation without a device; and the host restatement
(tests/helpers/catalogue_ref.py) against the reference-run fixture (tests/golden/catalogue_heads.npz,
make_golden_catalogue.py)."""
import ctypes
import json
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import abi  # noqa: E402
import catalogue_ref as cr  # noqa: E402
import make_golden_abi_heads as heads_abi  # noqa: E402

from sessionsimilaritysearch_amd import _lib  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = "sss_catalogue.h"
NAMES = ["sss_catalogue_bce", "sss_catalogue_bce_workspace_bytes", "sss_catalogue_hits"]
FIXTURE = os.path.join(ROOT, "tests", "golden", "catalogue_heads.npz")

# |reference float32 loss - float64 restatement| / loss: the largest over the fixture's cases is 6.66e-7 (case c, where both
# clip limits are hit: the reference's own float32 log(1 - val) cancels there), measured when the fixture was generated.
# The bound is 4 times that; the margin is over the reference's rounding, not over the code under test.
LOSS_MEASURED = 6.66e-7
LOSS_BOUND = 4 * LOSS_MEASURED


def test_heads_header_is_declared_bound_and_equals_its_snapshot():
    assert abi.declared(os.path.join("heads", HEADER)) == sorted(_lib.HEADS_HEADERS[HEADER]) == NAMES
    assert sorted(_lib.HEADS_HEADERS) == sorted(f for f in os.listdir(os.path.join(ROOT, "include", "heads")) if f.endswith(".h")) == [HEADER]
    with open(heads_abi.SNAPSHOT) as f:
        snap = json.load(f)
    assert heads_abi.record(_lib) == snap
    L = _lib.lib()
    for name in NAMES:                                                  # exported by libsss.so and bound by lib()
        fn = getattr(L, name)
        assert heads_abi.signature(fn.restype, fn.argtypes) == snap["functions"][HEADER][name]
    assert _lib.HEADS_PARAMS["sss_catalogue_bce"] == ("rep", "table", "ldw", "kp", "ptr", "items", "b", "v", "mode", "keep_thr", "seed",
                                                      "row_offset", "sums", "counts", "workspace", "workspace_bytes", "stream")
    sig = _lib.HEADS_HEADERS[HEADER]["sss_catalogue_bce"][1]
    assert sig[9] is ctypes.c_uint32 and sig[10] is ctypes.c_uint64     # keep_thr, seed: the two types the reader learned
    text = open(os.path.join(ROOT, "include", "heads", HEADER)).read()
    for words in ("CALLER-OWNED DEVICE", "0x9E3779B97F4A7C15", "0xBF58476D1CE4E5B9", "0x94D049BB133111EB", "ONE NUMERICAL DEVIATION",
                  "oracle_linear_chain", "No floating-point atomics"):
        assert words in text, words


def test_the_three_older_listings_are_unchanged_and_the_tables_are_disjoint():
    assert len(_lib.HEADERS) == 12 and len(_lib.PARAMS) == 98
    assert sorted(_lib.EXT_HEADERS) == ["sss_seqsim.h"] and sorted(_lib.EXT_PARAMS) == ["sss_seq_pair_scores", "sss_seq_query_metric"]
    assert sorted(_lib.LOWP_HEADERS) == ["sss_linear_bf16.h"] and sorted(_lib.LOWP_PARAMS) == ["sss_linear_grouped_bf16"]
    assert not set(_lib.HEADS_PARAMS) & (set(_lib.PARAMS) | set(_lib.EXT_PARAMS) | set(_lib.LOWP_PARAMS))
    for maker, table in (("make_golden_abi_ext", "abi_signatures_ext.json"), ("make_golden_abi_lowp", "abi_signatures_lowp.json")):
        mod = __import__(maker)
        with open(os.path.join(ROOT, "tests", "golden", table)) as f:
            assert mod.record(_lib) == json.load(f)                     # the reader's new types moved no older snapshot
    snap = abi.snapshot()
    assert {h: {n: abi.signature(*sig) for n, sig in t.items()} for h, t in _lib.HEADERS.items()} == snap["functions"]


def test_the_header_literals_are_the_derived_limits():
    """-log of the reference's clip limits, evaluated in float64 and rounded to float32."""
    f = np.float32
    want = {"P_LO": -math.log(float(f(0.9999))), "P_HI": -math.log(float(f(1e-4))),
            "N_LO": -math.log(float(f(1) - f(1e-4))), "N_HI": -math.log(float(f(1) - f(0.9999)))}
    for name, v in want.items():
        got = _lib.header_float("heads/" + HEADER, "SSS_CATALOGUE_" + name)
        assert got == float(f(v)) == getattr(cr, name), (name, got, v)
    assert _lib.header_constant("heads/" + HEADER, "SSS_CATALOGUE_SPAN") == 1024
    with pytest.raises(ValueError, match="hexadecimal"):
        _lib.header_float("heads/" + HEADER, "SSS_CATALOGUE_SPAN")


_P = 1 << 20                                                          # a non-null, 16-byte aligned address; never dereferenced


def _bce(**kw):
    a = dict(rep=_P, table=_P, ldw=224, kp=224, ptr=_P, items=_P, b=5, v=1000, mode=0, keep_thr=1 << 30, seed=7, row_offset=0,
             sums=_P, counts=_P, workspace=_P, workspace_bytes=1 << 20, stream=0)
    a.update(kw)
    L = _lib.lib()
    return L.sss_catalogue_bce(*[a[p] for p in _lib.HEADS_PARAMS["sss_catalogue_bce"]]), L.sss_last_error() or b""


def _hits(**kw):
    a = dict(I=_P, b=3, k=20, ptr=_P, items=_P, hits=_P, stream=0)
    a.update(kw)
    L = _lib.lib()
    return L.sss_catalogue_hits(*[a[p] for p in _lib.HEADS_PARAMS["sss_catalogue_hits"]]), L.sss_last_error() or b""


def test_arguments_are_rejected_before_any_launch():
    """No address given here is memory: a call that launched would fault.  Every rejection names what is wrong."""
    for kw, rc_want, words in ((dict(kp=200), -1, b"kp % 32"), (dict(kp=0), -1, b"kp % 32"), (dict(kp=-32), -1, b"kp % 32"),
                               (dict(ldw=192), -1, b"ldw >= kp"), (dict(ldw=226), -1, b"ldw % 4"),
                               (dict(v=0), -1, b"0 < v"), (dict(v=1 << 31), -1, b"0 < v"), (dict(b=-1), -1, b"0 <= b"),
                               (dict(b=65535 * 64 + 1), -1, b"0 <= b"), (dict(mode=2), -1, b"mode"), (dict(mode=-1), -1, b"mode"),
                               (dict(row_offset=-1), -1, b"row_offset"),
                               (dict(rep=0), -1, b"null"), (dict(table=0), -1, b"null"), (dict(ptr=0), -1, b"null"),
                               (dict(items=0), -1, b"null"), (dict(sums=0), -1, b"null"), (dict(counts=0), -1, b"null"),
                               (dict(workspace=0), -2, b"workspace"), (dict(workspace_bytes=255), -2, b"workspace"),
                               (dict(workspace=_P + 4), -1, b"aligned")):
        rc, msg = _bce(**kw)
        assert rc == rc_want and msg.startswith(b"catalogue_bce:") and words in msg, (kw, rc, msg)
    need = _lib.lib().sss_catalogue_bce_workspace_bytes(200, 391572)
    assert need == 1225728 + 612864                                     # 383 spans x 200 rows x 2: doubles, then ints, each to 256 bytes
    assert _bce(b=200, v=391572, workspace_bytes=need - 1)[0] == -2
    assert _bce(b=0, rep=0, sums=0, workspace=0)[0] == 0                # an empty batch touches nothing
    assert _bce(b=0, kp=100)[0] == -1                                   # but its shapes are still checked
    for kw, words in ((dict(k=0), b"k <= 1024"), (dict(k=1025), b"k <= 1024"), (dict(b=-1), b"0 <= b"), (dict(b=1 << 31), b"0 <= b"),
                      (dict(I=0), b"null"), (dict(ptr=0), b"null"), (dict(items=0), b"null"), (dict(hits=0), b"null")):
        rc, msg = _hits(**kw)
        assert rc == -1 and msg.startswith(b"catalogue_hits:") and words in msg, (kw, rc, msg)
    assert _hits(b=0, I=0)[0] == 0


def test_keep_threshold_and_the_hash():
    from sessionsimilaritysearch_amd.catalogue import keep_threshold
    for n_neg, V in ((1000, 391572), (1000, 4099), (0, 10), (1, 3), (4098, 4099), (4099, 4099), (5000, 4099), ("all", 7)):
        assert keep_threshold(n_neg, V) == cr.keep_threshold(n_neg, V)
    assert keep_threshold(1000, 391572) == (1000 << 32) // 391572 and keep_threshold(0, 9) == 0 and keep_threshold(9, 9) == 1 << 32
    for bad in (-1, 2.5, True, "some", None):
        with pytest.raises(ValueError, match="n_neg"):
            keep_threshold(bad, 10)
    # the vectorised hash is the formula of the header, in Python integers
    h = cr.hash_rows(0xDEADBEEFCAFEF00D, [0, 5, 2 ** 40 + 3], 300)
    for r, g in enumerate((0, 5, 2 ** 40 + 3)):
        for i in (0, 1, 63, 64, 299):
            assert int(h[r, i]) == cr.hash_scalar(0xDEADBEEFCAFEF00D, g, i, 300)
    # SplitMix64's first output for state 0 is the finaliser of the golden constant alone
    assert cr.hash_scalar(0, 0, 1, 5) == 0xE220A8397B1DCDAF >> 32


def test_the_kept_fraction_is_binomial():
    """V = 4099, B = 64, the fixture's seed of that shape: within 5 standard deviations of keep_thr / 2^32."""
    z = np.load(FIXTURE)
    seed, V, B = int(z["b_seed"]), 4099, 64
    thr = cr.keep_threshold(1000, V)
    p, n = thr / 2 ** 32, V * B
    kept = int(cr.keep_mask(seed, np.arange(B), V, 1000).sum())
    assert abs(kept - n * p) <= 5 * math.sqrt(n * p * (1 - p)), (kept, n * p)
    per_row = cr.keep_mask(seed, np.arange(B), V, 1000).sum(1)
    assert per_row.min() > 0 and len(set(per_row.tolist())) > 8          # rows draw different masks


def _cases():
    z = np.load(FIXTURE)
    for tag in z["tags"]:
        g = {k[len(tag) + 1:]: z[k] for k in z.files if k.startswith(f"{tag}_")}
        g["table"] = g["q"].astype(np.float32) / np.float32(64)
        yield str(tag), g, [int(k) for k in z["ks"]], int(z["n_neg"])


def _targets(g, which):
    ptr, items = (g["ptr"], g["items"]) if which == "next" else (g["all_ptr"], g["all_items"])
    return cr.csr([items[ptr[b]:ptr[b + 1]] for b in range(len(ptr) - 1)])


def test_the_restatement_reproduces_the_reference_run():
    """Counts, precision and recall exactly; the loss within LOSS_BOUND = 4 * 6.66e-7 = 2.66e-6 relative (the measured
    largest deviation of the reference's own float32 arithmetic from the float64 restatement, times 4: see the constants
    above and DESIGN.md section 5.13)."""
    from sessionsimilaritysearch_amd.catalogue import accuracy_of_hits
    worst = 0.0
    shapes = set()
    for tag, g, ks, n_neg in _cases():
        s = cr.logits(g["rep"], g["table"])
        shapes.add((int(g["V"]), g["rep"].shape[0], g["rep"].shape[1]))
        for which in ("next", "all"):
            ptr, items = _targets(g, which)
            loss, sums, counts = cr.bce(s, ptr, items, n_neg, int(g["seed"]), 0)
            assert int(counts.sum()) == int(g[f"{which}_kept"]), (tag, which)
            rel = abs(float(g[f"{which}_loss"]) - loss) / loss
            worst = max(worst, rel)
            print(f"{tag} {which}: reference {float(g[which + '_loss']):.9f} restatement {loss:.9f} relative {rel:.3e}")
            assert rel <= LOSS_BOUND, (tag, which, rel)
            for K in ks:
                if f"{which}_acc{K}" in g:
                    _, I = cr.topk(g["rep"], g["table"], K)
                    assert cr.accuracy(I, ptr, items, which == "next") == tuple(g[f"{which}_acc{K}"].tolist()), (tag, which, K)
                    # the package's own host step, from the restatement's hit counts
                    assert accuracy_of_hits(cr.hits(I, ptr, items).astype(np.int32), np.diff(ptr), K, which == "next") == \
                        tuple(g[f"{which}_acc{K}"].tolist()), (tag, which, K)
    print(f"largest relative deviation {worst:.3e}, bound {LOSS_BOUND:.3e}")
    assert worst > LOSS_BOUND / 8                                       # the bound is still 4 x what the fixture shows, not looser
    assert shapes == {(257, 7, 200), (4099, 64, 32), (257, 1, 32), (4099, 7, 32)}


def test_the_fixture_holds_the_cases_it_is_meant_to():
    for tag, g, ks, n_neg in _cases():
        ptr, items = g["ptr"], g["items"]
        rows = [items[ptr[b]:ptr[b + 1]].tolist() for b in range(len(ptr) - 1)]
        assert any(len(r) != len(set(r)) for r in rows), tag                      # duplicate targets
        assert len(rows) == 1 or any(len(r) == 0 for r in rows), tag              # a row without targets
        s = cr.logits(g["rep"], g["table"]).astype(np.float64)
        if tag == "c":                                                            # both clip limits are hit
            t = cr.softplus64(s)
            assert (t > cr.N_HI).any() and (t < cr.N_LO).any()
        else:
            assert any(float(g[f"next_acc{K}"][1]) > 0 for K in ks)               # the accuracies are not all zero


def test_accuracy_of_hits_edges():
    from sessionsimilaritysearch_amd.catalogue import accuracy_of_hits
    hit, size = np.array([1, 0, 2], np.int32), np.array([3, 0, 2], np.int64)
    assert accuracy_of_hits(hit, size, 20, True) == (float(np.mean([1 / 20, 2 / 20])), float(np.mean([1 / 3, 2 / 2])))
    with pytest.raises(ZeroDivisionError):
        accuracy_of_hits(hit, size, 20, False)
    assert all(np.isnan(x) for x in accuracy_of_hits(hit[1:2], size[1:2], 20, True))


def test_the_package_exports_the_catalogue_heads():
    import sessionsimilaritysearch_amd as pkg
    from sessionsimilaritysearch_amd import catalogue
    for name in ("CatalogueHead", "CatalogueLoss", "get_next_product_asin_accuracy", "get_all_product_asin_accuracy",
                 "get_next_product_asin_loss", "get_all_product_asin_loss"):
        assert getattr(pkg, name) is getattr(catalogue, name) and name in pkg.__all__
