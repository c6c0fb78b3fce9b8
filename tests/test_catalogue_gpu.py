"""The catalogue heads on the device (include/heads/sss_catalogue.h, csrc/catalogue.hip, catalogue.py) against the host
restatement tests/helpers/catalogue_ref.py.

The logits of the restatement are ``oracle.search_ref.linear_chain`` on the zero-extended operands: the kernel's fma chain,
bit for bit.  On those bits, counts are equal and every sum is within ``2^-20 * sum`` of the float64 restatement: 16 float32
ulps -- an OpenCL-grade ``expf`` <= 3 ulp and ``log1pf`` <= 2 ulp, one add, softplus 1-conditioned in its log1p part, the
clamps monotone; doubled for margin -- plus ``V * 2^-53 * sum`` for the float64 accumulation.  Shapes sit at the kernel's
edges: the 64-row and 64-item tile, the 1024-item span of one workgroup (SSS_CATALOGUE_SPAN), more than one of each."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import catalogue_ref as cr  # noqa: E402

from oracle import search_ref as sr  # noqa: E402
from sessionsimilaritysearch_amd import _lib, catalogue  # noqa: E402
from sessionsimilaritysearch_amd.sparse import SessionVectors, _device_triple  # noqa: E402
from sessionsimilaritysearch_amd.variants import MLPHead  # noqa: E402
from test_catalogue_cpu import LOSS_BOUND, _cases, _targets  # noqa: E402

pytestmark = pytest.mark.gpu

TILE, SPAN = 64, 1024
REL = 2.0 ** -20
_CACHE = {}


def vectors(ptr, items, dev) -> SessionVectors:
    return _device_triple(np.asarray(ptr, np.int64), np.asarray(items, np.int32), np.zeros(len(items), np.float32), dev)


def bits(x):
    return np.ascontiguousarray(x).view(np.int64)


def held(got: catalogue.CatalogueLoss, s, ptr, items, n_neg, seed, row_offset=0):
    """Counts equal, sums within the derived bound of the restatement on the logits ``s``."""
    loss, sums, counts = cr.bce(s, ptr, items, n_neg, seed, row_offset)
    assert np.array_equal(got.counts, counts)
    tol = (REL + s.shape[1] * 2.0 ** -53) * sums
    err = np.abs(got.sums - sums)
    print(f"V={s.shape[1]} B={s.shape[0]} n_neg={n_neg}: max |sum - ref| / ref = {np.max(err / np.maximum(sums, 1e-300)):.3e} (bound {REL:.3e})")
    assert (err <= tol).all(), (err / np.maximum(sums, 1e-300)).max()
    assert abs(got.loss - loss) <= (REL + s.shape[1] * 2.0 ** -53) * loss
    return sums, counts


def edge_case(V, B, d, seed):
    """Seeded operands with targets at items 0, tile - 1, tile, span - 1, span, V - 1 (those below V), a row with no
    targets and, where V is small, a row whose targets are all of V."""
    r = np.random.default_rng(seed)
    table = r.standard_normal((V, d)).astype(np.float32)
    rep = (2.5 * r.standard_normal((B, d)) / np.sqrt(d)).astype(np.float32)
    marks = sorted({x for x in (0, TILE - 1, TILE, SPAN - 1, SPAN, V - 1) if x < V})
    rows = [sorted(set(r.choice(V, size=min(V, int(r.integers(1, 7))), replace=False).tolist())) for _ in range(B)]
    rows[0] = marks
    if B > 2:
        rows[1] = []
        rows[B - 1] = sorted(set(rows[B - 1]) | set(marks))
    if V <= 65 and B > 3:
        rows[2] = list(range(V))
    ptr, items = cr.csr(rows)
    return table, rep, ptr, items, rows


# one shape per edge: a single item / row; one short of, exactly and one past the tile on either side; several row blocks;
# one span exactly filled to 1000 of 1024; five spans with a 3-item last tile; both widths (Kp = 32 and 224)
SHAPES = [(1, 1, 32), (63, 63, 32), (64, 65, 200), (65, 1, 200), (1000, 200, 32), (4099, 65, 200), (4099, 63, 32)]


@pytest.mark.parametrize("V,B,d", SHAPES)
def test_shapes_at_the_tile_edges(cuda, V, B, d):
    table, rep, ptr, items, rows = edge_case(V, B, d, 100 + V + B + d)
    head = catalogue.CatalogueHead(table, device=cuda)
    assert head.kp == (d + 31) // 32 * 32 and head.n_items == V
    t = vectors(ptr, items, cuda)
    s = cr.logits(rep, table)
    for n_neg, seed in ((1000, 5), (max(1, V // 4), 2 ** 63 + 11), ("all", 0)):
        got = head.bce(rep, t, n_neg, seed)
        sums, counts = held(got, s, ptr, items, n_neg, seed)
        assert np.array_equal(counts[:, 0], [len(x) for x in rows])
        if B > 2:
            assert counts[1, 0] == 0 and got.sums[1, 0] == 0.0                     # the row without targets
        if V <= 65 and B > 3:
            assert counts[2, 1] == 0 and got.sums[2, 1] == 0.0 and counts[2, 0] == V   # every item is a target
        if n_neg == "all":
            assert np.array_equal(counts.sum(1), np.full(B, V))


def test_each_logit_is_its_single_product(cuda):
    """Rows of +-powers of two with one non-zero column: every logit is one exact product, so the chain restatement equals
    the exact value bit for bit, and a row whose positive (or negative) part is a single pair shows that pair's term."""
    V, B, d = 65, 65, 200
    k_of = [(7 * b) % d for b in range(B)]
    rep = np.zeros((B, d), np.float32)
    for b in range(B):
        rep[b, k_of[b]] = (-1.0) ** b * 2.0 ** ((b % 5) - 2)
    vv, kk = np.meshgrid(np.arange(V), np.arange(d), indexing="ij")
    table = ((-1.0) ** (vv + kk // 3) * 2.0 ** ((vv + kk) % 7 - 3)).astype(np.float32)
    exact = np.array([[float(rep[b, k_of[b]]) * float(table[v, k_of[b]]) for v in range(V)] for b in range(B)])
    s = cr.logits(rep, table)
    assert np.array_equal(s.astype(np.float64), exact) and len(np.unique(exact)) >= 20
    single = [(3 * b + 1) % V for b in range(B)]
    rows = [[single[b]] if b % 2 == 0 else [v for v in range(V) if v != single[b]] for b in range(B)]
    ptr, items = cr.csr(rows)
    got = catalogue.CatalogueHead(table, device=cuda).bce(rep, vectors(ptr, items, cuda), "all")
    held(got, s, ptr, items, "all", 0)
    for b in range(B):
        z = exact[b, single[b]]
        q = b % 2                                                                   # even rows: one positive; odd rows: one negative
        want = float(cr.clamp_nan(cr.softplus64(-z), cr.P_LO, cr.P_HI)) if q == 0 else float(cr.clamp_nan(cr.softplus64(z), cr.N_LO, cr.N_HI))
        assert got.counts[b, q] == 1 and abs(got.sums[b, q] - want) <= REL * want, (b, z, got.sums[b, q], want)
        assert got.sums[b, q] == float(np.float32(got.sums[b, q]))                  # one float32 term, widened


def test_saturated_logits_give_the_header_literals(cuda):
    """Logits of +30, -30 and 0: the four clamp limits, exactly as include/heads/sss_catalogue.h writes them."""
    lim = {n: _lib.header_float("heads/sss_catalogue.h", "SSS_CATALOGUE_" + n) for n in ("P_LO", "P_HI", "N_LO", "N_HI")}
    table = np.zeros((3, 32), np.float32)
    table[:, 0] = (30.0, -30.0, 0.0)
    rows = [[0], [1], [0, 2], [1, 2], [0, 1], [2]]
    rep = np.zeros((len(rows), 32), np.float32)
    rep[:, 0] = 1.0
    ptr, items = cr.csr(rows)
    got = catalogue.CatalogueHead(table, device=cuda).bce(rep, vectors(ptr, items, cuda), "all")
    log2 = float(np.log(2.0))
    assert got.sums[0, 0] == lim["P_LO"] and got.sums[1, 0] == lim["P_HI"]         # a positive at +30 / at -30
    assert got.sums[2, 1] == lim["N_LO"] and got.sums[3, 1] == lim["N_HI"]         # the one negative at -30 / at +30
    assert abs(got.sums[4, 1] - log2) <= REL * log2 and abs(got.sums[5, 0] - log2) <= REL * log2
    assert got.sums[5, 1] == lim["N_HI"] + lim["N_LO"]                             # two float32 terms added in float64
    assert np.array_equal(got.counts, [[1, 2], [1, 2], [2, 1], [2, 1], [2, 1], [1, 2]])
    held(got, cr.logits(rep, table), ptr, items, "all", 0)


def big_case(cuda):
    """V = 4099, d = 200, B = 200: shared by the tests below; operands and the chain logits are made once and left alone."""
    if "big" not in _CACHE:
        table, rep, ptr, items, rows = edge_case(4099, 200, 200, 7)
        _CACHE["big"] = (table, rep, ptr, items, rows, cr.logits(rep, table), catalogue.CatalogueHead(table, device=cuda),
                         vectors(ptr, items, cuda))
    return _CACHE["big"]


def test_rows_do_not_depend_on_the_batch_around_them(cuda):
    """B = 200 in one call equals the same rows in chunks of 1, 63 and 136 with matching row_offset, bit for bit per row;
    two identical calls are bit-identical."""
    table, rep, ptr, items, rows, s, head, t = big_case(cuda)
    seed = 0x1234567890ABCDEF
    whole = head.bce(rep, t, 1000, seed)
    again = head.bce(rep, t, 1000, seed)
    assert np.array_equal(bits(whole.sums), bits(again.sums)) and np.array_equal(whole.counts, again.counts) and whole.loss == again.loss
    held(whole, s, ptr, items, 1000, seed)
    lo = 0
    for n in (1, 63, 136):
        part = head.bce(rep[lo:lo + n], SessionVectors(t.ptr[lo:lo + n + 1], t.items, t.weights), 1000, seed, row_offset=lo)
        assert np.array_equal(bits(part.sums), bits(whole.sums[lo:lo + n])) and np.array_equal(part.counts, whole.counts[lo:lo + n]), (lo, n)
        lo += n
    assert lo == 200
    shifted = head.bce(rep[:64], SessionVectors(t.ptr[:65], t.items, t.weights), 1000, seed, row_offset=1)     # another g: another mask
    assert not np.array_equal(shifted.counts[:, 1], whole.counts[:64, 1]) and np.array_equal(bits(shifted.sums[:, 0]), bits(whole.sums[:64, 0]))


def test_mode_equivalences(cuda):
    table, rep, ptr, items, rows, s, head, t = big_case(cuda)
    V, B = 4099, 200
    every = head.bce(rep, t, "all")
    for n_neg in (V, V + 5):
        same = head.bce(rep, t, n_neg, seed=99)
        assert np.array_equal(bits(same.sums), bits(every.sums)) and np.array_equal(same.counts, every.counts)
    none = head.bce(rep, t, 0, seed=3)
    assert (none.counts[:, 1] == 0).all() and (none.sums[:, 1] == 0.0).all()
    assert np.array_equal(bits(none.sums[:, 0]), bits(every.sums[:, 0])) and np.array_equal(none.counts[:, 0], every.counts[:, 0])
    # through the C ABI: mode 0 with the largest threshold keeps every negative whose hash is not 2^32 - 1 (none here)
    seed = 12345
    assert not (cr.hash_rows(seed, np.arange(B), V) == np.uint32(0xFFFFFFFF)).any()
    x = torch.zeros((B, head.kp), dtype=torch.float32, device=cuda)
    x[:, :200] = torch.from_numpy(rep).to(cuda)
    L = _lib.lib()
    ws = torch.empty(L.sss_catalogue_bce_workspace_bytes(B, V), dtype=torch.uint8, device=cuda)
    out = []
    for mode, thr in ((0, 0xFFFFFFFF), (1, 0)):
        sums = torch.full((B, 2), float("nan"), dtype=torch.float64, device=cuda)
        counts = torch.full((B, 2), -7, dtype=torch.int64, device=cuda)
        rc = L.sss_catalogue_bce(x.data_ptr(), head._image.data_ptr(), head._image.stride(0), head.kp, t.ptr.data_ptr(), t.items.data_ptr(),
                                 B, V, mode, thr, seed, 0, sums.data_ptr(), counts.data_ptr(), ws.data_ptr(), ws.numel(), _lib.stream_ptr(cuda))
        _lib.check(rc, "sss_catalogue_bce")
        out.append((sums.cpu().numpy(), counts.cpu().numpy()))
    assert np.array_equal(bits(out[0][0]), bits(out[1][0])) and np.array_equal(out[0][1], out[1][1])
    assert np.array_equal(bits(out[1][0]), bits(every.sums)) and np.array_equal(out[1][1], every.counts)


def test_a_nan_row_is_nan_alone_and_bce_raises(cuda):
    table, rep, ptr, items, rows, s, head, t = big_case(cuda)
    bad = rep[:70].copy()
    bad[66, 3] = np.nan
    tv = SessionVectors(t.ptr[:71], t.items, t.weights)
    sums, counts = head.bce_device(torch.from_numpy(bad).to(cuda), tv, "all")
    sums = sums.cpu().numpy()
    assert np.isnan(sums[66]).all() and not np.isnan(np.delete(sums, 66, 0)).any()
    with pytest.raises(AssertionError, match="NaN"):
        head.bce(bad, tv, "all")
    with pytest.raises(AssertionError, match="no element"):
        head.bce(rep[1:2], SessionVectors(t.ptr[1:3], t.items, t.weights), 0)       # the row without targets, no negatives


def small_head(cuda):
    r = np.random.default_rng(5)
    w = {"layers.0.w": torch.from_numpy(r.standard_normal((48, 64)).astype(np.float32) / 8), "layers.0.b": torch.from_numpy(r.standard_normal(48).astype(np.float32)),
         "bn.0.mean": torch.zeros(48), "bn.0.var": torch.ones(48), "bn.0.gamma": torch.ones(48), "bn.0.beta": torch.zeros(48),
         "layers.1.w": torch.from_numpy(r.standard_normal((200, 48)).astype(np.float32) / 4), "layers.1.b": torch.from_numpy(r.standard_normal(200).astype(np.float32) / 4)}
    return MLPHead(w, 0, cuda, last_act=False), r.standard_normal((200, 64)).astype(np.float32)


def test_predict_hits_and_accuracy(cuda):
    table, rep, ptr, items, rows, s, head, t = big_case(cuda)
    for K in (1, 20, 100):
        D, I = head.predict(rep, K)
        Dr, Ir = sr.search_exact(rep, table, K)
        assert np.array_equal(I.cpu().numpy(), Ir) and np.array_equal(D.cpu().numpy(), Dr)
        assert np.array_equal(head.hits(I, t).cpu().numpy(), cr.hits(Ir, ptr, items))
        assert head.accuracy(rep, t, K, skip_empty=True) == cr.accuracy(Ir, ptr, items, True)
        with pytest.raises(ZeroDivisionError):
            head.accuracy(rep, t, K, skip_empty=False)                              # row 1 has no targets
    # hits: duplicate ids count once, the padding -1 and ids beyond int32 never
    I = np.full((200, 7), -1, np.int64)
    for b in range(200):
        own = rows[b] if rows[b] else [5]
        I[b] = [own[0], own[0], own[-1], -1, (own[0] + 1) % 4099, 2 ** 33 + own[0], own[0]]
    assert np.array_equal(head.hits(torch.from_numpy(I).to(cuda), t).cpu().numpy(), cr.hits(I, ptr, items))
    assert cr.hits(I, ptr, items).max() >= 2 and cr.hits(I, ptr, items)[1] == 0
    # no empty row: both switches agree with the reference's two loops
    full_rows = [x if x else [17] for x in rows]
    fptr, fitems = cr.csr(full_rows)
    ft = vectors(fptr, fitems, cuda)
    _, Ir = sr.search_exact(rep, table, 20)
    assert head.accuracy(rep, ft, 20, skip_empty=False) == cr.accuracy(Ir, fptr, fitems, False) == head.accuracy(rep, ft, 20, skip_empty=True)
    assert catalogue.get_all_product_asin_accuracy(rep, None, ft, head, 20) == cr.accuracy(Ir, fptr, fitems, False)
    assert catalogue.get_next_product_asin_accuracy(rep, None, t, head, 20) == cr.accuracy(Ir, ptr, items, True)


def test_a_head_in_front_equals_the_calls_on_its_output(cuda):
    table, rep, ptr, items, rows, s, plain, t = big_case(cuda)
    mlp, emb = small_head(cuda)
    head = catalogue.CatalogueHead(table, mlp, cuda)
    out = mlp.forward(torch.from_numpy(emb).to(cuda))
    a, b = head.bce(emb, t, 1000, 77), plain.bce(out, t, 1000, 77)
    assert np.array_equal(bits(a.sums), bits(b.sums)) and np.array_equal(a.counts, b.counts) and a.loss == b.loss
    held(a, cr.logits(out.cpu().numpy(), table), ptr, items, 1000, 77)
    (Da, Ia), (Db, Ib) = head.predict(emb, 20), plain.predict(out, 20)
    assert torch.equal(Ia, Ib) and torch.equal(Da, Db)
    assert catalogue.get_next_product_asin_loss(emb, mlp, t, plain, cuda, seed=77) == a.loss == catalogue.get_all_product_asin_loss(emb, None, t, head, seed=77)
    assert catalogue.get_next_product_asin_accuracy(emb, mlp, t, plain, 20) == head.accuracy(emb, t, 20)


def test_end_to_end_against_the_reference_run(cuda):
    """The fixture the reference's own four functions produced (tests/golden/catalogue_heads.npz): kept counts and both
    accuracies exactly, the loss within LOSS_BOUND (tests/test_catalogue_cpu.py) plus the 2^-20 of the device's terms."""
    for tag, g, ks, n_neg in _cases():
        head = catalogue.CatalogueHead(g["table"], device=cuda)
        for which, loss_fn, acc_fn in (("next", catalogue.get_next_product_asin_loss, catalogue.get_next_product_asin_accuracy),
                                       ("all", catalogue.get_all_product_asin_loss, catalogue.get_all_product_asin_accuracy)):
            ptr, items = _targets(g, which)
            t = vectors(ptr, items, cuda)
            got = head.bce(g["rep"], t, n_neg, int(g["seed"]))
            ref = float(g[f"{which}_loss"])
            print(f"{tag} {which}: reference {ref:.9f} device {got.loss:.9f} relative {abs(got.loss - ref) / ref:.3e}")
            assert int(got.counts.sum()) == int(g[f"{which}_kept"])
            assert abs(got.loss - ref) <= (LOSS_BOUND + REL) * ref
            assert loss_fn(g["rep"], None, t, head, cuda, seed=int(g["seed"])) == got.loss
            for K in ks:
                if f"{which}_acc{K}" in g:
                    assert acc_fn(g["rep"], None, t, head, K) == tuple(g[f"{which}_acc{K}"].tolist()), (tag, which, K)
