"""``FlatIndex(d, pad_scan=True)``: a float32 index of a width without a scan of its own (d = 200, the reference's emb_len,
among them) takes the matrix-core scans at the next width they have, over images and queries with exact zero columns, and
re-scores from the d-wide rows.  Whatever serves a query -- scan + proof, threshold rung, exhaustive kernels -- ids and
scores equal the oracle's with ``array_equal``: ``sr.search_exact`` (inner product) or
``sr.topk_from_scores(sr.canonical_l2(q, c), k, largest=False)`` (L2).

Seeded unit rows, n = 20000, nq = 300.  The widths: d = 4 (one 16-byte chunk: the wave-per-query re-score has three empty
parts), 68 / 200 / 252 (uneven parts 5/5/5/2, 13/13/13/11, 16/16/16/15), 260 (rows of 1040 bytes: the rung's LDS-staged
re-score, with a one-chunk tail behind eight full steps; f16 scan at 512 only) and 508 (32/32/32/31)."""

import numpy as np
import pytest
import torch

from oracle import search_ref as sr

pytestmark = pytest.mark.gpu

N, NQ = 20000, 300
KS = (1, 10, 17, 100, 500)
SCANS = ("f16", "split", "f32")
WIDTHS = (4, 68, 200, 252, 260, 508)
CASES = [(d, s) for d in WIDTHS for s in (SCANS if d <= 256 else ("f16",))]
FLT_MAX = np.float32(3.4028234663852886e38)
_cache = {}


def _unit(d, n=N, nq=NQ, seed=None):
    rng = np.random.default_rng(20261018 + d if seed is None else seed)
    c = sr.normalize(rng.standard_normal((n, d)).astype(np.float32)).astype(np.float32)
    q = sr.normalize(rng.standard_normal((nq, d)).astype(np.float32)).astype(np.float32)
    return c, q


def _data(d):
    if ("data", d) not in _cache:
        _cache[("data", d)] = _unit(d)
    return _cache[("data", d)]


def _l2_scores(q, c, block=2048):
    """sr.canonical_l2(q, c), a block of rows at a time (every element is computed by the same chain)."""
    return np.concatenate([sr.canonical_l2(q, c[lo:lo + block]) for lo in range(0, c.shape[0], block)], axis=1)


def _oracle(q, c, k, metric):
    if metric == "ip":
        return sr.search_exact(q, c, k)
    return sr.topk_from_scores(_l2_scores(q, c), k, largest=False)


def _ref(d, metric, k):
    """The oracle's top-k of the seeded rows of width d: the top 500 computed once, its prefixes serve every k."""
    key = ("ref", d, metric)
    if key not in _cache:
        c, q = _data(d)
        _cache[key] = _oracle(q, c, 500, metric)
    D, I = _cache[key]
    return D[:, :k], I[:, :k]


def _padded_index(cuda, d, metric, scan, rows):
    from sessionsimilaritysearch_amd.index import FlatIndex
    idx = FlatIndex(d, metric, cuda, scan=scan, pad_scan=True)
    idx.add(rows)
    return idx


def _index(cuda, d, metric, scan):
    key = ("index", d, metric, scan)
    if key not in _cache:
        _cache[key] = _padded_index(cuda, d, metric, scan, _data(d)[0])
    return _cache[key]


def _equal(got, want):
    D, I = got
    Dr, Ir = want
    assert np.array_equal(I, Ir), int((I != Ir).sum())
    assert np.array_equal(D, Dr), int((D != Dr).sum())


def _route(idx, k):
    return idx.l2_scan_for(k) if idx.metric == "l2" else idx.scan_for(k)


def _zero_extended(x, ds):
    out = np.zeros((x.shape[0], ds), np.float32)
    out[:, :x.shape[1]] = x
    return out


# ------------------------------------------------------------------------------------------- 1. exactness
@pytest.mark.parametrize("metric", ["ip", "l2"])
@pytest.mark.parametrize("d,scan", CASES)
def test_padded_search_is_exact(cuda, d, scan, metric):
    idx = _index(cuda, d, metric, scan)
    assert idx._pad and idx.scan_width(scan) >= d and idx.scan_width(scan) in (64, 128, 256, 512)
    q = _data(d)[1]
    for k in KS:
        assert _route(idx, k) == scan
        _equal(idx.search(q, k), _ref(d, metric, k))
        print(f"pad_scan d={d} {metric} scan={scan} k={k}: unproven {idx.last_rescan_queries} of {NQ}, fallbacks {idx.last_fallback_queries}")
        assert idx.last_scan == scan
        assert idx.last_fallback_queries == 0            # random rows: the rung resolves whatever the scan leaves


def test_default_index_of_the_same_width_stays_exhaustive(cuda):
    """The switch is per index: a default index of width 200 answers as before, and equally."""
    from sessionsimilaritysearch_amd.index import FlatIndex, build_index
    c, q = _data(200)
    idx = FlatIndex(200, "ip", cuda)
    idx.add(c)
    assert idx._pad is False and idx.scan_for(10) == ""
    _equal(idx.search(q[:6], 10), tuple(x[:6] for x in _ref(200, "ip", 10)))
    assert idx.last_fallback_queries == 6
    on = build_index(c, "ip", cuda, pad_scan=True)
    assert on._pad and on.prepare(10) == "f16" and on._f16.shape[1] == 256
    _equal(on.search(q, 10), _ref(200, "ip", 10))
    assert on.last_scan == "f16"


# ------------------------------------------------------------------------------------------- 2. against native code
@pytest.mark.parametrize("metric", ["ip", "l2"])
@pytest.mark.parametrize("scan", SCANS)
@pytest.mark.parametrize("d", [200, 68])
def test_padded_index_equals_the_native_index_over_zero_extended_rows(cuda, d, scan, metric):
    """``FlatIndex(ds)`` over the rows and queries extended with zero columns runs the same scan on the same image under
    the same bound, through code that knows nothing of padding: results AND the count of queries the scan left unproven
    are equal -- no tolerance."""
    from sessionsimilaritysearch_amd.index import FlatIndex
    c, q = _data(d)
    idx = _index(cuda, d, metric, scan)
    ds = idx.scan_width(scan)
    assert ds == {200: 256, 68: 128}[d]
    native = FlatIndex(ds, metric, cuda, scan=scan)
    native.add(_zero_extended(c, ds))
    qz = _zero_extended(q, ds)
    for k in (10, 100):
        got = idx.search(q, k)
        rescans = idx.last_rescan_queries
        want = native.search(qz, k)
        assert native.last_scan == scan == idx.last_scan
        _equal(got, want)
        assert rescans == native.last_rescan_queries, (rescans, native.last_rescan_queries)
        assert native.last_fallback_queries == 0 == idx.last_fallback_queries


# ------------------------------------------------------------------------------------------- 3. ties
@pytest.mark.parametrize("metric", ["ip", "l2"])
@pytest.mark.parametrize("scan", SCANS)
def test_forty_copies_force_the_rung(cuda, scan, metric):
    c, q = _data(200)
    c, q = c.copy(), q[:40].copy()
    dup = np.arange(40) * 101 + 13
    c[dup] = c[5]
    q[0] = c[5]
    idx = _padded_index(cuda, 200, metric, scan, c)
    Dr, Ir = _oracle(q, c, 10, metric)
    assert Ir[0].tolist() == sorted([5] + dup.tolist())[:10] and (Dr[0] == Dr[0, 0]).all()     # lowest ids first
    _equal(idx.search(q, 10), (Dr, Ir))
    assert idx.last_scan == scan and idx.last_rescan_queries >= 1 and idx.last_fallback_queries == 0


@pytest.mark.parametrize("metric", ["ip", "l2"])
def test_more_copies_than_the_rung_holds_reach_the_exhaustive_kernels(cuda, metric):
    """9000 copies, above the rung's 8192: the query goes to the exhaustive kernels, which read d-wide rows and so must
    be handed the ORIGINAL queries -- the padded batch would be read at the wrong stride."""
    c, q = _data(200)
    c, q = c.copy(), q[:33].copy()
    c[1000:10000] = c[0]
    q[3] = c[0]
    idx = _padded_index(cuda, 200, metric, "f16", c)
    Dr, Ir = _oracle(q, c, 10, metric)
    assert Ir[3].tolist() == [0] + list(range(1000, 1009))
    _equal(idx.search(q, 10), (Dr, Ir))
    assert idx.last_scan == "f16" and idx.last_fallback_queries >= 1


# ------------------------------------------------------------------------------------------- 4. streaming
@pytest.mark.parametrize("metric", ["ip", "l2"])
@pytest.mark.parametrize("scan", SCANS)
def test_streaming_adds_reshift_and_adopt(cuda, scan, metric):
    from sessionsimilaritysearch_amd.index import FlatIndex
    c, q = _data(200)
    q = q[:64]
    idx = FlatIndex(200, metric, cuda, scan=scan, pad_scan=True)
    for lo, hi in ((0, 1), (1, 5000), (5000, N)):
        idx.add(c[lo:hi])
        idx.prepare(10)                                   # the images are extended batch by batch
    want = tuple(x[:64] for x in _ref(200, metric, 10))
    _equal(idx.search(q, 10), want)                       # ... to what one add builds
    assert idx.last_scan == scan and idx.last_fallback_queries == 0
    if scan != "f16":                                     # (the f16 image's shift depends on which rows came first)
        image = {"split": idx._split, "f32": idx._p32}[scan]
        one = _index(cuda, 200, metric, scan)
        one.prepare(10)
        whole = {"split": one._split, "f32": one._p32}[scan]
        assert image.shape[1] == {"split": 512, "f32": 256}[scan] and torch.equal(image[:N], whole[:N])
    # one row 2^4 times larger than any element: the f16 image is rebuilt under a new shift
    from sessionsimilaritysearch_amd import _lib
    shift = idx._c_shift
    big = (c[7:8] * np.float32(16.0 / np.abs(c[7]).max() * np.abs(c).max())).astype(np.float32)
    idx.add(big)
    c2 = np.concatenate([c, big])
    _equal(idx.search(q, 10), _oracle(q, c2, 10, metric))
    if scan == "f16":
        assert idx._c_shift == _lib.lib().sss_f16_shift(float(np.abs(big).max())) < shift and idx._f16_done == N + 1
    dropped = idx.adopt(torch.from_numpy(c[3000:9000]).to(cuda))
    assert dropped._f16 is None and dropped._split is None and dropped._p32 is None and dropped._bias is None
    _equal(idx.search(q, 10), _oracle(q, c[3000:9000], 10, metric))
    assert idx.last_scan == scan


# ------------------------------------------------------------------------------------------- 5. L2 away from unit norms
def _varnorm(d):
    """The "varnorm" construction of tests/test_l2_scan_gpu.py: directions of normal rows, norms log-uniform in [1/4, 4]."""
    rng = np.random.default_rng(20261017)
    c = rng.standard_normal((N, d)).astype(np.float32)
    q = rng.standard_normal((NQ, d)).astype(np.float32)
    s = np.exp(rng.uniform(np.log(.25), np.log(4), N)).astype(np.float32)
    c2 = (c / np.linalg.norm(c, axis=1, keepdims=True) * s[:, None]).astype(np.float32)
    q2 = (q / np.linalg.norm(q, axis=1, keepdims=True) * np.exp(rng.uniform(np.log(.25), np.log(4), NQ))[:, None]).astype(np.float32)
    return c2, q2


@pytest.mark.parametrize("scan", SCANS)
def test_l2_varnorm_is_exact_on_every_scan(cuda, scan):
    if "varnorm" not in _cache:
        c, q = _varnorm(200)
        _cache["varnorm"] = (c, q, _oracle(q, c, 10, "l2"))
    c, q, want = _cache["varnorm"]
    idx = _padded_index(cuda, 200, "l2", scan, c)
    _equal(idx.search(q, 10), want)
    assert idx.last_scan == scan
    print(f"pad_scan varnorm l2 scan={scan}: unproven {idx.last_rescan_queries} of {NQ}, fallbacks {idx.last_fallback_queries}")


# ------------------------------------------------------------------------------------------- 6. other routes
@pytest.mark.parametrize("metric", ["ip", "l2"])
def test_range_search_stays_on_the_exhaustive_route(cuda, metric):
    c, q = _data(200)
    c, q = c[:6000], q[:32]
    idx = _padded_index(cuda, 200, metric, "auto", c)
    s = sr.canonical_scores(q, c) if metric == "ip" else sr.canonical_l2(q, c)
    r = np.float32(np.quantile(s, 1.0 - 30 / 6000 if metric == "ip" else 30 / 6000))
    lims, D, I = idx.range_search(q, float(r))
    assert idx.last_range_scan == "" and idx.last_range_overflow_queries == 0
    keep = s > r if metric == "ip" else s < r
    assert np.array_equal(lims, np.concatenate([[0], np.cumsum(keep.sum(1))])) and lims[-1] > 32 * 5
    assert np.array_equal(I, np.nonzero(keep)[1]) and np.array_equal(D, s[keep])


def _sweep_search(c, q, k, metric, S, dev):
    """search() of S padded shards without a process group: local search + fix, pack, stack, merge."""
    from sessionsimilaritysearch_amd.distributed import HipEngine, ShardedFlatIndex, shard_range
    from sessionsimilaritysearch_amd.index import FlatIndex
    shards = []
    for s in range(S):
        lo, hi = shard_range(c.shape[0], S, s)
        shards.append(ShardedFlatIndex(HipEngine(FlatIndex(c.shape[1], metric, dev, pad_scan=True).adopt(c[lo:hi], id_offset=lo)), dev))
    nq = q.shape[0]
    chunk = shards[0]._buffers(nq, k)[0]
    stacked = torch.empty(S * chunk, dtype=torch.int64, device=dev)
    for s, sh in enumerate(shards):
        _, _, _, D, I, status, _, _ = sh._buffers(nq, k)
        sh.engine.local_search(q, k, D, I, status)
        sh.engine.fix_unproven(q, k, D, I, status)
        stacked[s * chunk:(s + 1) * chunk] = sh._pack_for_exchange(nq, k)
    D, I = shards[0]._merge(stacked, S, nq, k)
    return D.cpu().numpy(), I.cpu().numpy(), [sh.engine.index.last_scan for sh in shards]


@pytest.mark.parametrize("metric", ["ip", "l2"])
def test_four_padded_shards_equal_the_whole_index(cuda, metric):
    c_h, q_h = _data(200)
    c, q = torch.from_numpy(c_h).to(cuda), torch.from_numpy(q_h).to(cuda)
    D, I, scans = _sweep_search(c, q, 10, metric, 4, cuda)
    _equal((D, I), _ref(200, metric, 10))
    assert scans == ["f16"] * 4
    _equal(_index(cuda, 200, metric, "f16").search(q_h, 10), (D, I))


# ------------------------------------------------------------------------------------------- 7. C ABI
def _abi(cuda, d=200, ds=256, n=2048 + 37, nq=8, k=10):
    from sessionsimilaritysearch_amd import _lib
    L = _lib.lib()
    c_h, q_h = _unit(d, n, nq, seed=5)
    t = {"c": torch.from_numpy(c_h).to(cuda), "q": torch.from_numpy(q_h).to(cuda),
         "qp": torch.full((nq, ds), 9.0, dtype=torch.float32, device=cuda),
         "bias": torch.zeros(n + 4, dtype=torch.float32, device=cuda),
         "D": torch.full((nq, k), 7.0, dtype=torch.float32, device=cuda), "I": torch.full((nq, k), 7, dtype=torch.int64, device=cuda),
         "status": torch.full((nq,), 7, dtype=torch.int32, device=cuda),
         "state": torch.zeros(L.sss_ip_topk_state_bytes(nq), dtype=torch.uint8, device=cuda),
         "cmax": torch.zeros(1, dtype=torch.float32, device=cuda), "sel": torch.arange(nq, dtype=torch.int32, device=cuda)}
    assert L.sss_row_norm_max(t["c"].data_ptr(), n, d, 0, t["cmax"].data_ptr(), None) == 0
    assert L.sss_pad_rows_f32(t["q"].data_ptr(), nq, d, ds, t["qp"].data_ptr(), None) == 0
    assert L.sss_l2_row_bias(t["c"].data_ptr(), n, d, t["bias"].data_ptr(), None) == 0
    return L, (n, d, ds, nq, k), t, c_h, q_h


def _untouched(t):
    torch.cuda.synchronize()
    return bool((t["D"] == 7.0).all()) and bool((t["I"] == 7).all()) and bool((t["status"] == 7).all()) and not bool(t["state"].any())


def _images(L, t, n, d, ds, cuda):
    """(image tensor, scan code, shift, resid) per scan, built by the padded builders."""
    amax = torch.zeros(1, dtype=torch.float32, device=cuda)
    assert L.sss_abs_max(t["c"].data_ptr(), n * d, amax.data_ptr(), None) == 0
    shift = int(L.sss_f16_shift(float(amax.item())))
    f16 = torch.full((n + 1, ds), 3.0, dtype=torch.float16, device=cuda)
    split = torch.full((n + 1, 2 * ds), 3.0, dtype=torch.bfloat16, device=cuda)
    p32 = torch.full((n + 1, ds), 3.0, dtype=torch.float32, device=cuda)
    resid = torch.zeros(1, dtype=torch.float32, device=cuda)
    assert L.sss_pad_scale_f16(t["c"].data_ptr(), n, d, ds, shift, f16.data_ptr(), None) == 0
    assert L.sss_pad_f16_resid_max(t["c"].data_ptr(), f16.data_ptr(), n, d, ds, shift, resid.data_ptr(), None) == 0
    assert L.sss_pad_split_bf16(t["c"].data_ptr(), n, d, ds, split.data_ptr(), None) == 0
    assert L.sss_pad_rows_f32(t["c"].data_ptr(), n, d, ds, p32.data_ptr(), None) == 0
    return {"f16": (f16, 3, shift, float(resid.item())), "split": (split, 2, 0, 0.0), "f32": (p32, 0, 0, 0.0)}


@pytest.mark.parametrize("d,ds", [(200, 256), (4, 128), (68, 128), (260, 512)])
def test_builders_equal_the_native_builders_over_zero_extended_rows(cuda, d, ds):
    """Bit for bit: the padded images are the native images of the zero-extended rows (+0 in every padding column, the
    same shift rule and roundings), for an n that is no multiple of any block's rows, and nothing behind row n - 1 is
    written.  The residual norm is the same sum of squares in another order, rounded up to float32 once: within one
    float32 ulp (2^-23 relative)."""
    L, (n, _, _, nq, k), t, c_h, q_h = _abi(cuda, d, ds)
    img = _images(L, t, n, d, ds, cuda)
    cz = torch.from_numpy(_zero_extended(c_h, ds)).to(cuda)
    f16, _, shift, resid = img["f16"]
    want16 = torch.empty((n, ds), dtype=torch.float16, device=cuda)
    assert L.sss_scale_f16(cz.data_ptr(), n * ds, shift, want16.data_ptr(), None) == 0
    want_resid = torch.zeros(1, dtype=torch.float32, device=cuda)
    assert L.sss_f16_resid_max(cz.data_ptr(), want16.data_ptr(), n, ds, shift, want_resid.data_ptr(), None) == 0
    assert torch.equal(f16[:n].view(torch.int16), want16.view(torch.int16)) and bool((f16[n] == 3.0).all())
    assert bool((f16[:n, d:].view(torch.int16) == 0).all())                     # +0, not -0
    assert resid > 0 and abs(resid - float(want_resid.item())) <= 2.0 ** -23 * resid
    if ds <= 256:
        split = img["split"][0]
        want_split = torch.empty((n, 2 * ds), dtype=torch.bfloat16, device=cuda)
        assert L.sss_split_bf16(cz.data_ptr(), n, ds, want_split.data_ptr(), None) == 0
        assert torch.equal(split[:n].view(torch.int16), want_split.view(torch.int16)) and bool((split[n] == 3.0).all())
    p32 = img["f32"][0]
    assert torch.equal(p32[:n].view(torch.int32), cz.view(torch.int32)) and bool((p32[n] == 3.0).all())
    assert torch.equal(t["qp"].view(torch.int32), torch.from_numpy(_zero_extended(q_h, ds)).to(cuda).view(torch.int32))


@pytest.mark.parametrize("metric", ["ip", "l2"])
@pytest.mark.parametrize("scan", SCANS)
def test_abi_topk_workspace_state_and_stream(cuda, scan, metric):
    L, (n, d, ds, nq, k), t, c_h, q_h = _abi(cuda)
    image, code, shift, resid = _images(L, t, n, d, ds, cuda)[scan]
    cmax = float(t["cmax"].item())
    bias = t["bias"].data_ptr() if metric == "l2" else None
    nbytes = L.sss_pad_topk_workspace_bytes(nq, n, d, ds, k, code)
    assert nbytes > 0
    ws = torch.empty(nbytes, dtype=torch.uint8, device=cuda)

    def call(stream=None, ws_bytes=nbytes, state_bytes=None, d_row=d):
        return L.sss_pad_topk(t["qp"].data_ptr(), nq, t["c"].data_ptr(), image.data_ptr(), code, shift, resid, bias, n, d_row, ds, k, 0,
                              cmax, t["D"].data_ptr(), t["I"].data_ptr(), t["status"].data_ptr(), None, t["state"].data_ptr(),
                              t["state"].numel() if state_bytes is None else state_bytes, ws.data_ptr(), ws_bytes, stream)

    for rc, want in ((call(ws_bytes=nbytes - 1), -2), (call(state_bytes=16), -2), (call(d_row=202), -1), (call(d_row=260), -1)):
        assert rc == want
        assert L.sss_last_error().decode().startswith("pad_topk:"), L.sss_last_error()
        assert _untouched(t)                                                     # a failing call writes nothing
    assert call() == 0
    torch.cuda.synchronize()
    assert not bool(t["state"].any())                                            # handed back zeroed
    Dr, Ir = _oracle(q_h, c_h, k, metric)
    ok = t["status"].cpu().numpy() == 0
    D0, I0, st0 = t["D"].clone(), t["I"].clone(), t["status"].clone()
    assert ok.any() and np.array_equal(I0.cpu().numpy()[ok], Ir[ok]) and np.array_equal(D0.cpu().numpy()[ok], Dr[ok])
    t["D"].fill_(7.0), t["I"].fill_(7), t["status"].fill_(7)
    side = torch.cuda.Stream(device=cuda)
    torch.cuda.synchronize()
    assert call(stream=side.cuda_stream) == 0
    side.synchronize()
    assert torch.equal(t["D"], D0) and torch.equal(t["I"], I0) and torch.equal(t["status"], st0) and not bool(t["state"].any())


@pytest.mark.parametrize("metric", ["ip", "l2"])
@pytest.mark.parametrize("scan", SCANS)
def test_abi_threshold_workspace_and_stream(cuda, scan, metric):
    L, (n, d, ds, nq, k), t, c_h, q_h = _abi(cuda)
    image, code, shift, resid = _images(L, t, n, d, ds, cuda)[scan]
    cmax = float(t["cmax"].item())
    bias = t["bias"].data_ptr() if metric == "l2" else None
    nbytes = L.sss_pad_topk_threshold_workspace_bytes(nq, n, d, ds, code)
    assert nbytes > 0
    ws = torch.empty(nbytes, dtype=torch.uint8, device=cuda)

    def call(stream=None, ws_bytes=nbytes, d_row=d):
        return L.sss_pad_topk_threshold(t["qp"].data_ptr(), t["sel"].data_ptr(), nq, t["c"].data_ptr(), image.data_ptr(), code, shift,
                                        resid, bias, n, d_row, ds, k, 0, cmax, t["D"].data_ptr(), t["I"].data_ptr(),
                                        t["status"].data_ptr(), ws.data_ptr(), ws_bytes, stream)

    for rc, want in ((call(ws_bytes=nbytes - 1), -2), (call(d_row=202), -1), (call(d_row=260), -1)):
        assert rc == want
        assert L.sss_last_error().decode().startswith("pad_topk_threshold:"), L.sss_last_error()
        assert _untouched(t)
    # no k-th score known (the padding value in column k-1): the rung keeps every row -- 2085 of them, within its capacity
    none_known = float(FLT_MAX) if metric == "l2" else -float(FLT_MAX)
    Dr, Ir = _oracle(q_h, c_h, k, metric)
    for stream in (None, torch.cuda.Stream(device=cuda)):
        t["D"].fill_(none_known), t["I"].fill_(7), t["status"].fill_(7)
        torch.cuda.synchronize()
        assert call(stream=None if stream is None else stream.cuda_stream) == 0
        torch.cuda.synchronize()
        assert bool((t["status"] == 0).all())
        assert np.array_equal(t["I"].cpu().numpy(), Ir) and np.array_equal(t["D"].cpu().numpy(), Dr)
