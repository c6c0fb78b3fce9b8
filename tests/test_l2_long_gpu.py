"""L2 top-k on the long-row scan: ``FlatIndex(d, "l2")`` of a float32 index whose rows are beyond the fused scans
(d % 64 == 0 from 320 up; the reference's own 1600) takes the K-tiled matrix-core scan (``l2_long_for``,
``sss_l2_topk_long``) instead of the exhaustive kernels, and whatever route serves a query, ids and distances equal the
oracle's -- ``oracle.search_ref.build_index(c, "l2").search(q, k)`` -- with ``array_equal``.

The oracle scores every (query, row) pair on its own, so it is applied to blocks of rows (threads; a block's float64
copy stays in cache) and the blocks' results merged by (distance asc, id asc): the same (D, I) as one call over all rows,
in seconds instead of a minute at 450 001 rows.

Rows are "varnorm": Gaussian directions with norms log-uniform in [1/4, 4].  On unit rows the L2 order is the
inner-product order and a missing or mis-indexed bias would go unnoticed."""
import os
import sys

import numpy as np
import pytest
import torch

from oracle import search_ref as sr

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
from l2_long_ref import ORACLE_BLOCK, _equal, _oracle, _varnorm  # noqa: E402

pytestmark = pytest.mark.gpu
FLT_MAX = np.float32(3.4028234663852886e38)


def _l2_index(cuda, c):
    from sessionsimilaritysearch_amd.index import FlatIndex
    idx = FlatIndex(c.shape[1], "l2", cuda)
    idx.add(c)
    return idx


# ------------------------------------------------------------------------------------------- 1. route, level plan
@pytest.mark.parametrize("nq,n,d,k", [
    (8, 3000, 1600, 100),           # one level
    (33, 20_000, 320, 500),         # shortest long row, large k
    (5, 20_000, 320, 1024),         # largest k, growth factor 2
    (37, 70_001, 320, 10),          # ragged last tile, one big factor
    (50, 300_000, 320, 100),        # three levels: the disjoint schedule, every 6th tile sampled
    (37, 450_001, 320, 100),        # every 7th tile, ragged
])
def test_l2_long_route_is_taken_and_exact(cuda, nq, n, d, k):
    """The cap on fallbacks keeps the test from passing on the exhaustive route alone.  Measured on an MI355X: 0
    fallbacks at every shape (DESIGN 3 has the table)."""
    c, q = _varnorm(n, d, nq, n + d + k)
    idx = _l2_index(cuda, c)
    assert idx.l2_long_for(k) == "long" and idx.l2_scan_for(k) == ""
    _equal(idx.search(q, k), _oracle(q, c, k))
    assert idx.last_scan == "long"
    print(f"l2 long: nq={nq} n={n} d={d} k={k}: unproven {idx.last_rescan_queries}, fallbacks {idx.last_fallback_queries}")
    if n <= 8192:
        assert idx.last_fallback_queries == 0
    else:
        assert idx.last_fallback_queries <= nq // 10


# ------------------------------------------------------------------------------------------- 2. bias indexed by row
@pytest.mark.parametrize("descending", [False, True])
def test_l2_long_bias_is_indexed_by_row(cuda, descending):
    """Rows in the order of their norms; the query at the origin is nearest to the smallest-norm rows whatever q.c says
    (it is 0 for every row): a bias read from another row, block or tile picks other rows."""
    c, q = _varnorm(20_000, 320, 9, 77)
    order = np.argsort(np.linalg.norm(c.astype(np.float64), axis=1), kind="stable")
    c = np.ascontiguousarray(c[order[::-1] if descending else order])
    q[0] = 0
    idx = _l2_index(cuda, c)
    Dr, Ir = _oracle(q, c, 10)
    assert set(Ir[0].tolist()) == set(range(19_990, 20_000) if descending else range(10))
    _equal(idx.search(q, 10), (Dr, Ir))
    assert idx.last_scan == "long"


# ------------------------------------------------------------------------------------------- 3. ties, duplicates
def test_l2_long_duplicates_within_capacity(cuda):
    """40 copies of the row nearest to query 0 at scattered ids: the long route itself resolves the tie, ids ascending."""
    c, q = _varnorm(20_000, 320, 16, 78)
    dup = np.arange(40) * 487 + 13
    c[dup] = c[5]
    q[0] = c[5] + np.float32(0.001)
    idx = _l2_index(cuda, c)
    Dr, Ir = _oracle(q, c, 10)
    assert Ir[0].tolist() == sorted([5] + dup.tolist())[:10] and (Dr[0] == Dr[0, 0]).all()
    _equal(idx.search(q, 10), (Dr, Ir))
    assert idx.last_scan == "long" and idx.last_fallback_queries == 0


def test_l2_long_more_duplicates_than_capacity_go_exhaustive(cuda):
    """9000 copies, above the 8192 rows a query may keep, nearest to query 1: the exhaustive kernels resolve it."""
    c, q = _varnorm(20_000, 320, 16, 79)
    c[1000:10_000] = c[0]
    q[1] = c[0]
    idx = _l2_index(cuda, c)
    Dr, Ir = _oracle(q, c, 10)
    assert Dr[1, 9] == 0 and Ir[1].tolist() == [0] + list(range(1000, 1009))
    _equal(idx.search(q, 10), (Dr, Ir))
    assert idx.last_scan == "long" and idx.last_fallback_queries >= 1


# ------------------------------------------------------------------------------------------- 4. magnitudes
def _magnitude_case(name):
    c, q = _varnorm(3000, 320, 12, 80)
    if name == "both*2^40":
        return c * np.float32(2.0 ** 40), q * np.float32(2.0 ** 40), "long"
    if name == "both*2^-40":
        return c * np.float32(2.0 ** -40), q * np.float32(2.0 ** -40), "long"
    if name == "corpus*2^70":
        return c * np.float32(2.0 ** 70), q, ""
    if name == "queries*2^100":
        return c, q * np.float32(2.0 ** 100), "long"
    if name == "queries*2^-100":
        return c, q * np.float32(2.0 ** -100), "long"
    assert name == "shift+100"
    return (c + np.float32(100)).astype(np.float32), (q + np.float32(100)).astype(np.float32), "long"


@pytest.mark.parametrize("name", ["both*2^40", "both*2^-40", "corpus*2^70", "queries*2^100", "queries*2^-100", "shift+100"])
def test_l2_long_magnitudes(cuda, name):
    """Exact at every magnitude.  The route follows the CORPUS (largest row norm in [2^-60, 2^60]); a query whose own
    magnitude puts the scan's bound beyond float32 is resolved exhaustively, whatever the route."""
    c, q, route = _magnitude_case(name)
    idx = _l2_index(cuda, c)
    assert idx.l2_long_for(10) == route
    _equal(idx.search(q, 10), _oracle(q, c, 10))
    print(f"l2 long magnitudes: {name}: route {idx.last_scan if route else 'exhaustive'!r}, unproven {idx.last_rescan_queries}, "
          f"fallbacks {idx.last_fallback_queries} of {q.shape[0]}")
    if route:
        assert idx.last_scan == "long"
    else:
        assert idx.last_fallback_queries == q.shape[0]


# ------------------------------------------------------------------------------------------- 5. index plumbing
def test_l2_long_index_plumbing(cuda):
    from sessionsimilaritysearch_amd.index import FlatIndex
    c, q = _varnorm(9000, 320, 9, 81)
    idx = FlatIndex(320, "l2", cuda)
    idx.add(c[:4000])
    assert idx.prepare(100) == "long" and idx._bias_done == 4000
    _equal(idx.search(q, 10), _oracle(q, c[:4000], 10))
    idx.add(c[4000:])
    _equal(idx.search(q, 10), _oracle(q, c, 10))
    assert idx.last_scan == "long" and idx._bias_done == idx.ntotal == 9000 and idx._f16_done == 9000
    want = (-0.5 * (c.astype(np.float64) ** 2).sum(1)).astype(np.float32)
    assert np.allclose(idx._bias[:9000].cpu().numpy(), want, rtol=3e-7, atol=0)

    idx.adopt(torch.from_numpy(c[2000:7000]).to(cuda), id_offset=12345)
    assert idx._bias is None and idx._bias_done == 0
    Dr, Ir = _oracle(q, c[2000:7000], 10)
    _equal(idx.search(q, 10), (Dr, Ir + 12345))
    assert idx.last_scan == "long" and idx._bias_done == 5000

    few = _l2_index(cuda, c[:50])                                            # n < k: padding
    D, I = few.search(q, 100)
    _equal((D, I), _oracle(q, c[:50], 100))
    assert few.last_scan == "long" and (I[:, 50:] == -1).all() and (D[:, 50:] == FLT_MAX).all() and (I[:, :50] >= 0).all()

    wide = np.random.default_rng(82).standard_normal((300, 1600)).astype(np.float32)
    bf = FlatIndex(1600, "l2", cuda, dtype="bf16")                           # 16-bit rows have no L2 scan anywhere
    bf.add(wide)
    assert bf._route(10) == "" and bf.l2_long_for(10) == ""


# ------------------------------------------------------------------------------------------- 6. shards
def test_l2_long_sharded(cuda):
    from sessionsimilaritysearch_amd.distributed import HipEngine, ShardedFlatIndex, shard_range
    from sessionsimilaritysearch_amd.index import FlatIndex
    c_h, q_h = _varnorm(20_000, 320, 33, 83)
    c, q = torch.from_numpy(c_h).to(cuda), torch.from_numpy(q_h).to(cuda)
    S, k, nq = 2, 10, q_h.shape[0]
    shards = []
    for s in range(S):
        lo, hi = shard_range(c.shape[0], S, s)
        shards.append(ShardedFlatIndex(HipEngine(FlatIndex(320, "l2", cuda).adopt(c[lo:hi], id_offset=lo)), cuda))
    chunk = shards[0]._buffers(nq, k)[0]
    stacked = torch.empty(S * chunk, dtype=torch.int64, device=cuda)
    for s, sh in enumerate(shards):
        _, _, _, D, I, status, _, _ = sh._buffers(nq, k)
        sh.engine.local_search(q, k, D, I, status)
        sh.engine.fix_unproven(q, k, D, I, status)
        stacked[s * chunk:(s + 1) * chunk] = sh._pack_for_exchange(nq, k)
    D, I = shards[0]._merge(stacked, S, nq, k)
    want = _oracle(q_h, c_h, k)
    _equal((D.cpu().numpy(), I.cpu().numpy()), want)
    assert [sh.engine.index.last_scan for sh in shards] == ["long"] * S
    _equal(_l2_index(cuda, c_h).search(q_h, k), want)


# ------------------------------------------------------------------------------------------- 7. C ABI
def test_l2_long_abi_guards_and_result(cuda):
    """A refused call returns its code, names the entry point and writes nothing."""
    from sessionsimilaritysearch_amd import _lib
    L = _lib.lib()
    n, d, nq, k = 3000, 320, 8, 10
    c_h, q_h = _varnorm(n, d, nq, 84)
    idx = _l2_index(cuda, c_h)
    assert idx.prepare(k) == "long"
    image, _, shift, resid = idx._scan_image("long")
    qt = torch.from_numpy(q_h).to(cuda)
    D = torch.full((nq, k), 7.0, dtype=torch.float32, device=cuda)
    I = torch.full((nq, k), 7, dtype=torch.int64, device=cuda)
    status = torch.full((nq,), 7, dtype=torch.int32, device=cuda)
    nbytes = L.sss_l2_topk_long_workspace_bytes(nq, n, d)
    assert nbytes >= L.sss_ip_topk_long_workspace_bytes(nq, n, d, 0) > 0
    ws = torch.empty(nbytes + 256, dtype=torch.uint8, device=cuda)
    assert ws.data_ptr() % 256 == 0

    def call(bias=None, ws_ptr=None, ws_bytes=nbytes, k_=k, d_=d):
        return L.sss_l2_topk_long(qt.data_ptr(), nq, idx._xb.data_ptr(), image.data_ptr(), shift, resid,
                                  idx._bias.data_ptr() if bias is None else bias, n, d_, k_, 0, idx.corpus_max_norm(),
                                  D.data_ptr(), I.data_ptr(), status.data_ptr(), ws.data_ptr() if ws_ptr is None else ws_ptr,
                                  ws_bytes, None)

    for what, kwargs, want in (("null bias", dict(bias=0), -1), ("misaligned workspace", dict(ws_ptr=ws.data_ptr() + 16), -1),
                               ("short workspace", dict(ws_bytes=nbytes - 1), -2), ("k = 1025", dict(k_=1025), -1),
                               ("d = 200", dict(d_=200), -1)):
        rc = call(**kwargs)
        assert rc == want, (what, rc)
        assert L.sss_last_error().decode().startswith("l2_topk_long"), (what, L.sss_last_error())
        torch.cuda.synchronize()
        assert bool((D == 7.0).all()) and bool((I == 7).all()) and bool((status == 7).all()), what
    assert call() == 0, L.sss_last_error()
    torch.cuda.synchronize()
    assert bool((status == 0).all())                                        # 3000 rows: nothing can exceed the capacity
    _equal((D.cpu().numpy(), I.cpu().numpy()), _oracle(q_h, c_h, k))


def test_l2_long_abi_unresolved_query_leaves_a_distance_bound(cuda):
    """The C entry point itself, no fix-up behind it: 9000 copies of query 1's nearest row overflow the 8192-row capacity,
    so that query stays at status 1 -- and column k-1 of its row of D_out is what the header promises: an upper bound of
    its true k-th distance (here 0) in the DISTANCE domain, or +FLT_MAX.  Resolved queries are exact."""
    from sessionsimilaritysearch_amd import _lib
    L = _lib.lib()
    n, d, nq, k = 20_000, 320, 16, 10
    c_h, q_h = _varnorm(n, d, nq, 79)
    c_h[1000:10_000] = c_h[0]
    q_h[1] = c_h[0]
    idx = _l2_index(cuda, c_h)
    assert idx.prepare(k) == "long"
    image, _, shift, resid = idx._scan_image("long")
    qt = torch.from_numpy(q_h).to(cuda)
    D = torch.full((nq, k), -7.0, dtype=torch.float32, device=cuda)
    I = torch.full((nq, k), 7, dtype=torch.int64, device=cuda)
    status = torch.full((nq,), 7, dtype=torch.int32, device=cuda)
    ws = torch.empty(L.sss_l2_topk_long_workspace_bytes(nq, n, d), dtype=torch.uint8, device=cuda)
    rc = L.sss_l2_topk_long(qt.data_ptr(), nq, idx._xb.data_ptr(), image.data_ptr(), shift, resid, idx._bias.data_ptr(), n, d, k, 0,
                            idx.corpus_max_norm(), D.data_ptr(), I.data_ptr(), status.data_ptr(), ws.data_ptr(), ws.numel(), None)
    assert rc == 0, L.sss_last_error()
    torch.cuda.synchronize()
    st, Dg, Ig = status.cpu().numpy(), D.cpu().numpy(), I.cpu().numpy()
    Dr, Ir = _oracle(q_h, c_h, k)
    assert st[1] == 1 and set(st.tolist()) <= {0, 1}
    for qi in np.flatnonzero(st):
        assert Dg[qi, k - 1] >= Dr[qi, k - 1] and Dg[qi, k - 1] >= 0, (qi, Dg[qi, k - 1], Dr[qi, k - 1])
    print(f"l2 long abi: status-1 queries {np.flatnonzero(st).tolist()}, their column k-1 {Dg[st != 0, k - 1].tolist()}")
    ok = st == 0
    assert ok.sum() >= nq - 2
    assert np.array_equal(Ig[ok], Ir[ok]) and np.array_equal(Dg[ok], Dr[ok])


def test_blocked_oracle_equals_one_call():
    """The row-blocked use of the oracle (``_oracle`` beyond 16 384 rows) against ONE ``build_index(c, "l2").search(q, k)``
    over all rows: three blocks, the last ragged, ties across blocks (duplicate rows), k larger than what a block holds of
    the answer.  Needs no device, but lives with the helper it checks."""
    c, q = _varnorm(2 * ORACLE_BLOCK + 1234, 64, 7, 85)
    c[ORACLE_BLOCK + 5] = c[3]
    c[2 * ORACLE_BLOCK + 9] = c[3]
    q[0] = c[3]
    want = sr.build_index(c, "l2").search(q, 50)
    assert want[1][0, :3].tolist() == [3, ORACLE_BLOCK + 5, 2 * ORACLE_BLOCK + 9]
    _equal(_oracle(q, c, 50), want)
