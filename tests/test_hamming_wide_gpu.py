"""Binary codes of up to 2048 bits on the GPU: ``BinaryFlatIndex`` with rows stored in 128 / 256 bytes (1024 / 2048
bits; 1032 and 1600 bits padded up), the fused scan (``k_hamming_scan_wide``) and the exhaustive kernels at the new
widths, through the index and straight through the C ABI with guarded buffers.  Every comparison is ``np.array_equal``
on D and I against ``oracle.search_ref.hamming_search``: integer distances, no tolerance."""
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest
import torch

from oracle import search_ref as sr
from sessionsimilaritysearch_amd import _lib

pytestmark = pytest.mark.gpu

GUARD = 4096
OFF = 2 ** 33 + 5                       # id_offset: catches a 32-bit id anywhere on the way out


def L():
    return _lib.lib()


def _st():
    return torch.cuda.current_stream().cuda_stream


def _oracle(q, codes, k, id_offset=0):
    """``sr.hamming_search`` query block by query block (queries are independent) on a few threads: the 1600-bit case
    over 200 000 rows is minutes of numpy on one."""
    step = max(1, min(32, (q.shape[0] + 7) // 8))
    blocks = [q[lo:lo + step] for lo in range(0, q.shape[0], step)]
    with ThreadPoolExecutor(8) as pool:
        out = list(pool.map(lambda b: sr.hamming_search(b, codes, k, id_offset), blocks))
    return np.concatenate([o[0] for o in out]), np.concatenate([o[1] for o in out])


def _random_case(seed, nq, n, nbits):
    """Random codes [n, nbits / 8] and queries that are noisy copies of corpus rows (20 % of the bits flipped)."""
    rng = np.random.default_rng(seed)
    codes = rng.integers(0, 256, (n, nbits // 8), dtype=np.uint8)
    src = rng.integers(0, n, nq)
    flip = np.packbits(rng.random((nq, nbits)) < 0.2, axis=1)
    return codes, codes[src] ^ flip, src


def _signs(codes):
    """The +-1 float32 matrix whose sign bits are `codes` (what pack_sign_bits takes)."""
    return np.unpackbits(codes, axis=1).astype(np.float32) * 2.0 - 1.0


def _crowded(Ir, nq, n):
    """Per query: does some candidate list hold 16 or more of its true results?  Row id belongs to list
    (id // 256) % S, S = capacity / 16 (256-row tiles dealt round-robin, at every code width: hamming.hip); a list keeps
    16 rows, so only such a query can lose its proof.  A property of the inputs and the oracle (ids without offset) alone."""
    S = L().sss_hamming_topk_capacity(nq, n) // 16
    return np.array([np.bincount((row[row >= 0] // 256) % S, minlength=S).max() >= 16 for row in Ir])


CASES = [(300, 20000, 1024, 100), (64, 5000, 2048, 10), (1024, 200000, 1600, 100), (17, 3000, 1032, 100),
         (5, 40, 2048, 100),            # fewer rows than k: padding
         (257, 70000, 1600, 1)]         # a second query group, a ragged last tile


@pytest.mark.parametrize("nq,n,nbits,k", CASES)
def test_wide_hamming_search_matches_oracle(cuda, nq, n, nbits, k):
    from sessionsimilaritysearch_amd.index import BinaryFlatIndex, pack_sign_bits
    codes, qcodes, _ = _random_case(161 + n, nq, n, nbits)
    idx = BinaryFlatIndex(nbits, cuda)
    assert idx._w == (128 if nbits <= 1024 else 256)
    half = n // 2
    for lo in range(0, half, 20000):                                # device-packed rows ...
        idx.add(pack_sign_bits(_signs(codes[lo:min(half, lo + 20000)])))
    idx.add(codes[half:])                                           # ... and host-packed rows mix
    assert idx.ntotal == n
    D, I = idx.search(qcodes, k)
    Dr, Ir = _oracle(qcodes, codes, k)
    assert D.dtype == np.int32 and I.dtype == np.int64
    assert np.array_equal(D, Dr) and np.array_equal(I, Ir)
    # the fused scan, not the fallback, is what answered
    if k <= L().sss_hamming_topk_capacity(nq, n):
        crowded = int(_crowded(Ir, nq, n).sum())
        if n >= 70000:                                              # the two large random cases: fixed by their seeds
            assert crowded == 0
        if crowded == 0:
            assert idx.last_fallback_queries == 0
        assert idx.last_fallback_queries <= crowded
    else:
        assert idx.last_fallback_queries == nq


def test_wide_massive_ties(cuda):
    """Six distinct 2048-bit codes over 50 000 rows: thousands of rows tie at every distance, most queries go to the
    exhaustive kernels (here at 64 words per row); ids must come out ascending inside every tie."""
    from sessionsimilaritysearch_amd.index import BinaryFlatIndex
    rng = np.random.default_rng(162)
    protos = rng.integers(0, 256, (6, 256), dtype=np.uint8)
    codes = protos[rng.integers(0, 6, 50000)]
    q = protos[:4]
    idx = BinaryFlatIndex(2048, cuda)
    idx.add(codes)
    D, I = idx.search(q, 100)
    Dr, Ir = sr.hamming_search(q, codes, 100)
    assert np.array_equal(D, Dr) and np.array_equal(I, Ir)
    assert idx.last_fallback_queries > 0


@pytest.mark.parametrize("seed", [0, 1])
def test_two_distinct_bits_padded_from_1032(cuda, seed):
    """1032-bit codes (129 bytes, stored in 256) that differ in two bits only, one in byte 0 and one in byte 128 -- the
    byte past the 1024-bit boundary: four distinct codes, distances 0 / 1 / 2, more ties than a list holds."""
    from sessionsimilaritysearch_amd.index import BinaryFlatIndex
    rng = np.random.default_rng(163 + seed)
    n, nq = 5000, 40
    codes = np.tile(rng.integers(0, 256, (1, 129), dtype=np.uint8), (n + nq, 1))
    codes[:, 0] = (codes[:, 0] & 0x7F) | (rng.integers(0, 2, n + nq, dtype=np.uint8) << 7)
    codes[:, 128] = (codes[:, 128] & 0xFE) | rng.integers(0, 2, n + nq, dtype=np.uint8)
    idx = BinaryFlatIndex(1032, cuda)
    assert idx._w == 256
    idx.add(codes[nq:])
    D, I = idx.search(codes[:nq], 10)
    Dr, Ir = sr.hamming_search(codes[:nq], codes[nq:], 10)
    assert np.array_equal(I, Ir) and np.array_equal(D, Dr)
    assert set(np.unique(D)) <= {0, 1, 2}


def test_sign_code_of_the_1600_wide_vector_end_to_end(cuda):
    """float32 [n, 1600] -> pack_sign_bits (device) -> BinaryFlatIndex(1600) -> search(k = 100) equals the oracle on the
    oracle's own packing of the same matrix; every query's noisy-copy source row comes first."""
    from sessionsimilaritysearch_amd.index import BinaryFlatIndex, pack_sign_bits
    rng = np.random.default_rng(164)
    n, nq, c = 20000, 200, 1600
    base = np.sign(rng.standard_normal((n, c), dtype=np.float32))
    base[base == 0] = 1.0
    src = rng.choice(n, nq, replace=False)
    qe = base[src].copy()
    qe[rng.random(qe.shape) < 0.2] *= -1
    packed, qpacked = pack_sign_bits(base), pack_sign_bits(qe)
    assert tuple(packed.shape) == (n, 200)
    codes, qcodes = sr.pack_sign_bits(base), sr.pack_sign_bits(qe)
    assert np.array_equal(packed.cpu().numpy(), codes) and np.array_equal(qpacked.cpu().numpy(), qcodes)
    idx = BinaryFlatIndex(c, cuda)
    idx.add(packed)
    D, I = idx.search(qpacked, 100)                                 # tensors in, tensors out
    assert D.is_cuda and I.is_cuda
    Dr, Ir = _oracle(qcodes, codes, 100)
    assert np.array_equal(D.cpu().numpy(), Dr) and np.array_equal(I.cpu().numpy(), Ir)
    assert np.array_equal(I[:, 0].cpu().numpy(), src)               # rank 0 = the row the query was copied from
    assert idx.last_fallback_queries <= int(_crowded(Ir, nq, n).sum())


def test_id_offset_and_workspace_reuse(cuda):
    from sessionsimilaritysearch_amd.index import BinaryFlatIndex
    codes, qcodes, _ = _random_case(165, 33, 9000, 2048)
    idx = BinaryFlatIndex(2048, cuda)
    idx.add(codes)
    idx.id_offset = OFF
    D, I = idx.search(qcodes, 50)
    Dr, Ir = sr.hamming_search(qcodes, codes, 50, OFF)
    assert np.array_equal(D, Dr) and np.array_equal(I, Ir) and int(I.min()) >= OFF
    D2, I2 = idx.search(qcodes, 50)                                 # the same index object, its workspace reused
    assert np.array_equal(D2, D) and np.array_equal(I2, I)
    idx.id_offset = 0
    D3, I3 = idx.search(qcodes[:7], 5)                              # a smaller search in the larger workspace
    Dr3, Ir3 = sr.hamming_search(qcodes[:7], codes, 5)
    assert np.array_equal(D3, Dr3) and np.array_equal(I3, Ir3)


# ---- straight through the C ABI, every buffer exactly sized between guard bands
class Buf:
    """`shape` x `dtype` on the device, exactly that many bytes, 256-byte aligned, between two GUARD-byte bands of
    random bytes (kept in `pat`)."""

    def __init__(self, shape, dtype, seed):
        self.shape = tuple(int(s) for s in shape) if isinstance(shape, (tuple, list)) else (int(shape),)
        self.dtype = dtype
        self.nbytes = int(np.prod(self.shape, dtype=np.int64)) * torch.empty((), dtype=dtype).element_size()
        raw = torch.empty(2 * GUARD + self.nbytes + 256, dtype=torch.uint8, device="cuda")
        self.off = GUARD + (-(raw.data_ptr() + GUARD)) % 256
        g = torch.Generator().manual_seed(seed)
        self.pat = torch.randint(0, 256, (raw.numel(),), dtype=torch.uint8, generator=g).to("cuda")
        raw.copy_(self.pat)
        self.raw = raw

    @property
    def ptr(self):
        return self.raw.data_ptr() + self.off

    @property
    def bytes(self):
        return self.raw[self.off:self.off + self.nbytes]

    @property
    def t(self):
        return self.bytes.view(self.dtype).view(self.shape)

    def guards_ok(self):
        e = self.off + self.nbytes
        return torch.equal(self.raw[:self.off], self.pat[:self.off]) and torch.equal(self.raw[e:], self.pat[e:])


def _dev_buf(x, seed):
    x = torch.as_tensor(x)
    b = Buf(x.shape, x.dtype, seed)
    b.t.copy_(x)
    return b


@pytest.mark.parametrize("nbytes", [128, 256])
def test_c_abi_fused_with_guarded_buffers(cuda, nbytes):
    """sss_hamming_topk at the new widths: the rows after the n-th equal the query codes (a read past n would win), the
    outputs are poisoned twice; proven queries equal the oracle, no write leaves its buffer."""
    rng = np.random.default_rng(166 + nbytes)
    nq, n, k = 50, 20011, 100                                       # a ragged last tile: 20011 = 78 * 256 + 43
    codes = rng.integers(0, 256, (n + 64, nbytes), dtype=np.uint8)
    q = rng.integers(0, 256, (nq + 4, nbytes), dtype=np.uint8)
    codes[n:] = np.resize(q[:nq], (64, nbytes))
    codes[7:400:3] = codes[7]                                       # duplicated rows: ties broken by id
    q[5] = codes[7]
    cb, qb = _dev_buf(codes, 1), _dev_buf(q, 2)
    Dr, Ir = sr.hamming_search(q[:nq], codes[:n], k, OFF)
    assert k <= L().sss_hamming_topk_capacity(nq, n)
    D, I, status = Buf((nq, k), torch.int32, 3), Buf((nq, k), torch.int64, 4), Buf(nq, torch.int32, 5)
    ws = Buf(int(L().sss_hamming_topk_workspace_bytes(nq, n)), torch.uint8, 6)
    for poison in (0xFF, 0x5A):
        for b in (D, I, status, ws):
            b.bytes.fill_(poison)
        rc = L().sss_hamming_topk(qb.ptr, nq, cb.ptr, n, nbytes, k, OFF, D.ptr, I.ptr, status.ptr, ws.ptr, ws.nbytes, _st())
        assert rc == 0, L().sss_last_error()
        torch.cuda.synchronize()
        assert all(b.guards_ok() for b in (D, I, status, ws, cb, qb))
        st = status.t.cpu().numpy()
        assert set(np.unique(st)) <= {0, 1}
        ok = st == 0
        crowded = _crowded(Ir - OFF, nq, n)
        assert crowded[5] and crowded.sum() <= 2 and ok[~crowded].all()     # only the query inside the duplicates may go unproven
        assert np.array_equal(I.t.cpu().numpy()[ok], Ir[ok]) and np.array_equal(D.t.cpu().numpy()[ok], Dr[ok])
        assert (I.t.cpu().numpy() < OFF + n).all()


@pytest.mark.parametrize("nbytes", [128, 256])
def test_c_abi_exhaustive_with_guarded_buffers(cuda, nbytes):
    """sss_hamming_topk_exhaustive at the new widths on a qsel subset, also with k > n: the selected rows of D and I equal
    the oracle, the other rows keep their poison, no write leaves its buffer."""
    rng = np.random.default_rng(168 + nbytes)
    nq = 50
    for n, k in ((300, 400), (5003, 33)):
        codes = rng.integers(0, 256, (n + 64, nbytes), dtype=np.uint8)
        q = rng.integers(0, 256, (nq + 4, nbytes), dtype=np.uint8)
        codes[n:] = np.resize(q[:nq], (64, nbytes))
        codes[7:200:3] = codes[7]
        q[5] = codes[7]
        cb, qb = _dev_buf(codes, 11), _dev_buf(q, 12)
        Dr, Ir = sr.hamming_search(q[:nq], codes[:n], k, OFF)
        sel = np.r_[5, 0, 3:nq:4].astype(np.int32)
        rest = np.setdiff1d(np.arange(nq), sel)
        qsel = _dev_buf(sel, 13)
        D, I = Buf((nq, k), torch.int32, 14), Buf((nq, k), torch.int64, 15)
        ws = Buf(int(L().sss_hamming_topk_exhaustive_workspace_bytes(len(sel), n)), torch.uint8, 16)
        for poison in (0xFF, 0x5A):
            for b in (D, I, ws):
                b.bytes.fill_(poison)
            rc = L().sss_hamming_topk_exhaustive(qb.ptr, qsel.ptr, len(sel), cb.ptr, n, nbytes, k, OFF, D.ptr, I.ptr, ws.ptr,
                                                 ws.nbytes, _st())
            assert rc == 0, L().sss_last_error()
            torch.cuda.synchronize()
            assert all(b.guards_ok() for b in (D, I, ws, cb, qb, qsel))
            assert np.array_equal(I.t.cpu().numpy()[sel], Ir[sel]) and np.array_equal(D.t.cpu().numpy()[sel], Dr[sel])
            assert bool((D.t[torch.as_tensor(rest, device="cuda")].view(torch.uint8) == poison).all())
            assert bool((I.t[torch.as_tensor(rest, device="cuda")].view(torch.uint8) == poison).all())
