"""Binary codes of 1024 and 2048 bits (stored rows of 128 / 256 bytes) without a device: both Hamming entry points let
the new widths through their host-side argument checks exactly where they let 64 bytes through, every other width is
still turned away, the workspace / capacity functions (which take no width) report what they always reported, and
``BinaryFlatIndex`` maps a code length to its stored row width."""
import os

import pytest

P = 1 << 20                     # a 256-byte aligned stand-in for device pointers: never dereferenced


@pytest.fixture(scope="module")
def L():
    import sessionsimilaritysearch_amd as pkg
    return pkg.lib()


def _guards(L):
    """name -> call(nbytes): arguments that are valid but for a workspace one byte class too small -- a call that passes
    every argument check returns -2 and never launches."""
    def topk(nbytes):
        return L.sss_hamming_topk(P, 4, P, 1000, nbytes, 10, 0, P, P, P, P, 256, 0)

    def exhaustive(nbytes):
        return L.sss_hamming_topk_exhaustive(P, P, 4, P, 1000, nbytes, 10, 0, P, P, P, 256, 0)

    return {"sss_hamming_topk": topk, "sss_hamming_topk_exhaustive": exhaustive}


@pytest.mark.parametrize("entry", ["sss_hamming_topk", "sss_hamming_topk_exhaustive"])
def test_wide_rows_pass_the_argument_checks_where_64_bytes_do(L, entry):
    call = _guards(L)[entry]
    assert L.sss_hamming_topk_workspace_bytes(4, 1000) > 256 and L.sss_hamming_topk_exhaustive_workspace_bytes(4, 1000) > 256
    for nbytes in (16, 32, 64):
        assert call(nbytes) == -2, (nbytes, L.sss_last_error())     # valid but for the workspace
    for nbytes in (128, 256):
        assert call(nbytes) == -2, (nbytes, L.sss_last_error())     # 1024 / 2048 bits: the same
    for nbytes in (0, 8, 48, 512, 200, 208, 129, -128):
        assert call(nbytes) == -1, (entry, nbytes)
        msg = L.sss_last_error().decode()
        assert "16, 32, 64, 128 or 256" in msg, msg                 # the message names the accepted set


# (nq, n, workspace bytes, capacity) as the build before the wide rows reported them: neither function takes a width
PINNED = [(1, 1, 384, 16), (1, 256, 384, 16), (1, 257, 512, 32), (5, 40, 896, 16), (17, 3000, 26368, 192),
          (64, 5000, 164096, 320), (256, 16384, 2097408, 1024), (257, 70000, 2105600, 1024), (300, 20000, 2457856, 1024),
          (1024, 200000, 8388864, 1024), (1024, 1000000, 8388864, 1024), (4096, 1000000, 33554688, 1024),
          (5000, 100000, 32640256, 816), (70000, 1000000, 26880256, 48), (300000, 5000, 38400256, 16)]


def test_workspace_and_capacity_are_what_they_were(L):
    for nq, n, ws, cap in PINNED:
        assert L.sss_hamming_topk_workspace_bytes(nq, n) == ws, (nq, n)
        assert L.sss_hamming_topk_capacity(nq, n) == cap, (nq, n)
        assert ws == nq * cap * 8 + 256                             # 16 keys of 8 bytes per (query, split)
    assert L.sss_hamming_topk_capacity(0, 100) == 0 and L.sss_hamming_topk_capacity(100, 0) == 0


def test_stored_width_policy():
    from sessionsimilaritysearch_amd import index as ix
    assert ix.BinaryFlatIndex.WIDTHS == (16, 32, 64, 128, 256)
    want = {8: 16, 128: 16, 136: 32, 250 + 6: 32, 256: 32, 512: 64, 520: 128, 1024: 128, 1032: 256, 1600: 256, 2040: 256, 2048: 256}
    for nbits, w in want.items():
        assert ix.BinaryFlatIndex.stored_bytes(nbits) == w, nbits
    for nbits in (2056, 4096):
        with pytest.raises(ValueError, match="longer than 2048 bits"):
            ix.BinaryFlatIndex.stored_bytes(nbits)
    for nbits in (250, 1601, 2047):
        with pytest.raises(ValueError, match="multiple of 8"):
            ix.BinaryFlatIndex.stored_bytes(nbits)


def test_index_construction_without_a_device():
    """The constructor validates nbits before it asks for a device; a subclass that skips the device sees the policy."""
    import torch
    from sessionsimilaritysearch_amd import index as ix

    class Stub(ix.BinaryFlatIndex):
        def __init__(self, nbits):                                  # the constructor's policy lines, no device
            self._w = self.stored_bytes(nbits)
            self.d, self.code_bytes, self.device = int(nbits), nbits // 8, torch.device("cpu")

    for nbits, w in ((8, 16), (256, 32), (512, 64), (520, 128), (1024, 128), (1600, 256), (2040, 256), (2048, 256)):
        s = Stub(nbits)
        assert (s._w, s.code_bytes, s.d) == (w, nbits // 8, nbits)
        rows = s._rows(torch.full((3, nbits // 8), 0xA5, dtype=torch.uint8).numpy())        # zero padded to the stored width
        assert tuple(rows.shape) == (3, w) and bool((rows[:, :nbits // 8] == 0xA5).all()) and not bool(rows[:, nbits // 8:].any())
        with pytest.raises(ValueError):
            s._rows(torch.zeros((3, nbits // 8 + 1), dtype=torch.uint8))
    for nbits in (2056, 4096):                                      # before any device is touched
        with pytest.raises(ValueError, match="longer than 2048 bits"):
            ix.BinaryFlatIndex(nbits)
    with pytest.raises(ValueError, match="multiple of 8"):
        ix.BinaryFlatIndex(1601)


def test_header_names_the_wide_rows():
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "sss.h")).read()
    sec = hdr[hdr.index("binary-code (Hamming) index"):hdr.index("neighbour-weighted item vote")]
    assert "{16, 32, 64, 128, 256}" in sec and "2048 bits" in sec
    assert "{16, 32, 64}" not in hdr
