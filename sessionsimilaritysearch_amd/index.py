"""faiss-shaped flat index on one MI355X + the reference's ``build_index`` / ``normalize``.

Drop-in surface (same names, argument meaning and error behaviour as the reference):

* ``normalize(vec)``                  <- ``util_amazon_filtered.py:28-31``
* ``build_index(emb, metric)``        <- ``test_amazon_filterd.py:207-223`` ('cos' | 'l2' | 'ip',
                                         anything else raises ``RuntimeError("Unregnozed metric", metric)``)
* ``FlatIndex(d).add(x)`` / ``.search(x, k) -> (D, I)`` / ``.ntotal`` / ``.d``
                                      <- ``faiss.IndexFlatIP`` / ``IndexFlatL2`` as used at
                                         ``test_amazon_filterd.py:212-220,578``

All arithmetic runs in the HIP kernels of ``libsss.so``; torch only owns device memory and the
stream.  There is no CPU fallback.
"""
from __future__ import annotations

import dataclasses
from typing import Callable

import numpy as np
import torch

from . import _lib
from .routing import (AUTO_DECAY_SEARCHES, AUTO_ESCALATE, AUTO_F16_MAX_K, AUTO_SPLIT_MAX_K, F16_SCAN_DIMS, F32_SCAN_DIMS,  # noqa: F401
                      FUSED_MAX_K, L2_SCAN_MAX_NORM, L2_SCAN_MIN_NORM, LONG_MAX_K, LONG_MAX_ROW_BYTES, PAD_SCAN_MAX_D, _LADDER,
                      ScanRouting)
from ._device import EXHAUSTIVE_WS_BYTES as _EXHAUSTIVE_WS_BYTES, Workspace, exhaustive_chunk, grow_rows


@dataclasses.dataclass(frozen=True)
class _Format:
    """One storage format of a FlatIndex (csrc/elem.h holds the kernels' side of the same table)."""
    name: str
    code: int                       # include/sss.h: dtype
    torch_dtype: torch.dtype
    numpy_dtype: type | None        # numpy arrays of this type are stored as they are (None: numpy has no such type)
    elem_bytes: int
    fused_dims: tuple               # d of the fused scans: rows of 256 / 512 / 1024 bytes
    long_rows: bool                 # has a long-row scan (sss_ip_topk_long)
    from_f32: Callable              # (float32 device tensor, what) -> tensor of the stored type; ValueError for what it cannot hold
    checks_finite: bool = False     # add / adopt refuse rows that are not finite in the stored type

    @property
    def align(self) -> int:
        """Elements per 16-byte piece of a stored row: d % this == 0."""
        return 16 // self.elem_bytes


_FORMATS = {f.name: f for f in (
    _Format("f32", 0, torch.float32, np.float32, 4, F32_SCAN_DIMS, True, lambda x, what: x),
    _Format("bf16", 1, torch.bfloat16, None, 2, (128, 256, 512), True, lambda x, what: to_bf16(x)),
    _Format("f16", 4, torch.float16, np.float16, 2, (128, 256, 512), True, lambda x, what: to_f16(x), checks_finite=True),
    _Format("i8", 6, torch.int8, np.int8, 1, (256, 512, 1024), False, lambda x, what: _i8_from_f32(x, what)),
)}
FUSED_DIMS = {f.name: f.fused_dims for f in _FORMATS.values()}
_CODE = {f.name: f.code for f in _FORMATS.values()}              # include/sss.h: dtype (2, 3 are scan images, below; 5 is unassigned)
_TORCH_DTYPE = {f.name: f.torch_dtype for f in _FORMATS.values()}
DTYPE_CODE = {n: c for n, c in _CODE.items() if _TORCH_DTYPE[n].is_floating_point}    # the public views: float formats ...
INT_DTYPE_CODE = {n: c for n, c in _CODE.items() if n not in DTYPE_CODE}               # ... and integer ones
SEARCH_CHUNK = 65536             # queries per fused call of search_device (workspace 16 KB per query)
SEARCH_CHUNK_LONG = 16384        # ... on the long-row path (64 KB per query)
RANGE_CHUNK = 4096               # queries per fused range_search count / fill (workspace 64 KB per query)
_SCAN_CODE = {"split": 2, "f16": 3}                              # include/sss.h: scan image codes (else the dtype's own)


# Scan family (FlatIndex._family; "ip": by scan, else by the index's own rows) -> the entry point that serves it.  What a
# family takes -- a row bias, a state buffer, an unproven count -- is read from its declaration (_lib.PARAMS); its workspace
# is sized by <name>_workspace_bytes, with one exception.
_TOPK = {                                # search_fused
    "pad": "sss_pad_topk", "l2": "sss_l2_topk", "ip_f16": "sss_ip_topk_f16", "ip_split": "sss_ip_topk_split", "ip": "sss_ip_topk",
    "long_ip": "sss_ip_topk_long", "long_l2": "sss_l2_topk_long",
}
_THRESHOLD = {"pad": "sss_pad_topk_threshold", "l2": "sss_l2_topk_threshold", "ip": "sss_ip_topk_threshold"}   # search_threshold; long rows have no rung
_WORKSPACE_BYTES = {"sss_ip_topk_split": "sss_ip_topk_workspace_bytes"}      # the split scan's workspace is the f32 scan's (dtype 0)


def _dev(device=None):
    if not torch.cuda.is_available():
        raise _lib.SssError("no HIP device available: the session-similarity path runs on MI355X only")
    if device is None:
        return torch.device("cuda", torch.cuda.current_device())
    device = torch.device(device) if not isinstance(device, int) else torch.device("cuda", device)
    if device.type != "cuda":
        raise _lib.SssError(f"device must be a HIP device, got {device}")
    return torch.device("cuda", device.index if device.index is not None else torch.cuda.current_device())


def _as_device_f32(x, device):
    if isinstance(x, np.ndarray):
        x = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32))
    if not isinstance(x, torch.Tensor):
        raise TypeError("expected a numpy array or torch tensor")
    return x.to(device=device, dtype=torch.float32).contiguous()


def to_bf16(x: torch.Tensor) -> torch.Tensor:
    """float32 CUDA tensor -> bfloat16 (round to nearest even) through ``sss_f32_to_bf16``."""
    _lib.require_cuda(x, "x", torch.float32)
    if x.numel() % 8:
        raise _lib.SssError("to_bf16: element count must be a multiple of 8")
    y = torch.empty(x.shape, dtype=torch.bfloat16, device=x.device)
    rc = _lib.lib().sss_f32_to_bf16(x.data_ptr(), x.numel(), y.data_ptr(), _lib.stream_ptr(x.device))
    _lib.check(rc, "sss_f32_to_bf16")
    return y


def to_f16(x: torch.Tensor) -> torch.Tensor:
    """float32 CUDA tensor -> IEEE float16 (round to nearest even): what an f16 index stores.  Values beyond
    +-65504 become inf; ``FlatIndex.add`` refuses such rows."""
    _lib.require_cuda(x, "x", torch.float32)
    return x.to(torch.float16)


def integer_valued_i8(x: torch.Tensor) -> torch.Tensor:
    """Is every element of the float tensor ``x`` an integer in [-128, 127]?  A bool scalar tensor on x's device (no
    sync; NaN and inf are not).  What an int8 index asks of float input before it casts it."""
    return ((x == torch.round(x)) & (x >= -128.0) & (x <= 127.0)).all()


def _i8_from_f32(x: torch.Tensor, what: str) -> torch.Tensor:
    # one device reduction, one host read -- as the f16 index's "not finite" check
    if not bool(integer_valued_i8(x).item()):
        raise ValueError(f"{what}: an i8 index takes int8 rows, or floats that are integers in [-128, 127] "
                         "(quantize_i8 makes them)")
    return x.to(torch.int8)


def quantize_i8(x, scale=None):
    """Symmetric int8 quantisation for an ``dtype="i8"`` index: ``codes = clip(rint(x * scale), -127, 127)`` as int8
    (round half to even; -128 is never produced), ``scale`` defaulting to ``127 / max|x|`` (1.0 for an all-zero input).
    numpy in -> numpy codes, tensor in -> tensor codes (on its device); returns ``(codes, scale)``.  Scores of the
    codes are ``scale_q * scale_c`` times those of the vectors, up to the rounding."""
    is_np = isinstance(x, np.ndarray)
    t = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)) if is_np else x.to(torch.float32)
    if scale is None:
        amax = float(t.abs().max().item()) if t.numel() else 0.0
        scale = 127.0 / amax if amax > 0.0 else 1.0
    scale = float(scale)
    codes = torch.clamp(torch.round(t * scale), -127.0, 127.0).to(torch.int8)
    return (codes.numpy() if is_np else codes), scale


def normalize_(x: torch.Tensor, eps: float = 1e-6, rule: int = 0) -> torch.Tensor:
    """In-place row normalisation of a CUDA float32 [n, d] tensor (rows may be strided)."""
    if x.dim() != 2 or x.stride(1) != 1 or x.dtype != torch.float32 or not x.is_cuda:
        raise _lib.SssError("normalize_: need a CUDA float32 [n, d] tensor with unit inner stride")
    rc = _lib.lib().sss_normalize_rows(x.data_ptr(), x.shape[0], x.shape[1], x.stride(0), eps, rule,
                                       _lib.stream_ptr(x.device))
    _lib.check(rc, "sss_normalize_rows")
    return x


def normalize(vec, eps: float = 1e-6, rule: int = 0):
    """Reference ``normalize``: ``v / sqrt(clip(sum(v**2), 1e-6))`` row-wise (1-D input: the
    whole vector).  numpy in -> numpy out; CUDA tensor in -> new CUDA tensor out.
    ``rule=1, eps=1e-4`` gives the fine-tune scripts' ``v / (||v|| + 1e-4)``."""
    is_np = isinstance(vec, np.ndarray)
    dev = _dev() if is_np or not vec.is_cuda else vec.device
    one_d = vec.ndim == 1
    x = _as_device_f32(vec, dev)
    if x.data_ptr() == (vec.data_ptr() if isinstance(vec, torch.Tensor) else 0):
        x = x.clone()
    if one_d:
        x = x.view(1, -1)
    d = x.shape[1]
    if d % 4:                       # kernel moves 16 bytes per lane: pad the row, cut it back
        pad = torch.zeros(x.shape[0], (d + 3) // 4 * 4, device=dev, dtype=torch.float32)
        pad[:, :d] = x
        x = normalize_(pad, eps, rule)[:, :d].contiguous()
    else:
        normalize_(x, eps, rule)
    if one_d:
        x = x.view(-1)
    return x.cpu().numpy() if is_np else x


class FlatIndex(ScanRouting):
    """Exact flat index (faiss ``IndexFlatIP`` / ``IndexFlatL2`` semantics) with
    the canonical result contract of DESIGN.md: scores are float64-accumulated dot products
    rounded to float32, ordered by (score desc, id asc); missing results are (-FLT_MAX, -1).

    ``dtype="bf16"`` (BASELINE config C5) stores the corpus -- and rounds every query -- to
    bfloat16 and scores on the bf16 MFMA; the contract is then defined on the ROUNDED vectors
    (float64 dot of the stored bf16 values).

    ``dtype="f16"`` stores the corpus -- and rounds every query -- to IEEE float16 (11 significant bits against
    bfloat16's 8, the same 2 bytes per element; the format of faiss ``useFloat16`` and of a half-precision
    encoder's output) and scores on the f16 MFMA, with the same contract on the rounded vectors.  Float16 ends at
    65504: ``add`` raises ``ValueError`` for rows that do not stay finite, and stores nothing.

    ``dtype="i8"`` stores the corpus as int8, one byte per element (faiss ``QT_8bit_direct``, any int8 embedding
    export; ``quantize_i8`` makes such codes), with d % 16 == 0.  Queries are int8 as well.  ``add`` / ``search`` /
    ``adopt`` take ``np.int8`` arrays and ``torch.int8`` tensors as they are; float input is accepted only if every
    value is an integer in [-128, 127] -- anything else raises ``ValueError`` and ``add`` stores nothing.  The
    contract is the same float64 dot (or sum of squared differences) of the stored values: every partial sum is an
    integer, and the i8 MFMA scan (d = 256 / 512 / 1024, k <= 500) computes it exactly in int32, so a query stays
    unproven only on an exact tie at rank k.  Every other d, larger k and the L2 metric run on the exhaustive
    kernels; there is no long-row scan for int8 rows (d = 1600 is served exhaustively).

    ``scan`` picks how a float32 index finds its candidates (the results are the same, they are
    re-scored from the float32 rows and proven per query either way; what differs is speed and how
    many near-tied queries are left to the exhaustive fallback):
    ``"f16"`` keeps a float16 image of the corpus scaled by one power of two (half the bytes) and
    scans it with ONE f16 MFMA pass -- score error ~4e-4 |q||c| at d = 128 (d in 128/256/512);
    ``"split"`` keeps each element as a bfloat16 hi/lo pair (same bytes as the f32 row) and scans
    with three bf16 MFMA passes -- error <= ~2^-14 |q||c|;
    ``"f32"`` scans the float32 rows on the f32 MFMA (error ~ d 2^-24) and needs no second image;
    ``"auto"`` (default) takes "f16" for k <= 128 where the shape allows and "split" up to k = 500; "f32" is reached
    by escalation only, after searches that left too many queries unproven (``ScanRouting._note_fallbacks``).
    Images are built on first use (``prepare(k)`` does it ahead of time) and extended as rows are added.

    ``metric="l2"`` (faiss ``IndexFlatL2``): squared distances, the float64 chain of ``(q_k - c_k)**2`` rounded to
    float32, ordered by (distance asc, id asc), missing results (+FLT_MAX, -1).  A float32 index runs it on the same
    scans, same ``scan`` argument and ladder (``l2_scan_for``): the rows nearest to q are those with the largest
    ``q.c - |c|**2 / 2``, which is the inner-product scan with every score started from a per-row bias (one float32
    per row, kept beside the images).  Other dtypes, d without a scan, k > 500 and corpora whose largest row norm lies
    outside [2^-60, 2^60] run on the exhaustive kernels.

    Queries a scan leaves unproven are resolved in two further stages, both exact: the THRESHOLD RUNG
    (``search_threshold``: one more matrix-core scan for just those queries that keeps every row able to
    reach the k-th score already known, near ties and duplicate rows alike) and, for what exceeds its
    capacity, the exhaustive kernels (``search_exhaustive``).

    ``pad_scan=True`` (off by default) gives a float32 index of ANY width ``4 <= d <= 512`` with ``d % 4 == 0`` the same
    scans -- d = 200, the reference's default embedding width, among them; without it such an index runs on the exhaustive
    kernels.  The scan images and the query batch are built at ``scan_width(scan)``, the next width the scan has, with
    exact zero columns behind column d: they add nothing to a dot product or to ``|c|**2``, so scan, bound (taken at the
    scan width) and proof are those of the wider corpus, and candidates are re-scored from the d-wide rows.  Results are
    the same as without the switch.  It has no effect where d already has a scan (64 / 128 / 256 / 512, ``d % 64 == 0``
    long rows) and on other dtypes.  An image costs ``scan_width`` elements a row: d = 200 on the f16 scan keeps 512 bytes
    a row beside the 800-byte row."""

    def __init__(self, d: int, metric: str = "ip", device=None, dtype: str = "f32", scan: str | None = None, *,
                 pad_scan: bool = False):
        if dtype not in _FORMATS:
            names = [repr(n) for n in _FORMATS]
            raise ValueError(f"dtype must be {', '.join(names[:-1])} or {names[-1]}")
        fmt = _FORMATS[dtype]
        if dtype != "f32" and d % fmt.align:
            raise ValueError(f"{dtype} index needs d % {fmt.align} == 0")
        ScanRouting.__init__(self, d, metric, dtype, scan, pad_scan, fmt=fmt)
        self._tdtype = fmt.torch_dtype
        self.device = _dev(device)
        self._c_shift = 0               # the float16 image holds rows * 2^_c_shift
        self._resid = None
        self._reset_images()
        self._xb = torch.empty((0, self.d), dtype=self._tdtype, device=self.device)
        self._store = self._xb          # backing storage of _xb (grown geometrically by add())
        self._cmax_t = torch.zeros(1, dtype=torch.float32, device=self.device)
        self._cmax = None
        self._ws = Workspace(self.device)
        self._state = None              # per-query state words of sss_ip_topk: zeroed once, kept zero by the kernels
        self.id_offset = 0              # global id of row 0 (row-sharded corpora)
        self.last_fallback_queries = 0  # queries of the last search() re-run exhaustively
        self.last_rescan_queries = 0    # queries of the last search() the fused scan left unproven (threshold rung first)
        self.last_range_scan = None     # the scan the last range_search used ("" = exhaustive route only)
        self.last_range_overflow_queries = 0    # queries of the last range_search the fused route sent to the exhaustive one

    def _reset_images(self):
        """No derived corpus image yet: each is built on first use and extended as rows are added."""
        self._split, self._split_done = None, 0         # [cap, 2 w] bf16 hi|lo image of the rows ("split" scan; w = scan_width)
        self._f16, self._f16_done = None, 0             # [cap, w] float16 image of rows * 2^_c_shift ("f16" scan)
        self._p32, self._p32_done = None, 0             # [cap, w] float32 rows, zero-extended ("f32" scan of a padded index)
        self._bias, self._bias_done = None, 0           # [cap] float32 -|row|^2 / 2: what the L2 scans start every score from
        self._amax_t = torch.zeros(1, dtype=torch.float32, device=self.device)    # largest |element| in the f16 image
        self._resid_t = torch.zeros(1, dtype=torch.float32, device=self.device)   # largest row residual norm of it

    _fmt = property(lambda self: _FORMATS[self.dtype], doc="The record of this index's storage format (``dtype`` names it).")

    @property
    def ntotal(self) -> int:
        return int(self._xb.shape[0])

    def add(self, x):
        """Append rows (copied, ids = insertion order) -- ``IndexFlatIP.add``."""
        x = self._rows(x, "add")
        self._take_norm_max(x)
        self._store, self._xb = grow_rows(self._store, self._xb, x)
        # streaming adds keep what the searches have learned about this corpus; only once it has doubled since
        # an escalation was earned is that treated as a different corpus (adopt() always resets)
        if self._auto_level and self.ntotal > 2 * max(1, self._auto_rows):
            self._auto_level.clear()
            self._auto_clean.clear()

    def _image_complete(self, scan: str) -> bool:
        image, done = (self._f16, self._f16_done) if scan == "f16" else (self._split, self._split_done)
        return image is not None and done == self.ntotal

    def _grow_image(self, img, done, tdtype, width=None):
        """A derived per-row array -- [cap, width], or [cap] without a width -- with room for every row of the store, its
        first `done` rows kept."""
        cap = max(self._store.shape[0], self.ntotal)
        if img is None or img.shape[0] < cap:
            new = torch.empty((cap,) if width is None else (cap, width), dtype=tdtype, device=self.device)
            if img is not None and done:
                new[:done] = img[:done]
            img = new
        return img

    def _ensure_f16(self):
        """Bring the scaled float16 image up to date.  Its shift is fixed by the largest |element|
        present when it was last rebuilt (which then lies in [2^12, 2^13)); rows that would push an
        element past 2^15 trigger a rebuild of the whole image with a new shift."""
        n, lo = self.ntotal, self._f16_done
        if lo == n and self._f16 is not None:
            return
        L, st = _lib.lib(), _lib.stream_ptr(self.device)
        _lib.check(L.sss_abs_max(self._xb[lo:].data_ptr(), (n - lo) * self.d, self._amax_t.data_ptr(), st), "sss_abs_max")
        amax = float(self._amax_t.item())
        ds = self.scan_width("f16") if self._pad else self.d
        self._f16 = self._grow_image(self._f16, lo, torch.float16, ds)
        if lo == 0 or not (amax * 2.0 ** self._c_shift < 32768.0):
            self._c_shift = int(L.sss_f16_shift(amax))
            self._resid_t.zero_()
            lo = 0
        if self._pad:                   # the same image, ds wide with zero columns behind column d (include/sss_pad.h)
            _lib.check(L.sss_pad_scale_f16(self._xb[lo:].data_ptr(), n - lo, self.d, ds, self._c_shift,
                                           self._f16[lo:].data_ptr(), st), "sss_pad_scale_f16")
            _lib.check(L.sss_pad_f16_resid_max(self._xb[lo:].data_ptr(), self._f16[lo:].data_ptr(), n - lo, self.d, ds,
                                               self._c_shift, self._resid_t.data_ptr(), st), "sss_pad_f16_resid_max")
        else:
            _lib.check(L.sss_scale_f16(self._xb[lo:].data_ptr(), (n - lo) * self.d, self._c_shift,
                                       self._f16[lo:].data_ptr(), st), "sss_scale_f16")
            _lib.check(L.sss_f16_resid_max(self._xb[lo:].data_ptr(), self._f16[lo:].data_ptr(), n - lo, self.d,
                                           self._c_shift, self._resid_t.data_ptr(), st), "sss_f16_resid_max")
        self._resid = None
        self._f16_done = n

    def corpus_resid_norm(self) -> float:
        if self._resid is None:
            self._resid = float(self._resid_t.item())
        return self._resid

    def _ensure_split(self):
        """Bring the bf16 hi|lo image up to date."""
        n, lo = self.ntotal, self._split_done
        if lo == n and self._split is not None:
            return
        L, st = _lib.lib(), _lib.stream_ptr(self.device)
        ds = self.scan_width("split")
        self._split = self._grow_image(self._split, lo, torch.bfloat16, 2 * ds)
        if self._pad:
            _lib.check(L.sss_pad_split_bf16(self._xb[lo:].data_ptr(), n - lo, self.d, ds, self._split[lo:].data_ptr(), st),
                       "sss_pad_split_bf16")
        else:
            _lib.check(L.sss_split_bf16(self._xb[lo:].data_ptr(), n - lo, self.d, self._split[lo:].data_ptr(), st), "sss_split_bf16")
        self._split_done = n

    def _ensure_p32(self):
        """Bring the zero-extended float32 rows up to date: what the "f32" scan of a ``pad_scan`` index reads."""
        n, lo = self.ntotal, self._p32_done
        if lo == n and self._p32 is not None:
            return
        ds = self.scan_width("f32")
        self._p32 = self._grow_image(self._p32, lo, torch.float32, ds)
        rc = _lib.lib().sss_pad_rows_f32(self._xb[lo:].data_ptr(), n - lo, self.d, ds, self._p32[lo:].data_ptr(),
                                         _lib.stream_ptr(self.device))
        _lib.check(rc, "sss_pad_rows_f32")
        self._p32_done = n

    def _padded_queries(self, q: torch.Tensor, ds: int) -> torch.Tensor:
        """The query batch zero-extended to ds columns: one launch (``sss_pad_rows_f32``)."""
        qp = torch.empty((q.shape[0], ds), dtype=torch.float32, device=self.device)
        rc = _lib.lib().sss_pad_rows_f32(q.data_ptr(), q.shape[0], self.d, ds, qp.data_ptr(), _lib.stream_ptr(self.device))
        _lib.check(rc, "sss_pad_rows_f32")
        return qp

    def _ensure_bias(self):
        """Bring the L2 row bias up to date (rows added since the last call)."""
        n, lo = self.ntotal, self._bias_done
        if lo == n and self._bias is not None:
            return
        self._bias = self._grow_image(self._bias, lo, torch.float32)
        rc = _lib.lib().sss_l2_row_bias(self._xb[lo:].data_ptr(), n - lo, self.d, self._bias[lo:].data_ptr(),
                                        _lib.stream_ptr(self.device))
        _lib.check(rc, "sss_l2_row_bias")
        self._bias_done = n

    def prepare(self, k: int = 10):
        """Build whatever a fused search for k results needs (images, norms, the L2 row bias) now rather than on
        the first search; returns the scan that will be used."""
        mode = self._route(k)
        self._source(mode)
        return mode

    def _source(self, mode: str):
        """``_scan_image(mode)``, with the largest row norm and an L2 index's row bias brought up to date as well."""
        source = self._scan_image(mode)
        self.corpus_max_norm()
        if mode and self.metric == "l2":
            self._ensure_bias()
        return source

    def _scan_image(self, mode: str):
        """(image, scan code, corpus_shift, corpus_resid_norm) of what scan `mode` reads, the image brought up to date:
        the scaled float16 image ("f16", and "long" for a float32 index), the bf16 hi|lo image ("split"), else the
        index's own rows."""
        if mode == "f16" or (mode == "long" and self.dtype == "f32"):
            self._ensure_f16()
            return self._f16, _SCAN_CODE["f16"], self._c_shift, self.corpus_resid_norm()
        if mode == "split":
            self._ensure_split()
            return self._split, _SCAN_CODE["split"], 0, 0.0
        if self._pad and mode == "f32":
            self._ensure_p32()
            return self._p32, self._fmt.code, 0, 0.0
        return self._xb, self._fmt.code, 0, 0.0

    def _require_d_aligned(self):
        """The exhaustive kernels read rows in 16-byte pieces."""
        if self.d % self._fmt.align:
            by_align = {}
            for f in _FORMATS.values():
                by_align.setdefault(f.align, []).append(f.name)
            raise _lib.SssError("d must be a multiple of " + " / ".join(f"{a} ({', '.join(n)})" for a, n in sorted(by_align.items())))

    def _exhaustive_chunks(self, rows: torch.Tensor, ws_bytes):
        """(offset, query rows, workspace) per chunk of the device int32 `rows` whose [chunk, n] scores fit the exhaustive
        workspace budget; ``ws_bytes(nsel, n)`` sizes a chunk's workspace."""
        n = self.ntotal
        per = exhaustive_chunk(n, 4)
        for lo in range(0, rows.numel(), per):
            sel = rows[lo:lo + per].contiguous()
            yield lo, sel, self._ws.get(ws_bytes(sel.numel(), n))

    def _rows(self, x, what):
        """Input rows as a contiguous device tensor of the index's element type."""
        fmt = self._fmt
        if self.dtype != "f32" and isinstance(x, torch.Tensor) and x.dtype == fmt.torch_dtype:
            x = x.to(self.device).contiguous()
        elif self.dtype != "f32" and isinstance(x, np.ndarray) and fmt.numpy_dtype is not None and x.dtype == fmt.numpy_dtype:
            x = torch.from_numpy(np.ascontiguousarray(x)).to(self.device)
        else:
            x = fmt.from_f32(_as_device_f32(x, self.device), what)
        if x.dim() != 2 or x.shape[1] != self.d:
            raise ValueError(f"{what}: expected [n, {self.d}], got {tuple(x.shape)}")
        return x

    def _take_norm_max(self, x, reset=False):
        """Merge the largest row norm of the new rows ``x`` into ``_cmax_t`` (``reset``: start from zero -- the rows
        replace the corpus): one ``sss_row_norm_max`` into a fresh device [1] tensor, no host sync.  A format that
        checks its rows are finite (f16: a float32 value beyond 65504 became inf in ``to_f16``) reads the result
        first -- the reduction gives +inf for a row holding an inf or a NaN, so it serves both at one host sync --
        and raises before the index has changed.  Rows the reduction does not take (f32, d % 4 != 0) are skipped."""
        new_max = None
        if x.shape[0] and self.d % self._fmt.align == 0:
            new_max = torch.zeros(1, dtype=torch.float32, device=self.device)
            rc = _lib.lib().sss_row_norm_max(x.data_ptr(), x.shape[0], self.d, self._fmt.code, new_max.data_ptr(),
                                             _lib.stream_ptr(self.device))
            _lib.check(rc, "sss_row_norm_max")
            if self._fmt.checks_finite and not np.isfinite(float(new_max.item())):
                raise ValueError("f16 index: rows hold values that are not finite in float16 (|x| > 65504, inf or NaN)")
        if reset:
            self._cmax_t.zero_()
        if new_max is not None:
            torch.maximum(self._cmax_t, new_max, out=self._cmax_t)
        self._cmax = None

    def adopt(self, xb: torch.Tensor, id_offset: int = 0):
        """Use an existing CUDA [n, d] tensor of the index's element type as the corpus without
        copying it."""
        _lib.require_cuda(xb, "xb", self._tdtype)
        if xb.dim() != 2 or xb.shape[1] != self.d:
            raise ValueError("adopt: wrong shape")
        self._take_norm_max(xb, reset=True)
        self._xb = self._store = xb
        self.id_offset = int(id_offset)
        self._reset_images()
        self._auto_level.clear()
        self._auto_clean.clear()
        return self

    def corpus_max_norm(self) -> float:
        if self._cmax is None:
            self._cmax = float(self._cmax_t.item())
        return self._cmax

    # ------------------------------------------------------------------ device-level search
    def search_fused(self, q: torch.Tensor, k: int, out=None, unproven_count=None):
        """Enqueue the fused MFMA scoring + top-k on the current stream; no host sync.
        Returns (D [nq,k] f32, I [nq,k] i64, status [nq] i32) CUDA tensors; rows with
        status != 0 must be re-run with ``search_exhaustive`` (``search`` does that).  An L2 index takes the
        L2 scan ``l2_scan_for(k)`` names, or the long-row scan where ``l2_long_for(k)`` says so.
        ``unproven_count``: optional CUDA int32 [1] tensor, incremented once per unproven query."""
        L = _lib.lib()
        _lib.require_cuda(q, "q", self._tdtype)
        nq, n = q.shape[0], self.ntotal
        if out is None:
            D = torch.empty((nq, k), dtype=torch.float32, device=self.device)
            I = torch.empty((nq, k), dtype=torch.int64, device=self.device)
            status = torch.empty((nq,), dtype=torch.int32, device=self.device)
        else:
            D, I, status = out
        mode = self.last_scan = self._route(k)
        source = self._source(mode)
        if mode == "":
            raise _lib.SssError("search_fused: this index / k has no fused path (use search)")
        family = self._family(mode)
        name = _TOPK.get(f"{family}_{mode}") or _TOPK[family]
        v = self._values(source, k, mode, nq=nq, D_out=D.data_ptr(), I_out=I.data_ptr(), status=status.data_ptr(),
                         unproven_count=0 if unproven_count is None else unproven_count.data_ptr())
        self._set_workspace(name, v)
        stateful = "state" in _lib.PARAMS[name]                 # the long-row entries keep no state and count no unproven queries
        if stateful:
            sbytes = L.sss_ip_topk_state_bytes(nq)
            if self._state is None or self._state.numel() < sbytes:
                self._state = torch.zeros(sbytes, dtype=torch.uint8, device=self.device)
            v["state"], v["state_bytes"] = self._state.data_ptr(), self._state.numel()
        self._set_queries(q, v)
        rc = _lib.call(name, v)
        if rc != 0 and stateful:
            self._state = None          # re-made (zeroed) on the next call
        _lib.check(rc, name)
        if unproven_count is not None and "unproven_count" not in _lib.PARAMS[name]:
            unproven_count += (status != 0).sum().to(torch.int32)
        return D, I, status

    def _family(self, mode: str) -> str:
        """The scan family of a fused call on scan `mode`: which entry of ``_TOPK`` / ``_THRESHOLD`` serves it."""
        if mode == "long":
            return "long_" + self.metric
        return "pad" if self._pad else self.metric

    def _values(self, source, k: int, mode: str, **call) -> dict:
        """The arguments of a scan family's entry point under the names the headers give its parameters; ``source`` is
        ``_scan_image(mode)``'s, an L2 index's row bias up to date, ``call`` what the one call adds (counts, outputs)."""
        image, code, shift, resid = source
        v = {"corpus": self._xb.data_ptr(), "dtype": self._fmt.code, "scan_image": image.data_ptr(), "scan_dtype": code,
             "corpus_shift": shift, "corpus_resid_norm": resid, "bias": self._bias.data_ptr() if self.metric == "l2" else None,
             "n": self.ntotal, "d": self.d, "k": k, "id_offset": self.id_offset, "corpus_max_norm": self.corpus_max_norm(),
             "stream": _lib.stream_ptr(self.device), **call}
        if self._pad:
            v["d_row"], v["d_scan"] = self.d, self.scan_width(mode)
        return v

    def _set_queries(self, q: torch.Tensor, v: dict):
        """``v["q"]``: the batch -- on a ``pad_scan`` index zero-extended to the scan's width: the scan reads the padded
        batch and the d_scan-wide image, the re-score the d-wide rows (include/sss_pad.h)."""
        if self._pad:
            q = v["padded q"] = self._padded_queries(q, v["d_scan"])       # (names no parameter: holds the batch for the call)
        v["q"] = q.data_ptr()

    def _set_workspace(self, name: str, v: dict):
        """``v``'s workspace: the index's buffer at the size ``name``'s workspace function asks for on the values ``v``."""
        ws = self._ws.get(_lib.call(_WORKSPACE_BYTES.get(name, name + "_workspace_bytes"), v))
        v["workspace"], v["workspace_bytes"] = ws.data_ptr(), ws.numel()

    def search_threshold(self, q: torch.Tensor, k: int, D: torch.Tensor, I: torch.Tensor, status: torch.Tensor, rows):
        """Threshold rung (``sss_ip_topk_threshold``) for the query rows ``rows`` a fused search left
        unproven: one more scan for just those queries keeps every corpus row that could still reach the
        k-th score already known (column k-1 of their rows of D) and re-scores them all.  Resolved rows of
        D / I are rewritten and their status set to 0; returns the rows still unproven."""
        mode = self._rung_route()
        if mode == "" or rows.numel() == 0 or k > 8192:
            return rows
        source = self._scan_image(mode)
        sel = rows.to(device=self.device, dtype=torch.int32).contiguous()
        if self.metric == "l2":
            self._ensure_bias()
        name = _THRESHOLD[self._family(mode)]
        v = self._values(source, k, mode, qsel=sel.data_ptr(), nsel=sel.numel(), D_out=D.data_ptr(), I_out=I.data_ptr(),
                         status=status.data_ptr())
        self._set_queries(q, v)
        self._set_workspace(name, v)
        _lib.check(_lib.call(name, v), name)
        return sel[status[sel.long()] != 0]

    def fix_unproven(self, q: torch.Tensor, k: int, D: torch.Tensor, I: torch.Tensor, status: torch.Tensor) -> int:
        """Make the result of a fused search exact for every query: unproven ones (status != 0) go through
        the threshold rung, what that leaves (more tied rows than its capacity) through the exhaustive
        kernels.  One host sync per stage that has work.  Returns the number of queries the fused scan
        had left unproven."""
        bad = torch.nonzero(status).flatten()
        nbad = int(bad.numel())
        self.last_rescan_queries, self.last_fallback_queries = nbad, 0
        if nbad:
            left = self.search_threshold(q, k, D, I, status, bad)
            if left.numel():
                self.last_fallback_queries = int(left.numel())
                self.search_exhaustive(q, k, D, I, left, bounded=True)
        self._note_fallbacks(k, q.shape[0], nbad)
        return nbad

    def search_exhaustive(self, q: torch.Tensor, k: int, D: torch.Tensor, I: torch.Tensor, rows=None, bounded=False):
        """Exhaustive exact path for query rows ``rows`` (all when None); writes into D / I.
        ``bounded``: D[rows, k-1] holds a valid lower bound of each query's k-th best score (what a
        fused search leaves behind for its unproven queries) -- lets the kernel skip the float64
        chain for rows that cannot matter."""
        L = _lib.lib()
        n = self.ntotal
        if rows is None:
            rows = torch.arange(q.shape[0], dtype=torch.int32, device=self.device)
        rows = rows.to(device=self.device, dtype=torch.int32).contiguous()
        metric = 0 if self.metric == "ip" else 1
        for _, sel, ws in self._exhaustive_chunks(rows, L.sss_ip_topk_exhaustive_workspace_bytes):
            if bounded and metric == 0:
                lb = D[sel.long(), k - 1].contiguous()
                rc = L.sss_ip_topk_exhaustive_lb(q.data_ptr(), sel.data_ptr(), sel.numel(), self._xb.data_ptr(), n,
                                                 self.d, k, self._fmt.code, self.id_offset, lb.data_ptr(),
                                                 D.data_ptr(), I.data_ptr(), ws.data_ptr(), ws.numel(),
                                                 _lib.stream_ptr(self.device))
            else:
                rc = L.sss_ip_topk_exhaustive(q.data_ptr(), sel.data_ptr(), sel.numel(), self._xb.data_ptr(), n,
                                              self.d, k, self._fmt.code, self.id_offset, metric, D.data_ptr(),
                                              I.data_ptr(), ws.data_ptr(), ws.numel(), _lib.stream_ptr(self.device))
            _lib.check(rc, "sss_ip_topk_exhaustive")

    def search_device(self, q: torch.Tensor, k: int):
        """Exact search, CUDA tensors in and out (syncs once to read the status vector)."""
        if q.dtype != self._tdtype:
            q = self._rows(q, "search")
        nq = q.shape[0]
        D = torch.empty((nq, k), dtype=torch.float32, device=self.device)
        I = torch.empty((nq, k), dtype=torch.int64, device=self.device)
        self.last_fallback_queries = self.last_rescan_queries = 0
        if nq == 0:
            return D, I
        if self.ntotal == 0:
            D.fill_(-3.4028234663852886e38 if self.metric == "ip" else 3.4028234663852886e38)
            I.fill_(-1)
            return D, I
        self._require_d_aligned()
        mode = self._route(k)
        if mode:
            # the per-query workspace is 16 KB (fused scans) to 64 KB (long rows, threshold rung): the reference hands
            # `index.search` its whole test set at once (test_amazon_filterd.py:578), so large batches go in chunks
            step = SEARCH_CHUNK_LONG if mode == "long" else SEARCH_CHUNK
            status = torch.empty((nq,), dtype=torch.int32, device=self.device)
            rescans = fallbacks = 0
            for lo in range(0, nq, step):
                hi = min(nq, lo + step)
                part = (D[lo:hi], I[lo:hi], status[lo:hi])
                self.search_fused(q[lo:hi], k, part)
                self.fix_unproven(q[lo:hi], k, *part)
                rescans += self.last_rescan_queries
                fallbacks += self.last_fallback_queries
            self.last_rescan_queries, self.last_fallback_queries = rescans, fallbacks
        else:
            self.last_fallback_queries = nq
            self.search_exhaustive(q, k, D, I)
        return D, I

    def search(self, x, k: int):
        """``index.search(x, k) -> (D, I)``: numpy in -> numpy out (faiss), tensor in -> tensors."""
        is_np = isinstance(x, np.ndarray)
        q = self._rows(x, "search")
        D, I = self.search_device(q, int(k))
        if is_np:
            return D.cpu().numpy(), I.cpu().numpy()
        return D, I

    # ------------------------------------------------------------------ range search
    def _radius(self, radius, nq: int) -> torch.Tensor:
        """The radius as a device float32 [nq] tensor (a scalar for every query, or one per query); NaN raises."""
        if isinstance(radius, torch.Tensor):
            r = radius.detach().to(device=self.device, dtype=torch.float32).reshape(-1)
        else:
            r = torch.from_numpy(np.asarray(radius, dtype=np.float32).reshape(-1)).to(self.device)
        if r.numel() == 1:
            r = r.expand(nq)
        elif r.numel() != nq:
            raise ValueError(f"range_search: radius must be a scalar or have {nq} entries, got {r.numel()}")
        if bool(torch.isnan(r).any()):
            raise ValueError("range_search: radius is NaN")
        return r.contiguous()

    def range_search_device(self, q: torch.Tensor, radius):
        """Exact range search, CUDA tensors in and out: (lims int64 [nq + 1], D float32 [lims[nq]], I int64 [lims[nq]]).
        Query i's results are D[lims[i]:lims[i+1]] / I[...], in ascending id order: every row with canonical score
        > radius (inner product) or squared distance < radius (L2), radius converted to float32.  Syncs once per chunk
        of queries (to size the output).  A ``pad_scan`` index answers on the exhaustive route (``last_range_scan == ""``):
        the fused range route at padded widths is not built."""
        if q.dtype != self._tdtype:
            q = self._rows(q, "range_search")
        nq, n = q.shape[0], self.ntotal
        rad = self._radius(radius, nq)
        self.last_range_scan, self.last_range_overflow_queries = "", 0
        lims = torch.zeros(nq + 1, dtype=torch.int64, device=self.device)
        if nq == 0 or n == 0:
            return lims, torch.empty(0, dtype=torch.float32, device=self.device), torch.empty(0, dtype=torch.int64, device=self.device)
        self._require_d_aligned()
        L, st = _lib.lib(), _lib.stream_ptr(self.device)
        pieces = []                     # (query rows [host int64], their counts [host int64], D, I) in the order they were produced
        mode = self.last_range_scan = "" if self._pad else self.rung_scan()      # (pad_scan: the exhaustive route)
        left = []                       # query rows for the exhaustive route
        if mode:
            image, code, shift, resid = self._scan_image(mode)
            cmax = self.corpus_max_norm()
            for lo in range(0, nq, RANGE_CHUNK):
                m = min(nq, lo + RANGE_CHUNK) - lo
                ws = self._ws.get(L.sss_range_search_workspace_bytes(m, n, self.d, code))
                cs = torch.empty(2 * m, dtype=torch.int64, device=self.device)           # counts | status (one copy to the host)
                status = torch.empty(m, dtype=torch.int32, device=self.device)
                rc = L.sss_range_search_count(q[lo:].data_ptr(), m, self._xb.data_ptr(), self._fmt.code, image.data_ptr(),
                                              code, shift, resid, n, self.d, rad[lo:].data_ptr(), cmax, cs.data_ptr(),
                                              status.data_ptr(), ws.data_ptr(), ws.numel(), st)
                _lib.check(rc, "sss_range_search_count")
                cs[m:] = status
                host = cs.cpu().numpy()
                counts, bad = host[:m], np.flatnonzero(host[m:])
                D, I = self._range_fill(m, counts, lambda lims, D, I: L.sss_range_search_fill(
                    m, lims.data_ptr(), self.id_offset, D.data_ptr(), I.data_ptr(), ws.data_ptr(), ws.numel(), st),
                    "sss_range_search_fill")
                pieces.append((np.arange(lo, lo + m, dtype=np.int64), counts, D, I))
                left.extend((bad + lo).tolist())
            self.last_range_overflow_queries = len(left)
        else:
            left = range(nq)
        if len(left):
            metric = 0 if self.metric == "ip" else 1
            rows = torch.as_tensor(np.asarray(left, dtype=np.int32), device=self.device)
            for lo, sel, ws in self._exhaustive_chunks(rows, L.sss_range_search_exhaustive_workspace_bytes):
                m = sel.numel()
                counts_t = torch.empty(m, dtype=torch.int64, device=self.device)
                rc = L.sss_range_search_exhaustive_count(q.data_ptr(), sel.data_ptr(), m, self._xb.data_ptr(), n, self.d,
                                                         self._fmt.code, metric, rad.data_ptr(), counts_t.data_ptr(),
                                                         ws.data_ptr(), ws.numel(), st)
                _lib.check(rc, "sss_range_search_exhaustive_count")
                counts = counts_t.cpu().numpy()
                D, I = self._range_fill(m, counts, lambda lims, D, I: L.sss_range_search_exhaustive_fill(
                    sel.data_ptr(), m, n, metric, rad.data_ptr(), lims.data_ptr(), self.id_offset, D.data_ptr(), I.data_ptr(),
                    ws.data_ptr(), ws.numel(), st), "sss_range_search_exhaustive_fill")
                pieces.append((np.asarray(left[lo:lo + m], dtype=np.int64), counts, D, I))
        return self._range_merge(nq, pieces)

    def _range_fill(self, m, counts, fill, what):
        """Allocate one piece's output from its host counts and run its fill call (no-op when it is empty)."""
        lims_h = np.zeros(m + 1, dtype=np.int64)
        np.cumsum(counts, out=lims_h[1:])
        total = int(lims_h[-1])
        D = torch.empty(total, dtype=torch.float32, device=self.device)
        I = torch.empty(total, dtype=torch.int64, device=self.device)
        if total:
            lims = torch.from_numpy(lims_h).to(self.device)
            _lib.check(fill(lims, D, I), what)
        return D, I

    def _range_merge(self, nq, pieces):
        """One (lims, D, I) in query order from the pieces of the two routes."""
        counts = np.zeros(nq, dtype=np.int64)
        for rows, cnt, _, _ in pieces:
            counts[rows] = cnt
        lims_h = np.zeros(nq + 1, dtype=np.int64)
        np.cumsum(counts, out=lims_h[1:])
        lims = torch.from_numpy(lims_h).to(self.device)
        total = int(lims_h[-1])
        live = [p for p in pieces if p[2].numel()]
        if len(live) == 1 and len(live[0][0]) == nq:        # one piece holds every query, in order: it IS the result
            return lims, live[0][2], live[0][3]
        D = torch.empty(total, dtype=torch.float32, device=self.device)
        I = torch.empty(total, dtype=torch.int64, device=self.device)
        for rows, cnt, Dp, Ip in live:
            own = np.zeros(len(rows) + 1, dtype=np.int64)
            np.cumsum(cnt, out=own[1:])
            # destination of entry j of the piece's query t: lims[rows[t]] + (j - own[t])
            shift = torch.from_numpy(np.repeat(lims_h[rows] - own[:-1], cnt)).to(self.device)
            dest = shift + torch.arange(Dp.numel(), dtype=torch.int64, device=self.device)
            D[dest] = Dp
            I[dest] = Ip
        return lims, D, I

    def range_search(self, x, radius):
        """``index.range_search(x, radius) -> (lims, D, I)`` (faiss): numpy in -> numpy out, tensor in -> tensors.
        ``radius``: a scalar (faiss) or one value per query."""
        is_np = isinstance(x, np.ndarray)
        q = self._rows(x, "range_search")
        lims, D, I = self.range_search_device(q, radius)
        if is_np:
            return lims.cpu().numpy(), D.cpu().numpy(), I.cpu().numpy()
        return lims, D, I


def build_index(emb, metric: str, device=None, *, pad_scan: bool = False) -> FlatIndex:
    """Reference ``build_index(emb, metric)`` (test_amazon_filterd.py:207-223).  ``pad_scan``: as ``FlatIndex`` (the
    matrix-core scans for widths without one of their own, the reference's emb_len = 200 among them)."""
    if metric == "cos":
        index = FlatIndex(emb.shape[1], "ip", device, pad_scan=pad_scan)
        index.add(normalize(emb))
    elif metric == "l2":
        index = FlatIndex(emb.shape[1], "l2", device, pad_scan=pad_scan)
        index.add(emb)
    elif metric == "ip":
        index = FlatIndex(emb.shape[1], "ip", device, pad_scan=pad_scan)
        index.add(emb)
    else:
        raise RuntimeError("Unregnozed metric", metric)
    return index


# ------------------------------------------------------------------------------- binary codes
def pack_sign_bits(emb, code_bytes: int | None = None) -> torch.Tensor:
    """``np.packbits(((emb + 1) / 2).astype(int), axis=1)`` of the reference (fine_tune_ours.py:839-840,
    871-872) on the device: ``emb`` is the (+-1 valued) BinarizeHead output [n, c]; returns uint8
    [n, code_bytes] (default ceil(c / 8), zero padded like packbits)."""
    dev = _dev() if isinstance(emb, np.ndarray) or not emb.is_cuda else emb.device
    x = _as_device_f32(emb, dev)
    n, c = x.shape
    nbytes = (c + 7) // 8 if code_bytes is None else int(code_bytes)
    out = torch.empty((n, nbytes), dtype=torch.uint8, device=dev)
    rc = _lib.lib().sss_pack_sign_bits(x.data_ptr(), n, c, x.stride(0), out.data_ptr(), nbytes, _lib.stream_ptr(dev))
    _lib.check(rc, "sss_pack_sign_bits")
    return out


class BinaryFlatIndex:
    """``faiss.IndexBinaryFlat(nbits)`` as the reference uses it (fine_tune_ours.py:841-843,876):
    ``add(codes)`` with uint8 [n, nbits / 8] rows, ``search(codes, k) -> (D int32, I int64)`` by
    Hamming distance ascending, ties by ascending id.  Codes are stored in rows of 128 / 256 / 512 / 1024 / 2048 bits,
    zero padded to the next of these widths (padding adds no distance; 1600 bits, the sign code of the session
    vector, is stored in 2048), and every stored width runs on the fused scan; queries it cannot prove go through
    the exhaustive kernels."""

    WIDTHS = (16, 32, 64, 128, 256)     # stored row bytes

    @classmethod
    def stored_bytes(cls, nbits: int) -> int:
        """Row bytes a code of `nbits` bits is stored in: the next of WIDTHS."""
        if nbits % 8:
            raise ValueError("nbits must be a multiple of 8")
        if nbits > 8 * cls.WIDTHS[-1]:
            raise ValueError(f"codes longer than {8 * cls.WIDTHS[-1]} bits are not supported")
        return next(w for w in cls.WIDTHS if w >= nbits // 8)

    def __init__(self, nbits: int, device=None):
        self._w = self.stored_bytes(nbits)                                  # stored (padded) row bytes
        self.d = int(nbits)
        self.code_bytes = nbits // 8
        self.device = _dev(device)
        self._codes = torch.empty((0, self._w), dtype=torch.uint8, device=self.device)
        self._store = self._codes       # backing storage of _codes (grown geometrically by add())
        self._ws = Workspace(self.device)
        self.id_offset = 0
        self.last_fallback_queries = 0

    @property
    def ntotal(self) -> int:
        return int(self._codes.shape[0])

    def _rows(self, x):
        if isinstance(x, np.ndarray):
            x = torch.from_numpy(np.ascontiguousarray(x, dtype=np.uint8))
        x = x.to(self.device, torch.uint8)
        if x.dim() != 2 or x.shape[1] != self.code_bytes:
            raise ValueError(f"expected uint8 [n, {self.code_bytes}], got {tuple(x.shape)}")
        if self._w != self.code_bytes:
            pad = torch.zeros((x.shape[0], self._w), dtype=torch.uint8, device=self.device)
            pad[:, :self.code_bytes] = x
            x = pad
        return x.contiguous()

    def add(self, codes):
        self._store, self._codes = grow_rows(self._store, self._codes, self._rows(codes))

    def search(self, codes, k: int):
        is_np = isinstance(codes, np.ndarray)
        L = _lib.lib()
        q = self._rows(codes)
        nq, n, k = q.shape[0], self.ntotal, int(k)
        D = torch.full((nq, k), 0x7fffffff, dtype=torch.int32, device=self.device)
        I = torch.full((nq, k), -1, dtype=torch.int64, device=self.device)
        self.last_fallback_queries = 0
        if nq and n:
            st = _lib.stream_ptr(self.device)
            if k <= L.sss_hamming_topk_capacity(nq, n):
                ws = self._ws.get(L.sss_hamming_topk_workspace_bytes(nq, n))
                status = torch.empty((nq,), dtype=torch.int32, device=self.device)
                rc = L.sss_hamming_topk(q.data_ptr(), nq, self._codes.data_ptr(), n, self._w, k, self.id_offset, D.data_ptr(),
                                        I.data_ptr(), status.data_ptr(), ws.data_ptr(), ws.numel(), st)
                _lib.check(rc, "sss_hamming_topk")
                bad = torch.nonzero(status).flatten().to(torch.int32)
            else:                               # k beyond the fused capacity: everything through the exhaustive path
                bad = torch.arange(nq, dtype=torch.int32, device=self.device)
            self.last_fallback_queries = int(bad.numel())
            per = exhaustive_chunk(n, 2)
            for lo in range(0, bad.numel(), per):
                sel = bad[lo:lo + per].contiguous()
                ws = self._ws.get(L.sss_hamming_topk_exhaustive_workspace_bytes(sel.numel(), n))
                rc = L.sss_hamming_topk_exhaustive(q.data_ptr(), sel.data_ptr(), sel.numel(), self._codes.data_ptr(), n,
                                                   self._w, k, self.id_offset, D.data_ptr(), I.data_ptr(), ws.data_ptr(),
                                                   ws.numel(), st)
                _lib.check(rc, "sss_hamming_topk_exhaustive")
        if is_np:
            return D.cpu().numpy(), I.cpu().numpy()
        return D, I
