"""Which scan serves a search: the routing policy of ``FlatIndex`` as host logic that needs no device, tensor or library."""
from __future__ import annotations

F32_SCAN_DIMS = (64, 128, 256)                                   # "split" and "f32" scans: 4 bytes per element
F16_SCAN_DIMS = (128, 256, 512)                                  # scaled-f16 image: 2 bytes per element
PAD_SCAN_MAX_D = 512             # pad_scan=True: float32 rows of 4 <= d <= 512, d % 4 == 0, scanned at the next width a scan has
# scan="auto": the fastest scan whose error bound is still small against the spacing of the scores
# around rank k (the spacing shrinks as k grows): one-pass f16 up to k = 128, bf16 split up to k = 500
# (every k the fused path serves); the f32 MFMA scan is reached by escalation only.  Measured on random unit
# rows, d = 128, 1024 queries (round 3): f16 leaves 0 of 6144 queries unproven at k <= 64 on 10M rows, 8 at k = 128,
# 60 at k = 200 (the k classes are cut there); split leaves 0-1 up to k = 500, at 0.4x the f32 scan's time.  A
# search whose fallback share exceeds AUTO_ESCALATE moves that k class one scan up for the following searches
# (near-duplicate-heavy or unusually dense corpora); an unproven query costs a share of one more scan of the
# corpus for the unproven ones only (the threshold rung), so a few per batch are cheaper than the slower scan.
AUTO_F16_MAX_K = 128
AUTO_SPLIT_MAX_K = 500
AUTO_ESCALATE = 0.005
AUTO_DECAY_SEARCHES = 64        # clean searches at an escalated level before the class steps back down one scan
_LADDER = ("f16", "split", "f32")
FUSED_MAX_K = 500
LONG_MAX_K = 1024                                                # sss_ip_topk_long: what its exhaustive fallback resolves
LONG_MAX_ROW_BYTES = 16384
# The L2 scans start every score from the row bias -|c|^2 / 2, a float32: the scan route is taken only where the largest
# row norm keeps cmax^2 / 2 finite and normal with room to spare (2^-121 .. 2^119); beyond, the exhaustive kernels.
L2_SCAN_MIN_NORM = 2.0 ** -60
L2_SCAN_MAX_NORM = 2.0 ** 60


class ScanRouting:
    """The two decisions -- ``_route(k)``: the scan of a search, ``_rung_route()``: the scan of its threshold rung -- of
    which every public view is a projection, and the ``scan="auto"`` ladder state.  ``fmt`` is the storage format's record
    (``fused_dims``, ``long_rows``, ``elem_bytes``).  What the policy reads about the corpus -- ``ntotal``,
    ``corpus_max_norm()``, ``_image_complete(scan)`` -- an index answers from its own state; on its own the object
    answers ``ntotal``, ``max_norm`` and ``complete`` (the scans whose image holds every row) as given."""

    _pad = False                        # pad_scan is off unless __init__ finds the switch set on a shape it applies to

    def __init__(self, d: int, metric: str = "ip", dtype: str = "f32", scan: str | None = None, pad_scan: bool = False, *,
                 fmt, ntotal: int = 0, max_norm: float = 0.0, complete=()):
        if metric not in ("ip", "l2"):
            raise ValueError("metric must be 'ip' or 'l2'")
        if scan is None:
            scan = "auto" if dtype == "f32" else "native"
        if scan not in (("auto", "f16", "split", "f32") if dtype == "f32" else ("native",)):
            raise ValueError("scan must be 'auto', 'f16', 'split' or 'f32' for a float32 index")
        self.d, self.metric, self.dtype, self.scan, self._format = int(d), metric, dtype, scan, fmt
        self.last_scan = None           # the scan the last fused search used
        self._auto_level = {}           # scan="auto": k class -> lowest ladder level still allowed
        self._auto_clean = {}           # scan="auto": k class -> consecutive clean searches at the escalated level
        self._auto_rows = 0             # scan="auto": corpus size when a class last escalated
        # pad_scan: the scans run at scan_width(scan) >= d; where d has a scan of its own the switch changes nothing
        self._pad = bool(pad_scan) and dtype == "f32" and 4 <= self.d <= PAD_SCAN_MAX_D and self.d % 4 == 0 and self.d % 64 != 0
        self._ntotal, self._max_norm, self._complete = int(ntotal), float(max_norm), set(complete)

    # ------------------------------------------------------------------ what the policy reads: the format, the corpus
    _fmt = property(lambda self: self._format)

    @property
    def ntotal(self) -> int:
        return self._ntotal

    def corpus_max_norm(self) -> float:
        return self._max_norm

    def _image_complete(self, scan: str) -> bool:           # does the image scan "f16" / "split" reads hold every row?
        return scan in self._complete

    # ------------------------------------------------------------------ the scan of a search
    def _route(self, k: int) -> str:
        """The scan a search for k results runs on under this index's metric: "native" (the stored rows of a 16- or
        8-bit index), "f16" / "split" / "f32" (the ladder of a float32 index), "long" (the K-tiled scan for rows beyond
        the register-resident kernels), "" = the exhaustive kernels.  An L2 index has scans for float32 rows only and
        reads the corpus's largest row norm -- a host read on first use -- only once shape, dtype and k have passed."""
        l2 = self.metric == "l2"
        if k <= 0 or self.ntotal == 0 or (l2 and self.dtype != "f32"):
            return ""
        fused = self._fused_shape()
        served = k <= FUSED_MAX_K if fused else self._long_or_none(k) != ""
        if not served or (l2 and not L2_SCAN_MIN_NORM <= self.corpus_max_norm() <= L2_SCAN_MAX_NORM):
            return ""
        return "long" if not fused else self._ladder_scan(k) if self.dtype == "f32" else "native"

    def scan_for(self, k: int) -> str:
        """Which candidate scan a fused inner-product search for k results uses ("" = none: exhaustive; any L2 index)."""
        return self._route(k) if self.metric == "ip" else ""

    def l2_scan_for(self, k: int) -> str:
        """Which fused scan an L2 search for k results uses ("" = none): the ladder of ``scan_for``, for a float32 index
        whose d has a fused kernel, k <= 500 and a largest row norm in [2^-60, 2^60]."""
        route = self._route(k) if self.metric == "l2" else ""
        return "" if route == "long" else route

    def l2_long_for(self, k: int) -> str:
        """"long" where an L2 search for k results runs on the K-tiled long-row scan (``sss_l2_topk_long``), else "":
        float32 rows beyond the fused scans, k <= ``LONG_MAX_K``, a largest row norm in [2^-60, 2^60].  A ``pad_scan``
        index has a fused scan at every width it accepts and never comes here."""
        return "long" if self.metric == "l2" and self._route(k) == "long" else ""

    def fused_ok(self, k: int) -> bool:
        return self.scan_for(k) != ""

    def _fused_shape(self) -> bool:
        """Does a register-resident scan read rows of this d: the format's own, or one of a float32 index's images?"""
        return self.d in self._fmt.fused_dims or (self.dtype == "f32" and any(self._scan_served(s) for s in _LADDER))

    def _long_or_none(self, k: int) -> str:
        """"long": the K-tiled scan for rows beyond the register-resident kernels (``sss_ip_topk_long``)."""
        if not self._fmt.long_rows:
            return ""                            # (int8 rows: the exhaustive kernels)
        row_bytes = self.d * self._fmt.elem_bytes
        return "long" if (self.d % 64 == 0 and row_bytes <= LONG_MAX_ROW_BYTES and k <= LONG_MAX_K) else ""

    def _ladder_scan(self, k: int) -> str:
        """The scan of a float32 index for k results by its ``scan`` argument and, for "auto", what the searches
        so far have taught it ("" = this d has none)."""
        want = self.scan
        if want == "auto":
            level = max(self._k_class(k), self._auto_level.get(self._k_class(k), 0))
            served = [s for s in _LADDER[level:] if self._scan_served(s)]
            # nothing at or above the wanted level fits this d (e.g. d = 512: only the f16 image does):
            # stay on the fastest scan that does rather than fall off the ladder
            served = served or [s for s in _LADDER if self._scan_served(s)]
            return served[0] if served else ""
        if want == "f16" and not self._scan_served("f16"):
            want = "split"
        if self._pad and not self._scan_served(want):
            want = "f16"                         # pad_scan, 256 < d <= 512: the f16 image is the only scan that wide
        return want if self._scan_served(want) else ""

    def _scan_served(self, scan: str) -> bool:
        """Does a fused kernel exist for this scan at this d (``pad_scan``: at a width this d is padded to)?"""
        return self.scan_width(scan) != 0

    def scan_width(self, scan: str) -> int:
        """The row width scan "f16" / "split" / "f32" runs at on this float32 index: d where d is one of the scan's
        widths; on a ``pad_scan`` index the smallest of them that is at least d (``256 < d <= 512`` has the f16 scan only,
        whatever ``scan`` says); 0 where the scan does not serve it."""
        widths = F16_SCAN_DIMS if scan == "f16" else F32_SCAN_DIMS
        if self._pad:
            return next((w for w in widths if w >= self.d), 0)
        return self.d if self.d in widths else 0

    def next_scan(self, scan: str) -> str:
        """The next scan up the precision ladder that this d can run ("" = none)."""
        if self.dtype != "f32" or scan not in _LADDER:
            return ""
        return next((s for s in _LADDER[_LADDER.index(scan) + 1:] if self._scan_served(s)), "")

    # ------------------------------------------------------------------ the scan of the threshold rung
    def _rung_route(self) -> str:
        """The scan the threshold rung uses ("" = none): the one-pass f16 image where the shape has one (cheapest pass
        over the corpus; its wider error window only means a few more rows to re-score), else the index's own rows.
        Long rows have none: their scan IS a threshold scan, and what it leaves is mass ties.  An L2 index has one
        where its searches have a fused scan at all."""
        if self.ntotal == 0 or not self._fused_shape() or (self.metric == "l2" and self._route(1) == ""):
            return ""
        if self.dtype != "f32":
            return "native"
        served = self._scan_served
        if self.scan == "auto":
            # an image that is already complete beats building another one (n * d * 2 bytes) for a handful of queries
            split_ready = self._image_complete("split")
            if served("f16") and (self._image_complete("f16") or not split_ready):
                return "f16"
            if split_ready and served("split"):
                return "split"
        if self.scan in ("f16", "split") and served(self.scan):
            return self.scan
        return "f32" if served("f32") else ("f16" if served("f16") else "")

    def rung_scan(self) -> str:                             # the rung's scan of an inner-product index ("" on an L2 index)
        return self._rung_route() if self.metric == "ip" else ""

    def l2_rung_scan(self) -> str:                          # ... of an L2 index ("" on an inner-product index)
        return self._rung_route() if self.metric == "l2" else ""

    # ------------------------------------------------------------------ scan="auto": what the searches teach
    @staticmethod
    def _k_class(k: int) -> int:
        return 0 if k <= AUTO_F16_MAX_K else 1 if k <= AUTO_SPLIT_MAX_K else 2

    def _note_fallbacks(self, k: int, nq: int, bad: int):
        """scan="auto": move this k class one scan up when too many queries of a search were left
        unproven by it -- only to a scan this d can run -- and back down one scan after
        AUTO_DECAY_SEARCHES consecutive clean searches (one near-duplicate-heavy batch does not demote
        the index for good); an escalation that proves no more queries than the faster scan did is undone."""
        if self.scan != "auto" or self.last_scan not in _LADDER:
            return
        kc = self._k_class(k)
        share = bad / max(nq, 1)
        # The first search after an escalation tells whether it helped: exact ties (duplicate rows at the k-th place)
        # stay unproven under EVERY scan -- the threshold rung resolves them, at a cost that hardly depends on how
        # many there are -- so a slower scan that still leaves more than AUTO_ESCALATE of the batch unproven only
        # costs time.  Such a step is taken back and the class pinned for AUTO_DECAY_SEARCHES searches.
        probe = self._auto_clean.pop(("probe", kc), None)
        if probe is not None and nq >= 32 and bad >= 4 and share > AUTO_ESCALATE:
            self._auto_level[kc] = probe[0]
            self._auto_clean[("pin", kc)] = AUTO_DECAY_SEARCHES
            self._auto_clean[kc] = 0
            return
        pin = self._auto_clean.get(("pin", kc), 0)
        if pin > 0:
            self._auto_clean[("pin", kc)] = pin - 1
            return
        if nq >= 32 and bad >= 4 and bad > AUTO_ESCALATE * nq:
            up = self.next_scan(self.last_scan)
            if up:
                self._auto_clean[("probe", kc)] = (_LADDER.index(self.last_scan), share)
                self._auto_level[kc] = _LADDER.index(up)
                self._auto_rows = self.ntotal
            self._auto_clean[kc] = 0
        elif self._auto_level.get(kc, 0) > kc and nq >= 32:
            self._auto_clean[kc] = self._auto_clean.get(kc, 0) + 1 if bad == 0 else 0      # consecutive: any unproven query restarts the count
            if self._auto_clean[kc] >= AUTO_DECAY_SEARCHES:
                self._auto_level[kc] -= 1
                self._auto_clean[kc] = 0
