"""The query text encoder of the reference's two-tower model: ``NodeTextTransformer`` (``model/NodeEmbedding.py:62-98``) in
eval mode -- ``nn.Embedding * sqrt(ninp)`` + the sinusoidal ``PositionalEncoding``, ``nlayers`` post-norm
``nn.TransformerEncoderLayer(ninp, nhead, nhid)`` with relu and a key-padding mask, then a plain mean over the token axis.

* ``pack_tokens``            host side, numpy, device-free: ``[B, T]`` tokens + padding mask -> packed token rows
* ``text_fold_weights``      host side, float64, device-free: ``1 / sqrt(D)`` folded into the q rows of ``in_proj``, every
                             GEMM operand padded with zero columns to a multiple of 32
* ``NodeTextTransformer``    the drop-in: ``forward(src, mask) -> [B, ninp]`` float32 on the device

THE TWO PADDING RULES.  The reference's pooling is an unmasked mean over all
``T`` positions.  What the padded positions hold depends on how torch ran the encoder:

* ``pad_rule="compute"`` (default): the module's mathematics, and what it was trained under.  A padded position is an
  ordinary row: it attends over the valid keys only, goes through every layer and is averaged in with the rest.  This is
  what every torch returns in training mode, with the nested-tensor fast path off, or under a non-prefix mask.
* ``pad_rule="zero"``: what a current torch returns in ``eval()`` under ``no_grad()`` for a prefix mask (a tokenizer's): the
  fast path hands padded positions back as exact zeros, so the result is ``sum over real tokens / T``.  Padded tokens never
  reach a kernel: a batch of short queries costs only its real tokens.

Every arithmetic step runs in ``libsss.so``: ``sss_text_embed``, ``sss_seq_attention``, ``sss_add_layernorm``
(include/sss_text.h), ``sss_linear_grouped`` for the four GEMMs of a layer (``sss_linear_grouped_bf16`` of
include/lowp/sss_linear_bf16.h under ``gemm="bf16"``) and ``sss_segment_reduce`` for the pooling; torch owns memory only.
A layer is 7 launches, a forward ``7 * nlayers + 2`` per chunk of rows.

The second half of the module is the deployed model's node text encoder, ``PretrainedQAEAEncoder``
(``model/NodeEmbedding.py:100-125``): a BERT encoder without its pooling layer, a masked mean over the tokens and an
optional ``Linear``, on the same packed rows and the same layer launches:

* ``bert_pack_rows``         host side, numpy, device-free: ids, token types and attention mask -> packed rows + pool weights
* ``unique_rows``            host side, numpy, device-free: the distinct ``(ids, types, mask)`` rows, each encoded once
* ``bert_fold_weights``      host side, float64, device-free: ``query | key | value`` as one ``in_proj``, the same folds and pads
* ``BertNodeEncoder``        the drop-in: ``enc(input_ids, token_type_ids, attention_mask, get_token=False)``

Its embedding stage is ``sss_bert_embed`` (include/sss_bert.h), its feed-forward activation ``act = 5`` (exact GELU) of
``sss_linear_grouped``; de-duplicated rows are scattered with ``sss_gather_rows``.
"""
from __future__ import annotations

import ctypes
import math
from collections import namedtuple

import numpy as np

from ._lib import pad32 as _pad32

MAX_LEN = 64                                 # rows per sequence sss_seq_attention takes: one lane per query row
PAD_RULES = ("compute", "zero")
GEMMS = ("f32", "bf16")                     # what the dense layers run on: sss_linear_grouped / sss_linear_grouped_bf16
GEMM_WEIGHTS = ("in_w", "out_w", "l1_w", "l2_w")     # the keys of a folded layer that are a GEMM's weight

TokenRows = namedtuple("TokenRows", "tok pos ptr key_ok T")
TokenRows.__doc__ = """Packed token rows: ``tok`` int64 [n] and ``pos`` int32 [n] per row, ``ptr`` int32 [B + 1] the row range of
each sequence, ``key_ok`` uint8 [n] (1: the row is a key of its sequence), ``T`` the padded length the mean divides by."""


def _host(a):
    """numpy array of a numpy array or a torch tensor on any device (20 integers per node: the copy is cheap)."""
    if hasattr(a, "detach"):
        a = a.detach().cpu().numpy()
    return np.asarray(a)


def _check_rule(pad_rule):
    if pad_rule not in PAD_RULES:
        raise ValueError(f"pad_rule must be 'compute' or 'zero', got {pad_rule!r}")


def _check_gemm(gemm):
    if gemm not in GEMMS:
        raise ValueError(f"gemm must be 'f32' or 'bf16', got {gemm!r}")


def pack_tokens(src, mask, pad_rule="compute", ntoken=None):
    """``src [B, T]`` token ids and ``mask [B, T]`` (True = padding, as ``src_key_padding_mask``) -> ``TokenRows``.

    ``"compute"`` keeps all ``T`` rows of each sequence with ``key_ok = ~mask``; ``"zero"`` keeps only the unmasked rows,
    with their original positions and ``key_ok = 1`` (any mask, prefix or not).  ``T <= 64``; a sequence with no unmasked
    token raises ``ValueError`` (the reference's softmax gives NaN there and its own assert trips); with ``ntoken`` given, an
    id outside ``[0, ntoken)`` anywhere in ``src`` raises ``IndexError``, as ``nn.Embedding`` does."""
    _check_rule(pad_rule)
    src, mask = _host(src), _host(mask)
    if src.ndim != 2 or mask.shape != src.shape:
        raise ValueError(f"src and mask must both be [B, T]; got {src.shape} and {mask.shape}")
    if not np.issubdtype(src.dtype, np.integer):
        raise ValueError(f"src must hold integer token ids, got dtype {src.dtype}")
    B, T = src.shape
    if T > MAX_LEN:
        raise ValueError(f"sequences of T = {T} tokens: at most {MAX_LEN} are supported")
    mask = mask.astype(bool)
    if B and T == 0 or bool(mask.all(axis=1).any()):
        raise ValueError("a sequence has no unmasked token (the reference's softmax gives NaN there)")
    if ntoken is not None and src.size and (int(src.min()) < 0 or int(src.max()) >= ntoken):
        raise IndexError(f"token id out of range [0, {ntoken})")
    keep = np.ones((B, T), dtype=bool) if pad_rule == "compute" else ~mask
    counts = keep.sum(axis=1)
    if int(counts.sum()) >= 2 ** 31:
        raise ValueError(f"{int(counts.sum())} token rows: at most 2^31 - 1 fit one call")
    ptr = np.zeros(B + 1, dtype=np.int32)
    np.cumsum(counts, out=ptr[1:])
    b, t = np.nonzero(keep)                                  # row-major: sequences in order, positions ascending
    return TokenRows(src[b, t].astype(np.int64), t.astype(np.int32), ptr, (~mask[b, t]).astype(np.uint8), T)


LAYER = "transformer_encoder.layers.{}."
# the keys of a folded layer -> the tensor's name under LAYER; in_w / in_b arrive as q | k | v rows of one tensor
LAYER_NAMES = {"in_w": "self_attn.in_proj_weight", "in_b": "self_attn.in_proj_bias", "out_w": "self_attn.out_proj.weight",
               "out_b": "self_attn.out_proj.bias", "l1_w": "linear1.weight", "l1_b": "linear1.bias", "l2_w": "linear2.weight",
               "l2_b": "linear2.bias", "n1_w": "norm1.weight", "n1_b": "norm1.bias", "n2_w": "norm2.weight", "n2_b": "norm2.bias"}


def _pad(w, rows, cols):
    import torch
    out = torch.zeros((rows, cols), dtype=torch.float64)
    out[:w.shape[0], :w.shape[1]] = w
    return out


def _fold_layers(weights, prefix, names, stacked, e, D):
    """The layers of both folds, float64: ``(layers, inner)`` with ``layers`` the per-layer dicts ``text_fold_weights``
    documents and ``inner`` the feed-forward width.  ``names`` maps the twelve keys of such a dict to the tensor's name under
    ``prefix.format(l)``; ``stacked``: ``in_w`` / ``in_b`` name one tensor of q | k | v rows, otherwise the three of them.  The
    layers are counted by probing the first of these names; q is divided by ``sqrt(D)`` first, padded second."""
    import torch
    probe = prefix + (names["in_w"] if stacked else names["in_w"][0])
    nlayers = 0
    while probe.format(nlayers) in weights:
        nlayers += 1
    if nlayers == 0:
        raise ValueError(f"weights hold no {probe.format(0)}")
    inner = int(weights[prefix.format(0) + names["l1_w"]].shape[0])
    K, Hp = _pad32(e), _pad32(inner)
    layers = []
    for l in range(nlayers):
        f64 = lambda name: weights[prefix.format(l) + name].detach().to("cpu", torch.float64)
        g = lambda key: f64(names[key])

        def qkv(key):
            t = g(key) if stacked else torch.cat([f64(name) for name in names[key]])
            return torch.cat([t[:e] / math.sqrt(D), t[e:]])

        l1_b = torch.zeros(Hp, dtype=torch.float64)
        l1_b[:inner] = g("l1_b")
        layers.append({"in_w": _pad(qkv("in_w"), 3 * e, K), "in_b": qkv("in_b"), "out_w": _pad(g("out_w"), e, K), "out_b": g("out_b"),
                       "l1_w": _pad(g("l1_w"), Hp, K), "l1_b": l1_b, "l2_w": _pad(g("l2_w"), e, Hp), "l2_b": g("l2_b"),
                       "n1_w": g("n1_w"), "n1_b": g("n1_b"), "n2_w": g("n2_w"), "n2_b": g("n2_b")})
    return layers, inner


def text_fold_weights(weights, nhead):
    """Host-side, device-free, float64: the weights of ``NodeTextTransformer`` (the module's own ``state_dict()`` names) as
    the kernels take them.  ``1 / sqrt(D)`` is folded into the q rows of ``in_proj`` (weight and bias), so the attention
    kernel's score is a plain dot product; every GEMM's K is padded with zero columns to a multiple of 32, and ``linear1``
    with zero rows and zero bias to ``pad32(nhid)`` outputs, so that the relu writes the pad columns ``linear2`` reads as
    exact zeros.

    Returns ``{"ninp", "nhead", "nhid", "nlayers", "table" [ntoken, ninp], "pe" [n_pos, ninp], "scale" (float32
    sqrt(ninp)), "layers": [{"in_w" [3 e, K], "in_b", "out_w" [e, K], "out_b", "l1_w" [H, K], "l1_b" [H], "l2_w" [e, H],
    "l2_b", "n1_w", "n1_b", "n2_w", "n2_b"}]}`` with ``K = pad32(ninp)``, ``H = pad32(nhid)``."""
    import torch
    f64 = lambda name: weights[name].detach().to("cpu", torch.float64)
    table = f64("embedding.weight")
    e, H = int(table.shape[1]), int(nhead)
    if H < 1 or e % H:
        raise ValueError(f"ninp = {e} is not a multiple of nhead = {nhead}")
    D = e // H
    pe = f64("pos_encoder.pe").reshape(-1, e)[:MAX_LEN].contiguous()
    layers, nhid = _fold_layers(weights, LAYER, LAYER_NAMES, True, e, D)
    return {"ninp": e, "nhead": H, "nhid": nhid, "nlayers": len(layers), "table": table, "pe": pe,
            "scale": float(np.float32(math.sqrt(e))), "layers": layers}


def split_chunks(ptr, chunk_rows):
    """Sequence ranges ``[(s0, s1)]`` of whole sequences with at most ``chunk_rows`` packed rows each (in order)."""
    out, s0, B = [], 0, len(ptr) - 1
    while s0 < B:
        s1 = int(np.searchsorted(ptr, int(ptr[s0]) + chunk_rows, side="right")) - 1
        s1 = min(max(s1, s0 + 1), B)
        out.append((s0, s1))
        s0 = s1
    return out


class _PackedEncoder:
    """What the two encoders on packed token rows share: the launches of a post-norm transformer layer.  A subclass sets
    ``device``, ``gemm``, ``eps``, ``ninp``, ``nhead`` and ``layers`` (the per-layer dicts of ``text_fold_weights``, uploaded
    with ``_upload_layers``)."""

    def _gemm_weight(self, t):
        """A GEMM's weight on the device as ``_linear`` takes it: float32, or under ``gemm="bf16"`` its bfloat16 rounding
        (``sss_f32_to_bf16``, round to nearest even), converted once; the float32 upload is not kept."""
        import torch
        from . import _lib
        from ._device import upload_f32
        w = upload_f32(t, self.device)
        if self.gemm == "f32":
            return w
        wb = torch.empty(w.shape, dtype=torch.bfloat16, device=self.device)       # K is a multiple of 32: whole groups of 8
        _lib.check(_lib.lib().sss_f32_to_bf16(w.data_ptr(), w.numel(), wb.data_ptr(), _lib.stream_ptr(self.device)), "sss_f32_to_bf16")
        return wb

    def _upload_layers(self, layers):
        from ._device import upload_f32
        return [{n: self._gemm_weight(v) if n in GEMM_WEIGHTS else upload_f32(v, self.device) for n, v in lay.items()} for lay in layers]

    def _linear(self, x, w, b, y, n, act=0):
        """The one place that picks a GEMM's entry point: every dense layer of the instance goes the same way."""
        from . import _lib
        arr = (_lib.LinearProblem * 1)(_lib.linear_problem(x, w, b, y, n, w.shape[0], act))
        name = "sss_linear_grouped" if self.gemm == "f32" else "sss_linear_grouped_bf16"
        _lib.check(getattr(_lib.lib(), name)(arr, 1, w.shape[1], _lib.stream_ptr(self.device)), name)

    def _add_layernorm(self, x, res, gamma, beta, n):
        from . import _lib
        rc = _lib.lib().sss_add_layernorm(x.data_ptr(), x.stride(0), res.data_ptr(), res.stride(0), gamma.data_ptr(), beta.data_ptr(),
                                          self.eps, n, self.ninp, x.data_ptr(), x.stride(0), _lib.stream_ptr(self.device))
        _lib.check(rc, "sss_add_layernorm")

    def _run_layers(self, x, qkv, att, proj, hid, ptr, key_ok, n, n_seq, T, act):
        """Every layer on the ``n`` packed rows of ``x`` (in place): 7 launches each; ``act`` is the feed-forward block's."""
        from . import _lib
        args = _lib.SeqAttentionArgs(qkv=qkv.data_ptr(), ld_qkv=qkv.stride(0), ptr=ptr.data_ptr(), key_ok=key_ok.data_ptr(),
                                     n_rows=n, n_seq=n_seq, heads=self.nhead, head_dim=self.ninp // self.nhead, max_len=T,
                                     out=att.data_ptr(), ld_out=att.stride(0))
        L, st = _lib.lib(), _lib.stream_ptr(self.device)
        for lay in self.layers:
            self._linear(x, lay["in_w"], lay["in_b"], qkv, n)
            _lib.check(L.sss_seq_attention(ctypes.byref(args), st), "sss_seq_attention")
            self._linear(att, lay["out_w"], lay["out_b"], proj, n)
            self._add_layernorm(x, proj, lay["n1_w"], lay["n1_b"], n)
            self._linear(x, lay["l1_w"], lay["l1_b"], hid, n, act=act)
            self._linear(hid, lay["l2_w"], lay["l2_b"], proj, n)
            self._add_layernorm(x, proj, lay["n2_w"], lay["n2_b"], n)

    def _encode(self, rows, embed, act, pool_w, out, err_msg, extra=None, tokens=None):
        """The chunk walk over packed ``rows`` (``TokenRows``, at least one sequence), whole sequences of at most
        ``self.chunk_rows`` rows at a time: ``embed(tok, pos, extra, n, x, err)`` launches the subclass's embedding of the
        chunk's ``n`` rows into ``x`` (``extra``: its slice of that host array, uploaded), then every layer, then
        ``out[s] = sum_r pool_w[r] x[r]`` over the rows of sequence ``s`` -- ``pool_w`` one float for all rows or a host float32
        array.  ``tokens`` (``[B * T, e]``, every sequence kept all ``T`` rows) also receives the rows.  ``err`` (int32 [1], set
        by the embedding kernel on an index out of range) is read once, at the end: ``IndexError(err_msg)``."""
        import torch
        from . import _lib
        e, dev, T = self.ninp, self.device, rows.T
        L, st = _lib.lib(), _lib.stream_ptr(dev)
        chunks = split_chunks(rows.ptr, self.chunk_rows)
        cap = max(int(rows.ptr[s1] - rows.ptr[s0]) for s0, s1 in chunks)
        K, Hp = self.layers[0]["in_w"].shape[1], self.layers[0]["l1_w"].shape[0]
        buf = lambda width: torch.empty((cap, width), dtype=torch.float32, device=dev)
        x, qkv, att, proj, hid = buf(K), buf(3 * e), buf(K), buf(e), buf(Hp)
        same_w = None if isinstance(pool_w, np.ndarray) else torch.full((cap,), pool_w, dtype=torch.float32, device=dev)
        err = torch.zeros(1, dtype=torch.int32, device=dev)
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        for s0, s1 in chunks:
            r0, r1 = int(rows.ptr[s0]), int(rows.ptr[s1])
            n = r1 - r0
            tok, pos, key_ok = up(rows.tok[r0:r1]), up(rows.pos[r0:r1]), up(rows.key_ok[r0:r1])
            w = up(pool_w[r0:r1]) if same_w is None else same_w
            ptr = up(rows.ptr[s0:s1 + 1] - np.int32(r0))
            embed(tok, pos, None if extra is None else up(extra[r0:r1]), n, x, err)
            self._run_layers(x, qkv, att, proj, hid, ptr, key_ok, n, s1 - s0, T, act)
            rc = L.sss_segment_reduce(x.data_ptr(), x.stride(0), w.data_ptr(), ptr.data_ptr(), s1 - s0, e, 1, out[s0:s1].data_ptr(),
                                      out.stride(0), st)
            _lib.check(rc, "sss_segment_reduce")
            if tokens is not None:
                tokens[s0 * T:s1 * T].copy_(x[:n, :e])
        if int(err.item()):                                                  # one read per forward
            raise IndexError(err_msg)


class NodeTextTransformer(_PackedEncoder):
    """Drop-in for the reference's ``NodeTextTransformer`` in eval mode: ``forward(src [B, T], mask [B, T]) -> [B, ninp]``
    float32 on the device -- ``x_q`` of ``variants.HGT.forward``, or ``data['query'].feat`` of ``SessionEncoder``.

    ``weights``: flat ``{name: tensor}`` under the module's own ``state_dict()`` names (``embedding.weight``,
    ``pos_encoder.pe``, ``transformer_encoder.layers.{l}.self_attn.in_proj_weight`` / ``in_proj_bias`` /
    ``out_proj.weight`` / ``.bias``, ``linear1``, ``linear2``, ``norm1``, ``norm2``).  ``pad_rule``: see the module
    docstring.  ``eps``: the LayerNorms' (torch's default 1e-5, which the reference keeps).

    The batch is walked in chunks of whole sequences of at most ``chunk_rows`` packed rows, so a corpus of millions of query
    nodes never needs ``rows x nhid`` floats at once.  The default, 131072 rows, keeps the widest buffer (``rows x nhid``)
    at 0.42 GB at the reference's ``nhid = 800`` and all five row buffers together near 1.1 GB.

    ``gemm="bf16"`` (default ``"f32"``, exact): the four GEMMs of a layer round both operands to bfloat16 and sum in float32
    on the bf16 matrix cores; per GEMM ``|v - (s + bias)| <= K 2^-23 sum|x^ w^| + 2^-23 |s + bias|`` around the exact sum ``s``
    of the rounded operands (include/lowp/sss_linear_bf16.h; bf16 subnormals not covered), no pointwise bound per forward.

    Limits: ``ninp % 4 == 0``, ``ninp <= 1024``, head width ``ninp / nhead <= 64``, ``T <= 64``."""

    def __init__(self, weights, nhead, pad_rule="compute", device=None, chunk_rows=131072, eps=1e-5, gemm="f32"):
        from ._device import model_device, upload_f32
        _check_rule(pad_rule)
        _check_gemm(gemm)
        f = text_fold_weights(weights, nhead)                                # raises ValueError when nhead does not divide ninp
        e = f["ninp"]
        if e % 4 or e > 1024 or e // f["nhead"] > 64:
            raise ValueError(f"NodeTextTransformer needs ninp % 4 == 0, ninp <= 1024 and ninp / nhead <= 64; got ninp = {e}, nhead = {nhead}")
        if int(chunk_rows) < MAX_LEN:
            raise ValueError(f"chunk_rows must be at least {MAX_LEN} (one whole sequence), got {chunk_rows}")
        self.pad_rule, self.chunk_rows, self.eps = pad_rule, int(chunk_rows), float(eps)
        self.ninp, self.nhead, self.nhid, self.nlayers = e, f["nhead"], f["nhid"], f["nlayers"]
        self.ntoken, self.scale = int(f["table"].shape[0]), f["scale"]
        self.device, self.gemm = model_device(device), gemm
        d = lambda t: upload_f32(t, self.device)
        self.table, self.pe = d(f["table"]), d(f["pe"])
        self.layers = self._upload_layers(f["layers"])

    @classmethod
    def from_torch(cls, module, **kw):
        """From a live reference ``NodeTextTransformer`` (or any module with its ``state_dict()`` names); ``nhead`` is read
        from the first encoder layer."""
        nhead = module.transformer_encoder.layers[0].self_attn.num_heads
        eps = module.transformer_encoder.layers[0].norm1.eps
        return cls({k: v for k, v in module.state_dict().items()}, nhead, eps=eps, **kw)

    def forward(self, src, mask):
        import torch
        from . import _lib
        rows = pack_tokens(src, mask, self.pad_rule, self.ntoken)
        B, T, e, dev = len(rows.ptr) - 1, rows.T, self.ninp, self.device
        if T > self.pe.shape[0]:
            raise ValueError(f"T = {T} positions, the positional table has {self.pe.shape[0]}")
        with torch.no_grad():
            out = torch.empty((B, e), dtype=torch.float32, device=dev)
            if B == 0:
                return out
            L, st = _lib.lib(), _lib.stream_ptr(dev)

            def embed(tok, pos, _, n, x, err):
                rc = L.sss_text_embed(self.table.data_ptr(), self.ntoken, self.pe.data_ptr(), self.pe.shape[0], tok.data_ptr(),
                                      pos.data_ptr(), n, e, self.scale, x.data_ptr(), x.stride(0), err.data_ptr(), st)
                _lib.check(rc, "sss_text_embed")

            self._encode(rows, embed, 1, 1.0 / T, out,          # relu in the feed-forward block; the mean divides by the padded length
                         "a token id or position was out of range on the device (sss_text_embed wrote zero rows)")
        return out

    __call__ = forward


# --------------------------------------------------------------------------------------------------------------------------
# The node text encoder of the deployed model: PretrainedQAEAEncoder (model/NodeEmbedding.py:100-125), a BERT encoder without
# its pooling layer + a masked mean over the tokens + an optional Linear.  DESIGN.md section 5.10.
BERT_LAYER = "encoder.layer.{}."
BERT_LAYER_NAMES = {"in_w": tuple(f"attention.self.{n}.weight" for n in ("query", "key", "value")),
                    "in_b": tuple(f"attention.self.{n}.bias" for n in ("query", "key", "value")),
                    "out_w": "attention.output.dense.weight", "out_b": "attention.output.dense.bias",
                    "l1_w": "intermediate.dense.weight", "l1_b": "intermediate.dense.bias", "l2_w": "output.dense.weight",
                    "l2_b": "output.dense.bias", "n1_w": "attention.output.LayerNorm.weight", "n1_b": "attention.output.LayerNorm.bias",
                    "n2_w": "output.LayerNorm.weight", "n2_b": "output.LayerNorm.bias"}
BERT_POOLS = ("masked", "mean")

BertRows = namedtuple("BertRows", "rows tt w")
BertRows.__doc__ = """Packed rows of a BERT batch: ``rows`` the ``TokenRows`` (``tok`` = input id, ``pos`` = index in the padded row,
``key_ok`` = attention mask), ``tt`` int32 [n] the token type of each row, ``w`` float32 [n] the weight of each row in its
sequence's pooled sum (``1 / len`` on attended rows and 0 elsewhere for ``"masked"``, ``1 / T`` for ``"mean"``)."""


def bert_pack_rows(input_ids, token_type_ids, attention_mask, pool="masked", all_rows=False, n_word=None, n_type=None):
    """``[B, T]`` ids, token types and attention mask (non-zero = attended) -> ``BertRows``.

    Under ``pool="masked"`` without ``all_rows`` the padded rows are dropped: they are neither keys nor pooled, so the valid
    rows and the pooled output are exactly what they are with them.  Under ``pool="mean"`` or ``all_rows`` (``get_token``)
    every one of the ``T`` rows is kept; a padded row attends over the valid keys only and is never a key (HF's additive
    mask).  Raises as ``pack_tokens`` does, and ``IndexError`` for a token type outside ``[0, n_type)``."""
    if pool not in BERT_POOLS:
        raise ValueError(f"pool must be 'masked' or 'mean', got {pool!r}")
    ids, tt, am = _host(input_ids), _host(token_type_ids), _host(attention_mask)
    if tt.shape != ids.shape or am.shape != ids.shape:
        raise ValueError(f"input_ids, token_type_ids and attention_mask must share one [B, T] shape; got {ids.shape}, {tt.shape}, {am.shape}")
    if not np.issubdtype(tt.dtype, np.integer):
        raise ValueError(f"token_type_ids must hold integers, got dtype {tt.dtype}")
    pad = am == 0
    keep_all = pool == "mean" or all_rows
    rows = pack_tokens(ids, pad, "compute" if keep_all else "zero", n_word)
    if n_type is not None and tt.size and (int(tt.min()) < 0 or int(tt.max()) >= n_type):
        raise IndexError(f"token type out of range [0, {n_type})")
    B, T = ids.shape
    counts = np.diff(rows.ptr)
    b = np.repeat(np.arange(B), counts)
    if pool == "mean":
        w = np.full(len(b), 1.0 / T if T else 0.0, dtype=np.float32)
    else:
        w = (np.float32(1.0) / (~pad).sum(axis=1).astype(np.float32))[b] * rows.key_ok.astype(np.float32)
    return BertRows(rows, tt[b, rows.pos].astype(np.int32), w.astype(np.float32))


def unique_rows(ids, tt, am):
    """``(first int64 [U], inverse int64 [B])`` of the distinct ``(ids, types, mask)`` rows of ``[B, T]`` integer arrays whose
    values fit int32: ``first`` indexes one representative of each, ``row b == row first[inverse[b]]``.  One ``np.unique``
    over the rows as byte strings (int32 ids and types, uint8 mask: 9 bytes per position), four times as fast as ``axis=0``
    over int64 columns; the order of the distinct rows is the byte order, which no result depends on."""
    key = np.concatenate([ids.astype(np.int32), tt.astype(np.int32)], axis=1).view(np.uint8)
    key = np.ascontiguousarray(np.concatenate([key, (am != 0).astype(np.uint8)], axis=1))
    _, first, inverse = np.unique(key.view(np.dtype((np.void, key.shape[1]))).reshape(-1), return_index=True, return_inverse=True)
    return first.astype(np.int64), inverse.reshape(-1).astype(np.int64)


def bert_fold_weights(weights, num_heads):
    """Host-side, device-free, float64: the weights of a ``BertModel`` without its pooling layer (HF's own ``state_dict()``
    names) as the kernels take them, after ``text_fold_weights``: ``query | key | value`` become one ``in_w [3 e, K]`` with
    ``1 / sqrt(D)`` folded into the q rows and bias, every GEMM's K is padded with zero columns to a multiple of 32, and
    ``intermediate.dense`` with zero rows and zero bias to ``pad32(inter)`` outputs: ``gelu(0) = 0``, so the pad columns
    ``output.dense`` reads are exact zeros.  Optional ``lin.weight`` / ``lin.bias`` (the reference's ``Linear(768, nout)``).

    Returns ``{"e", "heads", "inter", "nlayers", "word" [n_word, e], "pos" [n_pos, e], "type" [n_type, e], "emb_g", "emb_b",
    "layers": [the keys of text_fold_weights], "lin_w" [nout, K] or None, "lin_b"}`` with ``K = pad32(e)``."""
    import torch
    f64 = lambda name: weights[name].detach().to("cpu", torch.float64)
    word = f64("embeddings.word_embeddings.weight")
    e, H = int(word.shape[1]), int(num_heads)
    if H < 1 or e % H:
        raise ValueError(f"hidden size {e} is not a multiple of num_heads = {num_heads}")
    D = e // H
    layers, inter = _fold_layers(weights, BERT_LAYER, BERT_LAYER_NAMES, False, e, D)
    lin_w = lin_b = None
    if "lin.weight" in weights:
        lin_w = _pad(f64("lin.weight"), int(weights["lin.weight"].shape[0]), _pad32(e))
        lin_b = f64("lin.bias") if "lin.bias" in weights else torch.zeros(lin_w.shape[0], dtype=torch.float64)
    return {"e": e, "heads": H, "inter": inter, "nlayers": len(layers), "word": word, "pos": f64("embeddings.position_embeddings.weight"),
            "type": f64("embeddings.token_type_embeddings.weight"), "emb_g": f64("embeddings.LayerNorm.weight"),
            "emb_b": f64("embeddings.LayerNorm.bias"), "layers": layers, "lin_w": lin_w, "lin_b": lin_b}


class BertNodeEncoder(_PackedEncoder):
    """Drop-in for the reference's ``PretrainedQAEAEncoder``: ``enc(input_ids, token_type_ids, attention_mask, get_token=False)``
    -> ``[B, e]`` (``[B, nout]`` with a ``lin`` head) float32 on the device, the pooled ``last_hidden_state`` of a BERT encoder
    without its pooling layer -- ``data['query'].feat`` / ``data['product'].feat`` of ``SessionEncoder``.  With
    ``get_token=True`` it also returns ``last_hidden_state [B, T, e]``.

    ``weights``: flat ``{name: tensor}`` under HF's own ``state_dict()`` names (``embeddings.word_embeddings.weight``,
    ``embeddings.position_embeddings.weight``, ``embeddings.token_type_embeddings.weight``, ``embeddings.LayerNorm.*``,
    ``encoder.layer.{l}.attention.self.query|key|value.*``, ``attention.output.dense|LayerNorm.*``, ``intermediate.dense.*``,
    ``output.dense|LayerNorm.*``), optionally ``lin.weight`` / ``lin.bias``.  ``pool``: ``"masked"`` is the reference's
    ``sum(token_emb * mask) / sum(mask)``, ``"mean"`` the plain ``mean(dim=1)`` of ``main2('QAEA')``.  ``hidden_act`` and
    ``position_embedding_type`` are the config's, taken only to be refused when the kernels do not compute them.

    ``dedup``: identical ``(ids, types, mask)`` rows are encoded once (host ``np.unique``) and scattered with
    ``sss_gather_rows``; the result is bit-equal with it on and off.  The unique sequences are walked in chunks of whole
    sequences of at most ``chunk_rows`` packed rows.  The default, 32768 rows, keeps the widest buffer (``rows x 3072`` floats
    at bert-base) at 0.40 GB and the five row buffers together (``rows x 7680`` floats) at 1.0 GB; the result does not
    depend on it.

    ``gemm="bf16"`` (default ``"f32"``, exact): every GEMM, the ``lin`` head included, rounds both operands to bfloat16 and sums
    in float32 on the bf16 matrix cores; only the bf16 copy of those weights is kept.  Per GEMM ``|v - (s + bias)| <=
    K 2^-23 sum|x^ w^| + 2^-23 |s + bias|`` around the exact sum ``s`` of the rounded operands (include/lowp/sss_linear_bf16.h;
    bf16 subnormals not covered); no pointwise bound per forward.

    Limits: ``e % 4 == 0``, ``e <= 1024``, head width ``e / num_heads <= 64``, ``T <= 64`` and ``<= max_position_embeddings``.
    The three inputs are what ``wordpiece.WordPieceTokenizer`` returns (``enc(*tokens)``).  Not here: ELECTRA's
    ``embeddings_project``, relative position embeddings."""

    def __init__(self, weights, num_heads, pool="masked", eps=1e-12, device=None, chunk_rows=32768, dedup=True, hidden_act="gelu",
                 position_embedding_type="absolute", gemm="f32"):
        from ._device import model_device, upload_f32
        _check_gemm(gemm)
        if pool not in BERT_POOLS:
            raise ValueError(f"pool must be 'masked' or 'mean', got {pool!r}")
        if hidden_act != "gelu":
            raise ValueError(f"hidden_act must be 'gelu' (the exact erf GELU), got {hidden_act!r}")
        if position_embedding_type not in (None, "absolute"):
            raise ValueError(f"position embeddings must be absolute, got {position_embedding_type!r}")
        if "embeddings_project.weight" in weights:
            raise ValueError("an embeddings_project (ELECTRA with embedding_size != hidden_size) is not supported")
        e = int(weights["embeddings.word_embeddings.weight"].shape[1])
        if int(num_heads) < 1 or e % int(num_heads) or e % 4 or e > 1024 or e // int(num_heads) > 64:
            raise ValueError(f"BertNodeEncoder needs e % 4 == 0, e <= 1024, e a multiple of num_heads and e / num_heads <= 64; "
                             f"got e = {e}, num_heads = {num_heads}")
        if int(chunk_rows) < MAX_LEN:
            raise ValueError(f"chunk_rows must be at least {MAX_LEN} (one whole sequence), got {chunk_rows}")
        if not float(eps) > 0.0:
            raise ValueError(f"eps must be positive, got {eps}")
        f = bert_fold_weights(weights, num_heads)
        self.pool, self.chunk_rows, self.eps, self.dedup = pool, int(chunk_rows), float(eps), bool(dedup)
        self.ninp, self.nhead, self.inter, self.nlayers = e, f["heads"], f["inter"], f["nlayers"]
        self.n_word, self.n_pos, self.n_type = int(f["word"].shape[0]), int(f["pos"].shape[0]), int(f["type"].shape[0])
        self.device, self.gemm = model_device(device), gemm
        d = lambda t: upload_f32(t, self.device)
        self.word, self.pos, self.type, self.emb_g, self.emb_b = (d(f[n]) for n in ("word", "pos", "type", "emb_g", "emb_b"))
        self.layers = self._upload_layers(f["layers"])
        self.lin_w, self.lin_b = (None, None) if f["lin_w"] is None else (self._gemm_weight(f["lin_w"]), d(f["lin_b"]))
        self.nout = e if self.lin_w is None else int(self.lin_w.shape[0])

    @classmethod
    def from_transformers(cls, model, lin=None, **kw):
        """From a live ``transformers.BertModel(config, add_pooling_layer=False)`` and, optionally, the ``nn.Linear`` head;
        ``num_attention_heads``, ``layer_norm_eps``, ``hidden_act`` and the position embedding type are read from its config."""
        cfg = model.config
        w = {k: v for k, v in model.state_dict().items()}
        if lin is not None:
            w["lin.weight"] = lin.weight
            if lin.bias is not None:
                w["lin.bias"] = lin.bias
        kw.setdefault("eps", cfg.layer_norm_eps)
        return cls(w, cfg.num_attention_heads, hidden_act=cfg.hidden_act,
                   position_embedding_type=getattr(cfg, "position_embedding_type", None), **kw)

    def forward(self, input_ids, token_type_ids, attention_mask, get_token=False):
        import torch
        from . import _lib
        ids, tt, am = _host(input_ids), _host(token_type_ids), _host(attention_mask)
        if ids.ndim != 2 or tt.shape != ids.shape or am.shape != ids.shape:
            raise ValueError(f"input_ids, token_type_ids and attention_mask must share one [B, T] shape; got {ids.shape}, {tt.shape}, {am.shape}")
        B, T = ids.shape
        if T > MAX_LEN or T > self.n_pos:
            raise ValueError(f"T = {T} positions: at most {min(MAX_LEN, self.n_pos)} are supported (the attention kernel takes {MAX_LEN}, "
                             f"the position table has {self.n_pos})")
        am = (am != 0).astype(np.uint8)
        inv = None
        if self.dedup and B > 1:                                             # encode each distinct (ids, types, mask) row once
            for a, hi, what in ((ids, self.n_word, "token id"), (tt, self.n_type, "token type")):     # before int32 can alias an id
                if a.size and (not np.issubdtype(a.dtype, np.integer) or int(a.min()) < 0 or int(a.max()) >= hi):
                    raise IndexError(f"{what} out of range [0, {hi}) (or not an integer)")
            first, inverse = unique_rows(ids, tt, am)
            if len(first) < B:
                ids, tt, am, inv = ids[first], tt[first], am[first], inverse
        packed = bert_pack_rows(ids, tt, am, self.pool, get_token, self.n_word, self.n_type)
        rows = packed.rows
        U, e, dev = len(rows.ptr) - 1, self.ninp, self.device
        with torch.no_grad():
            L, st = _lib.lib(), _lib.stream_ptr(dev)
            K = self.layers[0]["in_w"].shape[1]
            pooled = torch.zeros((U, K), dtype=torch.float32, device=dev)     # pad columns stay zero: the lin head's K operand
            tokens = torch.empty((U * T, e), dtype=torch.float32, device=dev) if get_token else None
            if U:
                def embed(tok, pos, typ, n, x, err):
                    rc = L.sss_bert_embed(self.word.data_ptr(), self.n_word, self.type.data_ptr(), self.n_type, self.pos.data_ptr(),
                                          self.n_pos, tok.data_ptr(), typ.data_ptr(), pos.data_ptr(), self.emb_g.data_ptr(),
                                          self.emb_b.data_ptr(), self.eps, n, e, x.data_ptr(), x.stride(0), err.data_ptr(), st)
                    _lib.check(rc, "sss_bert_embed")

                self._encode(rows, embed, 5, packed.w, pooled, "a token id, token type or position was out of range on the device "
                             "(sss_bert_embed wrote zero rows)", extra=packed.tt, tokens=tokens)      # 5: the exact GELU
            if inv is not None:                                              # scatter the distinct rows back to the batch
                d_inv = torch.from_numpy(inv).to(dev)
                full = torch.zeros((B, K), dtype=torch.float32, device=dev)
                _lib.check(L.sss_gather_rows(pooled.data_ptr(), d_inv.data_ptr(), B, K, full.data_ptr(), K, st), "sss_gather_rows")
                pooled = full
                if get_token:
                    t_ids = torch.from_numpy((inv[:, None] * T + np.arange(T)[None, :]).reshape(-1)).to(dev)
                    full_t = torch.empty((B * T, e), dtype=torch.float32, device=dev)
                    _lib.check(L.sss_gather_rows(tokens.data_ptr(), t_ids.data_ptr(), B * T, e, full_t.data_ptr(), e, st), "sss_gather_rows")
                    tokens = full_t
            if self.lin_w is not None:
                out = torch.empty((B, self.nout), dtype=torch.float32, device=dev)
                if B:
                    self._linear(pooled, self.lin_w, self.lin_b, out, B)
            else:
                out = pooled[:, :e] if K == e else pooled[:, :e].contiguous()
        return (out, tokens.view(B, T, e)) if get_token else out

    __call__ = forward
