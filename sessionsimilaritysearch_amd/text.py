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
(include/sss_text.h), ``sss_linear_grouped`` for the four GEMMs of a layer and ``sss_segment_reduce`` for the pooling;
torch owns memory only.  A layer is 7 launches, a forward ``7 * nlayers + 2`` per chunk of rows.
"""
from __future__ import annotations

import ctypes
import math
from collections import namedtuple

import numpy as np

MAX_LEN = 64                                 # rows per sequence sss_seq_attention takes: one lane per query row
PAD_RULES = ("compute", "zero")

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


def _pad32(n):
    return (n + 31) // 32 * 32


LAYER = "transformer_encoder.layers.{}."


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
    nlayers = 0
    while LAYER.format(nlayers) + "self_attn.in_proj_weight" in weights:
        nlayers += 1
    if nlayers == 0:
        raise ValueError("weights hold no transformer_encoder.layers.0.self_attn.in_proj_weight")
    nhid = int(weights[LAYER.format(0) + "linear1.weight"].shape[0])
    K, Hp = _pad32(e), _pad32(nhid)

    def pad(w, rows, cols):
        out = torch.zeros((rows, cols), dtype=torch.float64)
        out[:w.shape[0], :w.shape[1]] = w
        return out

    layers = []
    for l in range(nlayers):
        g = lambda n: f64(LAYER.format(l) + n)
        in_w, in_b = g("self_attn.in_proj_weight").clone(), g("self_attn.in_proj_bias").clone()
        in_w[:e] /= math.sqrt(D)
        in_b[:e] /= math.sqrt(D)
        l1_b = torch.zeros(Hp, dtype=torch.float64)
        l1_b[:nhid] = g("linear1.bias")
        layers.append({"in_w": pad(in_w, 3 * e, K), "in_b": in_b, "out_w": pad(g("self_attn.out_proj.weight"), e, K),
                       "out_b": g("self_attn.out_proj.bias"), "l1_w": pad(g("linear1.weight"), Hp, K), "l1_b": l1_b,
                       "l2_w": pad(g("linear2.weight"), e, Hp), "l2_b": g("linear2.bias"), "n1_w": g("norm1.weight"),
                       "n1_b": g("norm1.bias"), "n2_w": g("norm2.weight"), "n2_b": g("norm2.bias")})
    return {"ninp": e, "nhead": H, "nhid": nhid, "nlayers": nlayers, "table": table, "pe": pe,
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


class NodeTextTransformer:
    """Drop-in for the reference's ``NodeTextTransformer`` in eval mode: ``forward(src [B, T], mask [B, T]) -> [B, ninp]``
    float32 on the device -- ``x_q`` of ``variants.HGT.forward``, or ``data['query'].feat`` of ``SessionEncoder``.

    ``weights``: flat ``{name: tensor}`` under the module's own ``state_dict()`` names (``embedding.weight``,
    ``pos_encoder.pe``, ``transformer_encoder.layers.{l}.self_attn.in_proj_weight`` / ``in_proj_bias`` /
    ``out_proj.weight`` / ``.bias``, ``linear1``, ``linear2``, ``norm1``, ``norm2``).  ``pad_rule``: see the module
    docstring.  ``eps``: the LayerNorms' (torch's default 1e-5, which the reference keeps).

    The batch is walked in chunks of whole sequences of at most ``chunk_rows`` packed rows, so a corpus of millions of query
    nodes never needs ``rows x nhid`` floats at once.  The default, 131072 rows, keeps the widest buffer (``rows x nhid``)
    at 0.42 GB at the reference's ``nhid = 800`` and all five row buffers together near 1.1 GB.

    Limits: ``ninp % 4 == 0``, ``ninp <= 1024``, head width ``ninp / nhead <= 64``, ``T <= 64``."""

    def __init__(self, weights, nhead, pad_rule="compute", device=None, chunk_rows=131072, eps=1e-5):
        import torch
        _check_rule(pad_rule)
        f = text_fold_weights(weights, nhead)                                # raises ValueError when nhead does not divide ninp
        e = f["ninp"]
        if e % 4 or e > 1024 or e // f["nhead"] > 64:
            raise ValueError(f"NodeTextTransformer needs ninp % 4 == 0, ninp <= 1024 and ninp / nhead <= 64; got ninp = {e}, nhead = {nhead}")
        if int(chunk_rows) < MAX_LEN:
            raise ValueError(f"chunk_rows must be at least {MAX_LEN} (one whole sequence), got {chunk_rows}")
        self.pad_rule, self.chunk_rows, self.eps = pad_rule, int(chunk_rows), float(eps)
        self.ninp, self.nhead, self.nhid, self.nlayers = e, f["nhead"], f["nhid"], f["nlayers"]
        self.ntoken, self.scale = int(f["table"].shape[0]), f["scale"]
        self.device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        d = lambda t: t.to(device=self.device, dtype=torch.float32).contiguous()
        self.table, self.pe = d(f["table"]), d(f["pe"])
        self.layers = [{n: d(v) for n, v in lay.items()} for lay in f["layers"]]

    @classmethod
    def from_torch(cls, module, **kw):
        """From a live reference ``NodeTextTransformer`` (or any module with its ``state_dict()`` names); ``nhead`` is read
        from the first encoder layer."""
        nhead = module.transformer_encoder.layers[0].self_attn.num_heads
        eps = module.transformer_encoder.layers[0].norm1.eps
        return cls({k: v for k, v in module.state_dict().items()}, nhead, eps=eps, **kw)

    def _linear(self, x, w, b, y, n, act=0):
        from . import _lib
        from .variants import _prob
        arr = (_lib.LinearProblem * 1)(_prob(x, w, b, y, n, w.shape[0], act))
        _lib.check(_lib.lib().sss_linear_grouped(arr, 1, w.shape[1], _lib.stream_ptr(self.device)), "sss_linear_grouped")

    def _add_layernorm(self, x, res, gamma, beta, n):
        from . import _lib
        rc = _lib.lib().sss_add_layernorm(x.data_ptr(), x.stride(0), res.data_ptr(), res.stride(0), gamma.data_ptr(), beta.data_ptr(),
                                          self.eps, n, self.ninp, x.data_ptr(), x.stride(0), _lib.stream_ptr(self.device))
        _lib.check(rc, "sss_add_layernorm")

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
            chunks = split_chunks(rows.ptr, self.chunk_rows)
            cap = max(int(rows.ptr[s1] - rows.ptr[s0]) for s0, s1 in chunks)
            K, Hp = self.layers[0]["in_w"].shape[1], self.layers[0]["l1_w"].shape[0]
            buf = lambda width: torch.empty((cap, width), dtype=torch.float32, device=dev)
            x, qkv, att, proj, hid = buf(K), buf(3 * e), buf(K), buf(e), buf(Hp)
            inv_t = torch.full((cap,), 1.0 / T, dtype=torch.float32, device=dev)       # the mean divides by the padded length
            err = torch.zeros(1, dtype=torch.int32, device=dev)
            for s0, s1 in chunks:
                r0, r1 = int(rows.ptr[s0]), int(rows.ptr[s1])
                n = r1 - r0
                up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
                tok, pos, key_ok = up(rows.tok[r0:r1]), up(rows.pos[r0:r1]), up(rows.key_ok[r0:r1])
                ptr = up(rows.ptr[s0:s1 + 1] - np.int32(r0))
                rc = L.sss_text_embed(self.table.data_ptr(), self.ntoken, self.pe.data_ptr(), self.pe.shape[0], tok.data_ptr(),
                                      pos.data_ptr(), n, e, self.scale, x.data_ptr(), x.stride(0), err.data_ptr(), st)
                _lib.check(rc, "sss_text_embed")
                args = _lib.SeqAttentionArgs(qkv=qkv.data_ptr(), ld_qkv=qkv.stride(0), ptr=ptr.data_ptr(), key_ok=key_ok.data_ptr(),
                                             n_rows=n, n_seq=s1 - s0, heads=self.nhead, head_dim=e // self.nhead, max_len=T,
                                             out=att.data_ptr(), ld_out=att.stride(0))
                for lay in self.layers:
                    self._linear(x, lay["in_w"], lay["in_b"], qkv, n)
                    _lib.check(L.sss_seq_attention(ctypes.byref(args), st), "sss_seq_attention")
                    self._linear(att, lay["out_w"], lay["out_b"], proj, n)
                    self._add_layernorm(x, proj, lay["n1_w"], lay["n1_b"], n)
                    self._linear(x, lay["l1_w"], lay["l1_b"], hid, n, act=1)
                    self._linear(hid, lay["l2_w"], lay["l2_b"], proj, n)
                    self._add_layernorm(x, proj, lay["n2_w"], lay["n2_b"], n)
                view = out[s0:s1]
                rc = L.sss_segment_reduce(x.data_ptr(), x.stride(0), inv_t.data_ptr(), ptr.data_ptr(), s1 - s0, e, 1,
                                          view.data_ptr(), out.stride(0), st)
                _lib.check(rc, "sss_segment_reduce")
            if int(err.item()):                                              # one read per forward
                raise IndexError("a token id or position was out of range on the device (sss_text_embed wrote zero rows)")
        return out

    __call__ = forward
