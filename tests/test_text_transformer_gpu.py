"""GPU side of the query text encoder: the three entry points of include/sss_text.h called through the C ABI at the shapes
where their lane maps can go wrong, and text.NodeTextTransformer end to end, all against the float64 helper of
tests/helpers/text_ref.py (and, for the fixture records, against the reference's own stored outputs)."""
import ctypes
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import text_ref as tr  # noqa: E402

from sessionsimilaritysearch_amd import _lib  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-5                                  # times max(1, max |ref|), the project's float32 kernel tolerance
_CACHE = {}


def _dev(a, cuda):
    return torch.from_numpy(np.ascontiguousarray(a)).to(cuda)


# ------------------------------------------------------------------------------------------------ sss_text_embed
@pytest.mark.parametrize("e,ld", [(200, 224), (4, 4), (4, 12)])
def test_embed_is_bit_equal_to_float32_numpy(cuda, e, ld):
    """table[tok] * float32(sqrt(e)) + pe[pos], a rounded product then a rounded sum; pad columns exact zeros over a poisoned
    buffer; one out-of-range id (and one out-of-range position) writes a zero row, sets err and leaves its neighbours right."""
    L, rng = _lib.lib(), np.random.default_rng(e + ld)
    ntoken, n_pos, n = 50, 20, 300                                     # 300 x 224 / 4 float4s: more than one workgroup
    table = rng.standard_normal((ntoken, e)).astype(np.float32)
    pe = tr.sinusoid(n_pos, e).astype(np.float32)
    scale = np.float32(math.sqrt(e))
    tok, pos = rng.integers(0, ntoken, n).astype(np.int64), rng.integers(0, n_pos, n).astype(np.int32)
    want = table[tok] * scale + pe[pos]
    assert want.dtype == np.float32
    d_table, d_pe = _dev(table, cuda), _dev(pe, cuda)

    def run(tok, pos):
        x = torch.full((n + 2, ld), float("nan"), dtype=torch.float32, device=cuda)
        err = torch.zeros(1, dtype=torch.int32, device=cuda)
        d_tok, d_pos = _dev(tok, cuda), _dev(pos, cuda)
        rc = L.sss_text_embed(d_table.data_ptr(), ntoken, d_pe.data_ptr(), n_pos, d_tok.data_ptr(), d_pos.data_ptr(), n, e,
                              float(scale), x.data_ptr(), ld, err.data_ptr(), _lib.stream_ptr(cuda))
        assert rc == 0, L.sss_last_error()
        x = x.cpu().numpy()
        assert np.isnan(x[n:]).all() and (x[:n, e:] == 0).all()
        return x[:n, :e], int(err.item())

    got, err = run(tok, pos)
    assert err == 0 and np.array_equal(got, want)
    for bad_tok, bad_pos in ((ntoken, None), (-1, None), (1 << 40, None), (None, n_pos), (None, -1)):
        t2, p2 = tok.copy(), pos.copy()
        if bad_tok is not None:
            t2[7] = bad_tok
        else:
            p2[7] = bad_pos
        got, err = run(t2, p2)
        assert err == 1 and (got[7] == 0).all() and np.array_equal(np.delete(got, 7, 0), np.delete(want, 7, 0))


# ------------------------------------------------------------------------------------------------ sss_seq_attention
LENS = [1, 2, 20, 63, 64, 3]                # packed back to back: a read across a ptr boundary changes a result


def attention_ref(q, k, v, ptr, key_ok, heads):
    """float64 loops: softmax with the maximum subtracted over the valid keys of the row's own sequence; none: zeros."""
    n, e = q.shape
    D = e // heads
    out = np.zeros((n, e))
    for s in range(len(ptr) - 1):
        rows = np.arange(ptr[s], ptr[s + 1])
        keys = rows[key_ok[rows] != 0]
        if len(keys) == 0:
            continue
        for h in range(heads):
            c = slice(h * D, (h + 1) * D)
            sc = q[rows][:, c] @ k[keys][:, c].T
            p = np.exp(sc - sc.max(1, keepdims=True))
            out[rows, c] = (p / p.sum(1, keepdims=True)) @ v[keys][:, c]
    return out


@pytest.mark.parametrize("heads,head_dim", [(4, 50), (4, 25), (2, 64), (8, 3), (1, 1)])
def test_seq_attention_matches_the_loops(cuda, heads, head_dim):
    """(4, 50): the reference; (4, 25): model.py's other width, the 32-wide instance with idle columns; (2, 64): the ceiling;
    (8, 3) and (1, 1): head widths below a float4.  Sequence 1 has its first key invalid, sequence 2 only its last key
    valid, sequence 5 none (zeros, no NaN); in sequence 3 head 0 has scores of +-80.  ld_qkv > 3 e and ld_out > e with
    poisoned padding and poisoned rows past the last."""
    L, rng = _lib.lib(), np.random.default_rng(100 * heads + head_dim)
    e = heads * head_dim
    ptr = np.concatenate([[0], np.cumsum(LENS)]).astype(np.int32)
    n = int(ptr[-1])
    sc = head_dim ** -0.25                                             # scores ~ N(0, 1)
    q, k, v = (rng.standard_normal((n, e)).astype(np.float32) * np.float32(sc) for _ in range(3))
    v = v / np.float32(sc)
    rows3 = slice(int(ptr[3]), int(ptr[4]))
    q[rows3, :head_dim] = 0.0
    q[rows3, 0] = 1.0                                                  # head 0 of sequence 3: the score is k's first column
    k[rows3, 0] = rng.choice([-80.0, 80.0], size=LENS[3]).astype(np.float32)
    k[int(ptr[3]), 0], k[int(ptr[3]) + 1, 0] = 80.0, -80.0
    key_ok = np.ones(n, dtype=np.uint8)
    key_ok[ptr[1]] = 0
    key_ok[ptr[2]:ptr[3] - 1] = 0
    key_ok[ptr[4]:ptr[5]] = rng.integers(0, 2, LENS[4])
    key_ok[ptr[4] + 5] = 1
    key_ok[ptr[5]:] = 0
    ref = attention_ref(q.astype(np.float64), k.astype(np.float64), v.astype(np.float64), ptr, key_ok, heads)
    ld_qkv, ld_out = 3 * e + 5, e + 7
    qkv = np.full((n + 2, ld_qkv), np.nan, dtype=np.float32)
    qkv[:n, :e], qkv[:n, e:2 * e], qkv[:n, 2 * e:3 * e] = q, k, v
    d_qkv, d_ptr, d_ok = _dev(qkv, cuda), _dev(ptr, cuda), _dev(key_ok, cuda)

    def run():
        out = torch.full((n + 3, ld_out), -7.0, dtype=torch.float32, device=cuda)
        args = _lib.SeqAttentionArgs(qkv=d_qkv.data_ptr(), ld_qkv=ld_qkv, ptr=d_ptr.data_ptr(), key_ok=d_ok.data_ptr(), n_rows=n,
                                     n_seq=len(LENS), heads=heads, head_dim=head_dim, max_len=64, out=out.data_ptr(), ld_out=ld_out)
        assert L.sss_seq_attention(ctypes.byref(args), _lib.stream_ptr(cuda)) == 0, L.sss_last_error()
        return out.cpu().numpy()

    out = run()
    assert np.isfinite(out).all()
    assert (out[n:] == -7.0).all() and (out[:n, e:] == 0.0).all()       # nothing past the last row; pad columns zeroed
    assert (out[ptr[5]:n, :e] == 0.0).all()                             # the sequence with no valid key
    err, bound = np.abs(out[:n, :e] - ref).max(), TOL * max(1.0, np.abs(ref).max())
    print(f"H={heads} D={head_dim}: max|err| = {err:.3e}, bound {bound:.3e}")
    assert err < bound
    # only the last key valid: every row of sequence 2 is that key's v row, exactly
    assert np.array_equal(out[ptr[2]:ptr[3], :e], np.broadcast_to(v[ptr[3] - 1], (LENS[2], e)))
    assert np.array_equal(run(), out)


def test_seq_attention_clamps_a_bad_ptr(cuda):
    """Row ranges past n_rows or longer than max_len are cut, never followed: nothing outside [0, n_rows) is touched."""
    L, rng = _lib.lib(), np.random.default_rng(8)
    heads, D, n = 2, 6, 30
    e = heads * D
    qkv = _dev(rng.standard_normal((n, 3 * e)).astype(np.float32), cuda)
    ptr = _dev(np.array([0, 25, 900], dtype=np.int32), cuda)           # 25 rows with max_len 20; a range that ends past n
    ok = torch.ones(n, dtype=torch.uint8, device=cuda)
    out = torch.full((n + 4, e), -7.0, dtype=torch.float32, device=cuda)
    args = _lib.SeqAttentionArgs(qkv=qkv.data_ptr(), ld_qkv=3 * e, ptr=ptr.data_ptr(), key_ok=ok.data_ptr(), n_rows=n, n_seq=2,
                                 heads=heads, head_dim=D, max_len=20, out=out.data_ptr(), ld_out=e)
    assert L.sss_seq_attention(ctypes.byref(args), _lib.stream_ptr(cuda)) == 0
    out = out.cpu().numpy()
    assert np.isfinite(out).all() and (out[n:] == -7.0).all() and (out[20:25] == -7.0).all() and (out[:20] != -7.0).all()


# ------------------------------------------------------------------------------------------------ sss_add_layernorm
@pytest.mark.parametrize("e,ld", [(4, 4), (200, 224), (1024, 1024)])
def test_add_layernorm(cuda, e, ld):
    """Row 0 holds one repeated value (variance 0: eps decides, the result is beta); row 1 is 1e4 + noise, where a one-pass
    E[x^2] - E[x]^2 in float32 has lost the variance altogether (x^2 = 1e8 is spaced 8 apart).  In place equals out of
    place bit for bit; pad columns are zeros.

    Bound per row: TOL * max(1, max |ref|) for the arithmetic after the mean, plus what the float32 mean can be off by --
    at most 16 roundings of partial sums no larger than the row's, 16 * 2^-24 * max |x + res| -- carried to the output,
    i.e. times max |gamma| / sqrt(var + eps).  That is a few 1e-5 on an O(1) row and about 3e-2 on the 1e4 row, where one
    pass is wrong by O(1)."""
    L, rng = _lib.lib(), np.random.default_rng(e)
    n, eps = 9, 1e-5                                                   # three workgroups of four rows, the last one ragged
    x = rng.standard_normal((n, e)).astype(np.float32) * 2
    res = rng.standard_normal((n, e)).astype(np.float32)
    x[0], res[0] = 3.25, 0.0
    x[1], res[1] = (1e4 + rng.uniform(-1, 1, e)).astype(np.float32), 0.0
    gamma, beta = (1 + 0.2 * rng.standard_normal(e)).astype(np.float32), rng.standard_normal(e).astype(np.float32)
    s = x.astype(np.float64) + res.astype(np.float64)
    ref = tr.layer_norm(s, gamma.astype(np.float64), beta.astype(np.float64), eps)
    bound = TOL * np.maximum(1.0, np.abs(ref).max(1)) + 16 * 2.0 ** -24 * np.abs(s).max(1) * np.abs(gamma).max() / np.sqrt(s.var(1) + eps)
    d_res, d_g, d_b = _dev(res, cuda), _dev(gamma, cuda), _dev(beta, cuda)
    xbuf = np.full((n + 1, ld), np.nan, dtype=np.float32)
    xbuf[:n, :e] = x

    def run(in_place):
        d_x = _dev(xbuf, cuda)
        y = d_x if in_place else torch.full((n + 1, ld), float("nan"), dtype=torch.float32, device=cuda)
        rc = L.sss_add_layernorm(d_x.data_ptr(), ld, d_res.data_ptr(), e, d_g.data_ptr(), d_b.data_ptr(), eps, n, e, y.data_ptr(), ld,
                                 _lib.stream_ptr(cuda))
        assert rc == 0, L.sss_last_error()
        if not in_place:
            assert np.array_equal(d_x.cpu().numpy(), xbuf, equal_nan=True)                # the input is left alone
        return y.cpu().numpy()

    out = run(False)
    assert np.isnan(out[n]).all() and (out[:n, e:] == 0.0).all()
    err = np.abs(out[:n, :e] - ref).max(1)
    print(f"e={e}: max|err| per row {np.array2string(err, precision=2)}; bound {np.array2string(bound, precision=2)}")
    assert (err <= bound).all()
    assert np.array_equal(out[0, :e], beta)
    assert np.array_equal(run(True), out, equal_nan=True)


# ------------------------------------------------------------------------------------------------ the drop-in
class TorchText(torch.nn.Module):
    """A plain torch restatement with the reference module's attribute (state_dict) names."""

    def __init__(self, ntoken, ninp, nhead, nhid, nlayers, seed):
        super().__init__()
        torch.manual_seed(seed)
        self.ninp = ninp
        self.embedding = torch.nn.Embedding(ntoken, ninp)
        self.pos_encoder = torch.nn.Module()
        self.pos_encoder.register_buffer("pe", torch.from_numpy(tr.sinusoid(64, ninp)).float()[None])
        layer = torch.nn.TransformerEncoderLayer(ninp, nhead, nhid, 0.5, batch_first=True)
        self.transformer_encoder = torch.nn.TransformerEncoder(layer, nlayers)
        with torch.no_grad():
            for name, p in self.named_parameters():
                if name.endswith("bias"):
                    p.copy_(torch.randn_like(p) * 0.3)
                elif "norm" in name and name.endswith("weight"):
                    p.copy_(1.0 + torch.randn_like(p) * 0.2)
        self.eval()

    def forward(self, src, mask, rule):
        """float32 on the CPU with the fast path off (every position computed), the rule applied after it."""
        torch.backends.mha.set_fastpath_enabled(False)
        try:
            with torch.no_grad():
                x = self.embedding(src) * math.sqrt(self.ninp) + self.pos_encoder.pe[:, :src.shape[1]]
                x = self.transformer_encoder(x, src_key_padding_mask=mask)
                if rule == "zero":
                    x = x.masked_fill(mask[:, :, None], 0.0)
                return x.mean(1).numpy()
        finally:
            torch.backends.mha.set_fastpath_enabled(True)


def reference_geometry():
    """200 / 4 / 800 / 4 at T = 20, B = 37, built and referenced once: (module, src, {mask name: mask},
    {(mask name, rule): (float64 helper output, the CPU float32 forward's error against it)})."""
    if "geo" not in _CACHE:
        m = TorchText(1000, 200, 4, 800, 4, seed=31)
        rng = np.random.default_rng(31)
        B, T = 37, 20
        lengths = np.array([1, 2, 20] + list(rng.integers(1, 21, B - 3)))
        src = rng.integers(0, 1000, (B, T)).astype(np.int64)
        masks = {"prefix": tr.prefix_mask(lengths, T)}
        holes = masks["prefix"].copy()
        holes[2, 0] = True                                             # the full-length row loses its first token
        holes[3] = False
        holes[3, 9] = True                                             # a hole
        masks["holes"] = holes
        w = {k: v.numpy() for k, v in m.state_dict().items()}
        refs = {}
        for name, rule in (("prefix", "compute"), ("prefix", "zero"), ("holes", "compute")):
            ref = tr.forward(w, 4, src, masks[name], rule)
            cpu = m(torch.from_numpy(src), torch.from_numpy(masks[name]), rule)
            refs[name, rule] = (ref, float(np.abs(cpu - ref).max()))
        _CACHE["geo"] = (m, src, masks, refs)
    return _CACHE["geo"]


@pytest.mark.parametrize("mask_name,rule", [("prefix", "compute"), ("prefix", "zero"), ("holes", "compute")])
def test_drop_in_at_the_reference_geometry(cuda, mask_name, rule):
    """err_gpu <= 8 * err_torch + 1e-6 * max(1, max |ref|), err_torch the installed torch's CPU float32 error against the
    float64 helper on the same inputs: the factor covers the GEMMs' other accumulation order over K = 800 and the device's
    exp / rsqrt.  Observed on one MI355X: see DESIGN.md section 5.9."""
    from sessionsimilaritysearch_amd.text import NodeTextTransformer
    m, src, masks, refs = reference_geometry()
    ref, err_torch = refs[mask_name, rule]
    enc = NodeTextTransformer.from_torch(m, pad_rule=rule, device=cuda)
    got = enc.forward(src, masks[mask_name])
    assert got.shape == (37, 200) and got.dtype == torch.float32 and got.device.type == "cuda"
    err_gpu = float(np.abs(got.double().cpu().numpy() - ref).max())
    bound = 8 * err_torch + 1e-6 * max(1.0, float(np.abs(ref).max()))
    print(f"{mask_name} / {rule}: err_gpu = {err_gpu:.3e}, err_torch = {err_torch:.3e}, bound {bound:.3e}, scale {np.abs(ref).max():.2f}")
    assert err_gpu <= bound


def load_record(name):
    z = np.load(os.path.join(ROOT, "tests", "golden", "text_transformer.npz"))
    wname = "t64" if name == "t1" else name                            # t1 ran t64's module
    w = {k.split(":w:")[1]: torch.from_numpy(z[k].astype(np.float32)) for k in z.files if k.startswith(wname + ":w:")}
    rec = {k.split(":", 1)[1]: z[k] for k in z.files if k.startswith(name + ":") and ":w:" not in k}
    return w, int(rec["nhead"]), rec


@pytest.mark.parametrize("name", ["cfg_like", "t64", "t1", "full"])
def test_fixture_records_against_the_references_own_outputs(cuda, name):
    """Each stored output of the reference module against the drop-in under the rule that output followed, with the stored
    reference error in place of err_torch: err <= 8 * err_ref + 1e-6 * max(1, max |ref|)."""
    from sessionsimilaritysearch_amd.text import NodeTextTransformer
    w, nhead, rec = load_record(name)
    src = rec["src"]
    mask = tr.prefix_mask(rec["lengths"], src.shape[1])
    enc = {r: NodeTextTransformer(w, nhead, pad_rule=r, device=cuda) for r in ("compute", "zero")}
    got = {r: enc[r].forward(src, mask).cpu().numpy() for r in enc}
    rule = rec["rule_fast"]
    fast = np.stack([got["zero"][b] if rule[b] == 1 else got["compute"][b] for b in range(len(rule))])
    cases = [("fast path off", got["compute"], rec["out_slow"], rec["err_slow"]), ("fast path on", fast, rec["out_fast"], rec["err_fast"])]
    if "mask_np" in rec:
        cases.append(("non-prefix mask", enc["compute"].forward(src, rec["mask_np"]).cpu().numpy(), rec["out_np"], rec["err_np"]))
    for what, mine, ref, err_ref in cases:
        err, bound = float(np.abs(mine - ref).max()), 8 * float(err_ref) + 1e-6 * max(1.0, float(np.abs(ref).max()))
        print(f"{name} {what}: err = {err:.3e}, err_ref = {float(err_ref):.3e}, bound {bound:.3e}")
        assert err <= bound, (name, what)


def test_structure(cuda):
    """Three chunks with boundaries between sequences, and the same batch twice, are bit-equal to one chunk; "zero" on a batch
    with no padding equals "compute" bit for bit; an empty batch works; a bad id raises before any launch."""
    from sessionsimilaritysearch_amd.text import NodeTextTransformer, pack_tokens, split_chunks
    m, src, masks, _ = reference_geometry()
    mask = masks["prefix"]
    one = NodeTextTransformer.from_torch(m, device=cuda)
    a = one.forward(torch.from_numpy(src).to(cuda), torch.from_numpy(mask).to(cuda))       # device inputs are taken too
    assert torch.equal(a, one.forward(src, mask))
    small = NodeTextTransformer.from_torch(m, device=cuda, chunk_rows=300)
    chunks = split_chunks(pack_tokens(src, mask, "compute").ptr, 300)
    assert len(chunks) == 3 and chunks[0][1] == 15
    assert torch.equal(a, small.forward(src, mask))
    full = np.zeros_like(mask)
    z = NodeTextTransformer.from_torch(m, pad_rule="zero", device=cuda)
    assert torch.equal(one.forward(src, full), z.forward(src, full))
    assert not torch.equal(one.forward(src, mask), z.forward(src, mask))
    empty = one.forward(np.zeros((0, 20), np.int64), np.zeros((0, 20), bool))
    assert empty.shape == (0, 200) and empty.dtype == torch.float32 and empty.device.type == "cuda"
    bad = src.copy()
    bad[4, 19] = 1000                                                   # a padded position: nn.Embedding would raise too
    for enc in (one, z):
        with pytest.raises(IndexError):
            enc.forward(bad, mask)
    with pytest.raises(ValueError):
        one.forward(src, np.ones_like(mask))


def test_output_feeds_the_hgt_encoder(cuda):
    """tokens -> NodeTextTransformer -> HGT on a five-session batch: shape and finiteness only (each has its own tests)."""
    import hgt_ref as hr
    from sessionsimilaritysearch_amd import sessions as S
    from sessionsimilaritysearch_amd.sessions import EDGE_PP, EDGE_PQ, EDGE_QP
    from sessionsimilaritysearch_amd.text import NodeTextTransformer
    from sessionsimilaritysearch_amd.variants import HGT
    b = S.build_batch(S.synthetic_actions(5, 3, 500, 65)).to_numpy()
    ei = b.edge_index_dict
    edges = {"qp": ei[EDGE_QP], "pq": ei[EDGE_PQ], "pp": ei[EDGE_PP]}
    nq, np_ = len(b["query"].x), len(b["product"].x)
    m = TorchText(60, 40, 4, 16, 1, seed=5)
    rng = np.random.default_rng(5)
    src = rng.integers(0, 60, (nq, 12)).astype(np.int64)
    mask = tr.prefix_mask(rng.integers(1, 13, nq), 12)
    x_q = NodeTextTransformer.from_torch(m, pad_rule="zero", device=cuda).forward(src, mask)
    assert x_q.shape == (nq, 40)
    g = torch.Generator().manual_seed(40)
    w = hr.make_weights(g, 40, 96, 32, 8, 1)
    csr = {e: tuple(torch.from_numpy(a).to(cuda) for a in hr.csr_by_target(edges[e], n)) for e, n in (("qp", np_), ("pq", nq), ("pp", np_))}
    out = HGT(w, 8, 1, cuda).forward(x_q, torch.randn((np_, 96), generator=g).to(cuda), csr["qp"], csr["pq"], csr["pp"])
    assert out["query"].shape == (nq, 64) and out["product"].shape == (np_, 64)
    assert bool(torch.isfinite(out["query"]).all()) and bool(torch.isfinite(out["product"]).all())
