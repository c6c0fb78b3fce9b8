"""GPU side of the node text encoder: sss_bert_embed through the C ABI at the widths and row counts where its lane map can
go wrong, act = 5 (exact GELU) of sss_linear_grouped on a tile with an edge in both directions, and text.BertNodeEncoder end
to end against the float64 helper of tests/helpers/bert_ref.py (for the fixture record, against the `transformers`
BertModel's own stored outputs)."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import bert_ref as br  # noqa: E402

from sessionsimilaritysearch_amd import _lib  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-5                                  # times max(1, max |ref|), the project's float32 kernel tolerance
_CACHE = {}


def _dev(a, cuda):
    return torch.from_numpy(np.ascontiguousarray(a)).to(cuda)


# ------------------------------------------------------------------------------------------------ sss_bert_embed
@pytest.mark.parametrize("e,ld", [(4, 8), (64, 96), (200, 224), (768, 772), (1024, 1056)])
def test_bert_embed(cuda, e, ld):
    """n in {1, 63, 65, 257}: one ragged workgroup of four rows up to 65 workgroups.  The reference is a float64 LayerNorm of
    the float32 sums (word + type) + pos, held to the bound tests/test_text_transformer_gpu.py holds sss_add_layernorm to:
    TOL * max(1, max |ref|) per row, plus what the float32 mean can be off by (16 roundings of partial sums) carried to the
    output.  Row 0 (n > 1) sums to one repeated value: beta bit for bit at eps = 1e-12.  Pad columns are exact zeros over a
    poisoned buffer, nothing is written past row n; one bad tok, tt and p each give a zero row and err = 1 with every other
    row unchanged."""
    L, rng = _lib.lib(), np.random.default_rng(e)
    n_word, n_type, n_pos, eps = 50, 2, 20, 1e-12
    word, typ, pos = (rng.standard_normal((k, e)).astype(np.float32) for k in (n_word, n_type, n_pos))
    word[0], typ[1], pos[3] = 1.5, 0.25, 1.5                            # (1.5 + 0.25) + 1.5 = 3.25 in every column
    gamma, beta = (1 + 0.2 * rng.standard_normal(e)).astype(np.float32), rng.standard_normal(e).astype(np.float32)
    d_word, d_typ, d_pos, d_g, d_b = (_dev(a, cuda) for a in (word, typ, pos, gamma, beta))

    def run(tok, tt, p):
        n = len(tok)
        x = torch.full((n + 2, ld), float("nan"), dtype=torch.float32, device=cuda)
        err = torch.zeros(1, dtype=torch.int32, device=cuda)
        d_tok, d_tt, d_p = _dev(tok, cuda), _dev(tt, cuda), _dev(p, cuda)
        rc = L.sss_bert_embed(d_word.data_ptr(), n_word, d_typ.data_ptr(), n_type, d_pos.data_ptr(), n_pos, d_tok.data_ptr(),
                              d_tt.data_ptr(), d_p.data_ptr(), d_g.data_ptr(), d_b.data_ptr(), eps, n, e, x.data_ptr(), ld,
                              err.data_ptr(), _lib.stream_ptr(cuda))
        assert rc == 0, L.sss_last_error()
        x = x.cpu().numpy()
        assert np.isnan(x[n:]).all() and (x[:n, e:] == 0).all()
        return x[:n, :e], int(err.item())

    for n in (1, 63, 65, 257):
        tok, tt, p = rng.integers(0, n_word, n).astype(np.int64), rng.integers(0, n_type, n).astype(np.int32), rng.integers(0, n_pos, n).astype(np.int32)
        if n > 1:
            tok[0], tt[0], p[0] = 0, 1, 3
        s = (word[tok] + typ[tt]) + pos[p]
        assert s.dtype == np.float32
        s = s.astype(np.float64)
        mu, var = s.mean(1, keepdims=True), s.var(1, keepdims=True)
        ref = (s - mu) / np.sqrt(var + eps) * gamma.astype(np.float64) + beta.astype(np.float64)
        bound = TOL * np.maximum(1.0, np.abs(ref).max(1)) + 16 * 2.0 ** -24 * np.abs(s).max(1) * np.abs(gamma).max() / np.sqrt(s.var(1) + eps)
        if n > 1:
            assert (s[0] == 3.25).all()
            bound[0] = 0.0                                              # variance 0: (x - mean) = 0 exactly, the result is beta
            ref[0] = beta
        got, err = run(tok, tt, p)
        worst = (np.abs(got - ref).max(1) / np.maximum(bound, 1e-300)).max() if n > 1 else np.abs(got - ref).max() / bound[0]
        print(f"e={e} n={n}: max|err| = {np.abs(got - ref).max():.3e}, worst err / bound = {worst:.3f}")
        assert err == 0 and (np.abs(got - ref).max(1) <= bound).all()
        if n > 1:
            assert np.array_equal(got[0], beta)
        if n == 65:
            for what, bad in (("tok", n_word), ("tok", -1), ("tok", 1 << 40), ("tt", n_type), ("tt", -1), ("p", n_pos), ("p", -1)):
                t2, y2, p2 = tok.copy(), tt.copy(), p.copy()
                {"tok": t2, "tt": y2, "p": p2}[what][7] = bad
                g2, err = run(t2, y2, p2)
                assert err == 1 and (g2[7] == 0).all() and np.array_equal(np.delete(g2, 7, 0), np.delete(got, 7, 0)), (what, bad)
    assert L.sss_bert_embed(d_word.data_ptr(), n_word, d_typ.data_ptr(), n_type, d_pos.data_ptr(), n_pos, 0, 0, 0, d_g.data_ptr(),
                            d_b.data_ptr(), eps, 0, e, 0, ld, 0, _lib.stream_ptr(cuda)) == 0


# ------------------------------------------------------------------------------------------------ act = 5
def test_linear_grouped_exact_gelu(cuda):
    """n = 65, m = 96, k = 32: the 64 x 64 tile has an edge in both directions.  The pre-activation v is what an act = 0 launch
    on the same inputs writes (the same accumulation, so act = 5 is gelu of exactly these float32 values); against the float64
    GELU of v:  max err_gpu <= 8 * max err_torch + 1e-7, err_torch the error of torch's CPU float32 F.gelu on the same v.
    Row 3 of x is zero and column 5 has no bias: v = 0 exactly there, and gelu(0) = 0.  Columns 6 and 7 carry a bias of
    +-12 (|v| > 10: the identity and the zero tail), row 9 of x holds a NaN, which must come through as NaN."""
    L, rng = _lib.lib(), np.random.default_rng(55)
    n, m, k = 65, 96, 32
    x = rng.standard_normal((n, k)).astype(np.float32)
    w = (rng.standard_normal((m, k)) * 0.5).astype(np.float32)
    b = rng.standard_normal(m).astype(np.float32)
    x[3], b[5], b[6], b[7] = 0.0, 0.0, 12.0, -12.0
    w[6:8] *= 0.1
    x[9, 4] = np.nan
    d_x, d_w, d_b = _dev(x, cuda), _dev(w, cuda), _dev(b, cuda)

    def run(act):
        y = torch.full((n + 1, m + 4), -7.0, dtype=torch.float32, device=cuda)
        prob = (_lib.LinearProblem * 1)(_lib.LinearProblem(x=d_x.data_ptr(), ldx=k, w=d_w.data_ptr(), ldw=k, bias=d_b.data_ptr(),
                                                           y=y.data_ptr(), ldy=m + 4, n=n, m=m, act=act))
        assert L.sss_linear_grouped(prob, 1, k, _lib.stream_ptr(cuda)) == 0, L.sss_last_error()
        y = y.cpu().numpy()
        assert (y[n] == -7.0).all() and (y[:, m:] == -7.0).all()       # nothing past the edges
        return y[:n, :m]

    v, got = run(0), run(5)
    nan = np.isnan(v)
    assert nan[9].all() and not np.delete(nan, 9, 0).any() and np.array_equal(np.isnan(got), nan)
    assert v[3, 5] == 0.0 and got[3, 5] == 0.0
    assert v[:, 6][~nan[:, 6]].min() > 10 and v[:, 7][~nan[:, 7]].max() < -10
    ok = ~nan
    ref = br.gelu(torch.from_numpy(v).double()).numpy()
    cpu = torch.nn.functional.gelu(torch.from_numpy(v)).numpy()
    err_gpu, err_torch = np.abs(got - ref)[ok].max(), np.abs(cpu - ref)[ok].max()
    print(f"act=5: max err_gpu = {err_gpu:.3e}, max err_torch = {err_torch:.3e}, bound {8 * err_torch + 1e-7:.3e}")
    assert err_gpu <= 8 * err_torch + 1e-7
    assert np.array_equal(run(5), got, equal_nan=True)


# ------------------------------------------------------------------------------------------------ the drop-in
def load_fixture():
    z = np.load(os.path.join(ROOT, "tests", "golden", "bert_encoder.npz"))
    w = {k[2:]: torch.from_numpy(z[k].astype(np.float32)) for k in z.files if k.startswith("w:")}
    return w, int(z["heads"]), float(z["eps"]), {k: z[k] for k in z.files if not k.startswith("w:")}


def check(what, got, ref, err_f32):
    """err_gpu <= 8 * err_f32 + 1e-6 * max(1, max |ref|): err_f32 is what float32 arithmetic costs on a CPU at this shape (the
    helper in float32, or the float32 `transformers` model against a float64 copy of itself); the factor covers the GEMMs'
    other accumulation order and the device's exp / erf / rsqrt.  Observed on one MI355X: see DESIGN.md section 5.10."""
    got = got.double().cpu().numpy()
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    err_gpu, bound = float(np.abs(got - ref).max()), 8 * float(err_f32) + 1e-6 * max(1.0, float(np.abs(ref).max()))
    print(f"{what}: err_gpu = {err_gpu:.3e}, err_f32 = {float(err_f32):.3e}, bound {bound:.3e}, scale {np.abs(ref).max():.2f}")
    assert err_gpu <= bound, what


def test_fixture_record_against_the_transformers_outputs(cuda):
    """Both pools and get_token against the stored outputs of the float32 BertModel, with its stored error against a float64
    copy of itself as err_f32.  get_token returns every position, the padded ones as HF computes them (not zeros)."""
    from sessionsimilaritysearch_amd.text import BertNodeEncoder
    w, heads, eps, rec = load_fixture()
    ids, tt, am = rec["input_ids"], rec["token_type_ids"], rec["attention_mask"]
    for pool in ("masked", "mean"):
        enc = BertNodeEncoder(w, heads, pool=pool, eps=eps, device=cuda)
        out = enc(ids, tt, am)
        assert out.shape == (7, 64) and out.dtype == torch.float32 and out.device.type == "cuda"
        check(f"fixture {pool}", out, rec["pooled_" + pool].astype(np.float64), rec["err_" + pool])
        out2, tokens = enc(torch.from_numpy(ids).to(cuda), torch.from_numpy(tt).to(cuda), torch.from_numpy(am).to(cuda), get_token=True)
        assert tokens.shape == (7, 12, 64) and tokens.dtype == torch.float32 and tokens.device.type == "cuda"
        check(f"fixture {pool} tokens", tokens, rec["last_hidden_state"].astype(np.float64), rec["err_states"])
        check(f"fixture {pool} with get_token", out2, rec["pooled_" + pool].astype(np.float64), rec["err_" + pool])
    # padded ids never reach the masked mean: not a bit changes
    enc = BertNodeEncoder(w, heads, eps=eps, device=cuda)
    assert torch.equal(enc(ids, tt, am), enc(rec["input_ids_alt"], tt, am))


GEOMETRIES = {  # name: (vocab, e, heads, inter, nlayers, n_pos, T, lengths, nout)
    "bert-base width": (100, 768, 12, 3072, 2, 32, 20, [20, 1, 2, 7, 20, 3, 12, 5, 19], None),
    "pad32 under gelu": (60, 96, 4, 100, 2, 32, 11, [11, 1, 4, 2, 9], 10),     # D = 24, intermediate 100 -> 128, a lin head
}


def geometry(name):
    """(weights, heads, ids, tt, am, {pool: (float64 pooled, err_f32)}, (float64 states, err_f32)), built once."""
    if name not in _CACHE:
        vocab, e, heads, inter, nlayers, n_pos, T, lengths, nout = GEOMETRIES[name]
        w = br.seeded_weights(len(name), vocab, e, heads, inter, nlayers, n_pos, nout=nout)
        rng = np.random.default_rng(len(name))
        B = len(lengths)
        ids, tt = rng.integers(0, vocab, (B, T)).astype(np.int64), rng.integers(0, 2, (B, T)).astype(np.int64)
        am = (np.arange(T)[None, :] < np.asarray(lengths)[:, None]).astype(np.int64)
        s, s32 = br.token_states(w, heads, ids, tt, am), br.token_states(w, heads, ids, tt, am, dtype=torch.float32)
        assert s.dtype == np.float64 and s32.dtype == np.float32
        states = (s, np.abs(s32 - s).max())
        pooled = {}
        for pool in ("masked", "mean"):
            ref, f32 = br.head(w, s, am, pool), br.head(w, s32, am, pool)
            assert f32.dtype == np.float32
            pooled[pool] = (ref, np.abs(f32 - ref).max())
        _CACHE[name] = (w, heads, ids, tt, am, pooled, states)
    return _CACHE[name]


@pytest.mark.parametrize("name", list(GEOMETRIES))
@pytest.mark.parametrize("pool", ["masked", "mean"])
def test_drop_in_against_the_float64_helper(cuda, name, pool):
    """768 / 12 / 3072, 2 layers, T = 20, B = 9 with lengths 1, 2 and 20; and 96 / 4 heads (D = 24) / intermediate 100 with a
    Linear(96, 10) head, where the GEMMs read pad32 columns that the embedding, the attention and the GELU wrote as zeros."""
    from sessionsimilaritysearch_amd.text import BertNodeEncoder
    w, heads, ids, tt, am, pooled, states = geometry(name)
    nout = GEOMETRIES[name][8] or GEOMETRIES[name][1]
    enc = BertNodeEncoder(w, heads, pool=pool, device=cuda)
    out, tokens = enc(ids, tt, am, get_token=True)
    assert out.shape == (len(ids), nout) and tokens.shape == ids.shape + (GEOMETRIES[name][1],)
    check(f"{name} {pool}", out, *pooled[pool])
    check(f"{name} {pool} tokens", tokens, *states)
    check(f"{name} {pool} without get_token", enc(ids, tt, am), *pooled[pool])


def test_structure(cuda):
    """Bit-equality: dedup on and off on a batch with repeated rows (and a row that differs only in a padded id, which is not a
    duplicate under "mean"), one sequence per chunk against the default chunk, the same call twice.  An empty batch and a
    batch of one work; a sequence with no attended token raises ValueError."""
    from sessionsimilaritysearch_amd.text import BertNodeEncoder, bert_pack_rows, split_chunks
    w = br.seeded_weights(77, 60, 96, 4, 100, 2, 64, nout=10)
    rng = np.random.default_rng(77)
    T, lengths = 40, [40, 2, 2, 17, 2, 40, 1, 17, 33]
    B = len(lengths)
    ids, tt = rng.integers(0, 60, (B, T)).astype(np.int64), rng.integers(0, 2, (B, T)).astype(np.int64)
    am = (np.arange(T)[None, :] < np.asarray(lengths)[:, None]).astype(np.int64)
    for dst, src in ((2, 1), (4, 1), (7, 3), (5, 0)):                   # the root query repeats; so does a title
        ids[dst], tt[dst] = ids[src], tt[src]
    ids[4, 30] = (ids[4, 30] + 1) % 60                                  # a padded id: still the same row under "masked"
    for pool in ("masked", "mean"):
        on = BertNodeEncoder(w, 4, pool=pool, device=cuda)
        off = BertNodeEncoder(w, 4, pool=pool, device=cuda, dedup=False)
        one = BertNodeEncoder(w, 4, pool=pool, device=cuda, dedup=False, chunk_rows=64)
        a, a_tok = on(ids, tt, am, get_token=True)
        b, b_tok = off(ids, tt, am, get_token=True)
        c, c_tok = one(ids, tt, am, get_token=True)
        assert len(split_chunks(bert_pack_rows(ids, tt, am, pool, True).rows.ptr, 64)) == B      # 40 rows each: one per chunk
        assert torch.equal(a, b) and torch.equal(a_tok, b_tok) and torch.equal(a, c) and torch.equal(a_tok, c_tok)
        assert torch.equal(a[1], a[2]) and torch.equal(a[3], a[7]) and torch.equal(a[0], a[5])
        assert torch.equal(a[1], a[4]) == (pool == "masked")
        assert not torch.equal(a_tok[1], a_tok[4]) and torch.equal(a_tok[1, :2], a_tok[4, :2])
        plain = on(ids, tt, am)
        assert torch.equal(plain, off(ids, tt, am)) and torch.equal(plain, one(ids, tt, am)) and torch.equal(plain, on(ids, tt, am))
        assert torch.equal(plain, a)                                    # dropping the padded rows changes no bit of the pool
        assert torch.equal(on(ids[:1], tt[:1], am[:1]), plain[:1])
        empty, empty_tok = on(ids[:0], tt[:0], am[:0], get_token=True)
        assert empty.shape == (0, 10) and empty_tok.shape == (0, T, 96) and empty.device.type == "cuda"
    dead = am.copy()
    dead[6] = 0
    with pytest.raises(ValueError):
        on(ids, tt, dead)
