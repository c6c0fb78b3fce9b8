"""CPU side of the reduced-precision grouped GEMM (include/lowp/sss_linear_bf16.h, csrc/linear_bf16.hip) and of the
``gemm=`` switch of text.py: the lowp header against its binding and its snapshot (tests/golden/abi_signatures_lowp.json),
with the pinned listings of include/ and include/ext/ unchanged; argument validation without a device; the values ``gemm``
takes."""
import json
import os
import sys

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import abi  # noqa: E402
import bert_ref as br  # noqa: E402

from sessionsimilaritysearch_amd import _lib  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = "sss_linear_bf16.h"
NAME = "sss_linear_grouped_bf16"
SNAPSHOT = os.path.join(ROOT, "tests", "golden", "abi_signatures_lowp.json")


def test_lowp_header_is_declared_exported_bound_and_equals_its_snapshot():
    assert abi.declared(os.path.join("lowp", HEADER)) == sorted(_lib.LOWP_HEADERS[HEADER]) == [NAME]
    assert sorted(_lib.LOWP_HEADERS) == sorted(f for f in os.listdir(os.path.join(ROOT, "include", "lowp")) if f.endswith(".h"))
    assert len(_lib.HEADERS) == 12 and len(_lib.PARAMS) == 98
    assert sorted(_lib.EXT_HEADERS) == ["sss_seqsim.h"] and sorted(_lib.EXT_PARAMS) == ["sss_seq_pair_scores", "sss_seq_query_metric"]
    assert not set(_lib.LOWP_PARAMS) & (set(_lib.PARAMS) | set(_lib.EXT_PARAMS))
    with open(SNAPSHOT) as f:
        snap = json.load(f)
    assert {h: {n: abi.signature(*sig) for n, sig in t.items()} for h, t in _lib.LOWP_HEADERS.items()} == snap["functions"]
    assert {n: list(p) for n, p in _lib.LOWP_PARAMS.items()} == snap["params"]
    fn = getattr(_lib.lib(), NAME)                                     # exported by libsss.so and bound by lib()
    assert abi.signature(fn.restype, fn.argtypes) == snap["functions"][HEADER][NAME] == ["c_int", ["c_void_p", "c_int", "c_int", "c_void_p"]]
    assert _lib.LOWP_PARAMS[NAME] == ("problems", "n_problems", "k", "stream")
    # the same struct and the same parameters as the float32 entry point
    assert _lib.HEADERS["sss.h"]["sss_linear_grouped"] == _lib.LOWP_HEADERS[HEADER][NAME] and _lib.PARAMS["sss_linear_grouped"] == _lib.LOWP_PARAMS[NAME]
    text = open(os.path.join(ROOT, "include", "lowp", HEADER)).read()
    assert "CALLER-OWNED DEVICE" in text and "2^-23" in text and "SUBNORMAL" in text


_P = 1 << 20                                                          # a non-null, 16-byte aligned address; never dereferenced


def _problem(**kw):
    a = dict(x=_P, ldx=64, w=_P, ldw=64, bias=_P, y=_P, ldy=16, n=5, m=16, act=0)
    a.update(kw)
    return _lib.LinearProblem(**a)


def _call(probs, k=64):
    L = _lib.lib()
    arr = (_lib.LinearProblem * max(1, len(probs)))(*probs)
    return L.sss_linear_grouped_bf16(arr, len(probs), k, 0), L.sss_last_error() or b""


def test_arguments_are_rejected_before_any_launch():
    """No address given here is memory: a call that launched would fault.  Every rejection is -1 (SSS_EINVAL) with a message
    that names what is wrong; the good problem beside a bad one does not rescue the launch."""
    ok = _problem()
    for probs, k, words in (([], 64, b"1..4 problems"), ([ok] * 5, 64, b"1..4 problems"),
                            ([ok], 0, b"k % 32"), ([ok], 48, b"k % 32"), ([ok], -32, b"k % 32"),
                            ([_problem(ldw=68)], 64, b"ldw % 8"), ([_problem(ldw=32)], 64, b"ldw >= k"),
                            ([_problem(ldx=66)], 64, b"ldx % 4"), ([_problem(ldx=32)], 64, b"ldx >= k"),
                            ([_problem(ldy=15)], 64, b"ldy >= m"),
                            ([_problem(ids=_P)], 64, b"no gather"), ([_problem(table=_P)], 64, b"no gather"),
                            ([_problem(xcopy=_P, ld_xcopy=64)], 64, b"no gather"),
                            ([_problem(act=6)], 64, b"0..5"), ([_problem(act=-1)], 64, b"0..5"),
                            ([_problem(post_scale=_P)], 64, b"come together"), ([_problem(post_shift=_P)], 64, b"come together"),
                            ([_problem(m=0)], 64, b"m > 0"), ([_problem(n=-1)], 64, b"n >= 0"),
                            ([ok, _problem(ldy=15)], 64, b"problem 1"), ([ok, ok, ok, _problem(act=6)], 64, b"problem 3")):
        rc, msg = _call(probs, k)
        assert rc == -1 and msg.startswith(b"linear_grouped_bf16:") and words in msg, (k, words, rc, msg)
    assert _lib.lib().sss_linear_grouped_bf16(None, 1, 64, 0) == -1
    # a launch that would need more tiles than a grid has
    rc, msg = _call([_problem(n=1 << 40, m=1 << 20, ldy=1 << 20)], 64)
    assert rc == -1 and b"tiles" in msg


def test_an_empty_launch_returns_ok_without_a_device():
    assert _call([_problem(n=0)])[0] == 0
    wide = dict(n=0, ldx=96, ldw=96)
    assert _call([_problem(**wide), _problem(m=1, ldy=1, **wide), _problem(m=300, ldy=300, **wide), _problem(**wide)], 96)[0] == 0
    assert _call([_problem(n=0, x=0, y=0, w=0, bias=0)])[0] == 0      # nothing is read: no pointer is needed
    assert _call([_problem(n=0, ldy=15)])[0] == -1                      # an empty problem's shapes are still checked


def test_gemm_takes_f32_or_bf16_only():
    """Any other value raises ValueError before device work (device="cpu": nothing here reaches a kernel); "f32" constructs
    what the class constructs without the keyword."""
    import torch
    from sessionsimilaritysearch_amd.text import GEMMS, BertNodeEncoder, NodeTextTransformer
    assert GEMMS == ("f32", "bf16")
    w = br.seeded_weights(1, 30, 64, 4, 40, 1, 80)
    tw = {"embedding.weight": torch.randn(30, 64), "pos_encoder.pe": torch.randn(1, 80, 64)}
    p = "transformer_encoder.layers.0."
    for name, shape in (("self_attn.in_proj_weight", (192, 64)), ("self_attn.in_proj_bias", (192,)), ("self_attn.out_proj.weight", (64, 64)),
                        ("self_attn.out_proj.bias", (64,)), ("linear1.weight", (40, 64)), ("linear1.bias", (40,)), ("linear2.weight", (64, 40)),
                        ("linear2.bias", (64,)), ("norm1.weight", (64,)), ("norm1.bias", (64,)), ("norm2.weight", (64,)), ("norm2.bias", (64,))):
        tw[p + name] = torch.randn(*shape)
    for bad in ("fp8", "BF16", "f16", None, 16):
        with pytest.raises(ValueError, match="gemm"):
            BertNodeEncoder(w, 4, device="cpu", gemm=bad)
        with pytest.raises(ValueError, match="gemm"):
            NodeTextTransformer(tw, 4, device="cpu", gemm=bad)
    for enc in (BertNodeEncoder(w, 4, device="cpu"), BertNodeEncoder(w, 4, device="cpu", gemm="f32"),
                NodeTextTransformer(tw, 4, device="cpu"), NodeTextTransformer(tw, 4, device="cpu", gemm="f32")):
        assert enc.gemm == "f32" and all(t.dtype == torch.float32 for lay in enc.layers for t in lay.values())
