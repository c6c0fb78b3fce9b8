"""``sss_row_norm_max`` for each of the four storage formats at its shape edges: fewer rows than waves, rows of one
16-byte chunk, and rows of 65 chunks (a lane's loop runs a second, partial pass)."""
import numpy as np
import pytest
import torch

from sessionsimilaritysearch_amd import _lib

pytestmark = pytest.mark.gpu

FORMATS = {0: (torch.float32, 4), 1: (torch.bfloat16, 8), 4: (torch.float16, 8), 6: (torch.int8, 16)}   # code: (type, elements per chunk)


def _norm_max(x: torch.Tensor, code: int) -> float:
    out = torch.zeros(1, dtype=torch.float32, device=x.device)
    rc = _lib.lib().sss_row_norm_max(x.data_ptr(), x.shape[0], x.shape[1], code, out.data_ptr(), _lib.stream_ptr(x.device))
    _lib.check(rc, "sss_row_norm_max")
    return float(out.item())


def _rows(code, n, d, seed):
    g = torch.Generator().manual_seed(seed)
    if code == 6:
        return torch.randint(-128, 128, (n, d), generator=g, dtype=torch.int8)
    return (torch.randn((n, d), generator=g) * 3.0).to(FORMATS[code][0])


@pytest.mark.parametrize("chunks", [1, 65])
@pytest.mark.parametrize("code", [0, 1, 4, 6])
def test_row_norm_max_is_a_tight_upper_bound(cuda, code, chunks):
    n, d = 3, chunks * FORMATS[code][1]
    x = _rows(code, n, d, 100 * code + chunks)
    exact_max = float(np.sqrt((x.double().numpy() ** 2).sum(1).max()))       # float64 norm of the STORED values
    got = _norm_max(x.to(cuda), code)
    print(f"code {code} d {d}: exact {exact_max!r} got {got!r}")
    # the upper side: the bound of the corpus-max-norm assertion in tests/test_i8_index_gpu.py
    assert exact_max <= got <= exact_max * (1 + 1e-6)


@pytest.mark.parametrize("chunks", [1, 65])
@pytest.mark.parametrize("bad", [float("inf"), float("-inf"), float("nan")])
def test_f16_row_with_inf_or_nan_reads_as_inf(cuda, chunks, bad):
    n, d = 3, chunks * 8
    x = _rows(4, n, d, 7 + chunks)
    x[1, d - 3] = bad                                       # (65 chunks: in the lane loop's second pass)
    assert _norm_max(x.to(cuda), 4) == float("inf")
