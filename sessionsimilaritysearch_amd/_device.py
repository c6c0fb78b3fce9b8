"""Device plumbing the models and index classes share: the device a model binds to and the upload of a weight; a scratch
buffer that only grows, amortised row storage and the query chunking of the exhaustive kernels."""
from __future__ import annotations

import torch

EXHAUSTIVE_WS_BYTES = 1 << 30       # budget of a [chunk, n] score matrix of the exhaustive kernels


def model_device(device=None) -> torch.device:
    """The device a model is bound to: ``device``, or the current HIP device when it is None."""
    return torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)


def upload_f32(t: torch.Tensor, device) -> torch.Tensor:
    """``t`` as the kernels read a weight: detached, float32, contiguous, on ``device``."""
    return t.detach().to(device=device, dtype=torch.float32).contiguous()


class Workspace:
    """One scratch buffer per index, re-made only when a call needs more than it holds."""

    def __init__(self, device):
        self.device = device
        self.buf = None

    def get(self, nbytes: int) -> torch.Tensor:
        if self.buf is None or self.buf.numel() < nbytes:
            self.buf = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
        return self.buf


def grow_rows(store: torch.Tensor, view: torch.Tensor, x: torch.Tensor):
    """Append the rows ``x`` to ``view``, the first rows of its backing storage ``store``: amortised growth (the
    storage at least doubles when it is full), no re-copy per call.  Returns the new (store, view)."""
    n_old, n = view.shape[0], view.shape[0] + x.shape[0]
    if n > store.shape[0]:
        grown = torch.empty((max(n, 2 * store.shape[0]), store.shape[1]), dtype=store.dtype, device=store.device)
        grown[:n_old] = view
        store = grown
    store[n_old:n] = x
    return store, store[:n]


def exhaustive_chunk(n: int, bytes_per_score: int) -> int:
    """Queries per exhaustive call against n rows: what keeps their score matrix inside EXHAUSTIVE_WS_BYTES, at most
    the 65535 a launch grid takes."""
    return max(1, min(65535, EXHAUSTIVE_WS_BYTES // max(1, bytes_per_score * n)))
