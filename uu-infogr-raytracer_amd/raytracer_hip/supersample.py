"""The definition of the library's supersampling (rt_set_supersampling) in numpy.

At factor k an output pixel (x, y) is, per 8-bit channel, the round-half-up mean of the k x k
pixels (k x + i, k y + j) of the k W x k H frame: (sum + k*k/2) >> 2 log2 k, in integers.  The
trace kernels compute exactly this in registers; `box_resolve` computes it from a rendered
k W x k H frame, for tests and for anyone who wants to compare.
"""
from __future__ import annotations

import numpy as np

FACTORS = (1, 2, 4, 8)


def box_resolve(frame: np.ndarray, k: int) -> np.ndarray:
    """int32 0x00RRGGBB frame [k H, k W] -> int32 [H, W]: the k x k box mean per channel, ties rounded up."""
    if k not in FACTORS:
        raise ValueError(f"supersampling factor {k} is not one of {FACTORS}")
    f = np.asarray(frame)
    if f.ndim != 2 or f.shape[0] % k or f.shape[1] % k:
        raise ValueError(f"a 2-D frame with sides that are multiples of {k} is required, got {f.shape}")
    h, w = f.shape[0] // k, f.shape[1] // k
    f = f.astype(np.int64)
    out = np.zeros((h, w), dtype=np.int64)
    for shift in (16, 8, 0):
        s = ((f >> shift) & 0xFF).reshape(h, k, w, k).sum(axis=(1, 3))
        out |= ((s + (k * k) // 2) // (k * k)) << shift
    return out.astype(np.int32)
