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


# Adaptive supersampling (rt_set_adaptive_sampling): the decision is taken per 8x8 tile of the output, on the frame
# without supersampling, which is sample (0, 0) of every k x k block.
TILE = 8


def refine_mask(plain: np.ndarray, threshold: int) -> np.ndarray:
    """int32 0x00RRGGBB frame [H, W] -> bool [ceil(H / 8), ceil(W / 8)]: the tiles that are refined at `threshold`
    (1..256).  Tile (tx, ty) is the pixels [8 tx, 8 tx + 8) x [8 ty, 8 ty + 8) clipped to the frame; it is refined
    iff it holds two 4-adjacent pixels, both inside the tile, that differ by >= threshold in some 8-bit channel."""
    if not 1 <= int(threshold) <= 256:
        raise ValueError(f"adaptive threshold {threshold} is not in 1..256")
    p = np.asarray(plain)
    if p.ndim != 2:
        raise ValueError(f"a 2-D frame is required, got {p.shape}")
    h, w = p.shape
    ch = np.stack([(p.astype(np.int64) >> s) & 0xFF for s in (16, 8, 0)])
    # pair (x - 1, x) / (y - 1, y), marked at its second pixel; pairs that straddle a tile border do not count
    dx = np.zeros((h, w), dtype=bool)
    dy = np.zeros((h, w), dtype=bool)
    dx[:, 1:] = (np.abs(ch[:, :, 1:] - ch[:, :, :-1]) >= threshold).any(axis=0)
    dy[1:, :] = (np.abs(ch[:, 1:, :] - ch[:, :-1, :]) >= threshold).any(axis=0)
    dx[:, ::TILE] = False
    dy[::TILE, :] = False
    hit = dx | dy
    th, tw = -(-h // TILE), -(-w // TILE)
    pad = np.zeros((th * TILE, tw * TILE), dtype=bool)
    pad[:h, :w] = hit
    return pad.reshape(th, TILE, tw, TILE).any(axis=(1, 3))


def adaptive_resolve(plain: np.ndarray, samples: np.ndarray, k: int, threshold: int) -> np.ndarray:
    """The definition of adaptive supersampling: `plain` [H, W] (the frame without supersampling), `samples`
    [k H, k W] (the frame at k W x k H) -> box_resolve(samples, k) on the refined tiles of `plain`, `plain` on the
    others.  threshold 0 (off): box_resolve everywhere."""
    full = box_resolve(samples, k)
    p = np.asarray(plain).astype(np.int32)
    if p.shape != full.shape:
        raise ValueError(f"plain frame {p.shape} does not match the resolved samples {full.shape}")
    if int(threshold) == 0:
        return full
    m = refine_mask(p, threshold)
    px = np.repeat(np.repeat(m, TILE, axis=0), TILE, axis=1)[:p.shape[0], :p.shape[1]]
    return np.where(px, full, p).astype(np.int32)
