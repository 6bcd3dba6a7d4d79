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


def path_resolve(sample_frames: np.ndarray, k: int, m: int = 1) -> np.ndarray:
    """The definition of rt_set_path_supersampling: sample frames [F * m, k H, k W] of 0x00RRGGBB pixels (sub-frame s
    of output frame f at f * m + s, each rendered at k W x k H) -> int32 [F, H, W].  Per 8-bit channel the output is
    (sum over the m sub-frames and the k x k samples + m k k / 2) >> (log2 m + 2 log2 k): one rounding of the whole
    mean.  m = 1 is box_resolve per frame, k = 1 is path.shutter_mean.  m: a power of two with m k k <= 256."""
    if k not in FACTORS:
        raise ValueError(f"supersampling factor {k} is not one of {FACTORS}")
    if m < 1 or m & (m - 1) or m * k * k > 256:
        raise ValueError(f"shutter {m} is not a power of two with m * k * k <= 256 (k = {k})")
    a = np.asarray(sample_frames)
    if a.ndim != 3 or a.shape[0] % m:
        raise ValueError(f"sample frames {a.shape} are no [F * {m}, k H, k W]")
    if a.shape[1] % k or a.shape[2] % k:
        raise ValueError(f"frames with sides that are multiples of {k} are required, got {a.shape}")
    f, h, w = a.shape[0] // m, a.shape[1] // k, a.shape[2] // k
    n = m * k * k
    px = a.astype(np.int64).reshape(f, m, h, k, w, k)
    out = np.zeros((f, h, w), dtype=np.int64)
    for shift in (16, 8, 0):
        s = ((px >> shift) & 0xFF).sum(axis=(1, 3, 5))
        out |= ((s + n // 2) >> (n.bit_length() - 1)) << shift
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


def path_adaptive_resolve(plain_frames: np.ndarray, sample_frames: np.ndarray, k: int, threshold: int) -> np.ndarray:
    """The definition of rt_set_path_adaptive_sampling: `plain_frames` [F, H, W] (the frames at path factor 1),
    `sample_frames` [F, k H, k W] (the same cameras, and scenes, at k W x k H) -> int32 [F, H, W], adaptive_resolve
    per frame: every frame decides on its own plain frame.  threshold 0 (off): path_resolve(sample_frames, k, 1)."""
    p, s = np.asarray(plain_frames), np.asarray(sample_frames)
    if p.ndim != 3 or s.ndim != 3 or p.shape[0] != s.shape[0]:
        raise ValueError(f"plain frames {p.shape} and sample frames {s.shape} are no [F, H, W] and [F, k H, k W]")
    if not 0 <= int(threshold) <= 256:
        raise ValueError(f"adaptive threshold {threshold} is not in 0..256")
    if k not in FACTORS:
        raise ValueError(f"supersampling factor {k} is not one of {FACTORS}")
    if s.shape[1:] != (p.shape[1] * k, p.shape[2] * k):
        raise ValueError(f"plain frames {p.shape} do not match the sample frames {s.shape} at factor {k}")
    if int(threshold) == 0:
        return path_resolve(s, k, 1)
    out = np.empty(p.shape, dtype=np.int32)
    for f in range(p.shape[0]):
        out[f] = adaptive_resolve(p[f], s[f], k, threshold)
    return out


def shutter_adaptive_resolve(plain_subframes: np.ndarray, sample_subframes: np.ndarray, k: int, m: int,
                             threshold: int) -> np.ndarray:
    """The definition of rt_set_shutter_adaptive_sampling: `plain_subframes` [F * m, H, W] (sub-frame s of output frame
    f at f * m + s, at path factor 1) and `sample_subframes` [F * m, k H, k W] (the same cameras, and scenes, at k W x
    k H) -> int32 [F, H, W].  P = path.shutter_mean(plain_subframes, m) is the factor-1 shutter frame and S =
    path_resolve(sample_subframes, k, m) the fully supersampled one, each with its one rounding; output frame f is S_f
    on the tiles refine_mask(P_f, threshold) picks and P_f elsewhere: every output frame decides for itself, on the
    mean of its sub-frames.  threshold 0 (off): S."""
    from .path import shutter_mean
    p, s = np.asarray(plain_subframes), np.asarray(sample_subframes)
    if p.ndim != 3 or s.ndim != 3 or p.shape[0] != s.shape[0]:
        raise ValueError(f"plain sub-frames {p.shape} and sample sub-frames {s.shape} are no [F m, H, W] and [F m, k H, k W]")
    if not 0 <= int(threshold) <= 256:
        raise ValueError(f"adaptive threshold {threshold} is not in 0..256")
    if k not in FACTORS:
        raise ValueError(f"supersampling factor {k} is not one of {FACTORS}")
    if s.shape[1:] != (p.shape[1] * k, p.shape[2] * k):
        raise ValueError(f"plain sub-frames {p.shape} do not match the sample sub-frames {s.shape} at factor {k}")
    full = path_resolve(s, k, m)  # (checks m: a power of two with m k k <= 256, and F * m frames)
    if int(threshold) == 0:
        return full
    plain = shutter_mean(p, m)
    out = np.empty(plain.shape, dtype=np.int32)
    for f in range(plain.shape[0]):
        px = np.repeat(np.repeat(refine_mask(plain[f], threshold), TILE, axis=0), TILE, axis=1)[:plain.shape[1], :plain.shape[2]]
        out[f] = np.where(px, full[f], plain[f])
    return out


# Progressive accumulation (rt_set_progressive): a resting camera's Ticks take the k x k samples of a pixel one by
# one, coarse sub-grids first, and show the rounded mean of the samples so far.
def progressive_order(k: int) -> list:
    """The samples of a k x k block in the order a progressive run traces them: [(i, j)] (column, row), k*k long.
    With s = log2 k, sample n is found from n's base-4 digits d_0 (least significant) .. d_{s-1}: digit d_t gives
    bit s - 1 - t of i from its bit 0 and bit s - 1 - t of j from its bit 1.  The first 4^t samples are the 2^t x 2^t
    sub-grid of stride k / 2^t."""
    if k not in FACTORS:
        raise ValueError(f"progressive factor {k} is not one of {FACTORS}")
    s = k.bit_length() - 1
    order = []
    for n in range(k * k):
        i = j = 0
        for t in range(s):
            d = (n >> (2 * t)) & 3
            i |= (d & 1) << (s - 1 - t)
            j |= (d >> 1) << (s - 1 - t)
        order.append((i, j))
    return order


def progressive_resolve(samples_frame: np.ndarray, k: int, c: int) -> np.ndarray:
    """The frame P_c of a progressive run: int32 0x00RRGGBB frame [k H, k W] (the frame at k W x k H, which holds
    every sample) -> int32 [H, W], per channel (sum of samples 0 .. c-1 of progressive_order(k) + c // 2) // c."""
    order = progressive_order(k)
    if not 1 <= int(c) <= k * k:
        raise ValueError(f"sample count {c} is not in 1..{k * k}")
    f = np.asarray(samples_frame)
    if f.ndim != 2 or f.shape[0] % k or f.shape[1] % k:
        raise ValueError(f"a 2-D frame with sides that are multiples of {k} is required, got {f.shape}")
    f = f.astype(np.int64)
    out = np.zeros((f.shape[0] // k, f.shape[1] // k), dtype=np.int64)
    for shift in (16, 8, 0):
        ch = (f >> shift) & 0xFF
        total = sum(ch[j::k, i::k] for i, j in order[:c])
        out |= ((total + c // 2) // c) << shift
    return out.astype(np.int32)
