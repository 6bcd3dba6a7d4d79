"""Shared by tests/test_adaptive.py (CPU) and tests/test_gpu_adaptive.py: the cases of adaptive supersampling
(rt_set_adaptive_sampling) and their expectations from the definition, supersample.adaptive_resolve of the
oracle's plain and k W x k H frames.  Each oracle render is computed once per process and shared read-only."""
import numpy as np

from raytracer_hip import scenes
from raytracer_hip.supersample import TILE, adaptive_resolve, box_resolve, refine_mask
from test_gpu_supersample import SCENES

# (scene of test_gpu_supersample.SCENES, W, H, k, T): every kernel family, stack kind and shadow pass at k = 2 ...
CASES_K2 = [
    ("C3", 50, 30, 2, 96),           # direct, LDS stack
    ("REF", 45, 27, 2, 48),          # limit 32, scratch stack, ragged width
    ("C4", 96, 56, 2, 96),           # bundle, merged pass
    ("dense", 74, 42, 2, 96),
    ("bundle_L5", 64, 48, 2, 16),
    ("gpow_bundle", 64, 48, 2, 96),
    ("gpow_direct", 32, 24, 2, 96),
]
# ... both families at the larger factors (C4 at 50x30 and T = 96 leaves 3 pixels that differ from full supersampling:
# 128 leaves 48) ...
CASES_K48 = [(cid, W, H, k, 128) for cid in ("C3", "C4") for (W, H) in ((50, 30), (96, 56)) for k in (4, 8)]
# ... and the frame the band, batch, async and context tests render, at the factors they use
W0, H0, T0 = 50, 30, 128
CASES_API = [(cid, W0, H0, 2, T0) for cid in ("C3", "C4")]
CASES = CASES_K2 + CASES_K48 + CASES_API


def case_id(c):
    return f"{c[0]}-{c[1]}x{c[2]}-k{c[3]}-T{c[4]}"


_SCENES = {}
_FRAMES = {}


def scene(cid):
    if cid not in _SCENES:
        _SCENES[cid] = SCENES[cid]()
    return _SCENES[cid]


def frames(oracle, cid, W, H, k, view_h=None):
    """(frame [k H, k W], oracle stats) of the scene at factor k: rows [0, k H) of a view view_h output rows high."""
    key = (cid, W, H, k, view_h)
    if key not in _FRAMES:
        px, st = oracle.render(scene(cid).resized(k * W, k * (view_h or H)), oracle.MODE_NEAREST, 8, rows=(0, k * H))
        px.setflags(write=False)
        _FRAMES[key] = (px, st)
    return _FRAMES[key]


def expect(oracle, cid, W, H, k, T, view_h=None):
    """The definition's output [H, W] at threshold T (0: full supersampling; k = 1: the plain frame)."""
    plain = frames(oracle, cid, W, H, 1, view_h)[0]
    if k == 1:
        return plain
    return adaptive_resolve(plain, frames(oracle, cid, W, H, k, view_h)[0], k, T)


def pixel_mask(plain, T):
    """bool [H, W]: the pixels of the refined tiles."""
    m = refine_mask(plain, T)
    return np.repeat(np.repeat(m, TILE, axis=0), TILE, axis=1)[:plain.shape[0], :plain.shape[1]]


def traced_samples(plain, k, T):
    """bool [k H, k W]: the samples an adaptive render traces -- sample (0, 0) of every block, and every sample of
    the refined tiles' blocks."""
    t = np.repeat(np.repeat(pixel_mask(plain, T), k, axis=0), k, axis=1)
    t[::k, ::k] = True
    return t


def facts(oracle, cid, W, H, k, T):
    """refined tiles, all tiles, pixels != plain, pixels != full supersampling."""
    plain = frames(oracle, cid, W, H, 1)[0]
    full = box_resolve(frames(oracle, cid, W, H, k)[0], k)
    out = expect(oracle, cid, W, H, k, T)
    m = refine_mask(plain, T)
    return int(m.sum()), int(m.size), int((out != plain).sum()), int((out != full).sum())
