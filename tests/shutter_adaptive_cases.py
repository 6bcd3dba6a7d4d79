"""Shared by tests/test_shutter_adaptive.py (CPU) and tests/test_gpu_shutter_adaptive.py: the cases of adaptive supersampling
under a shutter (rt_set_shutter_adaptive_sampling) and their expectations from the definition,
supersample.shutter_adaptive_resolve of the unchanged oracle's per-sub-frame plain and k W x k H renders.  Camera shutters:
sub-frame j has tests/path_cases.py's camera j % 6 (path_adaptive_cases.cycled); track shutters: sub-frame j is frame j of
a tests/anim_shutter_cases.py track, in its own scene from its own camera.  Every oracle render is computed once per
process (path_cases / anim_cases) and shared read-only.  tests/test_shutter_adaptive.py holds the preconditions of every
case here."""
import dataclasses

import numpy as np

import anim_shutter_cases as ashut
import path_adaptive_cases as pc
from raytracer_hip import path
from raytracer_hip.supersample import path_resolve, refine_mask, shutter_adaptive_resolve

RAYS = pc.RAYS

# camera shutters: (scene of test_gpu_supersample.SCENES, W, H, m, k, T, output frames)
K2M2 = [(cid, 45 if cid == "REF" else 50, 27 if cid == "REF" else 30, 2, 2, 96, 3)
        for cid in ("C3", "C4", "REF", "gpow_direct", "gpow_bundle", "C1", "dense", "bundle_L5")]
M4K2 = [(cid, 45 if cid == "REF" else 50, 27 if cid == "REF" else 30, 4, 2, 64, 3) for cid in ("C3", "C4", "REF")]
M4K4 = [(cid, 50, 30, 4, 4, 64, 1) for cid in ("C3", "C4")]   # 64 values per pixel
M2K8 = [(cid, 50, 30, 2, 8, 96, 1) for cid in ("C3", "C4")]   # 128 values per pixel
CAMERA_CASES = K2M2 + M4K2 + M4K4 + M2K8
# the frame of the threshold, setting, band, view-height and chunk tests: C3, m = 2, k = 2
W0, H0, M0, K0, T0 = 50, 30, 2, 2, 96
VIEW_ROWS = 27


def mixed_track():
    """4 sub-frames of the 8-sphere class's scene, sub-frame 2 with specular exponent 7.3: a track mixing GPOW and other
    frames inside one output frame."""
    base, g = ashut.class_track("s8", False, 3), ashut.class_track("s8", True, 3)
    return [dataclasses.replace((g[f] if f == 2 else sc).resized(W0, H0), name=f"{sc.name}_expmix_sa") for f, sc in enumerate(base)]


# track shutters: name -> (builder, m, k, T, first_frame)
TRACKS = {
    "direct_m2": (lambda: ashut.direct_track(6, 50, 30), 2, 2, 96, 0),
    "direct_m4": (lambda: ashut.direct_track(8, 50, 30), 4, 2, 64, 0),
    "bundle_m2": (lambda: ashut.bundle_track(6, 50, 30), 2, 2, 96, 0),
    "direct_first1": (lambda: ashut.direct_track(7, 50, 30), 2, 2, 96, 1),
    "mixed": (mixed_track, 2, 2, 64, 0),
}
# saturation: 256 values of 255 in the floor's red channel; both tiles refined (no flat tile: the full-width sum alone)
SATURATION = (lambda: ashut.bright_track(16, 16, 8), 16, 4, 32, 0)

_TRACKS = {}


def track(name):
    if name not in _TRACKS:
        _TRACKS[name] = (SATURATION if name == "saturation" else TRACKS[name])[0]()
    return _TRACKS[name]


def track_case(name):
    return (SATURATION if name == "saturation" else TRACKS[name])[1:]


def camera_subframes(oracle, sc, k, n_sub, H=None, view_h=None):
    """(cameras, plain [n_sub, H, W], samples [n_sub, k H, k W], stats, camera indices) of n_sub sub-frame cameras."""
    cams, order = pc.cycled(sc, n_sub)
    plain, big, stats = pc.path_frames(oracle, sc, k, H, view_h)
    return cams, plain[order], big[order], [stats[i] for i in order], order


def track_subframes(oracle, tr, k, first_frame=0, m=1):
    """(plain, samples, stats, scenes) of the track's sub-frames from first_frame on, whole output frames of m only."""
    plain, big, stats = pc.track_frames(oracle, tr, k)
    n = (len(tr) - first_frame) // m * m
    sl = slice(first_frame, first_frame + n)
    return plain[sl], big[sl], stats[sl], tr[sl]


def masks(plain_sub, m, T):
    """Per output frame: the refine mask of P_f, the factor-1 shutter frame."""
    return [refine_mask(p, T) for p in path.shutter_mean(plain_sub, m)]


def expected_primary(plain_sub, m, k, T):
    """m rays per output pixel and m (k^2 - 1) more per pixel of every refined tile, over the output frames."""
    return sum(m * (p.size + (k * k - 1) * int(pc.pixel_mask(p, T).sum())) for p in path.shutter_mean(plain_sub, m))


def traced_counts(oracle, scenes_, plain_sub, big_sub, stats, m, k, T):
    """The rays of the samples an adaptive shutter render traces: sample (0, 0) of every block of every sub-frame, and every
    sample of the blocks of the tiles P_f refines -- the mask of P_f applied to each of frame f's sub-frames."""
    mean = path.shutter_mean(plain_sub, m)
    return pc.traced_counts(oracle, scenes_, [mean[j // m] for j in range(len(plain_sub))], big_sub, stats, k, T)


def camera_scenes(sc, order):
    """The scene of each sub-frame camera, named as path_adaptive_cases.path_counts names them (one per-sample table each)."""
    import path_cases
    moved = path_cases.path_scenes(sc)
    moved[pc.N - 1] = moved[0]
    return [dataclasses.replace(moved[i], name=f"{sc.name}@cam{i % (pc.N - 1)}") for i in order]


def facts(plain_sub, big_sub, m, k, T):
    """Per output frame: (mask of P_f, [mask of each sub-frame's plain frame], pixels != P_f, pixels != S_f)."""
    out = shutter_adaptive_resolve(plain_sub, big_sub, k, m, T)
    mean, full = path.shutter_mean(plain_sub, m), path_resolve(big_sub, k, m)
    return [(refine_mask(mean[f], T), [refine_mask(plain_sub[f * m + s], T) for s in range(m)], int((out[f] != mean[f]).sum()),
             int((out[f] != full[f]).sum())) for f in range(len(mean))]
