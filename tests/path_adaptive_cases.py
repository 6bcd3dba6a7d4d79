"""Shared by tests/test_path_adaptive.py (CPU) and tests/test_gpu_path_adaptive.py: the cases of adaptive supersampling in
the camera-path and scene-track renders (rt_set_path_adaptive_sampling) and their expectations from the definition,
supersample.path_adaptive_resolve of the unchanged oracle's plain and k W x k H frames.  Camera i of a list is
tests/path_cases.py's camera i % 6; every oracle render is computed once per process (path_cases / anim_cases) and shared
read-only.  The thresholds are held by tests/test_path_adaptive.py: at each of them every camera (every track frame) has
refined and flat tiles, the masks differ between cameras, and every expected frame differs from both the plain and the
fully supersampled one."""
import dataclasses

import numpy as np

import anim_cases
import path_cases
from raytracer_hip.supersample import TILE, path_adaptive_resolve, path_resolve, refine_mask
from test_gpu_supersample import SCENES

RAYS = ("primary_rays", "reflect_rays", "shadow_rays")
N = len(path_cases.OFFSETS)

# (scene of test_gpu_supersample.SCENES, W, H, T) at k = 2: every scene there, REF at 45 x 27 (at 13 x 7 both of its tiles
# are refined for some cameras) ...
PATH_K2 = [
    ("C3", 50, 30, 96),            # direct, LDS stack
    ("C4", 50, 30, 128),           # bundle, merged pass, clusters
    ("REF", 45, 27, 96),           # limit 32: the scratch stack; ragged in both axes
    ("gpow_direct", 50, 30, 96),
    ("gpow_bundle", 50, 30, 128),
    ("C1", 50, 30, 96),
    ("dense", 50, 30, 96),
    ("bundle_L5", 50, 30, 96),     # (camera 4 differs from full supersampling in one pixel, at every threshold)
]
# ... both families at the larger factors (64 passes fill the 16-bit sums; 50 x 30 has partly invalid edge tiles in both
# axes), 3 cameras at k = 8 ...
PATH_K48 = [("C3", 50, 30, 96, 4, 6), ("C4", 50, 30, 128, 4, 6), ("C3", 50, 30, 96, 8, 3), ("C4", 50, 30, 128, 8, 3)]
# ... and the frame of the band, view-height, chunk, stream and context tests
W0, H0, T0 = 50, 30, 96
VIEW_ROWS = 27  # rendered rows of the 30-row view: the last tile row is cut at 3 rows

# scene tracks: name -> (builder, T)
TRACKS = {
    "direct": (lambda: anim_cases.direct_track(W0, H0), 96),
    "bundle": (lambda: anim_cases.bundle_track(W0, H0), 128),
    # (the direct track's scenes all seen from frame 0's camera: the masks can differ through the scenes alone)
    "one_camera": (lambda: [dataclasses.replace(sc, camera=track("direct")[0].camera, name=f"{sc.name}_cam0")
                            for sc in track("direct")[:5]], 96),
    "mixed_s8": (lambda: mixed_track("s8"), 64),
    "mixed_s12": (lambda: mixed_track("s12"), 64),
}


def mixed_track(cls):
    """3 frames of a class's scene, frame 2 with specular exponent 7.3: a track mixing GPOW and other frames."""
    base, g = anim_cases.class_track(cls, False, 3), anim_cases.class_track(cls, True, 3)
    return [dataclasses.replace((g[f] if f == 2 else sc).resized(W0, H0), name=f"{sc.name}_expmix_pa") for f, sc in enumerate(base)]


_SCENES = {}
_TRACKS = {}


def scene(cid, W, H):
    if (cid, W, H) not in _SCENES:
        _SCENES[(cid, W, H)] = SCENES[cid]().resized(W, H)
    return _SCENES[(cid, W, H)]


def track(name):
    if name not in _TRACKS:
        _TRACKS[name] = TRACKS[name][0]()
    return _TRACKS[name]


def cycled(sc, n, start=0):
    """n cameras: camera i is the test path's camera (start + i) % 6; and their indices."""
    cams = path_cases.cameras(sc)
    order = [(start + i) % N for i in range(n)]
    return [cams[i] for i in order], order


def pixel_mask(plain, T):
    """bool [H, W]: the pixels of the refined tiles."""
    m = refine_mask(plain, T)
    return np.repeat(np.repeat(m, TILE, axis=0), TILE, axis=1)[:plain.shape[0], :plain.shape[1]]


def path_frames(oracle, sc, k, H=None, view_h=None):
    """(plain [6, H, W], samples [6, k H, k W], the sample frames' stats) of the test path over `sc`."""
    W, H = sc.width, H or sc.height
    plain = path_cases.oracle_frames(oracle, sc, W, H, view_h)[0]
    big, stats = path_cases.oracle_frames(oracle, sc, k * W, k * H, k * view_h if view_h else None)
    return plain, big, stats


def expected(oracle, sc, order, k, T, H=None, view_h=None):
    """The definition's frames [len(order), H, W] at threshold T (0: full supersampling)."""
    plain, big, _ = path_frames(oracle, sc, k, H, view_h)
    return path_adaptive_resolve(plain[order], big[order], k, T)


def expected_primary(plain_frames, k, T):
    """One primary ray per pixel and k^2 - 1 more per pixel of every refined tile, over the frames."""
    return sum(p.size + (k * k - 1) * int(pixel_mask(p, T).sum()) for p in plain_frames)


_SEGS = {}


def _per_sample(oracle, sc, big, st):
    """[primary, reflect, shadow] rays per sample of the oracle's frame `big` of `sc` (at big's size), whose totals are
    first held against oracle.render's counts."""
    key = (sc.name, big.shape)
    if key not in _SEGS:
        seg = oracle.segments(sc.resized(big.shape[1], big.shape[0]), 1)
        per = [np.bincount(seg["pixel"][seg["kind"] == kind], minlength=big.size).reshape(big.shape) for kind in (0, 1, 2)]
        assert [int(p.sum()) for p in per] == [st[r] for r in RAYS], "the per-sample segments add up to the oracle's counts"
        assert (per[0] == 1).all()
        _SEGS[key] = per
    return _SEGS[key]


def traced_counts(oracle, scenes_, plain_frames, big_frames, stats, k, T):
    """primary / reflect / shadow rays of the samples an adaptive render traces -- sample (0, 0) of every block and every
    sample of the refined tiles' blocks -- summed over the frames (frame f: scene scenes_[f] with its own camera)."""
    total = dict.fromkeys(RAYS, 0)
    for sc, plain, big, st in zip(scenes_, plain_frames, big_frames, stats):
        traced = np.repeat(np.repeat(pixel_mask(plain, T), k, axis=0), k, axis=1)
        traced[::k, ::k] = True
        for r, p in zip(RAYS, _per_sample(oracle, sc, big, st)):
            total[r] += int(p[traced].sum())
    return total


def path_counts(oracle, sc, order, k, T):
    plain, big, stats = path_frames(oracle, sc, k)
    moved = path_cases.path_scenes(sc)
    moved[N - 1] = moved[0]  # (the repeated camera: one oracle render, one name)
    return traced_counts(oracle, [dataclasses.replace(moved[i], name=f"{sc.name}@cam{i % (N - 1)}") for i in order], plain[order],
                         big[order], [stats[i] for i in order], k, T)


def track_frames(oracle, tr, k):
    """(plain [n, H, W], samples [n, k H, k W], stats) of a track, each frame in its own scene from its own camera."""
    W, H = tr[0].width, tr[0].height
    plain = anim_cases.oracle_frames(oracle, tr, W, H)[0]
    big, stats = anim_cases.oracle_frames(oracle, tr, k * W, k * H)
    return plain, big, stats


def facts(plain_frames, big_frames, k, T):
    """Per frame: (refine mask, pixels != plain, pixels != full supersampling) of the definition's output."""
    out = path_adaptive_resolve(plain_frames, big_frames, k, T)
    full = path_resolve(big_frames, k, 1)
    return [(refine_mask(p, T), int((o != p).sum()), int((o != f).sum())) for p, o, f in zip(plain_frames, out, full)]
