"""Shared by tests/test_path.py and tests/test_gpu_path.py: the camera path of the camera-path tests and its
oracle frames, one unchanged oracle render per camera."""
import dataclasses

import numpy as np

# (dyaw, dpitch, dx, dz) added to the scene's camera.  The last camera repeats the first on purpose: equal
# cameras in one launch must give equal frames, and a launch that reused frame 0's view for every frame would
# still get two frames right.
OFFSETS = [(0, 0, 0, 0), (0.35, 0, 0.5, 0), (-0.4, 0.1, -0.6, 0.3), (0, 0.25, 0, 1.0), (0.8, -0.1, 1.0, -0.5),
           (0, 0, 0, 0)]
DISTINCT = [0, 1, 2, 3, 4]  # indices of the pairwise different cameras


def _f32(x) -> float:
    return float(np.float32(x))


def moved(sc, off):
    """`sc` seen from its camera moved by one of OFFSETS (binary32 sums, as rt_camera holds them)."""
    dyaw, dpitch, dx, dz = off
    (px, py, pz), yaw, pitch = sc.camera
    cam = ((_f32(np.float32(px) + np.float32(dx)), _f32(py), _f32(np.float32(pz) + np.float32(dz))),
           _f32(np.float32(yaw) + np.float32(dyaw)), _f32(np.float32(pitch) + np.float32(dpitch)))
    return dataclasses.replace(sc, camera=cam)


def path_scenes(sc):
    return [moved(sc, off) for off in OFFSETS]


def cameras(sc):
    """The rt_camera of each frame of the test path over `sc`."""
    return [s.c_camera() for s in path_scenes(sc)]


_FRAMES = {}


def oracle_frames(oracle, sc, W=None, H=None, view_h=None):
    """(frames [6, H, W], [stats]) of the test path over `sc`: rows [0, H) of a view view_h rows high."""
    W, H = W or sc.width, H or sc.height
    key = (sc.name, W, H, view_h)
    if key not in _FRAMES:
        frames, stats = [], []
        for i, s in enumerate(path_scenes(sc)):
            if i == len(OFFSETS) - 1:  # the repeated camera
                frames.append(frames[0]), stats.append(stats[0])
                continue
            px, st = oracle.render(s.resized(W, view_h or H), oracle.MODE_NEAREST, 8, rows=(0, H))
            frames.append(px), stats.append(st)
        out = np.stack(frames)
        out.setflags(write=False)
        _FRAMES[key] = (out, stats)
    return _FRAMES[key]
