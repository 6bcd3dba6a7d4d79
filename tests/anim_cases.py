"""Shared by tests/test_gpu_anim.py: the scene tracks of the animated-scene tests and their oracle frames, one unchanged
oracle render per frame (that frame's scene and camera), cached per module run and shared read-only."""
import dataclasses

import numpy as np

import path_cases
from raytracer_hip import anim, scenes

RAYS = ("primary_rays", "reflect_rays", "shadow_rays")
ORIGIN_LIGHT = scenes.Light(scenes.vec(0, 0, 0), 1.0)  # 2a = 0: the shadow loops without the exact threshold


def named(track, prefix):
    return [dataclasses.replace(sc, name=f"{prefix}#{f}") for f, sc in enumerate(track)]


def with_path_cameras(track):
    """Frame f seen from its scene's camera moved by path_cases.OFFSETS[f]."""
    return [path_cases.moved(sc, path_cases.OFFSETS[f % len(path_cases.OFFSETS)]) for f, sc in enumerate(track)]


def direct_track(W=100, H=60):
    """C3's scene (the direct family), 6 frames, the last repeating frame 0's scene and camera.  From frame 0 to 4
    sphere 1 crosses from x = 3 to x = -3 at z = 5 (more than a third of the frame's width), sphere 0's radius doubles,
    light 0 sweeps the shadows over the floor, the floor rises and the ambient changes."""
    a = scenes.config("C3").resized(W, H)
    sph = list(a.spheres)
    sph[0] = scenes.Sphere(sph[0].center, scenes.f32(2 * sph[0].radius), sph[0].material)
    sph[1] = scenes.Sphere(scenes.vec(-3, 0, 5), sph[1].radius, sph[1].material)
    planes = [scenes.Plane(scenes.vec(0, -0.5, 0), a.planes[0].normal, a.planes[0].material)] + list(a.planes[1:])
    lights = [scenes.Light(scenes.vec(5, 6, -3), scenes.f32(0.8))] + list(a.lights[1:])
    b = dataclasses.replace(a, spheres=sph, planes=planes, lights=lights, ambient=scenes.vec(0.3, 0.1, 0.05))
    frames = anim.tween([a, b], 4)
    return named(with_path_cameras(frames + [frames[0]]), f"anim_direct_{W}x{H}")


def bundle_track(W=64, H=40):
    """C4's scene (64 spheres, 4 lights, limit 6: the bundle family with shadow grids and clusters), 4 frames: half the
    spheres and two lights move."""
    a = scenes.config("C4").resized(W, H)
    sph = [scenes.Sphere(scenes.vec(s.center[0] + (1.5 if i % 4 else -2.0), s.center[1] + 0.25 * (i % 3), s.center[2] - 1.0),
                         scenes.f32(s.radius * 1.25), s.material) if i % 2 else s for i, s in enumerate(a.spheres)]
    lights = [scenes.Light(scenes.vec(l.position[0] + 4, l.position[1] + 1, l.position[2] - 3), l.intensity) if i < 2 else l
              for i, l in enumerate(a.lights)]
    b = dataclasses.replace(a, spheres=sph, lights=lights)
    return named(with_path_cameras(anim.tween([a, b], 3)), f"anim_bundle_{W}x{H}")


# The variant sweep: sphere count (and lights) -> the kernel family and class the launch selects.
CLASS_W, CLASS_H = 32, 24
LIMITS = [0, 1, 3, 5, 7, 8]  # K = 1, 2, 4, 6, 8 and 64 (the scratch stack)
FIFTH_LIGHT = scenes.Light(scenes.vec(6, 9, -2), scenes.f32(0.6))
# name -> (spheres, planes, lights, (family, cls))
CLASSES = {
    "s0": (0, scenes.REF_PLANES, scenes.REF_LIGHTS, ("direct", 8)),
    "s3": (3, scenes.REF_PLANES, scenes.REF_LIGHTS, ("direct", 8)),
    "s8": (8, scenes.REF_PLANES, scenes.REF_LIGHTS, ("direct", 8)),
    "s11": (11, scenes.REF_PLANES, scenes.REF_LIGHTS, ("direct", 0)),
    "s12": (12, scenes.C4_PLANES, scenes.C4_LIGHTS[:2], ("bundle", 2)),
    "s12_origin": (12, scenes.C4_PLANES, [scenes.C4_LIGHTS[0], ORIGIN_LIGHT], ("bundle", 1)),
    "s64": (64, scenes.C4_PLANES, scenes.C4_LIGHTS, ("bundle", 2)),
    "s70": (70, scenes.C4_PLANES, scenes.C4_LIGHTS[:3], ("bundle", 0)),  # above 64 spheres: a shadow pass per light
}


def stack_size(limit):
    return next(k for k in (1, 2, 4, 6, 8, 64) if limit + 1 <= k)


def descriptor(cls, gpow, limit):
    """(family, gpow, class, K) of the ANIM instantiation a track of this class runs (rt_internal.h pick_trace_variant)."""
    family, c = CLASSES[cls][3]
    return (family, bool(gpow), c, stack_size(limit))


def class_track(cls, gpow, limit):
    """3 frames of a class's scene: every sphere and light 0 move, every third sphere grows.  Specular exponent 2 on
    every second sphere, or 7.3 (the Math.Pow instantiations)."""
    n, planes, lights, _ = CLASSES[cls]
    n_exp = 7.3 if gpow else 2.0
    base = scenes.generated_spheres(max(n, 3))[:n]
    base = [scenes.Sphere(s.center, s.radius, scenes.Material.metal(s.material.kd if any(s.material.kd) else (0.7, 0.6, 0.5), n_exp))
            if i % 2 == 0 else s for i, s in enumerate(base)]
    a = scenes.Scene(f"anim_{cls}", CLASS_W, CLASS_H, base, list(planes), list(lights), scenes.REF_AMBIENT, limit)
    sph = [scenes.Sphere(scenes.vec(s.center[0] + 0.75, s.center[1] + (0.5 if i % 2 else 0.0), s.center[2] - 0.5),
                         scenes.f32(s.radius * (1.5 if i % 3 == 0 else 1.0)), s.material) for i, s in enumerate(base)]
    l0 = lights[0]
    moved = [scenes.Light(scenes.vec(l0.position[0] + 3, l0.position[1] + 2, l0.position[2] + 1), l0.intensity)] + list(lights[1:])
    b = dataclasses.replace(a, spheres=sph, lights=moved, ambient=scenes.vec(0.05, 0.2, 0.25))
    return named(with_path_cameras(anim.tween([a, b], 2)), f"anim_{cls}_{'gpow' if gpow else 'pow'}_lim{limit}")


_FRAMES = {}


def oracle_frames(oracle, track, W=None, H=None, view_h=None):
    """(frames [n, H, W], [stats]) of the track: frame f = rows [0, H) of the oracle's render of scene f from its own
    camera on a view view_h rows high."""
    W, H = W or track[0].width, H or track[0].height
    frames, stats = [], []
    for sc in track:
        key = (sc.name, W, H, view_h)
        if key not in _FRAMES:
            px, st = oracle.render(sc.resized(W, view_h or H), oracle.MODE_NEAREST, 8, rows=(0, H))
            px.setflags(write=False)
            _FRAMES[key] = (px, {r: st[r] for r in RAYS})
        frames.append(_FRAMES[key][0]), stats.append(_FRAMES[key][1])
    out = np.stack(frames)
    out.setflags(write=False)
    return out, stats


def summed(stats):
    return {r: sum(s[r] for s in stats) for r in RAYS}
