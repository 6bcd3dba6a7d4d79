"""Animated scenes for Context.set_scene_track / render_anim: one scenes.Scene per frame.

`tween` is the scene counterpart of path.subframes (which supplies the cameras): between two key scenes the sphere
centres and radii, the plane centres, the light positions and intensities and the ambient move linearly, in binary32
as the C structs hold them; materials and plane normals are those of the earlier key.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import abi, scenes


def check_counts(track) -> None:
    """ValueError unless the scenes have equal sphere, plane and light counts and one recursion limit."""
    k = track[0]
    for i, sc in enumerate(track):
        if (len(sc.spheres), len(sc.planes), len(sc.lights)) != (len(k.spheres), len(k.planes), len(k.lights)):
            raise ValueError(f"scene {i} has {len(sc.spheres)} spheres, {len(sc.planes)} planes and {len(sc.lights)} "
                             f"lights; scene 0 has {len(k.spheres)}, {len(k.planes)} and {len(k.lights)}")
        if sc.recursion_limit != k.recursion_limit:
            raise ValueError(f"scene {i} has recursion limit {sc.recursion_limit}; scene 0 has {k.recursion_limit}")


def c_track(track):
    """rt_set_scene_track's arguments for a list of scenes: (spheres, n_spheres, planes, n_planes, lights, n_lights,
    ambients, recursion_limit, n_frames), the arrays frame-major.  ValueError for an empty list or unequal counts."""
    if not track:
        raise ValueError("a scene track needs at least one scene")
    check_counts(track)
    k = track[0]
    nS, nP, nL, n = len(k.spheres), len(k.planes), len(k.lights), len(track)
    S = (abi.rt_sphere * max(1, nS * n))()
    P = (abi.rt_plane * max(1, nP * n))()
    L = (abi.rt_light * max(1, nL * n))()
    A = (abi.rt_vec3 * n)()
    for f, sc in enumerate(track):
        s, p, l = sc.c_arrays()
        C.memmove(C.byref(S, f * nS * C.sizeof(abi.rt_sphere)), s, nS * C.sizeof(abi.rt_sphere))
        C.memmove(C.byref(P, f * nP * C.sizeof(abi.rt_plane)), p, nP * C.sizeof(abi.rt_plane))
        C.memmove(C.byref(L, f * nL * C.sizeof(abi.rt_light)), l, nL * C.sizeof(abi.rt_light))
        A[f] = abi.rt_vec3(*sc.ambient)
    return S, nS, P, nP, L, nL, A, k.recursion_limit, n


def lerp(a, b, w) -> float:
    """a + (b - a) * w, every step rounded to float32 (path.subframes' rule)."""
    f32 = np.float32
    return float(f32(f32(a) + f32(f32(f32(b) - f32(a)) * f32(w))))


def _lerp3(a, b, w) -> tuple:
    return tuple(lerp(x, y, w) for x, y in zip(a, b))


def tween(keys, m: int) -> list:
    """The frames of an animation over the key scenes: n keys -> (n - 1) * m + 1 scenes, frame s of interval k
    interpolated towards key k + 1 at w = float32(s) / float32(m).  Frame 0 of an interval is the key itself, and the
    last key closes the list, so both endpoints of every interval are reproduced exactly; m = 1 returns the keys.
    The camera, frame size and name stay those of the earlier key."""
    keys = list(keys)
    if m < 1:
        raise ValueError("m must be at least 1")
    if not keys:
        return []
    check_counts(keys)
    out = []
    for k in range(len(keys) - 1):
        a, b = keys[k], keys[k + 1]
        out.append(a)
        for s in range(1, m):
            w = np.float32(s) / np.float32(m)
            out.append(scenes.Scene(
                f"{a.name}+{s}/{m}", a.width, a.height,
                [scenes.Sphere(_lerp3(p.center, q.center, w), lerp(p.radius, q.radius, w), p.material)
                 for p, q in zip(a.spheres, b.spheres)],
                [scenes.Plane(_lerp3(p.center, q.center, w), p.normal, p.material) for p, q in zip(a.planes, b.planes)],
                [scenes.Light(_lerp3(p.position, q.position, w), lerp(p.intensity, q.intensity, w))
                 for p, q in zip(a.lights, b.lights)],
                _lerp3(a.ambient, b.ambient, w), a.recursion_limit, a.camera, a.note, dict(a.meta)))
    out.append(keys[-1])
    return out
