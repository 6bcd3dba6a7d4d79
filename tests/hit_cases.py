"""Shared by tests/test_hits.py and tests/test_gpu_hits.py: the reference for the hit buffers (rt_render_hits*, rt_pick)
and the scenes they are checked on.

expected_hits builds the four channels in numpy binary32 from tests/emu_f32.py's primitives -- Emu.camera, the primary
ray of Emu.render, isect_sphere, isect_plane, normalize -- and TracePixel's selection rule (RayTracer.cs:973-993):
spheres take `dist > 0 && best > dist` in scene order, planes likewise, and the sphere wins iff best_s < best_p.
tests/test_hits.py pins it to the unchanged oracle; the GPU tests compare against it bit for bit.  Each case is
computed once and shared read-only."""
import dataclasses

import numpy as np

from emu_f32 import V3, Emu, f32, normalize
from random_scenes import random_scene
from raytracer_hip import abi, scenes

CHANNELS = ("depth", "object", "position", "normal")
_EXPECTED = {}


def _stack(v):
    return np.stack([v.x, v.y, v.z], axis=-1).astype(f32)


def primary_rays(scene, rows=None):
    """(origin V3, direction V3) of the pixels of rows [0, rows) of the scene's W x H view, row-major (:963-971)."""
    em = Emu(scene)
    W, H = scene.width, scene.height
    cam, R, U, F, vp = em.camera()
    ys, xs = np.mgrid[0:(rows or H), 0:W]
    xs, ys = xs.ravel(), ys.ravel()
    px = xs.astype(f32) / f32(W) - f32(0.5)
    py = ys.astype(f32) / f32(H) - f32(0.5)
    n = xs.size
    local = V3(px, py, np.full(n, f32(1))).mul(vp)
    point = ((cam.bcast(n) + R.scale(local.x)) + U.scale(local.y)) + F.scale(local.z)
    return cam.bcast(n), normalize(point - cam.bcast(n))


def expected_hits(scene, rows=None):
    """{"depth" f32[h, W], "object" i32[h, W], "position" f32[h, W, 3], "normal" f32[h, W, 3]} of rows [0, rows) (all
    of them by default) of the scene's own W x H view from its own camera."""
    key = (scene.name, scene.width, scene.height, rows, scene.camera)
    if key in _EXPECTED:
        return _EXPECTED[key]
    em = Emu(scene)
    W, h = scene.width, rows or scene.height
    o, d = primary_rays(scene, rows)
    n = W * h
    best_s, win_s = np.full(n, np.inf, f32), np.full(n, -1, np.int32)
    for i, (c, r2, _m) in enumerate(em.spheres):
        _, dist = em.isect_sphere(o, d, c, r2)
        sel = (dist > 0) & (best_s > dist)
        best_s, win_s = np.where(sel, dist, best_s).astype(f32), np.where(sel, i, win_s).astype(np.int32)
    best_p, win_p = np.full(n, np.inf, f32), np.full(n, -1, np.int32)
    for j, (c, nrm, _m) in enumerate(em.planes):
        _, dist = em.isect_plane(o, d, c, nrm)
        sel = (dist > 0) & (best_p > dist)
        best_p, win_p = np.where(sel, dist, best_p).astype(f32), np.where(sel, j, win_p).astype(np.int32)
    sphere = best_s < best_p
    plane = ~sphere & (win_p >= 0)
    none = ~sphere & ~plane
    depth = np.where(sphere, best_s, np.where(plane, best_p, f32(np.inf))).astype(f32)
    obj = np.where(sphere, win_s, np.where(plane, len(em.spheres) + win_p, abi.RT_HIT_NONE)).astype(np.int32)
    pos = o + d.scale(np.where(none, f32(100), depth).astype(f32))
    normal = np.zeros((n, 3), f32)
    if em.spheres:
        cx, cy, cz = (np.array([getattr(c, a) for c, _r, _m in em.spheres], f32) for a in "xyz")
        k = np.where(sphere, win_s, 0)
        with np.errstate(all="ignore"):
            ns = _stack(normalize(pos - V3(cx[k], cy[k], cz[k])))
        normal = np.where(sphere[:, None], ns, normal)
    if em.planes:
        pn = np.array([[nrm.x, nrm.y, nrm.z] for _c, nrm, _m in em.planes], f32)
        normal = np.where(plane[:, None], pn[np.where(plane, win_p, 0)], normal)
    out = {"depth": depth.reshape(h, W), "object": obj.reshape(h, W), "position": _stack(pos).reshape(h, W, 3),
           "normal": normal.astype(f32).reshape(h, W, 3)}
    for a in out.values():
        a.setflags(write=False)
    _EXPECTED[key] = out
    return out


def bits(a):
    """The uint32 patterns of a float32 or int32 array: NaN payloads and the sign of zero compare too."""
    return np.ascontiguousarray(a).view(np.uint32)


def with_camera(scene, cam):
    """`scene` seen from an abi.rt_camera."""
    return dataclasses.replace(scene, camera=(cam.position.tuple(), cam.yaw, cam.pitch))


# ---- the cases: (scene, rows) -- rows: the frame's height when the view is higher (rt_set_view_height), else None ----
def _scene(name, W, H, spheres, planes, camera=(scenes.ZERO, 0.0, 0.0), limit=2):
    return scenes.Scene(name, W, H, list(spheres), list(planes), list(scenes.REF_LIGHTS), scenes.REF_AMBIENT, limit, camera)


DENSE_SEEDS = (3, 6)


def cases():
    out = [(scenes.reference(64, 64).resized(64, 64, "hits_ref"), None)]
    out += [(scenes.config(c).resized(w, h, f"hits_{c}"), None) for c, w, h in (("C2", 96, 54), ("C3", 96, 54), ("C4", 64, 36))]
    out += [(dataclasses.replace(random_scene(s, 40, 24, dense=s in DENSE_SEEDS), name=f"hits_rand{s}"), None) for s in range(8)]
    # past the 64-bit box mask: no primary constants, the pair loop over the padded table
    out.append((_scene("hits_s80", 48, 32, scenes.generated_spheres(80), scenes.C4_PLANES), None))
    # the camera inside sphere 0 (its near root is behind the ray: the reference sees through it)
    inside = [scenes.Sphere(scenes.vec(0, 0, 0.5), 2.0, scenes.Material.diffuse(scenes.vec(1, 0, 0)))] + list(scenes.REF_SPHERES)
    out.append((_scene("hits_inside", 40, 24, inside, scenes.REF_PLANES), None))
    # 0.005 above the floor, looking down: selected hits with t - 0.01 <= 0 (black in the colour frame)
    out.append((_scene("hits_near_plane", 40, 24, scenes.REF_SPHERES, scenes.REF_PLANES,
                       camera=(scenes.vec(0, -0.995, 0), 0.0, scenes.f32(1.45))), None))
    # a wall whose normal is perpendicular to the view direction: the centre column's denominator is 0
    wall = scenes.Plane(scenes.vec(2, 0, 0), scenes.vec(1, 0, 0), scenes.Material.diffuse(scenes.vec(0.5, 0.5, 1)))
    out.append((_scene("hits_parallel_plane", 40, 24, scenes.REF_SPHERES, list(scenes.REF_PLANES) + [wall]), None))
    out.append((_scene("hits_no_planes", 40, 24, scenes.generated_spheres(8), []), None))
    out.append((_scene("hits_no_spheres", 40, 24, [], scenes.C4_PLANES), None))
    # rt_set_view_height above the height: rows [0, 40) of a 64 x 64 view
    out.append((scenes.reference(64, 64).resized(64, 64, "hits_view_height"), 40))
    return out


CASES = cases()
CASE_IDS = [sc.name for sc, _rows in CASES]
