"""Animated scenes (rt_set_scene_track / rt_render_anim*), the parts that need no GPU: raytracer_hip.anim.tween against
binary32 arithmetic done in numpy, its endpoints and its refusals, and the public surface (header, bindings)."""
import dataclasses
import os
import re

import numpy as np
import pytest

from raytracer_hip import abi, anim, scenes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32


def _keys():
    a = scenes.config("C3").resized(100, 60)
    sph = list(a.spheres)
    sph[0] = scenes.Sphere(scenes.vec(-2.75, 0.3, 6.1), sph[0].radius, sph[0].material)
    sph[1] = scenes.Sphere(sph[1].center, scenes.f32(sph[1].radius * 2), scenes.Material.metal(scenes.vec(0.1, 0.2, 0.9), 7.3))
    planes = [scenes.Plane(scenes.vec(0, -0.37, 0), scenes.vec(0, 0, 1), a.planes[0].material)]
    lights = [scenes.Light(scenes.vec(4.1, 2.7, -1.3), scenes.f32(0.61)), a.lights[1]]
    b = dataclasses.replace(a, name="C3b", spheres=sph, planes=planes, lights=lights,
                            ambient=scenes.vec(0.31, 0.07, 0.11), camera=((1.0, 2.0, 3.0), 0.5, 0.25))
    c = dataclasses.replace(b, name="C3c", ambient=a.ambient)
    return [a, b, c]


def test_endpoints_are_reproduced_exactly_and_m1_returns_the_keys():
    keys = _keys()
    assert anim.tween(keys, 1) == keys
    for m in (2, 3, 7):
        out = anim.tween(keys, m)
        assert len(out) == (len(keys) - 1) * m + 1
        for k, key in enumerate(keys):
            assert out[k * m] == key and out[k * m] is key


def test_tween_is_binary32_linear_interpolation():
    keys = _keys()
    m = 7
    out = anim.tween(keys, m)

    def lerp(a, b, w):  # a + (b - a) * w with every step rounded to binary32
        a, b = np.asarray(a, dtype=F), np.asarray(b, dtype=F)
        r = a + (b - a) * w
        assert r.dtype == F
        return r

    moved = 0
    for k in range(len(keys) - 1):
        a, b = keys[k], keys[k + 1]
        for s in range(1, m):
            w = F(s) / F(m)
            sc = out[k * m + s]
            for p, q, r in zip(a.spheres, b.spheres, sc.spheres):
                assert np.array_equal(np.asarray(r.center, dtype=F), lerp(p.center, q.center, w))
                assert F(r.radius) == lerp(p.radius, q.radius, w) and r.radius == float(F(r.radius))
                assert r.material is p.material
                moved += r.center != p.center or r.radius != p.radius
            for p, q, r in zip(a.planes, b.planes, sc.planes):
                assert np.array_equal(np.asarray(r.center, dtype=F), lerp(p.center, q.center, w))
                assert r.normal == p.normal and r.material is p.material
            for p, q, r in zip(a.lights, b.lights, sc.lights):
                assert np.array_equal(np.asarray(r.position, dtype=F), lerp(p.position, q.position, w))
                assert F(r.intensity) == lerp(p.intensity, q.intensity, w)
            assert np.array_equal(np.asarray(sc.ambient, dtype=F), lerp(a.ambient, b.ambient, w))
            assert sc.recursion_limit == a.recursion_limit and sc.camera == a.camera
            assert (sc.width, sc.height) == (a.width, a.height)
    assert moved >= 2 * (m - 1)  # (the first interval moves two spheres)


def test_mismatched_counts_and_limits_raise():
    a = _keys()[0]
    fewer = dataclasses.replace(a, spheres=list(a.spheres[:-1]))
    no_light = dataclasses.replace(a, lights=list(a.lights[:1]))
    more_planes = dataclasses.replace(a, planes=list(a.planes) * 2)
    deeper = dataclasses.replace(a, recursion_limit=a.recursion_limit + 1)
    for other in (fewer, no_light, more_planes, deeper):
        with pytest.raises(ValueError):
            anim.tween([a, other], 3)
        with pytest.raises(ValueError):
            anim.check_counts([a, a, other])
    with pytest.raises(ValueError):
        anim.tween([a, a], 0)
    assert anim.tween([], 4) == [] and anim.tween([a], 4) == [a]


def test_header_and_bindings_declare_the_entry_points():
    header = open(os.path.join(ROOT, "include", "raytracer_hip.h")).read()
    names = {n for n, _, _ in abi.EXPORTS}
    for name in ("rt_set_scene_track", "rt_clear_scene_track", "rt_render_anim_bands", "rt_render_anim"):
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
        assert name in names
    m = re.search(r"#define\s+RT_MAX_TRACK_BYTES\s+\(\(size_t\)1\s*<<\s*30\)", header)
    assert m and abi.RT_MAX_TRACK_BYTES == 1 << 30
    assert re.search(r"#define\s+RT_ABI_VERSION\s+10\b", header) and abi.RT_ABI_VERSION == 10
