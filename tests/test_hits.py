"""The hit buffers' reference (tests/hit_cases.py expected_hits) pinned to the unchanged oracle, so that the GPU tests of
tests/test_gpu_hits.py compare against oracle-anchored values; and the entry points' NULL-context refusals.  No device."""
import ctypes as C

import numpy as np
import pytest

import hit_cases
from hit_cases import bits, expected_hits, primary_rays
from raytracer_hip import abi

KIND_PRIMARY = 0


@pytest.fixture(scope="module")
def segments(oracle):
    cache = {}

    def get(scene):
        if scene.name not in cache:
            cache[scene.name] = oracle.segments(scene, 1)
        return cache[scene.name]
    return get


def _vec(seg, prefix):
    """The origin ("o") or end ("e") of segment records as float32[n, 3]."""
    return np.stack([seg[prefix + "x"], seg[prefix + "y"], seg[prefix + "z"]], axis=-1).astype(np.float32)


def _first_primary(seg, n_pixels):
    """Index of each pixel's first kind-0 record."""
    idx = np.nonzero(seg["kind"] == KIND_PRIMARY)[0]
    first = np.full(n_pixels, -1, np.int64)
    pix = seg["pixel"][idx]
    first[pix[::-1]] = idx[::-1]  # (the earliest record of a pixel is written last)
    assert (first >= 0).all(), "every pixel has a primary record at stride 1"
    return first


@pytest.mark.parametrize("scene,rows", hit_cases.CASES, ids=hit_cases.CASE_IDS)
def test_expected_hits_match_the_oracles_primary_segments(oracle, segments, scene, rows):
    W, h = scene.width, rows or scene.height
    n = W * h
    want = expected_hits(scene, rows)
    seg = segments(scene)
    first = _first_primary(seg, scene.width * scene.height)[:n]
    end = _vec(seg, "e")[first].reshape(h, W, 3)
    assert np.array_equal(bits(want["position"]), bits(end)), "position is the end of the pixel's primary segment"

    # nothing selected <=> the segment ends at origin + 100 direction, and then depth is +inf
    o, d = primary_rays(scene, rows)
    far = hit_cases._stack(o + d.scale(np.float32(100))).reshape(h, W, 3)
    none = want["object"] == abi.RT_HIT_NONE
    assert np.array_equal(none, (bits(end) == bits(far)).all(axis=-1))
    assert np.array_equal(none, np.isposinf(want["depth"]))
    assert (want["normal"][none] == 0).all()

    # the record after the primary one, when it is the same pixel's (kind 1 or 2), starts at the hit point
    nxt = np.minimum(first + 1, len(seg) - 1)
    same = (first + 1 < len(seg)) & (seg["pixel"][nxt] == np.arange(n)) & (seg["kind"][nxt] != KIND_PRIMARY)
    origin = _vec(seg, "o")[nxt].reshape(h, W, 3)
    m = same.reshape(h, W)
    assert np.array_equal(bits(origin[m]), bits(want["position"][m]))
    assert not (m & none).any()


@pytest.mark.parametrize("scene,rows", hit_cases.CASES, ids=hit_cases.CASE_IDS)
def test_depth_is_the_oracles_intersection_distance(oracle, scene, rows):
    """Every 7th pixel: oracle_intersect_sphere / _plane of the reported object with the pixel's ray returns depth."""
    lib = oracle.lib()
    W, h = scene.width, rows or scene.height
    want = expected_hits(scene, rows)
    o, d = primary_rays(scene, rows)
    v3 = lambda v, i: abi.rt_vec3(float(v.x[i]), float(v.y[i]), float(v.z[i]))
    obj, depth = want["object"].ravel(), want["depth"].ravel()
    checked = 0
    for i in range(0, W * h, 7):
        if obj[i] == abi.RT_HIT_NONE:
            continue
        hit = C.c_int(0)
        if obj[i] < len(scene.spheres):
            s = scene.spheres[obj[i]]
            t = lib.oracle_intersect_sphere(v3(o, i), v3(d, i), abi.rt_vec3(*s.center), s.radius, 0.0, C.byref(hit))
        else:
            p = scene.planes[obj[i] - len(scene.spheres)]
            t = lib.oracle_intersect_plane(v3(o, i), v3(d, i), abi.rt_vec3(*p.center), abi.rt_vec3(*p.normal), C.byref(hit))
        assert hit.value and bits(np.float32(t)) == bits(depth[i]), f"pixel {i}: object {obj[i]}"
        checked += 1
    assert checked or (obj == abi.RT_HIT_NONE).all()


@pytest.mark.parametrize("scene,rows", hit_cases.CASES, ids=hit_cases.CASE_IDS)
def test_pixels_without_a_shadeable_hit_are_black(oracle, scene, rows):
    want = expected_hits(scene, rows)
    px, _ = oracle.render(scene, oracle.MODE_NEAREST, 8, rows=(0, rows or scene.height))
    with np.errstate(invalid="ignore"):
        black = (want["object"] == abi.RT_HIT_NONE) | (want["depth"] - np.float32(0.01) <= 0)
    assert (px[black] == 0).all()


def test_the_cases_cover_what_they_are_there_for():
    by = {sc.name: (sc, rows) for sc, rows in hit_cases.CASES}
    near = expected_hits(*by["hits_near_plane"])
    sel = near["object"] != abi.RT_HIT_NONE
    assert (sel & (near["depth"] - np.float32(0.01) <= 0)).any(), "a selected hit with t - 0.01 <= 0"
    inside = expected_hits(*by["hits_inside"])
    assert not (inside["object"] == 0).any() and (inside["object"] > 0).any(), "the sphere around the camera is seen through"
    s80 = expected_hits(*by["hits_s80"])
    assert (s80["object"][s80["object"] < 80] >= 64).any(), "a sphere past the 64-bit box mask is visible"
    assert len(by["hits_no_planes"][0].planes) == 0 and len(by["hits_no_spheres"][0].spheres) == 0
    assert sum(len(sc.spheres) >= 12 for sc, _ in hit_cases.CASES if sc.name.startswith("hits_rand")) == len(hit_cases.DENSE_SEEDS)
    for sc, rows in hit_cases.CASES:
        hits = expected_hits(sc, rows)
        kinds = {"none": (hits["object"] == abi.RT_HIT_NONE).any()}
        assert hits["depth"].shape == (rows or sc.height, sc.width) and hits["normal"].shape[-1] == 3, kinds


def test_null_context_is_refused_by_every_hit_entry_point(rtlib):
    bufs = abi.rt_hit_buffers()
    cams = (abi.rt_camera * 1)()
    pick = abi.rt_pick_result()
    calls = [rtlib.rt_render_hits_device(None, 8, 8, C.byref(bufs), None),
             rtlib.rt_render_path_hits_device(None, 8, 8, cams, 1, C.byref(bufs), None),
             rtlib.rt_render_anim_hits_device(None, 8, 8, cams, 0, 1, C.byref(bufs), None),
             rtlib.rt_render_hits(None, 8, 8, C.byref(bufs)),
             rtlib.rt_render_path_hits(None, 8, 8, cams, 1, C.byref(bufs)),
             rtlib.rt_render_anim_hits(None, 8, 8, cams, 0, 1, C.byref(bufs)),
             rtlib.rt_pick(None, 8, 8, 0, 0, C.byref(pick))]
    assert calls == [abi.RT_ERR_INVALID_ARG] * 7
    assert abi.RT_HIT_NONE == -1 and C.sizeof(abi.rt_pick_result) == 32 and C.sizeof(abi.rt_hit_buffers) == 4 * C.sizeof(C.c_void_p)
