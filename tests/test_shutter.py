"""The camera-path shutter (rt_render_shutter_bands / rt_render_shutter), the parts that need no GPU: known answers
of raytracer_hip.path.shutter_mean (the numpy reference of the in-kernel resolve, which tests/test_gpu_shutter.py
compares the GPU against), the properties of path.subframes, the public surface (header, bindings, exports), and
the precondition of the GPU tests -- the mean of two distinct oracle frames differs from both of them, so a kernel
that stored one sub-frame instead of the mean cannot pass."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import path_cases
from raytracer_hip import abi, path, scenes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _frames(values):
    """One 1x1 frame per value."""
    return np.array(values, dtype=np.int32).reshape(len(values), 1, 1)


def _mean(values):
    out = path.shutter_mean(_frames(values), len(values))
    assert out.shape == (1, 1, 1) and out.dtype == np.int32
    return int(out[0, 0, 0])


@pytest.mark.parametrize("shift", [0, 8, 16])
def test_shutter_mean_known_answers_per_channel(shift):
    s = lambda v: [x << shift for x in v]  # noqa: E731
    assert _mean(s([0, 255])) == 128 << shift, "(0 + 255 + 1) >> 1: a half rounds up"
    assert _mean(s([0, 0, 0, 1])) == 0, "(1 + 2) >> 2"
    assert _mean(s([1, 1, 1, 0])) == 1 << shift, "(3 + 2) >> 2"
    assert _mean(s([255] * 256)) == 255 << shift, "(256 * 255 + 128) >> 8: the field's capacity"
    assert _mean(s([7])) == 7 << shift, "m = 1 is the frame itself"


def test_shutter_mean_never_leaks_between_channels():
    # G sums to 256 * 255 while R and B stay 0, then each of the others alone: the neighbours stay 0
    for shift in (0, 8, 16):
        got = _mean([255 << shift] * 256)
        assert got == 255 << shift
        got = _mean([255 << shift, 255 << shift, 255 << shift, 254 << shift])
        assert got == 255 << shift, "(1019 + 2) >> 2 = 255: no carry into the channel above"
    # all three channels at once, each with its own rounding: R (0 + 255), G (1 + 2), B (255 + 255)
    assert _mean([0x0001FF, 0xFF02FF]) == (128 << 16) | (2 << 8) | 255


def test_shutter_mean_shapes_and_grouping():
    rng = np.random.default_rng(5)
    fr = rng.integers(0, 1 << 24, size=(8, 3, 5), dtype=np.int64).astype(np.int32)
    out = path.shutter_mean(fr, 4)
    assert out.shape == (2, 3, 5)
    for f in range(2):
        for sh in (0, 8, 16):
            ch = ((fr[4 * f:4 * f + 4].astype(np.int64) >> sh) & 255).sum(axis=0)
            assert np.array_equal((out[f] >> sh) & 255, (ch + 2) // 4)
    assert np.array_equal(path.shutter_mean(fr, 1), fr)
    for bad in (0, 3, 6):
        with pytest.raises(ValueError):
            path.shutter_mean(fr, bad)
    with pytest.raises(ValueError):
        path.shutter_mean(fr[:6], 4)


def _cam_tuple(c):
    return (c.position.x, c.position.y, c.position.z, c.yaw, c.pitch)


def test_subframes_properties():
    sc = scenes.config("C3")
    keys = path_cases.cameras(sc)
    for m in (1, 2, 4, 8):
        sub = path.subframes(keys, m)
        assert len(sub) == len(keys) * m
        for k, key in enumerate(keys):
            assert _cam_tuple(sub[k * m]) == _cam_tuple(key), "sub-frame 0 is the key"
        assert all(_cam_tuple(c) == _cam_tuple(keys[-1]) for c in sub[-m:]), "the last key holds"
    assert [_cam_tuple(c) for c in path.subframes(keys, 1)] == [_cam_tuple(k) for k in keys]
    assert all(a is not b for a, b in zip(path.subframes(keys, 1), keys)), "copies, not the keys themselves"
    # the interpolation, in binary32: half-way between keys 0 and 1
    f32 = np.float32
    a, b = keys[0], keys[1]
    mid = path.subframes(keys, 2)[1]
    assert mid.yaw == float(f32(f32(a.yaw) + f32(f32(f32(b.yaw) - f32(a.yaw)) * f32(0.5))))
    assert mid.position.x == float(f32(f32(a.position.x) + f32(f32(f32(b.position.x) - f32(a.position.x)) * f32(0.5))))
    assert min(a.yaw, b.yaw) < mid.yaw < max(a.yaw, b.yaw)
    with pytest.raises(ValueError):
        path.subframes(keys, 0)


def test_header_bindings_and_library_agree(rtlib):
    hdr = open(os.path.join(ROOT, "include", "raytracer_hip.h")).read()
    assert re.search(r"int rt_render_shutter_bands\(rt_ctx\* ctx, int width, int height, const rt_camera\* cameras, "
                     r"int n_frames,\s+int shutter, int band_rows, int band_first, int band_step, void\* d_out,\s+"
                     r"size_t frame_stride_bytes, int format, void\* hip_stream, int\* out_n_bands\);", hdr)
    assert re.search(r"int rt_render_shutter\(rt_ctx\* ctx, int width, int height, const rt_camera\* cameras, "
                     r"int n_frames,\s+int shutter, int32_t\* pixels\);", hdr)
    assert re.search(r"#define RT_MAX_SHUTTER (\d+)", hdr).group(1) == str(abi.RT_MAX_SHUTTER) == "256"
    assert re.search(r"#define RT_ABI_VERSION (\d+)", hdr).group(1) == "10", "no ABI bump"
    assert rtlib.rt_abi_version() == 10 == abi.RT_ABI_VERSION
    names = [e[0] for e in abi.EXPORTS]
    assert "rt_render_shutter_bands" in names and "rt_render_shutter" in names
    # the built library exports both (abi.load_library binds every entry of EXPORTS by name)
    assert rtlib.rt_render_shutter.argtypes == [C.c_void_p, C.c_int, C.c_int, C.POINTER(abi.rt_camera), C.c_int, C.c_int,
                                                C.c_void_p]
    assert len(rtlib.rt_render_shutter_bands.argtypes) == 14
    assert C.CDLL(abi.LIB_PATH).rt_render_shutter_bands is not None


def test_null_context_and_bad_shutters_are_invalid_arguments(rtlib):
    cams = path.as_array([scenes.config("C1").c_camera()] * 4)
    buf = (C.c_int32 * 64)()
    nb = C.c_int(7)
    for shutter in (1, 2, 4):
        assert rtlib.rt_render_shutter_bands(None, 4, 4, cams, 1, shutter, 4, 0, 1, buf, 64, abi.RT_BANDS_INT32, None,
                                             C.byref(nb)) == abi.RT_ERR_INVALID_ARG
        assert rtlib.rt_render_shutter(None, 4, 4, cams, 1, shutter, buf) == abi.RT_ERR_INVALID_ARG
    assert nb.value == 7 and all(v == 0 for v in buf)


# The m = 2 mean of two distinct oracle frames must differ from each of them in at least 1 % of the pixels (C3 at
# 50 x 30, consecutive cameras of tests/path_cases.py).  Cameras 4 and 5 are distinct too (5 repeats 0, not 4).
def test_teeth_the_mean_of_two_distinct_frames_is_neither_of_them(oracle):
    sc = scenes.config("C3").resized(50, 30)
    frames, _ = path_cases.oracle_frames(oracle, sc)
    n = len(path_cases.OFFSETS)
    checked = 0
    for a in range(n - 1):
        b = a + 1
        if path_cases.OFFSETS[a] == path_cases.OFFSETS[b]:
            continue
        mean = path.shutter_mean(np.stack([frames[a], frames[b]]), 2)[0]
        for f in (a, b):
            frac = float((mean != frames[f]).mean())
            print(f"cameras {a},{b}: the mean differs from frame {f} in {frac:.1%} of the pixels")
            assert frac >= 0.01, f"the mean of cameras {a} and {b} differs from frame {f} in only {frac:.2%}"
        checked += 1
    assert checked == n - 1, "every consecutive pair of the test path is a pair of distinct cameras"
    # and the pairs the GPU tests average at m = 2: (0, 1), (2, 3), (4, 5)
    for a in (0, 2, 4):
        assert path_cases.OFFSETS[a] != path_cases.OFFSETS[a + 1]
