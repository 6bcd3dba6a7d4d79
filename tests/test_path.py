"""Camera paths (rt_render_path_bands / rt_render_path), the parts that need no GPU: the precondition of
tests/test_gpu_path.py -- the oracle frames of the test path's cameras differ from one another, so no GPU test
there can pass by rendering one view for every frame -- raytracer_hip.path.replay against the rt_camera_on_*
calls made by hand, the argument checks that need no device, and the public surface (header, bindings)."""
import ctypes as C
import itertools
import os
import re

import pytest

import path_cases
from raytracer_hip import abi, path, scenes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _gpu_scenes():
    from test_gpu_supersample import SCENES  # the scenes of tests/test_gpu_path.py, built as that module builds them
    return SCENES


# Every pair of distinct cameras must differ in more than 25 % of the oracle's pixels (measured: REF 40-73 %,
# C1 41-66 %, C3 47-72 %, C4 55-82 %, bundle_L5 26-32 %, gpow_direct 49-69 %, gpow_bundle 56-85 %).  The dense
# 37 x 21 scene's small spheres leave most of its frame to the sky and the floor: its pairs differ in 18-38 %, so
# it is held to 15 % -- still far from "the same frame", which is all the GPU tests rely on.
PRECONDITION = {"REF": 0.25, "C1": 0.25, "C3": 0.25, "C4": 0.25, "dense": 0.15, "bundle_L5": 0.25,
                "gpow_direct": 0.25, "gpow_bundle": 0.25}


@pytest.mark.parametrize("name", list(PRECONDITION))
def test_oracle_frames_of_distinct_cameras_differ(oracle, name):
    sc = _gpu_scenes()[name]()
    frames, stats = path_cases.oracle_frames(oracle, sc)
    assert frames.shape == (len(path_cases.OFFSETS), sc.height, sc.width)
    for a, b in itertools.combinations(path_cases.DISTINCT, 2):
        frac = float((frames[a] != frames[b]).mean())
        assert frac > PRECONDITION[name], f"{name}: cameras {a} and {b} differ in only {frac:.0%} of the pixels"
    assert (frames[0] == frames[-1]).all() and path_cases.OFFSETS[0] == path_cases.OFFSETS[-1]


def test_every_gpu_scene_has_a_precondition():
    assert set(PRECONDITION) == set(_gpu_scenes())


def _cam_tuple(c):
    return (c.position.x, c.position.y, c.position.z, c.yaw, c.pitch)


def test_replay_equals_the_camera_calls_by_hand(rtlib):
    start = scenes.config("C3").c_camera()
    events = [("frame",), ("key", "W"), ("key", "W"), ("mouse", 40.0, -12.5), ("frame",), ("key", "A"),
              ("key", abi.RT_KEY_SPACE), ("frame",), ("frame",), ("mouse", -200.0, 33.0), ("key", "S"),
              ("key", "LeftShift"), ("key", "D"), ("key", "Q"), ("frame",)]
    got = path.replay(start, events)
    hand = path.copy_camera(start)
    want = [_cam_tuple(hand)]
    for key in (abi.RT_KEY_W, abi.RT_KEY_W):
        assert rtlib.rt_camera_on_key(C.byref(hand), key) == abi.RT_OK
    assert rtlib.rt_camera_on_mouse_move(C.byref(hand), 40.0, -12.5) == abi.RT_OK
    want.append(_cam_tuple(hand))
    for key in (abi.RT_KEY_A, abi.RT_KEY_SPACE):
        assert rtlib.rt_camera_on_key(C.byref(hand), key) == abi.RT_OK
    want += [_cam_tuple(hand)] * 2
    assert rtlib.rt_camera_on_mouse_move(C.byref(hand), -200.0, 33.0) == abi.RT_OK
    for key in (abi.RT_KEY_S, abi.RT_KEY_SHIFT, abi.RT_KEY_D, 0):  # (an unbound key moves nothing)
        assert rtlib.rt_camera_on_key(C.byref(hand), key) == abi.RT_OK
    want.append(_cam_tuple(hand))
    assert [_cam_tuple(c) for c in got] == want
    assert len({id(c) for c in got}) == len(got), "every frame has a camera object of its own"
    assert _cam_tuple(start) == want[0], "replay leaves the starting camera alone"
    assert want[1] != want[0] and want[2] != want[1] and want[4] != want[2]
    with pytest.raises(ValueError):
        path.replay(start, [("jump",)])


def test_as_array_is_contiguous_and_ordered(rtlib):
    cams = path.replay(scenes.config("C1").c_camera(), [("key", "W"), ("frame",)] * 5)
    arr = path.as_array(cams)
    assert isinstance(arr, C.Array) and len(arr) == 5 and C.sizeof(arr) == 5 * C.sizeof(abi.rt_camera)
    assert [_cam_tuple(c) for c in arr] == [_cam_tuple(c) for c in cams]
    assert path.as_array(arr) is arr
    assert len(path.as_array([])) == 0


def test_null_context_and_null_cameras_are_invalid_arguments(rtlib):
    cams = path.as_array([scenes.config("C1").c_camera()])
    nb = C.c_int(7)
    buf = (C.c_int32 * 16)()
    assert rtlib.rt_render_path_bands(None, 4, 4, cams, 1, 4, 0, 1, buf, 64, abi.RT_BANDS_INT32, None,
                                      C.byref(nb)) == abi.RT_ERR_INVALID_ARG
    assert nb.value == 7
    assert rtlib.rt_render_path(None, 4, 4, cams, 1, buf) == abi.RT_ERR_INVALID_ARG
    assert rtlib.rt_render_path_bands(None, 4, 4, None, 1, 4, 0, 1, buf, 64, abi.RT_BANDS_INT32, None,
                                      None) == abi.RT_ERR_INVALID_ARG
    assert rtlib.rt_render_path(None, 4, 4, None, 1, buf) == abi.RT_ERR_INVALID_ARG
    assert all(v == 0 for v in buf)


def test_header_bindings_and_library_agree(rtlib):
    hdr = open(os.path.join(ROOT, "include", "raytracer_hip.h")).read()
    assert re.search(r"int rt_render_path_bands\(rt_ctx\* ctx, int width, int height, const rt_camera\* cameras, "
                     r"int n_frames,\s+int band_rows, int band_first, int band_step, void\* d_out,\s+"
                     r"size_t frame_stride_bytes, int format, void\* hip_stream, int\* out_n_bands\);", hdr)
    assert re.search(r"int rt_render_path\(rt_ctx\* ctx, int width, int height, const rt_camera\* cameras, "
                     r"int n_frames,\s+int32_t\* pixels\);", hdr)
    assert re.search(r"\(ABI 10 addition\) Camera paths", hdr)
    assert re.search(r"#define RT_MAX_PATH_FRAMES (\d+)", hdr).group(1) == str(abi.RT_MAX_PATH_FRAMES) == "65535"
    assert re.search(r"#define RT_ABI_VERSION (\d+)", hdr).group(1) == "10", "no ABI bump"
    assert rtlib.rt_abi_version() == 10 == abi.RT_ABI_VERSION
    names = [e[0] for e in abi.EXPORTS]
    assert "rt_render_path_bands" in names and "rt_render_path" in names
    assert rtlib.rt_render_path.argtypes == [C.c_void_p, C.c_int, C.c_int, C.POINTER(abi.rt_camera), C.c_int,
                                             C.c_void_p]
    assert len(rtlib.rt_render_path_bands.argtypes) == 13
