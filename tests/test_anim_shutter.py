"""The scene-track shutter (rt_render_anim_shutter_bands / rt_render_anim_shutter), the parts that need no GPU: the
Python wrappers' camera defaults and ValueErrors against a stub library, the abi.py prototypes against the header, and
the two helpers that make sub-frame scenes and cameras (anim.tween, path.subframes) fitting together."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import anim_cases
from raytracer_hip import Context, abi, anim, path, scenes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class StubLib:
    """Records the two calls' arguments and answers RT_OK."""

    def __init__(self):
        self.calls = []

    def rt_render_anim_shutter_bands(self, ptr, w, h, cams, first, n, shutter, rows, bfirst, bstep, d_out, stride, fmt, stream, nb):
        self.calls.append(("bands", w, h, len(cams), first, n, shutter, rows, bfirst, bstep, d_out.value, stride, fmt, stream.value))
        nb._obj.value = 3
        return abi.RT_OK

    def rt_render_anim_shutter(self, ptr, w, h, cams, first, n, shutter, pixels):
        self.calls.append(("frames", w, h, [(c.position.x, c.yaw) for c in cams], first, n, shutter, pixels))
        return abi.RT_OK


def stub_context(track):
    ctx = Context.__new__(Context)
    ctx.lib, ctx.ptr, ctx.track = StubLib(), C.c_void_p(1), track
    return ctx


@pytest.fixture(scope="module")
def track():
    return anim_cases.class_track("s3", False, 1) + anim_cases.class_track("s3", False, 1)[:1]  # 4 scenes, cameras differ


def test_render_anim_shutter_takes_each_sub_frame_scenes_own_camera(track):
    ctx = stub_context(track)
    out = ctx.render_anim_shutter(None, 8, 4, shutter=2)
    assert out.shape == (2, 4, 8) and out.dtype == np.int32
    (kind, w, h, cams, first, n, shutter, pixels), = ctx.lib.calls
    assert (kind, w, h, first, n, shutter, pixels) == ("frames", 8, 4, 0, 2, 2, out.ctypes.data)
    want = [(sc.c_camera().position.x, sc.c_camera().yaw) for sc in track]
    assert cams == want and len({c for c in want}) > 1
    # from first_frame on: the cameras of the scenes behind it
    ctx = stub_context(track)
    assert ctx.render_anim_shutter(None, 8, 4, shutter=2, first_frame=2).shape == (1, 4, 8)
    assert ctx.lib.calls[0][3] == want[2:] and ctx.lib.calls[0][4:7] == (2, 1, 2)
    # explicit cameras, an output array of the caller's
    ctx = stub_context(track)
    mine = np.zeros((1, 4, 8), dtype=np.int32)
    got = ctx.render_anim_shutter(path.subframes([track[0].c_camera(), track[1].c_camera()], 2)[:2], 8, 4, 2, first_frame=1, out=mine)
    assert np.shares_memory(got, mine) and ctx.lib.calls[0][4:7] == (1, 1, 2)


def test_render_anim_shutter_bands_passes_every_argument_on(track):
    ctx = stub_context(track)
    nb = ctx.render_anim_shutter_bands(16, 12, None, 4, 5, 1, 2, 0x1000, 4096, abi.RT_BANDS_RGB24, 0x77, first_frame=0)
    assert nb == 3
    assert ctx.lib.calls == [("bands", 16, 12, 4, 0, 1, 4, 5, 1, 2, 0x1000, 4096, abi.RT_BANDS_RGB24, 0x77)]
    ctx = stub_context(track)
    ctx.render_anim_shutter_bands(16, 12, [sc.c_camera() for sc in track[1:3]], 2, 12, 0, 1, 0x1000, 0)
    assert ctx.lib.calls[0][3:7] == (2, 0, 1, 2) and ctx.lib.calls[0][12] == abi.RT_BANDS_INT32


@pytest.mark.parametrize("shutter", [0, -1, 3, 8])
def test_a_camera_count_that_is_no_multiple_of_the_shutter_is_a_value_error(track, shutter):
    """4 cameras: no multiple of 3 or 8; a shutter below 1 divides nothing.  Nothing reaches the library."""
    ctx = stub_context(track)
    with pytest.raises(ValueError):
        ctx.render_anim_shutter(None, 8, 4, shutter=shutter)
    with pytest.raises(ValueError):
        ctx.render_anim_shutter_bands(8, 4, None, shutter, 4, 0, 1, 0x1000, 0)
    with pytest.raises(ValueError):
        ctx.render_anim_shutter([track[0].c_camera()] * 5, 8, 4, shutter=2)
    assert ctx.lib.calls == []


def test_the_prototypes_agree_with_the_header():
    hdr = open(os.path.join(ROOT, "include", "raytracer_hip.h")).read()
    assert re.search(r"int rt_render_anim_shutter_bands\(rt_ctx\* ctx, int width, int height, const rt_camera\* cameras, "
                     r"int first_frame,\s+int n_frames, int shutter, int band_rows, int band_first, int band_step,\s+"
                     r"void\* d_out, size_t frame_stride_bytes, int format, void\* hip_stream,\s+int\* out_n_bands\);", hdr)
    assert re.search(r"int rt_render_anim_shutter\(rt_ctx\* ctx, int width, int height, const rt_camera\* cameras, "
                     r"int first_frame,\s+int n_frames, int shutter, int32_t\* pixels\);", hdr)
    assert re.search(r"#define RT_ABI_VERSION (\d+)", hdr).group(1) == "10" and abi.RT_ABI_VERSION == 10, "no ABI bump"
    protos = {e[0]: e for e in abi.EXPORTS}
    i, p = C.c_int, C.c_void_p
    assert protos["rt_render_anim_shutter_bands"][1:] == (i, [p, i, i, C.POINTER(abi.rt_camera), i, i, i, i, i, i, p, C.c_size_t, i, p,
                                                             C.POINTER(i)])
    assert protos["rt_render_anim_shutter"][1:] == (i, [p, i, i, C.POINTER(abi.rt_camera), i, i, i, p])
    # the track call's prototype with the shutter behind n_frames
    for new, old in (("rt_render_anim_shutter_bands", "rt_render_anim_bands"), ("rt_render_anim_shutter", "rt_render_anim")):
        a = list(protos[old][2])
        assert protos[new][2] == a[:6] + [i] + a[6:]
    # the header states the order of the refusals
    doc = hdr[hdr.index("Scene-track shutter"):hdr.index("int rt_render_anim_shutter_bands(")]
    order = ["NULL context", "RT_ERR_NO_SCENE", "first_frame < 0", "more than one", "rt_set_supersampling above 1", "2^31 - 1",
             "power of two", "n_frames * shutter above RT_MAX_PATH_FRAMES", "shutter * k*k above", "adaptive refusal", "band arguments"]
    at = [doc.index(s, doc.index("Refusals")) for s in order]
    assert at == sorted(at)


def test_the_built_library_exports_both_calls(rtlib):
    assert rtlib.rt_render_anim_shutter.argtypes[6] is C.c_int and len(rtlib.rt_render_anim_shutter_bands.argtypes) == 15
    cams = path.as_array([scenes.config("C1").c_camera()] * 4)
    buf = (C.c_int32 * 64)()
    nb = C.c_int(7)
    assert rtlib.rt_render_anim_shutter_bands(None, 4, 4, cams, 0, 1, 2, 4, 0, 1, buf, 64, abi.RT_BANDS_INT32, None,
                                              C.byref(nb)) == abi.RT_ERR_INVALID_ARG
    assert rtlib.rt_render_anim_shutter(None, 4, 4, cams, 0, 1, 2, buf) == abi.RT_ERR_INVALID_ARG
    assert nb.value == 7 and all(v == 0 for v in buf)


def test_tween_and_subframes_make_the_sub_frames_of_one_output_frame():
    """n keys at m sub-frames: tween(keys, m) holds the (n - 1) * m sub-frame scenes (and the closing key), and
    path.subframes of the keys' cameras the n * m cameras; the first (n - 1) * m of each belong together."""
    keys = [anim_cases.class_track("s3", False, 1)[i] for i in (0, 2)]
    m = 4
    sub = anim.tween(keys, m)
    cams = path.subframes([k.c_camera() for k in keys], m)
    assert len(sub) == m + 1 and len(cams) == 2 * m
    assert sub[0] is keys[0] and sub[-1] is keys[-1]
    assert cams[0].position.x == keys[0].c_camera().position.x and cams[m].yaw == keys[1].c_camera().yaw
