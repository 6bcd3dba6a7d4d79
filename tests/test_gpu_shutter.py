"""The camera-path shutter on the GPU (rt_render_shutter_bands / rt_render_shutter: m sub-frame cameras averaged per
output frame inside the trace kernel).  Every output frame is bit-exact against path.shutter_mean of the unchanged
oracle's frames of its sub-frame cameras, and the ray counts equal the sum of the oracle's over every sub-frame.  No
tolerance anywhere.  Camera i of a list is tests/path_cases.py's camera i % 6, so the oracle frames are rendered once
per scene; tests/test_shutter.py asserts that the mean of two of them is neither of the two, so a kernel that
stored one sub-frame cannot pass."""
import ctypes as C

import numpy as np
import pytest

import path_cases
from raytracer_hip import Context, abi, path, scenes
from test_gpu_supersample import SCENES, _band_rows_of

pytestmark = pytest.mark.gpu

N = len(path_cases.OFFSETS)
RAYS = ("primary_rays", "reflect_rays", "shadow_rays")
W0, H0 = 50, 30


def assert_same(px, want, what):
    bad = px != want
    if bad.any():
        idx = np.argwhere(bad)[0]
        pytest.fail(f"{what}: {int(bad.sum())} of {bad.size} pixels differ; first at {tuple(int(i) for i in idx)}: "
                    f"gpu {int(px[tuple(idx)]):#08x} expected {int(want[tuple(idx)]):#08x}")


def cycled(sc, n, start=0):
    """n cameras: camera i is the test path's camera (start + i) % 6; and their indices."""
    cams = path_cases.cameras(sc)
    order = [(start + i) % N for i in range(n)]
    return [cams[i] for i in order], order


def expected(oracle, sc, order, m, W=None, H=None, view_h=None):
    """(frames [len(order) / m, H, W], summed ray counts) of the cameras `order` under a shutter of m."""
    frames, stats = path_cases.oracle_frames(oracle, sc, W, H, view_h)
    return path.shutter_mean(frames[order], m), {k: sum(stats[i][k] for i in order) for k in RAYS}


def ray_counts(st):
    return {k: st[k] for k in RAYS}


def _stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


def _render(sc, n_cams, m, oracle):
    W, H = sc.width, sc.height
    cams, order = cycled(sc, n_cams)
    want, rays = expected(oracle, sc, order, m)
    with Context(1) as ctx:
        ctx.set_scene(sc)
        ctx.reset_stats()
        px = ctx.render_shutter(cams, W, H, m)
        st = ctx.stats()
    F = n_cams // m
    assert px.shape == (F, H, W)
    for f in range(F):
        assert_same(px[f], want[f], f"{sc.name} {W}x{H} shutter {m} frame {f}")
    assert ray_counts(st) == rays, "the ray counts are the sum of the oracle's over every sub-frame"
    assert st["primary_rays"] == n_cams * W * H
    assert st["frames"] == F and st["pixels"] == F * W * H


@pytest.mark.parametrize("name", list(SCENES))
def test_every_scene_at_shutter_2(oracle, name):
    _render(SCENES[name](), 6, 2, oracle)


@pytest.mark.parametrize("name", ["C3", "C4"])
def test_shutter_4(oracle, name):
    _render(SCENES[name](), 12, 4, oracle)


@pytest.mark.parametrize("name", ["C3", "C4"])
def test_shutter_256_fills_the_sum_fields(oracle, name):
    _render(SCENES[name](), 256, 256, oracle)


def test_shutter_256_of_one_camera_is_that_camera_s_frame(oracle):
    sc = SCENES["REF"]()
    frames, stats = path_cases.oracle_frames(oracle, sc)
    cam = path_cases.cameras(sc)[2]
    with Context(1) as ctx:
        ctx.set_scene(sc)
        ctx.reset_stats()
        px = ctx.render_shutter([cam] * 256, sc.width, sc.height, 256)
        st = ctx.stats()
    assert px.shape == (1, sc.height, sc.width)
    assert_same(px[0], frames[2], "256 identical sub-frames")
    assert ray_counts(st) == {k: 256 * stats[2][k] for k in RAYS}


@pytest.fixture(scope="module")
def c3():
    return scenes.config("C3").resized(W0, H0)


@pytest.fixture(scope="module")
def c3_ctx(c3):
    ctx = Context(1)
    ctx.set_scene(c3)
    yield ctx
    ctx.close()


@pytest.mark.parametrize("first,step", [(0, 1), (1, 2), (2, 3)])
def test_bands_and_formats_leave_padding_and_other_ranks_rows_alone(oracle, c3, c3_ctx, first, step):
    import torch
    band_rows, m, F = 8, 2, 3
    cams, order = cycled(c3, F * m)
    want, rays = expected(oracle, c3, order, m)
    rows = _band_rows_of(first, step, band_rows, H0)
    nb_want = -(-len(rows) // band_rows)
    others = [y for y in range(H0) if y not in rows]
    # INT32: packed band sets
    stride = nb_want * band_rows * W0 * 4 + 64
    out = torch.full((F * stride // 4,), -1, dtype=torch.int32, device="cuda")
    c3_ctx.reset_stats()
    nb = c3_ctx.render_shutter_bands(W0, H0, cams, m, band_rows, first, step, out.data_ptr(), stride, abi.RT_BANDS_INT32,
                                     _stream())
    torch.cuda.synchronize()
    assert nb == nb_want
    host = out.cpu().numpy().reshape(F, stride // 4)
    for f in range(F):
        assert_same(host[f, :len(rows) * W0].reshape(len(rows), W0), want[f][rows], f"INT32 ({first},{step}) frame {f}")
        assert (host[f, len(rows) * W0:] == -1).all(), "rows past the image and the stride's padding stay untouched"
    st = c3_ctx.stats()
    assert st["launches"] == 1
    assert st["primary_rays"] == F * m * len(rows) * W0 and st["pixels"] == F * nb * band_rows * W0
    if step == 1:
        assert ray_counts(st) == rays
    # RGB24: bytes B, G, R
    stride = nb_want * band_rows * W0 * 3 + 64
    raw = torch.full((F * stride,), 0xA5, dtype=torch.uint8, device="cuda")
    c3_ctx.render_shutter_bands(W0, H0, cams, m, band_rows, first, step, raw.data_ptr(), stride, abi.RT_BANDS_RGB24, _stream())
    torch.cuda.synchronize()
    hr = raw.cpu().numpy().reshape(F, stride)
    for f in range(F):
        b = hr[f, :len(rows) * W0 * 3].reshape(len(rows), W0, 3).astype(np.int32)
        assert_same(b[..., 0] | (b[..., 1] << 8) | (b[..., 2] << 16), want[f][rows], f"RGB24 ({first},{step}) frame {f}")
        assert (hr[f, len(rows) * W0 * 3:] == 0xA5).all()
    # FRAME: the bands in their rows of the row-major frame
    stride = H0 * W0 * 4 + 64
    frame = torch.full((F * stride // 4,), -1, dtype=torch.int32, device="cuda")
    c3_ctx.render_shutter_bands(W0, H0, cams, m, band_rows, first, step, frame.data_ptr(), stride, abi.RT_BANDS_FRAME, _stream())
    torch.cuda.synchronize()
    hf = frame.cpu().numpy().reshape(F, stride // 4)
    for f in range(F):
        img = hf[f, :H0 * W0].reshape(H0, W0)
        assert_same(img[rows], want[f][rows], f"FRAME ({first},{step}) frame {f}")
        assert (img[others] == -1).all(), "the rows of other ranks stay untouched"
        assert (hf[f, H0 * W0:] == -1).all()


@pytest.mark.parametrize("fmt", [abi.RT_BANDS_INT32, abi.RT_BANDS_RGB24, abi.RT_BANDS_FRAME])
def test_shutter_1_is_render_path_bands(c3, c3_ctx, fmt):
    import torch
    cams = path_cases.cameras(c3)
    nbytes = H0 * W0 * 4 + 64
    a = torch.full((N * nbytes,), 0x5A, dtype=torch.uint8, device="cuda")
    b = torch.full((N * nbytes,), 0x5A, dtype=torch.uint8, device="cuda")
    c3_ctx.reset_stats()
    c3_ctx.render_shutter_bands(W0, H0, cams, 1, 8, 0, 2, a.data_ptr(), nbytes, fmt, _stream())
    torch.cuda.synchronize()
    sa = c3_ctx.stats()
    c3_ctx.reset_stats()
    c3_ctx.render_path_bands(W0, H0, cams, 8, 0, 2, b.data_ptr(), nbytes, fmt, _stream())
    torch.cuda.synchronize()
    sb = c3_ctx.stats()
    ha, hb = a.cpu().numpy(), b.cpu().numpy()
    assert (hb != 0x5A).any()
    assert np.array_equal(ha, hb), "byte-identical buffers"
    keys = RAYS + ("frames", "pixels", "launches")
    assert {k: sa[k] for k in keys} == {k: sb[k] for k in keys}
    # and the whole-frame call
    c3_ctx.reset_stats()
    pa = c3_ctx.render_shutter(cams, W0, H0, 1).copy()
    sa = c3_ctx.stats()
    c3_ctx.reset_stats()
    pb = c3_ctx.render_path(cams, W0, H0)
    sb = c3_ctx.stats()
    assert np.array_equal(pa, pb)
    assert {k: sa[k] for k in keys} == {k: sb[k] for k in keys}


def test_view_height_applies_to_every_sub_frame(oracle, c3, c3_ctx):
    cams, order = cycled(c3, 6)
    want, rays = expected(oracle, c3, order, 2, W0, 22, view_h=H0)
    c3_ctx.set_view_height(H0)
    try:
        c3_ctx.reset_stats()
        px = c3_ctx.render_shutter(cams, W0, 22, 2)
        for f in range(3):
            assert_same(px[f], want[f], f"50x22 of a 50x30 view, frame {f}")
        assert ray_counts(c3_ctx.stats()) == rays
        with pytest.raises(abi.RayTracerError) as ei:
            c3_ctx.render_shutter(cams, W0, H0 + 1, 2)
        assert ei.value.code == abi.RT_ERR_INVALID_ARG
    finally:
        c3_ctx.set_view_height(0)


@pytest.mark.parametrize("registered", [True, False])
def test_chunked_render_shutter(oracle, c3, registered, monkeypatch):
    sc = c3.resized(16, 9)
    cams, order = cycled(sc, 10, start=1)
    want, rays = expected(oracle, sc, order, 2)
    monkeypatch.setenv("RT_PATH_CHUNK_FRAMES", "2")  # read at rt_create: chunks of 2, 2 and 1 output frames
    with Context(1) as ctx:
        ctx.set_scene(sc)
        out = np.full((5, 9, 16), -1, dtype=np.int32)
        if registered:
            ctx.register_host(out)
        try:
            ctx.reset_stats()
            got = ctx.render_shutter(cams, 16, 9, 2, out)
            st = ctx.stats()
        finally:
            if registered:
                ctx.unregister_host(out)
    assert np.shares_memory(got, out)
    for f in range(5):
        assert_same(out[f], want[f], f"chunked frame {f}, registered={registered}")
    assert st["launches"] == 3 and st["frames"] == 5 and st["pixels"] == 5 * 16 * 9
    assert ray_counts(st) == rays


def test_back_to_back_calls_on_two_streams(oracle, c3, c3_ctx):
    """Six calls with nothing waited for in between go round the four view-table slots with m records per frame:
    every slot's table must hold its own call's cameras when its launch runs."""
    import torch
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    picks = [cycled(c3, 6, start=i) for i in range(6)]
    outs = [torch.full((3, H0, W0), -1, dtype=torch.int32, device="cuda") for _ in picks]
    torch.cuda.synchronize()
    for i, ((cams, _), out) in enumerate(zip(picks, outs)):
        c3_ctx.render_shutter_bands(W0, H0, cams, 2, H0, 0, 1, out.data_ptr(), H0 * W0 * 4, abi.RT_BANDS_INT32,
                                    streams[i % 2].cuda_stream)
    torch.cuda.synchronize()
    for i, ((_, order), out) in enumerate(zip(picks, outs)):
        want, _ = expected(oracle, c3, order, 2)
        host = out.cpu().numpy()
        for f in range(3):
            assert_same(host[f], want[f], f"call {i} frame {f} (cameras {order[2 * f:2 * f + 2]})")


def test_context_camera_and_view_survive_a_shutter_call(oracle, c3, c3_ctx):
    frames, _ = path_cases.oracle_frames(oracle, c3)
    own = path_cases.moved(c3, path_cases.OFFSETS[3])
    c3_ctx.set_camera(own.c_camera())
    try:
        assert_same(c3_ctx.render(W0, H0).copy(), frames[3], "rt_render before the shutter call")
        c3_ctx.render_shutter(cycled(c3, 4)[0], W0, H0, 2)
        got = c3_ctx.get_camera()
        assert (got.position.x, got.position.z, got.yaw, got.pitch) == (
            own.c_camera().position.x, own.c_camera().position.z, own.c_camera().yaw, own.c_camera().pitch)
        assert_same(c3_ctx.render(W0, H0).copy(), frames[3], "rt_render after the shutter call")
    finally:
        c3_ctx.set_camera(c3.c_camera())


def test_counting_off_counts_no_rays_and_changes_no_pixel(oracle, c3, c3_ctx):
    cams, order = cycled(c3, 6)
    want, _ = expected(oracle, c3, order, 2)
    c3_ctx.reset_stats()
    c3_ctx.render_shutter(cams, W0, H0, 2)
    before = c3_ctx.stats()
    c3_ctx.set_counting(False)
    try:
        px = c3_ctx.render_shutter(cams, W0, H0, 2)
        after = c3_ctx.stats()
    finally:
        c3_ctx.set_counting(True)
    assert ray_counts(after) == ray_counts(before), "nothing counted"
    assert after["frames"] == before["frames"] + 3 and after["pixels"] == before["pixels"] + 3 * W0 * H0
    for f in range(3):
        assert_same(px[f], want[f], f"counting off, frame {f}")


def _code(fn):
    with pytest.raises(abi.RayTracerError) as ei:
        fn()
    return ei.value.code


def test_supersampling_is_unsupported_and_comes_back(oracle, c3, c3_ctx):
    import torch
    cams, order = cycled(c3, 4)
    want, _ = expected(oracle, c3, order, 2)
    out = torch.full((2, H0, W0), -1, dtype=torch.int32, device="cuda")
    bands = lambda: c3_ctx.render_shutter_bands(  # noqa: E731
        W0, H0, cams, 2, H0, 0, 1, out.data_ptr(), H0 * W0 * 4, abi.RT_BANDS_INT32, _stream())
    c3_ctx.set_supersampling(2)
    try:
        assert _code(bands) == abi.RT_ERR_UNSUPPORTED
        assert _code(lambda: c3_ctx.render_shutter(cams, W0, H0, 2)) == abi.RT_ERR_UNSUPPORTED
        torch.cuda.synchronize()
        assert (out.cpu().numpy() == -1).all(), "a refused call writes nothing"
    finally:
        c3_ctx.set_supersampling(1)
    bands()
    torch.cuda.synchronize()
    px = c3_ctx.render_shutter(cams, W0, H0, 2)
    for f in range(2):
        assert_same(out.cpu().numpy()[f], want[f], f"bands after supersampling, frame {f}")
        assert_same(px[f], want[f], f"whole frames after supersampling, frame {f}")


def test_bad_shutters_are_invalid_arguments(c3, c3_ctx):
    cams = cycled(c3, 6)[0]
    lib = c3_ctx.lib
    arr = path.as_array(cams)
    for shutter in (0, 3, 512, -2):
        assert lib.rt_render_shutter(c3_ctx.ptr, W0, H0, arr, 1, shutter, C.c_void_p(8)) == abi.RT_ERR_INVALID_ARG
    assert lib.rt_render_shutter(c3_ctx.ptr, W0, H0, arr, 256, 256, C.c_void_p(8)) == abi.RT_ERR_INVALID_ARG
    with pytest.raises(ValueError):
        c3_ctx.render_shutter(cams[:5], W0, H0, 2)
