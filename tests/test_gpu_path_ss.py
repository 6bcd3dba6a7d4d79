"""rt_set_path_supersampling on the GPU: the camera-path, shutter and scene-track renders box-filtered from k x k samples
per pixel inside the trace kernels (the PATH_SS / SHUTTER_SS / ANIM_SS instantiations).  Every output frame is bit-exact
against supersample.path_resolve of the unchanged oracle's frames at k W x k H -- one rounding over the shutter's
sub-frames and the samples (tests/test_path_ss.py shows that a mean of means differs) -- and the ray counts equal the sum
of the oracle's at the sample size over the cameras used.  No tolerance anywhere.  Camera i of a list is
tests/path_cases.py's camera i % 6, so the oracle frames are rendered once per scene and sample size."""
import ctypes as C
import dataclasses

import numpy as np
import pytest

import anim_cases
import path_cases
from raytracer_hip import Context, abi, path, scenes
from raytracer_hip.supersample import box_resolve, path_resolve
from test_gpu_supersample import SCENES, _band_rows_of

pytestmark = pytest.mark.gpu

N = len(path_cases.OFFSETS)
RAYS = ("primary_rays", "reflect_rays", "shadow_rays")
W0, H0 = 50, 30
SMALL = (13, 7)  # 52 x 28 and 104 x 56 samples: no multiple of 8 in either axis, so edge tiles hold partly invalid blocks


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


def expected(oracle, sc, order, k, m=1, W=None, H=None, view_h=None):
    """(frames [len(order) / m, H, W], summed ray counts at the sample size) of the cameras `order` at factor k under a
    shutter of m."""
    W, H = W or sc.width, H or sc.height
    frames, stats = path_cases.oracle_frames(oracle, sc, k * W, k * H, k * view_h if view_h else None)
    return path_resolve(frames[order], k, m), {r: sum(stats[i][r] for i in order) for r in RAYS}


def ray_counts(st):
    return {r: st[r] for r in RAYS}


def _stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


def _code(fn):
    with pytest.raises(abi.RayTracerError) as ei:
        fn()
    return ei.value.code


def _render(oracle, sc, k, m, n_cams, what):
    W, H = sc.width, sc.height
    cams, order = cycled(sc, n_cams)
    want, rays = expected(oracle, sc, order, k, m)
    F = n_cams // m
    with Context(1) as ctx:
        ctx.set_scene(sc)
        assert ctx.get_path_supersampling() == 1
        ctx.set_path_supersampling(k)
        assert ctx.get_path_supersampling() == k and ctx.supersampling == 1
        ctx.reset_stats()
        px = ctx.render_shutter(cams, W, H, m) if m > 1 else ctx.render_path(cams, W, H)
        st = ctx.stats()
    assert px.shape == (F, H, W)
    for f in range(F):
        assert_same(px[f], want[f], f"{what} {W}x{H} k={k} m={m} frame {f}")
    assert ray_counts(st) == rays, "the ray counts are the sum of the oracle's at k W x k H over every sub-frame"
    assert st["primary_rays"] == n_cams * k * k * W * H
    assert st["frames"] == F and st["pixels"] == F * W * H
    return px


# ---- path ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(SCENES))
def test_path_every_scene_at_k_2(oracle, name):
    """Both families, every class among them, the Math.Pow entry points (gpow_direct, gpow_bundle) and the scratch stack
    (REF: recursion limit 32, K = 64), 6 cameras each."""
    _render(oracle, SCENES[name](), 2, 1, 6, name)


def test_the_k_2_scenes_cover_gpow_and_the_scratch_stack():
    assert SCENES["REF"]().recursion_limit >= 8
    for name in ("gpow_direct", "gpow_bundle"):
        assert any(s.material.n not in (0.0, 0.5, 1.0, 2.0) for s in SCENES[name]().spheres)


@pytest.mark.parametrize("k", [4, 8])
@pytest.mark.parametrize("name", ["C3", "C4"])
def test_path_k_4_and_8_with_partly_invalid_edge_blocks(oracle, name, k):
    px = _render(oracle, scenes.config(name).resized(*SMALL), k, 1, 6, name)
    assert (px[0] == px[5]).all() and (px[0] != px[2]).any()


# ---- shutter -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["C3", "C4"])
def test_shutter_2_at_k_2(oracle, name):
    _render(oracle, SCENES[name](), 2, 2, 6, name)


@pytest.mark.parametrize("m,k", [(4, 8), (64, 2)])
def test_shutter_fills_the_sum_fields(oracle, m, k):
    """m k^2 = 256 values per channel: the largest sums the 16-bit fields hold."""
    _render(oracle, scenes.config("C3").resized(*SMALL), k, m, m, "C3")


@pytest.mark.parametrize("name", ["C3", "C4"])
def test_shutter_16_at_k_4(oracle, name):
    _render(oracle, scenes.config(name).resized(*SMALL), 4, 16, 32, name)


def test_64_identical_cameras_at_k_2_give_that_camera_s_resolved_frame(oracle):
    sc = SCENES["REF"]()
    frames, stats = path_cases.oracle_frames(oracle, sc, 2 * sc.width, 2 * sc.height)
    cam = path_cases.cameras(sc)[2]
    with Context(1) as ctx:
        ctx.set_scene(sc)
        ctx.set_path_supersampling(2)
        ctx.reset_stats()
        px = ctx.render_shutter([cam] * 64, sc.width, sc.height, 64)
        st = ctx.stats()
    assert px.shape == (1, sc.height, sc.width)
    assert_same(px[0], box_resolve(frames[2], 2), "64 identical sub-frames")
    assert ray_counts(st) == {r: 64 * stats[2][r] for r in RAYS}


@pytest.fixture(scope="module")
def c3():
    return scenes.config("C3").resized(W0, H0)


@pytest.fixture(scope="module")
def c3_ctx(c3):
    ctx = Context(1)
    ctx.set_scene(c3)
    ctx.set_path_supersampling(2)
    yield ctx
    ctx.close()


KEYS = RAYS + ("frames", "pixels", "launches")


@pytest.mark.parametrize("fmt", [abi.RT_BANDS_INT32, abi.RT_BANDS_RGB24, abi.RT_BANDS_FRAME])
def test_shutter_1_is_the_path_call_at_k_2(c3, c3_ctx, fmt):
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
    assert {k: sa[k] for k in KEYS} == {k: sb[k] for k in KEYS}
    assert sa["primary_rays"] == N * 4 * 16 * W0  # bands 0 and 2 of 8 rows: 16 output rows, 4 samples per pixel


# ---- scene tracks --------------------------------------------------------------------------------------------------
def check_track(oracle, track, k, what, first_frame=0):
    W, H = track[0].width, track[0].height
    frames, ost = anim_cases.oracle_frames(oracle, track, k * W, k * H)
    want = path_resolve(frames, k)
    n = len(track) - first_frame
    with Context(1) as ctx:
        ctx.set_scene_track(track)
        ctx.set_path_supersampling(k)
        ctx.reset_stats()
        px = ctx.render_anim(None, W, H, first_frame=first_frame)
        st = ctx.stats()
    assert px.shape == (n, H, W)
    for j in range(n):
        assert_same(px[j], want[first_frame + j], f"{what} k={k} frame {first_frame + j}")
    assert ray_counts(st) == anim_cases.summed(ost[first_frame:]), f"{what}: the oracle's counts at the sample size"
    assert st["primary_rays"] == n * k * k * W * H and st["frames"] == n and st["pixels"] == n * W * H and st["launches"] == 1
    return px


@pytest.fixture(scope="module")
def direct():
    return anim_cases.direct_track(25, 15)


@pytest.mark.parametrize("k", [2, 4])
def test_anim_direct_track(oracle, direct, k):
    px = check_track(oracle, direct, k, "direct track")
    assert (px[0] == px[5]).all() and (px[0] != px[2]).any() and (px[2] != px[4]).any()


def test_anim_frames_from_first_frame_2_use_their_own_scenes(oracle, direct):
    check_track(oracle, direct, 2, "direct track from frame 2", first_frame=2)


def test_anim_bundle_track_at_k_2(oracle):
    check_track(oracle, anim_cases.bundle_track(16, 10), 2, "bundle track")


@pytest.mark.parametrize("cls", ["s8", "s12"])
def test_anim_track_that_mixes_gpow_and_other_frames_at_k_2(oracle, cls):
    base, g = anim_cases.class_track(cls, False, 3), anim_cases.class_track(cls, True, 3)
    mixed = [dataclasses.replace(g[f] if f == 2 else sc, name=f"{sc.name}_expmix_ss") for f, sc in enumerate(base)]
    check_track(oracle, mixed, 2, f"{cls} exponent 7.3 in frame 2")


# ---- bands, formats, view height, chunks ---------------------------------------------------------------------------
@pytest.mark.parametrize("m", [1, 2])
@pytest.mark.parametrize("first,step", [(0, 1), (1, 2), (2, 3)])
def test_bands_and_formats_leave_padding_and_other_ranks_rows_alone(oracle, c3, c3_ctx, first, step, m):
    import torch
    band_rows, F, k = 8, 3, 2
    cams, order = cycled(c3, F * m)
    want, rays = expected(oracle, c3, order, k, m)
    rows = _band_rows_of(first, step, band_rows, H0)
    nb_want = -(-len(rows) // band_rows)
    others = [y for y in range(H0) if y not in rows]

    def call(ptr, stride, fmt):
        if m == 1:
            return c3_ctx.render_path_bands(W0, H0, cams, band_rows, first, step, ptr, stride, fmt, _stream())
        return c3_ctx.render_shutter_bands(W0, H0, cams, m, band_rows, first, step, ptr, stride, fmt, _stream())

    # INT32: packed band sets
    stride = nb_want * band_rows * W0 * 4 + 64
    out = torch.full((F * stride // 4,), -1, dtype=torch.int32, device="cuda")
    c3_ctx.reset_stats()
    nb = call(out.data_ptr(), stride, abi.RT_BANDS_INT32)
    torch.cuda.synchronize()
    assert nb == nb_want
    host = out.cpu().numpy().reshape(F, stride // 4)
    for f in range(F):
        assert_same(host[f, :len(rows) * W0].reshape(len(rows), W0), want[f][rows], f"INT32 ({first},{step}) m={m} frame {f}")
        assert (host[f, len(rows) * W0:] == -1).all(), "rows past the image and the stride's padding stay untouched"
    st = c3_ctx.stats()
    assert st["launches"] == 1
    assert st["primary_rays"] == F * m * k * k * len(rows) * W0 and st["pixels"] == F * nb * band_rows * W0
    if step == 1:
        assert ray_counts(st) == rays
    # RGB24: bytes B, G, R
    stride = nb_want * band_rows * W0 * 3 + 64
    raw = torch.full((F * stride,), 0xA5, dtype=torch.uint8, device="cuda")
    call(raw.data_ptr(), stride, abi.RT_BANDS_RGB24)
    torch.cuda.synchronize()
    hr = raw.cpu().numpy().reshape(F, stride)
    for f in range(F):
        b = hr[f, :len(rows) * W0 * 3].reshape(len(rows), W0, 3).astype(np.int32)
        assert_same(b[..., 0] | (b[..., 1] << 8) | (b[..., 2] << 16), want[f][rows], f"RGB24 ({first},{step}) m={m} frame {f}")
        assert (hr[f, len(rows) * W0 * 3:] == 0xA5).all()
    # FRAME: the bands in their rows of the row-major frame
    stride = H0 * W0 * 4 + 64
    frame = torch.full((F * stride // 4,), -1, dtype=torch.int32, device="cuda")
    call(frame.data_ptr(), stride, abi.RT_BANDS_FRAME)
    torch.cuda.synchronize()
    hf = frame.cpu().numpy().reshape(F, stride // 4)
    for f in range(F):
        img = hf[f, :H0 * W0].reshape(H0, W0)
        assert_same(img[rows], want[f][rows], f"FRAME ({first},{step}) m={m} frame {f}")
        assert (img[others] == -1).all(), "the rows of other ranks stay untouched"
        assert (hf[f, H0 * W0:] == -1).all()


def test_view_height_is_in_output_rows(oracle, c3, c3_ctx):
    cams, order = cycled(c3, 6)
    want, rays = expected(oracle, c3, order, 2, 1, W0, 22, view_h=H0)
    want2, rays2 = expected(oracle, c3, order, 2, 2, W0, 22, view_h=H0)
    c3_ctx.set_view_height(H0)
    try:
        c3_ctx.reset_stats()
        px = c3_ctx.render_path(cams, W0, 22)
        for f in range(6):
            assert_same(px[f], want[f], f"50x22 of a 50x30 view, frame {f}")
        assert ray_counts(c3_ctx.stats()) == rays
        c3_ctx.reset_stats()
        px = c3_ctx.render_shutter(cams, W0, 22, 2)
        for f in range(3):
            assert_same(px[f], want2[f], f"50x22 of a 50x30 view, shutter 2, frame {f}")
        assert ray_counts(c3_ctx.stats()) == rays2
        assert _code(lambda: c3_ctx.render_path(cams, W0, H0 + 1)) == abi.RT_ERR_INVALID_ARG
    finally:
        c3_ctx.set_view_height(0)


@pytest.mark.parametrize("m", [1, 2])
@pytest.mark.parametrize("registered", [True, False])
def test_chunked_render_path_and_render_shutter(oracle, c3, registered, m, monkeypatch):
    sc = c3.resized(16, 9)
    cams, order = cycled(sc, 5 * m, start=1)
    want, rays = expected(oracle, sc, order, 2, m)
    monkeypatch.setenv("RT_PATH_CHUNK_FRAMES", "2")  # read at rt_create: chunks of 2, 2 and 1 output frames
    with Context(1) as ctx:
        ctx.set_scene(sc)
        ctx.set_path_supersampling(2)
        out = np.full((5, 9, 16), -1, dtype=np.int32)
        if registered:
            ctx.register_host(out)
        try:
            ctx.reset_stats()
            got = ctx.render_shutter(cams, 16, 9, m, out) if m > 1 else ctx.render_path(cams, 16, 9, out)
            st = ctx.stats()
        finally:
            if registered:
                ctx.unregister_host(out)
    assert np.shares_memory(got, out)
    for f in range(5):
        assert_same(out[f], want[f], f"chunked frame {f}, registered={registered}, m={m}")
    assert st["launches"] == 3 and st["frames"] == 5 and st["pixels"] == 5 * 16 * 9
    assert ray_counts(st) == rays


def test_back_to_back_calls_on_two_streams_and_a_change_of_factor(oracle, c3, c3_ctx):
    """Six calls with nothing waited for in between go round the four view-table slots; a call at k = 4 straight after
    one at k = 2 finds the shared view tables built for the other sample size."""
    import torch
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    picks = [cycled(c3, 3, start=i) for i in range(6)]
    outs = [torch.full((3, H0, W0), -1, dtype=torch.int32, device="cuda") for _ in picks]
    torch.cuda.synchronize()
    for i, ((cams, _), out) in enumerate(zip(picks, outs)):
        c3_ctx.render_path_bands(W0, H0, cams, H0, 0, 1, out.data_ptr(), H0 * W0 * 4, abi.RT_BANDS_INT32, streams[i % 2].cuda_stream)
    torch.cuda.synchronize()
    for i, ((_, order), out) in enumerate(zip(picks, outs)):
        want, _ = expected(oracle, c3, order, 2)
        host = out.cpu().numpy()
        for f in range(3):
            assert_same(host[f], want[f], f"call {i} frame {f} (camera {order[f]})")
    small = scenes.config("C3").resized(*SMALL)  # (the context's scene and cameras: only the frame size differs)
    cams, order = cycled(small, 3)
    w2, _ = expected(oracle, small, order, 2)
    w4, _ = expected(oracle, small, order, 4)
    a = torch.full((3, SMALL[1], SMALL[0]), -1, dtype=torch.int32, device="cuda")
    b = torch.full((3, SMALL[1], SMALL[0]), -1, dtype=torch.int32, device="cuda")
    nbytes = SMALL[0] * SMALL[1] * 4
    try:
        c3_ctx.render_path_bands(SMALL[0], SMALL[1], cams, SMALL[1], 0, 1, a.data_ptr(), nbytes, abi.RT_BANDS_INT32, _stream())
        c3_ctx.set_path_supersampling(4)
        c3_ctx.render_path_bands(SMALL[0], SMALL[1], cams, SMALL[1], 0, 1, b.data_ptr(), nbytes, abi.RT_BANDS_INT32, _stream())
        torch.cuda.synchronize()
    finally:
        c3_ctx.set_path_supersampling(2)
    for f in range(3):
        assert_same(a.cpu().numpy()[f], w2[f], f"k = 2 before the change, frame {f}")
        assert_same(b.cpu().numpy()[f], w4[f], f"k = 4 straight after k = 2, frame {f}")


# ---- off means off -------------------------------------------------------------------------------------------------
def _three_band_calls(ctx, sc, track_cams):
    import torch
    cams = path_cases.cameras(sc)
    nbytes = H0 * W0 * 4 + 64
    bufs, stats = [], []
    for which in range(3):
        buf = torch.full((N * nbytes,), 0x5A, dtype=torch.uint8, device="cuda")
        ctx.reset_stats()
        if which == 0:
            ctx.render_path_bands(W0, H0, cams, 8, 1, 2, buf.data_ptr(), nbytes, abi.RT_BANDS_INT32, _stream())
        elif which == 1:
            ctx.render_shutter_bands(W0, H0, cams, 2, 8, 1, 2, buf.data_ptr(), nbytes, abi.RT_BANDS_RGB24, _stream())
        else:
            ctx.render_anim_bands(W0, H0, track_cams, 8, 1, 2, buf.data_ptr(), nbytes, abi.RT_BANDS_FRAME, _stream())
        torch.cuda.synchronize()
        st = ctx.stats()
        bufs.append(buf.cpu().numpy()), stats.append({k: st[k] for k in KEYS})
    return bufs, stats


def test_factor_1_is_the_library_without_the_setter(c3):
    track = anim_cases.direct_track(W0, H0)[:3]
    track_cams = [sc.c_camera() for sc in track]
    with Context(1) as ctx:
        ctx.set_scene(c3)
        ctx.set_scene_track(track)
        never, st_never = _three_band_calls(ctx, c3, track_cams)
    with Context(1) as ctx:
        ctx.set_scene(c3)
        ctx.set_scene_track(track)
        ctx.set_path_supersampling(4)
        ctx.set_path_supersampling(1)
        back, st_back = _three_band_calls(ctx, c3, track_cams)
    for i in range(3):
        assert (never[i] != 0x5A).any()
        assert np.array_equal(never[i], back[i]), f"call {i}: byte-identical buffers"
        assert st_never[i] == st_back[i], f"call {i}: identical stats"


def test_every_other_render_ignores_the_factor(c3):
    import torch

    def others(ctx):
        ctx.reset_stats()
        frame = ctx.render(W0, H0).copy()
        batch = torch.full((2, 16, W0), -1, dtype=torch.int32, device="cuda")
        ctx.render_bands_batch(W0, H0, 8, 0, 2, 2, batch.data_ptr(), 16 * W0 * 4, abi.RT_BANDS_INT32, _stream())
        torch.cuda.synchronize()
        segs, total = ctx.debug_segments(W0, H0, 97)
        st = ctx.stats()
        # (the segments are appended in the order the device's atomics fall: compared as a sorted list of records)
        return frame, batch.cpu().numpy(), (sorted(s.tobytes() for s in segs), total), {k: st[k] for k in KEYS}

    with Context(1) as ctx:
        ctx.set_scene(c3)
        plain = others(ctx)
        ctx.set_path_supersampling(4)
        with_factor = others(ctx)
    assert (plain[1] != -1).any() and plain[2][1] > 0
    assert np.array_equal(plain[0], with_factor[0]), "rt_render"
    assert np.array_equal(plain[1], with_factor[1]), "rt_render_bands_batch"
    assert plain[2] == with_factor[2], "rt_debug_segments"
    assert plain[3] == with_factor[3], "the stats"


@pytest.mark.parametrize("path_k", [1, 2, 8])
def test_rt_set_supersampling_still_refuses_all_six_calls(c3, path_k):
    import torch
    track = anim_cases.direct_track(W0, H0)[:2]
    cams = path_cases.cameras(c3)[:2]
    out = torch.full((2, H0, W0), -1, dtype=torch.int32, device="cuda")
    host = np.full((2, H0, W0), -1, dtype=np.int32)
    nbytes = H0 * W0 * 4
    with Context(1) as ctx:
        ctx.set_scene(c3)
        ctx.set_scene_track(track)
        ctx.set_path_supersampling(path_k)
        ctx.set_supersampling(2)
        calls = [
            lambda: ctx.render_path_bands(W0, H0, cams, H0, 0, 1, out.data_ptr(), nbytes, abi.RT_BANDS_INT32, _stream()),
            lambda: ctx.render_shutter_bands(W0, H0, cams, 2, H0, 0, 1, out.data_ptr(), nbytes, abi.RT_BANDS_INT32, _stream()),
            lambda: ctx.render_anim_bands(W0, H0, None, H0, 0, 1, out.data_ptr(), nbytes, abi.RT_BANDS_INT32, _stream()),
            lambda: ctx.render_path(cams, W0, H0, host),
            lambda: ctx.render_shutter(cams, W0, H0, 2, host[:1]),
            lambda: ctx.render_anim(None, W0, H0, out=host),
        ]
        for i, fn in enumerate(calls):
            assert _code(fn) == abi.RT_ERR_UNSUPPORTED, f"call {i} at path factor {path_k}"
        torch.cuda.synchronize()
    assert (out.cpu().numpy() == -1).all() and (host == -1).all(), "a refused call writes nothing"


# ---- refusals ------------------------------------------------------------------------------------------------------
def test_bad_factors_and_null_pointers(c3_ctx):
    lib = c3_ctx.lib
    for k in (0, 3, 16, -2):
        assert lib.rt_set_path_supersampling(c3_ctx.ptr, k) == abi.RT_ERR_INVALID_ARG
        assert c3_ctx.get_path_supersampling() == 2, "a refused factor changes nothing"
    assert lib.rt_set_path_supersampling(None, 2) == abi.RT_ERR_INVALID_ARG
    assert lib.rt_get_path_supersampling(None, C.byref(C.c_int(0))) == abi.RT_ERR_INVALID_ARG
    assert lib.rt_get_path_supersampling(c3_ctx.ptr, None) == abi.RT_ERR_INVALID_ARG


def test_too_many_samples_per_pixel_and_too_large_a_sample_frame_write_nothing(c3, c3_ctx):
    import torch
    lib = c3_ctx.lib
    cams = path.as_array(cycled(c3, 128)[0])
    out = torch.full((H0, W0), -1, dtype=torch.int32, device="cuda")
    host = np.full((H0, W0), -1, dtype=np.int32)
    before = c3_ctx.stats()
    # m k^2 = 128 * 4 = 512 (k = 2), and 64 * 16 = 1024 once k = 4; 64 * 4 = 256 is the largest allowed
    assert lib.rt_render_shutter(c3_ctx.ptr, W0, H0, cams, 1, 128, host.ctypes.data) == abi.RT_ERR_INVALID_ARG
    assert b"256" in lib.rt_last_error(c3_ctx.ptr)
    assert lib.rt_render_shutter_bands(c3_ctx.ptr, W0, H0, cams, 1, 128, H0, 0, 1, C.c_void_p(out.data_ptr()), H0 * W0 * 4,
                                       abi.RT_BANDS_INT32, C.c_void_p(_stream()), None) == abi.RT_ERR_INVALID_ARG
    # a sample frame of 65,536 x 65,536 = 2^32 samples (the output frame, 2^30 pixels, is allowed)
    big = 32768
    assert lib.rt_render_path(c3_ctx.ptr, big, big, cams, 1, host.ctypes.data) == abi.RT_ERR_INVALID_ARG
    assert b"2^31" in lib.rt_last_error(c3_ctx.ptr)
    assert lib.rt_render_path_bands(c3_ctx.ptr, big, big, cams, 1, 8, 0, 1, C.c_void_p(out.data_ptr()), 0, abi.RT_BANDS_INT32,
                                    C.c_void_p(_stream()), None) == abi.RT_ERR_INVALID_ARG
    # with a view height the bound is on the view: 2 x 32768 columns by 2 x 32768 view rows
    c3_ctx.set_view_height(big)
    try:
        assert lib.rt_render_path_bands(c3_ctx.ptr, big, 8, cams, 1, 8, 0, 1, C.c_void_p(out.data_ptr()), 0, abi.RT_BANDS_INT32,
                                        C.c_void_p(_stream()), None) == abi.RT_ERR_INVALID_ARG
    finally:
        c3_ctx.set_view_height(0)
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == -1).all() and (host == -1).all(), "a refused call writes nothing"
    after = c3_ctx.stats()
    assert {k: after[k] for k in KEYS} == {k: before[k] for k in KEYS}


# ---- counting, camera, view ----------------------------------------------------------------------------------------
def test_counting_off_counts_no_rays_and_changes_no_pixel(oracle, c3, c3_ctx):
    cams, order = cycled(c3, 6)
    want, _ = expected(oracle, c3, order, 2, 2)
    want1, _ = expected(oracle, c3, order, 2)
    c3_ctx.reset_stats()
    c3_ctx.render_shutter(cams, W0, H0, 2)
    before = c3_ctx.stats()
    c3_ctx.set_counting(False)
    try:
        px = c3_ctx.render_shutter(cams, W0, H0, 2)
        px1 = c3_ctx.render_path(cams, W0, H0)
        after = c3_ctx.stats()
    finally:
        c3_ctx.set_counting(True)
    assert ray_counts(after) == ray_counts(before), "nothing counted"
    assert after["frames"] == before["frames"] + 9 and after["pixels"] == before["pixels"] + 9 * W0 * H0
    for f in range(3):
        assert_same(px[f], want[f], f"counting off, shutter frame {f}")
    for f in range(6):
        assert_same(px1[f], want1[f], f"counting off, path frame {f}")


def test_context_camera_and_view_survive_a_call(oracle, c3, c3_ctx):
    frames, _ = path_cases.oracle_frames(oracle, c3)
    own = path_cases.moved(c3, path_cases.OFFSETS[3])
    c3_ctx.set_camera(own.c_camera())
    try:
        assert_same(c3_ctx.render(W0, H0).copy(), frames[3], "rt_render before the call")
        c3_ctx.render_path(cycled(c3, 4)[0], W0, H0)
        c3_ctx.render_shutter(cycled(c3, 4)[0], W0, H0, 2)
        got = c3_ctx.get_camera()
        assert (got.position.x, got.position.z, got.yaw, got.pitch) == (
            own.c_camera().position.x, own.c_camera().position.z, own.c_camera().yaw, own.c_camera().pitch)
        assert_same(c3_ctx.render(W0, H0).copy(), frames[3], "rt_render after the calls")
    finally:
        c3_ctx.set_camera(c3.c_camera())
