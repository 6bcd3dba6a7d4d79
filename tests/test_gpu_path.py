"""Camera paths on the GPU (rt_render_path_bands / rt_render_path: one batch launch, one camera per frame).
Every frame is bit-exact against the unchanged oracle rendered with that frame's camera, and the ray counts equal
the sum of the oracle's over the frames.  The test path's cameras (tests/path_cases.py) give frames that differ
from one another in 18-85 % of their pixels (tests/test_path.py asserts it), so a launch that rendered one view
for every frame, or reused frame 0's screen boxes, cannot pass.  Oracle frames are rendered once per module."""
import ctypes as C

import numpy as np
import pytest

import path_cases
from raytracer_hip import Context, abi, path, scenes
from test_gpu_supersample import SCENES, _band_rows_of

pytestmark = pytest.mark.gpu

N = len(path_cases.OFFSETS)
RAYS = ("primary_rays", "reflect_rays", "shadow_rays")


def assert_same(px, want, what):
    bad = px != want
    if bad.any():
        idx = np.argwhere(bad)[0]
        pytest.fail(f"{what}: {int(bad.sum())} of {bad.size} pixels differ; first at {tuple(int(i) for i in idx)}: "
                    f"gpu {int(px[tuple(idx)]):#08x} expected {int(want[tuple(idx)]):#08x}")


def summed(stats, frames=None):
    return {k: sum(stats[f][k] for f in (frames if frames is not None else range(len(stats)))) for k in RAYS}


def ray_counts(st):
    return {k: st[k] for k in RAYS}


def _stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


@pytest.mark.parametrize("name", list(SCENES))
def test_scenes_bit_exact_per_frame_with_summed_ray_counts(oracle, name):
    sc = SCENES[name]()
    W, H = sc.width, sc.height
    want, ost = path_cases.oracle_frames(oracle, sc)
    with Context(1) as ctx:
        ctx.set_scene(sc)
        ctx.reset_stats()
        px = ctx.render_path(path_cases.cameras(sc), W, H)
        st = ctx.stats()
    assert px.shape == (N, H, W)
    for f in range(N):
        assert_same(px[f], want[f], f"{name} {W}x{H} frame {f}")
    assert ray_counts(st) == summed(ost), "the ray counts are the sum of the oracle's over the frames"
    assert st["primary_rays"] == N * W * H
    assert st["frames"] == N and st["pixels"] == N * W * H


W0, H0 = 50, 30


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
    band_rows = 8
    want, ost = path_cases.oracle_frames(oracle, c3)
    cams = path_cases.cameras(c3)
    rows = _band_rows_of(first, step, band_rows, H0)
    nb_want = -(-len(rows) // band_rows)
    others = [y for y in range(H0) if y not in rows]
    # INT32: packed band sets
    stride = nb_want * band_rows * W0 * 4 + 64
    out = torch.full((N * stride // 4,), -1, dtype=torch.int32, device="cuda")
    c3_ctx.reset_stats()
    nb = c3_ctx.render_path_bands(W0, H0, cams, band_rows, first, step, out.data_ptr(), stride, abi.RT_BANDS_INT32,
                                  _stream())
    torch.cuda.synchronize()
    assert nb == nb_want
    host = out.cpu().numpy().reshape(N, stride // 4)
    for f in range(N):
        assert_same(host[f, :len(rows) * W0].reshape(len(rows), W0), want[f][rows], f"INT32 ({first},{step}) frame {f}")
        assert (host[f, len(rows) * W0:] == -1).all(), "rows past the image and the stride's padding stay untouched"
    st = c3_ctx.stats()
    assert st["primary_rays"] == N * len(rows) * W0 and st["pixels"] == N * nb * band_rows * W0 and st["launches"] == 1
    if step == 1:
        assert ray_counts(st) == summed(ost)
    # RGB24: bytes B, G, R
    stride = nb_want * band_rows * W0 * 3 + 64
    raw = torch.full((N * stride,), 0xA5, dtype=torch.uint8, device="cuda")
    c3_ctx.render_path_bands(W0, H0, cams, band_rows, first, step, raw.data_ptr(), stride, abi.RT_BANDS_RGB24, _stream())
    torch.cuda.synchronize()
    hr = raw.cpu().numpy().reshape(N, stride)
    for f in range(N):
        b = hr[f, :len(rows) * W0 * 3].reshape(len(rows), W0, 3).astype(np.int32)
        assert_same(b[..., 0] | (b[..., 1] << 8) | (b[..., 2] << 16), want[f][rows], f"RGB24 ({first},{step}) frame {f}")
        assert (hr[f, len(rows) * W0 * 3:] == 0xA5).all()
    # FRAME: the bands in their rows of the row-major frame
    stride = H0 * W0 * 4 + 64
    frame = torch.full((N * stride // 4,), -1, dtype=torch.int32, device="cuda")
    c3_ctx.render_path_bands(W0, H0, cams, band_rows, first, step, frame.data_ptr(), stride, abi.RT_BANDS_FRAME, _stream())
    torch.cuda.synchronize()
    hf = frame.cpu().numpy().reshape(N, stride // 4)
    for f in range(N):
        img = hf[f, :H0 * W0].reshape(H0, W0)
        assert_same(img[rows], want[f][rows], f"FRAME ({first},{step}) frame {f}")
        assert (img[others] == -1).all(), "the rows of other ranks stay untouched"
        assert (hf[f, H0 * W0:] == -1).all()


def test_one_frame_equals_render_bands_ex_with_that_camera(oracle, c3, c3_ctx):
    import torch
    want, _ = path_cases.oracle_frames(oracle, c3)
    cams = path_cases.cameras(c3)
    try:
        for f in (2, 4):
            a = torch.full((H0 * W0,), -1, dtype=torch.int32, device="cuda")
            b = torch.full((H0 * W0,), -2, dtype=torch.int32, device="cuda")
            c3_ctx.render_path_bands(W0, H0, [cams[f]], 8, 1, 2, a.data_ptr(), 0, abi.RT_BANDS_FRAME, _stream())
            c3_ctx.set_camera(cams[f])
            c3_ctx.render_bands_ex(W0, H0, 8, 1, 2, b.data_ptr(), abi.RT_BANDS_FRAME, _stream())
            torch.cuda.synchronize()
            rows = _band_rows_of(1, 2, 8, H0)
            ha, hb = a.cpu().numpy().reshape(H0, W0), b.cpu().numpy().reshape(H0, W0)
            assert_same(ha[rows], hb[rows], f"one-frame path against render_bands_ex, camera {f}")
            assert_same(ha[rows], want[f][rows], f"one-frame path, camera {f}")
    finally:
        c3_ctx.set_camera(c3.c_camera())


@pytest.mark.parametrize("fmt", [abi.RT_BANDS_INT32, abi.RT_BANDS_RGB24, abi.RT_BANDS_FRAME])
def test_equal_cameras_equal_render_bands_batch(c3, c3_ctx, fmt):
    import torch
    n, nbytes = 5, H0 * W0 * 4 + 64
    a = torch.full((n * nbytes,), 0x5A, dtype=torch.uint8, device="cuda")
    b = torch.full((n * nbytes,), 0x5A, dtype=torch.uint8, device="cuda")
    c3_ctx.render_path_bands(W0, H0, [c3.c_camera()] * n, 8, 0, 2, a.data_ptr(), nbytes, fmt, _stream())
    c3_ctx.render_bands_batch(W0, H0, 8, 0, 2, n, b.data_ptr(), nbytes, fmt, _stream())
    torch.cuda.synchronize()
    ha, hb = a.cpu().numpy(), b.cpu().numpy()
    assert (hb != 0x5A).any()
    assert np.array_equal(ha, hb), "byte-identical buffers"


def test_three_hundred_replayed_frames_in_one_launch(oracle, c3_ctx):
    import dataclasses
    import torch
    sc = scenes.config("C3").resized(16, 9)
    events = []
    for i in range(300):
        events += [("key", "WASD"[i % 4 if i % 7 else 0]), ("mouse", 9.0 if i % 50 < 25 else -11.0, 0.5 if i % 3 else -1.0),
                   ("frame",)]
    cams = path.replay(sc.c_camera(), events)
    assert len(cams) == 300
    out = torch.full((300, 9, 16), -1, dtype=torch.int32, device="cuda")
    c3_ctx.reset_stats()
    c3_ctx.render_path_bands(16, 9, cams, 9, 0, 1, out.data_ptr(), 16 * 9 * 4, abi.RT_BANDS_INT32, _stream())
    torch.cuda.synchronize()
    host = out.cpu().numpy()
    st = c3_ctx.stats()
    assert st["launches"] == 1
    total = {k: 0 for k in RAYS}
    for f, c in enumerate(cams):
        cam = ((c.position.x, c.position.y, c.position.z), c.yaw, c.pitch)
        px, ost = oracle.render(dataclasses.replace(sc, camera=cam), oracle.MODE_NEAREST, 8)
        assert_same(host[f], px, f"replayed frame {f}")
        for k in RAYS:
            total[k] += ost[k]
    assert ray_counts(st) == total
    assert not np.array_equal(host[0], host[299])


@pytest.mark.parametrize("registered", [True, False])
def test_chunked_render_path(oracle, c3, registered, monkeypatch):
    sc = c3.resized(16, 9)
    cams = (path_cases.cameras(sc) + path_cases.cameras(sc)[1:4])[:8]
    want, ost = path_cases.oracle_frames(oracle, sc)
    order = [0, 1, 2, 3, 4, 5, 1, 2]
    monkeypatch.setenv("RT_PATH_CHUNK_FRAMES", "3")  # read at rt_create: chunks of 3, 3 and 2 frames
    with Context(1) as ctx:
        ctx.set_scene(sc)
        out = np.full((8, 9, 16), -1, dtype=np.int32)
        if registered:
            ctx.register_host(out)
        try:
            ctx.reset_stats()
            got = ctx.render_path(cams, 16, 9, out)
            st = ctx.stats()
        finally:
            if registered:
                ctx.unregister_host(out)
    assert np.shares_memory(got, out)
    for i, f in enumerate(order):
        assert_same(out[i], want[f], f"chunked frame {i} (camera {f}), registered={registered}")
    assert st["launches"] == 3 and st["frames"] == 8
    assert ray_counts(st) == summed(ost, order)


def test_slot_reuse_back_to_back_on_two_streams(oracle, c3, c3_ctx):
    """Six calls go round the four view-table slots, so two slots are filled twice (and the slot that the
    300-frame test grew is cut back by the next call that reaches it), and every frame must still be exact.  This exercises the reuse path; it
    does not prove the event guard: launches this small finish long before their slot comes round again, so a
    missing guard would not make the test fail reliably."""
    import torch
    want, _ = path_cases.oracle_frames(oracle, c3)
    cams = path_cases.cameras(c3)
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    torch.cuda.synchronize()
    # six calls (more than the view-table slots), each with its own cameras and buffer, nothing waited for in between
    picks = [[(i + j) % N for j in range(3)] for i in range(6)]
    outs = [torch.full((3, H0, W0), -1, dtype=torch.int32, device="cuda") for _ in picks]
    torch.cuda.synchronize()
    for i, (pick, out) in enumerate(zip(picks, outs)):
        c3_ctx.render_path_bands(W0, H0, [cams[f] for f in pick], H0, 0, 1, out.data_ptr(), H0 * W0 * 4,
                                 abi.RT_BANDS_INT32, streams[i % 2].cuda_stream)
    torch.cuda.synchronize()
    for i, (pick, out) in enumerate(zip(picks, outs)):
        host = out.cpu().numpy()
        for j, f in enumerate(pick):
            assert_same(host[j], want[f], f"call {i} frame {j} (camera {f})")


def test_counting_off_counts_no_rays_and_changes_no_pixel(oracle, c3, c3_ctx):
    want, _ = path_cases.oracle_frames(oracle, c3)
    cams = path_cases.cameras(c3)
    c3_ctx.reset_stats()
    c3_ctx.render_path(cams, W0, H0)
    before = c3_ctx.stats()
    c3_ctx.set_counting(False)
    try:
        px = c3_ctx.render_path(cams, W0, H0)
        after = c3_ctx.stats()
    finally:
        c3_ctx.set_counting(True)
    assert ray_counts(after) == ray_counts(before), "nothing counted"
    assert after["frames"] == before["frames"] + N and after["pixels"] == before["pixels"] + N * W0 * H0
    for f in range(N):
        assert_same(px[f], want[f], f"counting off, frame {f}")


def test_context_camera_and_view_survive_a_path_call(oracle, c3, c3_ctx):
    want, _ = path_cases.oracle_frames(oracle, c3)
    cams = path_cases.cameras(c3)
    own = path_cases.moved(c3, path_cases.OFFSETS[3])
    c3_ctx.set_camera(own.c_camera())
    try:
        assert_same(c3_ctx.render(W0, H0).copy(), want[3], "rt_render before the path call")
        c3_ctx.render_path(cams[:3], W0, H0)
        got = c3_ctx.get_camera()
        assert (got.position.x, got.position.z, got.yaw, got.pitch) == (
            own.c_camera().position.x, own.c_camera().position.z, own.c_camera().yaw, own.c_camera().pitch)
        assert_same(c3_ctx.render(W0, H0).copy(), want[3], "rt_render after the path call")
    finally:
        c3_ctx.set_camera(c3.c_camera())


def test_view_height_applies_to_every_frame(oracle, c3, c3_ctx):
    want, ost = path_cases.oracle_frames(oracle, c3, W0, 22, view_h=H0)
    c3_ctx.set_view_height(H0)
    try:
        c3_ctx.reset_stats()
        px = c3_ctx.render_path(path_cases.cameras(c3), W0, 22)
        for f in range(N):
            assert_same(px[f], want[f], f"50x22 of a 50x30 view, frame {f}")
        assert ray_counts(c3_ctx.stats()) == summed(ost)
        with pytest.raises(abi.RayTracerError) as ei:
            c3_ctx.render_path(path_cases.cameras(c3), W0, H0 + 1)
        assert ei.value.code == abi.RT_ERR_INVALID_ARG
    finally:
        c3_ctx.set_view_height(0)


def _code(fn):
    with pytest.raises(abi.RayTracerError) as ei:
        fn()
    return ei.value.code


def test_errors(c3, c3_ctx):
    import torch
    cam = c3.c_camera()
    out = torch.full((2 * H0 * W0,), -1, dtype=torch.int32, device="cuda")
    st, fb = _stream(), H0 * W0 * 4
    bands = lambda cams, stride=fb, ctx=c3_ctx: ctx.render_path_bands(  # noqa: E731
        W0, H0, cams, 8, 0, 1, out.data_ptr(), stride, abi.RT_BANDS_INT32, st)
    assert _code(lambda: bands([])) == abi.RT_ERR_INVALID_ARG
    assert _code(lambda: c3_ctx.render_path([], W0, H0, np.zeros(0, dtype=np.int32))) == abi.RT_ERR_INVALID_ARG
    too_many = (abi.rt_camera * (abi.RT_MAX_PATH_FRAMES + 1))()
    assert _code(lambda: bands(too_many)) == abi.RT_ERR_INVALID_ARG
    lib = c3_ctx.lib
    assert lib.rt_render_path(c3_ctx.ptr, W0, H0, too_many, len(too_many), C.c_void_p(8)) == abi.RT_ERR_INVALID_ARG
    assert lib.rt_render_path_bands(c3_ctx.ptr, W0, H0, None, 2, 8, 0, 1, C.c_void_p(out.data_ptr()), fb,
                                    abi.RT_BANDS_INT32, C.c_void_p(st), None) == abi.RT_ERR_INVALID_ARG
    assert _code(lambda: bands([cam, cam], fb - 4)) == abi.RT_ERR_INVALID_ARG, "a stride below a frame's output"
    assert _code(lambda: c3_ctx.render_path_bands(W0, H0, [cam], 0, 0, 1, out.data_ptr(), fb, abi.RT_BANDS_INT32,
                                                  st)) == abi.RT_ERR_INVALID_ARG
    c3_ctx.set_supersampling(2)
    try:
        assert _code(lambda: bands([cam, cam])) == abi.RT_ERR_UNSUPPORTED
        assert _code(lambda: c3_ctx.render_path([cam], W0, H0)) == abi.RT_ERR_UNSUPPORTED
    finally:
        c3_ctx.set_supersampling(1)
    with Context(2, abi.RT_CREATE_SHARED_DEVICE) as two:
        two.set_scene(c3)
        assert _code(lambda: bands([cam, cam], fb, two)) == abi.RT_ERR_INVALID_ARG
        assert _code(lambda: two.render_path([cam], W0, H0)) == abi.RT_ERR_INVALID_ARG
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == -1).all(), "a refused call writes nothing"
