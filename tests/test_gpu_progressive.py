"""Progressive accumulation (rt_set_progressive) on the GPU: every frame of a run bit-exact against the definition,
supersample.progressive_resolve of the oracle's k W x k H frame, through every Tick call; the restarts; the calls that
must not disturb a run; the statistics.  tests/test_progressive.py asserts the precondition: consecutive frames P_c
differ, so a wrong order, divisor or count cannot pass.  Each oracle render is computed once per process and shared
read-only (tests/adaptive_cases.py)."""
import ctypes as C

import numpy as np
import pytest

import adaptive_cases as ac
from raytracer_hip import Context, abi, path
from raytracer_hip.supersample import progressive_resolve
from test_gpu_supersample import assert_same, ray_counts

pytestmark = pytest.mark.gpu

_WANT = {}


def want(oracle, cid, W, H, k, c, view_h=None):
    """P_c [H, W] of the scene at factor k (rows [0, H) of a view view_h rows high)."""
    key = (cid, W, H, k, c, view_h)
    if key not in _WANT:
        out = progressive_resolve(ac.frames(oracle, cid, W, H, k, view_h)[0], k, c)
        out.setflags(write=False)
        _WANT[key] = out
    return _WANT[key]


def _stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


def _code(call):
    with pytest.raises(abi.RayTracerError) as ei:
        call()
    return ei.value.code


def _moved(cam, dz=0.125):
    c = abi.rt_camera()
    C.memmove(C.byref(c), C.byref(cam), C.sizeof(c))
    c.position.z += dz
    return c


# (scene of test_gpu_supersample.SCENES, W, H, factors)
RUNS = [
    ("C3", 50, 30, (2, 4, 8)),           # direct, LDS stack
    ("REF", 45, 27, (2, 4, 8)),          # limit 32, scratch stack, ragged
    ("C4", 96, 56, (2, 4, 8)),           # bundle, merged
    ("bundle_L5", 64, 48, (2, 4, 8)),
    ("gpow_direct", 32, 24, (2, 4, 8)),
    ("gpow_bundle", 64, 48, (2,)),
]
K8_TICKS = (1, 2, 3, 4, 5, 16, 17, 63, 64, 65, 66)


@pytest.mark.parametrize("cid,W,H,k", [(cid, W, H, k) for cid, W, H, ks in RUNS for k in ks],
                         ids=lambda v: str(v))
def test_every_count_of_a_run(oracle, cid, W, H, k):
    kk = k * k
    compare = set(range(1, kk + 3)) if k < 8 else set(K8_TICKS)
    with Context(1) as ctx:
        ctx.set_scene(ac.scene(cid).resized(W, H))
        ctx.set_progressive(k)
        assert ctx.progressive() == (k, 0)
        for n in range(1, kk + 3):
            px = ctx.render(W, H)
            c = min(n, kk)
            assert ctx.progressive() == (k, c)
            if n in compare:
                assert_same(px.copy(), want(oracle, cid, W, H, k, c), f"{cid} {W}x{H} k={k} Tick {n} (P_{c})")
    assert_same(want(oracle, cid, W, H, k, 1), ac.frames(oracle, cid, W, H, 1)[0], "P_1 is the plain frame")


W0, H0 = ac.W0, ac.H0


@pytest.fixture(scope="module", params=["C3", "C4"])
def cid(request):
    return request.param


@pytest.fixture(scope="module")
def _ctx0(cid):
    ctx = Context(1)
    ctx.set_scene(ac.scene(cid).resized(W0, H0))
    yield ctx
    ctx.close()


@pytest.fixture
def ctx0(_ctx0, cid):
    """The module's context, with every setting a test may change put back after it."""
    yield _ctx0
    _ctx0.set_progressive(1)
    _ctx0.set_supersampling(1)
    _ctx0.set_counting(True)
    _ctx0.set_view_height(0)
    _ctx0.set_camera(ac.scene(cid).resized(W0, H0).c_camera())


def _ticks(ctx, oracle, cid, k, counts, what, W=W0, H=H0, view_h=None):
    for c in counts:
        px = ctx.render(W, H).copy()
        assert ctx.progressive() == (k, c), f"{what}: the count"
        assert_same(px, want(oracle, cid, W, H, k, c, view_h), f"{what}: P_{c}")


def test_restarts(oracle, cid, ctx0):
    k = 2
    sc = ac.scene(cid).resized(W0, H0)
    cam = sc.c_camera()
    ctx0.set_progressive(k)
    _ticks(ctx0, oracle, cid, k, (1, 2, 3), "a resting camera")
    ctx0.set_camera(cam)  # the same values: no restart
    _ticks(ctx0, oracle, cid, k, (4, 4), "rt_set_camera with unchanged values")
    # a camera step: the moved view's plain frame, then back
    ctx0.set_camera(_moved(cam))
    moved = ctx0.render(W0, H0).copy()
    assert ctx0.progressive() == (k, 1)
    assert (moved != want(oracle, cid, W0, H0, k, 1)).any(), "the camera moved"
    ctx0.set_camera(cam)
    _ticks(ctx0, oracle, cid, k, (1, 2, 3), "after a camera step")
    ctx0.set_scene(sc)  # (also sets the scene's camera)
    _ticks(ctx0, oracle, cid, k, (1, 2), "after rt_set_scene")
    ctx0.reset_progressive()
    _ticks(ctx0, oracle, cid, k, (1, 2, 3, 4), "after rt_reset_progressive")
    ctx0.reset_progressive()
    _ticks(ctx0, oracle, cid, k, (1, 2), "a reset of a converged run")
    # a size change and back
    ctx0.render(W0, H0 - 8)
    assert ctx0.progressive() == (k, 1)
    _ticks(ctx0, oracle, cid, k, (1, 2, 3), "after a size change")
    # the view height
    ctx0.set_view_height(H0 + 10)
    _ticks(ctx0, oracle, cid, k, (1, 2, 3, 4, 4), "with a view height above the height", view_h=H0 + 10)
    ctx0.set_view_height(0)
    _ticks(ctx0, oracle, cid, k, (1, 2), "after rt_set_view_height")
    # another factor
    ctx0.set_progressive(4)
    _ticks(ctx0, oracle, cid, 4, (1, 2, 3, 4, 5), "after rt_set_progressive(4)")
    ctx0.set_progressive(4)
    _ticks(ctx0, oracle, cid, 4, (6,), "rt_set_progressive with the same factor")
    ctx0.set_progressive(k)
    _ticks(ctx0, oracle, cid, k, (1, 2), "after rt_set_progressive(2)")


@pytest.mark.parametrize("mode", ["default", "slice"])
def test_render_async_six_frames_in_two_buffers(oracle, cid, ctx0, monkeypatch, mode):
    if mode == "slice":
        monkeypatch.setenv("RT_TICK_ASYNC", "slice")
    k = 4
    cam = ac.scene(cid).resized(W0, H0).c_camera()
    ctx0.set_progressive(k)
    for registered in (True, False):
        ctx0.reset_progressive()
        ctx0.set_camera(cam)
        bufs = [np.full(W0 * H0, -1, dtype=np.int32) for _ in range(2)]
        if registered:
            for b in bufs:
                ctx0.register_host(b)
        try:
            got = []
            for f in range(6):
                if f == 3:  # the camera changes at frame 4 ...
                    ctx0.set_camera(_moved(cam))
                ctx0.render_async(W0, H0, bufs[f % 2])
                assert ctx0.progressive() == (k, (1, 2, 3, 1, 2, 3)[f])
                if f % 2 == 1:  # both buffers hold a frame: collect them before they are traced again
                    ctx0.wait()
                    got += [bufs[0].reshape(H0, W0).copy(), bufs[1].reshape(H0, W0).copy()]
            ctx0.set_camera(cam)  # (after the calls: no queued frame may see it)
        finally:
            if registered:
                for b in bufs:
                    ctx0.unregister_host(b)
        for f in range(3):
            assert_same(got[f], want(oracle, cid, W0, H0, k, f + 1), f"async frame {f + 1} (registered {registered}, {mode})")
        # ... and frames 4-6 are P_1, P_2, P_3 of the moved view: checked against a synchronous run of it
        ctx0.reset_progressive()
        ctx0.set_camera(_moved(cam))
        for f in range(3):
            assert_same(got[3 + f], ctx0.render(W0, H0).copy(), f"async frame {4 + f} against the synchronous run")
        assert (got[3] != got[0]).any() and (got[4] != got[3]).any() and (got[5] != got[4]).any()


def test_two_frames_in_flight(oracle, cid, ctx0):
    k = 2
    ctx0.set_progressive(k)
    bufs = [np.full(W0 * H0, -1, dtype=np.int32) for _ in range(6)]
    for b in bufs:
        ctx0.render_async(W0, H0, b)
    ctx0.wait()
    for n, b in enumerate(bufs):
        c = min(n + 1, 4)
        assert_same(b.reshape(H0, W0), want(oracle, cid, W0, H0, k, c), f"queued frame {n + 1} (P_{c})")
    # a synchronous Tick and a device Tick go on with the same run
    _ticks(ctx0, oracle, cid, k, (4,), "rt_render after rt_render_async")


def test_render_device_into_a_tensor(oracle, cid, ctx0):
    import torch
    k = 2
    ctx0.set_progressive(k)
    out = torch.full((H0 * W0 + 64,), -1, dtype=torch.int32, device="cuda")
    for n in range(1, 7):
        ctx0.render_device(W0, H0, out.data_ptr(), _stream())
        torch.cuda.synchronize()
        host = out.cpu().numpy()
        c = min(n, 4)
        assert ctx0.progressive() == (k, c)
        assert_same(host[:H0 * W0].reshape(H0, W0), want(oracle, cid, W0, H0, k, c), f"rt_render_device Tick {n}")
        assert (host[H0 * W0:] == -1).all(), "nothing written past the width x height output"
    # the Tick calls share one run: rt_render, rt_render_async and rt_render_device in turn
    ctx0.reset_progressive()
    a = np.full(W0 * H0, -1, dtype=np.int32)
    assert_same(ctx0.render(W0, H0).copy(), want(oracle, cid, W0, H0, k, 1), "rt_render, Tick 1")
    ctx0.render_async(W0, H0, a)
    ctx0.render_device(W0, H0, out.data_ptr(), _stream())
    ctx0.wait()
    torch.cuda.synchronize()
    assert_same(a.reshape(H0, W0), want(oracle, cid, W0, H0, k, 2), "rt_render_async, Tick 2")
    assert_same(out.cpu().numpy()[:H0 * W0].reshape(H0, W0), want(oracle, cid, W0, H0, k, 3), "rt_render_device, Tick 3")
    _ticks(ctx0, oracle, cid, k, (4, 4), "rt_render, Ticks 4 and 5")


@pytest.mark.parametrize("workers", [2, 3])
def test_shared_device_contexts(oracle, cid, workers):
    import torch
    k = 2
    with Context(workers, abi.RT_CREATE_SHARED_DEVICE) as ctx:
        ctx.set_scene(ac.scene(cid).resized(W0, H0))
        ctx.set_progressive(k)
        _ticks(ctx, oracle, cid, k, (1, 2, 3, 4, 4), f"{workers} workers rt_render")
        ctx.reset_progressive()
        pinned = np.full(W0 * H0, -1, dtype=np.int32)
        ctx.register_host(pinned)
        try:
            for c in (1, 2, 3):
                ctx.render(W0, H0, pinned)
                assert_same(pinned.reshape(H0, W0), want(oracle, cid, W0, H0, k, c), f"{workers} workers, registered frame, P_{c}")
            a = np.full(W0 * H0, -1, dtype=np.int32)
            ctx.render_async(W0, H0, pinned)
            ctx.render_async(W0, H0, a)
            ctx.wait()
            assert_same(pinned.reshape(H0, W0), want(oracle, cid, W0, H0, k, 4), f"{workers} workers rt_render_async")
            assert_same(a.reshape(H0, W0), want(oracle, cid, W0, H0, k, 4), f"{workers} workers rt_render_async, converged")
        finally:
            ctx.unregister_host(pinned)
        ctx.reset_progressive()
        out = torch.full((H0 * W0,), -1, dtype=torch.int32, device="cuda")
        for c in (1, 2, 3, 4, 4):
            ctx.render_device(W0, H0, out.data_ptr(), _stream())
            torch.cuda.synchronize()
            assert_same(out.cpu().numpy().reshape(H0, W0), want(oracle, cid, W0, H0, k, c), f"{workers} workers rt_render_device P_{c}")


@pytest.mark.parametrize("copy", ["kernel", "stream"])
def test_registered_buffer_in_two_chunks(oracle, monkeypatch, copy):
    cid, W, H, k = "bundle_L5", 64, 48, 2
    monkeypatch.setenv("RT_TICK_CHUNKS", "2")
    monkeypatch.setenv("RT_TICK_COPY", copy)  # kernel: chunk 0's copy rides in chunk 1's PROG launch as its copy slice
    with Context(1) as ctx:
        ctx.set_scene(ac.scene(cid).resized(W, H))
        ctx.set_progressive(k)
        pinned = np.full(W * H, -1, dtype=np.int32)
        ctx.register_host(pinned)
        try:
            for n in range(1, 7):
                ctx.render(W, H, pinned)
                c = min(n, 4)
                assert_same(pinned.reshape(H, W), want(oracle, cid, W, H, k, c), f"chunked Tick {n} ({copy})")
            # an unregistered frame takes one chunk: the plan of the share changes, the accumulator's layout does not
            plain = ctx.render(W, H).copy()
            assert_same(plain, want(oracle, cid, W, H, k, 4), "an unchunked Tick after chunked ones")
        finally:
            ctx.unregister_host(pinned)


def test_other_renders_do_not_disturb_a_run(oracle, cid, ctx0):
    import torch
    k = 2
    sc = ac.scene(cid).resized(W0, H0)
    cam = sc.c_camera()
    with Context(1) as fresh:  # what the calls return today: a context that never heard of the feature
        fresh.set_scene(sc)
        bands0 = torch.full((H0 * W0,), -1, dtype=torch.int32, device="cuda")
        fresh.render_bands_ex(W0, H0, 8, 0, 1, bands0.data_ptr(), abi.RT_BANDS_INT32, _stream())
        torch.cuda.synchronize()
        cams = path.as_array([cam, _moved(cam)])
        path0 = fresh.render_path(cams, W0, H0).copy()
        work0 = fresh.count_work(W0, H0)
    ctx0.set_progressive(k)
    _ticks(ctx0, oracle, cid, k, (1, 2), "before the other renders")
    bands = torch.full((H0 * W0,), -1, dtype=torch.int32, device="cuda")
    ctx0.render_bands_ex(W0, H0, 8, 0, 1, bands.data_ptr(), abi.RT_BANDS_INT32, _stream())
    torch.cuda.synchronize()
    assert torch.equal(bands, bands0), "rt_render_bands_ex ignores the setting"
    assert_same(bands.cpu().numpy().reshape(H0, W0), want(oracle, cid, W0, H0, k, 1), "rt_render_bands_ex is the plain frame")
    assert np.array_equal(ctx0.render_path(cams, W0, H0), path0), "rt_render_path ignores the setting"
    assert ctx0.count_work(W0, H0) == work0, "rt_count_work ignores the setting"
    assert ctx0.progressive() == (k, 2)
    _ticks(ctx0, oracle, cid, k, (3, 4, 4), "after the other renders")


def test_off_is_off(oracle, cid, ctx0):
    sc = ac.scene(cid).resized(W0, H0)

    def three(ctx):
        ctx.reset_stats()
        frames = [ctx.render(W0, H0).copy() for _ in range(3)]
        st = ctx.stats()
        return frames, {key: st[key] for key in ("frames", "pixels", "launches", "primary_rays", "reflect_rays", "shadow_rays")}

    with Context(1) as fresh:
        fresh.set_scene(sc)
        f0, s0 = three(fresh)
    assert ctx0.progressive()[0] == 1
    f1, s1 = three(ctx0)
    assert ctx0.progressive() == (1, 1)
    ctx0.set_progressive(4)
    _ticks(ctx0, oracle, cid, 4, (1, 2, 3), "on")
    ctx0.set_progressive(1)
    f2, s2 = three(ctx0)
    assert s0 == s1 == s2, "k = 1: the statistics of a fresh context"
    for a, b, c in zip(f0, f1, f2):
        assert_same(a, ac.frames(oracle, cid, W0, H0, 1)[0], "the plain frame")
        assert_same(b, a, "k = 1 by default")
        assert_same(c, a, "k = 1 after rt_set_progressive(1)")


def test_errors(oracle, cid, ctx0):
    for bad in (0, 3, 5, 16, -2):
        assert _code(lambda: ctx0.set_progressive(bad)) == abi.RT_ERR_INVALID_ARG
    assert ctx0.progressive()[0] == 1
    k = C.c_int(5)
    assert ctx0.lib.rt_get_progressive(ctx0.ptr, None, C.byref(k)) == abi.RT_ERR_INVALID_ARG
    assert ctx0.lib.rt_get_progressive(ctx0.ptr, C.byref(k), None) == abi.RT_ERR_INVALID_ARG and k.value == 5
    ctx0.set_progressive(2)
    ctx0.set_supersampling(2)
    out = np.full(W0 * H0, -1, dtype=np.int32)
    assert _code(lambda: ctx0.render(W0, H0, out)) == abi.RT_ERR_UNSUPPORTED
    assert _code(lambda: ctx0.render_async(W0, H0, out)) == abi.RT_ERR_UNSUPPORTED
    import torch
    dev = torch.full((H0 * W0,), -1, dtype=torch.int32, device="cuda")
    assert _code(lambda: ctx0.render_device(W0, H0, dev.data_ptr(), _stream())) == abi.RT_ERR_UNSUPPORTED
    ctx0.wait()
    torch.cuda.synchronize()
    assert (out == -1).all() and (dev.cpu().numpy() == -1).all(), "a refused Tick writes nothing"
    ctx0.set_supersampling(1)
    _ticks(ctx0, oracle, cid, 2, (1, 2, 3, 4), "after rt_set_supersampling(1)")
    # k W * k H above 2^31 - 1
    ctx0.set_progressive(8)
    assert _code(lambda: ctx0.render_device(8192, 4097, dev.data_ptr(), _stream())) == abi.RT_ERR_INVALID_ARG


def test_stats_of_a_run(oracle):
    cid, k = "C3", 2
    _, big = ac.frames(oracle, cid, W0, H0, k)
    _, plain = ac.frames(oracle, cid, W0, H0, 1)
    with Context(1) as ctx:
        ctx.set_scene(ac.scene(cid).resized(W0, H0))
        ctx.set_progressive(k)
        ctx.reset_stats()
        primary = []
        before = 0
        for n in range(6):
            ctx.render(W0, H0)
            st = ctx.stats()
            primary.append(st["primary_rays"] - before)
            before = st["primary_rays"]
            assert st["frames"] == n + 1 and st["pixels"] == (n + 1) * W0 * H0, "converged Ticks still count"
        assert primary == [W0 * H0, 2 * W0 * H0, W0 * H0, W0 * H0, 0, 0]
        # sample 0 is traced twice: by the plain launch of Tick 1 and by the launch that starts the accumulator
        assert st["reflect_rays"] == big["reflect_rays"] + plain["reflect_rays"]
        assert st["shadow_rays"] == big["shadow_rays"] + plain["shadow_rays"]
        assert st["launches"] == 6
        # counting off: the same frames, nothing counted
        ctx.set_counting(False)
        ctx.reset_progressive()
        ctx.reset_stats()
        for c in (1, 2, 3, 4, 4):
            assert_same(ctx.render(W0, H0).copy(), want(oracle, cid, W0, H0, k, c), f"counting off, P_{c}")
        assert ray_counts(ctx.stats()) == {"primary_rays": 0, "reflect_rays": 0, "shadow_rays": 0}
