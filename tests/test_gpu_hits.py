"""Hit buffers and picking on the GPU (rt_render_hits*, rt_render_path_hits*, rt_render_anim_hits*, rt_pick): every
channel bit for bit -- uint32 views, so NaN patterns and the sign of zero count -- against tests/hit_cases.py
expected_hits, which tests/test_hits.py pins to the unchanged oracle.  Frames of at most 96 x 54."""
import ctypes as C
import dataclasses

import numpy as np
import pytest

import adaptive_cases as ac
import hit_cases
from hit_cases import CHANNELS, bits, expected_hits, with_camera
from raytracer_hip import Context, RayTracerError, abi, anim, path, scenes
from raytracer_hip.supersample import progressive_resolve

pytestmark = pytest.mark.gpu

WORDS = {"depth": 1, "object": 1, "position": 3, "normal": 3}  # 32-bit words per pixel
SENTINEL = 0x5EA15EA1


def _stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


def assert_hits(got, want, what, channels=CHANNELS):
    for c in channels:
        g, w = bits(got[c]), bits(want[c])
        assert g.shape == w.shape, f"{what} {c}: shape {g.shape}, expected {w.shape}"
        bad = g != w
        if bad.any():
            i = tuple(int(v) for v in np.argwhere(bad)[0])
            pytest.fail(f"{what} {c}: {int(bad.sum())} of {bad.size} words differ; first at {i}: gpu {int(g[i]):#010x} "
                        f"expected {int(w[i]):#010x}")


def device_hits(call, n, W, H, channels=CHANNELS):
    """The channels of an n-frame device call, each buffer one frame of sentinel words longer than it needs: `call`
    gets {channel: device pointer}.  Asserts that the sentinels survive; returns {channel: array with a frame axis}."""
    import torch
    bufs = {c: torch.full(((n + 1) * W * H * WORDS[c],), SENTINEL, dtype=torch.int32, device="cuda") for c in channels}
    call(**{c: b.data_ptr() for c, b in bufs.items()})
    torch.cuda.synchronize()
    out = {}
    for c, b in bufs.items():
        host = b.cpu().numpy()
        k = n * W * H * WORDS[c]
        assert (host[k:] == SENTINEL).all(), f"{c}: words behind the last frame were written"
        shape = (n, H, W) + ((3,) if WORDS[c] == 3 else ())
        out[c] = host[:k].view(np.int32 if c == "object" else np.float32).reshape(shape)
    return out


def _code(call):
    with pytest.raises(RayTracerError) as ei:
        call()
    return ei.value.code


@pytest.fixture(scope="module")
def ctx():
    with Context(1) as c:
        yield c


def _set(ctx, scene, rows=None):
    ctx.set_scene(scene)
    ctx.set_view_height(scene.height if rows else 0)
    return scene.width, rows or scene.height


# ---- 1. every case, host and device call --------------------------------------------------------------------------
@pytest.mark.parametrize("scene,rows", hit_cases.CASES, ids=hit_cases.CASE_IDS)
def test_every_case_host_and_device(ctx, scene, rows):
    want = expected_hits(scene, rows)
    try:
        W, H = _set(ctx, scene, rows)
        assert_hits(ctx.render_hits(W, H), want, f"{scene.name} rt_render_hits")
        dev = device_hits(lambda **p: ctx.render_hits_device(W, H, stream=_stream(), **p), 1, W, H)
        assert_hits({c: a[0] for c, a in dev.items()}, want, f"{scene.name} rt_render_hits_device")
    finally:
        ctx.set_view_height(0)


# ---- 2. partial tiles on both axes --------------------------------------------------------------------------------
@pytest.mark.parametrize("W,H", [(1, 1), (8, 8), (9, 8), (13, 11), (37, 21)])
def test_frame_sizes(ctx, W, H):
    sc = scenes.reference(W, H).resized(W, H, "hits_ref")
    ctx.set_scene(sc)
    assert_hits(ctx.render_hits(W, H), expected_hits(sc), f"{W}x{H}")
    dev = device_hits(lambda **p: ctx.render_hits_device(W, H, stream=_stream(), **p), 1, W, H)
    assert_hits({c: a[0] for c, a in dev.items()}, expected_hits(sc), f"{W}x{H} device")


# ---- 3. channel subsets -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("channels", [("depth",), ("object",), ("position",), ("normal",), ("depth", "object")],
                         ids=lambda c: "+".join(c))
def test_channel_subsets(ctx, channels):
    sc = scenes.config("C3").resized(37, 21, "hits_C3")
    cams = [m.c_camera() for m in (sc, dataclasses.replace(sc, camera=(scenes.vec(0.5, 0, 0.25), 0.25, 0.0)))]
    ctx.set_scene(sc)
    W, H = sc.width, sc.height
    want = [expected_hits(with_camera(sc, c)) for c in cams]
    host = ctx.render_hits(W, H, channels)
    assert set(host) == set(channels)
    assert_hits(host, want[0], "host subset", channels)
    dev = device_hits(lambda **p: ctx.render_path_hits_device(W, H, cams, stream=_stream(), **p), 2, W, H, channels)
    for f in range(2):
        assert_hits({c: a[f] for c, a in dev.items()}, want[f], f"device subset frame {f}", channels)


def test_no_channel_is_refused(ctx, rtlib):
    sc = scenes.reference(16, 16)
    ctx.set_scene(sc)
    empty = abi.rt_hit_buffers()
    cams = path.as_array([sc.c_camera()])
    assert rtlib.rt_render_hits(ctx.ptr, 16, 16, C.byref(empty)) == abi.RT_ERR_INVALID_ARG
    assert rtlib.rt_render_hits(ctx.ptr, 16, 16, None) == abi.RT_ERR_INVALID_ARG
    assert rtlib.rt_render_hits_device(ctx.ptr, 16, 16, C.byref(empty), None) == abi.RT_ERR_INVALID_ARG
    assert rtlib.rt_render_hits_device(ctx.ptr, 16, 16, None, None) == abi.RT_ERR_INVALID_ARG
    assert rtlib.rt_render_path_hits(ctx.ptr, 16, 16, cams, 1, C.byref(empty)) == abi.RT_ERR_INVALID_ARG
    assert rtlib.rt_render_path_hits_device(ctx.ptr, 16, 16, cams, 1, None, None) == abi.RT_ERR_INVALID_ARG


# ---- 4. camera paths ----------------------------------------------------------------------------------------------
EVENTS = [("key", "W"), ("mouse", 40.0, -12.0), ("frame",), ("key", "D"), ("key", "D"), ("mouse", -90.0, 25.0), ("frame",),
          ("key", "Space"), ("key", "S"), ("mouse", 15.0, 30.0), ("frame",)]


def test_path_frames(ctx):
    sc = scenes.config("C3").resized(40, 24, "hits_C3")
    W, H = sc.width, sc.height
    ctx.set_scene(sc)
    cams = path.replay(sc.c_camera(), EVENTS)
    assert len(cams) == 3
    own = ctx.get_camera()
    got = ctx.render_path_hits(cams, W, H)
    dev = device_hits(lambda **p: ctx.render_path_hits_device(W, H, cams, stream=_stream(), **p), 3, W, H)
    after = ctx.get_camera()
    assert bytes(own) == bytes(after), "the context's camera is unchanged"
    wants = [expected_hits(with_camera(sc, c)) for c in cams]
    assert not np.array_equal(wants[0]["object"], wants[1]["object"]) and not np.array_equal(wants[1]["depth"], wants[2]["depth"])
    for f, c in enumerate(cams):
        assert_hits({k: a[f] for k, a in got.items()}, wants[f], f"path frame {f}")
        assert_hits({k: a[f] for k, a in dev.items()}, wants[f], f"path frame {f} (device)")
        one = ctx.render_path_hits([c], W, H)
        assert_hits({k: a[0] for k, a in one.items()}, wants[f], f"n_frames == 1, camera {f}")
    try:
        for f, c in enumerate(cams):
            ctx.set_camera(c)
            assert_hits(ctx.render_hits(W, H), {k: a[f] for k, a in got.items()}, f"rt_set_camera + rt_render_hits, camera {f}")
    finally:
        ctx.set_camera(own)


def test_path_argument_errors(ctx, rtlib):
    sc = scenes.reference(16, 16)
    ctx.set_scene(sc)
    out = np.zeros(16 * 16, np.float32)
    bufs = abi.rt_hit_buffers(depth=out.ctypes.data)
    cams = path.as_array([sc.c_camera()])
    for n in (0, -1, abi.RT_MAX_PATH_FRAMES + 1):
        assert rtlib.rt_render_path_hits(ctx.ptr, 16, 16, cams, n, C.byref(bufs)) == abi.RT_ERR_INVALID_ARG
        assert rtlib.rt_render_path_hits_device(ctx.ptr, 16, 16, cams, n, C.byref(bufs), None) == abi.RT_ERR_INVALID_ARG
    assert rtlib.rt_render_path_hits(ctx.ptr, 16, 16, None, 1, C.byref(bufs)) == abi.RT_ERR_INVALID_ARG
    assert rtlib.rt_render_path_hits(ctx.ptr, 0, 16, cams, 1, C.byref(bufs)) == abi.RT_ERR_INVALID_ARG
    with Context(1) as bare:
        assert rtlib.rt_render_path_hits(bare.ptr, 16, 16, cams, 1, C.byref(bufs)) == abi.RT_ERR_NO_SCENE
        assert rtlib.rt_render_hits(bare.ptr, 16, 16, C.byref(bufs)) == abi.RT_ERR_NO_SCENE


# ---- 5. scene tracks ----------------------------------------------------------------------------------------------
def _track():
    a = scenes.config("C3").resized(40, 24, "hits_track")
    sph = list(a.spheres)
    sph[1] = scenes.Sphere(scenes.vec(-3, 0.5, 5), sph[1].radius, sph[1].material)
    lights = [scenes.Light(scenes.vec(5, 6, -3), a.lights[0].intensity)] + list(a.lights[1:])
    b = dataclasses.replace(a, spheres=sph, lights=lights)
    frames = anim.tween([a, b], 2)  # 3 frames
    cams = path.replay(a.c_camera(), EVENTS)
    return [dataclasses.replace(with_camera(sc, cams[f]), name=f"hits_track#{f}") for f, sc in enumerate(frames)]


def test_track_frames_and_argument_errors(ctx, rtlib):
    import torch
    track = _track()
    assert len(track) == 3
    W, H = track[0].width, track[0].height
    ctx.set_scene(scenes.reference(W, H))  # (the context's own scene plays no part)
    ctx.set_scene_track(track)
    try:
        cams = [sc.c_camera() for sc in track[1:]]
        wants = [expected_hits(sc) for sc in track[1:]]
        assert not np.array_equal(wants[0]["position"], wants[1]["position"])
        got = ctx.render_anim_hits(cams, W, H, first_frame=1, n_frames=2)
        own = ctx.render_anim_hits(None, W, H, first_frame=1, n_frames=2)
        dev = device_hits(lambda **p: ctx.render_anim_hits_device(W, H, cams, stream=_stream(), first_frame=1, **p), 2, W, H)
        for f in range(2):
            for what, g in (("host", got), ("own cameras", own), ("device", dev)):
                assert_hits({k: a[f] for k, a in g.items()}, wants[f], f"track frame {1 + f} ({what})")
        # the refusals of rt_render_anim_bands, for the same bad arguments
        out = torch.zeros(4 * W * H, dtype=torch.int32, device="cuda")
        bufs = abi.rt_hit_buffers(object=out.data_ptr())
        arr = path.as_array(cams)
        nb = C.c_int(0)
        for cm, first, n in ((arr, -1, 2), (arr, 2, 2), (arr, 0, 4), (arr, 3, 1), (arr, 0, 0), (arr, 0, -3),
                             (arr, 0, abi.RT_MAX_PATH_FRAMES + 1), (None, 0, 2)):
            bands = rtlib.rt_render_anim_bands(ctx.ptr, W, H, cm, first, n, H, 0, 1, C.c_void_p(out.data_ptr()), W * H * 4,
                                               abi.RT_BANDS_INT32, None, C.byref(nb))
            assert bands != abi.RT_OK
            assert rtlib.rt_render_anim_hits_device(ctx.ptr, W, H, cm, first, n, C.byref(bufs), None) == bands, (first, n)
            assert rtlib.rt_render_anim_hits(ctx.ptr, W, H, cm, first, n, C.byref(bufs)) == bands, (first, n)
        torch.cuda.synchronize()
    finally:
        ctx.clear_scene_track()
    assert _code(lambda: ctx.render_anim_hits(cams, W, H, first_frame=0)) == abi.RT_ERR_NO_SCENE


# ---- 6. picking ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["hits_C3", "hits_C4", "hits_s80", "hits_view_height"])
def test_pick_equals_the_buffers(ctx, name):
    scene, rows = next(c for c in hit_cases.CASES if c[0].name == name)
    try:
        W, H = _set(ctx, scene, rows)
        hits = ctx.render_hits(W, H)
        rng = np.random.default_rng(20261021)
        pixels = [(0, 0), (W - 1, 0), (0, H - 1), (W - 1, H - 1), (W // 2, H // 2)]
        pixels += [(int(rng.integers(0, W)), int(rng.integers(0, H))) for _ in range(16)]
        none = 0
        for x, y in pixels:
            p = ctx.pick(W, H, x, y)
            got = {"object": np.int32(p["object"]), "depth": np.float32(p["depth"]),
                   "position": np.array(p["position"], np.float32), "normal": np.array(p["normal"], np.float32)}
            assert_hits(got, {c: hits[c][y, x] for c in CHANNELS}, f"{name} pick ({x}, {y})")
            none += p["object"] == abi.RT_HIT_NONE
        if name == "hits_C3":
            assert none > 0, "the corners of the C3 frame see nothing"
        for x, y in ((-1, 0), (W, 0), (0, -1), (0, H)):
            assert _code(lambda: ctx.pick(W, H, x, y)) == abi.RT_ERR_INVALID_ARG
        assert ctx.lib.rt_pick(ctx.ptr, W, H, 0, 0, None) == abi.RT_ERR_INVALID_ARG
    finally:
        ctx.set_view_height(0)


# ---- 7. non-interference ------------------------------------------------------------------------------------------
def _all_hit_calls(ctx, W, H, cams):
    ctx.render_hits(W, H)
    ctx.render_path_hits(cams, W, H)
    ctx.pick(W, H, W // 2, H // 2)
    return device_hits(lambda **p: ctx.render_hits_device(W, H, stream=_stream(), **p), 1, W, H)


def test_renders_and_stats_are_untouched():
    sc = scenes.config("C3").resized(50, 30, "hits_C3")
    W, H = sc.width, sc.height
    cams = path.replay(sc.c_camera(), EVENTS)
    with Context(1) as c:
        c.set_scene(sc)
        c.set_timing(0)  # nothing is timed: the time fields stay 0 too
        before = c.render(W, H).copy()
        order = c.dispatch_order()
        st = c.stats()
        _all_hit_calls(c, W, H, cams)
        assert c.stats() == st, "rt_get_stats, field for field"
        assert c.dispatch_order() == order
        c.set_counting(False)
        _all_hit_calls(c, W, H, cams)
        c.set_counting(True)
        assert c.stats() == st
        assert np.array_equal(c.render(W, H), before)


def test_sampling_settings_are_ignored():
    sc = scenes.config("C3").resized(40, 24, "hits_C3")
    W, H = sc.width, sc.height
    cams = path.replay(sc.c_camera(), EVENTS)
    want = expected_hits(sc)
    with Context(1) as c:
        c.set_scene(sc)
        c.set_supersampling(2)
        c.set_adaptive_sampling(16)
        c.set_path_supersampling(4)
        c.set_path_adaptive_sampling(16)
        assert_hits(c.render_hits(W, H), want, "rt_render_hits under the sampling settings")
        got = c.render_path_hits(cams, W, H)
        for f, cam in enumerate(cams):
            assert_hits({k: a[f] for k, a in got.items()}, expected_hits(with_camera(sc, cam)), f"path frame {f} under the settings")
        p = c.pick(W, H, 20, 20)
        assert p["object"] == want["object"][20, 20] and bits(np.float32(p["depth"])) == bits(want["depth"][20, 20])
        assert c.supersampling == 2 and c.get_path_supersampling() == 4


def test_a_progressive_run_is_not_disturbed(oracle):
    cid, W, H, k = "C3", 50, 30, 2
    sc = ac.scene(cid).resized(W, H)
    samples = ac.frames(oracle, cid, W, H, k, None)[0]
    cams = path.replay(sc.c_camera(), EVENTS)
    with Context(1) as c:
        c.set_scene(sc)
        c.set_progressive(k)
        for n in (1, 2):
            assert np.array_equal(c.render(W, H), progressive_resolve(samples, k, n))
        assert c.progressive() == (k, 2)
        _all_hit_calls(c, W, H, cams)
        assert c.progressive() == (k, 2), "a hit call between Ticks leaves the sample count"
        assert np.array_equal(c.render(W, H), progressive_resolve(samples, k, 3)), "the next Tick is P_3"
        assert c.progressive() == (k, 3)


# ---- 8. the sky-wave shortcut against the traced result -------------------------------------------------------------
def test_sky_waves_store_what_tracing_gives(monkeypatch):
    sc = scenes.config("C3").resized(96, 54, "hits_C3")
    got = {}
    for foot in ("0", None):
        if foot is None:
            monkeypatch.delenv("RT_PRIM_FOOT", raising=False)
        else:
            monkeypatch.setenv("RT_PRIM_FOOT", foot)
        with Context(1) as c:
            c.set_scene(sc)  # (rt_set_scene reads the switch)
            got[foot] = c.render_hits(96, 54)
    assert_hits(got["0"], got[None], "RT_PRIM_FOOT=0 against the default")
    assert_hits(got[None], expected_hits(sc), "default")
    assert (got[None]["object"][:8] == abi.RT_HIT_NONE).all(), "the top tile row of the C3 frame is sky"


# ---- 9. more than one worker -------------------------------------------------------------------------------------
def test_contexts_with_two_workers_are_refused(rtlib):
    sc = scenes.reference(16, 16)
    with Context(2, abi.RT_CREATE_SHARED_DEVICE) as c:
        c.set_scene(sc)
        out = np.zeros(16 * 16, np.float32)
        bufs = abi.rt_hit_buffers(depth=out.ctypes.data)
        cams = path.as_array([sc.c_camera()])
        pick = abi.rt_pick_result()
        calls = [rtlib.rt_render_hits_device(c.ptr, 16, 16, C.byref(bufs), None),
                 rtlib.rt_render_path_hits_device(c.ptr, 16, 16, cams, 1, C.byref(bufs), None),
                 rtlib.rt_render_anim_hits_device(c.ptr, 16, 16, cams, 0, 1, C.byref(bufs), None),
                 rtlib.rt_render_hits(c.ptr, 16, 16, C.byref(bufs)),
                 rtlib.rt_render_path_hits(c.ptr, 16, 16, cams, 1, C.byref(bufs)),
                 rtlib.rt_render_anim_hits(c.ptr, 16, 16, cams, 0, 1, C.byref(bufs)),
                 rtlib.rt_pick(c.ptr, 16, 16, 0, 0, C.byref(pick))]
        assert calls == [abi.RT_ERR_UNSUPPORTED] * 7
        assert (out == 0).all()
