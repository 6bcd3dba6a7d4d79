"""Animated scenes on the GPU (rt_set_scene_track, rt_render_anim_bands / rt_render_anim: one batch launch, one scene
and one camera per frame).  Every frame is bit-exact against the unchanged oracle rendered with that frame's scene and
camera, and the ray counts equal the sum of the oracle's over the frames.  The tracks (tests/anim_cases.py) move
spheres, lights, the floor and the ambient between the frames, so a launch that read frame 0's scene everywhere, or
built its screen boxes against another frame's spheres, cannot pass.  Oracle frames are rendered once per module."""
import itertools
import os

import numpy as np
import pytest

import anim_cases
import path_cases
from raytracer_hip import Context, RayTracerError, abi, scenes
from test_gpu_supersample import _band_rows_of

pytestmark = pytest.mark.gpu

RAYS = anim_cases.RAYS


def assert_same(px, want, what):
    bad = px != want
    if bad.any():
        idx = np.argwhere(bad)[0]
        pytest.fail(f"{what}: {int(bad.sum())} of {bad.size} pixels differ; first at {tuple(int(i) for i in idx)}: "
                    f"gpu {int(px[tuple(idx)]):#08x} expected {int(want[tuple(idx)]):#08x}")


def ray_counts(st):
    return {k: st[k] for k in RAYS}


def _stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


def own_frames(ctx, track, W, H):
    """The library's own frames: set_scene(frame f) + its camera + render_bands_ex of the whole frame."""
    import torch
    out = []
    buf = torch.zeros(W * H, dtype=torch.int32, device="cuda")
    for sc in track:
        ctx.set_scene(sc)
        ctx.render_bands_ex(W, H, H, 0, 1, buf.data_ptr(), abi.RT_BANDS_FRAME, _stream())
        torch.cuda.synchronize()
        out.append(buf.cpu().numpy().reshape(H, W).copy())
    return np.stack(out)


def check_track(oracle, track, what, own=False):
    W, H = track[0].width, track[0].height
    want, ost = anim_cases.oracle_frames(oracle, track)
    with Context(1) as ctx:
        ctx.set_scene_track(track)
        ctx.reset_stats()
        px = ctx.render_anim(None, W, H)
        st = ctx.stats()
        assert px.shape == (len(track), H, W)
        for f in range(len(track)):
            assert_same(px[f], want[f], f"{what} frame {f}")
        assert ray_counts(st) == anim_cases.summed(ost), f"{what}: the ray counts are the sum of the oracle's over the frames"
        assert st["primary_rays"] == len(track) * W * H and st["frames"] == len(track) and st["pixels"] == len(track) * W * H
        assert st["launches"] == 1
        if own:
            mine = own_frames(ctx, track, W, H)
            for f in range(len(track)):
                assert_same(px[f], mine[f], f"{what} frame {f} against set_scene + render_bands_ex")
    return px


@pytest.fixture(scope="module")
def direct():
    return anim_cases.direct_track()


@pytest.fixture(scope="module")
def bundle():
    return anim_cases.bundle_track()


def test_direct_family_moving_spheres_light_floor_and_ambient(oracle, direct):
    """C3's scene at 100 x 60 (ragged tiles on both edges), 6 frames, the last repeating the first."""
    px = check_track(oracle, direct, "direct", own=True)
    for a, b in itertools.combinations(range(5), 2):
        assert (px[a] != px[b]).mean() > 0.25, f"frames {a} and {b} are (nearly) the same frame"
    assert (px[0] == px[5]).all()


def test_bundle_family_moving_spheres_and_lights(oracle, bundle):
    """C4's scene at 64 x 40, 4 frames: the shadow grids, slabs, clusters and shadow culls differ per frame."""
    px = check_track(oracle, bundle, "bundle", own=True)
    for a, b in itertools.combinations(range(4), 2):
        assert (px[a] != px[b]).any()


@pytest.mark.parametrize("gpow", [False, True], ids=["pow", "gpow"])
@pytest.mark.parametrize("cls", list(anim_cases.CLASSES))
def test_every_class_pow_and_depth(oracle, cls, gpow):
    """3-frame tracks at 32 x 24: one launch per (class, pow, limit), against the oracle."""
    W, H = anim_cases.CLASS_W, anim_cases.CLASS_H
    with Context(1) as ctx:
        for limit in anim_cases.LIMITS:
            track = anim_cases.class_track(cls, gpow, limit)
            want, ost = anim_cases.oracle_frames(oracle, track)
            ctx.set_scene_track(track)
            ctx.reset_stats()
            px = ctx.render_anim(None, W, H)
            for f in range(len(track)):
                assert_same(px[f], want[f], f"{track[f].name}")
            st = ctx.stats()
            assert ray_counts(st) == anim_cases.summed(ost) and st["launches"] == 1, track[0].name
            if anim_cases.CLASSES[cls][0] > 0:
                assert (px[0] != px[1]).any() and (px[1] != px[2]).any(), track[0].name


def test_the_sweep_reaches_every_anim_descriptor():
    reached = {anim_cases.descriptor(cls, gpow, limit) for cls in anim_cases.CLASSES for gpow in (False, True)
               for limit in anim_cases.LIMITS}
    assert len(reached) == 60
    assert {d[:3] for d in reached} == {(f, g, c) for f, cs in (("direct", (8, 0)), ("bundle", (0, 1, 2))) for c in cs
                                        for g in (False, True)}


@pytest.mark.parametrize("cls", ["s8", "s12"])
def test_mixed_tracks_are_exact(oracle, cls):
    """One frame with a light at the origin (the track runs the kernels that test each light's 2a), and one frame with
    exponent 7.3 among exponent-2 frames (the track runs the Math.Pow kernels, which dispatch per material)."""
    import dataclasses
    base = anim_cases.class_track(cls, False, 3)
    origin = [dataclasses.replace(sc, name=f"{sc.name}_originmix", lights=[sc.lights[0], anim_cases.ORIGIN_LIGHT] if f == 1 else sc.lights)
              for f, sc in enumerate(base)]
    check_track(oracle, origin, f"{cls} origin light in frame 1")
    g = anim_cases.class_track(cls, True, 3)
    expo = [dataclasses.replace(g[f] if f == 2 else sc, name=f"{sc.name}_expmix") for f, sc in enumerate(base)]
    check_track(oracle, expo, f"{cls} exponent 7.3 in frame 2")


W0, H0 = 100, 60


@pytest.fixture(scope="module")
def direct_ctx(direct):
    ctx = Context(1)
    ctx.set_scene_track(direct)
    yield ctx
    ctx.close()


@pytest.mark.parametrize("band_rows,first,step", [(8, 1, 2), (5, 0, 1), (5, 2, 3)])
def test_bands_formats_strides_and_first_frame(oracle, direct, direct_ctx, band_rows, first, step):
    """first_frame = 2, n_frames = 3 of the 6-frame track, every format, a frame stride larger than a frame."""
    import torch
    ctx, F0, N = direct_ctx, 2, 3
    want, ost = anim_cases.oracle_frames(oracle, direct)
    cams = [sc.c_camera() for sc in direct[F0:F0 + N]]
    rows = _band_rows_of(first, step, band_rows, H0)
    nb_want = -(-len(rows) // band_rows)
    others = [y for y in range(H0) if y not in rows]
    stride = nb_want * band_rows * W0 * 4 + 64
    out = torch.full((N * stride // 4,), -1, dtype=torch.int32, device="cuda")
    ctx.reset_stats()
    nb = ctx.render_anim_bands(W0, H0, cams, band_rows, first, step, out.data_ptr(), stride, abi.RT_BANDS_INT32, _stream(),
                               first_frame=F0)
    torch.cuda.synchronize()
    assert nb == nb_want
    host = out.cpu().numpy().reshape(N, stride // 4)
    for j in range(N):
        assert_same(host[j, :len(rows) * W0].reshape(len(rows), W0), want[F0 + j][rows], f"INT32 ({first},{step}) frame {F0 + j}")
        assert (host[j, len(rows) * W0:] == -1).all(), "rows past the image and the stride's gap stay untouched"
    st = ctx.stats()
    assert st["primary_rays"] == N * len(rows) * W0 and st["pixels"] == N * nb * band_rows * W0 and st["launches"] == 1
    if step == 1:
        assert ray_counts(st) == anim_cases.summed(ost[F0:F0 + N])
    stride = nb_want * band_rows * W0 * 3 + 64
    raw = torch.full((N * stride,), 0xA5, dtype=torch.uint8, device="cuda")
    ctx.render_anim_bands(W0, H0, cams, band_rows, first, step, raw.data_ptr(), stride, abi.RT_BANDS_RGB24, _stream(), first_frame=F0)
    torch.cuda.synchronize()
    hr = raw.cpu().numpy().reshape(N, stride)
    for j in range(N):
        b = hr[j, :len(rows) * W0 * 3].reshape(len(rows), W0, 3).astype(np.int32)
        assert_same(b[..., 0] | (b[..., 1] << 8) | (b[..., 2] << 16), want[F0 + j][rows], f"RGB24 ({first},{step}) frame {F0 + j}")
        assert (hr[j, len(rows) * W0 * 3:] == 0xA5).all()
    stride = H0 * W0 * 4 + 64
    frame = torch.full((N * stride // 4,), -1, dtype=torch.int32, device="cuda")
    ctx.render_anim_bands(W0, H0, cams, band_rows, first, step, frame.data_ptr(), stride, abi.RT_BANDS_FRAME, _stream(), first_frame=F0)
    torch.cuda.synchronize()
    hf = frame.cpu().numpy().reshape(N, stride // 4)
    for j in range(N):
        img = hf[j, :H0 * W0].reshape(H0, W0)
        assert_same(img[rows], want[F0 + j][rows], f"FRAME ({first},{step}) frame {F0 + j}")
        assert (img[others] == -1).all(), "the rows of other ranks stay untouched"
        assert (hf[j, H0 * W0:] == -1).all()


def test_chunked_host_frames_and_a_view_height_above_the_frame(oracle, direct, monkeypatch):
    """rt_render_anim in chunks of 2 frames (three chunks), and rows [0, 44) of a view 60 rows high."""
    want, ost = anim_cases.oracle_frames(oracle, direct)
    cut, _ = anim_cases.oracle_frames(oracle, direct, W0, 44, view_h=H0)
    monkeypatch.setenv("RT_PATH_CHUNK_FRAMES", "2")  # read at rt_create
    with Context(1) as ctx:
        ctx.set_scene_track(direct)
        ctx.reset_stats()
        px = ctx.render_anim(None, W0, H0)
        st = ctx.stats()
        for f in range(6):
            assert_same(px[f], want[f], f"chunked frame {f}")
        assert st["launches"] == 3 and st["frames"] == 6 and ray_counts(st) == anim_cases.summed(ost)
        px = ctx.render_anim([sc.c_camera() for sc in direct[1:6]], W0, H0, first_frame=1)
        for j in range(5):
            assert_same(px[j], want[1 + j], f"chunked frame {1 + j} from first_frame 1")
        ctx.set_view_height(H0)
        px = ctx.render_anim(None, W0, 44)
        for f in range(6):
            assert_same(px[f], cut[f], f"view height {H0}, frame {f}")
        with pytest.raises(RayTracerError) as e:
            ctx.set_view_height(40)
            ctx.render_anim(None, W0, 44)
        assert e.value.code == abi.RT_ERR_INVALID_ARG


def test_the_track_is_apart_from_the_contexts_scene(oracle, direct, bundle):
    """render, render_path and a progressive run of the context's own scene are what they were without a track; a
    replaced track gives the new frames; a cleared one refuses."""
    sc = scenes.config("C3").resized(50, 30)
    cams = path_cases.cameras(sc)
    with Context(1) as ctx:
        ctx.set_scene(sc)
        before = ctx.render(50, 30).copy()
        before_path = ctx.render_path(cams, 50, 30).copy()
        ctx.set_progressive(2)
        before_prog = [ctx.render(50, 30).copy() for _ in range(4)]
        run = ctx.progressive()
        ctx.set_progressive(1)
        ctx.set_scene_track(direct)
        want, _ = anim_cases.oracle_frames(oracle, direct)
        px = ctx.render_anim(None, W0, H0)
        assert_same(px[3], want[3], "direct track frame 3")
        assert_same(ctx.render(50, 30), before, "render with a track set")
        assert_same(ctx.render_path(cams, 50, 30), before_path, "render_path with a track set")
        ctx.set_progressive(2)
        for i in range(4):
            assert_same(ctx.render(50, 30), before_prog[i], f"progressive Tick {i} with a track set")
            if i == 1:  # an anim render between two Ticks leaves the run alone
                ctx.render_anim(None, W0, H0)
        assert ctx.progressive() == run and run[0] == 2 and run[1] > 1
        ctx.set_progressive(1)
        assert_same(ctx.render_anim(None, W0, H0)[4], want[4], "direct track frame 4 after the context's renders")
        # a replaced track (other counts, another family)
        ctx.set_scene_track(bundle)
        wb, _ = anim_cases.oracle_frames(oracle, bundle)
        px = ctx.render_anim(None, bundle[0].width, bundle[0].height)
        for f in range(len(bundle)):
            assert_same(px[f], wb[f], f"replaced track frame {f}")
        assert_same(ctx.render(50, 30), before, "render after the track was replaced")
        ctx.clear_scene_track()
        with pytest.raises(RayTracerError) as e:
            ctx.render_anim([sc.c_camera()], 50, 30)
        assert e.value.code == abi.RT_ERR_NO_SCENE and "rt_set_scene_track" in str(e.value)
        assert_same(ctx.render(50, 30), before, "render after the track was cleared")


@pytest.mark.parametrize("switch", ["RT_SHADOW_PRE", "RT_SHADOW_GRID", "RT_TRACE_CLUSTERS"])
def test_switches_change_no_pixel(oracle, direct, bundle, switch):
    os.environ[switch] = "0"
    try:
        check_track(oracle, direct, f"direct {switch}=0")
        check_track(oracle, bundle, f"bundle {switch}=0")
    finally:
        del os.environ[switch]


def test_counting_off_counts_nothing(oracle, direct):
    want, _ = anim_cases.oracle_frames(oracle, direct)
    with Context(1) as ctx:
        ctx.set_scene_track(direct)
        ctx.set_counting(False)
        ctx.reset_stats()
        px = ctx.render_anim(None, W0, H0)
        st = ctx.stats()
        for f in range(6):
            assert_same(px[f], want[f], f"counting off, frame {f}")
        assert ray_counts(st) == {r: 0 for r in RAYS} and st["frames"] == 6 and st["launches"] == 1


def test_refusals_on_a_live_context(direct):
    with Context(1) as ctx:
        ctx.set_scene_track(direct)
        ctx.set_supersampling(2)
        with pytest.raises(RayTracerError) as e:
            ctx.render_anim(None, W0, H0)
        assert e.value.code == abi.RT_ERR_UNSUPPORTED
        ctx.set_supersampling(1)
        with pytest.raises(RayTracerError) as e:
            ctx.render_anim([direct[0].c_camera()] * 2, W0, H0, first_frame=5)
        assert e.value.code == abi.RT_ERR_INVALID_ARG
        import dataclasses
        with pytest.raises(ValueError):
            ctx.set_scene_track(direct[:2] + [dataclasses.replace(direct[2], spheres=direct[2].spheres[:-1])])
    with Context(2, abi.RT_CREATE_SHARED_DEVICE) as ctx:
        ctx.set_scene_track(direct)
        with pytest.raises(RayTracerError) as e:
            ctx.render_anim(None, W0, H0)
        assert e.value.code == abi.RT_ERR_INVALID_ARG
