"""Scene-track shutter on the GPU (rt_render_anim_shutter_bands / rt_render_anim_shutter: every output frame the
in-kernel mean of m sub-frames, each with its own scene image and its own camera -- the ANIM_SHUTTER / ANIM_SHUTTER_SS
instantiations).  Every output frame is bit-exact against the shutter's rounding (path.shutter_mean, or
supersample.path_resolve at k > 1) of the unchanged oracle's per-sub-frame renders, each in that sub-frame's scene and
camera; the ray counts equal the sum of the oracle's over every sub-frame.  No tolerance anywhere.  The tracks
(tests/anim_shutter_cases.py) move spheres, lights, the floor and the ambient between sub-frames, and the tests assert on
the CPU side that a kernel reading sub-frame 0's image, grid z's image or the image with first_frame ignored would write
other frames."""
import ctypes as C
import dataclasses
import os

import numpy as np
import pytest

import anim_cases
import anim_shutter_cases as cases
from raytracer_hip import Context, RayTracerError, abi, path, scenes
from test_gpu_supersample import _band_rows_of

pytestmark = pytest.mark.gpu

RAYS = cases.RAYS
KEYS = RAYS + ("frames", "pixels", "launches")
W0, H0 = 100, 60


def assert_same(px, want, what):
    bad = px != want
    if bad.any():
        idx = np.argwhere(bad)[0]
        pytest.fail(f"{what}: {int(bad.sum())} of {bad.size} pixels differ; first at {tuple(int(i) for i in idx)}: "
                    f"gpu {int(px[tuple(idx)]):#08x} expected {int(want[tuple(idx)]):#08x}")


def ray_counts(st):
    return {r: st[r] for r in RAYS}


def _stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


def check(oracle, track, m, what, k=1, first_frame=0, n_frames=None, ctx=None, want=None):
    """One rt_render_anim_shutter of n_frames output frames from track frame first_frame on: pixels and stats."""
    W, H = track[0].width, track[0].height
    exp, rays = cases.expected(oracle, track, m, k, first_frame, n_frames)
    if want is not None:
        assert np.array_equal(want, exp)
    n = exp.shape[0]
    cams = cases.cameras(track[first_frame:first_frame + n * m])
    own = ctx is None
    ctx = ctx or Context(1)
    try:
        if own:
            ctx.set_scene_track(track)
            ctx.set_path_supersampling(k)
        ctx.reset_stats()
        px = ctx.render_anim_shutter(cams, W, H, m, first_frame=first_frame)
        st = ctx.stats()
    finally:
        if own:
            ctx.close()
    assert px.shape == (n, H, W)
    for f in range(n):
        assert_same(px[f], exp[f], f"{what} m={m} k={k} first_frame={first_frame} output frame {f}")
    assert ray_counts(st) == rays, f"{what}: the ray counts are the sum of the oracle's over every sub-frame"
    assert st["primary_rays"] == n * m * k * k * W * H
    assert st["frames"] == n and st["pixels"] == n * W * H and st["launches"] == 1
    return px


# ---- direct family ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def direct9():
    return cases.direct_track(9)


@pytest.mark.parametrize("m", [2, 4])
def test_direct_family_whole_frames(oracle, direct9, m):
    """C3's moving scene at 100 x 60 (the last tile row and column are partial), 2 output frames of m sub-frames, from
    track frame 0 and from track frame 1 (no multiple of m)."""
    track = direct9[:2 * m + 1]
    want = cases.assert_discriminates(oracle, track, m, first_frame=1, n_frames=2)
    with Context(1) as ctx:
        ctx.set_scene_track(track)
        check(oracle, track, m, "direct", first_frame=0, n_frames=2, ctx=ctx)
        check(oracle, track, m, "direct", first_frame=1, n_frames=2, ctx=ctx, want=want)


@pytest.mark.parametrize("m", [2, 4])
@pytest.mark.parametrize("band_rows,first,step", [(8, 1, 2), (5, 0, 1)])
def test_direct_family_bands_formats_stride_and_first_frame_1(oracle, direct9, m, band_rows, first, step):
    """The bands call in INT32, RGB24 and FRAME, first_frame = 1, a frame stride larger than a frame."""
    import torch
    F0, N = 1, 2
    track = direct9[:2 * m + 1]
    want, rays = cases.expected(oracle, track, m, 1, F0, N)
    cams = cases.cameras(track[F0:F0 + N * m])
    rows = _band_rows_of(first, step, band_rows, H0)
    nb_want = -(-len(rows) // band_rows)
    others = [y for y in range(H0) if y not in rows]
    with Context(1) as ctx:
        ctx.set_scene_track(track)
        stride = nb_want * band_rows * W0 * 4 + 64
        out = torch.full((N * stride // 4,), -1, dtype=torch.int32, device="cuda")
        ctx.reset_stats()
        nb = ctx.render_anim_shutter_bands(W0, H0, cams, m, band_rows, first, step, out.data_ptr(), stride, abi.RT_BANDS_INT32,
                                           _stream(), first_frame=F0)
        torch.cuda.synchronize()
        assert nb == nb_want
        host = out.cpu().numpy().reshape(N, stride // 4)
        for j in range(N):
            assert_same(host[j, :len(rows) * W0].reshape(len(rows), W0), want[j][rows], f"INT32 ({first},{step}) m={m} frame {j}")
            assert (host[j, len(rows) * W0:] == -1).all(), "rows past the image and the stride's gap stay untouched"
        st = ctx.stats()
        assert st["primary_rays"] == N * m * len(rows) * W0 and st["pixels"] == N * nb * band_rows * W0 and st["launches"] == 1
        if step == 1:
            assert ray_counts(st) == rays
        stride = nb_want * band_rows * W0 * 3 + 64
        raw = torch.full((N * stride,), 0xA5, dtype=torch.uint8, device="cuda")
        ctx.render_anim_shutter_bands(W0, H0, cams, m, band_rows, first, step, raw.data_ptr(), stride, abi.RT_BANDS_RGB24,
                                      _stream(), first_frame=F0)
        torch.cuda.synchronize()
        hr = raw.cpu().numpy().reshape(N, stride)
        for j in range(N):
            b = hr[j, :len(rows) * W0 * 3].reshape(len(rows), W0, 3).astype(np.int32)
            assert_same(b[..., 0] | (b[..., 1] << 8) | (b[..., 2] << 16), want[j][rows], f"RGB24 ({first},{step}) m={m} frame {j}")
            assert (hr[j, len(rows) * W0 * 3:] == 0xA5).all()
        stride = H0 * W0 * 4 + 64
        frame = torch.full((N * stride // 4,), -1, dtype=torch.int32, device="cuda")
        ctx.render_anim_shutter_bands(W0, H0, cams, m, band_rows, first, step, frame.data_ptr(), stride, abi.RT_BANDS_FRAME,
                                      _stream(), first_frame=F0)
        torch.cuda.synchronize()
        hf = frame.cpu().numpy().reshape(N, stride // 4)
        for j in range(N):
            img = hf[j, :H0 * W0].reshape(H0, W0)
            assert_same(img[rows], want[j][rows], f"FRAME ({first},{step}) m={m} frame {j}")
            assert (img[others] == -1).all(), "the rows of other ranks stay untouched"
            assert (hf[j, H0 * W0:] == -1).all()


# ---- bundle family ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def bundle5():
    return cases.bundle_track(5)


def test_bundle_family(oracle, bundle5):
    """C4's scene at 64 x 40, m = 2: the shadow grids, slabs, clusters and shadow culls differ per sub-frame."""
    want = cases.assert_discriminates(oracle, bundle5, 2, first_frame=1, n_frames=2)
    with Context(1) as ctx:
        ctx.set_scene_track(bundle5)
        check(oracle, bundle5, 2, "bundle", first_frame=0, n_frames=2, ctx=ctx)
        check(oracle, bundle5, 2, "bundle", first_frame=1, n_frames=2, ctx=ctx, want=want)


# ---- every descriptor ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("gpow", [False, True], ids=["pow", "gpow"])
@pytest.mark.parametrize("cls", list(anim_cases.CLASSES))
def test_every_class_pow_and_depth(oracle, cls, gpow):
    """4-sub-frame tracks at 32 x 24, m = 2, 2 output frames: one launch per (class, pow, limit)."""
    with Context(1) as ctx:
        for limit in anim_cases.LIMITS:
            track = cases.class_track(cls, gpow, limit)
            ctx.set_scene_track(track)
            px = check(oracle, track, 2, track[0].name, ctx=ctx)
            if anim_cases.CLASSES[cls][0] > 0:
                sub, _ = cases.subframes(oracle, track)
                assert (sub[0] != sub[1]).any() and (sub[2] != sub[3]).any() and (px[0] != px[1]).any(), track[0].name


def test_the_sweep_reaches_every_anim_shutter_descriptor():
    reached = {cases.descriptor(cls, gpow, limit) for cls in anim_cases.CLASSES for gpow in (False, True)
               for limit in anim_cases.LIMITS}
    assert len(reached) == 60
    assert {d[:3] for d in reached} == {(f, g, c) for f, cs in (("direct", (8, 0)), ("bundle", (0, 1, 2))) for c in cs
                                        for g in (False, True)}


# ---- supersampled ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [2, 4])
def test_supersampled_direct_track(oracle, k):
    track = cases.direct_track(5, 25, 15)
    want = cases.assert_discriminates(oracle, track, 2, k, first_frame=1, n_frames=2)
    check(oracle, track, 2, "direct", k, first_frame=1, n_frames=2, want=want)


@pytest.mark.parametrize("k", [2, 4])
def test_supersampled_bundle_track(oracle, k):
    track = cases.bundle_track(5, 16, 10)
    want = cases.assert_discriminates(oracle, track, 2, k, first_frame=1, n_frames=2)
    check(oracle, track, 2, "bundle", k, first_frame=1, n_frames=2, want=want)


SS_LIMITS = [0, 3, 8]  # K = 1, 4 and 64


@pytest.mark.parametrize("gpow", [False, True], ids=["pow", "gpow"])
@pytest.mark.parametrize("cls", list(anim_cases.CLASSES))
def test_every_class_supersampled_at_k_2(oracle, cls, gpow):
    with Context(1) as ctx:
        ctx.set_path_supersampling(2)
        for limit in SS_LIMITS:
            track = cases.class_track(cls, gpow, limit)
            ctx.set_scene_track(track)
            check(oracle, track, 2, track[0].name, 2, ctx=ctx)


def test_the_supersampled_sweep_reaches_stack_sizes_1_4_and_64():
    assert [anim_cases.stack_size(limit) for limit in SS_LIMITS] == [1, 4, 64]


def test_supersampled_at_the_bound_m_4_k_8(oracle):
    """m k^2 = 256 values per channel: the largest sums the 16-bit fields hold."""
    track = cases.direct_track(4, 16, 8)
    check(oracle, track, 4, "direct at the bound", 8)


# ---- sum width -------------------------------------------------------------------------------------------------------
def test_256_sub_frames_with_a_saturated_channel(oracle):
    """m = 256 on a 16 x 8 frame of a 256-frame track.  Some pixel holds a channel at 255 in all 256 sub-frames, so its
    sum is 256 * 255 = 65,280: the largest a 16-bit field must hold before the rounding term."""
    track = cases.bright_track(256, 16, 8)
    sub, _ = cases.subframes(oracle, track)
    sat = np.zeros(sub.shape[1:], dtype=bool)
    for shift in (16, 8, 0):
        sat |= (((sub >> shift) & 0xFF) == 255).all(axis=0)
    assert sat.any(), "no pixel keeps a channel at 255 through all 256 sub-frames"
    px = check(oracle, track, 256, "m = 256")
    y, x = np.argwhere(sat)[0]
    assert any(((int(px[0, y, x]) >> shift) & 0xFF) == 255 for shift in (16, 8, 0))


# ---- mixed tracks ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cls", ["s8", "s12"])
def test_mixed_tracks_are_exact(oracle, cls):
    """Sub-frames with and without a light at the origin, and with and without a general exponent, in one output
    frame (tests/test_gpu_anim.py test_mixed_tracks_are_exact's scenes)."""
    base = anim_cases.class_track(cls, False, 3)
    base = base + [dataclasses.replace(base[1], name=f"{base[1].name}_again")]  # 4 sub-frames: 2 output frames at m = 2
    origin = [dataclasses.replace(sc, name=f"{sc.name}_ashut_originmix", lights=[sc.lights[0], anim_cases.ORIGIN_LIGHT] if f == 1 else sc.lights)
              for f, sc in enumerate(base)]
    check(oracle, origin, 2, f"{cls} origin light in sub-frame 1")
    g = anim_cases.class_track(cls, True, 3)
    expo = [dataclasses.replace(g[2] if f == 2 else sc, name=f"{sc.name}_ashut_expmix") for f, sc in enumerate(base)]
    check(oracle, expo, 2, f"{cls} exponent 7.3 in sub-frame 2")
    check(oracle, expo, 4, f"{cls} exponent 7.3 in sub-frame 2, one output frame")


# ---- identities ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", [abi.RT_BANDS_INT32, abi.RT_BANDS_RGB24, abi.RT_BANDS_FRAME])
def test_shutter_1_is_render_anim_bands(direct9, fmt):
    import torch
    N, F0 = 4, 2
    cams = cases.cameras(direct9[F0:F0 + N])
    nbytes = H0 * W0 * 4 + 64
    with Context(1) as ctx:
        ctx.set_scene_track(direct9)
        a = torch.full((N * nbytes,), 0x5A, dtype=torch.uint8, device="cuda")
        b = torch.full((N * nbytes,), 0x5A, dtype=torch.uint8, device="cuda")
        ctx.reset_stats()
        ctx.render_anim_shutter_bands(W0, H0, cams, 1, 8, 0, 2, a.data_ptr(), nbytes, fmt, _stream(), first_frame=F0)
        torch.cuda.synchronize()
        sa = ctx.stats()
        ctx.reset_stats()
        ctx.render_anim_bands(W0, H0, cams, 8, 0, 2, b.data_ptr(), nbytes, fmt, _stream(), first_frame=F0)
        torch.cuda.synchronize()
        sb = ctx.stats()
        ha, hb = a.cpu().numpy(), b.cpu().numpy()
        assert (hb != 0x5A).any()
        assert np.array_equal(ha, hb), "byte-identical buffers"
        assert {k: sa[k] for k in KEYS} == {k: sb[k] for k in KEYS}
        ctx.reset_stats()
        pa = ctx.render_anim_shutter(cams, W0, H0, 1, first_frame=F0).copy()
        sa = ctx.stats()
        ctx.reset_stats()
        pb = ctx.render_anim(cams, W0, H0, first_frame=F0)
        sb = ctx.stats()
        assert np.array_equal(pa, pb) and {k: sa[k] for k in KEYS} == {k: sb[k] for k in KEYS}


@pytest.mark.parametrize("name,W,H", [("C3", 50, 30), ("C4", 32, 20)])
def test_a_track_of_one_scene_is_render_shutter(name, W, H):
    sc = scenes.config(name).resized(W, H)
    track = anim_cases.with_path_cameras([sc] * 4)
    cams = cases.cameras(track)
    with Context(1) as ctx:
        ctx.set_scene(sc)
        ctx.set_scene_track(track)
        ctx.reset_stats()
        want = ctx.render_shutter(cams, W, H, 2).copy()
        sw = ctx.stats()
        ctx.reset_stats()
        got = ctx.render_anim_shutter(cams, W, H, 2)
        sg = ctx.stats()
    assert (want[0] != want[1]).any()
    assert np.array_equal(got, want) and {k: sg[k] for k in KEYS} == {k: sw[k] for k in KEYS}


# ---- stats -----------------------------------------------------------------------------------------------------------
def test_counting_off_counts_nothing(oracle, direct9):
    track = direct9[:4]
    want, _ = cases.expected(oracle, track, 2)
    with Context(1) as ctx:
        ctx.set_scene_track(track)
        ctx.set_counting(False)
        ctx.reset_stats()
        px = ctx.render_anim_shutter(None, W0, H0, 2)
        st = ctx.stats()
    for f in range(2):
        assert_same(px[f], want[f], f"counting off, output frame {f}")
    assert ray_counts(st) == {r: 0 for r in RAYS} and st["frames"] == 2 and st["pixels"] == 2 * W0 * H0 and st["launches"] == 1


# ---- chunks ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("registered", [True, False])
@pytest.mark.parametrize("chunk", [1, 2])
def test_chunked_host_frames_under_a_view_height_above_the_frame(oracle, chunk, registered, monkeypatch):
    """3 output frames at m = 2 from track frame 1, rows [0, 22) of a view 30 rows high, in chunks of 1 and 2 output
    frames: chunk c takes its cameras and its track frames from output frame f0's sub-frames."""
    W, H, VH, m, F0 = 50, 22, 30, 2, 1
    track = cases.direct_track(7, W, VH)
    want, rays = cases.expected(oracle, track, m, 1, F0, 3, W, H, view_h=VH)
    cams = cases.cameras(track[F0:])
    monkeypatch.setenv("RT_PATH_CHUNK_FRAMES", str(chunk))  # read at rt_create
    with Context(1) as ctx:
        ctx.set_scene_track(track)
        ctx.set_view_height(VH)
        out = np.full((3, H, W), -1, dtype=np.int32)
        if registered:
            ctx.register_host(out)
        try:
            ctx.reset_stats()
            got = ctx.render_anim_shutter(cams, W, H, m, first_frame=F0, out=out)
            st = ctx.stats()
        finally:
            if registered:
                ctx.unregister_host(out)
    assert np.shares_memory(got, out)
    for f in range(3):
        assert_same(out[f], want[f], f"chunks of {chunk}, registered={registered}, output frame {f}")
    assert st["launches"] == -(-3 // chunk) and st["frames"] == 3 and st["pixels"] == 3 * W * H
    assert ray_counts(st) == rays and st["primary_rays"] == 3 * m * W * H


# ---- refusals --------------------------------------------------------------------------------------------------------
def test_refusals_on_a_live_context(oracle, direct9):
    """Every refusal of the header, in its order: the code, rt_last_error naming the argument, the sentinel-filled output
    untouched, the stats unchanged.  (n_frames * shutter above RT_MAX_PATH_FRAMES cannot be reached on a live context:
    the track bound comes first and a track has at most RT_MAX_PATH_FRAMES frames; tests/native/anim_shutter_host.cpp
    reaches the rule itself.)  Afterwards the context's own scene, rt_render_shutter and rt_render_anim give their old
    frames."""
    import torch
    sc = scenes.config("C3").resized(W0, H0)
    cams = path.as_array(cases.cameras(direct9))
    dev = torch.full((2, H0, W0), -1, dtype=torch.int32, device="cuda")
    host = np.full((2, H0, W0), -1, dtype=np.int32)
    nbytes = H0 * W0 * 4
    OK_BANDS = (H0, 0, 1)

    def both(ctx, want_code, text, W=W0, H=H0, cameras=cams, first=0, n=2, shutter=2, bands=OK_BANDS, d_out=None, stride=nbytes,
             fmt=abi.RT_BANDS_INT32, pixels=True, bands_only=False):
        lib, before = ctx.lib, ctx.stats()
        d_ptr = C.c_void_p(dev.data_ptr() if d_out is None else d_out)
        rc = lib.rt_render_anim_shutter_bands(ctx.ptr, W, H, cameras, first, n, shutter, bands[0], bands[1], bands[2], d_ptr, stride,
                                              fmt, C.c_void_p(_stream()), None)
        assert rc == want_code, (text, rc, lib.rt_last_error(ctx.ptr))
        assert text.encode() in lib.rt_last_error(ctx.ptr), (text, lib.rt_last_error(ctx.ptr))
        if not bands_only:
            rc = lib.rt_render_anim_shutter(ctx.ptr, W, H, cameras, first, n, shutter, host.ctypes.data if pixels else None)
            assert rc == want_code, (text, rc, lib.rt_last_error(ctx.ptr))
            assert text.encode() in lib.rt_last_error(ctx.ptr), (text, lib.rt_last_error(ctx.ptr))
        after = ctx.stats()
        assert {k: after[k] for k in KEYS} == {k: before[k] for k in KEYS}, text

    INV, UNS = abi.RT_ERR_INVALID_ARG, abi.RT_ERR_UNSUPPORTED
    with Context(1) as ctx:
        assert ctx.lib.rt_render_anim_shutter(None, W0, H0, cams, 0, 2, 2, host.ctypes.data) == INV
        assert ctx.lib.rt_render_anim_shutter_bands(None, W0, H0, cams, 0, 2, 2, H0, 0, 1, C.c_void_p(dev.data_ptr()), nbytes,
                                                    abi.RT_BANDS_INT32, None, None) == INV
        ctx.set_scene(sc)
        own = ctx.render(W0, H0).copy()
        shut = ctx.render_shutter(cases.cameras(direct9[:4]), W0, H0, 2).copy()
        both(ctx, abi.RT_ERR_NO_SCENE, "rt_set_scene_track")
        both(ctx, INV, "NULL cameras", cameras=None)  # (ahead of the missing track)
        ctx.set_scene_track(direct9)
        anim_px = ctx.render_anim(None, W0, H0).copy()
        # rt_render_anim*'s refusals
        both(ctx, INV, "NULL cameras", cameras=None)
        both(ctx, INV, "frame count", n=0)
        both(ctx, INV, "frame count", n=abi.RT_MAX_PATH_FRAMES + 1, shutter=1)
        both(ctx, INV, "frame size", W=0)
        both(ctx, INV, "frame size", H=-1)
        both(ctx, INV, "outside the track", first=-1)
        both(ctx, INV, "outside the track", first=6, n=2, shutter=2)   # 6 + 4 > 9
        both(ctx, INV, "outside the track", first=0, n=5, shutter=2)   # 10 > 9: each frame takes `shutter` track frames
        both(ctx, INV, "outside the track", first=2, n=1, shutter=8)
        both(ctx, INV, "outside the track", first=0, n=4, shutter=3)   # (the track bound comes before the shutter's)
        ctx.set_supersampling(2)
        both(ctx, UNS, "rt_set_supersampling")
        ctx.set_supersampling(1)
        ctx.set_path_supersampling(2)
        both(ctx, INV, "2^31", W=32768, H=32768)
        # the shutter's refusals
        for bad in (0, -2, 3, 6):
            both(ctx, INV, f"shutter {bad} is not a power of two", n=1, shutter=bad)
        ctx.set_path_supersampling(8)
        both(ctx, INV, "above 256 samples per pixel", n=1, shutter=8)   # 8 * 64 = 512
        ctx.set_path_supersampling(2)
        ctx.set_path_adaptive_sampling(16)
        both(ctx, UNS, "rt_set_path_adaptive_sampling", shutter=2)
        ctx.set_path_adaptive_sampling(0)
        ctx.set_path_supersampling(1)
        # then the band arguments, the stride and the output
        both(ctx, INV, "band", bands=(0, 0, 1), bands_only=True)
        both(ctx, INV, "band", bands=(8, 0, 0), bands_only=True)
        both(ctx, INV, "band", d_out=0, bands_only=True)
        both(ctx, INV, "band", fmt=99, bands_only=True)
        both(ctx, INV, "frame stride", stride=nbytes - 4, bands_only=True)
        rc = ctx.lib.rt_render_anim_shutter(ctx.ptr, W0, H0, cams, 0, 2, 2, None)
        assert rc == INV and b"NULL pixels" in ctx.lib.rt_last_error(ctx.ptr)
        ctx.set_view_height(H0 - 1)
        both(ctx, INV, "view height")
        ctx.set_view_height(0)
        torch.cuda.synchronize()
        assert (dev.cpu().numpy() == -1).all() and (host == -1).all(), "a refused call writes nothing"
        # the Python wrapper: a camera count that is no multiple of the shutter
        with pytest.raises(ValueError):
            ctx.render_anim_shutter(cases.cameras(direct9[:3]), W0, H0, 2)
        # everything else is what it was
        assert_same(ctx.render(W0, H0), own, "rt_render after the refusals")
        assert_same(ctx.render_shutter(cases.cameras(direct9[:4]), W0, H0, 2), shut, "rt_render_shutter after the refusals")
        assert_same(ctx.render_anim(None, W0, H0), anim_px, "rt_render_anim after the refusals")
        want, _ = cases.expected(oracle, direct9, 2, 1, 1, 2)
        assert_same(ctx.render_anim_shutter(cases.cameras(direct9[1:5]), W0, H0, 2, first_frame=1), want, "a valid call after the refusals")
        # a shutter above RT_MAX_SHUTTER needs a track that holds its sub-frames: the track bound comes first
        long = cases.direct_track(513, 16, 8)
        ctx.set_scene_track(long)
        both(ctx, INV, "shutter 512 is not a power of two", W=16, H=8, cameras=path.as_array(cases.cameras(long)), n=1, shutter=512)
        assert (host == -1).all()
    with Context(2, abi.RT_CREATE_SHARED_DEVICE) as ctx:
        ctx.set_scene_track(direct9)
        both(ctx, INV, "single-GPU")
        assert (host == -1).all()


# ---- switches --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("switch", ["RT_SHADOW_PRE", "RT_SHADOW_GRID", "RT_TRACE_CLUSTERS"])
def test_switches_change_no_pixel(oracle, direct9, bundle5, switch):
    os.environ[switch] = "0"
    try:
        check(oracle, direct9[:5], 2, f"direct {switch}=0", first_frame=1, n_frames=2)
        check(oracle, bundle5, 2, f"bundle {switch}=0", first_frame=1, n_frames=2)
    finally:
        del os.environ[switch]
