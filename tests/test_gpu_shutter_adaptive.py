"""rt_set_shutter_adaptive_sampling on the GPU: the camera and scene-track shutters supersampled per 8x8 output tile inside
the trace kernels (the SHUTTER_ADAPT / ANIM_SHUTTER_ADAPT instantiations), the decision taken on the mean of the sub-frames.
Every output frame is bit-exact against supersample.shutter_adaptive_resolve of the unchanged oracle's per-sub-frame plain
and k W x k H renders, and the ray counts equal the oracle's over the samples the definition traces.  No tolerance
anywhere.  tests/test_shutter_adaptive.py holds the preconditions of every case used here: refined and flat tiles in every
output frame, a mask that is no sub-frame's own (nor, in some frame, their OR), expectations that are neither the factor-1
shutter frame nor the fully supersampled one."""
import os

import numpy as np
import pytest

import anim_shutter_cases as ashut
import shutter_adaptive_cases as sa
from raytracer_hip import Context, abi, path
from raytracer_hip.supersample import path_resolve, refine_mask, shutter_adaptive_resolve
from test_gpu_supersample import _band_rows_of

pytestmark = pytest.mark.gpu

pc = sa.pc
RAYS = sa.RAYS
KEYS = RAYS + ("frames", "pixels", "launches")
W0, H0, M0, K0, T0 = sa.W0, sa.H0, sa.M0, sa.K0, sa.T0


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


def _code(fn):
    with pytest.raises(abi.RayTracerError) as ei:
        fn()
    return ei.value.code


# ---- camera shutters -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", sa.CAMERA_CASES, ids=lambda c: f"{c[0]}-m{c[3]}-k{c[4]}-T{c[5]}")
def test_camera_shutter_every_scene(oracle, case):
    """Both families, every class among them, the Math.Pow entry points and the scratch stack (REF); 50 x 30 has a 2-wide
    last tile column and a 6-high last tile row; m k^2 up to 128 values per pixel."""
    cid, W, H, m, k, T, n = case
    sc = pc.scene(cid, W, H)
    cams, plain, big, stats, order = sa.camera_subframes(oracle, sc, k, n * m)
    want = shutter_adaptive_resolve(plain, big, k, m, T)
    counts = sa.traced_counts(oracle, sa.camera_scenes(sc, order), plain, big, stats, m, k, T)
    with Context(1) as ctx:
        ctx.set_scene(sc)
        assert ctx.get_shutter_adaptive_sampling() == 0, "a context that never called the setter reads 0"
        ctx.set_path_supersampling(k)
        ctx.set_shutter_adaptive_sampling(T)
        assert ctx.get_shutter_adaptive_sampling() == T and ctx.get_path_adaptive_sampling() == 0 and ctx.adaptive_sampling == 0
        ctx.reset_stats()
        px = ctx.render_shutter(cams, W, H, m)
        st = ctx.stats()
    assert px.shape == (n, H, W)
    for f in range(n):
        assert_same(px[f], want[f], f"{cid} {W}x{H} m={m} k={k} T={T} frame {f}")
    assert counts["primary_rays"] == sa.expected_primary(plain, m, k, T)
    assert ray_counts(st) == counts, "the ray counts are the oracle's over the traced samples of every sub-frame"
    assert st["frames"] == n and st["pixels"] == n * W * H and st["launches"] == 1


def test_equal_cameras_give_equal_frames(oracle):
    sc = pc.scene("C3", W0, H0)
    cams, plain, big, _, order = sa.camera_subframes(oracle, sc, K0, 6 * M0)
    assert order[:6] == order[6:]
    with Context(1) as ctx:
        ctx.set_scene(sc)
        ctx.set_path_supersampling(K0)
        ctx.set_shutter_adaptive_sampling(T0)
        px = ctx.render_shutter(cams, W0, H0, M0)
    want = shutter_adaptive_resolve(plain, big, K0, M0, T0)
    for f in range(6):
        assert_same(px[f], want[f], f"frame {f}")
    assert (px[:3] == px[3:]).all() and (px[0] != px[1]).any()


# ---- scene-track shutters ------------------------------------------------------------------------------------------
def check_track(oracle, name, counts=True):
    m, k, T, first = sa.track_case(name)
    tr = sa.track(name)
    W, H = tr[0].width, tr[0].height
    plain, big, stats, scs = sa.track_subframes(oracle, tr, k, first, m)
    n = len(plain) // m
    want = shutter_adaptive_resolve(plain, big, k, m, T)
    with Context(1) as ctx:
        ctx.set_scene_track(tr)
        ctx.set_path_supersampling(k)
        ctx.set_shutter_adaptive_sampling(T)
        ctx.reset_stats()
        px = ctx.render_anim_shutter(ashut.cameras(tr)[first:first + n * m], W, H, m, first_frame=first)
        st = ctx.stats()
    assert px.shape == (n, H, W)
    for f in range(n):
        assert_same(px[f], want[f], f"track {name} m={m} k={k} T={T} output frame {f}")
    assert st["primary_rays"] == sa.expected_primary(plain, m, k, T)
    if counts:
        assert ray_counts(st) == sa.traced_counts(oracle, scs, plain, big, stats, m, k, T)
    assert st["frames"] == n and st["pixels"] == n * W * H and st["launches"] == 1
    return px, want


@pytest.mark.parametrize("name", ["direct_m2", "direct_m4", "bundle_m2"])
def test_track_shutter(oracle, name):
    check_track(oracle, name)


def test_track_from_first_frame_1_reads_its_own_scenes(oracle):
    m, k, T, first = sa.track_case("direct_first1")
    _, want = check_track(oracle, "direct_first1")
    for what, alt in ashut.wrong_scene_alternatives(oracle, sa.track("direct_first1"), m, k, first).items():
        assert (alt != want).any(), f"a kernel tracing in {what} would pass"


def test_track_that_mixes_gpow_and_other_frames(oracle):
    check_track(oracle, "mixed")


def test_saturation_gives_255_not_a_wrapped_sum(oracle):
    """m = 16, k = 4: 256 values of 255 in a channel."""
    px, want = check_track(oracle, "saturation", counts=False)
    sat = (want[0] >> 16) == 255
    assert int(sat.sum()) >= 30 and ((px[0] >> 16)[sat] == 255).all()


# ---- the frame of the threshold, setting, band, view and chunk tests -----------------------------------------------
@pytest.fixture(scope="module")
def c3():
    return pc.scene("C3", W0, H0)


@pytest.fixture(scope="module")
def _c3_ctx(c3):
    ctx = Context(1)
    ctx.set_scene(c3)
    ctx.set_scene_track(sa.track("direct_m2"))
    yield ctx
    ctx.close()


@pytest.fixture
def c3_ctx(_c3_ctx):
    """The module's context at k = 2 and shutter threshold T0, with every setting a test may change put back after it."""
    _c3_ctx.set_path_supersampling(K0)
    _c3_ctx.set_shutter_adaptive_sampling(T0)
    yield _c3_ctx
    _c3_ctx.set_path_supersampling(1)
    _c3_ctx.set_shutter_adaptive_sampling(0)
    _c3_ctx.set_path_adaptive_sampling(0)
    _c3_ctx.set_counting(True)
    _c3_ctx.set_view_height(0)


@pytest.fixture(scope="module")
def c3_sub(oracle, c3):
    """(cameras, plain, samples, stats, order) of 3 output frames of the C3 case."""
    return sa.camera_subframes(oracle, c3, K0, 3 * M0)


def test_256_is_the_factor_1_shutter_render(oracle, c3_ctx, c3_sub):
    cams, plain, big, stats, _ = c3_sub
    c3_ctx.set_path_supersampling(1)
    c3_ctx.reset_stats()
    base = c3_ctx.render_shutter(cams, W0, H0, M0).copy()
    st_base = c3_ctx.stats()
    for k in (2, 4):
        c3_ctx.set_path_supersampling(k)
        c3_ctx.set_shutter_adaptive_sampling(256)
        c3_ctx.reset_stats()
        px = c3_ctx.render_shutter(cams, W0, H0, M0)
        assert np.array_equal(px, base), f"T = 256 at k = {k}: bit for bit the k = 1 shutter render"
        assert ray_counts(c3_ctx.stats()) == ray_counts(st_base)
    assert np.array_equal(base, path.shutter_mean(plain, M0))


def test_1_refines_every_tile_that_is_not_one_colour(oracle, c3_ctx, c3_sub):
    cams, plain, big, _, _ = c3_sub
    c3_ctx.set_shutter_adaptive_sampling(1)
    c3_ctx.reset_stats()
    px = c3_ctx.render_shutter(cams, W0, H0, M0)
    want = shutter_adaptive_resolve(plain, big, K0, M0, 1)
    for f in range(3):
        assert_same(px[f], want[f], f"T = 1 frame {f}")
    assert c3_ctx.stats()["primary_rays"] == sa.expected_primary(plain, M0, K0, 1)
    assert any(not refine_mask(p, 1).all() for p in path.shutter_mean(plain, M0)) or (want == path_resolve(big, K0, M0)).all()


def test_setting_interplay(oracle, c3_ctx, c3_sub):
    cams, plain, big, stats, order = c3_sub
    full = path_resolve(big, K0, M0)
    # shutter T = 0, path T = 0: SHUTTER_SS -- the bytes, launches and counts of the library without the setting
    c3_ctx.set_shutter_adaptive_sampling(0)
    c3_ctx.reset_stats()
    px = c3_ctx.render_shutter(cams, W0, H0, M0).copy()
    st = c3_ctx.stats()
    for f in range(3):
        assert_same(px[f], full[f], f"both thresholds 0, frame {f}")
    assert ray_counts(st) == {r: sum(s[r] for s in stats) for r in RAYS} and st["launches"] == 1 and st["frames"] == 3
    # shutter T = 0, path T > 0: the refusal, nothing counted
    c3_ctx.set_path_adaptive_sampling(T0)
    before = c3_ctx.stats()
    assert _code(lambda: c3_ctx.render_shutter(cams, W0, H0, M0)) == abi.RT_ERR_UNSUPPORTED
    assert _code(lambda: c3_ctx.render_anim_shutter(None, W0, H0, M0)) == abi.RT_ERR_UNSUPPORTED
    assert {k: c3_ctx.stats()[k] for k in KEYS} == {k: before[k] for k in KEYS}
    # both set: a render at the shutter threshold (the path threshold differs and is not consulted)
    c3_ctx.set_path_adaptive_sampling(16)
    c3_ctx.set_shutter_adaptive_sampling(T0)
    want = shutter_adaptive_resolve(plain, big, K0, M0, T0)
    px = c3_ctx.render_shutter(cams, W0, H0, M0)
    for f in range(3):
        assert_same(px[f], want[f], f"both thresholds set, frame {f}")
    assert (want != shutter_adaptive_resolve(plain, big, K0, M0, 16)).any()
    # shutter == 1 with both set: render_path / render_anim at the path threshold
    p6, b6, _ = pc.path_frames(oracle, pc.scene("C3", W0, H0), K0)
    want1 = pc.path_adaptive_resolve(p6[order], b6[order], K0, 16)
    px1 = c3_ctx.render_shutter(cams, W0, H0, 1)
    assert np.array_equal(px1, c3_ctx.render_path(cams, W0, H0))
    for f in range(6):
        assert_same(px1[f], want1[f], f"shutter 1, frame {f}")
    assert (want1 != pc.path_adaptive_resolve(p6[order], b6[order], K0, T0)).any()
    tr = sa.track("direct_m2")
    tp, tb, _ = pc.track_frames(oracle, tr, K0)
    a1 = c3_ctx.render_anim_shutter(None, W0, H0, 1)
    assert np.array_equal(a1, c3_ctx.render_anim(None, W0, H0))
    assert np.array_equal(a1, pc.path_adaptive_resolve(tp, tb, K0, 16))


def test_setter_and_getter_bounds(c3_ctx):
    assert c3_ctx.get_shutter_adaptive_sampling() == T0
    for bad in (-1, 257):
        assert _code(lambda: c3_ctx.set_shutter_adaptive_sampling(bad)) == abi.RT_ERR_INVALID_ARG
    assert c3_ctx.get_shutter_adaptive_sampling() == T0
    assert c3_ctx.lib.rt_set_shutter_adaptive_sampling(None, 8) == abi.RT_ERR_INVALID_ARG
    assert c3_ctx.lib.rt_get_shutter_adaptive_sampling(c3_ctx.ptr, None) == abi.RT_ERR_INVALID_ARG
    # shutter x k^2 keeps its bound
    c3_ctx.set_path_supersampling(8)
    cams = pc.cycled(pc.scene("C3", W0, H0), 8)[0]
    assert _code(lambda: c3_ctx.render_shutter(cams, W0, H0, 8)) == abi.RT_ERR_INVALID_ARG


@pytest.mark.parametrize("anim", [False, True], ids=["camera", "track"])
def test_bands_of_8_rows_interleaved_in_two_formats_on_the_caller_s_stream(oracle, c3_ctx, c3_sub, anim):
    import torch
    band_rows, first, step, F = 8, 1, 2, 3
    if anim:
        tr = sa.track("direct_m2")
        plain, big, _, _ = sa.track_subframes(oracle, tr, K0, 0, M0)
        cams = ashut.cameras(tr)
    else:
        cams, plain, big, _, _ = c3_sub
    want = shutter_adaptive_resolve(plain, big, K0, M0, T0)
    mean = path.shutter_mean(plain, M0)
    rows = _band_rows_of(first, step, band_rows, H0)
    others = [y for y in range(H0) if y not in rows]
    nb_want = -(-len(rows) // band_rows)

    def call(ptr, stride, fmt, stream):
        if anim:
            return c3_ctx.render_anim_shutter_bands(W0, H0, cams, M0, band_rows, first, step, ptr, stride, fmt, stream)
        return c3_ctx.render_shutter_bands(W0, H0, cams, M0, band_rows, first, step, ptr, stride, fmt, stream)

    side = torch.cuda.Stream()
    stride = H0 * W0 * 4 + 64
    frame = torch.full((F * stride // 4,), -1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    c3_ctx.reset_stats()
    with torch.cuda.stream(side):
        nb = call(frame.data_ptr(), stride, abi.RT_BANDS_FRAME, side.cuda_stream)
    side.synchronize()
    assert nb == nb_want
    hf = frame.cpu().numpy().reshape(F, stride // 4)
    for f in range(F):
        img = hf[f, :H0 * W0].reshape(H0, W0)
        assert_same(img[rows], want[f][rows], f"FRAME frame {f}")
        assert (img[others] == -1).all() and (hf[f, H0 * W0:] == -1).all(), "other ranks' rows and the padding stay untouched"
    st = c3_ctx.stats()
    assert st["launches"] == 1 and st["pixels"] == F * nb * band_rows * W0
    # (8-row bands are tile rows: a band's tiles decide as the whole frame's do)
    assert st["primary_rays"] == sum(M0 * (len(rows) * W0 + (K0 * K0 - 1) * int(pc.pixel_mask(p, T0)[rows].sum())) for p in mean)
    stride = nb_want * band_rows * W0 * 3 + 64
    raw = torch.full((F * stride,), 0xA5, dtype=torch.uint8, device="cuda")
    call(raw.data_ptr(), stride, abi.RT_BANDS_RGB24, _stream())
    torch.cuda.synchronize()
    hr = raw.cpu().numpy().reshape(F, stride)
    for f in range(F):
        b = hr[f, :len(rows) * W0 * 3].reshape(len(rows), W0, 3).astype(np.int32)
        assert_same(b[..., 0] | (b[..., 1] << 8) | (b[..., 2] << 16), want[f][rows], f"RGB24 frame {f}")
        assert (hr[f, len(rows) * W0 * 3:] == 0xA5).all()


def test_bands_of_12_rows_are_unsupported_write_nothing_and_count_nothing(c3_ctx, c3_sub):
    import torch
    cams = c3_sub[0]
    nbytes = H0 * W0 * 4
    out = torch.full((3, H0, W0), -1, dtype=torch.int32, device="cuda")
    before = c3_ctx.stats()
    assert _code(lambda: c3_ctx.render_shutter_bands(W0, H0, cams, M0, 12, 0, 1, out.data_ptr(), nbytes, abi.RT_BANDS_INT32, _stream())) == abi.RT_ERR_UNSUPPORTED
    assert _code(lambda: c3_ctx.render_anim_shutter_bands(W0, H0, ashut.cameras(sa.track("direct_m2")), M0, 12, 0, 1, out.data_ptr(), nbytes,
                                                          abi.RT_BANDS_FRAME, _stream())) == abi.RT_ERR_UNSUPPORTED
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == -1).all(), "a refused call writes nothing"
    assert {k: c3_ctx.stats()[k] for k in KEYS} == {k: before[k] for k in KEYS}
    # not in effect (T = 0): 12-row bands are fine -- 3 bands of 12 packed rows per frame
    packed = torch.full((3, 36, W0), -1, dtype=torch.int32, device="cuda")
    c3_ctx.set_shutter_adaptive_sampling(0)
    assert c3_ctx.render_shutter_bands(W0, H0, cams, M0, 12, 0, 1, packed.data_ptr(), 36 * W0 * 4, abi.RT_BANDS_INT32, _stream()) == 3
    c3_ctx.set_shutter_adaptive_sampling(T0)
    # band_rows >= height: the frame as one band
    assert c3_ctx.render_shutter_bands(W0, H0, cams, M0, H0 + 7, 0, 1, out.data_ptr(), nbytes, abi.RT_BANDS_FRAME, _stream()) == 1
    torch.cuda.synchronize()


def test_view_height_cuts_the_last_tile_row_and_its_decision(oracle, c3, c3_ctx):
    rows = sa.VIEW_ROWS
    cams, plain, big, _, _ = sa.camera_subframes(oracle, c3, K0, 3 * M0, rows, H0)
    want = shutter_adaptive_resolve(plain, big, K0, M0, T0)
    c3_ctx.set_view_height(H0)
    c3_ctx.reset_stats()
    px = c3_ctx.render_shutter(cams, W0, rows, M0)
    assert px.shape == (3, rows, W0)
    for f in range(3):
        assert_same(px[f], want[f], f"{W0}x{rows} of a {W0}x{H0} view, frame {f}")
    assert c3_ctx.stats()["primary_rays"] == sa.expected_primary(plain, M0, K0, T0)


def test_counting_off_counts_nothing(c3_ctx, c3_sub):
    c3_ctx.set_counting(False)
    c3_ctx.reset_stats()
    c3_ctx.render_shutter(c3_sub[0], W0, H0, M0)
    st = c3_ctx.stats()
    assert ray_counts(st) == dict.fromkeys(RAYS, 0) and st["frames"] == 3


def test_chunks_of_one_output_frame_equal_the_one_launch_result(oracle, c3, c3_sub, monkeypatch):
    cams, plain, big, _, _ = c3_sub
    want = shutter_adaptive_resolve(plain, big, K0, M0, T0)
    tr = sa.track("direct_first1")
    m, k, T, first = sa.track_case("direct_first1")
    tplain, tbig, _, _ = sa.track_subframes(oracle, tr, k, first, m)
    twant = shutter_adaptive_resolve(tplain, tbig, k, m, T)
    monkeypatch.setenv("RT_PATH_CHUNK_FRAMES", "1")
    with Context(1) as ctx:
        ctx.set_scene(c3)
        ctx.set_scene_track(tr)
        ctx.set_path_supersampling(K0)
        ctx.set_shutter_adaptive_sampling(T0)
        ctx.reset_stats()
        px = ctx.render_shutter(cams, W0, H0, M0)
        st = ctx.stats()
        apx = ctx.render_anim_shutter(ashut.cameras(tr)[first:first + len(tplain)], W0, H0, m, first_frame=first)
    for f in range(3):
        assert_same(px[f], want[f], f"chunked frame {f}")
        assert_same(apx[f], twant[f], f"chunked track frame {f}")
    assert st["launches"] == 3 and st["frames"] == 3 and st["primary_rays"] == sa.expected_primary(plain, M0, K0, T0)


def test_after_the_refusals_the_other_renders_are_what_they_were(oracle, c3, c3_ctx, c3_sub):
    import torch
    cams, plain, _, _, order = c3_sub
    c3_ctx.set_path_supersampling(1)
    c3_ctx.set_shutter_adaptive_sampling(0)
    c3_ctx.render(W0, H0)
    ref_render = c3_ctx.render(W0, H0).copy()
    ref_shutter = c3_ctx.render_shutter(cams, W0, H0, M0).copy()
    ref_anim = c3_ctx.render_anim(None, W0, H0).copy()
    c3_ctx.set_path_supersampling(K0)
    c3_ctx.set_shutter_adaptive_sampling(T0)
    out = torch.empty((3, H0, W0), dtype=torch.int32, device="cuda")
    assert _code(lambda: c3_ctx.render_shutter_bands(W0, H0, cams, M0, 12, 0, 1, out.data_ptr(), H0 * W0 * 4, abi.RT_BANDS_INT32, _stream())) == abi.RT_ERR_UNSUPPORTED
    c3_ctx.set_shutter_adaptive_sampling(0)
    c3_ctx.set_path_adaptive_sampling(T0)
    assert _code(lambda: c3_ctx.render_shutter(cams, W0, H0, M0)) == abi.RT_ERR_UNSUPPORTED
    c3_ctx.set_path_adaptive_sampling(0)
    c3_ctx.set_shutter_adaptive_sampling(T0)
    assert np.array_equal(c3_ctx.render(W0, H0), ref_render), "render ignores the setting"
    c3_ctx.set_path_supersampling(1)
    assert np.array_equal(c3_ctx.render_shutter(cams, W0, H0, M0), ref_shutter), "k = 1: the shutter render it was"
    assert np.array_equal(ref_shutter, path.shutter_mean(plain, M0))
    assert np.array_equal(c3_ctx.render_anim(None, W0, H0), ref_anim)
    c3_ctx.set_path_supersampling(K0)
    tp, tb, _ = pc.track_frames(oracle, sa.track("direct_m2"), K0)
    assert np.array_equal(c3_ctx.render_anim(None, W0, H0), path_resolve(tb, K0, 1)), "render_anim at k = 2 ignores the shutter threshold"
