"""Adaptive supersampling (rt_set_adaptive_sampling with rt_set_supersampling) on the GPU: every frame bit-exact
against the definition, supersample.adaptive_resolve of the oracle's plain and k W x k H frames, and the ray counts
equal to the oracle's over the samples the definition traces -- sample (0, 0) of every pixel and every sample of the
refined tiles.  tests/test_adaptive.py asserts the preconditions: every case has refined and flat tiles, and an
expectation that is neither the plain frame nor the fully supersampled one.  Each oracle render is computed once and
shared read-only (tests/adaptive_cases.py)."""
import numpy as np
import pytest

import adaptive_cases as ac
from raytracer_hip import Context, abi, path, wire_layout
from raytracer_hip.supersample import box_resolve
from test_gpu_supersample import _band_rows_of, assert_same, ray_counts

pytestmark = pytest.mark.gpu


def _stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


def _code(call):
    with pytest.raises(abi.RayTracerError) as ei:
        call()
    return ei.value.code


def expected_primary(oracle, cid, W, H, k, T):
    plain = ac.frames(oracle, cid, W, H, 1)[0]
    return W * H + (k * k - 1) * int(ac.pixel_mask(plain, T).sum())


_SEGS = {}


def expected_counts(oracle, cid, W, H, k, T):
    """primary / reflect / shadow rays of the samples an adaptive render traces, from the oracle's per-sample
    segments at k W x k H (whose totals are first held against oracle.render's counts)."""
    key = (cid, W, H, k)
    if key not in _SEGS:
        big, st = ac.frames(oracle, cid, W, H, k)
        seg = oracle.segments(ac.scene(cid).resized(k * W, k * H), 1)
        per = [np.bincount(seg["pixel"][seg["kind"] == kind], minlength=big.size).reshape(big.shape) for kind in (0, 1, 2)]
        assert [int(p.sum()) for p in per] == [st["primary_rays"], st["reflect_rays"], st["shadow_rays"]], \
            "the per-sample segments add up to the oracle's counts"
        assert (per[0] == 1).all()
        _SEGS[key] = per
    per = _SEGS[key]
    traced = ac.traced_samples(ac.frames(oracle, cid, W, H, 1)[0], k, T)
    return {name: int(p[traced].sum()) for name, p in zip(("primary_rays", "reflect_rays", "shadow_rays"), per)}


@pytest.mark.parametrize("case", ac.CASES_K2, ids=ac.case_id)
def test_scenes_bit_exact_with_traced_sample_counts(oracle, case):
    cid, W, H, k, T = case
    want = ac.expect(oracle, cid, W, H, k, T)
    counts = expected_counts(oracle, cid, W, H, k, T)
    with Context(1) as ctx:
        ctx.set_scene(ac.scene(cid))
        ctx.set_supersampling(k)
        ctx.set_adaptive_sampling(T)
        assert ctx.adaptive_sampling == T and ctx.supersampling == k
        ctx.reset_stats()
        px = ctx.render(W, H).copy()
        st = ctx.stats()
    assert_same(px, want, ac.case_id(case))
    assert st["primary_rays"] == expected_primary(oracle, cid, W, H, k, T) == counts["primary_rays"]
    assert ray_counts(st) == counts, "the ray counts are the oracle's over the traced samples"
    assert st["pixels"] == W * H and st["frames"] == 1, "frames and pixels count the output"


@pytest.mark.parametrize("case", ac.CASES_K48, ids=ac.case_id)
def test_both_families_at_4_and_8(oracle, case):
    cid, W, H, k, T = case
    want = ac.expect(oracle, cid, W, H, k, T)
    with Context(1) as ctx:
        ctx.set_scene(ac.scene(cid))
        ctx.set_supersampling(k)
        ctx.set_adaptive_sampling(T)
        ctx.reset_stats()
        px = ctx.render(W, H).copy()
        st = ctx.stats()
    assert_same(px, want, ac.case_id(case))
    assert st["primary_rays"] == expected_primary(oracle, cid, W, H, k, T)


W0, H0, T0 = ac.W0, ac.H0, ac.T0


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
def ctx0(_ctx0):
    """The module's context, with every setting a test may change put back after it."""
    yield _ctx0
    _ctx0.set_supersampling(1)
    _ctx0.set_adaptive_sampling(0)
    _ctx0.set_counting(True)
    _ctx0.set_view_height(0)


def _plain_counts(oracle, cid):
    return ray_counts(ac.frames(oracle, cid, W0, H0, 1)[1])


@pytest.mark.parametrize("k", [2, 4])
def test_256_is_the_plain_frame_and_its_counts(oracle, cid, ctx0, k):
    ctx0.set_supersampling(k)
    ctx0.set_adaptive_sampling(256)
    ctx0.reset_stats()
    px = ctx0.render(W0, H0).copy()
    assert_same(px, ac.frames(oracle, cid, W0, H0, 1)[0], f"{cid} k={k} T=256")
    assert ray_counts(ctx0.stats()) == _plain_counts(oracle, cid)


def test_0_is_full_supersampling_before_and_after_a_threshold(oracle, cid, ctx0):
    k = 2
    big, ost = ac.frames(oracle, cid, W0, H0, k)
    want = box_resolve(big, k)
    ctx0.set_supersampling(k)
    assert ctx0.adaptive_sampling == 0
    runs = []
    for T in (0, T0, 0):
        ctx0.set_adaptive_sampling(T)
        ctx0.reset_stats()
        runs.append((ctx0.render(W0, H0).copy(), ray_counts(ctx0.stats())))
    assert_same(runs[0][0], want, "T = 0")
    assert runs[0][1] == ray_counts(ost) and runs[0][1]["primary_rays"] == k * k * W0 * H0
    assert_same(runs[2][0], runs[0][0], "T = 0 after T > 0")
    assert runs[2][1] == runs[0][1]
    assert_same(runs[1][0], ac.expect(oracle, cid, W0, H0, k, T0), "T > 0 between")
    assert (runs[1][0] != runs[0][0]).sum() >= 16


def test_the_setting_is_ignored_at_factor_1(oracle, cid, ctx0):
    ctx0.set_adaptive_sampling(1)
    ctx0.reset_stats()
    assert_same(ctx0.render(W0, H0).copy(), ac.frames(oracle, cid, W0, H0, 1)[0], "k = 1, T = 1")
    assert ray_counts(ctx0.stats()) == _plain_counts(oracle, cid)
    assert ctx0.adaptive_sampling == 1
    for bad in (-1, 257):
        assert _code(lambda: ctx0.set_adaptive_sampling(bad)) == abi.RT_ERR_INVALID_ARG
    assert ctx0.adaptive_sampling == 1


@pytest.mark.parametrize("w,h,k,T", [(1, 1, 2, 1), (9, 9, 2, 16), (5, 3, 4, 16), (9, 9, 8, 1), (17, 8, 4, 32)])
def test_ragged_output_sizes(oracle, w, h, k, T):
    want = ac.expect(oracle, "C3", w, h, k, T)
    with Context(1) as ctx:
        ctx.set_scene(ac.scene("C3").resized(w, h))
        ctx.set_supersampling(k)
        ctx.set_adaptive_sampling(T)
        ctx.reset_stats()
        assert_same(ctx.render(w, h).copy(), want, f"{w}x{h} k={k} T={T}")
        assert ctx.stats()["primary_rays"] == expected_primary(oracle, "C3", w, h, k, T)


@pytest.mark.parametrize("first,step", [(0, 1), (1, 2), (2, 3)])
@pytest.mark.parametrize("band_rows", [8, 16])
def test_render_bands_ex_every_format(oracle, cid, ctx0, band_rows, first, step):
    import torch
    k = 2
    want = ac.expect(oracle, cid, W0, H0, k, T0)
    ctx0.set_supersampling(k)
    ctx0.set_adaptive_sampling(T0)
    st = _stream()
    rows = _band_rows_of(first, step, band_rows, H0)
    others = sorted(set(range(H0)) - set(rows))
    nb_want = -(-len(rows) // band_rows)
    what = f"{cid} band_rows={band_rows} bands ({first}, {step})"
    # FRAME: the bands straight into their rows of a row-major frame; every other row stays
    frame = torch.full((H0 * W0 + 64,), -1, dtype=torch.int32, device="cuda")
    assert ctx0.render_bands_ex(W0, H0, band_rows, first, step, frame.data_ptr(), abi.RT_BANDS_FRAME, st) == nb_want
    torch.cuda.synchronize()
    host = frame.cpu().numpy()
    got = host[:H0 * W0].reshape(H0, W0)
    assert_same(got[rows], want[rows], f"FRAME {what}")
    assert (got[others] == -1).all(), "other ranks' rows untouched"
    assert (host[H0 * W0:] == -1).all()
    # INT32: the packed band set
    bands = torch.full((nb_want * band_rows * W0 + 64,), -1, dtype=torch.int32, device="cuda")
    assert ctx0.render_bands_ex(W0, H0, band_rows, first, step, bands.data_ptr(), abi.RT_BANDS_INT32, st) == nb_want
    torch.cuda.synchronize()
    hb = bands.cpu().numpy()
    assert_same(hb[:len(rows) * W0].reshape(len(rows), W0), want[rows], f"INT32 {what}")
    assert (hb[len(rows) * W0:] == -1).all(), "rows past the image and past the band set stay untouched"
    # RGB24: bytes B, G, R
    raw = torch.full((len(rows) * W0 * 3 + 64,), 0xA5, dtype=torch.uint8, device="cuda")
    ctx0.render_bands_ex(W0, H0, band_rows, first, step, raw.data_ptr(), abi.RT_BANDS_RGB24, st)
    torch.cuda.synchronize()
    hr = raw.cpu().numpy()
    b = hr[:len(rows) * W0 * 3].reshape(len(rows), W0, 3).astype(np.int32)
    assert_same(b[..., 0] | (b[..., 1] << 8) | (b[..., 2] << 16), want[rows], f"RGB24 {what}")
    assert (hr[len(rows) * W0 * 3:] == 0xA5).all()


def test_bands_off_the_tile_grid_are_unsupported(oracle, cid, ctx0):
    import torch
    k = 2
    ctx0.set_supersampling(k)
    ctx0.set_adaptive_sampling(T0)
    out = torch.full((3 * H0 * W0,), -1, dtype=torch.int32, device="cuda")
    for fmt in (abi.RT_BANDS_INT32, abi.RT_BANDS_RGB24, abi.RT_BANDS_FRAME):
        assert _code(lambda: ctx0.render_bands_ex(W0, H0, 12, 0, 1, out.data_ptr(), fmt, _stream())) == abi.RT_ERR_UNSUPPORTED
    assert _code(lambda: ctx0.render_bands_batch(W0, H0, 12, 0, 1, 3, out.data_ptr(), H0 * W0 * 4, abi.RT_BANDS_FRAME,
                                                 _stream())) == abi.RT_ERR_UNSUPPORTED
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == -1).all(), "a refused call writes nothing"
    # the context goes on: the same bands with the setting off, a band that covers the frame with it on
    want = ac.expect(oracle, cid, W0, H0, k, T0)
    assert ctx0.render_bands_ex(W0, H0, H0 + 3, 0, 1, out.data_ptr(), abi.RT_BANDS_INT32, _stream()) == 1
    torch.cuda.synchronize()
    assert_same(out.cpu().numpy()[:H0 * W0].reshape(H0, W0), want, "one band of more rows than the frame")
    ctx0.set_adaptive_sampling(0)
    assert ctx0.render_bands_ex(W0, H0, 12, 0, 1, out.data_ptr(), abi.RT_BANDS_INT32, _stream()) == 3
    torch.cuda.synchronize()
    assert_same(out.cpu().numpy()[:H0 * W0].reshape(H0, W0), box_resolve(ac.frames(oracle, cid, W0, H0, k)[0], k),
                "band_rows 12 with the setting off")


def test_render_bands_batch(oracle, cid, ctx0):
    import torch
    n_frames, world, band_rows, k = 3, 3, 8, 2
    want = ac.expect(oracle, cid, W0, H0, k, T0)
    counts = expected_counts(oracle, cid, W0, H0, k, T0)
    ctx0.set_supersampling(k)
    ctx0.set_adaptive_sampling(T0)
    ctx0.reset_stats()
    stride = H0 * W0 + 32  # int32 per frame
    out = torch.full((n_frames * stride,), -1, dtype=torch.int32, device="cuda")
    for r in range(world):
        ctx0.render_bands_batch(W0, H0, band_rows, r, world, n_frames, out.data_ptr(), stride * 4, abi.RT_BANDS_FRAME, _stream())
    torch.cuda.synchronize()
    host = out.cpu().numpy().reshape(n_frames, stride)
    for f in range(n_frames):
        assert_same(host[f, :H0 * W0].reshape(H0, W0), want, f"batch frame {f}")
        assert (host[f, H0 * W0:] == -1).all()
    assert ray_counts(ctx0.stats()) == {key: n_frames * v for key, v in counts.items()}, "frame 0 counts for all frames"
    # a whole frame as one band, packed INT32
    out = torch.full((n_frames * stride,), -1, dtype=torch.int32, device="cuda")
    ctx0.render_bands_batch(W0, H0, H0, 0, 1, n_frames, out.data_ptr(), stride * 4, abi.RT_BANDS_INT32, _stream())
    torch.cuda.synchronize()
    host = out.cpu().numpy().reshape(n_frames, stride)
    for f in range(n_frames):
        assert_same(host[f, :H0 * W0].reshape(H0, W0), want, f"one-band batch frame {f}")


def test_render_async_captures_the_threshold(oracle, cid, ctx0):
    k = 2
    ctx0.set_supersampling(k)
    Ts = (T0, 256)
    outs = [np.full(W0 * H0, -1, dtype=np.int32) for _ in Ts]
    for T, out in zip(Ts, outs):
        ctx0.set_adaptive_sampling(T)
        ctx0.render_async(W0, H0, out)
    ctx0.set_adaptive_sampling(0)  # (after the calls: no queued frame may see it)
    ctx0.wait()
    for T, out in zip(Ts, outs):
        assert_same(out.reshape(H0, W0), ac.expect(oracle, cid, W0, H0, k, T), f"async frame queued at T={T}")


@pytest.mark.parametrize("k", [2, 4])
def test_render_and_render_device(oracle, cid, ctx0, k):
    import torch
    want = ac.expect(oracle, cid, W0, H0, k, T0)
    ctx0.set_supersampling(k)
    ctx0.set_adaptive_sampling(T0)
    assert_same(ctx0.render(W0, H0).copy(), want, f"{cid} rt_render k={k}")
    pinned = np.full(W0 * H0, -1, dtype=np.int32)
    ctx0.register_host(pinned)
    try:
        ctx0.render(W0, H0, pinned)
        assert_same(pinned.reshape(H0, W0), want, f"{cid} rt_render into a registered buffer k={k}")
    finally:
        ctx0.unregister_host(pinned)
    out = torch.full((H0 * W0 + 64,), -1, dtype=torch.int32, device="cuda")
    for _ in range(2):
        ctx0.render_device(W0, H0, out.data_ptr(), _stream())
    torch.cuda.synchronize()
    host = out.cpu().numpy()
    assert_same(host[:H0 * W0].reshape(H0, W0), want, f"{cid} rt_render_device k={k}")
    assert (host[H0 * W0:] == -1).all(), "nothing written past the width x height output"


def test_shared_device_context_of_two_workers(oracle, cid):
    import torch
    k = 2
    want = ac.expect(oracle, cid, W0, H0, k, T0)
    counts = expected_counts(oracle, cid, W0, H0, k, T0)
    with Context(2, abi.RT_CREATE_SHARED_DEVICE) as ctx:
        ctx.set_scene(ac.scene(cid).resized(W0, H0))
        ctx.set_supersampling(k)
        ctx.set_adaptive_sampling(T0)
        ctx.reset_stats()
        assert_same(ctx.render(W0, H0).copy(), want, "2 workers rt_render")
        assert ray_counts(ctx.stats()) == counts
        pinned = np.full(W0 * H0, -1, dtype=np.int32)
        ctx.register_host(pinned)
        try:
            ctx.render(W0, H0, pinned)
            assert_same(pinned.reshape(H0, W0), want, "2 workers rt_render into a registered frame (copy slices)")
            a = np.full(W0 * H0, -1, dtype=np.int32)
            ctx.render_async(W0, H0, pinned)
            ctx.render_async(W0, H0, a)
            ctx.wait()
            assert_same(pinned.reshape(H0, W0), want, "2 workers rt_render_async")
            assert_same(a.reshape(H0, W0), want, "2 workers rt_render_async, second frame")
        finally:
            ctx.unregister_host(pinned)
        out = torch.full((H0 * W0,), -1, dtype=torch.int32, device="cuda")
        ctx.render_device(W0, H0, out.data_ptr(), _stream())
        torch.cuda.synchronize()
        assert_same(out.cpu().numpy().reshape(H0, W0), want, "2 workers rt_render_device")


def test_view_height_cuts_the_last_tile_row(oracle, cid, ctx0):
    k, rows = 2, 22
    want = ac.expect(oracle, cid, W0, rows, k, T0, view_h=H0)
    whole = ac.expect(oracle, cid, W0, H0, k, T0)
    ctx0.set_supersampling(k)
    ctx0.set_adaptive_sampling(T0)
    ctx0.set_view_height(H0)
    ctx0.reset_stats()
    px = ctx0.render(W0, rows).copy()
    assert_same(px, want, f"50x{rows} of a 50x{H0} view")
    plain = ac.frames(oracle, cid, W0, rows, 1, H0)[0]
    assert ctx0.stats()["primary_rays"] == W0 * rows + (k * k - 1) * int(ac.pixel_mask(plain, T0).sum())
    assert_same(px[:16], whole[:16], "tile rows that are whole in both renders")


def test_counting_off_changes_no_pixel(oracle, cid, ctx0):
    k = 2
    ctx0.set_supersampling(k)
    ctx0.set_adaptive_sampling(T0)
    ctx0.reset_stats()
    ctx0.set_counting(False)
    assert_same(ctx0.render(W0, H0).copy(), ac.expect(oracle, cid, W0, H0, k, T0), "counting off")
    st = ctx0.stats()
    assert st["primary_rays"] == 0 and st["reflect_rays"] == 0 and st["shadow_rays"] == 0, "nothing is counted"
    assert st["frames"] == 1 and st["pixels"] == W0 * H0


def test_paths_shutters_and_tiles_still_refuse_supersampling(cid, ctx0):
    import torch
    cam = ac.scene(cid).c_camera()
    lay = wire_layout(W0, H0, 8, 1, 1)
    wire = torch.zeros(int(lay.max_bytes) + 8, dtype=torch.uint8, device="cuda")
    out = torch.full((2 * H0 * W0,), -1, dtype=torch.int32, device="cuda")
    ctx0.set_supersampling(2)
    ctx0.set_adaptive_sampling(T0)
    cams = path.as_array([cam, cam])
    fb = H0 * W0 * 4
    refused = [
        lambda: ctx0.render_path_bands(W0, H0, cams, H0, 0, 1, out.data_ptr(), fb, abi.RT_BANDS_INT32, _stream()),
        lambda: ctx0.render_path(cams, W0, H0),
        lambda: ctx0.render_shutter_bands(W0, H0, cams, 2, H0, 0, 1, out.data_ptr(), fb, abi.RT_BANDS_INT32, _stream()),
        lambda: ctx0.render_shutter(cams, W0, H0, 2),
        lambda: ctx0.render_bands_tiles(W0, H0, 8, 0, 1, 0, 1, 1, wire.data_ptr(), _stream()),
        lambda: ctx0.count_work(W0, H0),
    ]
    for call in refused:
        assert _code(call) == abi.RT_ERR_UNSUPPORTED
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == -1).all(), "a refused call writes nothing"
