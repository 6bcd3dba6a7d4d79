"""rt_set_path_adaptive_sampling on the GPU: the camera-path and scene-track renders supersampled per 8x8 output tile
inside the trace kernels (the PATH_ADAPT / ANIM_ADAPT instantiations).  Every output frame is bit-exact against
supersample.path_adaptive_resolve of the unchanged oracle's plain and k W x k H frames -- each frame decided on its own
plain frame, in its own view and scene -- and the ray counts equal the oracle's over the samples the definition traces,
summed over the frames.  No tolerance anywhere.  tests/test_path_adaptive.py holds the preconditions: at every scene, size
and threshold used here the cameras have refined and flat tiles, different masks, and expectations that are neither the
plain nor the fully supersampled frames.  Camera i of a list is tests/path_cases.py's camera i % 6."""
import ctypes as C

import numpy as np
import pytest

import anim_cases
import path_adaptive_cases as pc
import path_cases
from raytracer_hip import Context, abi
from raytracer_hip.supersample import path_resolve
from test_gpu_supersample import _band_rows_of

pytestmark = pytest.mark.gpu

N, RAYS = pc.N, pc.RAYS
W0, H0, T0 = pc.W0, pc.H0, pc.T0
KEYS = RAYS + ("frames", "pixels", "launches")


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


# ---- path renders --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", pc.PATH_K2, ids=lambda c: f"{c[0]}-{c[1]}x{c[2]}-T{c[3]}")
def test_path_every_scene_at_k_2(oracle, case):
    """Both families, every class among them, the Math.Pow entry points and the scratch stack (REF), 6 cameras each."""
    cid, W, H, T = case
    sc = pc.scene(cid, W, H)
    cams, order = pc.cycled(sc, 6)
    want = pc.expected(oracle, sc, order, 2, T)
    counts = pc.path_counts(oracle, sc, order, 2, T)
    with Context(1) as ctx:
        ctx.set_scene(sc)
        assert ctx.get_path_adaptive_sampling() == 0
        ctx.set_path_supersampling(2)
        ctx.set_path_adaptive_sampling(T)
        assert ctx.get_path_adaptive_sampling() == T and ctx.get_path_supersampling() == 2 and ctx.adaptive_sampling == 0
        ctx.reset_stats()
        px = ctx.render_path(cams, W, H)
        st = ctx.stats()
    assert px.shape == (6, H, W)
    for f in range(6):
        assert_same(px[f], want[f], f"{cid} {W}x{H} T={T} frame {f}")
    assert (px[0] == px[5]).all(), "equal cameras, equal frames"
    assert counts["primary_rays"] == pc.expected_primary(pc.path_frames(oracle, sc, 2)[0][order], 2, T)
    assert ray_counts(st) == counts, "the ray counts are the oracle's over the traced samples, summed over the frames"
    assert st["frames"] == 6 and st["pixels"] == 6 * W * H and st["launches"] == 1


@pytest.mark.parametrize("case", pc.PATH_K48, ids=lambda c: f"{c[0]}-k{c[4]}")
def test_path_k_4_and_8_with_partly_invalid_edge_tiles(oracle, case):
    """k = 8: 64 passes fill the 16-bit sums.  50 x 30: the last tile column is 2 wide, the last tile row 6 high."""
    cid, W, H, T, k, n = case
    sc = pc.scene(cid, W, H)
    cams, order = pc.cycled(sc, n)
    want = pc.expected(oracle, sc, order, k, T)
    with Context(1) as ctx:
        ctx.set_scene(sc)
        ctx.set_path_supersampling(k)
        ctx.set_path_adaptive_sampling(T)
        ctx.reset_stats()
        px = ctx.render_path(cams, W, H)
        st = ctx.stats()
    for f in range(n):
        assert_same(px[f], want[f], f"{cid} k={k} T={T} frame {f}")
    assert st["primary_rays"] == pc.expected_primary(pc.path_frames(oracle, sc, k)[0][order], k, T)
    assert st["frames"] == n and st["pixels"] == n * W * H


# ---- scene tracks --------------------------------------------------------------------------------------------------
def check_track(oracle, name, k, first_frame=0, counts=True):
    tr, T = pc.track(name), pc.TRACKS[name][1]
    W, H = tr[0].width, tr[0].height
    plain, big, stats = pc.track_frames(oracle, tr, k)
    sl = slice(first_frame, len(tr))
    want = pc.path_adaptive_resolve(plain[sl], big[sl], k, T)
    n = len(tr) - first_frame
    with Context(1) as ctx:
        ctx.set_scene_track(tr)
        ctx.set_path_supersampling(k)
        ctx.set_path_adaptive_sampling(T)
        ctx.reset_stats()
        px = ctx.render_anim(None, W, H, first_frame=first_frame)
        st = ctx.stats()
    assert px.shape == (n, H, W)
    for j in range(n):
        assert_same(px[j], want[j], f"track {name} k={k} T={T} frame {first_frame + j}")
    assert st["primary_rays"] == pc.expected_primary(plain[sl], k, T)
    if counts:
        assert ray_counts(st) == pc.traced_counts(oracle, tr[sl], plain[sl], big[sl], stats[sl], k, T)
    assert st["frames"] == n and st["pixels"] == n * W * H and st["launches"] == 1
    return px


def test_anim_direct_track_at_k_2(oracle):
    px = check_track(oracle, "direct", 2)
    assert (px[0] == px[5]).all() and (px[0] != px[2]).any() and (px[2] != px[4]).any()


def test_anim_direct_track_at_k_4(oracle):
    check_track(oracle, "direct", 4, counts=False)


def test_anim_frames_from_first_frame_2_use_their_own_scenes(oracle):
    check_track(oracle, "direct", 2, first_frame=2)


def test_anim_bundle_track_at_k_2(oracle):
    check_track(oracle, "bundle", 2)


@pytest.mark.parametrize("name", ["mixed_s8", "mixed_s12"])
def test_anim_track_that_mixes_gpow_and_other_frames(oracle, name):
    check_track(oracle, name, 2)


def test_anim_decision_follows_each_frame_s_scene_under_one_camera(oracle):
    """Every frame from frame 0's camera: only the scenes differ, and so do the masks (tests/test_path_adaptive.py)."""
    check_track(oracle, "one_camera", 2)


# ---- the frame of the band, view, chunk and context tests ----------------------------------------------------------
@pytest.fixture(scope="module")
def c3():
    return pc.scene("C3", W0, H0)


@pytest.fixture(scope="module")
def _c3_ctx(c3):
    ctx = Context(1)
    ctx.set_scene(c3)
    ctx.set_scene_track(pc.track("direct"))
    yield ctx
    ctx.close()


@pytest.fixture
def c3_ctx(_c3_ctx):
    """The module's context at k = 2 and T0, with every setting a test may change put back after it."""
    _c3_ctx.set_path_supersampling(2)
    _c3_ctx.set_path_adaptive_sampling(T0)
    yield _c3_ctx
    _c3_ctx.set_path_supersampling(1)
    _c3_ctx.set_path_adaptive_sampling(0)
    _c3_ctx.set_supersampling(1)
    _c3_ctx.set_adaptive_sampling(0)
    _c3_ctx.set_counting(True)
    _c3_ctx.set_view_height(0)


@pytest.mark.parametrize("anim", [False, True], ids=["path", "anim"])
@pytest.mark.parametrize("first,step", [(0, 1), (1, 2), (2, 3)])
def test_bands_and_formats_leave_padding_and_other_ranks_rows_alone(oracle, c3, c3_ctx, first, step, anim):
    import torch
    band_rows, F, k = 8, 3, 2
    if anim:
        plain, big, _ = pc.track_frames(oracle, pc.track("direct"), k)
        want, plain, cams = pc.path_adaptive_resolve(plain[1:1 + F], big[1:1 + F], k, T0), plain[1:1 + F], None
    else:
        cams, order = pc.cycled(c3, F)
        want, plain = pc.expected(oracle, c3, order, k, T0), pc.path_frames(oracle, c3, k)[0][order]
    rows = _band_rows_of(first, step, band_rows, H0)
    nb_want = -(-len(rows) // band_rows)
    others = [y for y in range(H0) if y not in rows]

    def call(ptr, stride, fmt):
        if anim:
            return c3_ctx.render_anim_bands(W0, H0, [sc.c_camera() for sc in pc.track("direct")[1:1 + F]], band_rows, first, step, ptr,
                                            stride, fmt, _stream(), first_frame=1)
        return c3_ctx.render_path_bands(W0, H0, cams, band_rows, first, step, ptr, stride, fmt, _stream())

    # INT32: packed band sets
    stride = nb_want * band_rows * W0 * 4 + 64
    out = torch.full((F * stride // 4,), -1, dtype=torch.int32, device="cuda")
    c3_ctx.reset_stats()
    nb = call(out.data_ptr(), stride, abi.RT_BANDS_INT32)
    torch.cuda.synchronize()
    assert nb == nb_want
    host = out.cpu().numpy().reshape(F, stride // 4)
    for f in range(F):
        assert_same(host[f, :len(rows) * W0].reshape(len(rows), W0), want[f][rows], f"INT32 ({first},{step}) frame {f}")
        assert (host[f, len(rows) * W0:] == -1).all(), "rows past the image and the stride's padding stay untouched"
    st = c3_ctx.stats()
    assert st["launches"] == 1 and st["pixels"] == F * nb * band_rows * W0
    # (8-row bands are tile rows: a band's tiles decide as the whole frame's do)
    assert st["primary_rays"] == sum(len(rows) * W0 + (k * k - 1) * int(pc.pixel_mask(p, T0)[rows].sum()) for p in plain)
    # RGB24: bytes B, G, R
    stride = nb_want * band_rows * W0 * 3 + 64
    raw = torch.full((F * stride,), 0xA5, dtype=torch.uint8, device="cuda")
    call(raw.data_ptr(), stride, abi.RT_BANDS_RGB24)
    torch.cuda.synchronize()
    hr = raw.cpu().numpy().reshape(F, stride)
    for f in range(F):
        b = hr[f, :len(rows) * W0 * 3].reshape(len(rows), W0, 3).astype(np.int32)
        assert_same(b[..., 0] | (b[..., 1] << 8) | (b[..., 2] << 16), want[f][rows], f"RGB24 ({first},{step}) frame {f}")
        assert (hr[f, len(rows) * W0 * 3:] == 0xA5).all()
    # FRAME: the bands in their rows of the row-major frame
    stride = H0 * W0 * 4 + 64
    frame = torch.full((F * stride // 4,), -1, dtype=torch.int32, device="cuda")
    call(frame.data_ptr(), stride, abi.RT_BANDS_FRAME)
    torch.cuda.synchronize()
    hf = frame.cpu().numpy().reshape(F, stride // 4)
    for f in range(F):
        img = hf[f, :H0 * W0].reshape(H0, W0)
        assert_same(img[rows], want[f][rows], f"FRAME ({first},{step}) frame {f}")
        assert (img[others] == -1).all(), "the rows of other ranks stay untouched"
        assert (hf[f, H0 * W0:] == -1).all()


def test_bands_of_5_rows_are_unsupported_and_one_band_of_the_frame_is_accepted(oracle, c3, c3_ctx):
    import torch
    cams, order = pc.cycled(c3, 2)
    track_cams = [sc.c_camera() for sc in pc.track("direct")[:2]]
    nbytes = H0 * W0 * 4
    out = torch.full((2, H0, W0), -1, dtype=torch.int32, device="cuda")
    before = c3_ctx.stats()
    assert _code(lambda: c3_ctx.render_path_bands(W0, H0, cams, 5, 0, 1, out.data_ptr(), nbytes, abi.RT_BANDS_INT32, _stream())) == abi.RT_ERR_UNSUPPORTED
    assert _code(lambda: c3_ctx.render_anim_bands(W0, H0, track_cams, 5, 0, 1, out.data_ptr(), nbytes, abi.RT_BANDS_FRAME, _stream())) == abi.RT_ERR_UNSUPPORTED
    assert _code(lambda: c3_ctx.render_shutter_bands(W0, H0, cams, 1, 5, 0, 1, out.data_ptr(), nbytes, abi.RT_BANDS_INT32, _stream())) == abi.RT_ERR_UNSUPPORTED
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == -1).all(), "a refused call writes nothing"
    after = c3_ctx.stats()
    assert {k: after[k] for k in KEYS} == {k: before[k] for k in KEYS}
    # T = 0 or k = 1: 5-row bands are fine again
    c3_ctx.set_path_adaptive_sampling(0)
    c3_ctx.render_path_bands(W0, H0, cams, 5, 0, 1, out.data_ptr(), nbytes, abi.RT_BANDS_INT32, _stream())
    c3_ctx.set_path_adaptive_sampling(T0)
    c3_ctx.set_path_supersampling(1)
    c3_ctx.render_path_bands(W0, H0, cams, 5, 0, 1, out.data_ptr(), nbytes, abi.RT_BANDS_INT32, _stream())
    c3_ctx.set_path_supersampling(2)
    # band_rows >= height: the frame as one band, whatever the number
    want = pc.expected(oracle, c3, order, 2, T0)
    for band_rows in (H0, H0 + 7):
        out.fill_(-1)
        assert c3_ctx.render_path_bands(W0, H0, cams, band_rows, 0, 1, out.data_ptr(), nbytes, abi.RT_BANDS_FRAME, _stream()) == 1
        torch.cuda.synchronize()
        host = out.cpu().numpy()
        for f in range(2):
            assert_same(host[f], want[f], f"band_rows {band_rows} frame {f}")


def test_view_height_cuts_the_last_tile_row_and_its_decision(oracle, c3, c3_ctx):
    rows = pc.VIEW_ROWS
    cams, order = pc.cycled(c3, 6)
    want = pc.expected(oracle, c3, order, 2, T0, rows, H0)
    plain = pc.path_frames(oracle, c3, 2, rows, H0)[0][order]
    c3_ctx.set_view_height(H0)
    c3_ctx.reset_stats()
    px = c3_ctx.render_path(cams, W0, rows)
    st = c3_ctx.stats()
    assert px.shape == (6, rows, W0)
    for f in range(6):
        assert_same(px[f], want[f], f"{W0}x{rows} of a {W0}x{H0} view, frame {f}")
    assert st["primary_rays"] == pc.expected_primary(plain, 2, T0)
    assert _code(lambda: c3_ctx.render_path(cams, W0, H0 + 1)) == abi.RT_ERR_INVALID_ARG


# ---- threshold edges -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [2, 4])
def test_256_is_the_plain_path_render_and_its_counts(oracle, c3, c3_ctx, k):
    cams, order = pc.cycled(c3, 6)
    c3_ctx.set_path_supersampling(1)
    c3_ctx.reset_stats()
    plain = c3_ctx.render_path(cams, W0, H0).copy()
    st_plain = c3_ctx.stats()
    c3_ctx.set_path_supersampling(k)
    c3_ctx.set_path_adaptive_sampling(256)
    c3_ctx.reset_stats()
    px = c3_ctx.render_path(cams, W0, H0)
    st = c3_ctx.stats()
    frames, stats = path_cases.oracle_frames(oracle, c3)
    for f in range(6):
        assert_same(px[f], frames[order[f]], f"T = 256 at k = {k}, frame {f}")
    assert np.array_equal(px, plain), "bit for bit the k = 1 render"
    assert ray_counts(st) == ray_counts(st_plain) == {r: sum(stats[i][r] for i in order) for r in RAYS}


def test_0_is_the_path_ss_render_before_and_after_a_threshold(oracle, c3, c3_ctx):
    cams, order = pc.cycled(c3, 6)
    _, big, stats = pc.path_frames(oracle, c3, 2)
    want = path_resolve(big[order], 2)
    runs = []
    for T in (0, T0, 0):
        c3_ctx.set_path_adaptive_sampling(T)
        c3_ctx.reset_stats()
        runs.append((c3_ctx.render_path(cams, W0, H0).copy(), {k: v for k, v in c3_ctx.stats().items() if k in KEYS}))
    for f in range(6):
        assert_same(runs[0][0][f], want[f], f"T = 0 frame {f}")
    assert ray_counts(runs[0][1]) == {r: sum(stats[i][r] for i in order) for r in RAYS}
    assert np.array_equal(runs[0][0], runs[2][0]) and runs[0][1] == runs[2][1], "T = 0 after a threshold is T = 0 before it"
    assert (runs[1][0] != runs[0][0]).any() and runs[1][1]["primary_rays"] < runs[0][1]["primary_rays"]


def _three_band_calls(ctx, sc, track_cams, shutter=2):
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
            ctx.render_shutter_bands(W0, H0, cams, shutter, 8, 1, 2, buf.data_ptr(), nbytes, abi.RT_BANDS_RGB24, _stream())
        else:
            ctx.render_anim_bands(W0, H0, track_cams, 8, 1, 2, buf.data_ptr(), nbytes, abi.RT_BANDS_FRAME, _stream())
        torch.cuda.synchronize()
        st = ctx.stats()
        bufs.append(buf.cpu().numpy()), stats.append({k: st[k] for k in KEYS})
    return bufs, stats


def test_factor_1_with_a_threshold_is_the_library_without_the_setter(c3):
    track = pc.track("direct")[:3]
    track_cams = [sc.c_camera() for sc in track]
    with Context(1) as ctx:
        ctx.set_scene(c3)
        ctx.set_scene_track(track)
        never, st_never = _three_band_calls(ctx, c3, track_cams)
    with Context(1) as ctx:
        ctx.set_scene(c3)
        ctx.set_scene_track(track)
        ctx.set_path_adaptive_sampling(16)
        assert ctx.get_path_supersampling() == 1
        with_t, st_t = _three_band_calls(ctx, c3, track_cams)  # (k = 1: even the shutter of 2 is rendered)
    for i in range(3):
        assert (never[i] != 0x5A).any()
        assert np.array_equal(never[i], with_t[i]), f"call {i}: byte-identical buffers"
        assert st_never[i] == st_t[i], f"call {i}: identical stats"


# ---- shutter -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", [abi.RT_BANDS_INT32, abi.RT_BANDS_RGB24, abi.RT_BANDS_FRAME])
def test_shutter_1_is_the_path_call(oracle, c3, c3_ctx, fmt):
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
    rows = _band_rows_of(0, 2, 8, H0)
    plain = pc.path_frames(oracle, c3, 2)[0]
    assert sa["primary_rays"] == sum(len(rows) * W0 + 3 * int(pc.pixel_mask(p, T0)[rows].sum()) for p in plain), "the adaptive launch"
    whole = c3_ctx.render_shutter(cams, W0, H0, 1)
    assert np.array_equal(whole, c3_ctx.render_path(cams, W0, H0))
    assert_same(whole[3], pc.expected(oracle, c3, [3], 2, T0)[0], "rt_render_shutter with shutter 1")


def test_shutter_2_is_unsupported_and_writes_nothing(c3, c3_ctx):
    import torch
    cams = path_cases.cameras(c3)
    out = torch.full((3, H0, W0), -1, dtype=torch.int32, device="cuda")
    host = np.full((3, H0, W0), -1, dtype=np.int32)
    before = c3_ctx.stats()
    assert _code(lambda: c3_ctx.render_shutter_bands(W0, H0, cams, 2, H0, 0, 1, out.data_ptr(), H0 * W0 * 4, abi.RT_BANDS_INT32,
                                                     _stream())) == abi.RT_ERR_UNSUPPORTED
    assert b"rt_set_path_adaptive_sampling" in c3_ctx.lib.rt_last_error(c3_ctx.ptr)
    assert _code(lambda: c3_ctx.render_shutter(cams, W0, H0, 2, host)) == abi.RT_ERR_UNSUPPORTED
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == -1).all() and (host == -1).all(), "a refused call writes nothing"
    after = c3_ctx.stats()
    assert {k: after[k] for k in KEYS} == {k: before[k] for k in KEYS}
    # (a bad shutter is still a bad argument, and T = 0 renders the shutter again)
    assert _code(lambda: c3_ctx.render_shutter(cams, W0, H0, 3, host[:2])) == abi.RT_ERR_INVALID_ARG
    c3_ctx.set_path_adaptive_sampling(0)
    assert c3_ctx.render_shutter(cams, W0, H0, 2, host).shape == (3, H0, W0) and (host != -1).all()


# ---- chunks and streams --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("registered", [True, False])
def test_chunked_render_path(oracle, c3, registered, monkeypatch):
    cams, order = pc.cycled(c3, 5, start=1)
    want = pc.expected(oracle, c3, order, 2, T0)
    monkeypatch.setenv("RT_PATH_CHUNK_FRAMES", "2")  # read at rt_create: chunks of 2, 2 and 1 frames
    with Context(1) as ctx:
        ctx.set_scene(c3)
        ctx.set_path_supersampling(2)
        ctx.set_path_adaptive_sampling(T0)
        out = np.full((5, H0, W0), -1, dtype=np.int32)
        if registered:
            ctx.register_host(out)
        try:
            ctx.reset_stats()
            got = ctx.render_path(cams, W0, H0, out)
            st = ctx.stats()
        finally:
            if registered:
                ctx.unregister_host(out)
    assert np.shares_memory(got, out)
    for f in range(5):
        assert_same(out[f], want[f], f"chunked frame {f}, registered={registered}")
    assert st["launches"] == 3 and st["frames"] == 5 and st["pixels"] == 5 * W0 * H0
    assert ray_counts(st) == pc.path_counts(oracle, c3, order, 2, T0)


def test_back_to_back_calls_on_two_streams_with_different_thresholds(oracle, c3, c3_ctx):
    import torch
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    Ts = [T0, 32, 256, 0]
    picks = [pc.cycled(c3, 3, start=i) for i in range(len(Ts))]
    outs = [torch.full((3, H0, W0), -1, dtype=torch.int32, device="cuda") for _ in picks]
    torch.cuda.synchronize()
    for i, ((cams, _), out) in enumerate(zip(picks, outs)):
        c3_ctx.set_path_adaptive_sampling(Ts[i])
        c3_ctx.render_path_bands(W0, H0, cams, H0, 0, 1, out.data_ptr(), H0 * W0 * 4, abi.RT_BANDS_INT32, streams[i % 2].cuda_stream)
    torch.cuda.synchronize()
    for i, ((_, order), out) in enumerate(zip(picks, outs)):
        want = pc.expected(oracle, c3, order, 2, Ts[i])
        host = out.cpu().numpy()
        for f in range(3):
            assert_same(host[f], want[f], f"call {i} at T = {Ts[i]}, frame {f} (camera {order[f]})")
    assert (outs[0].cpu().numpy()[1] != outs[1].cpu().numpy()[0]).any(), "camera 1 at T0 and at 32 differ"


# ---- counting ------------------------------------------------------------------------------------------------------
def test_counting_off_counts_no_rays_and_changes_no_pixel(oracle, c3, c3_ctx):
    cams, order = pc.cycled(c3, 6)
    want = pc.expected(oracle, c3, order, 2, T0)
    plain, big, _ = pc.track_frames(oracle, pc.track("direct"), 2)
    want_anim = pc.path_adaptive_resolve(plain, big, 2, T0)
    c3_ctx.reset_stats()
    c3_ctx.render_path(cams, W0, H0)
    before = c3_ctx.stats()
    c3_ctx.set_counting(False)
    px = c3_ctx.render_path(cams, W0, H0)
    pa = c3_ctx.render_anim(None, W0, H0)
    after = c3_ctx.stats()
    assert ray_counts(after) == ray_counts(before), "nothing counted"
    assert after["frames"] == before["frames"] + 12 and after["pixels"] == before["pixels"] + 12 * W0 * H0
    for f in range(6):
        assert_same(px[f], want[f], f"counting off, path frame {f}")
        assert_same(pa[f], want_anim[f], f"counting off, track frame {f}")


# ---- other renders and context state -------------------------------------------------------------------------------
def test_every_other_render_ignores_the_threshold(c3):
    import torch

    def others(ctx):
        ctx.reset_stats()
        frame = ctx.render(W0, H0).copy()
        batch = torch.full((2, 16, W0), -1, dtype=torch.int32, device="cuda")
        ctx.render_bands_batch(W0, H0, 8, 0, 2, 2, batch.data_ptr(), 16 * W0 * 4, abi.RT_BANDS_INT32, _stream())
        dev = torch.full((H0, W0), -1, dtype=torch.int32, device="cuda")
        ctx.render_device(W0, H0, dev.data_ptr(), _stream())
        torch.cuda.synchronize()
        st = ctx.stats()
        return frame, batch.cpu().numpy(), dev.cpu().numpy(), {k: st[k] for k in KEYS}

    with Context(1) as ctx:
        ctx.set_scene(c3)
        runs = [others(ctx)]
        ctx.set_path_supersampling(4)
        ctx.set_path_adaptive_sampling(16)
        runs.append(others(ctx))
        ctx.set_supersampling(2)  # (and under the one-camera factor: full supersampling, not adaptive)
        ss = others(ctx)
        ctx.set_path_adaptive_sampling(0)
        ss0 = others(ctx)
    assert (runs[0][1] != -1).any() and (runs[0][2] != -1).all()
    for i, what in enumerate(("rt_render", "rt_render_bands_batch", "rt_render_device")):
        assert np.array_equal(runs[0][i], runs[1][i]), what
        assert np.array_equal(ss[i], ss0[i]), f"{what} while supersampling"
    assert runs[0][3] == runs[1][3] and ss[3] == ss0[3], "the stats"
    assert ss[3]["primary_rays"] == 4 * runs[0][3]["primary_rays"]


def test_rt_set_adaptive_sampling_stays_ignored_by_the_six_calls(oracle, c3, c3_ctx):
    track_cams = [sc.c_camera() for sc in pc.track("direct")]
    c3_ctx.set_path_adaptive_sampling(0)  # (so that the shutter of 2 is rendered)
    cams = path_cases.cameras(c3)

    def six():
        bufs, stats = _three_band_calls(c3_ctx, c3, track_cams)
        c3_ctx.reset_stats()
        whole = [c3_ctx.render_path(cams, W0, H0).copy(), c3_ctx.render_shutter(cams, W0, H0, 2).copy(), c3_ctx.render_anim(None, W0, H0).copy()]
        st = c3_ctx.stats()
        return bufs + whole, stats + [{k: st[k] for k in KEYS}]

    without, st_without = six()
    c3_ctx.set_adaptive_sampling(16)
    with_t, st_with = six()
    for i in range(6):
        assert np.array_equal(without[i], with_t[i]), f"call {i}"
    assert st_without == st_with
    # and beside the path threshold: the path threshold alone decides
    c3_ctx.set_path_adaptive_sampling(T0)
    order = list(range(N))
    px = c3_ctx.render_path(cams, W0, H0)
    want = pc.expected(oracle, c3, order, 2, T0)
    for f in range(N):
        assert_same(px[f], want[f], f"rt_set_adaptive_sampling(16) beside the path threshold, frame {f}")


def test_rt_set_supersampling_still_refuses_all_six_calls(c3, c3_ctx):
    import torch
    cams = path_cases.cameras(c3)[:2]
    out = torch.full((2, H0, W0), -1, dtype=torch.int32, device="cuda")
    host = np.full((2, H0, W0), -1, dtype=np.int32)
    nbytes = H0 * W0 * 4
    c3_ctx.set_supersampling(2)
    calls = [
        lambda: c3_ctx.render_path_bands(W0, H0, cams, H0, 0, 1, out.data_ptr(), nbytes, abi.RT_BANDS_INT32, _stream()),
        lambda: c3_ctx.render_shutter_bands(W0, H0, cams, 1, H0, 0, 1, out.data_ptr(), nbytes, abi.RT_BANDS_INT32, _stream()),
        lambda: c3_ctx.render_anim_bands(W0, H0, cams, H0, 0, 1, out.data_ptr(), nbytes, abi.RT_BANDS_INT32, _stream()),
        lambda: c3_ctx.render_path(cams, W0, H0, host),
        lambda: c3_ctx.render_shutter(cams, W0, H0, 1, host),
        lambda: c3_ctx.render_anim(cams, W0, H0, out=host),
    ]
    for i, fn in enumerate(calls):
        assert _code(fn) == abi.RT_ERR_UNSUPPORTED, f"call {i}"
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == -1).all() and (host == -1).all(), "a refused call writes nothing"


def test_context_camera_and_view_survive_a_call(oracle, c3, c3_ctx):
    frames, _ = path_cases.oracle_frames(oracle, c3)
    own = path_cases.moved(c3, path_cases.OFFSETS[3])
    c3_ctx.set_camera(own.c_camera())
    try:
        assert_same(c3_ctx.render(W0, H0).copy(), frames[3], "rt_render before the call")
        c3_ctx.render_path(pc.cycled(c3, 4)[0], W0, H0)
        c3_ctx.render_anim(None, W0, H0)
        got = c3_ctx.get_camera()
        assert (got.position.x, got.position.z, got.yaw, got.pitch) == (
            own.c_camera().position.x, own.c_camera().position.z, own.c_camera().yaw, own.c_camera().pitch)
        assert_same(c3_ctx.render(W0, H0).copy(), frames[3], "rt_render after the calls")
    finally:
        c3_ctx.set_camera(c3.c_camera())


# ---- bad arguments -------------------------------------------------------------------------------------------------
def test_bad_thresholds_and_null_pointers(c3_ctx):
    lib = c3_ctx.lib
    for t in (-1, 257):
        assert lib.rt_set_path_adaptive_sampling(c3_ctx.ptr, t) == abi.RT_ERR_INVALID_ARG
        assert c3_ctx.get_path_adaptive_sampling() == T0, "a refused threshold changes nothing"
    for t in (0, 1, 256):
        assert lib.rt_set_path_adaptive_sampling(c3_ctx.ptr, t) == abi.RT_OK and c3_ctx.get_path_adaptive_sampling() == t
    assert lib.rt_set_path_adaptive_sampling(None, 16) == abi.RT_ERR_INVALID_ARG
    assert lib.rt_get_path_adaptive_sampling(None, C.byref(C.c_int(0))) == abi.RT_ERR_INVALID_ARG
    assert lib.rt_get_path_adaptive_sampling(c3_ctx.ptr, None) == abi.RT_ERR_INVALID_ARG
