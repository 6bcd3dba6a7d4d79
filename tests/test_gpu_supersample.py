"""Supersampling (rt_set_supersampling, k = 2 / 4 / 8) on the GPU: every frame bit-exact against the definition,
supersample.box_resolve(oracle frame at k W x k H) -- the oracle unchanged, box-reduced in numpy -- and the ray
counts equal to the oracle's at k W x k H.  The expectation is never the plain W x H frame (38-56 % of the
pixels differ, tests/test_supersample.py asserts the precondition), so nothing here passes by ignoring k.
Each oracle render (at most 400 x 240) is computed once per module and shared read-only.
"""
import numpy as np
import pytest

from raytracer_hip import Context, abi, scenes, wire_layout
from raytracer_hip.supersample import box_resolve

pytestmark = pytest.mark.gpu

_EXPECT = {}


def expect(oracle, sc, W, H, k, view_h=None):
    """(frame [H, W], oracle stats) of scene `sc` at W x H output pixels and factor k (rows [0, H) of a view
    `view_h` output rows high)."""
    key = (sc.name, W, H, k, view_h)
    if key not in _EXPECT:
        big = sc.resized(k * W, k * (view_h or H))
        px, st = oracle.render(big, oracle.MODE_NEAREST, 8, rows=(0, k * H))
        out = box_resolve(px, k) if k > 1 else px
        out.setflags(write=False)
        _EXPECT[key] = (out, st)
    return _EXPECT[key]


def assert_same(px, want, what):
    bad = px != want
    if bad.any():
        ys, xs = np.nonzero(bad)
        pytest.fail(f"{what}: {int(bad.sum())} of {bad.size} pixels differ; first at (x={xs[0]}, y={ys[0]}): "
                    f"gpu {px[ys[0], xs[0]]:#08x} expected {want[ys[0], xs[0]]:#08x}")


def ray_counts(st):
    return {k: st[k] for k in ("primary_rays", "reflect_rays", "shadow_rays")}


def _gpow(cid):
    """C3 (direct kernel) / C4 (bundle kernel) with specular exponents 3.7 and 7.25: the Math.Pow instantiations."""
    base = scenes.config(cid)
    sph = [scenes.Sphere(s.center, s.radius, (scenes.Material.metal if i % 2 else scenes.Material.plastic)(
        s.material.kd if any(s.material.kd) else (0.7, 0.6, 0.5), 7.25 if i % 2 else 3.7)) if i % 3 != 2 else s
           for i, s in enumerate(base.spheres)]
    return scenes.Scene(f"{cid}_gpow_ss", 32, 24, sph, base.planes, base.lights, base.ambient, base.recursion_limit,
                        base.camera)


def _bundle_l5():
    """A pass per light (5 lights: past the merged shadow pass), as test_bundle_light_counts_and_stacks builds it."""
    import random_scenes
    n_lights, limit = 5, 5
    base = random_scenes.random_scene(100 + 7 * n_lights + limit, 128, 96, dense=True)
    rng = np.random.default_rng(1000 * n_lights + limit)
    lights = [scenes.Light(tuple(float(np.float32(x)) for x in rng.uniform(-30, 30, 3)),
                           float(np.float32(rng.uniform(0.2, 1.2)))) for _ in range(n_lights)]
    return scenes.Scene(f"bundle_L{n_lights}_lim{limit}_ss", 32, 24, base.spheres, base.planes, lights, base.ambient,
                        limit, base.camera)


def _dense():
    import random_scenes
    return random_scenes.random_scene(101, 128, 96, dense=True).resized(37, 21, "dense101_ss")


SCENES = {
    "REF": lambda: scenes.reference(13, 7),            # direct kernel, limit 32: the scratch stack; k W not a multiple of 8
    "C1": lambda: scenes.config("C1").resized(24, 16),
    "C3": lambda: scenes.config("C3").resized(50, 30),  # direct kernel, LDS stack
    "C4": lambda: scenes.config("C4").resized(50, 30),  # bundle kernel, merged shadow pass, clusters
    "dense": _dense,
    "bundle_L5": _bundle_l5,
    "gpow_direct": lambda: _gpow("C3"),
    "gpow_bundle": lambda: _gpow("C4"),
}


@pytest.mark.parametrize("k", [2, 4, 8])
@pytest.mark.parametrize("name", list(SCENES))
def test_scenes_bit_exact_with_sample_ray_counts(oracle, name, k):
    sc = SCENES[name]()
    W, H = sc.width, sc.height
    want, ost = expect(oracle, sc, W, H, k)
    with Context(1) as ctx:
        ctx.set_scene(sc)
        ctx.set_supersampling(k)
        assert ctx.supersampling == k
        ctx.reset_stats()
        px = ctx.render(W, H).copy()
        st = ctx.stats()
    assert_same(px, want, f"{name} {W}x{H} k={k}")
    assert ray_counts(st) == ray_counts(ost), "the ray counts are the oracle's at k W x k H"
    assert st["primary_rays"] == W * H * k * k
    assert st["pixels"] == W * H and st["frames"] == 1, "frames and pixels count the output"


@pytest.mark.parametrize("w,h,k", [(3, 2, 8), (5, 3, 4), (1, 1, 2)])
def test_ragged_output_sizes(oracle, w, h, k):
    sc = scenes.config("C3").resized(w, h)
    want, _ = expect(oracle, sc, w, h, k)
    with Context(1) as ctx:
        ctx.set_scene(sc)
        ctx.set_supersampling(k)
        assert_same(ctx.render(w, h).copy(), want, f"{w}x{h} k={k}")


W0, H0 = 50, 30


@pytest.fixture(scope="module", params=["C3", "C4"])
def path_scene(request):
    return scenes.config(request.param).resized(W0, H0)


@pytest.fixture(scope="module")
def path_ctx(path_scene):
    ctx = Context(1)
    ctx.set_scene(path_scene)
    yield ctx
    ctx.close()


def _stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


@pytest.mark.parametrize("k", [2, 4])
def test_render_and_render_device(oracle, path_scene, path_ctx, k):
    import torch
    want, _ = expect(oracle, path_scene, W0, H0, k)
    path_ctx.set_supersampling(k)
    assert_same(path_ctx.render(W0, H0).copy(), want, f"{path_scene.name} rt_render k={k}")
    out = torch.full((H0 * W0 + 64,), -1, dtype=torch.int32, device="cuda")
    for _ in range(2):
        path_ctx.render_device(W0, H0, out.data_ptr(), _stream())
    torch.cuda.synchronize()
    host = out.cpu().numpy()
    assert_same(host[:H0 * W0].reshape(H0, W0), want, f"{path_scene.name} rt_render_device k={k}")
    assert (host[H0 * W0:] == -1).all(), "nothing written past the width x height output"


def _band_rows_of(rank, world, band_rows, H):
    """Frame rows of rank's bands, in packed order."""
    rows = []
    b = rank
    while b * band_rows < H:
        rows += list(range(b * band_rows, min((b + 1) * band_rows, H)))
        b += world
    return rows


@pytest.mark.parametrize("band_rows", [8, 3])
@pytest.mark.parametrize("k", [2, 4])
def test_render_bands_ex_every_format(oracle, path_scene, path_ctx, k, band_rows):
    import torch
    world = 3
    want, _ = expect(oracle, path_scene, W0, H0, k)
    path_ctx.set_supersampling(k)
    st = _stream()
    # FRAME: every rank's bands straight into the row-major frame
    frame = torch.full((H0 * W0 + 64,), -1, dtype=torch.int32, device="cuda")
    for r in range(world):
        path_ctx.render_bands_ex(W0, H0, band_rows, r, world, frame.data_ptr(), abi.RT_BANDS_FRAME, st)
    torch.cuda.synchronize()
    host = frame.cpu().numpy()
    assert_same(host[:H0 * W0].reshape(H0, W0), want, f"FRAME band_rows={band_rows} k={k}")
    assert (host[H0 * W0:] == -1).all()
    # INT32: packed band sets, reassembled by rt_scatter_bands
    frame = torch.full((H0 * W0,), -1, dtype=torch.int32, device="cuda")
    for r in range(world):
        rows = _band_rows_of(r, world, band_rows, H0)
        nb_want = -(-len(rows) // band_rows)
        bands = torch.full((nb_want * band_rows * W0 + 64,), -1, dtype=torch.int32, device="cuda")
        nb = path_ctx.render_bands_ex(W0, H0, band_rows, r, world, bands.data_ptr(), abi.RT_BANDS_INT32, st)
        assert nb == nb_want
        torch.cuda.synchronize()
        hb = bands.cpu().numpy()
        assert_same(hb[:len(rows) * W0].reshape(len(rows), W0), want[rows], f"INT32 rank {r} band_rows={band_rows} k={k}")
        assert (hb[len(rows) * W0:] == -1).all(), "rows past the image and past the band set stay untouched"
        path_ctx.scatter_bands(W0, H0, band_rows, r, world, bands.data_ptr(), frame.data_ptr(), st)
    torch.cuda.synchronize()
    assert_same(frame.cpu().numpy().reshape(H0, W0), want, f"INT32 scattered band_rows={band_rows} k={k}")
    # RGB24: bytes B, G, R
    for r in range(world):
        rows = _band_rows_of(r, world, band_rows, H0)
        raw = torch.full((len(rows) * W0 * 3 + 64,), 0xA5, dtype=torch.uint8, device="cuda")
        path_ctx.render_bands_ex(W0, H0, band_rows, r, world, raw.data_ptr(), abi.RT_BANDS_RGB24, st)
        torch.cuda.synchronize()
        hr = raw.cpu().numpy()
        b = hr[:len(rows) * W0 * 3].reshape(len(rows), W0, 3).astype(np.int32)
        assert_same(b[..., 0] | (b[..., 1] << 8) | (b[..., 2] << 16), want[rows], f"RGB24 rank {r} band_rows={band_rows} k={k}")
        assert (hr[len(rows) * W0 * 3:] == 0xA5).all()


@pytest.mark.parametrize("k", [2, 4])
def test_render_bands_batch(oracle, path_scene, path_ctx, k):
    import torch
    n_frames, world, band_rows = 3, 3, 8
    want, ost = expect(oracle, path_scene, W0, H0, k)
    path_ctx.set_supersampling(k)
    path_ctx.reset_stats()
    stride = H0 * W0 + 32  # int32 per frame
    out = torch.full((n_frames * stride,), -1, dtype=torch.int32, device="cuda")
    for r in range(world):
        path_ctx.render_bands_batch(W0, H0, band_rows, r, world, n_frames, out.data_ptr(), stride * 4, abi.RT_BANDS_FRAME,
                                    _stream())
    torch.cuda.synchronize()
    host = out.cpu().numpy().reshape(n_frames, stride)
    for f in range(n_frames):
        assert_same(host[f, :H0 * W0].reshape(H0, W0), want, f"batch frame {f} k={k}")
        assert (host[f, H0 * W0:] == -1).all()
    st = path_ctx.stats()
    assert ray_counts(st) == {key: n_frames * v for key, v in ray_counts(ost).items()}
    # a whole frame as one band, packed INT32
    out = torch.full((n_frames * stride,), -1, dtype=torch.int32, device="cuda")
    path_ctx.render_bands_batch(W0, H0, H0, 0, 1, n_frames, out.data_ptr(), stride * 4, abi.RT_BANDS_INT32, _stream())
    torch.cuda.synchronize()
    host = out.cpu().numpy().reshape(n_frames, stride)
    for f in range(n_frames):
        assert_same(host[f, :H0 * W0].reshape(H0, W0), want, f"one-band batch frame {f} k={k}")


@pytest.mark.parametrize("k", [2, 4])
def test_shared_device_context_of_three_workers(oracle, path_scene, k):
    want, ost = expect(oracle, path_scene, W0, H0, k)
    with Context(3, abi.RT_CREATE_SHARED_DEVICE) as ctx:
        ctx.set_scene(path_scene)
        ctx.set_supersampling(k)
        ctx.reset_stats()
        assert_same(ctx.render(W0, H0).copy(), want, f"3 workers rt_render k={k}")
        assert ray_counts(ctx.stats()) == ray_counts(ost)
        pinned = np.full(W0 * H0, -1, dtype=np.int32)
        ctx.register_host(pinned)
        try:
            ctx.render(W0, H0, pinned)
            assert_same(pinned.reshape(H0, W0), want, f"3 workers rt_render into a registered frame k={k}")
        finally:
            ctx.unregister_host(pinned)


def test_render_async_captures_the_factor(oracle, path_scene, path_ctx):
    ks = (2, 1, 4)
    outs = [np.full(W0 * H0, -1, dtype=np.int32) for _ in ks]
    for k, out in zip(ks, outs):
        path_ctx.set_supersampling(k)
        path_ctx.render_async(W0, H0, out)
    path_ctx.set_supersampling(8)  # (after the calls: no queued frame may see it)
    path_ctx.wait()
    for k, out in zip(ks, outs):
        assert_same(out.reshape(H0, W0), expect(oracle, path_scene, W0, H0, k)[0], f"async frame at k={k}")


@pytest.mark.parametrize("k", [2, 4])
def test_view_height_in_output_pixels(oracle, path_scene, path_ctx, k):
    want, ost = expect(oracle, path_scene, W0, 22, k, view_h=H0)
    path_ctx.set_supersampling(k)
    path_ctx.set_view_height(H0)
    try:
        path_ctx.reset_stats()
        assert_same(path_ctx.render(W0, 22).copy(), want, f"50x22 of a 50x30 view k={k}")
        assert ray_counts(path_ctx.stats()) == ray_counts(ost)
        with pytest.raises(abi.RayTracerError) as ei:
            path_ctx.render(W0, H0 + 1)
        assert ei.value.code == abi.RT_ERR_INVALID_ARG
    finally:
        path_ctx.set_view_height(0)


def test_back_at_one_is_the_plain_frame(oracle, path_scene, path_ctx):
    import torch
    path_ctx.set_supersampling(4)
    path_ctx.render(W0, H0)
    path_ctx.set_supersampling(1)
    assert path_ctx.supersampling == 1
    want, ost = expect(oracle, path_scene, W0, H0, 1)
    path_ctx.reset_stats()
    assert_same(path_ctx.render(W0, H0).copy(), want, "k = 1 after k = 4")
    st = path_ctx.stats()
    assert ray_counts(st) == ray_counts(ost) and st["pixels"] == W0 * H0
    out = torch.zeros(W0 * H0, dtype=torch.int32, device="cuda")
    path_ctx.render_device(W0, H0, out.data_ptr(), _stream())
    torch.cuda.synchronize()
    assert_same(out.cpu().numpy().reshape(H0, W0), want, "k = 1 rt_render_device")
    assert path_ctx.dispatch_order() in (-1, 0, 1, 2, 3)


def test_tiles_and_count_work_unsupported_while_supersampling(path_scene, path_ctx):
    import torch
    lay = wire_layout(W0, H0, 8, 1, 1)
    wire = torch.zeros(int(lay.max_bytes) + 8, dtype=torch.uint8, device="cuda")
    path_ctx.set_supersampling(2)
    with pytest.raises(abi.RayTracerError) as ei:
        path_ctx.render_bands_tiles(W0, H0, 8, 0, 1, 0, 1, 1, wire.data_ptr(), _stream())
    assert ei.value.code == abi.RT_ERR_UNSUPPORTED
    with pytest.raises(abi.RayTracerError) as ei:
        path_ctx.count_work(W0, H0)
    assert ei.value.code == abi.RT_ERR_UNSUPPORTED
    path_ctx.set_supersampling(1)
    path_ctx.render_bands_tiles(W0, H0, 8, 0, 1, 0, 1, 1, wire.data_ptr(), _stream())
    torch.cuda.synchronize()
    assert path_ctx.count_work(W0, H0)["primary_rays"] == W0 * H0


def test_stats_count_output_pixels(path_scene, path_ctx):
    path_ctx.set_supersampling(4)
    path_ctx.reset_stats()
    path_ctx.render(W0, H0)
    path_ctx.render(W0, 8)
    st = path_ctx.stats()
    assert st["frames"] == 2 and st["pixels"] == W0 * H0 + W0 * 8
    assert st["primary_rays"] == 16 * (W0 * H0 + W0 * 8)
    path_ctx.set_supersampling(1)
