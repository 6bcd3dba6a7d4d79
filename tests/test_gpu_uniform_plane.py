"""Plane-uniform waves of the direct kernel (csrc/rt_kernel.hip trace_tile_direct): a wave whose level-0
records all lie on one plane shades them converged, with the plane's material and geometry read through a
wave-uniform index.  Only where the operands come from changes, so with the path on (the default) and off
(RT_UNIFORM_PLANE=0, read by rt_set_scene) every frame is bit-exact against the oracle and the three ray counts are the
oracle's: the classification's edges (one tile, partial tiles, the horizon, the camera on and below the plane,
silhouettes, a seam between two planes, no plane), every plane material the shader branches on, every stack depth, the
light cases of the shadow scan, every launch route, and a far and a NaN camera.  Frames of at most 160 x 90; each
oracle frame is rendered once per module and shared read-only.
"""
import dataclasses

import numpy as np
import pytest

import adaptive_cases as ac
from raytracer_hip import Context, abi, path, scenes, tilecodec as tc, wire_layout
from raytracer_hip.scenes import Light, Material, Plane, Scene, vec
from raytracer_hip.supersample import box_resolve, progressive_order, progressive_resolve

pytestmark = pytest.mark.gpu

RAYS = ("primary_rays", "reflect_rays", "shadow_rays")
UNIFORM = ("1", "0")
_EXPECT = {}


def f32(x):
    return float(np.float32(x))


def expect(oracle, sc, k=1):
    """(pixels, ray counts) of `sc` (k > 1: the box mean of its k W x k H frame, and that frame's counts)."""
    key = (sc.name, sc.width, sc.height, repr(sc.camera), k)
    if key not in _EXPECT:
        px, st = oracle.render(sc.resized(k * sc.width, k * sc.height) if k > 1 else sc, oracle.MODE_NEAREST, 8)
        if k > 1:
            px = box_resolve(px, k)
        px.setflags(write=False)
        _EXPECT[key] = (px, {r: st[r] for r in RAYS})
    return _EXPECT[key]


def rays(ctx):
    st = ctx.stats()
    return {r: st[r] for r in RAYS}


def add(a, b):
    return {r: a[r] + b[r] for r in RAYS}


def assert_same(px, want, what):
    bad = px != want
    if bad.any():
        ys, xs = np.nonzero(bad)
        pytest.fail(f"{what}: {int(bad.sum())} of {bad.size} pixels differ; first at (x={xs[0]}, y={ys[0]}): "
                    f"gpu {px[ys[0], xs[0]]:#08x} oracle {want[ys[0], xs[0]]:#08x}")


def _stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


FLOOR = scenes.REF_PLANES[0]
FLOOR_MAT = FLOOR.material  # diffuse, specular (n = 0.5) and mirror
WALL = scenes.C4_PLANES[1]  # z = 48, diffuse only
DOWN = (scenes.ZERO, f32(0.3), f32(1.2))  # pitched down: the floor in every pixel, no sphere in view
ORIGIN_LIGHT = Light(vec(0, 0, 0), 1.0)  # 2a = 0: the shadow_scan<false> side


def _floor(**kw):
    return dataclasses.replace(FLOOR, **kw)


def _floor_mat(**kw):
    return _floor(material=dataclasses.replace(FLOOR_MAT, **kw))


def _c3(name, w=96, h=54, planes=None, lights=None, limit=3, cam=None, n_spheres=8):
    return Scene(f"up_{name}", w, h, scenes.generated_spheres(n_spheres), list(scenes.REF_PLANES if planes is None else planes),
                 list(lights or scenes.REF_LIGHTS), scenes.REF_AMBIENT, limit, cam or (scenes.ZERO, 0.0, 0.0))


EDGES = {
    "one_floor_tile_8x8": lambda: _c3("tile", 8, 8, cam=DOWN),
    "frame_1x1": lambda: _c3("1x1", 1, 1, cam=DOWN),
    "frame_8x1": lambda: _c3("8x1", 8, 1, cam=DOWN),
    "frame_13x11": lambda: _c3("13x11", 13, 11, cam=DOWN),
    # the horizon at row 27 of 54 cuts tile row 3: floor lanes and miss lanes in one wave; sphere silhouettes cut others
    "horizon_and_silhouettes": lambda: _c3("horizon"),
    "horizon_no_spheres": lambda: _c3("horizon_s0", n_spheres=0),
    # t - 0.01 <= 0 on the steep rays of a camera 0.005 above the floor, on every ray of one 0.001 above it
    "camera_0.005_above_the_floor": lambda: _c3("near005", cam=(vec(0, -0.995, 0), 0.0, f32(0.4))),
    "camera_0.001_above_the_floor": lambda: _c3("near001", 40, 24, cam=(vec(0, -0.999, 0), 0.0, f32(1.2))),
    "camera_below_the_floor": lambda: _c3("below", cam=(vec(0, -3, 0), 0.0, f32(-0.2))),
    # P = 2: the floor-wall seam runs through a tile row, and each plane is the uniform one elsewhere (index 1 too)
    "floor_and_wall": lambda: _c3("wall", planes=scenes.C4_PLANES, cam=(vec(0, 0, 30), 0.0, f32(0.1))),
    "wall_and_floor": lambda: _c3("wall_first", planes=[WALL, FLOOR], cam=(vec(0, 0, 30), 0.0, f32(0.1))),
    "wall_and_floor_11_spheres": lambda: _c3("wall11", 100, 60, planes=[WALL, FLOOR], n_spheres=11),
    "no_planes": lambda: _c3("p0", planes=[]),
}
MATERIALS = {
    "diffuse_only": lambda: _c3("m_d", planes=[_floor(material=Material.diffuse(vec(0.8, 0.7, 0.6)))]),
    "mirror_only": lambda: _c3("m_m", planes=[_floor(material=Material.mirror(scenes.ONE))]),
    "diffuse_mirror_no_specular": lambda: _c3("m_dm", planes=[_floor(material=Material.diffuse_mirror(vec(0.8, 0.7, 0.6), vec(0.5, 0.5, 0.5)))]),
    "specular_n_0.5": lambda: _c3("m_n05"),
    "specular_n_1": lambda: _c3("m_n1", planes=[_floor_mat(n=1.0)]),
    "specular_n_2": lambda: _c3("m_n2", planes=[_floor_mat(n=2.0)]),
    "specular_n_3.7_gpow": lambda: _c3("m_n37", planes=[_floor_mat(n=f32(3.7))]),
    "km_not_one": lambda: _c3("m_km", planes=[_floor_mat(km=(0.5, 0.25, 0.75))]),
    # floors for which the dark guard refuses (tests/test_gpu_dark_tiles.py REFUSED)
    "dark_refused_normal_scaled_1.01": lambda: _c3("m_n101", planes=[_floor(normal=vec(0, 1.01, 0))]),
    "dark_refused_light_on_the_floor": lambda: _c3("m_onfloor", lights=[scenes.REF_LIGHTS[0], Light(vec(-2, -1, 7), 1.0)]),
    "dark_refused_kd_nan": lambda: _c3("m_kdnan", planes=[_floor_mat(kd=(1.0, float("nan"), 1.0))]),
}
DEPTHS = {f"limit_{n}": (lambda n=n: _c3(f"l{n}", 100, 60, limit=n)) for n in (0, 1, 3, 7, 8, 12)}
LIGHTS = {
    "one_light": lambda: _c3("li1", lights=scenes.REF_LIGHTS[:1]),
    "two_lights": lambda: _c3("li2", 100, 60),
    "light_at_the_origin": lambda: _c3("li0", lights=[scenes.REF_LIGHTS[0], ORIGIN_LIGHT]),
}
UNUSUAL = {
    "camera_1e6_above_the_floor": lambda: _c3("far", 40, 24, cam=(vec(0, 1e6, 0), 0.0, f32(1.2))),
    "camera_x_nan": lambda: _c3("nan", 40, 24, cam=((float("nan"), 0.0, 0.0), 0.0, f32(0.3))),
    "camera_y_nan": lambda: _c3("nan_y", 40, 24, cam=((0.0, float("nan"), 0.0), 0.0, f32(0.3))),
}
SCENES = {**EDGES, **MATERIALS, **DEPTHS, **LIGHTS, **UNUSUAL}
# the routes: the C3 scene at the golden size and on a ragged frame (13 x 8 tiles, partial at the right and bottom)
ROUTE = {"C3_96x54": lambda: scenes.config("C3").resized(96, 54), "C3_100x60": lambda: scenes.config("C3").resized(100, 60)}


@pytest.fixture(scope="module")
def ctx():
    c = Context(1)
    yield c
    c.close()


@pytest.mark.parametrize("name", list(SCENES))
def test_pixels_and_ray_counts_equal_the_oracle_path_on_and_off(ctx, oracle, monkeypatch, name):
    import torch
    sc = SCENES[name]()
    W, H = sc.width, sc.height
    want, cnt = expect(oracle, sc)
    for uni in UNIFORM:
        monkeypatch.setenv("RT_UNIFORM_PLANE", uni)
        ctx.set_scene(sc)
        ctx.reset_stats()
        px = ctx.render(W, H).copy()  # a lone frame: the workgroups of 4 tiles
        assert_same(px, want, f"{sc.name} RT_UNIFORM_PLANE={uni}")
        assert rays(ctx) == cnt, f"{sc.name} RT_UNIFORM_PLANE={uni}"
        out = torch.full((2 * W * H + 64,), -1, dtype=torch.int32, device="cuda")
        ctx.reset_stats()  # a batch of two frames: one tile per workgroup
        assert ctx.render_bands_batch(W, H, H, 0, 1, 2, out.data_ptr(), W * H * 4, abi.RT_BANDS_INT32, _stream()) == 1
        torch.cuda.synchronize()
        host = out.cpu().numpy()
        for f in range(2):
            assert_same(host[f * W * H:(f + 1) * W * H].reshape(H, W), want, f"{sc.name} batch frame {f} RT_UNIFORM_PLANE={uni}")
        assert (host[2 * W * H:] == -1).all()
        assert rays(ctx) == {r: 2 * v for r, v in cnt.items()}, f"{sc.name} batch RT_UNIFORM_PLANE={uni}"


def test_the_cases_hold_what_they_are_named_for(oracle):
    """Preconditions, from the oracle's frames: the floor-only views hit in every pixel, the horizon cuts a tile row,
    the near cameras lose records, the wall scenes show both planes as whole tiles, P = 0 shows sky."""
    for name in ("one_floor_tile_8x8", "frame_1x1", "frame_8x1", "frame_13x11"):
        px, cnt = expect(oracle, SCENES[name]())
        assert (px != 0).all() and cnt["shadow_rays"] > 0, name
    px, _ = expect(oracle, SCENES["horizon_no_spheres"]())
    assert (px[:27] == 0).all() and (px[28:] != 0).all() and 27 % 8 != 0
    full = expect(oracle, _c3("near_ref", cam=(vec(0, -0.9, 0), 0.0, f32(0.4))))[1]
    some = expect(oracle, SCENES["camera_0.005_above_the_floor"]())[1]
    assert 0 < some["shadow_rays"] < full["shadow_rays"], "some lanes are within 0.01 of the plane, some are not"
    assert expect(oracle, SCENES["camera_0.001_above_the_floor"]())[1]["shadow_rays"] == 0
    for name in ("floor_and_wall", "wall_and_floor"):
        sc = SCENES[name]()
        both, _ = expect(oracle, sc)
        only_floor, _ = expect(oracle, dataclasses.replace(sc, name=sc.name + "_floor", planes=[FLOOR]))
        wall_rows = np.nonzero((both != only_floor).any(axis=1))[0]
        assert len(wall_rows) >= 16, "the wall fills whole tiles above the seam"
        assert (wall_rows.max() + 1) % 8 != 0, "the seam cuts a tile row"
    assert (expect(oracle, SCENES["no_planes"]())[0] == 0).any()


@pytest.mark.parametrize("uni", UNIFORM)
@pytest.mark.parametrize("size", list(ROUTE))
def test_render_device_of_a_lone_frame_in_tile_order(oracle, monkeypatch, size, uni):
    import torch
    sc = ROUTE[size]()
    W, H = sc.width, sc.height
    want, cnt = expect(oracle, sc)
    monkeypatch.setenv("RT_UNIFORM_PLANE", uni)
    monkeypatch.setenv("RT_DISPATCH_ORDER", "3")  # read when the context is made
    with Context(1) as c:
        c.set_scene(sc)
        out = torch.full((H * W + 64,), -1, dtype=torch.int32, device="cuda")
        for k in range(3):  # the first launch records the tiles' durations, the later ones run the sorted order
            out.fill_(-1)
            c.reset_stats()
            c.render_device(W, H, out.data_ptr(), _stream())
            torch.cuda.synchronize()
            host = out.cpu().numpy()
            assert_same(host[:H * W].reshape(H, W), want, f"lone frame {k} RT_UNIFORM_PLANE={uni}")
            assert (host[H * W:] == -1).all()
            assert rays(c) == cnt


@pytest.mark.parametrize("uni", UNIFORM)
@pytest.mark.parametrize("size", list(ROUTE))
def test_render_bands_batch_of_three_frames(ctx, oracle, monkeypatch, size, uni):
    import torch
    sc = ROUTE[size]()
    W, H = sc.width, sc.height
    want, cnt = expect(oracle, sc)
    monkeypatch.setenv("RT_UNIFORM_PLANE", uni)
    ctx.set_scene(sc)
    ctx.reset_stats()
    out = torch.full((3 * W * H + 64,), -1, dtype=torch.int32, device="cuda")
    assert ctx.render_bands_batch(W, H, H, 0, 1, 3, out.data_ptr(), W * H * 4, abi.RT_BANDS_INT32, _stream()) == 1
    torch.cuda.synchronize()
    host = out.cpu().numpy()
    for f in range(3):
        assert_same(host[f * W * H:(f + 1) * W * H].reshape(H, W), want, f"batch frame {f} RT_UNIFORM_PLANE={uni}")
    assert (host[3 * W * H:] == -1).all()
    assert rays(ctx) == {r: 3 * v for r, v in cnt.items()}


@pytest.mark.parametrize("uni", UNIFORM)
@pytest.mark.parametrize("size", list(ROUTE))
def test_render_bands_of_eight_rows_interleaved_over_three_ranks(ctx, oracle, monkeypatch, size, uni):
    import torch
    sc = ROUTE[size]()
    W, H = sc.width, sc.height
    want, cnt = expect(oracle, sc)
    monkeypatch.setenv("RT_UNIFORM_PLANE", uni)
    ctx.set_scene(sc)
    ctx.reset_stats()
    frame = torch.full((H * W,), -1, dtype=torch.int32, device="cuda")
    for r in (1, 0, 2):
        n_bands = len(range(r, -(-H // 8), 3))
        bands = torch.full((n_bands * 8 * W + 64,), -1, dtype=torch.int32, device="cuda")
        assert ctx.render_bands(W, H, 8, r, 3, bands.data_ptr(), _stream()) == n_bands
        ctx.scatter_bands(W, H, 8, r, 3, bands.data_ptr(), frame.data_ptr(), _stream())
        torch.cuda.synchronize()
        host = bands.cpu().numpy()
        assert (host[n_bands * 8 * W:] == -1).all()
        for k, band in enumerate(range(r, -(-H // 8), 3)):
            rows = min(8, H - band * 8)
            assert_same(host[k * 8 * W:(k * 8 + rows) * W].reshape(rows, W), want[band * 8:band * 8 + rows],
                        f"rank {r} of 3, band {band}, RT_UNIFORM_PLANE={uni}")
    assert_same(frame.cpu().numpy().reshape(H, W), want, f"8-row bands, world 3, RT_UNIFORM_PLANE={uni}")
    assert rays(ctx) == cnt


@pytest.mark.parametrize("uni", UNIFORM)
@pytest.mark.parametrize("size", list(ROUTE))
def test_fused_tile_encoder_wire_equals_the_host_mirror(ctx, oracle, monkeypatch, size, uni):
    import torch
    sc = ROUTE[size]()
    W, H = sc.width, sc.height
    want, cnt = expect(oracle, sc)
    monkeypatch.setenv("RT_UNIFORM_PLANE", uni)
    ctx.set_scene(sc)
    ctx.reset_stats()
    # (world 1: the band set is the frame, its last band padded to 8 rows that the encoder ignores)
    mirror = tc.encode(np.pad(want, ((0, -H % 8), (0, 0))).reshape(-1), W, H, 8, 0, 1, 1)
    stride = (int(wire_layout(W, H, 8, 1, 1).max_bytes) + 255) // 256 * 256
    wire = torch.full((stride,), 0xA5, dtype=torch.uint8, device="cuda")
    size_t = torch.zeros(1, dtype=torch.int64, device="cuda")
    out = torch.full((W * H,), -1, dtype=torch.int32, device="cuda")
    st = _stream()
    ctx.render_bands_tiles(W, H, 8, 0, 1, 0, 1, 1, wire.data_ptr(), st)
    ctx.finish_wire(W, H, 8, 0, 1, 1, wire.data_ptr(), size_t.data_ptr(), st)
    ctx.decode_gathered(W, H, 8, 1, wire.data_ptr(), stride, 1, out.data_ptr(), W * H, st)
    torch.cuda.synchronize()
    assert int(size_t.item()) == len(mirror)
    assert wire[:len(mirror)].cpu().numpy().tobytes() == mirror, f"fused wire differs from the host mirror RT_UNIFORM_PLANE={uni}"
    assert_same(out.cpu().numpy().reshape(H, W), want, f"fused tile encoder RT_UNIFORM_PLANE={uni}")
    assert rays(ctx) == cnt


@pytest.mark.parametrize("uni", UNIFORM)
@pytest.mark.parametrize("size", list(ROUTE))
def test_supersampling_two(oracle, monkeypatch, size, uni):
    sc = ROUTE[size]()
    want, cnt = expect(oracle, sc, 2)
    monkeypatch.setenv("RT_UNIFORM_PLANE", uni)
    with Context(1) as c:
        c.set_scene(sc)
        c.set_supersampling(2)
        c.reset_stats()
        px = c.render(sc.width, sc.height).copy()
        got = rays(c)
    assert_same(px, want, f"k=2 RT_UNIFORM_PLANE={uni}")
    assert got == cnt, "the ray counts are the oracle's at 2 W x 2 H"


def _sample_counts(oracle, big_scene):
    """Per sample of the frame: [primary, reflect, shadow] ray counts, from the oracle's segments."""
    key = ("segments", big_scene.name, big_scene.width, big_scene.height)
    if key not in _EXPECT:
        _, cnt = expect(oracle, big_scene)
        seg = oracle.segments(big_scene, 1)
        n = big_scene.width * big_scene.height
        per = [np.bincount(seg["pixel"][seg["kind"] == kind], minlength=n).reshape(big_scene.height, big_scene.width)
               for kind in (0, 1, 2)]
        assert [int(p.sum()) for p in per] == [cnt[r] for r in RAYS], "the per-sample segments add up to the oracle's counts"
        _EXPECT[key] = per
    return _EXPECT[key]


@pytest.mark.parametrize("uni", UNIFORM)
@pytest.mark.parametrize("size", list(ROUTE))
def test_adaptive_supersampling_two(oracle, monkeypatch, size, uni):
    sc = ROUTE[size]()
    W, H, k, T = sc.width, sc.height, 2, 96
    want = ac.expect(oracle, "C3", W, H, k, T)
    plain = ac.frames(oracle, "C3", W, H, 1)[0]
    refined = ac.pixel_mask(plain, T)
    assert refined.any() and not refined.all(), "refined and flat tiles"
    traced = ac.traced_samples(plain, k, T)
    per = _sample_counts(oracle, sc.resized(k * W, k * H))
    counts = {r: int(p[traced].sum()) for r, p in zip(RAYS, per)}
    monkeypatch.setenv("RT_UNIFORM_PLANE", uni)
    with Context(1) as c:
        c.set_scene(sc)
        c.set_supersampling(k)
        c.set_adaptive_sampling(T)
        c.reset_stats()
        px = c.render(W, H).copy()
        got = rays(c)
    assert_same(px, want, f"adaptive k=2 RT_UNIFORM_PLANE={uni}")
    assert got == counts, "the ray counts are the oracle's over the traced samples"


@pytest.mark.parametrize("uni", UNIFORM)
@pytest.mark.parametrize("size", list(ROUTE))
def test_progressive_two_ticks(oracle, monkeypatch, size, uni):
    sc = ROUTE[size]()
    W, H, k = sc.width, sc.height, 2
    big_scene = sc.resized(k * W, k * H)
    big, _ = expect(oracle, big_scene)
    plain, plain_cnt = expect(oracle, sc)
    per = _sample_counts(oracle, big_scene)
    # Tick 1 is the plain launch; Tick 2 starts the accumulator with the run's first two samples
    two = {r: int(sum(p[j::k, i::k].sum() for i, j in progressive_order(k)[:2])) for r, p in zip(RAYS, per)}
    monkeypatch.setenv("RT_UNIFORM_PLANE", uni)
    with Context(1) as c:
        c.set_scene(sc)
        c.set_progressive(k)
        c.reset_stats()
        assert_same(c.render(W, H).copy(), progressive_resolve(big, k, 1), f"Tick 1 RT_UNIFORM_PLANE={uni}")
        assert rays(c) == plain_cnt
        assert_same(c.render(W, H).copy(), progressive_resolve(big, k, 2), f"Tick 2 RT_UNIFORM_PLANE={uni}")
        assert c.progressive() == (k, 2)
        assert rays(c) == add(plain_cnt, two)
    assert_same(progressive_resolve(big, k, 1), plain, "P_1 is the plain frame")


@pytest.mark.parametrize("uni", UNIFORM)
@pytest.mark.parametrize("size", list(ROUTE))
def test_camera_path_and_shutter_of_two_cameras_one_of_them_floor_only(ctx, oracle, monkeypatch, size, uni):
    import torch
    sc = ROUTE[size]()
    W, H = sc.width, sc.height
    views = [sc, dataclasses.replace(sc, camera=DOWN)]
    frames, cnts = zip(*(expect(oracle, v) for v in views))
    assert (frames[1] != 0).all(), "the second camera sees only the floor"
    total = add(cnts[0], cnts[1])
    cams = [v.c_camera() for v in views]
    monkeypatch.setenv("RT_UNIFORM_PLANE", uni)
    ctx.set_scene(sc)
    ctx.reset_stats()
    out = torch.full((2 * W * H,), -1, dtype=torch.int32, device="cuda")
    ctx.render_path_bands(W, H, cams, H, 0, 1, out.data_ptr(), W * H * 4, abi.RT_BANDS_INT32, _stream())
    torch.cuda.synchronize()
    host = out.cpu().numpy().reshape(2, H, W)
    for f in range(2):
        assert_same(host[f], frames[f], f"path frame {f} RT_UNIFORM_PLANE={uni}")
    assert rays(ctx) == total
    ctx.reset_stats()
    px = ctx.render_shutter(cams, W, H, 2)
    assert_same(px[0], path.shutter_mean(np.stack(frames), 2)[0], f"shutter 2 RT_UNIFORM_PLANE={uni}")
    assert rays(ctx) == total


@pytest.mark.parametrize("size", list(ROUTE))
def test_count_work_matches_the_oracle_path_on_and_off(ctx, oracle, monkeypatch, size):
    sc = ROUTE[size]()
    _, cnt = expect(oracle, sc)
    work = {}
    for uni in UNIFORM:
        monkeypatch.setenv("RT_UNIFORM_PLANE", uni)
        ctx.set_scene(sc)
        work[uni] = ctx.count_work(sc.width, sc.height)
        assert {r: work[uni][r] for r in RAYS} == cnt, f"rt_count_work RT_UNIFORM_PLANE={uni}"
    for key in ("sphere_tests", "plane_tests", "plane_tests_run", "shadow_rays_run"):
        assert work["1"][key] == work["0"][key], f"{key} does not depend on the path"
