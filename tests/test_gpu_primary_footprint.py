"""The sky-wave skip of the direct kernel (csrc/rt_foot.h): a wave whose 8x8 tile lies outside
every sphere's screen box and whose valid pixels fail every plane's footprint rule traces nothing and stores 0.  The
skip changes no pixel and no ray count: with it on (the default) and off (RT_PRIM_FOOT=0, read by rt_set_scene) every
frame is bit-exact against the oracle and the ray counts are the oracle's -- cameras whose horizon lies on and beside
a tile-row boundary, all-sky and all-floor views, the camera below and on the floor, planes of arbitrary normals (0, 4
and 5 of them, zero and NaN normals), every kernel shape of the direct family, and the camera-path and shutter
launches, which carry no skip.  Frames of 64 x 40, 96 x 64 and 100 x 60: the smallest at which a tile row can be all
sky, all floor or cut by the horizon, with partial tiles at the right and bottom edges.  Each oracle frame is
rendered once per module and shared read-only.
"""
import dataclasses
import math

import numpy as np
import pytest

import adaptive_cases as ac
import path_cases
import random_scenes
from raytracer_hip import Context, abi, path, scenes, wire_layout
from raytracer_hip.scenes import Material, Plane, Scene, Sphere, vec
from raytracer_hip.supersample import box_resolve

pytestmark = pytest.mark.gpu

RAYS = ("primary_rays", "reflect_rays", "shadow_rays")
FOOT = ("1", "0")
SIZES = ((64, 40), (96, 64), (100, 60))
_EXPECT = {}


def f32(x):
    return float(np.float32(x))


def expect(oracle, sc, k=1):
    key = (sc.name, sc.width, sc.height, sc.camera, k)
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


def assert_same(px, want, what):
    bad = px != want
    if bad.any():
        ys, xs = np.nonzero(bad)
        pytest.fail(f"{what}: {int(bad.sum())} of {bad.size} pixels differ; first at (x={xs[0]}, y={ys[0]}): "
                    f"gpu {px[ys[0], xs[0]]:#08x} oracle {want[ys[0], xs[0]]:#08x}")


def _stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


def _c3(name, w, h, cam=None, limit=3, planes=None, spheres=None):
    return Scene(name, w, h, scenes.generated_spheres(8) if spheres is None else spheres,
                 list(scenes.REF_PLANES if planes is None else planes), list(scenes.REF_LIGHTS), scenes.REF_AMBIENT,
                 limit, cam or (scenes.ZERO, 0.0, 0.0))


def horizon_pitch(row, h):
    """The pitch at which the floor's horizon (the camera at the floor's height + 1, any yaw: the camera never rolls)
    falls on frame row `row`: ly = (row / h - 0.5) ph = -near tan(pitch), ph = 2 near tan(30 deg)."""
    return f32(math.atan((0.5 - row / h) * 2.0 * math.tan(math.radians(30.0))))


def _cameras():
    out = {}
    # the horizon on a tile-row boundary and one row either side of it, at each size (boundary rows 16, 24, 32)
    for (w, h), edge, yaw in zip(SIZES, (16, 24, 32), (0.0, f32(0.7), f32(-2.4))):
        for row in (edge - 1, edge, edge + 1):
            out[f"horizon_row{row}_{w}x{h}"] = (w, h, (scenes.ZERO, yaw, horizon_pitch(row, h)))
    out["all_sky_64x40"] = (64, 40, (scenes.ZERO, 0.0, f32(-1.2)))
    out["all_floor_100x60"] = (100, 60, (scenes.ZERO, f32(0.3), f32(1.2)))
    out["below_the_floor_96x64"] = (96, 64, (vec(0, -3, 0), 0.0, f32(-0.2)))
    out["below_the_floor_looking_down_64x40"] = (64, 40, (vec(1, -2.5, 0), f32(0.5), f32(0.4)))
    out["on_the_floor_100x60"] = (100, 60, (vec(0, -1, 0), 0.0, f32(0.1)))
    out["on_the_floor_looking_up_96x64"] = (96, 64, (vec(0, -1, 2), f32(-0.3), f32(-0.3)))
    return out


CAMERAS = _cameras()


def _random_planes(seed, n):
    rng = np.random.default_rng(4000 + seed)
    planes = []
    for _ in range(n):
        v = rng.normal(size=3)
        v = v / np.linalg.norm(v)
        planes.append(Plane(random_scenes._v(rng, -3, 3), tuple(f32(x) for x in v), random_scenes._material(rng)))
    return planes


def _random(seed, w, h, n_planes=None, extra=(), spheres=None, limit=None):
    """tests/random_scenes.py scene `seed` (0-11 spheres: the direct family) with planes of arbitrary normals."""
    sc = random_scenes.random_scene(seed, w, h)
    kw = {}
    if n_planes is not None:
        kw["planes"] = _random_planes(seed, n_planes) + list(extra)
    if spheres is not None:
        kw["spheres"] = spheres
    if limit is not None:
        kw["recursion_limit"] = limit
    return dataclasses.replace(sc, name=f"foot_rand{seed}_{w}x{h}_{n_planes}_{len(extra)}", **kw)


FLOOR = scenes.REF_PLANES[0]
RANDOM = {
    "planes_0": lambda: _random(3, 64, 40, 0),
    "planes_1": lambda: _random(5, 100, 60, 1),
    "planes_2": lambda: _random(54, 96, 64, 2),
    "planes_4": lambda: _random(44, 96, 64, 4),
    "planes_4_b": lambda: _random(29, 100, 60, 4),
    "planes_4_limit32": lambda: _random(42, 64, 40, 4),
    "planes_5_footprints_off": lambda: _random(22, 64, 40, 5),
    "zero_normal": lambda: _random(30, 96, 64, 1, extra=[dataclasses.replace(FLOOR, normal=vec(0, 0, 0))]),
    "nan_normal": lambda: _random(47, 100, 60, 1, extra=[dataclasses.replace(FLOOR, normal=(0.0, float("nan"), 0.0))]),
    "no_spheres": lambda: _random(49, 100, 60, 2, spheres=[]),
    "no_spheres_floor": lambda: _c3("foot_s0", 64, 40, spheres=[]),
    "nothing_at_all": lambda: _random(17, 64, 40, 0, spheres=[]),
    # a mirror sphere that reaches above the horizon: its tiles carry reflections of the floor into the sky rows
    "mirror_above_horizon": lambda: _c3("foot_mirror", 96, 64, spheres=[Sphere(vec(0, 1.5, 6), 2.0, Material.mirror(scenes.ONE)),
                                                                          Sphere(vec(-4, 3, 9), 1.0, Material.mirror(scenes.ONE))]),
}
GPOW_FLOOR = [dataclasses.replace(FLOOR, material=dataclasses.replace(FLOOR.material, n=f32(3.7)))]
SHAPES = {
    "limit0_K1": lambda: _c3("foot_l0", 100, 60, limit=0),
    "limit1_K2": lambda: _c3("foot_l1", 100, 60, limit=1),
    "limit3_K4": lambda: _c3("foot_l3", 100, 60, limit=3),
    "limit7_K8": lambda: _c3("foot_l7", 100, 60, limit=7),
    "limit8_scratch_stack": lambda: _c3("foot_l8", 100, 60, limit=8),
    "gpow": lambda: _c3("foot_gpow", 96, 64, planes=GPOW_FLOOR),
}
SCENES = {**{k: (lambda k=k: _c3(f"foot_{k}", *CAMERAS[k][:2], cam=CAMERAS[k][2])) for k in CAMERAS}, **RANDOM, **SHAPES}


@pytest.fixture(scope="module")
def ctx():
    c = Context(1)
    yield c
    c.close()


@pytest.mark.parametrize("name", list(SCENES))
def test_pixels_and_ray_counts_equal_the_oracle_skip_on_and_off(ctx, oracle, monkeypatch, name):
    sc = SCENES[name]()
    want, cnt = expect(oracle, sc)
    for foot in FOOT:
        monkeypatch.setenv("RT_PRIM_FOOT", foot)
        ctx.set_scene(sc)
        ctx.reset_stats()
        px = ctx.render(sc.width, sc.height).copy()
        assert_same(px, want, f"{sc.name} RT_PRIM_FOOT={foot}")
        assert rays(ctx) == cnt, f"{sc.name} RT_PRIM_FOOT={foot}"
        # a batch of two frames: one tile per workgroup (rt_render of one frame runs the 4-tile workgroups)
        import torch
        W, H = sc.width, sc.height
        out = torch.full((2 * W * H + 64,), -1, dtype=torch.int32, device="cuda")
        ctx.reset_stats()
        assert ctx.render_bands_batch(W, H, H, 0, 1, 2, out.data_ptr(), W * H * 4, abi.RT_BANDS_INT32, _stream()) == 1
        torch.cuda.synchronize()
        host = out.cpu().numpy()
        for f in range(2):
            assert_same(host[f * W * H:(f + 1) * W * H].reshape(H, W), want, f"{sc.name} batch frame {f} RT_PRIM_FOOT={foot}")
        assert (host[2 * W * H:] == -1).all()
        assert rays(ctx) == {r: 2 * v for r, v in cnt.items()}, f"{sc.name} batch RT_PRIM_FOOT={foot}"


def test_the_camera_cases_hold_sky_floor_and_cut_tile_rows(oracle):
    """The preconditions of the camera cases, from the oracle's frames of the floor alone: the rows above the case's
    horizon row are sky and the rows below it floor (the row itself may be either)."""
    for (w, h), edge in zip(SIZES, (16, 24, 32)):
        for row in (edge - 1, edge, edge + 1):
            name = f"horizon_row{row}_{w}x{h}"
            px, _ = expect(oracle, _c3(f"foot_floor_only_{name}", w, h, cam=CAMERAS[name][2], spheres=[]))
            assert (px[:row] == 0).all() and (px[row + 1:] != 0).all(), name
    assert (expect(oracle, SCENES["all_sky_64x40"]())[0] == 0).all()
    assert (expect(oracle, SCENES["all_floor_100x60"]())[0] != 0).all()


@pytest.mark.parametrize("foot", FOOT)
def test_render_bands_of_eight_rows_rank_1_of_3(ctx, oracle, monkeypatch, foot):
    import torch
    sc = SCENES["horizon_row32_100x60"]()
    W, H = sc.width, sc.height
    want, cnt = expect(oracle, sc)
    monkeypatch.setenv("RT_PRIM_FOOT", foot)
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
                        f"rank {r} of 3, band {band}, RT_PRIM_FOOT={foot}")
    assert_same(frame.cpu().numpy().reshape(H, W), want, f"8-row bands, world 3, RT_PRIM_FOOT={foot}")
    assert rays(ctx) == cnt


@pytest.mark.parametrize("foot", FOOT)
def test_fused_tile_encoder(ctx, oracle, monkeypatch, foot):
    import torch
    sc = SCENES["horizon_row24_96x64"]()
    W, H = sc.width, sc.height
    want, cnt = expect(oracle, sc)
    monkeypatch.setenv("RT_PRIM_FOOT", foot)
    ctx.set_scene(sc)
    ctx.reset_stats()
    stride = (int(wire_layout(W, H, 8, 1, 1).max_bytes) + 255) // 256 * 256
    wire = torch.zeros(stride, dtype=torch.uint8, device="cuda")
    out = torch.full((W * H,), -1, dtype=torch.int32, device="cuda")
    st = _stream()
    ctx.render_bands_tiles(W, H, 8, 0, 1, 0, 1, 1, wire.data_ptr(), st)
    ctx.finish_wire(W, H, 8, 0, 1, 1, wire.data_ptr(), 0, st)
    ctx.decode_gathered(W, H, 8, 1, wire.data_ptr(), stride, 1, out.data_ptr(), W * H, st)
    torch.cuda.synchronize()
    assert_same(out.cpu().numpy().reshape(H, W), want, f"fused tile encoder RT_PRIM_FOOT={foot}")
    assert rays(ctx) == cnt


@pytest.mark.parametrize("foot", FOOT)
def test_supersampling_two(oracle, monkeypatch, foot):
    sc = SCENES["horizon_row17_64x40"]()
    want, cnt = expect(oracle, sc, 2)
    monkeypatch.setenv("RT_PRIM_FOOT", foot)
    with Context(1) as c:
        c.set_scene(sc)
        c.set_supersampling(2)
        c.reset_stats()
        px = c.render(sc.width, sc.height).copy()
        got = rays(c)
    assert_same(px, want, f"k=2 RT_PRIM_FOOT={foot}")
    assert got == cnt, "the ray counts are the oracle's at 2 W x 2 H"


@pytest.mark.parametrize("foot", FOOT)
def test_adaptive_supersampling_two(oracle, monkeypatch, foot):
    from test_gpu_adaptive import expected_counts
    cid, W, H, k, T = "C3", 100, 60, 2, 96
    want = ac.expect(oracle, cid, W, H, k, T)
    counts = expected_counts(oracle, cid, W, H, k, T)
    plain = ac.frames(oracle, cid, W, H, 1)[0]
    refined = ac.pixel_mask(plain, T)
    assert refined.any() and not refined.all() and (plain[:8] == 0).all(), "refined, flat and sky tiles"
    monkeypatch.setenv("RT_PRIM_FOOT", foot)
    with Context(1) as c:
        c.set_scene(ac.scene(cid))
        c.set_supersampling(k)
        c.set_adaptive_sampling(T)
        c.reset_stats()
        px = c.render(W, H).copy()
        got = rays(c)
    assert_same(px, want, f"adaptive k=2 RT_PRIM_FOOT={foot}")
    assert got == counts, "the ray counts are the oracle's over the traced samples"


@pytest.mark.parametrize("foot", FOOT)
def test_lone_frame_workgroups_with_a_measured_tile_order(oracle, monkeypatch, foot):
    import torch
    sc = SCENES["horizon_row31_100x60"]()
    W, H = sc.width, sc.height
    want, cnt = expect(oracle, sc)
    monkeypatch.setenv("RT_PRIM_FOOT", foot)
    monkeypatch.setenv("RT_DISPATCH_ORDER", "3")  # read when the context is made
    with Context(1) as c:
        c.set_scene(sc)
        assert c.dispatch_order() == 3
        out = torch.full((H * W + 64,), -1, dtype=torch.int32, device="cuda")
        for k in range(3):  # the first launch records the tiles' durations, the later ones run the sorted order
            out.fill_(-1)
            c.reset_stats()
            c.render_device(W, H, out.data_ptr(), _stream())
            torch.cuda.synchronize()
            host = out.cpu().numpy()
            assert_same(host[:H * W].reshape(H, W), want, f"lone frame {k} RT_PRIM_FOOT={foot}")
            assert (host[H * W:] == -1).all()
            assert rays(c) == cnt


@pytest.mark.parametrize("foot", FOOT)
def test_camera_path_and_shutter_launches_are_unchanged(ctx, oracle, monkeypatch, foot):
    import torch
    sc = _c3("foot_path", 96, 64)
    W, H = sc.width, sc.height
    frames, stats = path_cases.oracle_frames(oracle, sc)
    cams = path_cases.cameras(sc)
    monkeypatch.setenv("RT_PRIM_FOOT", foot)
    ctx.set_scene(sc)
    ctx.reset_stats()
    out = torch.full((len(cams) * W * H,), -1, dtype=torch.int32, device="cuda")
    ctx.render_path_bands(W, H, cams, H, 0, 1, out.data_ptr(), W * H * 4, abi.RT_BANDS_INT32, _stream())
    torch.cuda.synchronize()
    host = out.cpu().numpy().reshape(len(cams), H, W)
    for f in range(len(cams)):
        assert_same(host[f], frames[f], f"path frame {f} RT_PRIM_FOOT={foot}")
    assert rays(ctx) == {r: sum(st[r] for st in stats) for r in RAYS}
    ctx.reset_stats()
    px = ctx.render_shutter(cams, W, H, 2)
    want = path.shutter_mean(frames, 2)
    for f in range(len(cams) // 2):
        assert_same(px[f], want[f], f"shutter 2 frame {f} RT_PRIM_FOOT={foot}")
    assert rays(ctx) == {r: sum(st[r] for st in stats) for r in RAYS}


def test_count_work_matches_the_oracle_and_the_skip_runs_fewer_plane_tests(ctx, oracle, monkeypatch):
    sc = scenes.config("C3").resized(160, 90)
    want, cnt = expect(oracle, sc)
    work = {}
    for foot in FOOT:
        monkeypatch.setenv("RT_PRIM_FOOT", foot)
        ctx.set_scene(sc)
        work[foot] = ctx.count_work(sc.width, sc.height)
        assert {r: work[foot][r] for r in RAYS} == cnt, f"rt_count_work RT_PRIM_FOOT={foot}"
    print("plane_tests_run: skip on", work["1"]["plane_tests_run"], "off", work["0"]["plane_tests_run"])
    assert work["1"]["plane_tests_run"] < work["0"]["plane_tests_run"]
    for key in ("primary_rays", "reflect_rays", "shadow_rays", "sphere_tests", "plane_tests"):
        assert work["1"][key] == work["0"][key], f"nominal count {key} unchanged"


def test_the_skip_stops_on_a_view_without_sky(ctx, oracle, monkeypatch):
    sc = SCENES["all_floor_100x60"]()
    want, cnt = expect(oracle, sc)
    work = {}
    for foot in FOOT:
        monkeypatch.setenv("RT_PRIM_FOOT", foot)
        ctx.set_scene(sc)
        work[foot] = ctx.count_work(sc.width, sc.height)
        assert {r: work[foot][r] for r in RAYS} == cnt
    assert work["1"]["plane_tests_run"] == work["0"]["plane_tests_run"]
