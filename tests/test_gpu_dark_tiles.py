"""The dark-tile skip (rt_dark.h): at a plane hit on a dark checkerboard square whose light
terms are provably +0 both trace kernels skip the light loop -- Phong and the shadow scans.  The skip changes no
pixel and no nominal ray count: with it on (the default) and off (RT_DARK_SKIP=0, read by rt_set_scene) every frame
is bit-exact against the oracle and the ray counts are the oracle's, through every kernel family and route, and in
scenes where the guard must refuse (the flag clear, or the lane part failing).  Frames of at most 160 x 90; each
oracle frame is rendered once per module and shared read-only.
"""
import dataclasses

import numpy as np
import pytest

import path_cases
from raytracer_hip import Context, abi, scenes, wire_layout
from raytracer_hip.scenes import Light, Material, Plane, Scene, vec
from raytracer_hip.supersample import box_resolve

pytestmark = pytest.mark.gpu

RAYS = ("primary_rays", "reflect_rays", "shadow_rays")
_EXPECT = {}


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


FLOOR = scenes.REF_PLANES[0]
FLOOR_MAT = FLOOR.material  # diffuse, specular (n = 0.5) and mirror


def _floor(**kw):
    return dataclasses.replace(FLOOR, **kw)


def _floor_mat(**kw):
    return _floor(material=dataclasses.replace(FLOOR_MAT, **kw))


def _c3(name, w=96, h=54, planes=None, lights=None, limit=3, cam=None, n_spheres=8):
    return Scene(name, w, h, scenes.generated_spheres(n_spheres), list(planes or scenes.REF_PLANES),
                 list(lights or scenes.REF_LIGHTS), scenes.REF_AMBIENT, limit, cam or (scenes.ZERO, 0.0, 0.0))


def _bundle(name, lights, planes=None):
    return _c3(name, planes=planes or scenes.C4_PLANES, lights=lights, n_spheres=12)


FIFTH_LIGHT = Light(vec(6, 9, -2), scenes.f32(0.6))
ORIGIN_LIGHT = Light(vec(0, 0, 0), 1.0)  # 2a = 0: the bundle kernel's MERGED 1
GPOW_FLOOR = [_floor_mat(n=scenes.f32(3.7))]

PARITY = {
    # the golden sizes
    "C1_64x64": lambda: scenes.config("C1").resized(64, 64),
    "C2_96x54": lambda: scenes.config("C2").resized(96, 54),
    "C3_96x54": lambda: scenes.config("C3").resized(96, 54),
    "C4_64x36": lambda: scenes.config("C4").resized(64, 36),
    # K = 1, 2 and 4 of the direct kernel, a ragged frame of 13 x 8 tiles
    "C3_100x60_limit0": lambda: _c3("c3_l0", 100, 60, limit=0),
    "C3_100x60_limit1": lambda: _c3("c3_l1", 100, 60, limit=1),
    "C3_100x60_limit3": lambda: _c3("c3_l3", 100, 60, limit=3),
    # a general exponent on the floor: the _gpow kernels, direct and bundle
    "C3_gpow_floor": lambda: _c3("c3_gpow", planes=GPOW_FLOOR),
    "bundle_gpow_floor": lambda: _bundle("bundle_gpow", scenes.C4_LIGHTS[:2], GPOW_FLOOR + scenes.C4_PLANES[1:]),
    # 12 spheres: the merged shadow pass (MERGED 2 and 1) and the pass per light (5 lights, MERGED 0)
    "bundle_1_light": lambda: _bundle("bundle_l1", scenes.C4_LIGHTS[:1]),
    "bundle_origin_light": lambda: _bundle("bundle_origin", [scenes.C4_LIGHTS[0], ORIGIN_LIGHT]),
    "bundle_5_lights": lambda: _bundle("bundle_l5", scenes.C4_LIGHTS + [FIFTH_LIGHT]),
    # a light whose 2a = 2 p.p overflows
    "light_2a_infinite": lambda: _c3("a2inf", lights=[scenes.REF_LIGHTS[0], Light(vec(3e19, 1, 1), 1.0)]),
    "bundle_light_2a_infinite": lambda: _bundle("bundle_a2inf", [scenes.C4_LIGHTS[0], Light(vec(3e19, 1, 1), 1.0)]),
}

# The flag must be clear or the lane guard must fail; the floor's checkerboard has u = -z, v = -x, so
# (0.5, -1, 4.5) lies in a dark square in front of the camera.
REFUSED = {
    "light_on_the_floor": lambda: _c3("on_floor", lights=[scenes.REF_LIGHTS[0], Light(vec(-2, -1, 7), 1.0)]),
    "light_at_a_dark_hit_point": lambda: _c3("at_hit", lights=[Light(vec(0.5, -1, 4.5), 1.0), scenes.REF_LIGHTS[1]]),
    "normal_scaled_1.01": lambda: _c3("n101", planes=[_floor(normal=vec(0, 1.01, 0))]),
    "intensity_3e38": lambda: _c3("i3e38", lights=[scenes.REF_LIGHTS[0], Light(vec(33, 1, 10), scenes.f32(3e38))]),
    "kd_nan": lambda: _c3("kdnan", planes=[_floor_mat(kd=(1.0, float("nan"), 1.0))]),
    "camera_1e5_above_the_floor": lambda: _c3("far", planes=[_floor(center=vec(0, -1e5, 0))],
                                              cam=(scenes.ZERO, 0.0, 0.5)),
    # Q11: cross(n, (1, 0, 0)) = 0 normalises to NaN, (int)NaN + (int)NaN is even -- tile 0 on the whole plane
    "plane_normal_x": lambda: _c3("nx", planes=list(scenes.REF_PLANES) + [Plane(vec(-6, 0, 0), vec(1, 0, 0), FLOOR_MAT)]),
    "bundle_light_on_the_floor": lambda: _bundle("bundle_on_floor", [scenes.C4_LIGHTS[0], Light(vec(-2, -1, 7), 1.0)]),
}
SCENES = {**PARITY, **REFUSED}

SKIP = ("1", "0")


@pytest.fixture(scope="module")
def ctx():
    c = Context(1)
    yield c
    c.close()


def _stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


@pytest.mark.parametrize("name", list(SCENES))
def test_pixels_and_ray_counts_equal_the_oracle_skip_on_and_off(ctx, oracle, monkeypatch, name):
    sc = SCENES[name]()
    want, cnt = expect(oracle, sc)
    for skip in SKIP:
        monkeypatch.setenv("RT_DARK_SKIP", skip)
        ctx.set_scene(sc)
        ctx.reset_stats()
        px = ctx.render(sc.width, sc.height).copy()
        assert_same(px, want, f"{sc.name} RT_DARK_SKIP={skip}")
        assert rays(ctx) == cnt, f"{sc.name} RT_DARK_SKIP={skip}"


@pytest.mark.parametrize("skip", SKIP)
def test_render_bands_batch_of_three_frames(ctx, oracle, monkeypatch, skip):
    import torch
    sc = SCENES["C3_96x54"]()
    W, H = sc.width, sc.height
    want, cnt = expect(oracle, sc)
    monkeypatch.setenv("RT_DARK_SKIP", skip)
    ctx.set_scene(sc)
    ctx.reset_stats()
    out = torch.full((3 * W * H + 64,), -1, dtype=torch.int32, device="cuda")
    assert ctx.render_bands_batch(W, H, H, 0, 1, 3, out.data_ptr(), W * H * 4, abi.RT_BANDS_INT32, _stream()) == 1
    torch.cuda.synchronize()
    host = out.cpu().numpy()
    for f in range(3):
        assert_same(host[f * W * H:(f + 1) * W * H].reshape(H, W), want, f"batch frame {f} RT_DARK_SKIP={skip}")
    assert (host[3 * W * H:] == -1).all()
    assert rays(ctx) == {r: 3 * v for r, v in cnt.items()}


@pytest.mark.parametrize("skip", SKIP)
def test_render_path_bands_of_three_cameras(ctx, oracle, monkeypatch, skip):
    import torch
    sc = SCENES["C3_96x54"]()
    W, H = sc.width, sc.height
    path = [path_cases.moved(sc, path_cases.OFFSETS[i]) for i in (0, 2, 4)]
    monkeypatch.setenv("RT_DARK_SKIP", skip)
    ctx.set_scene(sc)
    ctx.reset_stats()
    out = torch.full((3 * W * H,), -1, dtype=torch.int32, device="cuda")
    ctx.render_path_bands(W, H, [s.c_camera() for s in path], H, 0, 1, out.data_ptr(), W * H * 4, abi.RT_BANDS_INT32,
                          _stream())
    torch.cuda.synchronize()
    host = out.cpu().numpy()
    total = {r: 0 for r in RAYS}
    for f, s in enumerate(path):
        want, cnt = expect(oracle, s)
        assert_same(host[f * W * H:(f + 1) * W * H].reshape(H, W), want, f"path frame {f} RT_DARK_SKIP={skip}")
        total = {r: total[r] + cnt[r] for r in RAYS}
    assert rays(ctx) == total


@pytest.mark.parametrize("skip", SKIP)
def test_supersampling_two(oracle, monkeypatch, skip):
    sc = scenes.config("C3").resized(80, 45)
    want, cnt = expect(oracle, sc, 2)
    monkeypatch.setenv("RT_DARK_SKIP", skip)
    with Context(1) as c:
        c.set_scene(sc)
        c.set_supersampling(2)
        c.reset_stats()
        px = c.render(sc.width, sc.height).copy()
        got = rays(c)
    assert_same(px, want, f"k=2 RT_DARK_SKIP={skip}")
    assert got == cnt, "the ray counts are the oracle's at 2 W x 2 H"


@pytest.mark.parametrize("skip", SKIP)
def test_fused_tile_encoder(ctx, oracle, monkeypatch, skip):
    import torch
    sc = SCENES["C3_96x54"]()
    W, H = sc.width, sc.height
    want, cnt = expect(oracle, sc)
    monkeypatch.setenv("RT_DARK_SKIP", skip)
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
    assert_same(out.cpu().numpy().reshape(H, W), want, f"fused tile encoder RT_DARK_SKIP={skip}")
    assert rays(ctx) == cnt


def test_skip_runs_fewer_shadow_rays_on_c3(ctx, monkeypatch):
    sc = scenes.config("C3").resized(160, 90)
    work = {}
    for skip in SKIP:
        monkeypatch.setenv("RT_DARK_SKIP", skip)
        ctx.set_scene(sc)
        work[skip] = ctx.count_work(sc.width, sc.height)
    print("shadow_rays_run: skip on", work["1"]["shadow_rays_run"], "off", work["0"]["shadow_rays_run"])
    assert work["1"]["shadow_rays_run"] < work["0"]["shadow_rays_run"]
    for key in ("primary_rays", "reflect_rays", "shadow_rays", "sphere_tests", "plane_tests"):
        assert work["1"][key] == work["0"][key], f"nominal count {key} unchanged"
