"""The shadow pre-test's group and union records in plane-uniform waves (csrc/rt_kernel.hip shadow_scan's GROUPS,
csrc/rt_scene.h build_shadow_groups): a wave whose lanes keep no group of a sphere pair skips the
pair's per-lane pre-tests.  Only pre-tests that would have dropped their sphere are skipped, so with the records on (the
default) and off (RT_SHADOW_GROUPS=0, read by rt_set_scene) every frame is bit-exact against the oracle, the three ray
counts are the oracle's, and the executed exact tests (rt_count_work's sphere_tests and plane_tests) are the same either
way.  Frames of at most 160 x 90; each oracle frame is rendered once per module and shared read-only.
"""
import dataclasses

import numpy as np
import pytest

from raytracer_hip import Context, abi, scenes
from raytracer_hip.scenes import Light, Material, Scene, Sphere, vec
from raytracer_hip.supersample import box_resolve

pytestmark = pytest.mark.gpu

RAYS = ("primary_rays", "reflect_rays", "shadow_rays")
GROUPS = ("1", "0")
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
DOWN = (scenes.ZERO, f32(0.3), f32(0.9))  # pitched down: the floor in every tile
MATTE = Material.diffuse(vec(0.9, 0.2, 0.2))


def _scene(name, w=96, h=54, spheres=8, planes=None, lights=None, limit=3, cam=None):
    sph = scenes.generated_spheres(spheres) if isinstance(spheres, int) else list(spheres)
    return Scene(f"sg_{name}", w, h, sph, list(scenes.REF_PLANES if planes is None else planes),
                 list(scenes.REF_LIGHTS if lights is None else lights), scenes.REF_AMBIENT, limit, cam or (scenes.ZERO, 0.0, 0.0))


def _balls(xs, r=0.75):
    return [Sphere(vec(x, r - 1.0, 9.0), r, MATTE) for x in xs]


SCENES = {
    # the C3 scene: every tile floor, and the horizon with the sphere silhouettes in one tile row
    "c3_pitched_down": lambda: _scene("down", cam=DOWN),
    "c3_level": lambda: _scene("level"),
    **{f"spheres_{n}": (lambda n=n: _scene(f"s{n}", 80, 48, spheres=n, cam=(scenes.ZERO, 0.0, f32(0.3)))) for n in (0, 1, 2, 3, 11)},
    "lights_1": lambda: _scene("l1", lights=scenes.REF_LIGHTS[:1], cam=(scenes.ZERO, 0.0, f32(0.3))),
    "lights_4": lambda: _scene("l4", lights=scenes.C4_LIGHTS, cam=(scenes.ZERO, 0.0, f32(0.3))),
    # 2a = 0: the scan without pre-test (shadow_scan<false>); the other light scans with the records
    "light_at_the_origin": lambda: _scene("l0", lights=[scenes.REF_LIGHTS[0], Light(vec(0, 0, 0), 1.0)], cam=DOWN),
    # a = p.p = 2^42 is outside [2^-40, 2^40]: every record of that light, its groups and its union are +inf
    "light_with_inf_records": lambda: _scene("linf", lights=[Light(vec(2.0 ** 21, 2.0 ** 19, 0), 1.0), scenes.REF_LIGHTS[1]], cam=DOWN),
    # hit points with |O|_1 >= 2^38: the lane margin is +inf and every record is kept
    # (x and z swallow the view plane's offsets: the rays below the horizon point straight down and hit at (1e12, -1, 1e12))
    "camera_at_x_z_1e12": lambda: _scene("far", 40, 24, cam=(vec(1e12, 0, 1e12), 0.0, f32(0.4))),
    "camera_x_nan": lambda: _scene("nan", 40, 24, cam=((float("nan"), 0.0, 0.0), 0.0, f32(0.3))),
    # two spheres 12 apart, a group each: the floor between their shadows lies inside the union, outside both groups
    "inside_the_union_outside_the_groups": lambda: _scene("two", spheres=_balls((-6.0, 6.0)), cam=(scenes.ZERO, 0.0, f32(0.35))),
    # three pairs of spheres, a group per pair: the floor between a pair's shadows lies inside its group, outside both members
    "inside_a_group_outside_its_members": lambda: _scene("pairs", spheres=_balls((-7.0, -4.5, -1.25, 1.25, 4.5, 7.0)),
                                                         cam=(scenes.ZERO, 0.0, f32(0.35))),
    **{f"limit_{n}": (lambda n=n: _scene(f"k{n}", 80, 48, limit=n, cam=(scenes.ZERO, 0.0, f32(0.2)))) for n in (0, 1, 3, 8)},
    # n = 3.7 needs the f64 pow: the kernels without plane-uniform waves, the flat loop
    "gpow_floor": lambda: _scene("gpow", planes=[dataclasses.replace(FLOOR, material=dataclasses.replace(FLOOR.material, n=f32(3.7)))],
                                 cam=(scenes.ZERO, 0.0, f32(0.3))),
}


@pytest.fixture(scope="module")
def ctx():
    c = Context(1)
    yield c
    c.close()


@pytest.mark.parametrize("name", list(SCENES))
def test_pixels_ray_counts_and_exact_tests_with_the_records_on_and_off(ctx, oracle, monkeypatch, name):
    sc = SCENES[name]()
    W, H = sc.width, sc.height
    want, cnt = expect(oracle, sc)
    work = {}
    for sw in GROUPS:
        monkeypatch.setenv("RT_SHADOW_GROUPS", sw)
        ctx.set_scene(sc)
        ctx.reset_stats()
        px = ctx.render(W, H).copy()  # a lone frame: the workgroups of 4 tiles
        assert_same(px, want, f"{sc.name} RT_SHADOW_GROUPS={sw}")
        assert rays(ctx) == cnt, f"{sc.name} RT_SHADOW_GROUPS={sw}"
        work[sw] = ctx.count_work(W, H)
        assert {r: work[sw][r] for r in RAYS} == cnt, f"rt_count_work RT_SHADOW_GROUPS={sw}"
    for key in ("sphere_tests", "plane_tests"):
        assert work["1"][key] == work["0"][key], f"{key} does not depend on the records"


def test_the_cases_hold_what_they_are_named_for(oracle):
    """Preconditions, from the oracle's frames: the pitched view is floor in every pixel with shadows on it, the level
    one has sky, and the spheres of the two geometric scenes cast separate shadows on a lit floor."""
    px, cnt = expect(oracle, SCENES["c3_pitched_down"]())
    assert (px != 0).all() and cnt["shadow_rays"] > 0
    assert (expect(oracle, SCENES["c3_level"]())[0] == 0).any()
    assert expect(oracle, SCENES["camera_at_x_z_1e12"]())[1]["shadow_rays"] > 0, "the far camera's rays hit the floor"
    for name in ("inside_the_union_outside_the_groups", "inside_a_group_outside_its_members"):
        sc = SCENES[name]()
        with_s, _ = expect(oracle, sc)
        without, _ = expect(oracle, dataclasses.replace(sc, name=sc.name + "_empty", spheres=[]))
        changed = (with_s != without).any(axis=0)  # columns the spheres or their shadows touch
        runs = int((np.diff(changed.astype(np.int8)) == 1).sum()) + int(changed[0])
        assert runs >= 2 and not changed.all(), f"{name}: separate spheres with untouched floor between them"


@pytest.mark.parametrize("sw", GROUPS)
def test_render_bands_batch_of_three_frames(ctx, oracle, monkeypatch, sw):
    import torch
    sc = scenes.config("C3").resized(100, 60)  # 13 x 8 tiles, partial at the right and bottom
    W, H = sc.width, sc.height
    want, cnt = expect(oracle, sc)
    monkeypatch.setenv("RT_SHADOW_GROUPS", sw)
    ctx.set_scene(sc)
    ctx.reset_stats()
    out = torch.full((3 * W * H + 64,), -1, dtype=torch.int32, device="cuda")
    assert ctx.render_bands_batch(W, H, H, 0, 1, 3, out.data_ptr(), W * H * 4, abi.RT_BANDS_INT32, _stream()) == 1
    torch.cuda.synchronize()
    host = out.cpu().numpy()
    for f in range(3):
        assert_same(host[f * W * H:(f + 1) * W * H].reshape(H, W), want, f"batch frame {f} RT_SHADOW_GROUPS={sw}")
    assert (host[3 * W * H:] == -1).all()
    assert rays(ctx) == {r: 3 * v for r, v in cnt.items()}


@pytest.mark.parametrize("sw", GROUPS)
def test_render_device(oracle, monkeypatch, sw):
    import torch
    sc = scenes.config("C3").resized(100, 60)
    W, H = sc.width, sc.height
    want, cnt = expect(oracle, sc)
    monkeypatch.setenv("RT_SHADOW_GROUPS", sw)
    with Context(1) as c:
        c.set_scene(sc)
        out = torch.full((H * W + 64,), -1, dtype=torch.int32, device="cuda")
        c.reset_stats()
        c.render_device(W, H, out.data_ptr(), _stream())
        torch.cuda.synchronize()
        host = out.cpu().numpy()
        assert_same(host[:H * W].reshape(H, W), want, f"rt_render_device RT_SHADOW_GROUPS={sw}")
        assert (host[H * W:] == -1).all()
        assert rays(c) == cnt


@pytest.mark.parametrize("sw", GROUPS)
def test_supersampling_two(oracle, monkeypatch, sw):
    sc = scenes.config("C3").resized(80, 45)
    want, cnt = expect(oracle, sc, 2)
    monkeypatch.setenv("RT_SHADOW_GROUPS", sw)
    with Context(1) as c:
        c.set_scene(sc)
        c.set_supersampling(2)
        c.reset_stats()
        px = c.render(sc.width, sc.height).copy()
        got = rays(c)
    assert_same(px, want, f"k=2 RT_SHADOW_GROUPS={sw}")
    assert got == cnt, "the ray counts are the oracle's at 2 W x 2 H"


@pytest.mark.parametrize("sw", GROUPS)
def test_camera_path_of_two_cameras_one_of_them_floor_only(ctx, oracle, monkeypatch, sw):
    import torch
    sc = scenes.config("C3").resized(96, 54)
    W, H = sc.width, sc.height
    views = [sc, dataclasses.replace(sc, camera=DOWN)]
    frames, cnts = zip(*(expect(oracle, v) for v in views))
    cams = [v.c_camera() for v in views]
    monkeypatch.setenv("RT_SHADOW_GROUPS", sw)
    ctx.set_scene(sc)
    ctx.reset_stats()
    out = torch.full((2 * W * H,), -1, dtype=torch.int32, device="cuda")
    ctx.render_path_bands(W, H, cams, H, 0, 1, out.data_ptr(), W * H * 4, abi.RT_BANDS_INT32, _stream())
    torch.cuda.synchronize()
    host = out.cpu().numpy().reshape(2, H, W)
    for f in range(2):
        assert_same(host[f], frames[f], f"path frame {f} RT_SHADOW_GROUPS={sw}")
    assert rays(ctx) == {r: cnts[0][r] + cnts[1][r] for r in RAYS}
