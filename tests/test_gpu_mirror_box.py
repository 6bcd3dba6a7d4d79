"""Mirrored screen boxes of the direct kernel (S < 12 spheres, limit >= 1): the first reflected segment off a boxed
mirror plane tests only the spheres whose mirrored box (rt_view.h mirror_boxes, LaunchParams::mbox) meets the
wave's pixels.  Culling only: with the boxes on (the default) and off (RT_MIRROR_BOX=0, read by rt_set_scene) every
frame and every ray count equals the oracle's.  Frames of at most 160 x 96; each oracle frame is rendered once per
module and shared read-only.
"""
import numpy as np
import pytest

from raytracer_hip import Context, scenes
from raytracer_hip.scenes import Light, Material, Plane, Scene, Sphere, vec
from raytracer_hip.supersample import box_resolve

pytestmark = pytest.mark.gpu

_EXPECT = {}


def expect(oracle, sc, k=1):
    key = (sc.name, sc.width, sc.height, k)
    if key not in _EXPECT:
        px, st = oracle.render(sc.resized(k * sc.width, k * sc.height) if k > 1 else sc, oracle.MODE_NEAREST, 8)
        if k > 1:
            px = box_resolve(px, k)
        px.setflags(write=False)
        _EXPECT[key] = (px, st)
    return _EXPECT[key]


def ray_counts(st):
    return {k: st[k] for k in ("primary_rays", "reflect_rays", "shadow_rays")}


def assert_same(px, want, what):
    bad = px != want
    if bad.any():
        ys, xs = np.nonzero(bad)
        pytest.fail(f"{what}: {int(bad.sum())} of {bad.size} pixels differ; first at (x={xs[0]}, y={ys[0]}): "
                    f"gpu {px[ys[0], xs[0]]:#08x} oracle {want[ys[0], xs[0]]:#08x}")


FLOOR_MAT = scenes.REF_PLANES[0].material  # diffuse, specular and mirror: every floor pixel reflects
MIRROR = Material.mirror(scenes.ONE)
HALF = Material.diffuse_mirror(vec(0.8, 0.7, 0.3), vec(0.5, 0.5, 0.5))


def _unit(x, y, z, s=1.0):
    v = np.array([x, y, z], dtype=np.float64)
    v = v / np.linalg.norm(v) * s
    return tuple(float(np.float32(c)) for c in v)


def _scene(name, planes, w=96, h=64, limit=3, cam=(scenes.ZERO, 0.0, 0.0), spheres=None):
    return Scene(name, w, h, list(spheres if spheres is not None else scenes.generated_spheres(8)), planes,
                 list(scenes.REF_LIGHTS), scenes.REF_AMBIENT, limit, cam)


def _random(seed):
    import random_scenes
    sc = random_scenes.random_scene(seed)
    assert len(sc.spheres) < 12
    return sc


SCENES = {
    "C3_160x90": lambda: scenes.config("C3").resized(160, 90),
    "tilted": lambda: _scene("tilted", [Plane(vec(0, -1, 0), _unit(0.2, 1.0, -0.1), FLOOR_MAT)]),
    "two_mirror_planes": lambda: _scene("two", [Plane(vec(0, -1, 0), vec(0, 1, 0), FLOOR_MAT),
                                                Plane(vec(0, 0, 40), _unit(0.3, 0.0, -1.0), MIRROR)]),
    # the third mirror plane has no table: its lanes take every sphere
    "three_mirror_planes": lambda: _scene("three", [Plane(vec(0, -1, 0), vec(0, 1, 0), FLOOR_MAT),
                                                    Plane(vec(-9, 0, 0), _unit(1.0, 0.0, 0.1), MIRROR),
                                                    Plane(vec(9, 0, 0), _unit(-1.0, 0.1, 0.0), HALF)], limit=2),
    # |n.n - 1| far above 2^-20: no table (the reference's "reflection" about it is no mirror image)
    "non_unit_normal": lambda: _scene("nonunit", [Plane(vec(0, -1, 0), _unit(0.0, 1.0, 0.0, 1.25), FLOOR_MAT)]),
    # ... and just inside the gate (2^-22 off unit length)
    "near_unit_normal": lambda: _scene("nearunit", [Plane(vec(0, -1, 0), (0.0, float(np.float32(1.0 + 2.0 ** -22)), 0.0),
                                                          FLOOR_MAT)]),
    "camera_below_plane": lambda: _scene("below", [Plane(vec(0, 1.5, 0), vec(0, 1, 0), FLOOR_MAT)],
                                         cam=(vec(0, -0.5, 0), 0.0, -0.3)),
    # pitch up a little: the horizon and the rows under it (t beyond t_max: the full test) are in the frame
    "horizon": lambda: _scene("horizon", [Plane(vec(0, -1, 0), vec(0, 1, 0), FLOOR_MAT)], w=64, h=96,
                              cam=(scenes.ZERO, 0.1, -0.2)),
    "sphere_cut_by_plane": lambda: _scene("cut", [Plane(vec(0, -1, 0), vec(0, 1, 0), FLOOR_MAT)],
                                          spheres=scenes.generated_spheres(8) + [
                                              Sphere(vec(0.5, -1.2, 6), 0.8, HALF), Sphere(vec(-1.5, -1.0, 4), 0.5, MIRROR),
                                              Sphere(vec(1.0, -2.5, 7), 1.0, Material.diffuse(vec(0, 0, 1)))]),
    "ragged_frame": lambda: _scene("ragged", [Plane(vec(0, -1, 0), vec(0, 1, 0), FLOOR_MAT)], w=93, h=61),
    "limit0": lambda: _scene("limit0", [Plane(vec(0, -1, 0), vec(0, 1, 0), FLOOR_MAT)], limit=0),
    "limit1": lambda: _scene("limit1", [Plane(vec(0, -1, 0), vec(0, 1, 0), FLOOR_MAT)], limit=1),
    "limit3_near_camera": lambda: _scene("near", [Plane(vec(0, -0.02, 0), vec(0, 1, 0), FLOOR_MAT)], limit=3),
}
SCENES.update({f"rand{seed}": (lambda seed=seed: _random(seed)) for seed in range(0, 40, 2)})


@pytest.fixture(scope="module")
def ctx():
    c = Context(1)
    yield c
    c.close()


@pytest.mark.parametrize("name", list(SCENES))
def test_pixels_and_ray_counts_equal_the_oracle_boxes_on_and_off(ctx, oracle, monkeypatch, name):
    sc = SCENES[name]()
    want, ost = expect(oracle, sc)
    for box in ("1", "0"):
        monkeypatch.setenv("RT_MIRROR_BOX", box)
        ctx.set_scene(sc)
        ctx.reset_stats()
        px = ctx.render(sc.width, sc.height).copy()
        assert_same(px, want, f"{sc.name} RT_MIRROR_BOX={box}")
        assert ray_counts(ctx.stats()) == ray_counts(ost), f"{sc.name} RT_MIRROR_BOX={box}"


def _stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


@pytest.mark.parametrize("box", ["1", "0"])
def test_render_bands_of_eight_rows_world_two(ctx, oracle, monkeypatch, box):
    import torch
    sc = SCENES["C3_160x90"]()
    W, H = sc.width, sc.height
    want, ost = expect(oracle, sc)
    monkeypatch.setenv("RT_MIRROR_BOX", box)
    ctx.set_scene(sc)
    ctx.reset_stats()
    frame = torch.full((H * W,), -1, dtype=torch.int32, device="cuda")
    for r in range(2):
        n_bands = len(range(r, -(-H // 8), 2))
        bands = torch.full((n_bands * 8 * W,), -1, dtype=torch.int32, device="cuda")
        assert ctx.render_bands(W, H, 8, r, 2, bands.data_ptr(), _stream()) == n_bands
        ctx.scatter_bands(W, H, 8, r, 2, bands.data_ptr(), frame.data_ptr(), _stream())
    torch.cuda.synchronize()
    assert_same(frame.cpu().numpy().reshape(H, W), want, f"8-row bands, world 2, RT_MIRROR_BOX={box}")
    assert ray_counts(ctx.stats()) == ray_counts(ost)


@pytest.mark.parametrize("box", ["1", "0"])
def test_render_device_lone_frame_workgroups(ctx, oracle, monkeypatch, box):
    import torch
    sc = SCENES["C3_160x90"]()
    W, H = sc.width, sc.height
    want, ost = expect(oracle, sc)
    monkeypatch.setenv("RT_MIRROR_BOX", box)
    ctx.set_scene(sc)
    ctx.reset_stats()
    out = torch.full((H * W + 64,), -1, dtype=torch.int32, device="cuda")
    ctx.render_device(W, H, out.data_ptr(), _stream())
    torch.cuda.synchronize()
    host = out.cpu().numpy()
    assert_same(host[:H * W].reshape(H, W), want, f"rt_render_device RT_MIRROR_BOX={box}")
    assert (host[H * W:] == -1).all()
    assert ray_counts(ctx.stats()) == ray_counts(ost)


@pytest.mark.parametrize("box", ["1", "0"])
def test_supersampling_two(oracle, monkeypatch, box):
    sc = scenes.config("C3").resized(80, 45)
    want, ost = expect(oracle, sc, 2)
    monkeypatch.setenv("RT_MIRROR_BOX", box)
    with Context(1) as c:
        c.set_scene(sc)
        c.set_supersampling(2)
        c.reset_stats()
        px = c.render(sc.width, sc.height).copy()
        st = c.stats()
    assert_same(px, want, f"k=2 RT_MIRROR_BOX={box}")
    assert ray_counts(st) == ray_counts(ost), "the ray counts are the oracle's at 2 W x 2 H"


def test_boxes_skip_sphere_tests_on_c3(ctx, monkeypatch):
    sc = SCENES["C3_160x90"]()
    work = {}
    for box in ("1", "0"):
        monkeypatch.setenv("RT_MIRROR_BOX", box)
        ctx.set_scene(sc)
        work[box] = ctx.count_work(sc.width, sc.height)
    print("sphere_tests_run: boxes on", work["1"]["sphere_tests_run"], "off", work["0"]["sphere_tests_run"])
    assert work["1"]["sphere_tests_run"] < work["0"]["sphere_tests_run"]
    for key in ("primary_rays", "reflect_rays", "shadow_rays", "sphere_tests", "plane_tests"):
        if key in work["1"]:
            assert work["1"][key] == work["0"][key], f"nominal count {key} unchanged"
