"""The grid of trace kernel variants (rt_internal.h TraceVariant), swept deterministically: scene
class (the direct kernel unrolled and generic; the bundle kernel's three shadow passes) x pow (with and without a
general specular exponent) x depth (one limit per stack size) x route (batch, lone frames in every dispatch
order, the measured order and its recording, the diagnostic tallies, the fused tile encoder, supersampling, a
camera path).  Every frame is bit-exact against the oracle and the ray counts equal the oracle's.

Frames of 20 x 12: 3 x 2 tiles with a partial tile in both directions, the smallest frame at which tile indexing,
the lone frame's 4-tile workgroups and their padding can all go wrong.  Each oracle frame is rendered once per
module and shared read-only.
"""

import numpy as np
import pytest

import path_cases
from raytracer_hip import Context, abi, scenes, wire_layout
from raytracer_hip.supersample import box_resolve

pytestmark = pytest.mark.gpu

W, H = 20, 12
LIMITS = [0, 1, 3, 5, 7, 8]  # K = 1, 2, 4, 6, 8 and 64 (the scratch stack)
RAYS = ("primary_rays", "reflect_rays", "shadow_rays")
FIFTH_LIGHT = scenes.Light(scenes.vec(6, 9, -2), scenes.f32(0.6))
ORIGIN_LIGHT = scenes.Light(scenes.vec(0, 0, 0), 1.0)  # 2a = 0: the shadow loops without the exact threshold

# name -> (spheres, planes, lights)
CLASSES = {
    "direct_s8": (8, scenes.REF_PLANES, scenes.REF_LIGHTS),                         # SMAX 8: unrolled pair loops
    "direct_s11": (11, scenes.REF_PLANES, scenes.REF_LIGHTS),                       # SMAX 0
    "bundle_merged2": (12, scenes.C4_PLANES, scenes.C4_LIGHTS[:2]),                 # MERGED 2
    "bundle_merged1": (12, scenes.C4_PLANES, [scenes.C4_LIGHTS[0], ORIGIN_LIGHT]),  # MERGED 1
    "bundle_l5": (12, scenes.C4_PLANES, scenes.C4_LIGHTS + [FIFTH_LIGHT]),          # MERGED 0: a pass per light
}


def scene_of(cls, gpow, limit):
    n, planes, lights = CLASSES[cls]
    sph = scenes.generated_spheres(n)
    if gpow:  # specular exponents 3.7 and 7.25: the Math.Pow instantiations
        sph = [scenes.Sphere(s.center, s.radius, (scenes.Material.metal if i % 2 else scenes.Material.plastic)(
            s.material.kd if any(s.material.kd) else (0.7, 0.6, 0.5), 7.25 if i % 2 else 3.7)) if i % 3 != 2 else s
               for i, s in enumerate(sph)]
    return scenes.Scene(f"{cls}_{'gpow' if gpow else 'pow'}_lim{limit}", W, H, sph, list(planes), list(lights),
                        scenes.REF_AMBIENT, limit)


_EXPECT = {}


def expect(oracle, sc, k=1):
    """(frame [H, W], oracle ray counts) of `sc` at supersampling factor k."""
    key = (sc.name, sc.camera, k)
    if key not in _EXPECT:
        px, st = oracle.render(sc.resized(k * W, k * H), oracle.MODE_NEAREST, 8)
        out = box_resolve(px, k) if k > 1 else px
        out.setflags(write=False)
        _EXPECT[key] = (out, {r: st[r] for r in RAYS})
    return _EXPECT[key]


def assert_same(px, want, what):
    bad = px != want
    if bad.any():
        ys, xs = np.nonzero(bad)
        pytest.fail(f"{what}: {int(bad.sum())} of {bad.size} pixels differ; first at (x={xs[0]}, y={ys[0]}): "
                    f"gpu {px[ys[0], xs[0]]:#08x} expected {want[ys[0], xs[0]]:#08x}")


def rays(ctx):
    st = ctx.stats()
    return {r: st[r] for r in RAYS}


def times(counts, n):
    return {r: n * v for r, v in counts.items()}


@pytest.mark.parametrize("gpow", [False, True], ids=["pow", "gpow"])
@pytest.mark.parametrize("cls", list(CLASSES))
def test_every_depth_and_route(oracle, monkeypatch, cls, gpow):
    import torch
    st = torch.cuda.current_stream().cuda_stream
    ctxs = {}
    try:
        # RT_DISPATCH_ORDER is read when the context is made
        for order in (0, 1, 2):
            monkeypatch.setenv("RT_DISPATCH_ORDER", str(order))
            ctxs[order] = Context(1)
        monkeypatch.delenv("RT_DISPATCH_ORDER")
        ctxs[None] = ctx = Context(1)
        stride = (int(wire_layout(W, H, 8, 1, 1).max_bytes) + 255) // 256 * 256
        for limit in LIMITS:
            sc = scene_of(cls, gpow, limit)
            what = sc.name
            want, cnt = expect(oracle, sc)
            out = torch.zeros(2 * W * H + 64, dtype=torch.int32, device="cuda")

            def frame(f=0):
                torch.cuda.synchronize()
                host = out.cpu().numpy()
                out.zero_()
                return host[f * W * H:(f + 1) * W * H].reshape(H, W)

            # lone frames under each fixed dispatch order (the direct kernel: SINGLE_WPG tiles per workgroup)
            for order in (0, 1, 2):
                c = ctxs[order]
                c.set_scene(sc)
                c.reset_stats()
                c.render_device(W, H, out.data_ptr(), st)
                assert_same(frame(), want, f"{what} lone frame, order {order}")
                assert c.dispatch_order() == order
                assert rays(c) == cnt, f"{what} lone frame, order {order}"

            ctx.set_scene(sc)
            # a batch of two frames: one tile per workgroup
            ctx.reset_stats()
            nb = ctx.render_bands_batch(W, H, H, 0, 1, 2, out.data_ptr(), W * H * 4, abi.RT_BANDS_INT32, st)
            assert nb == 1
            torch.cuda.synchronize()
            host = out.cpu().numpy().copy()
            out.zero_()
            for f in range(2):
                assert_same(host[f * W * H:(f + 1) * W * H].reshape(H, W), want, f"{what} batch frame {f}")
            assert (host[2 * W * H:] == 0).all(), "nothing written past the two frames"
            assert rays(ctx) == times(cnt, 2), f"{what} batch"

            # lone frames while the library measures the orders: well past the tuner's 28 probes, the tile
            # durations' recording and the measured order
            ctx.reset_stats()
            for k in range(60):
                ctx.render_device(W, H, out.data_ptr(), st)
                if k % 10 == 9:
                    assert_same(frame(), want, f"{what} untuned lone frame {k}")
            assert ctx.dispatch_order() in (-1, 0, 1, 2, 3)
            assert rays(ctx) == times(cnt, 60), f"{what} untuned lone frames"

            # the diagnostic tallies
            work = ctx.count_work(W, H)
            assert {r: work[r] for r in RAYS} == cnt, f"{what} count_work"

            # the fused tile encoder, finished and decoded as a world of one
            wire = torch.zeros(stride, dtype=torch.uint8, device="cuda")
            ctx.reset_stats()
            ctx.render_bands_tiles(W, H, 8, 0, 1, 0, 1, 1, wire.data_ptr(), st)
            ctx.finish_wire(W, H, 8, 0, 1, 1, wire.data_ptr(), 0, st)
            ctx.decode_gathered(W, H, 8, 1, wire.data_ptr(), stride, 1, out.data_ptr(), W * H, st)
            assert_same(frame(), want, f"{what} fused tile encoder")
            assert rays(ctx) == cnt, f"{what} fused tile encoder"

            # supersampling: the 40 x 24 sample frame, box-resolved
            want2, cnt2 = expect(oracle, sc, 2)
            ctx.set_supersampling(2)
            try:
                ctx.reset_stats()
                assert_same(ctx.render(W, H).copy(), want2, f"{what} supersampled 2 x 2")
                assert rays(ctx) == cnt2, f"{what} supersampled 2 x 2"
            finally:
                ctx.set_supersampling(1)

            # a camera path of two different cameras
            path = [sc, path_cases.moved(sc, path_cases.OFFSETS[2])]
            ctx.reset_stats()
            px = ctx.render_path([s.c_camera() for s in path], W, H)
            total = {r: 0 for r in RAYS}
            for f, s in enumerate(path):
                wantf, cntf = expect(oracle, s)
                assert_same(px[f], wantf, f"{what} path frame {f}")
                total = {r: total[r] + cntf[r] for r in RAYS}
            assert not np.array_equal(px[0], px[1]), "the two cameras see different frames"
            assert rays(ctx) == total, f"{what} path"
    finally:
        for c in ctxs.values():
            c.close()
