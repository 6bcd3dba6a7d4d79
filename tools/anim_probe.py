"""What does a scene per frame cost a batch launch, and what does it replace?

    python tools/anim_probe.py [--repeats 7] [--out profiles/ab/anim.txt]

64-frame launches of whole frames (FRAME format), counters off (rt_set_counting(0)), C3 at 1920x1080 and C4 at
3840x2160, the legs of one build in one process, alternating, each after a warm-up:
    (a) path       rt_render_path_bands with 64 copies of the scene's camera (the PATH kernels, the context's scene);
        anim-same  rt_render_anim_bands with the same cameras over a track whose 64 frames are all that scene: the same
                   rays, every scene table read at its pointer + z * scene_stride -- the cost of the indirection alone;
    (b) anim-move  the same over a track that really moves (anim.tween: half the spheres and one light): other rays
                   than (a), so its time says what such an animation costs, not what the mechanism costs;
    (c) rt_set_scene_track per frame on the host (build on the thread pool, upload, the synchronisation in front);
    (d) what the feature replaces: a loop of rt_set_scene + rt_render_device per frame, wall time per frame.
(a) and (b) with 8 launches queued per synchronisation -- the host side of a call runs under the launches already
queued: the device's rate -- and with one in flight.  The yardstick of (a) is path's own run-to-run spread (max - min
of its repeats).  No threshold: exit status 0 whenever the legs ran.
"""
import argparse
import dataclasses
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "uu-infogr-raytracer_amd"))

BATCH = 64
SHAPES = (("C3", 1920, 1080), ("C4", 3840, 2160))


def timed(torch, fn, depth, min_s=0.3):
    """us per frame of back-to-back launches, `depth` queued per synchronisation, over >= min_s and >= 3 rounds."""
    n, t0 = 0, time.perf_counter()
    while True:
        for _ in range(depth):
            fn()
        torch.cuda.synchronize()
        n += depth
        dt = time.perf_counter() - t0
        if dt >= min_s and n >= 3 * depth:
            return dt / (n * BATCH) * 1e6


def warm(torch, fn, seconds=0.08):
    t0 = time.perf_counter()
    while time.perf_counter() - t0 < seconds:
        fn()
        torch.cuda.synchronize()


def moving(sc, scenes):
    """A second key for anim.tween: half the spheres and light 0 moved."""
    sph = [scenes.Sphere(scenes.vec(s.center[0] + (1.5 if i % 4 else -2.0), s.center[1] + 0.25 * (i % 3), s.center[2] - 1.0),
                         s.radius, s.material) if i % 2 else s for i, s in enumerate(sc.spheres)]
    l0 = sc.lights[0]
    lights = [scenes.Light(scenes.vec(l0.position[0] + 4, l0.position[1] + 1, l0.position[2] - 3), l0.intensity)] + list(sc.lights[1:])
    return dataclasses.replace(sc, spheres=sph, lights=lights)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert a.repeats >= 5
    import torch
    from raytracer_hip import Context, abi, anim, path, scenes
    torch.cuda.set_device(0)
    st = torch.cuda.current_stream().cuda_stream
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    say(f"anim_probe: {BATCH}-frame launches of whole frames (FRAME), counting off, {a.repeats} alternating repeats; "
        f"us per frame, median (min .. max)")
    for cid, W, H in SHAPES:
        sc = scenes.config(cid).resized(W, H)
        cams = path.as_array([sc.c_camera()] * BATCH)
        same = [sc] * BATCH
        move = anim.tween([sc, moving(sc, scenes)], BATCH - 1)
        assert len(move) == BATCH
        out = torch.empty(BATCH * W * H, dtype=torch.int32, device="cuda")
        with Context(1) as ctx:
            ctx.set_scene(sc)
            ctx.set_timing(0)
            ctx.set_counting(False)
            run_path = lambda: ctx.render_path_bands(W, H, cams, H, 0, 1, out.data_ptr(), W * H * 4, abi.RT_BANDS_FRAME, st)
            run_anim = lambda: ctx.render_anim_bands(W, H, cams, H, 0, 1, out.data_ptr(), W * H * 4, abi.RT_BANDS_FRAME, st)
            for depth, label in ((8, "8 launches queued per synchronisation (the device's rate)"), (1, "one launch in flight")):
                t = {"path": [], "anim-same": [], "anim-move": []}
                for _ in range(a.repeats):
                    warm(torch, run_path)
                    t["path"].append(timed(torch, run_path, depth))
                    for k, track in (("anim-same", same), ("anim-move", move)):
                        ctx.set_scene_track(track)
                        warm(torch, run_anim)
                        t[k].append(timed(torch, run_anim, depth))
                med = {k: statistics.median(v) for k, v in t.items()}
                spread = max(t["path"]) - min(t["path"])
                say(f"{cid} {W}x{H}, {label}:")
                for k in t:
                    say(f"    {k:10s} {med[k]:9.2f}  ({min(t[k]):.2f} .. {max(t[k]):.2f})   / path {med[k] / med['path']:.4f}")
                d = med["anim-same"] - med["path"]
                say(f"    (a) anim-same - path = {d:+.2f} us per frame; path's own spread {spread:.2f}: "
                    f"{'inside' if abs(d) <= spread else 'OUTSIDE'} it")
            # (c) the host side of a track
            for k, track in (("same", same), ("move", move)):
                ts = []
                args = anim.c_track(track)  # (the Python marshalling is not the library's cost)
                for _ in range(a.repeats):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    abi.check(ctx.lib, ctx.lib.rt_set_scene_track(ctx.ptr, *args), ctx.ptr)
                    ts.append((time.perf_counter() - t0) / BATCH * 1e6)
                say(f"{cid} (c) rt_set_scene_track ({k}, {BATCH} frames): {statistics.median(ts):.1f} us per frame "
                    f"({min(ts):.1f} .. {max(ts):.1f})")
            # (d) the loop the feature replaces
            ts = []
            one = [(sc_f.c_arrays(), abi.rt_vec3(*sc_f.ambient)) for sc_f in move]  # (marshalled ahead, as in (c))
            for _ in range(a.repeats):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for f in range(BATCH):
                    (S, P, L), amb = one[f]
                    abi.check(ctx.lib, ctx.lib.rt_set_scene(ctx.ptr, S, len(sc.spheres), P, len(sc.planes), L, len(sc.lights), amb,
                                                            sc.recursion_limit), ctx.ptr)
                    ctx.render_device(W, H, out.data_ptr() + f * W * H * 4, st)
                torch.cuda.synchronize()
                ts.append((time.perf_counter() - t0) / BATCH * 1e6)
            say(f"{cid} (d) set_scene + render_device per frame, wall: {statistics.median(ts):.1f} us per frame "
                f"({min(ts):.1f} .. {max(ts):.1f})")
        del out
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
