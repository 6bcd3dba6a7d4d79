"""What does a scene per sub-frame cost a shutter launch, and what does the call replace?

    python tools/anim_shutter_probe.py [--repeats 5] [--host-frames 16] [--out profiles/ab/anim_shutter.txt]

64-output-frame launches of whole frames (FRAME format), counters off (rt_set_counting(0)), C3 at 1920x1080 and C4 at
3840x2160, the legs of one build in one process, alternating, each after a warm-up launch; us per traced sub-frame:
    (a) anim            rt_render_anim_bands over 64 frames of a track whose frames are all the scene (the ANIM kernels);
        shutter m       rt_render_shutter_bands, m copies of the scene's camera per output frame (SHUTTER, the context's scene);
        anim-shutter m  rt_render_anim_shutter_bands with the same cameras over a track of 64 m copies of the scene: the
                        same rays as both, every scene table read at its pointer + rec * scene_stride -- what the
                        indirection by the sub-frame's record costs a SHUTTER sub-frame, and a sub-frame against an ANIM
                        frame (which also stores its pixels); m = 2 and 8;
        anim-shutter-move m   the same over a track that really moves (anim.tween: other rays, so its time says what
                        such an animation costs, not what the mechanism costs);
    (b) at rt_set_path_supersampling(2), m = 2: anim-ss (ANIM_SS), shutter-ss (SHUTTER_SS), anim-shutter-ss
        (ANIM_SHUTTER_SS), us per sub-frame of k^2 samples per pixel;
    (c) rt_render_anim_shutter into registered host memory at m = 8 against the loop it replaces: rt_render_anim of 8 x
        the frames into registered host memory plus path.shutter_mean on the host (per output frame, so that numpy's
        int64 copy stays one frame's size); wall time per output frame, --host-frames output frames (8 x as many
        sub-frames are pinned for the loop: 64 frames of 4K would pin 17 GB).
The yardstick of (a) and (b) is the spread (max - min) of the twin leg's repeats.  No threshold: exit status 0 whenever
the legs ran.
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


def timed(torch, fn, sub_frames, min_s=0.25):
    """us per sub-frame of back-to-back launches, one in flight, over >= min_s."""
    n, t0 = 0, time.perf_counter()
    while True:
        fn()
        torch.cuda.synchronize()
        n += 1
        dt = time.perf_counter() - t0
        if dt >= min_s:
            return dt / (n * sub_frames) * 1e6


def moving(sc, scenes):
    """A second key for anim.tween: half the spheres and light 0 moved (tools/anim_probe.py's)."""
    sph = [scenes.Sphere(scenes.vec(s.center[0] + (1.5 if i % 4 else -2.0), s.center[1] + 0.25 * (i % 3), s.center[2] - 1.0),
                         s.radius, s.material) if i % 2 else s for i, s in enumerate(sc.spheres)]
    l0 = sc.lights[0]
    lights = [scenes.Light(scenes.vec(l0.position[0] + 4, l0.position[1] + 1, l0.position[2] - 3), l0.intensity)] + list(sc.lights[1:])
    return dataclasses.replace(sc, spheres=sph, lights=lights)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--host-frames", type=int, default=16)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert a.repeats >= 3
    import numpy as np
    import torch
    from raytracer_hip import Context, abi, anim, path, scenes
    torch.cuda.set_device(0)
    st = torch.cuda.current_stream().cuda_stream
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    def row(name, v, per=None):
        med = statistics.median(v)
        tail = "" if per is None else f"   / {per[0]} {med / statistics.median(per[1]):.4f} (its spread {max(per[1]) - min(per[1]):.2f})"
        say(f"    {name:24s} {med:9.2f}  ({min(v):.2f} .. {max(v):.2f}){tail}")

    say(f"anim_shutter_probe: {BATCH}-output-frame launches of whole frames (FRAME), counting off, one launch in flight, "
        f"{a.repeats} alternating repeats; us per sub-frame, median (min .. max)")
    for cid, W, H in SHAPES:
        sc = scenes.config(cid).resized(W, H)
        out = torch.empty(BATCH * W * H, dtype=torch.int32, device="cuda")
        fb = W * H * 4
        with Context(1) as ctx:
            ctx.set_scene(sc)
            ctx.set_timing(0)
            ctx.set_counting(False)
            cams = {m: path.as_array([sc.c_camera()] * (BATCH * m)) for m in (1, 2, 8)}
            move = {m: anim.tween([sc, moving(sc, scenes)], BATCH * m - 1) for m in (2, 8)}
            run_anim = lambda: ctx.render_anim_bands(W, H, cams[1], H, 0, 1, out.data_ptr(), fb, abi.RT_BANDS_FRAME, st)
            run_shut = lambda m: ctx.render_shutter_bands(W, H, cams[m], m, H, 0, 1, out.data_ptr(), fb, abi.RT_BANDS_FRAME, st)
            run_ashut = lambda m: ctx.render_anim_shutter_bands(W, H, cams[m], m, H, 0, 1, out.data_ptr(), fb, abi.RT_BANDS_FRAME, st)
            # (a)
            t = {"anim": [], "shutter 2": [], "anim-shutter 2": [], "anim-shutter-move 2": [], "shutter 8": [], "anim-shutter 8": [],
                 "anim-shutter-move 8": []}
            for _ in range(a.repeats):
                ctx.set_scene_track([sc] * BATCH)
                run_anim(), torch.cuda.synchronize()
                t["anim"].append(timed(torch, run_anim, BATCH))
                for m in (2, 8):
                    run_shut(m), torch.cuda.synchronize()
                    t[f"shutter {m}"].append(timed(torch, lambda: run_shut(m), BATCH * m))
                    for k, track in ((f"anim-shutter {m}", [sc] * (BATCH * m)), (f"anim-shutter-move {m}", move[m])):
                        ctx.set_scene_track(track)
                        run_ashut(m), torch.cuda.synchronize()
                        t[k].append(timed(torch, lambda: run_ashut(m), BATCH * m))
            say(f"{cid} {W}x{H} (a):")
            row("anim", t["anim"])
            for m in (2, 8):
                row(f"shutter {m}", t[f"shutter {m}"], ("anim", t["anim"]))
                row(f"anim-shutter {m}", t[f"anim-shutter {m}"], (f"shutter {m}", t[f"shutter {m}"]))
                d = statistics.median(t[f"anim-shutter {m}"]) - statistics.median(t[f"shutter {m}"])
                sp = max(t[f"shutter {m}"]) - min(t[f"shutter {m}"])
                say(f"        anim-shutter {m} - shutter {m} = {d:+.2f} us per sub-frame: {'inside' if abs(d) <= sp else 'OUTSIDE'} "
                    f"shutter {m}'s spread; / anim {statistics.median(t[f'anim-shutter {m}']) / statistics.median(t['anim']):.4f}")
                row(f"anim-shutter-move {m}", t[f"anim-shutter-move {m}"])
            # (b)
            ctx.set_path_supersampling(2)
            t = {"anim-ss": [], "shutter-ss 2": [], "anim-shutter-ss 2": []}
            for _ in range(a.repeats):
                ctx.set_scene_track([sc] * BATCH)
                run_anim(), torch.cuda.synchronize()
                t["anim-ss"].append(timed(torch, run_anim, BATCH))
                run_shut(2), torch.cuda.synchronize()
                t["shutter-ss 2"].append(timed(torch, lambda: run_shut(2), BATCH * 2))
                ctx.set_scene_track([sc] * (BATCH * 2))
                run_ashut(2), torch.cuda.synchronize()
                t["anim-shutter-ss 2"].append(timed(torch, lambda: run_ashut(2), BATCH * 2))
            ctx.set_path_supersampling(1)
            say(f"{cid} {W}x{H} (b), k = 2:")
            row("anim-ss", t["anim-ss"])
            row("shutter-ss 2", t["shutter-ss 2"], ("anim-ss", t["anim-ss"]))
            row("anim-shutter-ss 2", t["anim-shutter-ss 2"], ("anim-ss", t["anim-ss"]))
            say(f"        anim-shutter-ss 2 / shutter-ss 2 = "
                f"{statistics.median(t['anim-shutter-ss 2']) / statistics.median(t['shutter-ss 2']):.4f} "
                f"(shutter-ss 2's spread {max(t['shutter-ss 2']) - min(t['shutter-ss 2']):.2f})")
            # (c)
            F, m = a.host_frames, 8
            track = move[8][:F * m]
            ctx.set_scene_track(track)
            tcams = path.as_array([sc.c_camera()] * (F * m))
            small = np.empty((F, H, W), dtype=np.int32)
            big = np.empty((F * m, H, W), dtype=np.int32)
            ctx.register_host(small), ctx.register_host(big)
            try:
                t = {"in-kernel": [], "loop": [], "loop: render": []}
                for _ in range(max(3, a.repeats - 2)):
                    t0 = time.perf_counter()
                    ctx.render_anim_shutter(tcams, W, H, m, out=small)
                    t["in-kernel"].append((time.perf_counter() - t0) / F * 1e6)
                    t0 = time.perf_counter()
                    ctx.render_anim(tcams, W, H, out=big)
                    t1 = time.perf_counter()
                    mean = np.stack([path.shutter_mean(big[f * m:(f + 1) * m], m)[0] for f in range(F)])
                    t["loop"].append((time.perf_counter() - t0) / F * 1e6)
                    t["loop: render"].append((t1 - t0) / F * 1e6)
                    assert np.array_equal(mean, small), "the in-kernel mean is the host's"
            finally:
                ctx.unregister_host(small), ctx.unregister_host(big)
            say(f"{cid} {W}x{H} (c), m = 8, {F} output frames into registered host memory, wall us per output frame:")
            row("rt_render_anim_shutter", t["in-kernel"])
            row("rt_render_anim x 8 + mean", t["loop"], ("rt_render_anim_shutter", t["in-kernel"]))
            row("  of it rt_render_anim", t["loop: render"])
            del small, big
        del out
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
