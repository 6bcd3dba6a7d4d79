"""What does rt_set_path_adaptive_sampling cost against full path supersampling, and against the plain path frame?

    python tools/path_adaptive_probe.py [--repeats 7] [--out profiles/ab/path_adaptive.txt]

Device time per output frame.  64-frame launches of whole frames (FRAME format), counting and timing off, launches queued
per synchronisation (the device's rate; one per synchronisation once a launch takes a quarter of a second), C3 at a
1920x1080 and C4 at a 3840x2160 output, k = 2 and 4, every leg in one process and one context, alternating; wall clock
around work that ends in a synchronisation.
    (p) PATH         rt_render_path_bands at path factor 1: the plain frame;
    (s) PATH_SS      the same cameras at factor k, threshold 0: every pixel gets its k^2 samples;
    (a) PATH_ADAPT   threshold 16, and 256 (nothing is refined: the cost of the adaptive kernel itself);
    (S) ANIM_SS      rt_render_anim_bands over a track of 64 x the same scene, the same cameras, threshold 0;
    (A) ANIM_ADAPT   threshold 16, and 256.
The share of tiles refined comes from one counting launch per threshold: (primary_rays - pixels) / ((k^2 - 1) pixels)
(both sizes are whole tiles in both axes).  (a) at 16 beats (s) when the difference of the medians exceeds both legs'
spreads (max - min of their repeats).

End to end into registered host memory, C3, 1920x1080 output, 4 frames: rt_render_path at threshold 16 against threshold 0.

No threshold on any figure: exit status 0 whenever the legs ran.
"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "uu-infogr-raytracer_amd"))

CAMERAS = 64
FACTORS = (2, 4)
SHAPES = (("C3", 1920, 1080), ("C4", 3840, 2160))
THRESHOLD = 16
HOST_FRAMES = 4


def timed_queued(torch, fn, per_launch, min_s=0.3):
    """us per unit of `per_launch`: after one warm launch, which also sizes the queue (4 launches per synchronisation, 1
    once a launch takes a quarter of a second), launches until min_s have passed."""
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    depth = 1 if time.perf_counter() - t0 >= 0.25 else 4
    n, t0 = 0, time.perf_counter()
    while True:
        for _ in range(depth):
            fn()
        torch.cuda.synchronize()
        n += depth
        dt = time.perf_counter() - t0
        if dt >= min_s:
            return dt / (n * per_launch) * 1e6


def walk(path, cam, n):
    events = []
    for i in range(n):
        events += [("key", "W"), ("mouse", 3.0, 0.5 if i % 2 else -0.5), ("frame",)]
    return path.as_array(path.replay(cam, events))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert a.repeats >= 3
    import numpy as np
    import torch
    from raytracer_hip import Context, abi, path, scenes
    torch.cuda.set_device(0)
    st = torch.cuda.current_stream().cuda_stream
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    def stat(v):
        return f"{statistics.median(v):10.2f}  ({min(v):.2f} .. {max(v):.2f})"

    say(f"path_adaptive_probe: {CAMERAS}-camera launches, whole frames (FRAME), counting off, {a.repeats} alternating repeats; "
        f"us per output frame, median (min .. max)")
    for cid, W, H in SHAPES:
        sc = scenes.config(cid).resized(W, H)
        cams = walk(path, sc.c_camera(), CAMERAS)
        out = torch.empty(CAMERAS * W * H, dtype=torch.int32, device="cuda")
        with Context(1) as ctx:
            ctx.set_scene(sc)
            ctx.set_scene_track([sc] * CAMERAS)
            ctx.set_timing(0)
            for k in FACTORS:
                def leg(anim, kk, T):
                    def fn():
                        ctx.set_path_supersampling(kk)
                        ctx.set_path_adaptive_sampling(T)
                        call = ctx.render_anim_bands if anim else ctx.render_path_bands
                        call(W, H, cams, H, 0, 1, out.data_ptr(), W * H * 4, abi.RT_BANDS_FRAME, st)
                    return fn

                share = {}
                ctx.set_counting(True)
                for T in (THRESHOLD, 256):
                    ctx.reset_stats()
                    leg(False, k, T)()
                    torch.cuda.synchronize()
                    px = CAMERAS * W * H
                    share[T] = (ctx.stats()["primary_rays"] - px) / ((k * k - 1) * px)
                ctx.set_counting(False)
                legs = {
                    "p PATH k=1": leg(False, 1, 0),
                    "s PATH_SS": leg(False, k, 0),
                    f"a PATH_ADAPT T={THRESHOLD}": leg(False, k, THRESHOLD),
                    "a PATH_ADAPT T=256": leg(False, k, 256),
                    "S ANIM_SS": leg(True, k, 0),
                    f"A ANIM_ADAPT T={THRESHOLD}": leg(True, k, THRESHOLD),
                    "A ANIM_ADAPT T=256": leg(True, k, 256),
                }
                t = {name: [] for name in legs}
                for _ in range(a.repeats):
                    for name, fn in legs.items():
                        t[name].append(timed_queued(torch, fn, CAMERAS))
                med = {name: statistics.median(v) for name, v in t.items()}
                say(f"{cid} {W}x{H} output, k = {k} ({k * W}x{k * H} samples): {100 * share[THRESHOLD]:.1f} % of the tiles refined at "
                    f"T = {THRESHOLD}, {100 * share[256]:.1f} % at 256")
                p_name = "p PATH k=1"
                for name in legs:
                    ref = "S ANIM_SS" if name[0] == "A" else "s PATH_SS"
                    extra = f"   {med[name] / med[p_name]:6.2f} plain frames"
                    if name[0] in "aA":
                        d = med[ref] - med[name]
                        both = (max(t[name]) - min(t[name])) + (max(t[ref]) - min(t[ref]))
                        extra += f"   {med[name] / med[ref]:.4f} of {ref[2:]}: {d:+.2f} us, " + \
                                 ("outside" if abs(d) > both else "INSIDE") + f" the two spreads ({both:.2f} us)"
                    say(f"    {name:24s} {stat(t[name])}{extra}")
        del out

    cid, W, H = SHAPES[0]
    sc = scenes.config(cid).resized(W, H)
    cams = walk(path, sc.c_camera(), HOST_FRAMES)
    say(f"end to end into registered host memory, {cid} {W}x{H} output, {HOST_FRAMES} frames, counting off, {a.repeats} "
        f"alternating repeats; us per output frame, median (min .. max)")
    buf = np.empty((HOST_FRAMES, H, W), dtype=np.int32)
    with Context(1) as ctx:
        ctx.set_scene(sc)
        ctx.set_timing(0)
        ctx.set_counting(False)
        ctx.register_host(buf)
        try:
            for k in FACTORS:
                ctx.set_path_supersampling(k)
                t = {0: [], THRESHOLD: []}
                for rep in range(a.repeats + 1):  # (the first round warms both)
                    for T in t:
                        ctx.set_path_adaptive_sampling(T)
                        t0 = time.perf_counter()
                        ctx.render_path(cams, W, H, buf)
                        if rep:
                            t[T].append((time.perf_counter() - t0) / HOST_FRAMES * 1e6)
                say(f"    k = {k}: rt_render_path at T = {THRESHOLD} {stat(t[THRESHOLD])}    at T = 0 (PATH_SS) {stat(t[0])}    "
                    f"ratio {statistics.median(t[THRESHOLD]) / statistics.median(t[0]):.3f}")
        finally:
            ctx.unregister_host(buf)
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
