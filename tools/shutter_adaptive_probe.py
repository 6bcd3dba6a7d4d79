"""What does rt_set_shutter_adaptive_sampling cost against full supersampling under a shutter, and against the factor-1
shutter frame?

    python tools/shutter_adaptive_probe.py [--repeats 5] [--out profiles/ab/shutter_adaptive.txt] [--parent LIB]

Device time per output frame.  64-output-frame launches of whole frames (FRAME format), counting and timing off, launches
queued per synchronisation (one per synchronisation once a launch takes a quarter of a second), C3 at a 1920x1080 and C4
at a 3840x2160 output, shutters m = 2 and 8, k = 2 and 4, every leg in one process and one context, alternating; wall
clock around work that ends in a synchronisation.
    (p) SHUTTER              rt_render_shutter_bands at path factor 1: the factor-1 shutter frame;
    (s) SHUTTER_SS           the same cameras at factor k, every threshold 0: every pixel gets its m k^2 samples;
    (a) SHUTTER_ADAPT        shutter threshold 16, and 256 (nothing is refined: the cost of the adaptive kernel itself);
    (P) (S) (A)              the same for rt_render_anim_shutter_bands over a track of 64 m x the same scene.
The share of tiles refined comes from one counting launch per threshold: (primary_rays - m pixels) / (m (k^2 - 1) pixels)
(both sizes are whole tiles in both axes).  (a) at 16 beats (s) when the difference of the medians exceeds both legs'
spreads (max - min of their repeats).

End to end into registered host memory, C3, 1920x1080 output, 4 output frames: rt_render_shutter at threshold 16 against
threshold 0.

--parent LIB: the unchanged paths.  SHUTTER_SS and ANIM_SHUTTER_SS at shutter threshold 0 through this build and through
another build of the library (the parent commit's), both loaded into this process, alternating: the same kernels, so the
difference of the medians should lie inside the parent legs' own spread.

No threshold on any figure: exit status 0 whenever the legs ran.
"""
import argparse
import ctypes as C
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "uu-infogr-raytracer_amd"))

FRAMES = 64
SHUTTERS = (2, 8)
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
    return path.replay(cam, events)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--parent", default=None, help="another build of libraytracer_hip.so for the unchanged-paths legs")
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

    say(f"shutter_adaptive_probe: {FRAMES}-output-frame launches, whole frames (FRAME), counting off, {a.repeats} alternating repeats; "
        f"us per output frame, median (min .. max)")
    for cid, W, H in SHAPES:
        sc = scenes.config(cid).resized(W, H)
        out = torch.empty(FRAMES * W * H, dtype=torch.int32, device="cuda")
        for m in SHUTTERS:
            cams = path.as_array(path.subframes(walk(path, sc.c_camera(), FRAMES), m))
            with Context(1) as ctx:
                ctx.set_scene(sc)
                ctx.set_scene_track([sc] * (FRAMES * m))
                ctx.set_timing(0)
                for k in FACTORS:
                    def leg(anim, kk, T):
                        def fn():
                            ctx.set_path_supersampling(kk)
                            ctx.set_shutter_adaptive_sampling(T)
                            call = ctx.render_anim_shutter_bands if anim else ctx.render_shutter_bands
                            call(W, H, cams, m, H, 0, 1, out.data_ptr(), W * H * 4, abi.RT_BANDS_FRAME, st)
                        return fn

                    share = {}
                    ctx.set_counting(True)
                    for T in (THRESHOLD, 256):
                        ctx.reset_stats()
                        leg(False, k, T)()
                        torch.cuda.synchronize()
                        px = FRAMES * W * H * m
                        share[T] = (ctx.stats()["primary_rays"] - px) / ((k * k - 1) * px)
                    ctx.set_counting(False)
                    legs = {
                        "p SHUTTER k=1": leg(False, 1, 0),
                        "s SHUTTER_SS": leg(False, k, 0),
                        f"a SHUTTER_ADAPT T={THRESHOLD}": leg(False, k, THRESHOLD),
                        "a SHUTTER_ADAPT T=256": leg(False, k, 256),
                        "P ANIM_SHUTTER k=1": leg(True, 1, 0),
                        "S ANIM_SHUTTER_SS": leg(True, k, 0),
                        f"A ANIM_SHUTTER_ADAPT T={THRESHOLD}": leg(True, k, THRESHOLD),
                        "A ANIM_SHUTTER_ADAPT T=256": leg(True, k, 256),
                    }
                    t = {name: [] for name in legs}
                    for _ in range(a.repeats):
                        for name, fn in legs.items():
                            t[name].append(timed_queued(torch, fn, FRAMES))
                    med = {name: statistics.median(v) for name, v in t.items()}
                    say(f"{cid} {W}x{H} output, m = {m}, k = {k} ({m * k * k} samples per pixel): {100 * share[THRESHOLD]:.1f} % of the tiles "
                        f"refined at T = {THRESHOLD}, {100 * share[256]:.1f} % at 256")
                    for name in legs:
                        track = name[0] in "PSA"
                        ref, plain = ("S ANIM_SHUTTER_SS", "P ANIM_SHUTTER k=1") if track else ("s SHUTTER_SS", "p SHUTTER k=1")
                        extra = f"   {med[name] / med[plain]:6.2f} factor-1 shutter frames"
                        if name[0] in "aA":
                            d = med[ref] - med[name]
                            both = (max(t[name]) - min(t[name])) + (max(t[ref]) - min(t[ref]))
                            extra += f"   {med[name] / med[ref]:.4f} of {ref[2:]}: {d:+.2f} us, " + \
                                     ("outside" if abs(d) > both else "INSIDE") + f" the two spreads ({both:.2f} us)"
                        say(f"    {name:32s} {stat(t[name])}{extra}")
        del out

    cid, W, H = SHAPES[0]
    sc = scenes.config(cid).resized(W, H)
    say(f"end to end into registered host memory, {cid} {W}x{H} output, {HOST_FRAMES} output frames, counting off, {a.repeats} "
        f"alternating repeats; us per output frame, median (min .. max)")
    buf = np.empty((HOST_FRAMES, H, W), dtype=np.int32)
    with Context(1) as ctx:
        ctx.set_scene(sc)
        ctx.set_timing(0)
        ctx.set_counting(False)
        ctx.register_host(buf)
        try:
            for m in SHUTTERS:
                cams = path.as_array(path.subframes(walk(path, sc.c_camera(), HOST_FRAMES), m))
                for k in FACTORS:
                    ctx.set_path_supersampling(k)
                    t = {0: [], THRESHOLD: []}
                    for rep in range(a.repeats + 1):  # (the first round warms both)
                        for T in t:
                            ctx.set_shutter_adaptive_sampling(T)
                            t0 = time.perf_counter()
                            ctx.render_shutter(cams, W, H, m, buf)
                            if rep:
                                t[T].append((time.perf_counter() - t0) / HOST_FRAMES * 1e6)
                    say(f"    m = {m}, k = {k}: rt_render_shutter at T = {THRESHOLD} {stat(t[THRESHOLD])}    at T = 0 (SHUTTER_SS) {stat(t[0])}    "
                        f"ratio {statistics.median(t[THRESHOLD]) / statistics.median(t[0]):.3f}")
        finally:
            ctx.unregister_host(buf)

    def flush():
        if a.out:
            with open(a.out, "w") as f:
                f.write("\n".join(lines) + "\n")

    flush()
    if a.parent:
        # the unchanged paths: this build and the other one through the plain C ABI, one context each, alternating
        say(f"unchanged paths: SHUTTER_SS and ANIM_SHUTTER_SS at shutter threshold 0, this build against {os.path.basename(os.path.dirname(a.parent)) or a.parent} "
            f"(the parent commit's library), {FRAMES}-output-frame launches, m = 2, k = 2, {a.repeats} alternating repeats; us per output frame")
        libs = {"parent": abi.load_library(os.path.abspath(a.parent), local=True), "branch": abi.load_library()}
        for cid, W, H in SHAPES:
            sc = scenes.config(cid).resized(W, H)
            m, k = 2, 2
            cams = path.as_array(path.subframes(walk(path, sc.c_camera(), FRAMES), m))
            out = torch.empty(FRAMES * W * H, dtype=torch.int32, device="cuda")
            S, P, L = sc.c_arrays()
            n = FRAMES * m
            amb = (abi.rt_vec3 * n)(*[abi.rt_vec3(*sc.ambient)] * n)
            ctxs = {}
            for who, lib in libs.items():
                ctx = C.c_void_p()
                assert lib.rt_create(1, C.byref(ctx)) == 0
                assert lib.rt_set_scene(ctx, S, len(sc.spheres), P, len(sc.planes), L, len(sc.lights), abi.rt_vec3(*sc.ambient), sc.recursion_limit) == 0
                tS = (type(S)._type_ * (len(sc.spheres) * n))(*list(S) * n)
                tP = (type(P)._type_ * (len(sc.planes) * n))(*list(P) * n)
                tL = (type(L)._type_ * (len(sc.lights) * n))(*list(L) * n)
                assert lib.rt_set_scene_track(ctx, tS, len(sc.spheres), tP, len(sc.planes), tL, len(sc.lights), amb, sc.recursion_limit, n) == 0
                assert lib.rt_set_timing(ctx, 0) == 0 and lib.rt_set_counting(ctx, 0) == 0 and lib.rt_set_path_supersampling(ctx, k) == 0
                ctxs[who] = ctx

            def leg(who, anim):
                lib, ctx = libs[who], ctxs[who]
                nb = C.c_int(0)

                def fn():
                    if anim:
                        rc = lib.rt_render_anim_shutter_bands(ctx, W, H, cams, 0, FRAMES, m, H, 0, 1, C.c_void_p(out.data_ptr()), W * H * 4,
                                                              abi.RT_BANDS_FRAME, C.c_void_p(st), C.byref(nb))
                    else:
                        rc = lib.rt_render_shutter_bands(ctx, W, H, cams, FRAMES, m, H, 0, 1, C.c_void_p(out.data_ptr()), W * H * 4,
                                                         abi.RT_BANDS_FRAME, C.c_void_p(st), C.byref(nb))
                    assert rc == 0
                return fn

            legs = {f"{who} {'ANIM_SHUTTER_SS' if anim else 'SHUTTER_SS'}": leg(who, anim) for anim in (False, True) for who in libs}
            t = {name: [] for name in legs}
            for _ in range(a.repeats):
                for name, fn in legs.items():
                    t[name].append(timed_queued(torch, fn, FRAMES))
            say(f"{cid} {W}x{H} output")
            for mode in ("SHUTTER_SS", "ANIM_SHUTTER_SS"):
                pa, br = t[f"parent {mode}"], t[f"branch {mode}"]
                d = statistics.median(br) - statistics.median(pa)
                say(f"    {mode:18s} parent {stat(pa)}    branch {stat(br)}    {d:+.2f} us, " +
                    ("inside" if abs(d) <= max(pa) - min(pa) else "OUTSIDE") + f" the parent legs' spread ({max(pa) - min(pa):.2f} us)")
            torch.cuda.synchronize()
            for who, lib in libs.items():
                lib.rt_destroy(ctxs[who])
            del out
    flush()
    return 0


if __name__ == "__main__":
    sys.exit(main())
