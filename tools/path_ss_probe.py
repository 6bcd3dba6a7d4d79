"""What does rt_set_path_supersampling cost against the workaround it replaces, and against its own parts?

    python tools/path_ss_probe.py --parent-lib PATH/libraytracer_hip.so [--repeats 5] [--out profiles/ab/path_ss.txt]

Device time per output frame.  64-frame launches of whole frames (FRAME format), counting and timing off, several
launches queued per synchronisation (the device's rate), C3 and C4 at a 1920x1080 output, k = 2 and 4, every leg in one
process, alternating; wall clock around work that ends in a synchronisation.
    (a) baseline   the parent commit's library (--parent-lib): rt_render_path_bands of 64 frames at kW x kH -- the
                   device half of the workaround (render big, copy k^2 times the pixels, box-filter on the host);
    (b) PATH_SS    this library: rt_render_path_bands of the same 64 cameras at W x H with rt_set_path_supersampling(k):
                   the same traces, 1/k^2 of the stores;
    (c) SHUTTER_SS rt_render_shutter_bands, m = 2: 32 output frames of the same 64 cameras, per sub-frame;
    (d) ANIM_SS    rt_render_anim_bands over a track of 64 x the same scene, the same cameras.
The yardstick is (a): its own run-to-run spread (max - min of its repeats) is what (b) - (a) has to exceed to mean
anything; (c) and (d) are set against (b).

End to end into registered host memory, C3, 1920x1080 output, 4 frames: rt_render_path at (W, H, k) with this library
against the parent's rt_render_path at (kW, kH) plus numpy's supersample.box_resolve of its frames (timed once per
frame: it is host arithmetic).

No threshold: exit status 0 whenever the legs ran.
"""
import argparse
import ctypes as C
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "uu-infogr-raytracer_amd"))

CAMERAS = 64
FACTORS = (2, 4)
SHAPES = (("C3", 1920, 1080), ("C4", 1920, 1080))
HOST_FRAMES = 4


def timed_queued(torch, fn, per_launch, depth=4, min_s=0.3):
    """us per unit of `per_launch` with `depth` launches queued per synchronisation."""
    n, t0 = 0, time.perf_counter()
    while True:
        for _ in range(depth):
            fn()
        torch.cuda.synchronize()
        n += depth
        dt = time.perf_counter() - t0
        if dt >= min_s:
            return dt / (n * per_launch) * 1e6


def warm(torch, fn, launches=2):
    for _ in range(launches):
        fn()
    torch.cuda.synchronize()


def walk(path, cam, n):
    events = []
    for i in range(n):
        events += [("key", "W"), ("mouse", 3.0, 0.5 if i % 2 else -0.5), ("frame",)]
    return path.as_array(path.replay(cam, events))


def open_context(Context, check, lib):
    """A Context of another build of the library (an older one lacks the newer entry points: only what it has is called)."""
    ctx = Context.__new__(Context)
    ctx.lib, ctx.ptr, ctx.n_gpus, ctx.scene = lib, C.c_void_p(), 1, None
    check(lib, lib.rt_create_ex(1, 0, C.byref(ctx.ptr)))
    return ctx


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", required=True, help="libraytracer_hip.so built from the parent commit")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert a.repeats >= 3
    import numpy as np
    import torch
    from raytracer_hip import Context, abi, path, scenes
    from raytracer_hip.supersample import box_resolve
    torch.cuda.set_device(0)
    st = torch.cuda.current_stream().cuda_stream
    parent = abi.load_library(os.path.abspath(a.parent_lib), local=True)
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    def stat(v):
        return f"{statistics.median(v):9.2f}  ({min(v):.2f} .. {max(v):.2f})"

    say(f"path_ss_probe: {CAMERAS}-camera launches, whole frames (FRAME), counting off, 4 launches queued per "
        f"synchronisation, {a.repeats} alternating repeats; us per output frame (c: per sub-frame), median (min .. max)")
    for cid, W, H in SHAPES:
        sc = scenes.config(cid).resized(W, H)
        cams = walk(path, sc.c_camera(), CAMERAS)
        for k in FACTORS:
            big = torch.empty(CAMERAS * k * W * k * H, dtype=torch.int32, device="cuda")
            small = big[:CAMERAS * W * H]
            base = open_context(Context, abi.check, parent)
            with Context(1) as ctx:
                try:
                    for c in (base, ctx):
                        c.set_scene(sc)
                        c.set_timing(0)
                        c.set_counting(False)
                    ctx.set_path_supersampling(k)
                    ctx.set_scene_track([sc] * CAMERAS)
                    legs = {
                        "a baseline PATH kWxkH": (lambda: base.render_path_bands(k * W, k * H, cams, k * H, 0, 1, big.data_ptr(),
                                                                                k * W * k * H * 4, abi.RT_BANDS_FRAME, st), CAMERAS),
                        "b PATH_SS": (lambda: ctx.render_path_bands(W, H, cams, H, 0, 1, small.data_ptr(), W * H * 4,
                                                                    abi.RT_BANDS_FRAME, st), CAMERAS),
                        "c SHUTTER_SS m=2": (lambda: ctx.render_shutter_bands(W, H, cams, 2, H, 0, 1, small.data_ptr(), W * H * 4,
                                                                              abi.RT_BANDS_FRAME, st), CAMERAS),
                        "d ANIM_SS": (lambda: ctx.render_anim_bands(W, H, cams, H, 0, 1, small.data_ptr(), W * H * 4,
                                                                    abi.RT_BANDS_FRAME, st), CAMERAS),
                    }
                    t = {name: [] for name in legs}
                    for _ in range(a.repeats):
                        for name, (fn, per) in legs.items():
                            warm(torch, fn)
                            t[name].append(timed_queued(torch, fn, per))
                finally:
                    base.close()
            med = {name: statistics.median(v) for name, v in t.items()}
            a_name, b_name = "a baseline PATH kWxkH", "b PATH_SS"
            spread = max(t[a_name]) - min(t[a_name])
            say(f"{cid} {W}x{H} output, k = {k} ({k * W}x{k * H} samples):")
            for name in legs:
                ref = a_name if name in (a_name, b_name) else b_name
                extra = ""
                if name == b_name:
                    d = med[name] - med[a_name]
                    extra = f"   b - a {d:+.2f} us ({med[name] / med[a_name]:.4f} of a): " + \
                            ("inside" if d <= spread else "OUTSIDE") + f" a's own spread of {spread:.2f} us"
                elif name != a_name:
                    extra = f"   / b {med[name] / med[ref]:.4f}"
                say(f"    {name:24s} {stat(t[name])}{extra}")
            del big, small

    cid, W, H = SHAPES[0]
    sc = scenes.config(cid).resized(W, H)
    cams = walk(path, sc.c_camera(), HOST_FRAMES)
    say(f"end to end into registered host memory, {cid} {W}x{H} output, {HOST_FRAMES} frames, counting off, {a.repeats} "
        f"alternating repeats; us per output frame, median (min .. max)")
    for k in FACTORS:
        out_small = np.empty((HOST_FRAMES, H, W), dtype=np.int32)
        out_big = np.empty((HOST_FRAMES, k * H, k * W), dtype=np.int32)
        base = open_context(Context, abi.check, parent)
        with Context(1) as ctx:
            try:
                for c, buf in ((base, out_big), (ctx, out_small)):
                    c.set_scene(sc)
                    c.set_timing(0)
                    c.set_counting(False)
                    c.register_host(buf)
                ctx.set_path_supersampling(k)
                legs = {"new": lambda: ctx.render_path(cams, W, H, out_small),
                        "parent": lambda: base.render_path(cams, k * W, k * H, out_big)}
                t = {name: [] for name in legs}
                for fn in legs.values():
                    fn()
                for _ in range(a.repeats):
                    for name, fn in legs.items():
                        t0 = time.perf_counter()
                        fn()
                        t[name].append((time.perf_counter() - t0) / HOST_FRAMES * 1e6)
                t0 = time.perf_counter()
                resolved = box_resolve(out_big[0], k)
                t_resolve = (time.perf_counter() - t0) * 1e6
                same = bool(np.array_equal(resolved, out_small[0]))
            finally:
                base.unregister_host(out_big)
                ctx.unregister_host(out_small)
                base.close()
        m_new, m_par = statistics.median(t["new"]), statistics.median(t["parent"])
        say(f"    k = {k}: rt_render_path at (W, H, k) {stat(t['new'])}    parent rt_render_path at (kW, kH) {stat(t['parent'])}"
            f"    numpy box_resolve of one frame {t_resolve:.0f}")
        say(f"           parent trace + copy / new {m_par / m_new:.2f}; with the host resolve {(m_par + t_resolve) / m_new:.1f}; "
            f"the workaround's frame 0, resolved, {'equals' if same else 'DIFFERS FROM'} the new call's")
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
