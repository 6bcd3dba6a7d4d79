"""What do hit buffers cost beside the colour frame?

    python tools/hits_probe.py --baseline PATH/libraytracer_hip.so [--repeats 5] [--out profiles/ab/hits.txt]

64-frame launches over 64 distinct cameras from path.replay (a slow walk and turn), C3 at 1920x1080 and C4 at
3840x2160, counters off, three legs in one process, alternating:
    (a) hits-do    rt_render_path_hits_device, depth + object: 8 B stored per pixel;
    (b) hits-all   rt_render_path_hits_device, all four channels: 32 B stored per pixel;
    (c) plain      rt_render_path_bands of the same cameras (whole frames, FRAME format) from the BASELINE library --
                   the build of the parent commit, loaded side by side (--baseline); never this build's.
us per frame, median (min .. max), two ways: one launch in flight (a synchronisation after each: the host side of a
call -- 64 views built, their upload enqueued -- is in the figure), and 8 launches queued per synchronisation, where
the host side runs under the launches already queued: the device's own rate, the figure to compare.  The yardstick
is (c): its own run-to-run spread (max - min of its repeats) is what a difference has to exceed to mean anything.
Then, this build alone: rt_render_hits_device of a lone frame (all four channels and depth + object; one in flight and
8 queued), rt_pick's wall time (median of 200 calls, each synchronous), and for contrast rt_debug_segments at stride 1
of the same frame (wall, synchronous; the records beyond 2 per pixel are counted and dropped).
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

BATCH = 64
SHAPES = (("C3", 1920, 1080), ("C4", 3840, 2160))


def per_frame(torch, fn, depth, frames, min_s=0.3):
    """us per frame of back-to-back calls, `depth` of them queued per synchronisation, over >= min_s and >= 3 rounds."""
    n, t0 = 0, time.perf_counter()
    while True:
        for _ in range(depth):
            fn()
        torch.cuda.synchronize()
        n += depth
        dt = time.perf_counter() - t0
        if dt >= min_s and n >= 3 * depth:
            return dt / (n * frames) * 1e6


def warm(torch, fn, seconds=0.08):
    t0 = time.perf_counter()
    while time.perf_counter() - t0 < seconds:
        fn()
        torch.cuda.synchronize()


def fmt(v):
    return f"{statistics.median(v):9.2f}  ({min(v):.2f} .. {max(v):.2f})"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--baseline", required=True, help="libraytracer_hip.so of the parent commit (the plain leg)")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert a.repeats >= 3
    import torch
    from raytracer_hip import Context, abi, path, scenes
    torch.cuda.set_device(0)
    st = torch.cuda.current_stream().cuda_stream
    base_lib = abi.load_library(os.path.abspath(a.baseline), local=True)
    assert getattr(base_lib, "rt_render_hits_device", None) is None, "--baseline is a build with hit buffers, not the parent's"

    class BaselineContext(Context):
        """A single-GPU context of the baseline library (Context's methods call self.lib)."""

        def __init__(self):
            self.lib, self.ptr, self.n_gpus, self.scene = base_lib, C.c_void_p(), 1, None
            abi.check(base_lib, base_lib.rt_create_ex(1, 0, C.byref(self.ptr)))

    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    say(f"hits_probe: {BATCH}-frame launches, {BATCH} distinct cameras, counters off, {a.repeats} alternating repeats; "
        f"us per frame, median (min .. max); plain = rt_render_path_bands of the baseline library {a.baseline}")
    for cid, W, H in SHAPES:
        sc = scenes.config(cid).resized(W, H)
        cam = sc.c_camera()
        events = []
        for i in range(BATCH):
            events += [("key", "W"), ("mouse", 3.0, 0.5 if i % 2 else -0.5), ("frame",)]
        move = path.as_array(path.replay(cam, events))
        n = BATCH * W * H
        colour = torch.empty(n, dtype=torch.int32, device="cuda")
        depth, obj = torch.empty(n, dtype=torch.float32, device="cuda"), torch.empty(n, dtype=torch.int32, device="cuda")
        pos, nrm = torch.empty(3 * n, dtype=torch.float32, device="cuda"), torch.empty(3 * n, dtype=torch.float32, device="cuda")
        do = dict(depth=depth.data_ptr(), object=obj.data_ptr())
        full = dict(do, position=pos.data_ptr(), normal=nrm.data_ptr())
        with Context(1) as ctx, BaselineContext() as base:
            for c in (ctx, base):
                c.set_scene(sc)
                c.set_timing(0)
                c.set_counting(False)
            legs = {
                "hits-do": lambda: ctx.render_path_hits_device(W, H, move, stream=st, **do),
                "hits-all": lambda: ctx.render_path_hits_device(W, H, move, stream=st, **full),
                "plain": lambda: base.render_path_bands(W, H, move, H, 0, 1, colour.data_ptr(), W * H * 4, abi.RT_BANDS_FRAME, st),
            }
            for depth_q, what in ((1, "one launch in flight"), (8, "8 launches queued per synchronisation (the device's rate)")):
                t = {k: [] for k in legs}
                for _ in range(a.repeats):
                    for k, fn in legs.items():
                        warm(torch, fn)
                        t[k].append(per_frame(torch, fn, depth_q, BATCH))
                med = {k: statistics.median(v) for k, v in t.items()}
                spread = max(t["plain"]) - min(t["plain"])
                say(f"{cid} {W}x{H}, {what}:")
                for k in legs:
                    say(f"    {k:9s} {fmt(t[k])}   / plain {med[k] / med['plain']:.4f}")
                for k in ("hits-do", "hits-all"):
                    d = med[k] - med["plain"]
                    say(f"    {k} - plain = {d:+.2f} us per frame; plain's own spread {spread:.2f}: "
                        f"{'inside' if abs(d) <= spread else 'below' if d < 0 else 'ABOVE'} it")
                if depth_q == 8:
                    px = W * H
                    say(f"    stores: hits-do {8 * px / med['hits-do'] / 1e3:.1f} GB/s, hits-all {32 * px / med['hits-all'] / 1e3:.1f} GB/s, "
                        f"plain {4 * px / med['plain'] / 1e3:.1f} GB/s")
            # this build alone: the lone frame, the pick, the debug view
            lone = {
                "lone-do": lambda: ctx.render_hits_device(W, H, stream=st, **do),
                "lone-all": lambda: ctx.render_hits_device(W, H, stream=st, **full),
            }
            for k, fn in lone.items():
                warm(torch, fn)
                one = [per_frame(torch, fn, 1, 1, 0.15) for _ in range(a.repeats)]
                eight = [per_frame(torch, fn, 8, 1, 0.15) for _ in range(a.repeats)]
                say(f"{cid} {W}x{H} rt_render_hits_device {k}: one in flight {fmt(one)} us, 8 queued {fmt(eight)} us per frame")
            torch.cuda.synchronize()
            ts = []
            for i in range(200):
                t0 = time.perf_counter()
                ctx.pick(W, H, (i * 97) % W, (i * 61) % H)
                ts.append((time.perf_counter() - t0) * 1e6)
            say(f"{cid} {W}x{H} rt_pick wall: median {statistics.median(ts):.1f} us (min {min(ts):.1f}, max {max(ts):.1f}) of 200 calls")
            ts = []
            for _ in range(3):
                t0 = time.perf_counter()
                _, total = ctx.debug_segments(W, H, 1, 2 * W * H)
                ts.append((time.perf_counter() - t0) * 1e6)
            say(f"{cid} {W}x{H} rt_debug_segments stride 1: wall {statistics.median(ts):.0f} us median of 3 "
                f"(min {min(ts):.0f}), {total} records appended")
        del colour, depth, obj, pos, nrm
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
