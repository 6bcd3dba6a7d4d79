"""What does a camera per frame cost a batch launch?

    python tools/path_probe.py [--repeats 7] [--out profiles/ab/r08_camera_path.txt]

64-frame launches of whole frames (FRAME format), one in flight (a synchronisation after each), wall clock per
frame, C3 at 1920x1080 and C4 at 3840x2160, three legs of the same build in one process, alternating:
    (a) batch      rt_render_bands_batch: 64 frames of the scene's camera, the views in the kernarg block;
    (b) path-same  rt_render_path_bands with 64 copies of that camera: the same rays, every view read from
                   its DevView record in device memory;
    (c) path-move  rt_render_path_bands with 64 distinct cameras from path.replay (a slow walk and turn).
Each leg with counting on and off (rt_set_counting).  The yardstick is (a): its own run-to-run spread (max - min
of its repeats) is what a difference has to exceed to mean anything.  (c) traces other rays than (a) and (b), so
its time says what such a path costs, not what the mechanism costs.
Also reported: the legs with 8 launches queued per synchronisation (counting off), where the host side of a call
runs under the launches already queued -- the device's own rate -- and the host time of the calls themselves (a
path call builds 64 views -- screen boxes in double precision -- and enqueues their upload before the launch;
both calls return without waiting for the GPU).
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


def timed(torch, fn, min_s=0.3):
    """us per frame of back-to-back launches, one in flight, over >= min_s and >= 3 launches."""
    n, t0 = 0, time.perf_counter()
    while True:
        fn()
        torch.cuda.synchronize()
        n += 1
        dt = time.perf_counter() - t0
        if dt >= min_s and n >= 3:
            return dt / (n * BATCH) * 1e6


def timed_queued(torch, fn, depth=8, min_s=0.3):
    """us per frame with `depth` launches queued per synchronisation: the host side of a call runs under the
    launches already queued, so this is the device's rate."""
    n, t0 = 0, time.perf_counter()
    while True:
        for _ in range(depth):
            fn()
        torch.cuda.synchronize()
        n += depth
        dt = time.perf_counter() - t0
        if dt >= min_s:
            return dt / (n * BATCH) * 1e6


def warm(torch, fn, seconds=0.08):
    t0 = time.perf_counter()
    while time.perf_counter() - t0 < seconds:
        fn()
        torch.cuda.synchronize()


def host_us(torch, fn, n=20):
    """Median host time of the call alone (it returns before the GPU has run), the GPU idle at each call."""
    ts = []
    for _ in range(n):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e6)
    torch.cuda.synchronize()
    return statistics.median(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert a.repeats >= 5
    import torch
    from raytracer_hip import Context, abi, path, scenes
    torch.cuda.set_device(0)
    st = torch.cuda.current_stream().cuda_stream
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    say(f"path_probe: {BATCH}-frame launches of whole frames (FRAME), one in flight, {a.repeats} alternating repeats; "
        f"us per frame, median (min .. max)")
    for cid, W, H in SHAPES:
        sc = scenes.config(cid).resized(W, H)
        cam = sc.c_camera()
        same = path.as_array([cam] * BATCH)
        events = []
        for i in range(BATCH):
            events += [("key", "W"), ("mouse", 3.0, 0.5 if i % 2 else -0.5), ("frame",)]
        move = path.as_array(path.replay(cam, events))
        out = torch.empty(BATCH * W * H, dtype=torch.int32, device="cuda")
        with Context(1) as ctx:
            ctx.set_scene(sc)
            ctx.set_timing(0)
            legs = {
                "batch": lambda: ctx.render_bands_batch(W, H, H, 0, 1, BATCH, out.data_ptr(), W * H * 4, abi.RT_BANDS_FRAME, st),
                "path-same": lambda: ctx.render_path_bands(W, H, same, H, 0, 1, out.data_ptr(), W * H * 4, abi.RT_BANDS_FRAME, st),
                "path-move": lambda: ctx.render_path_bands(W, H, move, H, 0, 1, out.data_ptr(), W * H * 4, abi.RT_BANDS_FRAME, st),
            }
            for counting in (False, True):
                ctx.set_counting(counting)
                t = {k: [] for k in legs}
                for _ in range(a.repeats):
                    for k, fn in legs.items():
                        warm(torch, fn)
                        t[k].append(timed(torch, fn))
                med = {k: statistics.median(v) for k, v in t.items()}
                spread = max(t["batch"]) - min(t["batch"])
                say(f"{cid} {W}x{H} counting {'on ' if counting else 'off'}:")
                for k in legs:
                    say(f"    {k:10s} {med[k]:9.2f}  ({min(t[k]):.2f} .. {max(t[k]):.2f})   / batch {med[k] / med['batch']:.4f}")
                d = med["path-same"] - med["batch"]
                say(f"    path-same - batch = {d:+.2f} us per frame; batch's own spread {spread:.2f}: "
                    f"{'inside' if abs(d) <= spread else 'OUTSIDE'} it")
            ctx.set_counting(False)
            q = {k: [] for k in legs}
            for _ in range(a.repeats):
                for k, fn in legs.items():
                    warm(torch, fn)
                    q[k].append(timed_queued(torch, fn))
            qm = {k: statistics.median(v) for k, v in q.items()}
            say(f"{cid} {W}x{H} counting off, 8 launches queued per synchronisation (host time of a call hidden):")
            for k in legs:
                say(f"    {k:10s} {qm[k]:9.2f}  ({min(q[k]):.2f} .. {max(q[k]):.2f})   / batch {qm[k] / qm['batch']:.4f}")
            say(f"    path-same - batch = {qm['path-same'] - qm['batch']:+.2f} us per frame; batch's own spread "
                f"{max(q['batch']) - min(q['batch']):.2f}")
            h = {k: host_us(torch, fn) for k, fn in legs.items()}
            say(f"{cid} {W}x{H} host time of one call (median of 20, GPU idle): batch {h['batch']:.1f} us, path-same "
                f"{h['path-same']:.1f} us, path-move {h['path-move']:.1f} us -- {BATCH} views built and their upload "
                f"enqueued: +{h['path-move'] - h['batch']:.1f} us per call, {(h['path-move'] - h['batch']) / BATCH:.2f} us per frame")
        del out
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
