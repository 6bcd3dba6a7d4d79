"""What does a sub-frame of a shutter launch cost against a frame of a path launch, and what does the shutter save
a path render into host memory?

    python tools/shutter_probe.py [--repeats 7] [--out profiles/r11_shutter.txt]

Device time per sub-frame.  The same 64 cameras (a slow walk and turn from path.replay) go through
    (a) path       rt_render_path_bands: 64 frames, 64 stores per pixel;
    (b) shutter m  rt_render_shutter_bands: 64 / m output frames of m sub-frames each, m = 2, 8, 64;
whole frames (FRAME format), counting off, 8 launches queued per synchronisation (the host side of a call runs
under the launches already queued: the device's rate), wall clock per traced camera, C3 at 1920x1080 and C4 at
3840x2160, every leg of the same library in one process, alternating.  The yardstick is (a), the PATH kernels:
its own run-to-run spread (max - min of its repeats) is what a difference has to exceed to mean anything.

Host wall time per output frame.  16 output frames of C3 at 1920x1080 into registered host memory:
    rt_render_shutter with m = 2, 8   against   rt_render_path of the same 16 m cameras
(the averaging that the path leg's caller would still have to do on the host is left out, in its favour), once
with the default chunks (256 MiB of output per launch: the shutter's 16 frames are one chunk, so its copy starts
when its trace has ended) and once with RT_PATH_CHUNK_FRAMES=4 for both legs (four chunks: copies under traces).

No threshold: exit status 0 whenever the legs ran.
"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "uu-infogr-raytracer_amd"))

CAMERAS = 64
SHUTTERS = (2, 8, 64)
SHAPES = (("C3", 1920, 1080), ("C4", 3840, 2160))
HOST_FRAMES = 16
HOST_SHUTTERS = (2, 8)


def timed_queued(torch, fn, per_launch, depth=8, min_s=0.3):
    """us per traced camera with `depth` launches queued per synchronisation."""
    n, t0 = 0, time.perf_counter()
    while True:
        for _ in range(depth):
            fn()
        torch.cuda.synchronize()
        n += depth
        dt = time.perf_counter() - t0
        if dt >= min_s:
            return dt / (n * per_launch) * 1e6


def warm(torch, fn, seconds=0.08):
    t0 = time.perf_counter()
    while time.perf_counter() - t0 < seconds:
        fn()
        torch.cuda.synchronize()


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
    assert a.repeats >= 5
    import numpy as np
    import torch
    from raytracer_hip import Context, abi, path, scenes
    torch.cuda.set_device(0)
    st = torch.cuda.current_stream().cuda_stream
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    say(f"shutter_probe: {CAMERAS} cameras per launch, whole frames (FRAME), counting off, 8 launches queued per "
        f"synchronisation, {a.repeats} alternating repeats; us per traced camera, median (min .. max)")
    for cid, W, H in SHAPES:
        sc = scenes.config(cid).resized(W, H)
        cams = walk(path, sc.c_camera(), CAMERAS)
        out = torch.empty(CAMERAS * W * H, dtype=torch.int32, device="cuda")
        with Context(1) as ctx:
            ctx.set_scene(sc)
            ctx.set_timing(0)
            ctx.set_counting(False)
            legs = {"path": lambda: ctx.render_path_bands(W, H, cams, H, 0, 1, out.data_ptr(), W * H * 4,
                                                          abi.RT_BANDS_FRAME, st)}
            for m in SHUTTERS:
                legs[f"shutter {m}"] = (lambda m=m: ctx.render_shutter_bands(W, H, cams, m, H, 0, 1, out.data_ptr(),
                                                                             W * H * 4, abi.RT_BANDS_FRAME, st))
            t = {k: [] for k in legs}
            for _ in range(a.repeats):
                for k, fn in legs.items():
                    warm(torch, fn)
                    t[k].append(timed_queued(torch, fn, CAMERAS))
            med = {k: statistics.median(v) for k, v in t.items()}
            spread = max(t["path"]) - min(t["path"])
            say(f"{cid} {W}x{H}:")
            for k in legs:
                d = med[k] - med["path"]
                verdict = "" if k == "path" else (f"   {d:+.2f} us: " + ("inside" if abs(d) <= spread else "OUTSIDE") +
                                                  " path's own spread")
                say(f"    {k:10s} {med[k]:9.2f}  ({min(t[k]):.2f} .. {max(t[k]):.2f})   / path {med[k] / med['path']:.4f}{verdict}")
            say(f"    path's own spread {spread:.2f} us")
        del out

    cid, W, H = SHAPES[0]
    sc = scenes.config(cid).resized(W, H)
    say(f"host wall time, {cid} {W}x{H}, {HOST_FRAMES} output frames into registered host memory, counting off, "
        f"{a.repeats} alternating repeats; us per output frame, median (min .. max)")
    for chunk, m in [(c, m) for c in (None, 4) for m in HOST_SHUTTERS]:
        if chunk is None:
            os.environ.pop("RT_PATH_CHUNK_FRAMES", None)  # (read when a context is created)
        else:
            os.environ["RT_PATH_CHUNK_FRAMES"] = str(chunk)
        if m == HOST_SHUTTERS[0]:
            say(f"  chunks of {'256 MiB' if chunk is None else f'{chunk} output frames'}:")
        cams = walk(path, sc.c_camera(), HOST_FRAMES * m)
        with Context(1) as ctx:
            ctx.set_scene(sc)
            ctx.set_timing(0)
            ctx.set_counting(False)
            big = np.empty((HOST_FRAMES * m, H, W), dtype=np.int32)
            ctx.register_host(big)
            try:
                small = big[:HOST_FRAMES]
                legs = {"shutter": lambda: ctx.render_shutter(cams, W, H, m, small),
                        "path": lambda: ctx.render_path(cams, W, H, big)}
                t = {k: [] for k in legs}
                for k, fn in legs.items():
                    fn()
                for _ in range(a.repeats):
                    for k, fn in legs.items():
                        t0 = time.perf_counter()
                        fn()
                        t[k].append((time.perf_counter() - t0) / HOST_FRAMES * 1e6)
            finally:
                ctx.unregister_host(big)
        med = {k: statistics.median(v) for k, v in t.items()}
        say(f"    m = {m}: rt_render_shutter {med['shutter']:9.1f}  ({min(t['shutter']):.1f} .. {max(t['shutter']):.1f})    "
            f"rt_render_path of {HOST_FRAMES * m} frames {med['path']:9.1f}  ({min(t['path']):.1f} .. {max(t['path']):.1f})    "
            f"path / shutter {med['path'] / med['shutter']:.2f}")
        say(f"           per traced camera: shutter {med['shutter'] / m:.1f} us, path {med['path'] / m:.1f} us; one frame "
            f"is {W * H * 4 / 1e6:.1f} MB: the shutter's copies ran at {W * H * 4 / 1e3 / med['shutter']:.1f} GB/s of output")
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
