"""What does adaptive supersampling (rt_set_adaptive_sampling) cost beside full supersampling and the plain frame?

    python tools/adaptive_probe.py --baseline-lib PATH/libraytracer_hip.so [--repeats 7] [--out profiles/adaptive_probe.txt]

Wall clock per frame, counters and timing off, one launch in flight: 64-frame rt_render_bands_batch launches in FRAME
format at 1920x1080, for C3 and C4 at k = 2 and 4, six legs in one process, alternating, each after a warm-up of at
least 50 ms; median of the repeats with min and max:
    (a) the baseline library (a build of the parent commit), plain k = 1 frame
    (b) the baseline library, full supersampling at k
    (c) this build, T = 256 (the adaptive kernels, nothing refined)
    (d) this build, T = 16
    (e) this build, T = 1
    (f) this build, T = 0 (full supersampling by the SS kernels)
Beside each adaptive leg the model 1 + share (k^2 - 1) plain frames, share = the refined tiles' part of the oracle's
1080p frame (supersample.refine_mask, computed here on the CPU).
Bars, both against the baseline library in the same session:
    (f) <= (b) + (b)'s own spread (max - min of its repeats): the existing supersampling has not become slower;
    (d) <  (b): the point of the feature.
Reported with no bar: (c) against (a), the price of the mode on a frame that refines nothing; (d) against the model;
lone rt_render_device frames and Tick(), synchronous and two deep, at k = 2 and 4 and T = 16 on C3.
"""
import argparse
import ctypes as C
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "uu-infogr-raytracer_amd"))
sys.path.insert(0, os.path.join(ROOT, "oracle"))

BATCH = 64
W, H = 1920, 1080
THRESHOLDS = (256, 16, 1)


class Lib:
    """One build of the library with a single-GPU context (the baseline build lacks the newer entry points)."""

    def __init__(self, path, abi):
        self.abi = abi
        self.lib = abi.load_library(os.path.abspath(path), local=True) if path else abi.load_library()
        self.ctx = C.c_void_p()
        assert self.lib.rt_create(1, C.byref(self.ctx)) == 0, self.lib.rt_last_error(None)
        assert self.lib.rt_set_counting(self.ctx, 0) == 0
        assert self.lib.rt_set_timing(self.ctx, 0) == 0

    def scene(self, sc):
        S, P, L = sc.c_arrays()
        assert self.lib.rt_set_scene(self.ctx, S, len(sc.spheres), P, len(sc.planes), L, len(sc.lights),
                                     self.abi.rt_vec3(*sc.ambient), sc.recursion_limit) == 0
        assert self.lib.rt_set_camera(self.ctx, C.byref(sc.c_camera())) == 0

    def sampling(self, k, T=None):
        assert self.lib.rt_set_supersampling(self.ctx, k) == 0
        if T is not None:
            assert self.lib.rt_set_adaptive_sampling(self.ctx, T) == 0

    def batch(self, d_ptr, stream):
        rc = self.lib.rt_render_bands_batch(self.ctx, W, H, H, 0, 1, BATCH, C.c_void_p(d_ptr), W * H * 4,
                                            self.abi.RT_BANDS_FRAME, C.c_void_p(stream), None)
        assert rc == 0, self.lib.rt_last_error(self.ctx)

    def device(self, d_ptr, stream):
        assert self.lib.rt_render_device(self.ctx, W, H, C.c_void_p(d_ptr), C.c_void_p(stream)) == 0


def timed(torch, fn, frames_per_call, min_s=0.25):
    """us per frame of back-to-back calls, one in flight (a synchronisation after each), over >= min_s."""
    n, t0 = 0, time.perf_counter()
    while True:
        fn()
        torch.cuda.synchronize()
        n += 1
        dt = time.perf_counter() - t0
        if dt >= min_s and n >= 3:
            return dt / (n * frames_per_call) * 1e6


def warm(torch, fn, seconds=0.06):
    t0 = time.perf_counter()
    while time.perf_counter() - t0 < seconds:
        fn()
        torch.cuda.synchronize()


def fmt(ts):
    return f"{statistics.median(ts):9.2f} (min {min(ts):.2f} max {max(ts):.2f})"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--baseline-lib", required=True)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert a.repeats >= 5
    import numpy as np
    import torch

    import pyoracle
    from raytracer_hip import abi, scenes
    from raytracer_hip.supersample import refine_mask
    torch.cuda.set_device(0)
    st = torch.cuda.current_stream().cuda_stream
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    new, base = Lib(None, abi), Lib(a.baseline_lib, abi)
    say(f"adaptive_probe: {BATCH}-frame rt_render_bands_batch launches (FRAME), one in flight, counters and timing off, "
        f"{W}x{H}; {a.repeats} alternating repeats; us per frame, median (min max)")
    out = torch.empty(BATCH * W * H, dtype=torch.int32, device="cuda")
    ok_all = True
    for cid in ("C3", "C4"):
        sc = scenes.config(cid).resized(W, H)
        new.scene(sc)
        base.scene(sc)
        plain, _ = pyoracle.render(sc, pyoracle.MODE_NEAREST, 16)
        share = {T: float(refine_mask(plain, T).mean()) for T in THRESHOLDS}
        # the plain frame of this build is the oracle's (the shares describe what the kernels decide on)
        new.sampling(1, 0)
        new.device(out.data_ptr(), st)
        torch.cuda.synchronize()
        assert np.array_equal(out[:W * H].cpu().numpy().reshape(H, W), plain), "the plain frame is not the oracle's"
        say(f"{cid}: refined share of the 8x8 tiles of the oracle's {W}x{H} frame: " +
            ", ".join(f"T={T}: {share[T]:.4f}" for T in THRESHOLDS))
        for k in (2, 4):
            legs = {"a": lambda: (base.sampling(1), base.batch(out.data_ptr(), st)),
                    "b": lambda: (base.sampling(k), base.batch(out.data_ptr(), st)),
                    "c": lambda: (new.sampling(k, 256), new.batch(out.data_ptr(), st)),
                    "d": lambda: (new.sampling(k, 16), new.batch(out.data_ptr(), st)),
                    "e": lambda: (new.sampling(k, 1), new.batch(out.data_ptr(), st)),
                    "f": lambda: (new.sampling(k, 0), new.batch(out.data_ptr(), st))}
            t = {name: [] for name in legs}
            for _ in range(a.repeats):
                for name, fn in legs.items():
                    warm(torch, fn)
                    t[name].append(timed(torch, fn, BATCH))
            m = {name: statistics.median(v) for name, v in t.items()}
            spread = max(t["b"]) - min(t["b"])
            ok_f, ok_d = m["f"] <= m["b"] + spread, m["d"] < m["b"]
            ok_all = ok_all and ok_f and ok_d
            say(f"{cid} k={k}:")
            say(f"  (a) baseline k=1            {fmt(t['a'])}")
            say(f"  (b) baseline k={k} full       {fmt(t['b'])}   = {m['b'] / m['a']:.2f} plain frames, spread {spread:.2f}")
            for name, T in (("c", 256), ("d", 16), ("e", 1)):
                model = 1.0 + share[T] * (k * k - 1)
                say(f"  ({name}) this build k={k} T={T:<3}   {fmt(t[name])}   = {m[name] / m['a']:.2f} plain frames, model "
                    f"{model:.2f} ({m[name] / (model * m['a']):.2f} x the model), {m[name] / m['b']:.3f} of (b)")
            say(f"  (f) this build k={k} T=0     {fmt(t['f'])}   = {m['f'] / m['b']:.3f} of (b)")
            say(f"  bar (f) <= (b) + spread = {m['b'] + spread:.2f}: {'OK' if ok_f else 'SLOWER'};   bar (d) < (b): "
                f"{'OK' if ok_d else 'NOT BELOW'};   (c) / (a) = {m['c'] / m['a']:.3f}")
    say(f"bars: {'both met for every config' if ok_all else 'AT LEAST ONE BAR MISSED'}")

    # C3: lone rt_render_device frames (no bar)
    sc = scenes.config("C3").resized(W, H)
    new.scene(sc)
    base.scene(sc)
    for name, lib, k, T in (("baseline k=1", base, 1, None), ("baseline k=2 full", base, 2, None),
                            ("this build k=2 T=16", new, 2, 16), ("baseline k=4 full", base, 4, None),
                            ("this build k=4 T=16", new, 4, 16), ("this build k=4 T=0", new, 4, 0)):
        lib.sampling(k, T)
        fn = lambda: lib.device(out.data_ptr(), st)  # noqa: E731
        warm(torch, fn, 0.3)  # (past the dispatch-order tuner's probes at k = 1)
        say(f"C3 lone rt_render_device frame, wall with the synchronisation: {name:<20} {timed(torch, fn, 1):8.1f}")
    del out

    # Tick() on C3 at 1080p into a registered frame: synchronous, and two deep with an rt_wait per pair
    from raytracer_hip import Context
    with Context(1) as ctx:
        ctx.set_scene(sc)
        ctx.set_counting(False)
        ctx.set_timing(0)
        hosts = [np.zeros(W * H, dtype=np.int32) for _ in range(2)]
        for hb in hosts:
            ctx.register_host(hb)
        for k, T in ((1, 0), (2, 0), (2, 16), (4, 0), (4, 16)):
            ctx.set_supersampling(k)
            ctx.set_adaptive_sampling(T)

            def sync():
                ctx.render(W, H, hosts[0])

            def pair():
                ctx.render_async(W, H, hosts[0])
                ctx.render_async(W, H, hosts[1])
                ctx.wait()
            warm(torch, sync, 0.1)
            t_s = timed(torch, sync, 1)
            warm(torch, pair, 0.1)
            t_p = timed(torch, pair, 2)
            say(f"Tick C3 {W}x{H} k={k} T={T}: rt_render {t_s:.1f} us per frame ({1e6 / t_s:.0f} fps)   "
                f"rt_render_async two deep {t_p:.1f} us per frame ({1e6 / t_p:.0f} fps)")
        for hb in hosts:
            ctx.unregister_host(hb)
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0 if ok_all else 1


if __name__ == "__main__":
    sys.exit(main())
