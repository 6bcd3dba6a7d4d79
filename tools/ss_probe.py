"""Does fused supersampling cost less than what a user had to do before -- render k W x k H and shrink it?

    python tools/ss_probe.py --baseline-lib PATH/libraytracer_hip.so [--repeats 7] [--out profiles/ss_probe.txt]

Gated comparison (wall clock per frame, counters off, one launch in flight): 64-frame rt_render_bands_batch
launches in FRAME format,
    ss    this build at width x height with rt_set_supersampling(k)  -- traces k*k samples per pixel, stores one;
    base  the baseline library (a build of the parent commit) rendering the plain k width x k height frame
          -- the same samples, every one stored, and the shrink still to do.
Both legs run in one process, alternating, each after a warm-up of at least 50 ms.  Expectation: the ss median
is at most the baseline's median plus the baseline's own spread (max - min of its repeats).
Also reported, with no bar: lone rt_render_device frames (supersampled ones run in natural tile order, the
plain ones under the dispatch-order tuner), and Tick() -- rt_render, and rt_render_async two deep -- at k = 1,
2, 4 on C3 at 1080p into a registered host frame.
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
W, H = 1920, 1080


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

    def batch(self, w, h, d_ptr, stream):
        rc = self.lib.rt_render_bands_batch(self.ctx, w, h, h, 0, 1, BATCH, C.c_void_p(d_ptr), w * h * 4,
                                            self.abi.RT_BANDS_FRAME, C.c_void_p(stream), None)
        assert rc == 0, self.lib.rt_last_error(self.ctx)

    def device(self, w, h, d_ptr, stream):
        assert self.lib.rt_render_device(self.ctx, w, h, C.c_void_p(d_ptr), C.c_void_p(stream)) == 0


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--baseline-lib", required=True)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert a.repeats >= 5
    import numpy as np
    import torch
    from raytracer_hip import abi, scenes
    torch.cuda.set_device(0)
    st = torch.cuda.current_stream().cuda_stream
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    new, base = Lib(None, abi), Lib(a.baseline_lib, abi)
    say(f"ss_probe: {BATCH}-frame rt_render_bands_batch launches (FRAME), one in flight, counters off, {W}x{H} output; "
        f"{a.repeats} alternating repeats; us per frame")
    ok_all = True
    for cid, ks in (("C3", (2, 4)), ("C4", (2,))):
        sc = scenes.config(cid).resized(W, H)
        new.scene(sc)
        base.scene(sc)
        for k in ks:
            kw, kh = k * W, k * H
            out_ss = torch.empty(BATCH * W * H, dtype=torch.int32, device="cuda")
            out_b = torch.empty(BATCH * kw * kh, dtype=torch.int32, device="cuda")
            assert new.lib.rt_set_supersampling(new.ctx, k) == 0
            f_ss = lambda: new.batch(W, H, out_ss.data_ptr(), st)  # noqa: E731
            f_b = lambda: base.batch(kw, kh, out_b.data_ptr(), st)  # noqa: E731
            t_ss, t_b = [], []
            for _ in range(a.repeats):
                warm(torch, f_ss)
                t_ss.append(timed(torch, f_ss, BATCH))
                warm(torch, f_b)
                t_b.append(timed(torch, f_b, BATCH))
            # the plain k = 1 frame of this build, for scale
            assert new.lib.rt_set_supersampling(new.ctx, 1) == 0
            f_1 = lambda: new.batch(W, H, out_ss.data_ptr(), st)  # noqa: E731
            warm(torch, f_1)
            t_1 = timed(torch, f_1, BATCH)
            m_ss, m_b = statistics.median(t_ss), statistics.median(t_b)
            spread = max(t_b) - min(t_b)
            ok = m_ss <= m_b + spread
            ok_all = ok_all and ok
            say(f"{cid} k={k}: ss {m_ss:9.2f} (min {min(t_ss):.2f} max {max(t_ss):.2f})   baseline {kw}x{kh} {m_b:9.2f} "
                f"(min {min(t_b):.2f} max {max(t_b):.2f}, spread {spread:.2f})   ss/baseline {m_ss / m_b:.3f}   "
                f"{'OK' if ok else 'SLOWER'} (bar {m_b + spread:.2f});   k=1 {W}x{H} {t_1:.2f}")
            # lone frames (no bar): supersampled in natural tile order, the baseline's kW x kH under its order tuner
            assert new.lib.rt_set_supersampling(new.ctx, k) == 0
            g_ss = lambda: new.device(W, H, out_ss.data_ptr(), st)  # noqa: E731
            g_b = lambda: base.device(kw, kh, out_b.data_ptr(), st)  # noqa: E731
            warm(torch, g_ss, 0.1)
            l_ss = timed(torch, g_ss, 1)
            warm(torch, g_b, 0.3)  # (past the tuner's probes)
            l_b = timed(torch, g_b, 1)
            say(f"{cid} k={k}: lone rt_render_device frame, wall with the synchronisation: ss {l_ss:.1f}   baseline {kw}x{kh} {l_b:.1f}")
            del out_ss, out_b
    say(f"gated comparison: {'every ss median within the bar' if ok_all else 'AT LEAST ONE ss MEDIAN ABOVE THE BAR'}")

    # Tick() on C3 at 1080p into a registered frame: synchronous, and two deep with an rt_wait per pair
    from raytracer_hip import Context
    sc = scenes.config("C3").resized(W, H)
    with Context(1) as ctx:
        ctx.set_scene(sc)
        ctx.set_counting(False)
        ctx.set_timing(0)
        hosts = [np.zeros(W * H, dtype=np.int32) for _ in range(2)]
        for hb in hosts:
            ctx.register_host(hb)
        for k in (1, 2, 4):
            ctx.set_supersampling(k)

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
            say(f"Tick C3 {W}x{H} k={k}: rt_render {t_s:.1f} us per frame ({1e6 / t_s:.0f} fps)   "
                f"rt_render_async two deep {t_p:.1f} us per frame ({1e6 / t_p:.0f} fps)")
        for hb in hosts:
            ctx.unregister_host(hb)
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0 if ok_all else 1


if __name__ == "__main__":
    sys.exit(main())
