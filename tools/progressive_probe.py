"""What does progressive accumulation (rt_set_progressive) cost a display loop?

    python tools/progressive_probe.py [--baseline-lib PATH/libraytracer_hip.so] [--k 4] [--repeats 7]
                                      [--out profiles/ab/progressive_probe.txt]

Tick() into a registered frame, counters and timing off, C3 at 1920x1080 and C4 at 3840x2160, in one process; wall
clock per Tick in us, median of the repeats with min and max.
  Moving camera (every Tick has another camera, so every Tick is P_1 and runs the plain launch): the loop with
    rt_set_progressive(k) against the same loop with it off, alternating, synchronous (rt_render) and two deep
    (pairs of rt_render_async with an rt_wait).  The launches are identical by construction; the gap is reported beside
    the off runs' own spread (max - min of their repeats).
  Resting camera, synchronous: the Tick that outputs P_2 (two samples, starts the accumulator), the Ticks for P_3 ..
    P_{k*k} (one sample), and the converged Tick (no trace, emits from the accumulator), each against the plain Tick of
    this session -- and, with --baseline-lib, against the plain Tick of that build (the parent commit) in this session.
  Resting camera, two deep: a whole run of k*k Ticks from a restart, per Tick, and converged pairs.
No bars: the figures go to the file named by --out.
"""
import argparse
import ctypes as C
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "uu-infogr-raytracer_amd"))

CONFIGS = (("C3", 1920, 1080), ("C4", 3840, 2160))


def fmt(ts):
    return f"{statistics.median(ts):9.1f} (min {min(ts):.1f} max {max(ts):.1f})"


class Loop:
    """A context of one build with a scene and two registered frames (a baseline build lacks the newer entry points)."""

    def __init__(self, abi, path, sc, W, H, np):
        self.abi, self.W, self.H = abi, W, H
        self.lib = abi.load_library(os.path.abspath(path), local=True) if path else abi.load_library()
        self.ctx = C.c_void_p()
        assert self.lib.rt_create(1, C.byref(self.ctx)) == 0, self.lib.rt_last_error(None)
        assert self.lib.rt_set_counting(self.ctx, 0) == 0 and self.lib.rt_set_timing(self.ctx, 0) == 0
        S, P, L = sc.c_arrays()
        assert self.lib.rt_set_scene(self.ctx, S, len(sc.spheres), P, len(sc.planes), L, len(sc.lights),
                                     abi.rt_vec3(*sc.ambient), sc.recursion_limit) == 0
        self.cam = sc.c_camera()
        self.x0 = self.cam.position.x
        self.step = 0
        self.set_camera()
        self.hosts = [np.zeros(W * H, dtype=np.int32) for _ in range(2)]
        for hb in self.hosts:
            assert self.lib.rt_register_host(self.ctx, hb.ctypes.data_as(C.c_void_p), hb.nbytes) == 0

    def close(self):
        for hb in self.hosts:
            self.lib.rt_unregister_host(self.ctx, hb.ctypes.data_as(C.c_void_p))
        self.lib.rt_destroy(self.ctx)

    def set_camera(self):
        assert self.lib.rt_set_camera(self.ctx, C.byref(self.cam)) == 0

    def move(self):
        """Another camera than the last Tick's: a sideways step of 2^-10, back and forth (the view stays the scene's)."""
        self.step ^= 1
        self.cam.position.x = self.x0 + self.step / 1024.0
        self.set_camera()

    def rest(self):
        self.cam.position.x = self.x0
        self.step = 0
        self.set_camera()

    def progressive(self, k):
        assert self.lib.rt_set_progressive(self.ctx, k) == 0, self.lib.rt_last_error(self.ctx)

    def restart(self):
        assert self.lib.rt_reset_progressive(self.ctx) == 0

    def count(self):
        k, c = C.c_int(), C.c_int()
        assert self.lib.rt_get_progressive(self.ctx, C.byref(k), C.byref(c)) == 0
        return c.value

    def tick(self, slot=0):
        rc = self.lib.rt_render(self.ctx, self.W, self.H, self.hosts[slot].ctypes.data_as(C.c_void_p))
        assert rc == 0, self.lib.rt_last_error(self.ctx)

    def tick_async(self, slot):
        rc = self.lib.rt_render_async(self.ctx, self.W, self.H, self.hosts[slot].ctypes.data_as(C.c_void_p))
        assert rc == 0, self.lib.rt_last_error(self.ctx)

    def wait(self):
        assert self.lib.rt_wait(self.ctx) == 0


def wall(fn, ticks_per_call, min_s=0.25, warm_s=0.1):
    """us per Tick of back-to-back calls of fn over >= min_s, after a warm-up."""
    t0 = time.perf_counter()
    while time.perf_counter() - t0 < warm_s:
        fn()
    n, t0 = 0, time.perf_counter()
    while True:
        fn()
        n += 1
        dt = time.perf_counter() - t0
        if dt >= min_s and n >= 3:
            return dt / (n * ticks_per_call) * 1e6


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--baseline-lib", default=None)
    ap.add_argument("--k", type=int, default=4)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert a.repeats >= 5 and a.k in (2, 4, 8)
    import numpy as np
    import torch

    from raytracer_hip import abi, scenes
    torch.cuda.set_device(0)
    k, kk = a.k, a.k * a.k
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    say(f"progressive_probe: Tick() into a registered frame, one GPU, counters and timing off, k = {k}; {a.repeats} repeats; "
        f"us per Tick, median (min max)")
    for cid, W, H in CONFIGS:
        sc = scenes.config(cid).resized(W, H)
        new = Loop(abi, None, sc, W, H, np)
        base = Loop(abi, a.baseline_lib, sc, W, H, np) if a.baseline_lib else None
        say(f"{cid} {W}x{H}:")

        # ---- moving camera: on against off, alternating ----
        def moving_sync(lp):
            lp.move()
            lp.tick()

        def moving_pair(lp):
            for slot in (0, 1):
                lp.move()
                lp.tick_async(slot)
            lp.wait()
        for name, fn, per in (("rt_render", moving_sync, 1), ("rt_render_async two deep", moving_pair, 2)):
            t = {"off": [], "on": [], "parent": []}
            for _ in range(a.repeats):
                new.progressive(1)
                t["off"].append(wall(lambda: fn(new), per))
                new.progressive(k)
                t["on"].append(wall(lambda: fn(new), per))
                assert new.count() == 1, "a moving camera's Ticks are all P_1"
                if base:
                    t["parent"].append(wall(lambda: fn(base), per))
            new.progressive(1)
            m_off, m_on = statistics.median(t["off"]), statistics.median(t["on"])
            say(f"  moving camera, {name}:")
            say(f"    off            {fmt(t['off'])}   spread {max(t['off']) - min(t['off']):.1f}")
            say(f"    on             {fmt(t['on'])}   on - off = {m_on - m_off:+.1f} ({(m_on / m_off - 1) * 100:+.2f} %)")
            if base:
                say(f"    parent build   {fmt(t['parent'])}   off / parent = {m_off / statistics.median(t['parent']):.3f}")

        # ---- resting camera, synchronous: one run per repeat, every Tick timed on its own ----
        new.rest()
        new.progressive(1)
        plain = [wall(new.tick, 1) for _ in range(a.repeats)]
        parent = [wall(base.tick, 1) for _ in range(a.repeats)] if base else None
        new.progressive(k)
        p2, mid, conv = [], [], []
        for _ in range(a.repeats):
            new.restart()
            per_tick = []
            for _n in range(kk + 8):
                t0 = time.perf_counter()
                new.tick()
                per_tick.append((time.perf_counter() - t0) * 1e6)
            assert new.count() == kk
            p2.append(per_tick[1])
            mid.append(statistics.median(per_tick[2:kk]))
            conv.append(statistics.median(per_tick[kk:]))
        m_plain = statistics.median(plain)
        say("  resting camera, rt_render:")
        say(f"    plain Tick (off)       {fmt(plain)}")
        if parent:
            say(f"    plain Tick, parent     {fmt(parent)}   off / parent = {m_plain / statistics.median(parent):.3f}")
        for name, ts in ((f"Tick for P_2            ", p2), (f"Ticks for P_3..P_{kk}   ", mid), ("converged Tick         ", conv)):
            line = f"    {name}{fmt(ts)}   = {statistics.median(ts) / m_plain:.2f} plain Ticks"
            if parent:
                line += f", {statistics.median(ts) / statistics.median(parent):.2f} of the parent's"
            say(line)

        # ---- resting camera, two deep ----
        def run_pairs():
            new.restart()
            for n in range(kk):
                new.tick_async(n % 2)
                if n % 2:
                    new.wait()
            new.wait()

        def conv_pair():
            new.tick_async(0)
            new.tick_async(1)
            new.wait()
        run = [wall(run_pairs, kk) for _ in range(a.repeats)]
        run_pairs()
        cp = [wall(conv_pair, 2) for _ in range(a.repeats)]
        new.progressive(1)
        pl2 = [wall(conv_pair, 2) for _ in range(a.repeats)]
        say("  resting camera, rt_render_async two deep:")
        say(f"    plain Tick (off)       {fmt(pl2)}")
        say(f"    a run of {kk} Ticks     {fmt(run)}   per Tick = {statistics.median(run) / statistics.median(pl2):.2f} plain Ticks")
        say(f"    converged Tick         {fmt(cp)}   = {statistics.median(cp) / statistics.median(pl2):.2f} plain Ticks")
        new.close()
        if base:
            base.close()
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
