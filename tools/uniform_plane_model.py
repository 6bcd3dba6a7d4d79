#!/usr/bin/env python3
"""CPU model (float64, statistics only -- never a parity reference) of the direct kernel's plane-uniform waves
(csrc/rt_kernel.hip trace_tile_direct): the census of a BASELINE config's 8x8 tiles (one wave each) by the primary
hits of their pixels.  A tile is plane-uniform when some pixel pushes a level-0 record (a primary hit with
t - 0.01 > 0) and every such pixel hit the same plane; pixels that miss stay outside the rule.  The other tiles with a
record are split into those with a sphere pixel (silhouettes and sphere interiors) and those with two planes (seams);
tiles without any record are the sky.  Camera at the origin, yaw = pitch = 0 (the configs' camera).  Usage:
  python tools/uniform_plane_model.py [--configs C1,C2,C3] [--size WxH]
"""
import argparse
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "uu-infogr-raytracer_amd"))
from raytracer_hip import scenes  # noqa: E402

TILE = 8


def primary_codes(sc):
    """[H, W] int: -1 no level-0 record, 1000 + i sphere i, k plane k."""
    W, H = sc.width, sc.height
    near, fov = 0.3, 60.0
    ph = near * math.tan(math.radians(fov / 2)) * 2
    pw = ph * (W / H)
    xs, ys = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64))
    d = np.stack([(xs / W - 0.5) * pw, -(ys / H - 0.5) * ph, np.full_like(xs, near)], axis=-1).reshape(-1, 3)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    n = len(d)
    ts, si = np.full(n, np.inf), np.zeros(n, dtype=np.int64)
    if sc.spheres:
        C = np.array([s.center for s in sc.spheres], dtype=np.float64)
        r2 = np.array([s.radius ** 2 for s in sc.spheres], dtype=np.float64)
        b = -2 * d @ C.T
        disc = b * b - 4 * ((C * C).sum(1) - r2)[None]
        with np.errstate(invalid="ignore"):
            t1 = (-b - np.sqrt(np.where(disc >= 0, disc, np.nan))) / 2
        t1 = np.where(t1 > 0, t1, np.inf)
        si = np.argmin(t1, axis=1)
        ts = t1[np.arange(n), si]
    tpl, pi = np.full(n, np.inf), np.zeros(n, dtype=np.int64)
    if sc.planes:
        PC = np.array([p.center for p in sc.planes], dtype=np.float64)
        PN = np.array([p.normal for p in sc.planes], dtype=np.float64)
        with np.errstate(divide="ignore", invalid="ignore"):
            tp = np.einsum("pk,pk->p", PC, PN)[None] / (d @ PN.T)
        tp = np.where(tp > 0, tp, np.inf)
        pi = np.argmin(tp, axis=1)
        tpl = tp[np.arange(n), pi]
    is_s = ts < tpl
    t = np.where(is_s, ts, tpl)
    rec = np.isfinite(t) & (t - 0.01 > 0)
    return np.where(rec, np.where(is_s, 1000 + si, pi), -1).reshape(H, W)


def census(sc):
    code = primary_codes(sc)
    H, W = code.shape
    c = dict(tiles=0, sky=0, uniform=0, sphere=0, seam=0, uniform_px=0, record_px=int((code >= 0).sum()))
    for y0 in range(0, H, TILE):
        for x0 in range(0, W, TILE):
            t = code[y0:y0 + TILE, x0:x0 + TILE]
            kinds = np.unique(t[t >= 0])
            c["tiles"] += 1
            if len(kinds) == 0:
                c["sky"] += 1
            elif len(kinds) == 1 and kinds[0] < 1000:
                c["uniform"] += 1
                c["uniform_px"] += int((t >= 0).sum())
            elif (kinds >= 1000).any():
                c["sphere"] += 1
            else:
                c["seam"] += 1
    return c


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="C1,C2,C3")
    ap.add_argument("--size", default="", help="WxH override")
    a = ap.parse_args()
    for name in a.configs.split(","):
        sc = scenes.config(name)
        if a.size:
            sc = sc.resized(*map(int, a.size.split("x")))
        c = census(sc)
        walking = c["tiles"] - c["sky"]
        print(f"{name} {sc.width}x{sc.height}: {c['tiles']} tiles, {c['sky']} without a level-0 record, {walking} with one: "
              f"{c['uniform']} plane-uniform ({100 * c['uniform'] / max(1, walking):.1f} % of them, "
              f"{100 * c['uniform'] / c['tiles']:.1f} % of all), {c['sphere']} with a sphere pixel, {c['seam']} with two planes; "
              f"{c['uniform_px']} of {c['record_px']} level-0 records ({100 * c['uniform_px'] / max(1, c['record_px']):.1f} %) "
              f"lie in plane-uniform tiles")


if __name__ == "__main__":
    main()
