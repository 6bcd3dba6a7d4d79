#!/usr/bin/env python3
"""CPU model (float64, statistics only -- never a parity reference) of what the dark-tile skip (csrc/rt_dark.h)
can save at the primary level of a BASELINE config: the census of the frame's 8x8 tiles (one wave each).

A wave skips the light loop of a fold step only when no lane of it needs the loop, so what counts is not the share
of dark floor pixels but the share of tiles whose shaded pixels are all dark floor: tiles with floor pixels are
split into entirely dark (no lit floor pixel and no diffuse sphere pixel), entirely lit (no dark floor pixel) and
mixed.  The prediction printed beside the census is DESIGN.md 5's crude model: the shading share of a frame
(0.40 - 0.45, the round-5 split) x the primary level's share of the shaded diffuse hits (--level0-share, 0.83 on
C3) x the entirely dark share of the shading tiles.  Usage:
  python tools/dark_tile_model.py [--configs C2,C3,C4] [--size WxH]
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


def checker_basis(n):
    """RayTracer.cs:760-765 (rt_scene.h scene_build): the checkerboard's e1, e2 of a plane normal."""
    def unit(v):
        with np.errstate(invalid="ignore", divide="ignore"):
            return v / np.linalg.norm(v)
    e1 = unit(np.cross(n, [1.0, 0.0, 0.0]))
    if not e1.any():
        e1 = unit(np.cross(n, [0.0, 0.0, 1.0]))
    return e1, unit(np.cross(n, e1))


def primary_rows(sc, y0, y1):
    """Primary hits of rows [y0, y1) (camera at the origin, yaw = pitch = 0): per pixel (floor, dark, lit) --
    a diffuse plane hit, of those the dark squares, and every other diffuse hit (lit squares, diffuse spheres)."""
    W, H = sc.width, sc.height
    near, fov = 0.3, 60.0
    ph = near * math.tan(math.radians(fov / 2)) * 2
    pw = ph * (W / H)
    xs, ys = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(y0, y1, dtype=np.float64))
    d = np.stack([(xs / W - 0.5) * pw, -(ys / H - 0.5) * ph, np.full_like(xs, near)], axis=-1).reshape(-1, 3)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    n = len(d)
    C = np.array([s.center for s in sc.spheres], dtype=np.float64)
    r2 = np.array([s.radius ** 2 for s in sc.spheres], dtype=np.float64)
    s_diff = np.array([any(s.material.kd) for s in sc.spheres])
    b = -2 * d @ C.T
    disc = b * b - 4 * ((C * C).sum(1) - r2)[None]
    with np.errstate(invalid="ignore"):
        t1 = (-b - np.sqrt(np.where(disc >= 0, disc, np.nan))) / 2
    t1 = np.where(t1 > 0, t1, np.inf)
    si = np.argmin(t1, axis=1)
    ts = t1[np.arange(n), si]
    PC = np.array([p.center for p in sc.planes], dtype=np.float64)
    PN = np.array([p.normal for p in sc.planes], dtype=np.float64)
    p_diff = np.array([any(p.material.kd) for p in sc.planes])
    with np.errstate(divide="ignore", invalid="ignore"):
        tp = np.einsum("pk,pk->p", PC, PN)[None] / (d @ PN.T)
    tp = np.where(tp > 0, tp, np.inf)
    pi = np.argmin(tp, axis=1)
    tpl = tp[np.arange(n), pi]
    is_s = ts < tpl
    t = np.where(is_s, ts, tpl)
    hit = np.isfinite(t) & (t - 0.01 > 0)
    hp = d * np.where(hit, t, 0.0)[:, None]
    tile = np.ones(n, dtype=np.int64)
    for k, p in enumerate(sc.planes):
        e1, e2 = checker_basis(np.array(p.normal, dtype=np.float64))
        with np.errstate(invalid="ignore"):
            u, v = np.nan_to_num(hp @ e1), np.nan_to_num(hp @ e2)  # (a NaN basis: (int)NaN + (int)NaN is even)
        tile = np.where(pi == k, (np.trunc(u).astype(np.int64) + np.trunc(v).astype(np.int64)) & 1, tile)
    floor = hit & ~is_s & p_diff[pi]
    dark = floor & (tile == 0)
    lit = (floor & ~dark) | (hit & is_s & s_diff[si])
    shape = (y1 - y0, W)
    return floor.reshape(shape), dark.reshape(shape), lit.reshape(shape)


def tiles_any(a, W):
    """[rows <= 8, W] -> per 8-column tile: any pixel set."""
    pad = (-W) % TILE
    a = np.pad(a, ((0, 0), (0, pad)))
    return a.reshape(a.shape[0], -1, TILE).any(axis=(0, 2))


def census(sc):
    W, H = sc.width, sc.height
    c = dict(tiles=0, floor=0, dark=0, lit=0, mixed=0, shading=0, dark_px=0, dark_px_in_dark_tiles=0, diffuse_px=0)
    for y0 in range(0, H, TILE):
        y1 = min(H, y0 + TILE)
        floor, dark, lit = primary_rows(sc, y0, y1)
        tf, td, tl = tiles_any(floor, W), tiles_any(dark, W), tiles_any(lit, W)
        all_dark = td & ~tl
        c["tiles"] += len(tf)
        c["floor"] += int(tf.sum())
        c["dark"] += int(all_dark.sum())
        c["lit"] += int((tf & ~td).sum())
        c["mixed"] += int((tf & td & tl).sum())
        c["shading"] += int((td | tl).sum())
        c["dark_px"] += int(dark.sum())
        c["diffuse_px"] += int(dark.sum() + lit.sum())
        pad = (-W) % TILE
        per_tile = np.pad(dark, ((0, 0), (0, pad))).reshape(dark.shape[0], -1, TILE).sum(axis=(0, 2))
        c["dark_px_in_dark_tiles"] += int(per_tile[all_dark].sum())
    return c


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="C2,C3,C4")
    ap.add_argument("--size", default="", help="WxH override")
    ap.add_argument("--level0-share", type=float, default=0.83,
                    help="the primary level's share of the shaded diffuse hits (C3: 0.83)")
    a = ap.parse_args()
    for name in a.configs.split(","):
        sc = scenes.config(name)
        if a.size:
            sc = sc.resized(*map(int, a.size.split("x")))
        c = census(sc)
        f = c["dark"] / max(1, c["shading"])
        print(f"{name} {sc.width}x{sc.height}: {c['tiles']} tiles, {c['shading']} shade a diffuse hit, {c['floor']} "
              f"carry floor pixels: {c['dark']} entirely dark, {c['lit']} entirely lit, {c['mixed']} mixed; "
              f"dark floor pixels {c['dark_px']} of {c['diffuse_px']} diffuse primary hits "
              f"({100 * c['dark_px'] / max(1, c['diffuse_px']):.1f} %), "
              f"{100 * c['dark_px_in_dark_tiles'] / max(1, c['dark_px']):.0f} % of them in entirely dark tiles")
        lo, hi = 0.40 * a.level0_share * f, 0.45 * a.level0_share * f
        print(f"  entirely dark share of the shading tiles {f:.3f}; model: {100 * lo:.1f} - {100 * hi:.1f} % of a "
              f"frame, less the guard")


if __name__ == "__main__":
    main()
