#!/usr/bin/env python3
"""CPU model (float64, statistics only -- never a parity reference) of the shadow pre-test's group and union records
(csrc/rt_scene.h build_shadow_groups, csrc/rt_kernel.hip shadow_scan's GROUPS) on a BASELINE config seen from its
camera (origin, yaw = pitch = 0).  The tiles come from tools/uniform_plane_model.py; a lane scans when its floor
square is lit (the checkerboard's ((int)u + (int)v) & 1, in float64) and a wave when some lane does.  Per light it
reports, for the scanning plane-uniform waves and for the tiles with sphere pixels (their plane lanes only: the
per-lane fold), how many waves keep any sphere, the union and each group, and the expected per-lane pre-tests per scan
(out of S) of four schemes for G = 1..4 groups:
  flat         the G group records, then the kept groups' members
  union-first  the union; if kept, the G group records, then the kept groups' members
both in the kernel's unit of skipping, the sphere pair, and per single sphere.  The records follow the builder: the
pre-test's margins, complete-linkage merging, discs around the smallest enclosing disc's centre, radii inflated by
2^-16, lane margins widened by 2^-10 (groups) and 2^-9 (union).  Usage:
  python tools/shadow_group_model.py [--configs C3] [--size WxH]
"""
import argparse
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "uu-infogr-raytracer_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from raytracer_hip import scenes  # noqa: E402
from shadow_cull_model import light_frame  # noqa: E402
from uniform_plane_model import TILE, primary_codes  # noqa: E402


def pre_records(sc, frame):
    """[S, 4] (cu, cv, ca', rr') of build_shadow_pre for one light."""
    U, V, A = frame
    out = []
    for s in sc.spheres:
        c = np.asarray(s.center, dtype=np.float64)
        cu, cv, ca = c @ U, c @ V, c @ A
        mc = 2.0 ** -8 * (abs(cu) + abs(cv) + abs(ca)) * (1 + 2.0 ** -20)
        rr = abs(s.radius) * (1 + 2.0 ** -8)
        out.append((cu, cv, ca + mc, rr + 2.0 ** -18 * np.linalg.norm(c) + mc))
    return np.array(out, dtype=np.float64).reshape(-1, 4)


def enclosing_centre(x, y, r):
    """Centre of the smallest disc containing the discs (x, y, r): convex minimisation of max_i |c - c_i| + r_i."""
    def far(px, py):
        return float(np.max(np.hypot(x - px, y - py) + r))

    def best_y(px):
        lo, hi = float(y.min()), float(y.max())
        for _ in range(48):
            a, b = lo + (hi - lo) / 3, hi - (hi - lo) / 3
            if far(px, a) <= far(px, b):
                hi = b
            else:
                lo = a
        return far(px, (lo + hi) / 2), (lo + hi) / 2

    lo, hi = float(x.min()), float(x.max())
    for _ in range(48):
        a, b = lo + (hi - lo) / 3, hi - (hi - lo) / 3
        if best_y(a)[0] <= best_y(b)[0]:
            hi = b
        else:
            lo = a
    px = (lo + hi) / 2
    return px, best_y(px)[1]


def enclose(recs):
    """The record around `recs` ([n, 4]): shadow_enclose."""
    cx, cy = enclosing_centre(recs[:, 0], recs[:, 1], recs[:, 3])
    rr = float(np.max(np.hypot(recs[:, 0] - cx, recs[:, 1] - cy) + recs[:, 3])) * (1 + 2.0 ** -16)
    return np.array([cx, cy, recs[:, 2].max(), rr])


def group_members(recs, G):
    """Complete-linkage merging on the pair span (d + rr_i + rr_j) / 2 down to at most G groups: lists of indices."""
    cl = [[i] for i in range(len(recs))]

    def span(a, b):
        return max(0.5 * (math.hypot(recs[p, 0] - recs[q, 0], recs[p, 1] - recs[q, 1]) + recs[p, 3] + recs[q, 3]) for p in a for q in b)

    while len(cl) > max(G, 1):
        _, a, b = min((span(cl[a], cl[b]), a, b) for a in range(len(cl)) for b in range(a + 1, len(cl)))
        cl[a] += cl.pop(b)
    return cl


def lane_records(hp, frame):
    U, V, A = frame
    ou, ov, oa = hp @ U, hp @ V, hp @ A
    ml = (abs(ou) + abs(ov) + abs(oa)) * (2.0 ** -8) * (1 + 2.0 ** -8) + 2.0 ** -30
    return ou, ov, oa, ml


def keep(q, rec, widen=1.0):
    """[lanes] bool: shadow_pre_keep of one record."""
    ou, ov, oa, ml = q
    ml = ml * widen
    line = (rec[0] - ou) ** 2 + (rec[1] - ov) ** 2 > (rec[3] + ml) ** 2
    return ~(line | (oa - rec[2] > ml))


def floor_points(sc):
    """[H, W, 3] hit points of the primary rays on plane 0 and [H, W] whether the square is lit."""
    W, H = sc.width, sc.height
    near, fov = 0.3, 60.0
    ph = near * math.tan(math.radians(fov / 2)) * 2
    pw = ph * (W / H)
    xs, ys = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64))
    d = np.stack([(xs / W - 0.5) * pw, -(ys / H - 0.5) * ph, np.full_like(xs, near)], axis=-1)
    d /= np.linalg.norm(d, axis=-1, keepdims=True)
    pl = sc.planes[0]
    n = np.asarray(pl.normal, dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        t = (np.asarray(pl.center, dtype=np.float64) @ n) / (d @ n)
    hp = d * t[..., None]
    e1 = np.cross(n, [1.0, 0.0, 0.0])
    if not e1.any():
        e1 = np.cross(n, [0.0, 0.0, 1.0])
    e1 /= np.linalg.norm(e1)
    e2 = np.cross(n, e1)
    e2 /= np.linalg.norm(e2)
    with np.errstate(invalid="ignore"):
        lit = ((np.trunc(hp @ e1) + np.trunc(hp @ e2)) % 2) != 0
    return hp, lit


def census(sc, out=print):
    code = primary_codes(sc)
    hp, lit = floor_points(sc)
    H, W = code.shape
    S = len(sc.spheres)
    frames = [light_frame(l.position) for l in sc.lights]
    pres = [pre_records(sc, f) for f in frames]
    hier = {}  # (light, G) -> (members, group records, union record)
    for li, pre in enumerate(pres):
        for G in (1, 2, 3, 4):
            mem = group_members(pre, G)
            grp = [enclose(pre[m]) for m in mem]
            hier[li, G] = (mem, grp, enclose(np.array(grp)))
    kinds = {"plane-uniform": [], "with sphere pixels": []}
    for y0 in range(0, H, TILE):
        for x0 in range(0, W, TILE):
            t = code[y0:y0 + TILE, x0:x0 + TILE]
            k = np.unique(t[t >= 0])
            if len(k) == 1 and k[0] == 0:
                kinds["plane-uniform"].append((y0, x0))
            elif (k >= 1000).any() and (k == 0).any():
                kinds["with sphere pixels"].append((y0, x0))
    for kind, tiles in kinds.items():
        scanning = 0
        stat = {li: dict(any=0, spheres=0, union=0, groups=np.zeros(SCHEME_G), flat=np.zeros((5, 2)), ufirst=np.zeros((5, 2)))
                for li in range(len(frames))}
        for y0, x0 in tiles:
            sel = (code[y0:y0 + TILE, x0:x0 + TILE] == 0) & lit[y0:y0 + TILE, x0:x0 + TILE]
            if not sel.any():
                continue
            scanning += 1
            pts = hp[y0:y0 + TILE, x0:x0 + TILE][sel]
            for li, frame in enumerate(frames):
                q = lane_records(pts, frame)
                kept = np.array([keep(q, pres[li][i]).any() for i in range(S)], dtype=bool)
                st = stat[li]
                st["any"] += bool(kept.any())
                st["spheres"] += int(kept.sum())
                for G in (1, 2, 3, 4):
                    mem, grp, uni = hier[li, G]
                    ku = bool(keep(q, uni, 1 + 2.0 ** -9).any())
                    kg = [bool(keep(q, g, 1 + 2.0 ** -10).any()) for g in grp]
                    assert all(kg[g] for g, m in enumerate(mem) if kept[m].any()) and (ku or not any(kg)), "containment"
                    live = np.zeros(S, dtype=bool)
                    for g, m in enumerate(mem):
                        if kg[g]:
                            live[m] = True
                    pairs = 2 * int((live[0::2][:len(live[1::2])] | live[1::2]).sum()) + (int(live[-1]) if S & 1 else 0)
                    for col, members in enumerate((pairs, int(live.sum()))):
                        st["flat"][G, col] += len(grp) + members
                        st["ufirst"][G, col] += 1 + (len(grp) + members if ku else 0)
                    if G == SCHEME_G:
                        st["union"] += ku
                        st["groups"][:len(grp)] += kg
        out(f"{sc.name} {W}x{H} {kind}: {len(tiles)} tiles, {scanning} with a lit floor lane (they scan); S = {S}, flat pair loop = {S} pre-tests per scan")
        n = max(1, scanning)
        for li in range(len(frames)):
            st = stat[li]
            mem = hier[li, SCHEME_G][0]
            out(f"  light {li}: some lane keeps some sphere in {st['any']} waves ({100 * st['any'] / n:.1f} %), {st['spheres'] / n:.3f} spheres per wave; "
                f"G = {SCHEME_G} groups {mem}: union kept in {100 * st['union'] / n:.1f} %, groups in "
                + ", ".join(f"{100 * v / n:.1f} %" for v in st["groups"][:len(mem)]))
            for G in (1, 2, 3, 4):
                out(f"    G = {G}: pre-tests per scan, skipping pairs (single spheres): flat {st['flat'][G, 0] / n:.2f} ({st['flat'][G, 1] / n:.2f}), "
                    f"union-first {st['ufirst'][G, 0] / n:.2f} ({st['ufirst'][G, 1] / n:.2f})")


SCHEME_G = 3  # rt_internal.h SHADOW_GROUPS


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="C3")
    ap.add_argument("--size", default="", help="WxH override")
    a = ap.parse_args()
    for name in a.configs.split(","):
        sc = scenes.config(name)
        if a.size:
            sc = sc.resized(*map(int, a.size.split("x")))
        census(sc)


if __name__ == "__main__":
    main()
