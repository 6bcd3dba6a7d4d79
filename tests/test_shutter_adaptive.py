"""rt_set_shutter_adaptive_sampling without a device: the numpy definition (supersample.shutter_adaptive_resolve) against a
plain-loops restatement, the wrappers and prototypes, and the preconditions of every case of
tests/test_gpu_shutter_adaptive.py on the unchanged oracle -- conditions that keep a wrong kernel from passing there:
every output frame has refined and flat tiles; its mask differs from the mask of each of its own sub-frames' plain frames
(a kernel that decides on one sub-frame fails) and, in some frame of the case, from their OR; the expectation differs
from both the factor-1 shutter frame P and the fully supersampled S; sample (0, 0) of the k W x k H frame is the plain
pixel.  The saturation case claims only the full-width sum: both of its tiles are refined."""
import numpy as np
import pytest

import anim_shutter_cases as ashut
import shutter_adaptive_cases as sa
from raytracer_hip import Context, abi, path
from raytracer_hip.supersample import TILE, path_resolve, refine_mask, shutter_adaptive_resolve


def loops_resolve(plain, big, k, m, T):
    """The header's definition in plain loops over frames, tiles, pixels and channels."""
    F, H, W = plain.shape[0] // m, plain.shape[1], plain.shape[2]
    out = np.zeros((F, H, W), dtype=np.int32)
    ch = lambda v, s: (int(v) >> s) & 0xFF
    for f in range(F):
        P = np.zeros((H, W), dtype=np.int64)
        S = np.zeros((H, W), dtype=np.int64)
        for y in range(H):
            for x in range(W):
                for s in (16, 8, 0):
                    P[y, x] |= ((sum(ch(plain[f * m + j, y, x], s) for j in range(m)) + m // 2) // m) << s
                    tot = sum(ch(big[f * m + j, k * y + b, k * x + a], s) for j in range(m) for b in range(k) for a in range(k))
                    S[y, x] |= ((tot + m * k * k // 2) // (m * k * k)) << s
        for ty in range(0, H, TILE):
            for tx in range(0, W, TILE):
                ys, xs = range(ty, min(ty + TILE, H)), range(tx, min(tx + TILE, W))
                refined = T > 0 and any(
                    abs(ch(P[y, x], s) - ch(P[y2, x2], s)) >= T
                    for y in ys for x in xs for y2, x2 in ((y, x + 1), (y + 1, x)) if y2 in ys and x2 in xs for s in (16, 8, 0))
                for y in ys:
                    for x in xs:
                        out[f, y, x] = S[y, x] if refined or T == 0 else P[y, x]
    return out


@pytest.mark.parametrize("m,k,T", [(2, 2, 40), (4, 2, 24), (2, 4, 1), (2, 2, 256), (2, 2, 0), (1, 2, 40)])
def test_definition_against_plain_loops(m, k, T):
    rng = np.random.default_rng(7 * m + k + T)
    H, W, F = 11, 13, 2
    # smooth frames with a few edges, so that thresholds split the tiles
    base = rng.integers(0, 256, size=(F * m, 3, 3, 3))
    big = np.zeros((F * m, k * H, k * W), dtype=np.int32)
    for j in range(F * m):
        up = np.kron(base[j], np.ones((1, -(-k * H // 3), -(-k * W // 3)), dtype=np.int64))[:, :k * H, :k * W]
        up = (up + rng.integers(0, 12 if T != 1 else 1, size=up.shape)) & 0xFF
        big[j] = (up[0] << 16) | (up[1] << 8) | up[2]
    plain = big[:, ::k, ::k].copy()
    got = shutter_adaptive_resolve(plain, big, k, m, T)
    assert got.dtype == np.int32 and np.array_equal(got, loops_resolve(plain, big, k, m, T))
    if T == 0:
        assert np.array_equal(got, path_resolve(big, k, m))
    if T == 256:
        assert np.array_equal(got, path.shutter_mean(plain, m))


def test_definition_refuses_bad_arguments():
    p, s = np.zeros((2, 8, 8), dtype=np.int32), np.zeros((2, 16, 16), dtype=np.int32)
    for bad in (lambda: shutter_adaptive_resolve(p, s, 2, 2, 257), lambda: shutter_adaptive_resolve(p, s, 3, 2, 8),
                lambda: shutter_adaptive_resolve(p, s, 2, 3, 8), lambda: shutter_adaptive_resolve(p, s[:1], 2, 2, 8),
                lambda: shutter_adaptive_resolve(p, s, 4, 2, 8), lambda: shutter_adaptive_resolve(p[0], s[0], 2, 2, 8)):
        with pytest.raises(ValueError):
            bad()


def test_prototypes_and_wrappers_exist():
    names = [p[0] for p in abi.PROTOTYPES] if hasattr(abi, "PROTOTYPES") else None
    src = open(abi.__file__).read()
    assert '"rt_set_shutter_adaptive_sampling", C.c_int, [C.c_void_p, C.c_int]' in src
    assert '"rt_get_shutter_adaptive_sampling", C.c_int, [C.c_void_p, C.POINTER(C.c_int)]' in src
    assert names is None or "rt_set_shutter_adaptive_sampling" in names
    assert callable(Context.set_shutter_adaptive_sampling) and callable(Context.get_shutter_adaptive_sampling)
    assert abi.RT_ABI_VERSION == 10


def test_header_states_the_setting_and_keeps_the_refusal():
    import os
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "raytracer_hip.h")).read()
    assert "int rt_set_shutter_adaptive_sampling(rt_ctx* ctx, int threshold);" in hdr
    assert "int rt_get_shutter_adaptive_sampling(const rt_ctx* ctx, int* out_threshold);" in hdr
    assert "which is not built" in hdr and "while rt_set_shutter_adaptive_sampling's threshold is 0" in hdr


def check_facts(facts, what, saturation=False):
    or_differs = False
    for f, (mask, sub_masks, ne_p, ne_s) in enumerate(facts):
        if saturation:
            assert mask.all(), f"{what} frame {f}: every tile is refined"
            continue
        assert mask.any() and not mask.all(), f"{what} frame {f}: {int(mask.sum())} of {mask.size} tiles refined"
        for s, sm in enumerate(sub_masks):
            assert (sm != mask).any(), f"{what} frame {f}: sub-frame {s}'s own mask is the mean's"
        or_differs |= bool((np.logical_or.reduce(sub_masks) != mask).any())
        assert ne_p > 0 and ne_s > 0, f"{what} frame {f}: the expectation is P or S ({ne_p}, {ne_s} pixels differ)"
    assert saturation or or_differs, f"{what}: the mask is the OR of the sub-frames' masks in every frame"


@pytest.mark.parametrize("case", sa.CAMERA_CASES, ids=lambda c: f"{c[0]}-m{c[3]}-k{c[4]}")
def test_camera_cases_hold_their_preconditions(oracle, case):
    cid, W, H, m, k, T, n = case
    sc = sa.pc.scene(cid, W, H)
    _, plain, big, _, _ = sa.camera_subframes(oracle, sc, k, n * m)
    assert np.array_equal(big[:, ::k, ::k], plain), "sample (0, 0) of every block is the plain pixel"
    check_facts(sa.facts(plain, big, m, k, T), f"{cid} m={m} k={k} T={T}")


@pytest.mark.parametrize("name", list(sa.TRACKS) + ["saturation"])
def test_track_cases_hold_their_preconditions(oracle, name):
    m, k, T, first = sa.track_case(name)
    plain, big, _, _ = sa.track_subframes(oracle, sa.track(name), k, first, m)
    assert len(plain) >= m and np.array_equal(big[:, ::k, ::k], plain)
    facts = sa.facts(plain, big, m, k, T)
    check_facts(facts, f"track {name}", saturation=name == "saturation")
    if name == "saturation":
        want = shutter_adaptive_resolve(plain, big, k, m, T)
        assert m * k * k == 256 and int(((want[0] >> 16) == 255).sum()) >= 30, "refined pixels whose red sum is 256 x 255"
        for T2 in (8, 64):
            assert refine_mask(path.shutter_mean(plain, m)[0], T2).all()


def test_view_height_case_holds_its_preconditions(oracle):
    sc = sa.pc.scene("C3", sa.W0, sa.H0)
    _, plain, big, _, _ = sa.camera_subframes(oracle, sc, sa.K0, 3 * sa.M0, sa.VIEW_ROWS, sa.H0)
    assert plain.shape[1] == sa.VIEW_ROWS
    check_facts(sa.facts(plain, big, sa.M0, sa.K0, sa.T0), "27 rows of the 30-row view")


def test_track_expectations_differ_from_wrong_scene_renders(oracle):
    for name in ("direct_m2", "direct_first1"):
        m, k, T, first = sa.track_case(name)
        tr = sa.track(name)
        plain, big, _, _ = sa.track_subframes(oracle, tr, k, first, m)
        want = shutter_adaptive_resolve(plain, big, k, m, T)
        for what, alt in ashut.wrong_scene_alternatives(oracle, tr, m, k, first).items():
            if what == "first_frame ignored" and first == 0:
                continue
            assert (alt != want).any(), f"{name}: a kernel tracing in {what} at full supersampling would pass"
