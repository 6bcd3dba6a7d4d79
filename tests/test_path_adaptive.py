"""Adaptive supersampling in the camera-path and scene-track renders (rt_set_path_adaptive_sampling), the parts that need
no GPU: the numpy definition (supersample.path_adaptive_resolve: adaptive_resolve per frame), the public surface, and the
preconditions of tests/test_gpu_path_adaptive.py computed from the unchanged oracle -- at every scene, size and threshold
used there each camera (each track frame) has refined and flat tiles, the refine masks differ between cameras (between
track frames under one camera, too), and every expected frame differs from both its plain and its fully supersampled
frame, so that a GPU test cannot pass by refining everything or nothing, or by deciding once for every frame."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import path_adaptive_cases as pc
import path_cases
from raytracer_hip import abi
from raytracer_hip.supersample import adaptive_resolve, box_resolve, path_adaptive_resolve, path_resolve

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _frames(f, h, w, k, seed):
    rng = np.random.default_rng(seed)
    plain = np.full((f, h, w), 0x202020, dtype=np.int32)
    for i in range(f):  # frame i: an edge inside tile (i % 3, 0) only
        plain[i, 2, 8 * (i % 3) + 1:8 * (i % 3) + 4] = 0xE0E0E0
    samples = rng.integers(0, 1 << 24, size=(f, k * h, k * w), dtype=np.int64).astype(np.int32)
    return plain, samples


@pytest.mark.parametrize("k", [2, 4, 8])
def test_definition_is_adaptive_resolve_per_frame(k):
    plain, samples = _frames(4, 11, 19, k, 7 + k)
    out = path_adaptive_resolve(plain, samples, k, 64)
    assert out.shape == plain.shape and out.dtype == np.int32
    for f in range(4):
        assert np.array_equal(out[f], adaptive_resolve(plain[f], samples[f], k, 64))
        tx = f % 3
        full = box_resolve(samples[f], k)
        assert np.array_equal(out[f, :8, 8 * tx:8 * tx + 8], full[:8, 8 * tx:8 * tx + 8]), "the frame's own tile is refined"
        rest = np.ones(plain.shape[1:], dtype=bool)
        rest[:8, 8 * tx:8 * tx + 8] = False
        assert np.array_equal(out[f][rest], plain[f][rest]), "and no other: every frame decides for itself"
    assert (out[0] != out[1]).any()


@pytest.mark.parametrize("k", [2, 4])
def test_threshold_0_and_256_and_factor_1(k):
    plain, samples = _frames(3, 9, 17, k, 11)
    assert np.array_equal(path_adaptive_resolve(plain, samples, k, 0), path_resolve(samples, k, 1))
    assert np.array_equal(path_adaptive_resolve(plain, samples, k, 256), plain)
    assert np.array_equal(path_adaptive_resolve(plain, plain, 1, 1), plain), "k = 1: the samples are the plain frames"


def test_shape_and_argument_errors():
    plain, samples = _frames(2, 8, 16, 2, 3)
    for bad in (lambda: path_adaptive_resolve(plain[0], samples[0], 2, 16),        # no frame axis
                lambda: path_adaptive_resolve(plain, samples[:1], 2, 16),          # frame counts differ
                lambda: path_adaptive_resolve(plain, samples, 4, 16),              # sizes do not match the factor
                lambda: path_adaptive_resolve(plain[:, :-1], samples, 2, 16),
                lambda: path_adaptive_resolve(plain, samples, 3, 16),              # no factor
                lambda: path_adaptive_resolve(plain, samples, 2, -1),
                lambda: path_adaptive_resolve(plain, samples, 2, 257)):
        with pytest.raises(ValueError):
            bad()


def test_header_bindings_and_library_agree(rtlib):
    hdr = open(os.path.join(ROOT, "include", "raytracer_hip.h")).read()
    assert re.search(r"int rt_set_path_adaptive_sampling\(rt_ctx\* ctx, int threshold\);", hdr)
    assert re.search(r"int rt_get_path_adaptive_sampling\(const rt_ctx\* ctx, int\* out_threshold\);", hdr)
    assert re.search(r"#define RT_ABI_VERSION (\d+)", hdr).group(1) == "10"
    names = [e[0] for e in abi.EXPORTS]
    assert "rt_set_path_adaptive_sampling" in names and "rt_get_path_adaptive_sampling" in names
    assert rtlib.rt_set_path_adaptive_sampling.argtypes == [C.c_void_p, C.c_int]
    assert rtlib.rt_get_path_adaptive_sampling.argtypes == [C.c_void_p, C.POINTER(C.c_int)]
    assert rtlib.rt_abi_version() == 10 and abi.RT_ABI_VERSION == 10


def test_null_arguments_are_invalid(rtlib):
    assert rtlib.rt_set_path_adaptive_sampling(None, 16) == abi.RT_ERR_INVALID_ARG
    assert b"rt_set_path_adaptive_sampling" in rtlib.rt_last_error(None)
    t = C.c_int(7)
    assert rtlib.rt_get_path_adaptive_sampling(None, C.byref(t)) == abi.RT_ERR_INVALID_ARG
    assert b"rt_get_path_adaptive_sampling" in rtlib.rt_last_error(None)
    assert t.value == 7


def test_python_surface_and_docs():
    import raytracer_hip
    assert callable(raytracer_hip.Context.set_path_adaptive_sampling) and callable(raytracer_hip.Context.get_path_adaptive_sampling)
    for doc in ("README.md", "DESIGN.md", "INTEGRATION.md"):
        assert "rt_set_path_adaptive_sampling" in open(os.path.join(ROOT, doc)).read(), doc


# ---- the preconditions of the GPU cases ----------------------------------------------------------------------------
def _hold(fs, distinct, what):
    masks = [fs[i][0] for i in distinct]
    print(f"{what}: {[int(m.sum()) for m in masks]} of {masks[0].size} tiles refined, "
          f"pixels != plain {[f[1] for f in fs]}, != full {[f[2] for f in fs]}")
    for i, m in zip(distinct, masks):
        assert m.any() and not m.all(), f"{what}: frame {i} has refined and flat tiles"
    assert any((a != b).any() for n, a in enumerate(masks) for b in masks[:n]), f"{what}: two frames have different masks"
    for i, (_, ne_plain, ne_full) in enumerate(fs):
        assert ne_plain >= 1 and ne_full >= 1, f"{what}: frame {i} is neither the plain nor the fully supersampled frame"


@pytest.mark.parametrize("case", pc.PATH_K2, ids=lambda c: f"{c[0]}-{c[1]}x{c[2]}-T{c[3]}")
def test_path_cases_at_k_2(oracle, case):
    cid, W, H, T = case
    plain, big, _ = pc.path_frames(oracle, pc.scene(cid, W, H), 2)
    _hold(pc.facts(plain, big, 2, T), path_cases.DISTINCT, f"{cid} {W}x{H} T={T}")
    assert np.array_equal(plain[0], plain[5]), "cameras 0 and 5 are equal"


@pytest.mark.parametrize("case", pc.PATH_K48, ids=lambda c: f"{c[0]}-k{c[4]}")
def test_path_cases_at_k_4_and_8(oracle, case):
    cid, W, H, T, k, n = case
    plain, big, _ = pc.path_frames(oracle, pc.scene(cid, W, H), k)
    _hold(pc.facts(plain[:n], big[:n], k, T), list(range(min(n, 5))), f"{cid} k={k} T={T}")


def test_view_height_case(oracle):
    plain, big, _ = pc.path_frames(oracle, pc.scene("C3", pc.W0, pc.H0), 2, pc.VIEW_ROWS, pc.H0)
    assert plain.shape[1] == pc.VIEW_ROWS and pc.VIEW_ROWS % 8 != 0
    fs = pc.facts(plain, big, 2, pc.T0)
    _hold(fs, path_cases.DISTINCT, f"{pc.VIEW_ROWS} rows of a {pc.H0}-row view")
    assert any(f[0][-1].any() for f in fs), "a tile of the cut last tile row is refined"


@pytest.mark.parametrize("name", list(pc.TRACKS))
def test_track_cases(oracle, name):
    tr, T = pc.track(name), pc.TRACKS[name][1]
    for k in (2, 4) if name == "direct" else (2,):
        plain, big, _ = pc.track_frames(oracle, tr, k)
        _hold(pc.facts(plain, big, k, T), list(range(len(tr))), f"track {name} k={k} T={T}")


def test_the_decision_follows_each_frame_s_scene(oracle):
    """Track frames under one camera: their masks can differ through the scenes alone, and do."""
    tr, T = pc.track("one_camera"), pc.TRACKS["one_camera"][1]
    assert all(sc.camera == tr[0].camera for sc in tr)
    plain, big, _ = pc.track_frames(oracle, tr, 2)
    fs = pc.facts(plain, big, 2, T)
    assert (fs[0][0] != fs[4][0]).any() and (fs[1][0] != fs[3][0]).any()


def test_mixed_tracks_mix_exponents():
    for name in ("mixed_s8", "mixed_s12"):
        tr = pc.track(name)
        gp = [any(s.material.n not in (0.0, 0.5, 1.0, 2.0) for s in sc.spheres) for sc in tr]
        assert gp == [False, False, True], name
