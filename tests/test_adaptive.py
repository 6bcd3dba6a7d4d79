"""Adaptive supersampling (rt_set_adaptive_sampling), the parts that need no GPU: the numpy definition
(supersample.refine_mask / adaptive_resolve) on hand-made frames, the identity it rests on -- sample (0, 0) of
every k x k block is the pixel of the plain frame, bit for bit -- against the oracle, the public surface, and the
preconditions of tests/test_gpu_adaptive.py: every case there has refined and flat tiles and an expectation that
is neither the plain nor the fully supersampled frame."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import adaptive_cases as ac
from raytracer_hip import abi
from raytracer_hip.supersample import adaptive_resolve, box_resolve, refine_mask

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _flat(h, w, v=0x101010):
    return np.full((h, w), v, dtype=np.int32)


def test_pair_across_a_tile_border_does_not_refine():
    f = _flat(16, 24)
    f[:, 8:] = 0xF0F0F0  # the edge lies between columns 7 and 8: between tiles
    f[8:, :] ^= 0x0F0F0F  # and another between rows 7 and 8
    assert not refine_mask(f, 1).any()
    f[3, 7] = 0xF0F0F0  # one pixel of the left tile takes its neighbour tile's colour: a pair inside tile (0, 0)
    assert refine_mask(f, 1).tolist() == [[True, False, False], [False, False, False]]


@pytest.mark.parametrize("shift", [16, 8, 0])
@pytest.mark.parametrize("T", [1, 2, 16, 255])
def test_threshold_is_inclusive_in_each_channel(shift, T):
    for horizontal in (True, False):
        f = _flat(8, 8, 0)
        g = _flat(8, 8, 0)
        a, b = ((2, 3), (2, 4)) if horizontal else ((3, 5), (4, 5))
        f[b] = (T - 1) << shift
        g[b] = T << shift
        assert not refine_mask(f, T).any()
        assert refine_mask(g, T).all()
        # the sign of the difference plays no part
        h = _flat(8, 8, 255 << shift)
        h[a] = (255 - T) << shift
        assert refine_mask(h, T).all()


def test_ragged_last_tiles():
    f = _flat(11, 19)
    assert refine_mask(f, 1).shape == (2, 3)
    f[10, 18] = 0  # the last tile is 3 wide and 3 high
    assert refine_mask(f, 1).tolist() == [[False, False, False], [False, False, True]]
    f = _flat(9, 9)
    f[8, 8] = 0  # a 1 x 1 tile has no pair
    assert not refine_mask(f, 1).any()
    f[8, 3] = 0  # an 8 x 1 tile has horizontal pairs only
    assert refine_mask(f, 1).tolist() == [[False, False], [True, False]]
    assert refine_mask(_flat(1, 1), 1).shape == (1, 1)


def test_256_never_refines_and_1_refines_on_any_difference():
    rng = np.random.default_rng(3)
    f = rng.integers(0, 1 << 24, size=(21, 37), dtype=np.int64).astype(np.int32)
    assert not refine_mask(f, 256).any()
    assert refine_mask(f, 1).all()
    g = _flat(8, 16)
    g[0, 9] += 1  # one step of blue
    assert refine_mask(g, 1).tolist() == [[False, True]] and not refine_mask(g, 2).any()
    for bad in (0, 257, -1):
        with pytest.raises(ValueError):
            refine_mask(g, bad)


def test_adaptive_resolve_takes_refined_tiles_from_the_samples():
    rng = np.random.default_rng(5)
    k = 2
    samples = rng.integers(0, 1 << 24, size=(2 * 11, 2 * 19), dtype=np.int64).astype(np.int32)
    plain = _flat(11, 19)
    plain[2, 9:12] = 0  # tile (1, 0) only
    out = adaptive_resolve(plain, samples, k, 8)
    full = box_resolve(samples, k)
    assert np.array_equal(out[:8, 8:16], full[:8, 8:16])
    rest = np.ones_like(plain, dtype=bool)
    rest[:8, 8:16] = False
    assert np.array_equal(out[rest], plain[rest])
    assert np.array_equal(adaptive_resolve(plain, samples, k, 256), plain)
    assert np.array_equal(adaptive_resolve(plain, samples, k, 0), full)
    with pytest.raises(ValueError):
        adaptive_resolve(plain[:-1], samples, k, 8)


IDENTITY = [("REF", 13, 7), ("C1", 24, 16), ("C3", 50, 30), ("C4", 50, 30), ("dense", 37, 21), ("bundle_L5", 32, 24),
            ("gpow_direct", 32, 24), ("gpow_bundle", 32, 24)]


@pytest.mark.parametrize("k", [2, 4])
@pytest.mark.parametrize("cid,W,H", IDENTITY)
def test_sample_00_is_the_plain_pixel(oracle, cid, W, H, k):
    plain = ac.frames(oracle, cid, W, H, 1)[0]
    big = ac.frames(oracle, cid, W, H, k)[0]
    assert np.array_equal(big[::k, ::k], plain)


def test_header_bindings_and_library_agree(rtlib):
    hdr = open(os.path.join(ROOT, "include", "raytracer_hip.h")).read()
    assert re.search(r"int rt_set_adaptive_sampling\(rt_ctx\* ctx, int threshold\);", hdr)
    assert re.search(r"int rt_get_adaptive_sampling\(const rt_ctx\* ctx, int\* out_threshold\);", hdr)
    assert re.search(r"\(ABI 10 addition\) Adaptive supersampling", hdr)
    assert re.search(r"#define RT_ABI_VERSION (\d+)", hdr).group(1) == "10"
    names = [e[0] for e in abi.EXPORTS]
    assert "rt_set_adaptive_sampling" in names and "rt_get_adaptive_sampling" in names
    assert rtlib.rt_set_adaptive_sampling.argtypes == [C.c_void_p, C.c_int]
    assert rtlib.rt_get_adaptive_sampling.argtypes == [C.c_void_p, C.POINTER(C.c_int)]
    assert rtlib.rt_abi_version() == 10 and abi.RT_ABI_VERSION == 10


def test_null_arguments_are_invalid(rtlib):
    assert rtlib.rt_set_adaptive_sampling(None, 16) == abi.RT_ERR_INVALID_ARG
    assert b"rt_set_adaptive_sampling" in rtlib.rt_last_error(None)
    t = C.c_int(7)
    assert rtlib.rt_get_adaptive_sampling(None, C.byref(t)) == abi.RT_ERR_INVALID_ARG
    assert b"rt_get_adaptive_sampling" in rtlib.rt_last_error(None)
    assert t.value == 7


def test_python_surface():
    import inspect

    import raytracer_hip
    assert callable(raytracer_hip.Context.set_adaptive_sampling)
    assert isinstance(raytracer_hip.Context.adaptive_sampling, property)
    sig = inspect.signature(raytracer_hip.RayTracer.__init__)
    assert sig.parameters["adaptive"].default == 0 and sig.parameters["samples"].default == 1


def test_shim_binds_the_call_and_reads_rt_adaptive():
    cs = open(os.path.join(ROOT, "shim", "csharp", "RayTracer.cs")).read()
    assert re.search(r"\[DllImport\(Lib\)\] internal static extern int rt_set_adaptive_sampling\(IntPtr ctx, int threshold\);", cs)
    assert re.search(r"\[DllImport\(Lib\)\] internal static extern int rt_get_adaptive_sampling\(IntPtr ctx, out int threshold\);", cs)
    assert 'GetEnvironmentVariable("RT_ADAPTIVE")' in cs and "Native.rt_set_adaptive_sampling(_ctx," in cs
    assert re.search(r"AbiVersion = (\d+);", cs).group(1) == "10"
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "rt_set_adaptive_sampling" in doc and "RT_ADAPTIVE" in doc


@pytest.mark.parametrize("case", ac.CASES, ids=ac.case_id)
def test_gpu_cases_can_not_pass_by_ignoring_the_setting(oracle, case):
    cid, W, H, k, T = case
    refined, tiles, ne_plain, ne_full = ac.facts(oracle, cid, W, H, k, T)
    print(f"{ac.case_id(case)}: {refined} / {tiles} tiles refined, {ne_plain} pixels != plain, {ne_full} != full")
    assert refined >= 2 and tiles - refined >= 2
    assert ne_plain >= 16 and ne_full >= 16
