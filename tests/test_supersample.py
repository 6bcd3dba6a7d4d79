"""Supersampling (rt_set_supersampling), the parts that need no GPU: the numpy definition
(raytracer_hip.supersample.box_resolve), the public surface (header, bindings, exports, shim), and the
precondition of tests/test_gpu_supersample.py -- the expected frames there differ from the plain frames and
exercise the rounding rule, so no GPU test can pass by ignoring the factor."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from raytracer_hip import abi, scenes
from raytracer_hip.supersample import box_resolve

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _frame(rows):
    return np.array(rows, dtype=np.int32)


def test_box_resolve_known_answers():
    assert box_resolve(_frame([[0, 0], [0, 1]]), 2).tolist() == [[0]]          # 1/4 rounds down
    assert box_resolve(_frame([[0, 0], [1, 1]]), 2).tolist() == [[1]]          # a tie rounds up
    assert box_resolve(_frame([[255, 255], [255, 254]]), 2).tolist() == [[255]]
    # no carry crosses channels: 2 x 0x00FF00 + 2 x 0xFF00FF -> 0x808080 (510 / 4 = 127.5 -> 128 in each)
    assert box_resolve(_frame([[0x00FF00, 0xFF00FF], [0xFF00FF, 0x00FF00]]), 2).tolist() == [[0x808080]]
    # 3 x 0x00FF00 + 0xFF00FF: G (765 + 2) >> 2 = 191, R and B (255 + 2) >> 2 = 64
    assert box_resolve(_frame([[0x00FF00, 0x00FF00], [0xFF00FF, 0x00FF00]]), 2).tolist() == [[0x40BF40]]
    assert box_resolve(np.full((8, 8), 0xFFFFFF, dtype=np.int32), 8).tolist() == [[0xFFFFFF]]
    assert box_resolve(np.full((8, 16), 0xFFFFFF, dtype=np.int32), 4).tolist() == [[0xFFFFFF] * 4] * 2
    f = _frame([[1, 2, 3], [4, 5, 6]])
    assert np.array_equal(box_resolve(f, 1), f)


def test_box_resolve_is_the_per_channel_definition():
    rng = np.random.default_rng(7)
    for k in (2, 4, 8):
        f = rng.integers(0, 1 << 24, size=(3 * k, 5 * k), dtype=np.int64).astype(np.int32)
        got = box_resolve(f, k)
        assert got.dtype == np.int32 and got.shape == (3, 5)
        for y in range(3):
            for x in range(5):
                blk = f[y * k:(y + 1) * k, x * k:(x + 1) * k].astype(np.int64)
                want = 0
                for sh in (16, 8, 0):
                    want |= ((int(((blk >> sh) & 255).sum()) + k * k // 2) >> (2 * k.bit_length() - 2)) << sh
                assert int(got[y, x]) == want


@pytest.mark.parametrize("bad", [0, 3, 16, -2])
def test_box_resolve_rejects_other_factors(bad):
    with pytest.raises(ValueError):
        box_resolve(np.zeros((48, 48), dtype=np.int32), bad)


def test_box_resolve_rejects_ragged_frames():
    with pytest.raises(ValueError):
        box_resolve(np.zeros((6, 7), dtype=np.int32), 2)


def test_header_bindings_and_library_agree(rtlib):
    hdr = open(os.path.join(ROOT, "include", "raytracer_hip.h")).read()
    assert re.search(r"int rt_set_supersampling\(rt_ctx\* ctx, int k\);", hdr)
    assert re.search(r"int rt_get_supersampling\(const rt_ctx\* ctx, int\* out_k\);", hdr)
    assert "ABI 10 addition" in hdr
    assert re.search(r"#define RT_ABI_VERSION (\d+)", hdr).group(1) == "10"
    names = [e[0] for e in abi.EXPORTS]
    assert "rt_set_supersampling" in names and "rt_get_supersampling" in names
    assert rtlib.rt_set_supersampling.argtypes == [C.c_void_p, C.c_int]
    assert rtlib.rt_get_supersampling.argtypes == [C.c_void_p, C.POINTER(C.c_int)]
    assert rtlib.rt_abi_version() == 10


def test_null_context_is_an_invalid_argument(rtlib):
    assert rtlib.rt_set_supersampling(None, 2) == abi.RT_ERR_INVALID_ARG
    assert b"rt_set_supersampling" in rtlib.rt_last_error(None)
    k = C.c_int(7)
    assert rtlib.rt_get_supersampling(None, C.byref(k)) == abi.RT_ERR_INVALID_ARG
    assert k.value == 7


def test_shim_binds_the_call_and_reads_rt_samples():
    cs = open(os.path.join(ROOT, "shim", "csharp", "RayTracer.cs")).read()
    assert re.search(r"\[DllImport\(Lib\)\] internal static extern int rt_set_supersampling\(IntPtr ctx, int k\);", cs)
    assert 'GetEnvironmentVariable("RT_SAMPLES")' in cs and "Native.rt_set_supersampling(_ctx," in cs
    assert re.search(r"AbiVersion = (\d+);", cs).group(1) == "10"


PRECONDITION = {"REF": (13, 7), "C3": (50, 30), "C4": (50, 30)}


@pytest.mark.parametrize("k", [2, 4, 8])
@pytest.mark.parametrize("cid", list(PRECONDITION))
def test_resolved_oracle_frames_differ_from_the_plain_ones_and_hold_ties(oracle, cid, k):
    W, H = PRECONDITION[cid]
    sc = scenes.config(cid)
    plain, _ = oracle.render(sc.resized(W, H), oracle.MODE_NEAREST, 8)
    big, st = oracle.render(sc.resized(k * W, k * H), oracle.MODE_NEAREST, 8)
    assert st["primary_rays"] == k * k * W * H
    res = box_resolve(big, k)
    assert res.shape == plain.shape
    assert (res != plain).mean() > 0.25, "the supersampled frame is not the plain one"
    ties = rem = 0
    for sh in (16, 8, 0):
        s = ((big.astype(np.int64) >> sh) & 255).reshape(H, k, W, k).sum(axis=(1, 3))
        ties += int((s % (k * k) == k * k // 2).sum())
        rem += int((s % (k * k) != 0).sum())
    assert ties >= 1, "no exact half-way tie: the rounding rule would go unexercised"
    assert rem > ties, "channel sums that are no multiples of k*k"
