"""Progressive accumulation (rt_set_progressive), the parts that need no GPU: the numpy definition
(raytracer_hip.supersample.progressive_order / progressive_resolve) against the oracle, the public surface (header,
bindings, exports, shim), and the precondition of tests/test_gpu_progressive.py -- consecutive frames P_c of a run
differ, so no GPU test can pass with a wrong order or divisor."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from raytracer_hip import abi, scenes
from raytracer_hip.supersample import box_resolve, progressive_order, progressive_resolve

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [(40, 24), (37, 19)]
_FRAMES = {}


def _frame(oracle, cid, W, H, k):
    """The oracle's frame of config `cid` at k W x k H, rendered once per process and shared read-only."""
    key = (cid, W, H, k)
    if key not in _FRAMES:
        px, _ = oracle.render(scenes.config(cid).resized(k * W, k * H), oracle.MODE_NEAREST, 8)
        px.setflags(write=False)
        _FRAMES[key] = px
    return _FRAMES[key]


@pytest.mark.parametrize("k", [2, 4, 8])
def test_order_is_a_permutation_of_the_block(k):
    order = progressive_order(k)
    assert len(order) == k * k and sorted(order) == sorted((i, j) for i in range(k) for j in range(k))
    assert order[0] == (0, 0)
    # the coarse sub-grids come first: the first 4^t samples are the 2^t x 2^t grid of stride k / 2^t
    for t in range(k.bit_length()):
        step = k >> t
        assert sorted(order[:4 ** t]) == sorted((i, j) for i in range(0, k, step) for j in range(0, k, step))


def test_order_known_answers():
    assert progressive_order(1) == [(0, 0)]
    assert progressive_order(2) == [(0, 0), (1, 0), (0, 1), (1, 1)]
    assert progressive_order(4) == [(0, 0), (2, 0), (0, 2), (2, 2), (1, 0), (3, 0), (1, 2), (3, 2),
                                    (0, 1), (2, 1), (0, 3), (2, 3), (1, 1), (3, 1), (1, 3), (3, 3)]
    assert progressive_order(8)[:6] == [(0, 0), (4, 0), (0, 4), (4, 4), (2, 0), (6, 0)]
    for bad in (0, 3, 16, -2):
        with pytest.raises(ValueError):
            progressive_order(bad)


def test_resolve_known_answers():
    f = np.array([[0x000000, 0xFF00FF], [0x00FF00, 0x030201]], dtype=np.int32)  # samples (0,0) (1,0) / (0,1) (1,1)
    assert progressive_resolve(f, 2, 1).tolist() == [[0x000000]]
    assert progressive_resolve(f, 2, 2).tolist() == [[0x800080]]                 # (255 + 1) // 2 = 128 in R and B
    assert progressive_resolve(f, 2, 3).tolist() == [[0x555555]]                 # (255 + 1) // 3 = 85 in each
    assert progressive_resolve(f, 2, 4).tolist() == [[0x414040]]                 # (258 + 2) // 4 = 65, (257 + 2) // 4, (256 + 2) // 4 = 64
    assert np.array_equal(progressive_resolve(f, 2, 4), box_resolve(f, 2))
    for bad_c in (0, 5, -1):
        with pytest.raises(ValueError):
            progressive_resolve(f, 2, bad_c)
    with pytest.raises(ValueError):
        progressive_resolve(np.zeros((6, 7), dtype=np.int32), 2, 1)
    with pytest.raises(ValueError):
        progressive_resolve(f, 3, 1)


@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("cid", ["C3", "C4"])
@pytest.mark.parametrize("k", [2, 4, 8])
def test_definition_against_the_oracle(oracle, cid, size, k):
    W, H = size
    big = _frame(oracle, cid, W, H, k)
    # P_1 is the plain frame, P_{k^2} the supersampled one, P_{4^t} the frame supersampled at 2^t
    assert np.array_equal(progressive_resolve(big, k, 1), _frame(oracle, cid, W, H, 1))
    assert np.array_equal(progressive_resolve(big, k, k * k), box_resolve(big, k))
    for t in range(1, k.bit_length() - 1):
        assert np.array_equal(progressive_resolve(big, k, 4 ** t), box_resolve(_frame(oracle, cid, W, H, 2 ** t), 2 ** t)), \
            f"P_{4 ** t} at k = {k} is not the frame of factor {2 ** t}"
    # consecutive counts give different frames: a wrong order or divisor cannot pass
    prev = progressive_resolve(big, k, 1)
    changed = []
    for c in range(2, k * k + 1):
        cur = progressive_resolve(big, k, c)
        assert cur.dtype == np.int32 and cur.shape == (H, W)
        changed.append(int((cur != prev).sum()))
        prev = cur
    assert min(changed) > 0, f"P_c == P_(c-1) at c = {2 + changed.index(0)}"


def test_header_bindings_and_library_agree(rtlib):
    hdr = open(os.path.join(ROOT, "include", "raytracer_hip.h")).read()
    assert re.search(r"int rt_set_progressive\(rt_ctx\* ctx, int k\);", hdr)
    assert re.search(r"int rt_get_progressive\(const rt_ctx\* ctx, int\* out_k, int\* out_samples\);", hdr)
    assert re.search(r"int rt_reset_progressive\(rt_ctx\* ctx\);", hdr)
    assert re.search(r"#define RT_ABI_VERSION (\d+)", hdr).group(1) == "10"
    names = [e[0] for e in abi.EXPORTS]
    assert {"rt_set_progressive", "rt_get_progressive", "rt_reset_progressive"} <= set(names)
    assert rtlib.rt_set_progressive.argtypes == [C.c_void_p, C.c_int]
    assert rtlib.rt_get_progressive.argtypes == [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    assert rtlib.rt_reset_progressive.argtypes == [C.c_void_p]
    assert rtlib.rt_abi_version() == 10


def test_null_arguments_are_invalid(rtlib):
    assert rtlib.rt_set_progressive(None, 2) == abi.RT_ERR_INVALID_ARG
    assert b"rt_set_progressive" in rtlib.rt_last_error(None)
    k, c = C.c_int(7), C.c_int(9)
    assert rtlib.rt_get_progressive(None, C.byref(k), C.byref(c)) == abi.RT_ERR_INVALID_ARG
    assert (k.value, c.value) == (7, 9)
    assert rtlib.rt_reset_progressive(None) == abi.RT_ERR_INVALID_ARG
    assert b"rt_reset_progressive" in rtlib.rt_last_error(None)


def test_shim_binds_the_calls_and_reads_rt_progressive():
    cs = open(os.path.join(ROOT, "shim", "csharp", "RayTracer.cs")).read()
    assert re.search(r"\[DllImport\(Lib\)\] internal static extern int rt_set_progressive\(IntPtr ctx, int k\);", cs)
    assert re.search(r"\[DllImport\(Lib\)\] internal static extern int rt_get_progressive\(IntPtr ctx, out int k, out int samples\);", cs)
    assert re.search(r"\[DllImport\(Lib\)\] internal static extern int rt_reset_progressive\(IntPtr ctx\);", cs)
    assert 'GetEnvironmentVariable("RT_PROGRESSIVE")' in cs and "Native.rt_set_progressive(_ctx," in cs
