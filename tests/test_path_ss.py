"""supersample.path_resolve, the numpy definition of rt_set_path_supersampling (CPU only): per 8-bit channel the output
is (sum over the m sub-frames and the k x k samples + m k k / 2) >> (log2 m + 2 log2 k), one rounding of the whole mean.
It is box_resolve per frame at m = 1 and path.shutter_mean at k = 1, and it is not the shutter's mean of box-resolved
frames: an input on which the two differ is constructed here, so a kernel that rounds twice cannot pass
tests/test_gpu_path_ss.py, whose expectation is this function."""
import numpy as np
import pytest

from raytracer_hip import path
from raytracer_hip.supersample import box_resolve, path_resolve


def _frames(n, h, w, seed):
    rng = np.random.default_rng(seed)
    return rng.integers(0, 1 << 24, (n, h, w), dtype=np.int64).astype(np.int32)


@pytest.mark.parametrize("k", [1, 2, 4, 8])
def test_m_1_is_box_resolve_per_frame(k):
    f = _frames(3, 2 * k, 3 * k, 10 + k)
    got = path_resolve(f, k)
    assert got.shape == (3, 2, 3) and got.dtype == np.int32
    for i in range(3):
        assert np.array_equal(got[i], box_resolve(f[i], k))


@pytest.mark.parametrize("m", [1, 2, 16, 256])
def test_k_1_is_the_shutter_mean(m):
    f = _frames(2 * m, 3, 5, 20 + m)
    assert np.array_equal(path_resolve(f, 1, m), path.shutter_mean(f, m))


@pytest.mark.parametrize("k,m", [(2, 2), (2, 64), (4, 16), (8, 4), (4, 2)])
def test_the_formula_per_channel(k, m):
    f = _frames(2 * m, 2 * k, 2 * k, 30 + k + m)
    got = path_resolve(f, k, m).astype(np.int64)
    n = m * k * k
    for shift in (16, 8, 0):
        ch = (f.astype(np.int64) >> shift) & 0xFF
        for fr in range(2):
            for y in range(2):
                for x in range(2):
                    total = int(ch[fr * m:(fr + 1) * m, y * k:(y + 1) * k, x * k:(x + 1) * k].sum())
                    assert (got[fr, y, x] >> shift) & 0xFF == (total + n // 2) // n
    assert (got >> 24 == 0).all()


def test_extremes_fill_and_empty_the_sum():
    for k, m in [(2, 64), (8, 4), (4, 16), (1, 256)]:
        assert (path_resolve(np.full((m, k, k), 0xFFFFFF, dtype=np.int32), k, m) == 0xFFFFFF).all()
        assert (path_resolve(np.zeros((m, k, k), dtype=np.int32), k, m) == 0).all()
        one = np.full((m, k, k), 0x00FF00, dtype=np.int32)  # a full channel between two empty ones, and the reverse
        assert (path_resolve(one, k, m) == 0x00FF00).all() and (path_resolve(one ^ 0xFFFFFF, k, m) == 0xFF00FF).all()


def test_one_rounding_is_not_a_mean_of_means():
    """k = 2, m = 2, one output pixel, one channel: sub-frame 0's block sums to 2, sub-frame 1's to 0.  Rounding each
    block first gives (2 + 2) >> 2 = 1 and 0, and their shutter mean (1 + 0 + 1) >> 1 = 1; the single rounding gives
    (2 + 4) >> 3 = 0."""
    f = np.zeros((2, 2, 2), dtype=np.int32)
    f[0, 0, 0] = f[0, 1, 1] = 0x010101
    twice = path.shutter_mean(np.stack([box_resolve(f[0], 2), box_resolve(f[1], 2)]), 2)
    once = path_resolve(f, 2, 2)
    assert twice.tolist() == [[[0x010101]]] and once.tolist() == [[[0]]]
    # in general the two never differ by more than one step of a channel
    rng = np.random.default_rng(5)
    g = rng.integers(0, 1 << 24, (8, 8, 12), dtype=np.int64).astype(np.int32)
    a = path_resolve(g, 4, 2)
    b = path.shutter_mean(np.stack([box_resolve(x, 4) for x in g]), 2)
    assert a.shape == b.shape == (4, 2, 3)
    assert np.abs(((a >> 8) & 0xFF) - ((b >> 8) & 0xFF)).max() <= 1, "the two roundings differ by one step at most"


def test_bad_shapes_and_counts_are_rejected():
    ok = np.zeros((4, 4, 6), dtype=np.int32)
    assert path_resolve(ok, 2, 2).shape == (2, 2, 3)
    for bad, k, m in [(np.zeros((4, 5, 6), dtype=np.int32), 2, 2),   # rows no multiple of k
                      (np.zeros((4, 4, 7), dtype=np.int32), 2, 2),   # columns no multiple of k
                      (np.zeros((3, 4, 6), dtype=np.int32), 2, 2),   # frames no multiple of m
                      (np.zeros((4, 6), dtype=np.int32), 2, 1),      # no frame axis
                      (ok, 3, 1), (ok, 2, 3), (ok, 2, 0),            # factors that do not exist
                      (np.zeros((128, 2, 2), dtype=np.int32), 2, 128)]:  # m k k = 512: past the 16-bit sums
        with pytest.raises(ValueError):
            path_resolve(bad, k, m)
