"""Host check of the dark-tile skip's guard (csrc/rt_dark.h): CPU only.  tests/native/dark_host.cpp,
built by tests/native/Makefile under host-side ASan + UBSan without FMA contraction and run as a plain executable,
restates the reference's per-light term of a plane hit in binary32 and sweeps a product of edge inputs (normals
around the 2^-10 band, lights above, on and beside the plane and at the hit point, intensities and material terms
up to inf and NaN, exponents, distances, ray directions, hit points up to 1e9).  Wherever both parts of the guard
pass the term on a dark square is +0 bit for bit, with the light's intensity and with 0; and the guard does pass on
the REF / C3 and C4 planes with their lights, on a 64 x 64 grid of each plane."""
import re

import pytest

import host_check


@pytest.fixture(scope="module")
def output():
    return host_check.run("dark_host")


def test_term_is_plus_zero_wherever_the_guard_passes(output):
    assert "dark_host: 0 failures" in output, output[-4000:]
    m = re.search(r"dark_host: (\d+) host inputs, (\d+) accepted, (\d+) terms checked, (\d+) refused terms not \+0",
                  output)
    assert m, output[-2000:]
    hosts, accepted, checked, refused_nonzero = map(int, m.groups())
    assert hosts == 16 * 10 * 7 * 7 * 7 * 9  # normals, lights, I, kd, ks, exponents
    # the guard accepts a real share of the sweep, and the sweep holds inputs the skip would get wrong
    assert accepted >= 1000 and checked >= 100000
    assert refused_nonzero >= 1000


def test_guard_passes_on_the_reference_and_benchmark_planes(output):
    assert f"dark_host: grid {3 * 64 * 64} of {3 * 64 * 64} passed" in output, output[-2000:]
