"""Host check of the dark-tile skip's guard (csrc/rt_dark.h): CPU only.  tests/native/dark_host.cpp,
built by tests/native/dark.mk under host-side ASan + UBSan without FMA contraction and run as a plain executable,
restates the reference's per-light term of a plane hit in binary32 and sweeps a product of edge inputs (normals
around the 2^-10 band, lights above, on and beside the plane and at the hit point, intensities and material terms
up to inf and NaN, exponents, distances, ray directions, hit points up to 1e9).  Wherever both parts of the guard
pass the term on a dark square is +0 bit for bit, with the light's intensity and with 0; and the guard does pass on
the REF / C3 and C4 planes with their lights, on a 64 x 64 grid of each plane."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NATIVE = os.path.join(ROOT, "tests", "native")
EXE = os.path.join(NATIVE, "build", "dark_host")


@pytest.fixture(scope="module")
def output():
    subprocess.run(["make", "-s", "-f", "dark.mk", "-C", NATIVE], check=True, timeout=600)
    env = dict(os.environ)
    # a preloaded library (if any) stays: ASan is told not to insist on coming first
    env["ASAN_OPTIONS"] = ":".join(x for x in (env.get("ASAN_OPTIONS", ""), "verify_asan_link_order=0") if x)
    env["UBSAN_OPTIONS"] = "print_stacktrace=1"
    r = subprocess.run([EXE], capture_output=True, text=True, timeout=300, env=env)
    out = r.stdout + r.stderr
    for marker in ("ERROR: AddressSanitizer", "runtime error:", "ERROR: LeakSanitizer"):
        assert marker not in out, out[-4000:]
    assert r.returncode == 0, out[-4000:]
    return out


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
