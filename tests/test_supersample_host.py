"""Host sanitizer run of the supersampling additions: tests/native/ss_host.cpp compiles rt_api.cpp's host code
into a stand-alone program under host-side ASan + UBSan (the gfx950 device code is not instrumented) and checks
the factor's setter / getter, the sample-count rejection, the render entry points' argument checks at k > 1, the
two unsupported paths, the view of a supersampled render and the resolve arithmetic the kernels share
(csrc/rt_resolve.h).  CPU only: no device call is reached, and nothing is loaded into python."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NATIVE = os.path.join(ROOT, "tests", "native")
CSRC = os.path.join(ROOT, "uu-infogr-raytracer_amd", "csrc")
BUILD = os.path.join(NATIVE, "build")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
FP = ["-ffp-contract=off", "-fno-fast-math"]
HSAN = ["-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all"]


@pytest.fixture(scope="module")
def ss_host():
    # the product's kernel objects (uninstrumented device code + launch stubs): built already after build()
    subprocess.run(["make", "-s", "-C", CSRC], check=True, timeout=1800)
    os.makedirs(BUILD, exist_ok=True)
    obj, exe = os.path.join(BUILD, "ss_host.o"), os.path.join(BUILD, "ss_host_asan")
    subprocess.run([HIPCC, "-O1", "-g", "-std=c++17", "-fPIC", "--offload-arch=gfx950", *FP,
                    "-fhip-fp32-correctly-rounded-divide-sqrt", "-fno-gpu-flush-denormals-to-zero",
                    "-fno-omit-frame-pointer", "-Wall", *HSAN, "-x", "hip", "-c", "-o", obj,
                    os.path.join(NATIVE, "ss_host.cpp")], check=True, timeout=600)
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-fsanitize=address,undefined", "-fno-gpu-sanitize", "-o", exe, obj,
                    os.path.join(CSRC, "obj", "rt_kernel.o"), os.path.join(CSRC, "obj", "rt_codec.o"),
                    "-ldl", "-lm", "-pthread"], check=True, timeout=600)
    return exe


def test_supersampling_host_code_asan_ubsan(ss_host):
    env = dict(os.environ, UBSAN_OPTIONS="print_stacktrace=1")
    # a preloaded library (if any) stays: ASan is told not to insist on coming first
    env["ASAN_OPTIONS"] = ":".join(x for x in (env.get("ASAN_OPTIONS", ""), "verify_asan_link_order=0") if x)
    r = subprocess.run([ss_host], capture_output=True, text=True, timeout=300, env=env)
    out = r.stdout + r.stderr
    assert r.returncode == 0, out[-4000:]
    for marker in ("ERROR: AddressSanitizer", "runtime error:", "ERROR: LeakSanitizer"):
        assert marker not in out, out[-4000:]
    assert "ss_host: 0 failures" in out
    assert "resolve: " in out
