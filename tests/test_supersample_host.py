"""Host sanitizer run of the supersampling additions: tests/native/ss_host.cpp compiles rt_api.cpp's host code
into a stand-alone program under host-side ASan + UBSan (the gfx950 device code is not instrumented) and checks
the factor's setter / getter, the sample-count rejection, the render entry points' argument checks at k > 1, the
two unsupported paths, the view of a supersampled render and the resolve arithmetic the kernels share
(csrc/rt_resolve.h).  CPU only: no device call is reached, and nothing is loaded into python."""
import pytest

import host_check


@pytest.fixture(scope="module")
def ss_host():
    return host_check.run("ss_host_asan")


def test_supersampling_host_code_asan_ubsan(ss_host):
    out = ss_host
    assert "ss_host: 0 failures" in out
    assert "resolve: " in out
