"""Host sanitizer builds ("host ASan/UBSan build of the oracle and the C ABI"):
tests/native/Makefile builds the oracle under ASan+UBSan and under TSan (the row-parallel
loop of RayTracer.cs:898-901 writes disjoint pixels, :1038), and rt_api.cpp's host code under
host-side ASan+UBSan (scene packing, view set-up and screen boxes, camera input, PPM, wire
layout, argument checks).  CPU only: no device call is reached."""
import os

import pytest

import host_check


@pytest.fixture(scope="module")
def built():
    return host_check.BUILD


def _run(cmd, env_extra=None):
    return host_check.run(os.path.basename(cmd[0]), cmd[1:], env_extra)


def test_oracle_asan_ubsan(built):
    out = _run([os.path.join(built, "san_oracle_asan"), "60"], {"UBSAN_OPTIONS": "print_stacktrace=1"})
    assert "0 failures" in out


def test_oracle_tsan_disjoint_rows(built):
    out = _run([os.path.join(built, "san_oracle_tsan"), "20"], {"TSAN_OPTIONS": "halt_on_error=1"})
    assert "0 failures" in out


def test_host_api_asan_ubsan(built):
    out = _run([os.path.join(built, "san_host_asan")], {"UBSAN_OPTIONS": "print_stacktrace=1"})
    assert "san_host: 0 failures" in out
    # the Tick hand-off's band plan: 7 sizes x 8 worker counts x 8 chunk counts x pinned / unpinned
    assert "band_plans: 896 plans" in out
