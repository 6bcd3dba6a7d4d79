"""Host check of the shadow pre-test's group and union records (csrc/rt_scene.h build_shadow_groups; DESIGN.md 3 and
4): CPU only.  tests/native/shadow_group_host.cpp, built by tests/native/shadow_group.mk under host-side ASan + UBSan and
run as a plain executable (nothing is loaded into python, nothing is preloaded), builds the records of the configs, of
degenerate scenes and of 3000 seeded random scenes with the library's own builder and checks, with the kernels' own
pre-test functions in binary32, that a member some lane keeps keeps its group and the union -- on hit points of every
scale, on both sides of every record's line-rule and behind-rule boundary, and on NaN, infinities and zeros."""
import os
import re
import subprocess

import pytest

import host_check


@pytest.fixture(scope="module")
def output():
    subprocess.run(["make", "-s", "-f", "shadow_group.mk", "-C", host_check.NATIVE], check=True, timeout=600)
    env = dict(os.environ, UBSAN_OPTIONS="print_stacktrace=1")
    # a preloaded library (if any) stays: ASan is told not to insist on coming first
    env["ASAN_OPTIONS"] = ":".join(x for x in (env.get("ASAN_OPTIONS", ""), "verify_asan_link_order=0") if x)
    r = subprocess.run([os.path.join(host_check.BUILD, "shadow_group_host")], capture_output=True, text=True, timeout=600, env=env)
    out = r.stdout + r.stderr
    assert r.returncode == 0, out[-4000:]
    for marker in host_check.MARKERS:
        assert marker not in out, out[-4000:]
    return out


def test_no_kept_member_loses_its_group_or_the_union(output):
    m = re.search(r"shadow_group_host: (\d+) scenes, (\d+) lights, (\d+) samples, (\d+) member checks, (\d+) failures", output)
    assert m, output[-2000:]
    scenes, lights, samples, checks, failures = map(int, m.groups())
    assert failures == 0, output[-4000:]
    assert scenes == 5 + 15 + 3000 and lights > 2 * 3000 and samples > 1000 * lights and checks > samples


def test_the_samples_find_records_that_are_too_small(output):
    m = re.search(r"shadow_group_host_shrunk: (\d+) failures", output)
    assert m and int(m.group(1)) > 0, output[-2000:]
