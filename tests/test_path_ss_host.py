"""Host checks of supersampled path, shutter and track launches (rt_set_path_supersampling): CPU only.
tests/native/path_ss_host.cpp, built by tests/native/path_ss.mk once plain and once under ASan + UBSan and run as a
stand-alone executable each time (nothing is loaded into python, nothing is preloaded), checks the variant selection with
LaunchParams::view_ss zero (today's rule, 624 descriptors) and set (the three new modes, 804 descriptors, every refusal),
the single rounding of rt_resolve.h over every (s, t) and the butterfly's lane pattern."""
import os
import re
import subprocess

import pytest

import host_check


@pytest.fixture(scope="module", params=["path_ss_host", "path_ss_host_asan"])
def output(request):
    subprocess.run(["make", "-s", "-f", "path_ss.mk", "-C", host_check.NATIVE], check=True, timeout=1800)
    env = dict(os.environ, UBSAN_OPTIONS="print_stacktrace=1")
    # a preloaded library (if any) stays: ASan is told not to insist on coming first
    env["ASAN_OPTIONS"] = ":".join(x for x in (env.get("ASAN_OPTIONS", ""), "verify_asan_link_order=0") if x)
    r = subprocess.run([os.path.join(host_check.BUILD, request.param)], capture_output=True, text=True, timeout=600, env=env)
    out = r.stdout + r.stderr
    assert r.returncode == 0, out[-4000:]
    for marker in host_check.MARKERS:
        assert marker not in out, out[-4000:]
    assert "path_ss_host: 0 failures" in out, out[-4000:]
    return out


def test_variant_selection_with_the_field_zero_and_set(output):
    m = re.search(r"path_ss_host: (\d+) variant cases with the field zero, (\d+) with it set \(refused: (\d+) tiles, (\d+) stats, "
                  r"(\d+) ordered, (\d+) copy slice, (\d+) factor above 3, (\d+) without views, (\d+) sums too wide, "
                  r"(\d+) another value\), (\d+) descriptors with the field zero, (\d+) in all \((\d+) PATH_SS, (\d+) SHUTTER_SS, "
                  r"(\d+) ANIM_SS\), (\d+) built", output)
    assert m, output[-2000:]
    g = [int(x) for x in m.groups()]
    # anim_host's grid: two full passes and four with a stride over the launches that could take one
    assert g[0] == 2 * 3 * 4 * 2867200 + 4 * 4 * (2867200 * 2 // 5) and g[1] > 0
    assert min(g[2:10]) > 0, "every refusal is reached"
    assert g[10:] == [624, 804, 60, 60, 60, 804]


def test_one_rounding_of_the_whole_mean(output):
    m = re.search(r"path_ss_host: (\d+) sample sets over (\d+) \(s, t\) pairs round to the integer mean", output)
    assert m, output[-2000:]
    # s = 0..3 with t + 2 s <= 8: 9 + 7 + 5 + 3 pairs; 8 fixed pixels x 3 patterns and 10^5 random sets each
    assert int(m.group(2)) == 24 and int(m.group(1)) == 24 * (8 * 3 + 100000)


def test_butterfly_sums_each_block_into_its_leader(output):
    m = re.search(r"path_ss_host: (\d+) block leaders hold exactly their block's sum", output)
    assert m and int(m.group(1)) == 16 + 4 + 1, output[-2000:]
