"""Host checks of adaptive path and track launches (rt_set_path_adaptive_sampling): CPU only.
tests/native/path_adaptive_host.cpp, built by tests/native/path_adaptive.mk once plain and once under ASan + UBSan and run
as a stand-alone executable each time (nothing is loaded into python, nothing is preloaded), checks the variant selection
with LaunchParams::view_adapt zero (today's rule over path_ss_host's grid, 804 descriptors) and set (the two new modes, 924
descriptors, every refusal), the variant word, and that the field lies in the block's tail padding (static_asserts)."""
import os
import re
import subprocess

import pytest

import host_check


@pytest.fixture(scope="module", params=["path_adaptive_host", "path_adaptive_host_asan"])
def output(request):
    subprocess.run(["make", "-s", "-f", "path_adaptive.mk", "-C", host_check.NATIVE], check=True, timeout=1800)
    env = dict(os.environ, UBSAN_OPTIONS="print_stacktrace=1")
    # a preloaded library (if any) stays: ASan is told not to insist on coming first
    env["ASAN_OPTIONS"] = ":".join(x for x in (env.get("ASAN_OPTIONS", ""), "verify_asan_link_order=0") if x)
    r = subprocess.run([os.path.join(host_check.BUILD, request.param)], capture_output=True, text=True, timeout=600, env=env)
    out = r.stdout + r.stderr
    assert r.returncode == 0, out[-4000:]
    for marker in host_check.MARKERS:
        assert marker not in out, out[-4000:]
    assert "path_adaptive_host: 0 failures" in out, out[-4000:]
    return out


def test_variant_selection_with_the_field_zero_and_set(output):
    m = re.search(r"path_adaptive_host: (\d+) variant cases with the field zero \((\d+) refused\), (\d+) with it set \(refused: "
                  r"(\d+) without views, (\d+) view_ss not 1, (\d+) factor 0, (\d+) factor above 3, (\d+) shutter, "
                  r"(\d+) value outside 1\.\.256, (\d+) tiles, (\d+) stats, (\d+) ordered, (\d+) copy slice\), "
                  r"(\d+) descriptors with the field zero, (\d+) in all \((\d+) PATH_ADAPT, (\d+) ANIM_ADAPT\), (\d+) built", output)
    assert m, output[-2000:]
    g = [int(x) for x in m.groups()]
    # path_ss_host's grid: anim_host's (two full passes and four with a stride) and its own three passes with view_ss set
    assert g[0] > 2 * 3 * 4 * 2867200 + 4 * 4 * (2867200 * 2 // 5) and g[1] > 0 and g[2] > 0
    assert min(g[3:13]) > 0, "every refusal is reached"
    assert g[13:] == [804, 924, 60, 60, 924]
