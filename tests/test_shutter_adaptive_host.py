"""Host checks of adaptive shutters (rt_set_shutter_adaptive_sampling): CPU only.
tests/native/shutter_adaptive_host.cpp, built by tests/native/shutter_adaptive.mk with rt_api.cpp's host code inside, once
plain and once under host-side ASan + UBSan, and run as a stand-alone executable each time on contexts without devices
(nothing is loaded into python, nothing is preloaded), checks the variant selection with LaunchParams::shutter_adapt zero
(today's rule, the 1044 earlier descriptors, view_adapt with a shutter still refused) and set (the two new modes, every
refusal, distinct variant words), counts the built descriptors, pins the layout of the block, and asks the setting's
rules through the C ABI."""
import os
import re
import subprocess

import pytest

import host_check


@pytest.fixture(scope="module", params=["shutter_adaptive_host", "shutter_adaptive_host_asan"])
def output(request):
    subprocess.run(["make", "-s", "-f", "shutter_adaptive.mk", "-C", host_check.NATIVE], check=True, timeout=1800)
    env = dict(os.environ, UBSAN_OPTIONS="print_stacktrace=1")
    # a preloaded library (if any) stays: ASan is told not to insist on coming first
    env["ASAN_OPTIONS"] = ":".join(x for x in (env.get("ASAN_OPTIONS", ""), "verify_asan_link_order=0") if x)
    r = subprocess.run([os.path.join(host_check.BUILD, request.param)], capture_output=True, text=True, timeout=600, env=env)
    out = r.stdout + r.stderr
    assert r.returncode == 0, out[-4000:]
    for marker in host_check.MARKERS:
        assert marker not in out, out[-4000:]
    assert "shutter_adaptive_host: 0 failures" in out, out[-4000:]
    return out


def test_variant_selection_with_the_field_zero_and_set(output):
    m = re.search(r"shutter_adaptive_host: (\d+) variant cases with the field zero \((\d+) refused, (\d+) of them view_adapt with a shutter\), "
                  r"(\d+) with it set \(refused: (\d+) value, (\d+) without views, (\d+) view_ss not 1, (\d+) factor, (\d+) no shutter, "
                  r"(\d+) shutter above 8, (\d+) sums too wide, (\d+) view_adapt, (\d+) scene, (\d+) tiles, (\d+) stats, (\d+) ordered, "
                  r"(\d+) copy slice\), (\d+) descriptors with the field zero, (\d+) in all \((\d+) SHUTTER_ADAPT, (\d+) ANIM_SHUTTER_ADAPT\), "
                  r"(\d+) built", output)
    assert m, output[-2000:]
    g = [int(x) for x in m.groups()]
    assert g[0] > 10 ** 7 and g[1] > 0 and g[2] > 0 and g[3] > 10 ** 6
    assert min(g[4:17]) > 0, "every refusal is reached"
    n_zero, n_all, n_cam, n_track, n_built = g[17:]
    assert n_zero == 1044, "the earlier descriptors, unchanged"
    # (the new modes are counted, not assumed: as many each as any views mode has, and all of them built)
    assert n_cam == n_track > 0 and n_all == n_zero + n_cam + n_track == n_built


def test_the_setting_through_the_c_abi(output):
    m = re.search(r"shutter_adaptive_host: (\d+) refusals", output)
    # the NULL context and the getter's two NULLs, 3 thresholds outside 0..256, the path threshold alone, m k^2 above 256, and
    # the band rule under the shutter threshold and under the path threshold
    assert m and int(m.group(1)) == 3 + 3 + 1 + 1 + 2, output[-2000:]
