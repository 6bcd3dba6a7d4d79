"""Host checks of scene-track shutters (rt_render_anim_shutter[_bands]): CPU only.
tests/native/anim_shutter_host.cpp, built by tests/native/anim_shutter.mk with rt_api.cpp's host code inside, once plain
and once under host-side ASan + UBSan, and run as a stand-alone executable each time on contexts without devices (nothing
is loaded into python, nothing is preloaded), checks the variant selection with LaunchParams::scene_shutter zero (today's
rule, 924 descriptors, a stride with a shutter still refused) and set (the two new modes, 1044 descriptors, every
refusal), and the refusals of both calls through the C ABI in the header's order."""
import os
import re
import subprocess

import pytest

import host_check


@pytest.fixture(scope="module", params=["anim_shutter_host", "anim_shutter_host_asan"])
def output(request):
    subprocess.run(["make", "-s", "-f", "anim_shutter.mk", "-C", host_check.NATIVE], check=True, timeout=1800)
    env = dict(os.environ, UBSAN_OPTIONS="print_stacktrace=1")
    # a preloaded library (if any) stays: ASan is told not to insist on coming first
    env["ASAN_OPTIONS"] = ":".join(x for x in (env.get("ASAN_OPTIONS", ""), "verify_asan_link_order=0") if x)
    r = subprocess.run([os.path.join(host_check.BUILD, request.param)], capture_output=True, text=True, timeout=600, env=env)
    out = r.stdout + r.stderr
    assert r.returncode == 0, out[-4000:]
    for marker in host_check.MARKERS:
        assert marker not in out, out[-4000:]
    assert "anim_shutter_host: 0 failures" in out, out[-4000:]
    return out


def test_variant_selection_with_the_field_zero_and_set(output):
    m = re.search(r"anim_shutter_host: (\d+) variant cases with the field zero \((\d+) refused, (\d+) of them a stride with a shutter\), "
                  r"(\d+) with it set \(refused: (\d+) another value, (\d+) no stride, (\d+) unaligned, (\d+) no shutter, "
                  r"(\d+) shutter above 8, (\d+) without views, (\d+) adaptive, (\d+) view_ss not 0 or 1, (\d+) factor, "
                  r"(\d+) sums too wide, (\d+) tiles, (\d+) stats, (\d+) ordered, (\d+) copy slice\), (\d+) descriptors with the field "
                  r"zero, (\d+) in all \((\d+) ANIM_SHUTTER, (\d+) ANIM_SHUTTER_SS\), (\d+) built", output)
    assert m, output[-2000:]
    g = [int(x) for x in m.groups()]
    assert g[0] > 10 ** 7 and g[1] > 0 and g[2] > 0 and g[3] > 10 ** 6
    assert min(g[4:18]) > 0, "every refusal is reached"
    assert g[18:] == [924, 1044, 60, 60, 1044]


def test_refusals_through_the_c_abi(output):
    m = re.search(r"anim_shutter_host: (\d+) refusals", output)
    # per call 23 in the order's front part and 5 shutters that are no power of two, then 3 band refusals or NULL pixels,
    # then a shutter of 512; and the n_frames * shutter rule asked directly
    assert m and int(m.group(1)) == (24 + 3) + (24 + 1) - 2 + 1, output[-2000:]
