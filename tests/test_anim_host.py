"""Host checks of scene tracks (rt_set_scene_track / rt_render_anim*): CPU only.
tests/native/anim_host.cpp, built by tests/native/anim.mk with rt_api.cpp's host code inside under host-side ASan +
UBSan and run as a plain executable on contexts without devices (nothing is loaded into python, nothing is preloaded),
checks the variant selection with and without a scene stride (564 descriptors, 624 with the 60 ANIM ones), rt_scene.h
track_build against scene_build frame by frame, the launch scalars of mixed tracks, the pooled build against the serial
one and every refusal in its documented order."""
import os
import re
import subprocess

import pytest

import host_check


@pytest.fixture(scope="module")
def output():
    subprocess.run(["make", "-s", "-f", "anim.mk", "-C", host_check.NATIVE], check=True, timeout=1800)
    env = dict(os.environ, UBSAN_OPTIONS="print_stacktrace=1")
    # a preloaded library (if any) stays: ASan is told not to insist on coming first
    env["ASAN_OPTIONS"] = ":".join(x for x in (env.get("ASAN_OPTIONS", ""), "verify_asan_link_order=0") if x)
    r = subprocess.run([os.path.join(host_check.BUILD, "anim_host")], capture_output=True, text=True, timeout=600, env=env)
    out = r.stdout + r.stderr
    assert r.returncode == 0, out[-4000:]
    for marker in host_check.MARKERS:
        assert marker not in out, out[-4000:]
    assert "anim_host: 0 failures" in out, out[-4000:]
    return out


def test_variant_selection_with_and_without_a_scene_stride(output):
    m = re.search(r"anim_host: (\d+) variant cases with the stride 0, (\d+) with it set \((\d+) refused for a shutter, "
                  r"(\d+) without views, (\d+) unaligned\), (\d+) descriptors without a stride, (\d+) in all \((\d+) ANIM\), "
                  r"(\d+) built", output)
    assert m, output[-2000:]
    g = [int(x) for x in m.groups()]
    assert g[0] == 2 * 3 * 4 * 2867200 and g[1] > 0 and min(g[2:5]) > 0
    assert g[5:] == [564, 624, 60, 624]


def test_track_build_equals_scene_build_frame_by_frame(output):
    m = re.search(r"anim_host: (\d+) track slices equal scene_build, (\d+) pooled builds equal the serial one, (\d+) mixed tracks",
                  output)
    assert m, output[-2000:]
    # 5 + 4 + 4 + 3 + 3 frames of the five plain tracks, 4 frames of each of the 4 mixed ones; 3 pool sizes per track
    assert int(m.group(1)) == 19 + 16 and int(m.group(2)) == 3 * 9 and int(m.group(3)) == 4


def test_every_refusal_in_order_without_a_device(output):
    m = re.search(r"anim_host: (\d+) refusals", output)
    assert m and int(m.group(1)) == 12 + 2 * 15 + 1, output[-2000:]
