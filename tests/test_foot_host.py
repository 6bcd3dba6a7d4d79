"""Host check of the plane footprints (csrc/rt_foot.h): CPU only.  tests/native/foot_host.cpp, built by
tests/native/Makefile under host-side ASan + UBSan without FMA contraction and run as a plain executable, takes its
views, screen boxes and view tables from the library's csrc/rt_view.h, restates the kernel's primary direction and plane_take's `may` in binary32 and evaluates them at every pixel of 64 x 40, 37 x 23
and 100 x 60 frames for 11 cameras (at the origin, below and exactly on the floor, up to 1e4 away) x 14 pitches x 7
yaws, against plane sets of 0 to 5 planes: the floor, arbitrary normals, normals scaled by 1e-3 and 1e3, |cn| up to
1e6, zero, NaN and inf normals.  Wherever a footprint says "cannot hit", may is false; the same sweep with
footprints built without margins does report failures; and on C3's 1920 x 1080 view the rule and the spheres' screen
boxes leave at least 12,500 of the 32,400 tiles with nothing to trace, none on a view that looks straight down."""
import re

import pytest

import host_check


@pytest.fixture(scope="module")
def output():
    return host_check.run("foot_host")


def test_no_plane_is_selectable_where_its_footprint_excludes_it(output):
    assert "foot_host: 0 failures" in output, output[-4000:]
    m = re.search(r"foot_host: (\d+) views, (\d+) plane sets without footprints, (\d+) rules checked, (\d+) excluded",
                  output)
    assert m, output[-2000:]
    views, off, checked, excluded = map(int, m.groups())
    assert views == 11 * 14 * 7
    # the sweep holds sets the footprints refuse (5 planes, bad normals, far cameras) and excludes a real share
    assert off >= 1000 and checked >= 10_000_000 and excluded >= 1_000_000


def test_footprints_without_margins_fail_the_same_sweep(output):
    m = re.search(r"foot_host: teeth without margins: (\d+) failures of (\d+) excluded", output)
    assert m, output[-2000:]
    failures, excluded = map(int, m.groups())
    assert failures > 0 and excluded >= 1_000_000


def test_effect_on_the_benchmark_view_and_on_a_view_without_sky(output):
    m = re.search(r"foot_host: C3 1920x1080: (\d+) of 32400 tiles skippable", output)
    assert m, output[-2000:]
    assert int(m.group(1)) >= 12500
    assert "foot_host: straight down 1920x1080: 0 of 32400 tiles skippable" in output, output[-2000:]
