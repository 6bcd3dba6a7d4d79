"""Host check of the camera-path view records (csrc/rt_view.h view_build / view_record behind rt_api.cpp view_fill): CPU only.
tests/native/path_host.cpp, built by tests/native/Makefile under host-side ASan + UBSan and run as a plain
executable, draws random scenes (0, 1, 11, 12, 64 and 65 spheres, with and without mirror planes, with and
without a view height) and random cameras; the DevView record of each camera must equal, byte for byte, the view
fields view_params puts into LaunchParams after rt_set_camera of that camera, and building the records must leave
the context's camera and cached view alone."""
import re

import pytest

import host_check


@pytest.fixture(scope="module")
def output():
    return host_check.run("path_host")


def test_records_equal_the_one_camera_launch_params(output):
    assert "path_host: 0 failures" in output, output[-4000:]
    m = re.search(r"path_host: (\d+) scenes, (\d+) records, (\d+) with screen boxes, (\d+) with mirrored boxes", output)
    assert m, output[-2000:]
    assert int(m.group(1)) == 24 and int(m.group(2)) == 24 * 6
    assert int(m.group(3)) > 0 and int(m.group(4)) > 0, "screen boxes and mirrored boxes were compared"


def test_records_of_different_cameras_differ(output):
    m = re.search(r"path_host: (\d+) record pairs of different cameras differ", output)
    assert m and int(m.group(1)) == 24 * 4, output[-2000:]
