"""Host check of the direct kernel's mirrored screen boxes (csrc/rt_view.h mirror_boxes): CPU only.
tests/native/mirror_box_host.cpp, built by tests/native/Makefile as plain host C++ on csrc/rt_scene.h and rt_view.h under ASan + UBSan and run as
a plain executable, draws random scenes (1-11 spheres, 1-3 mirror planes: tilted, next to the camera, the camera on
either side, normals off unit length, spheres touching / cutting / behind the plane, cameras far from the origin)
and, for every sampled pixel outside a sphere's mirrored box whose primary ray meets the plane within t_max, runs
the oracle's binary32 chain -- primary ray, IntersectPlane, reflection, IntersectsSphere -- which must report no
collision.  The same boxes without the added allowances must fail that check (the allowances are needed)."""
import re

import pytest

import host_check


@pytest.fixture(scope="module")
def output():
    return host_check.run("mirror_box_host")


def test_no_sphere_outside_its_mirrored_box_is_hit(output):
    m = re.search(r"mirror_box: (\d+) \(pixel, plane, sphere\) triples outside a box, (\d+) failures", output)
    assert m, output[-2000:]
    assert int(m.group(1)) > 100000, "the check looked at pixels outside boxes"
    assert "triples outside a box, 0 failures" in output
    t = re.search(r"mirror_box: (\d+) tables \((\d+) sphere boxes\), (\d+) planes without one", output)
    assert t and int(t.group(1)) > 0 and int(t.group(2)) > 0 and int(t.group(3)) > 0, "tables, boxes and refused planes"


def test_boxes_without_the_allowances_fail(output):
    m = re.search(r"mirror_box_nomargin: (\d+) triples, (\d+) failures", output)
    assert m, output[-2000:]
    assert int(m.group(2)) > 0, "the check has teeth: prim_box of the mirrored sphere alone is not enough"
