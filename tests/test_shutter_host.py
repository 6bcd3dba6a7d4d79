"""Host checks of the camera-path shutter (rt_render_shutter_bands / rt_render_shutter): CPU only.
tests/native/shutter_host.cpp, built by tests/native/Makefile under host-side ASan + UBSan and run as a plain
executable, checks resolve_round_n against per-channel integer arithmetic, the variant selection with a shutter
(444 descriptors, 384 of them without one), the argument checks of both entry points on a context without devices,
and the order of a shutter launch's view table."""
import re

import pytest

import host_check


@pytest.fixture(scope="module")
def output():
    out = host_check.run("shutter_host")
    assert "shutter_host: 0 failures" in out, out[-4000:]
    return out


def test_resolve_round_n_equals_per_channel_integer_arithmetic(output):
    m = re.search(r"shutter_host: (\d+) resolve cases", output)
    assert m and int(m.group(1)) > 8 * 20 ** 3, output[-2000:]


def test_variant_selection_with_a_shutter(output):
    m = re.search(r"shutter_host: (\d+) variant cases, (\d+) refused, (\d+) descriptors \((\d+) without a shutter, "
                  r"(\d+) SHUTTER\), (\d+) built", output)
    assert m, output[-2000:]
    assert int(m.group(1)) == 4 * 2867200 and int(m.group(2)) > 0
    assert (int(m.group(3)), int(m.group(4)), int(m.group(5)), int(m.group(6))) == (444, 384, 60, 444)


def test_argument_checks_come_before_any_device_call(output):
    m = re.search(r"shutter_host: (\d+) argument checks", output)
    assert m and int(m.group(1)) >= 60, output[-2000:]


def test_view_table_order(output):
    m = re.search(r"shutter_host: (\d+) table records, (\d+) differ from record 0", output)
    assert m and (int(m.group(1)), int(m.group(2))) == (48, 44), output[-2000:]
