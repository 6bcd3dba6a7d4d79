"""Host checks of adaptive supersampling (rt_set_adaptive_sampling): CPU only.
tests/native/adaptive_host.cpp, built by tests/native/Makefile under host-side ASan + UBSan and run as a plain
executable, checks the kernels' difference / threshold function against plain integer code, the argument checks of
both calls, the band-row rule on a context without devices, and the variant selection with a threshold (504
descriptors, 444 of them without one and selected as before)."""
import re

import pytest

import host_check


@pytest.fixture(scope="module")
def output():
    out = host_check.run("adaptive_host", run_timeout=600)
    assert "adaptive_host: 0 failures" in out, out[-4000:]
    return out


def test_difference_function_equals_plain_integer_code(output):
    m = re.search(r"adaptive_host: (\d+) difference cases", output)
    assert m and int(m.group(1)) == 4 * 256 * 256 * 7, output[-2000:]


def test_argument_checks_and_the_band_row_rule(output):
    m = re.search(r"adaptive_host: (\d+) argument checks, (\d+) band checks", output)
    assert m and int(m.group(1)) >= 14 and int(m.group(2)) > 6 * 1100 + 9 * 3 * 8 * 2, output[-2000:]


def test_variant_selection_with_a_threshold(output):
    m = re.search(r"adaptive_host: (\d+) variant cases, (\d+) refused, (\d+) descriptors \((\d+) without a threshold, "
                  r"(\d+) ADAPT\), (\d+) built", output)
    assert m, output[-2000:]
    assert int(m.group(1)) == 3 * 4 * 2867200 and int(m.group(2)) > 0
    assert (int(m.group(3)), int(m.group(4)), int(m.group(5)), int(m.group(6))) == (504, 444, 60, 504)
