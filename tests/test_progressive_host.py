"""Host checks of progressive accumulation (rt_set_progressive): CPU only.
tests/native/progressive_host.cpp, built by tests/native/progressive.mk under host-side ASan + UBSan and run as a
plain executable (nothing is loaded into python, nothing is preloaded), checks the kernels' rounding function against
plain integer division, the sample order against a table, the per-Tick plan over scripted sequences and the variant
selection with and without the new launch fields (564 descriptors, 60 of them PROG)."""
import os
import re
import subprocess

import pytest

import host_check


@pytest.fixture(scope="module")
def output():
    subprocess.run(["make", "-s", "-f", "progressive.mk", "-C", host_check.NATIVE], check=True, timeout=600)
    env = dict(os.environ, UBSAN_OPTIONS="print_stacktrace=1")
    # a preloaded library (if any) stays: ASan is told not to insist on coming first
    env["ASAN_OPTIONS"] = ":".join(x for x in (env.get("ASAN_OPTIONS", ""), "verify_asan_link_order=0") if x)
    r = subprocess.run([os.path.join(host_check.BUILD, "progressive_host")], capture_output=True, text=True, timeout=600, env=env)
    out = r.stdout + r.stderr
    assert r.returncode == 0, out[-4000:]
    for marker in host_check.MARKERS:
        assert marker not in out, out[-4000:]
    assert "progressive_host: 0 failures" in out, out[-4000:]
    return out


def test_rounding_equals_integer_division_for_every_count_and_sum(output):
    m = re.search(r"progressive_host: (\d+) rounding cases, (\d+) against resolve_round_n", output)
    assert m, output[-2000:]
    assert int(m.group(1)) == sum(255 * c + 1 for c in range(1, 65))
    assert int(m.group(2)) == sum(255 * c + 1 for c in (1, 2, 4, 8, 16, 32, 64))


def test_order_and_plan(output):
    m = re.search(r"progressive_host: (\d+) order cases, (\d+) plan ticks", output)
    assert m and int(m.group(1)) == 16 + 4 + 1 + 4 + 16 + 64 and int(m.group(2)) > 3 * (2 * 64 // 8 + 30), output[-2000:]


def test_variant_selection_with_and_without_the_new_fields(output):
    m = re.search(r"progressive_host: (\d+) variant cases with the fields at zero, (\d+) with them set \((\d+) refused\), "
                  r"(\d+) descriptors \((\d+) PROG\), (\d+) built", output)
    assert m, output[-2000:]
    assert int(m.group(1)) == 3 * 4 * 2867200 and int(m.group(2)) > int(m.group(1)) and int(m.group(3)) > 0
    assert (int(m.group(4)), int(m.group(5)), int(m.group(6))) == (564, 60, 564)
