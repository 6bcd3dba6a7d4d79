"""Host check of the trace kernels' variant selection (rt_internal.h pick_trace_variant): CPU only.
tests/native/variant_host.cpp, built by tests/native/Makefile under host-side ASan + UBSan and run as a plain
executable, enumerates the launch parameters the selection reads (sphere and light counts around every threshold,
every depth class, pow, stats, output format, supersampling 0..4, camera path, frame count, copy slice, tile order
and cost, row order and column-major) and compares each result with the rules written out as one if-chain.  The
descriptors returned are 384, split over the kernels as the code object's are, and exactly those
trace_variant_built admits."""
import re

import pytest

import host_check

# S 7 x L 4 x a2 2 x limit 10 x pow 2 x frames 2, each with 1280 combinations of stats, format, supersampling
# 0..4, views, copy slice, tile order, tile cost, row order and column-major.
GROUPS = 7 * 4 * 2 * 10 * 2 * 2
# Refused of the 1280: with views all but one of 640; without, supersampling 1..3 with tiles, stats, a tile order
# or a tile cost (120 of 128 each), and every one at supersampling 4 (128).
REFUSED = 639 + 3 * 120 + 128


@pytest.fixture(scope="module")
def output():
    return host_check.run("variant_host")


def test_selection_equals_the_rules_written_out(output):
    assert "variant_host: 0 failures" in output, output[-4000:]
    m = re.search(r"variant_host: (\d+) cases, (\d+) refused, (\d+) descriptors, (\d+) built", output)
    assert m, output[-2000:]
    assert int(m.group(1)) == GROUPS * 1280
    assert int(m.group(2)) == GROUPS * REFUSED


def test_descriptors_are_the_384_kernels(output):
    m = re.search(r"variant_host: \d+ cases, \d+ refused, (\d+) descriptors, (\d+) built", output)
    assert m and int(m.group(1)) == 384 and int(m.group(2)) == 384, output[-2000:]
    # per kernel name of the code object: plain / _ss / _path without and with _gpow
    assert "variant_host: direct 72 12 12 / 72 12 12, bundle 66 18 18 / 54 18 18" in output, output[-2000:]
