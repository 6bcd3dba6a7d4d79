"""Shared by the host-check tests (test_*_host.py, test_sanitizers.py): one native program of tests/native built and
run.  The programs are stand-alone executables compiled with sanitizers (tests/native/Makefile); nothing is loaded
into python."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NATIVE = os.path.join(ROOT, "tests", "native")
BUILD = os.path.join(NATIVE, "build")
MARKERS = ("ERROR: AddressSanitizer", "runtime error:", "WARNING: ThreadSanitizer", "ERROR: LeakSanitizer")


def run(target, args=(), env_extra=None, make_timeout=1800, run_timeout=300):
    """Make tests/native/build/<target> alone, run it, require exit status 0 and no sanitizer report; its output."""
    subprocess.run(["make", "-s", "-C", NATIVE, "build/" + target], check=True, timeout=make_timeout)
    env = dict(os.environ, UBSAN_OPTIONS="print_stacktrace=1")
    env.update(env_extra or {})
    # a preloaded library (if any) stays: ASan is told not to insist on coming first
    env["ASAN_OPTIONS"] = ":".join(x for x in (env.get("ASAN_OPTIONS", ""), "verify_asan_link_order=0") if x)
    r = subprocess.run([os.path.join(BUILD, target), *args], capture_output=True, text=True, timeout=run_timeout, env=env)
    out = r.stdout + r.stderr
    assert r.returncode == 0, out[-4000:]
    for marker in MARKERS:
        assert marker not in out, out[-4000:]
    return out
