"""The stand-alone host harnesses of tools/host_sanitize under AddressSanitizer + UBSan: one build
line, one environment, one set of assertions for every test that runs one."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIR = os.path.join(ROOT, "tools", "host_sanitize")


def run_sanitized(tmp_path, name, extra_sources=(), timeout=120, args=()):
    """Build tools/host_sanitize/<name>_harness.cpp (and extra_sources) with -fsanitize=address,undefined
    into tmp_path, run it with `args`, and return its stdout.  Skips where the sanitizer build itself
    is unavailable; an error of the harness's own source fails.  Asserts a clean exit, no UBSan
    report, and the closing "<name> harness ok" with no failed CHECK."""
    source = f"{name}_harness.cpp"
    exe = str(tmp_path / f"{name}_harness")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
                        "-fno-omit-frame-pointer", os.path.join(DIR, source), *extra_sources, "-o", exe],
                       capture_output=True, text=True)
    if r.returncode != 0 and "sanitize" in r.stderr and source not in r.stderr:
        pytest.skip(f"sanitizer build unavailable: {r.stderr[-300:]}")
    assert r.returncode == 0, r.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1",
               UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([exe, *args], capture_output=True, text=True, env=env, timeout=timeout)
    assert r.returncode == 0 and "runtime error" not in r.stderr, (r.stdout[-2000:], r.stderr[-3000:])
    assert f"{name} harness ok" in r.stdout and "FAILED" not in r.stdout
    return r.stdout
