"""The window scheduler of the host-memory batch calls (charls_amd/csrc/host/host_schedule.h; charls_amd.h part 2i) with fake
lanes: which frames form which window, the offset carry from window to window, alignment gaps, and the capacity rule when the
lanes finish out of order -- every offset, size, errc and copied byte against one serial walk.  Pure C++, no GPU.  The same
scenarios run under AddressSanitizer + UndefinedBehaviorSanitizer and under ThreadSanitizer, as the coalescer's do
(tests/test_coalescer_cpu.py)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _build_and_run(tmp_path, name, extra_flags, env=None):
    exe = tmp_path / name
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-pthread", "-Wall", "-Wextra", *extra_flags,
                           "-I" + os.path.join(ROOT, "charls_amd", "csrc"), "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "host_schedule", "host_schedule_test.cpp"), "-o", str(exe)])
    return subprocess.run([str(exe)], capture_output=True, text=True, timeout=300, env=env)


def _sanitizer_available(flag):
    probe = subprocess.run(["g++", flag, "-x", "c++", "-", "-o", os.devnull], input="int main(){return 0;}", capture_output=True, text=True)
    return probe.returncode == 0


def test_the_scheduler_header_has_no_hip_in_it():
    with open(os.path.join(ROOT, "charls_amd", "csrc", "host", "host_schedule.h")) as f:
        text = f.read()
    assert "#include <hip" not in text and "runtime.h" not in text


def test_lanes_in_any_order_give_the_serial_walk(tmp_path):
    r = _build_and_run(tmp_path, "host_schedule_test", [])
    assert r.returncode == 0 and "host schedule ok" in r.stdout and "FAILED" not in r.stdout, r.stdout + r.stderr


def test_under_address_and_undefined_behavior_sanitizers(tmp_path):
    if not _sanitizer_available("-fsanitize=address,undefined"):
        pytest.skip("this g++ has no libasan / libubsan")
    r = _build_and_run(tmp_path, "host_schedule_asan", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    assert r.returncode == 0 and "host schedule ok" in r.stdout and "FAILED" not in r.stdout, r.stdout + r.stderr
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr


def test_under_thread_sanitizer(tmp_path):
    if not _sanitizer_available("-fsanitize=thread"):
        pytest.skip("this g++ has no libtsan")
    env = dict(os.environ, TSAN_OPTIONS="halt_on_error=0 exitcode=66")
    r = _build_and_run(tmp_path, "host_schedule_tsan", ["-fsanitize=thread"], env=env)
    assert "WARNING: ThreadSanitizer" not in r.stderr, r.stderr[-4000:]
    assert r.returncode == 0 and "host schedule ok" in r.stdout and "FAILED" not in r.stdout, r.stdout + r.stderr
