"""The wavefront launch rules under the sanitizers: wc-path-tracer_amd/csrc/wf_plan.h -- what launch_wavefront evaluates
on every render -- compiled with AddressSanitizer and UndefinedBehaviorSanitizer into a stand-alone driver
(tests/wf_plan_asan_driver.cpp) and run over the frames at the edges of 32 bits and a sweep of frames, modes, options,
occupancies and CU counts, with the plan's invariants checked on each. A sanitizer report aborts the driver
(-fno-sanitize-recover); its own checks fail it with exit code 1. CPU only."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")
def test_wf_plan_clean_under_asan_and_ubsan(tmp_path):
    exe = tmp_path / "wf_plan_asan_driver"
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=all", "-Wall", "-Werror",
           os.path.join(ROOT, "tests", "wf_plan_asan_driver.cpp"), "-o", str(exe)]
    subprocess.run(cmd, check=True, capture_output=True, text=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:halt_on_error=1",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    p = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300, env=env)
    assert p.returncode == 0, (p.stdout[-2000:], p.stderr[-4000:])
    assert "0 failed checks" in p.stdout
    assert "runtime error" not in p.stderr and "AddressSanitizer" not in p.stderr
