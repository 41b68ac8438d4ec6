"""The tiny-tree classifier under the sanitizers: wc-path-tracer_amd/csrc/mk_tiny_rule.h -- the function the device scan
evaluates on a draw's BVH buffer -- compiled with AddressSanitizer and UndefinedBehaviorSanitizer into a stand-alone
driver (tests/mk_tiny_rule_asan_driver.cpp) beside the host builders, and run over built trees, every prefix of them and
random node words, each in a heap array of exactly the size the rule is told. A sanitizer report aborts the driver
(-fno-sanitize-recover); its own checks fail it with exit code 1. CPU only."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")
def test_tiny_rule_clean_under_asan_and_ubsan(tmp_path):
    exe = tmp_path / "mk_tiny_rule_asan_driver"
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=all", "-ffp-contract=off",
           os.path.join(ROOT, "tests", "mk_tiny_rule_asan_driver.cpp"),
           os.path.join(ROOT, "wc-path-tracer_amd", "host", "wcpt_host.cpp"), "-o", str(exe)]
    subprocess.run(cmd, check=True, capture_output=True, text=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:halt_on_error=1",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    p = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300, env=env)
    assert p.returncode == 0, (p.stdout[-2000:], p.stderr[-4000:])
    assert "0 failed checks" in p.stdout
    assert "runtime error" not in p.stderr and "AddressSanitizer" not in p.stderr
