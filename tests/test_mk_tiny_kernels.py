"""Which renders take the walk-only kernels (wc-path-tracer_amd/csrc/mk_tiny_rule.h mk_tiny_kernels, the one statement
of it: pt_kernels.hip launch_megakernel calls the same function). tests/mk_tiny_kernels_shim.cpp prints the function over
its whole truth table -- mode, the draw's tiny-tree flag, split, pair records, single draw, arithmetic -- and this test
holds every row against the rule as the kernels' list states it: a render, the flag, a split, pair records, one draw
command, exact arithmetic, and nothing else. The shim is a stand-alone program built with AddressSanitizer and
UndefinedBehaviorSanitizer. CPU only."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODE_RENDER, ARITH_EXACT = 0, 0


@pytest.fixture(scope="module")
def table(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    exe = tmp_path_factory.mktemp("mk_tiny_kernels") / "mk_tiny_kernels_shim"
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=all", os.path.join(ROOT, "tests", "mk_tiny_kernels_shim.cpp"), "-o", str(exe)]
    subprocess.run(cmd, check=True, capture_output=True, text=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    p = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60, env=env)
    assert p.returncode == 0, (p.stdout[-2000:], p.stderr[-4000:])
    assert "runtime error" not in p.stderr and "AddressSanitizer" not in p.stderr
    return p.stdout.splitlines()


def test_the_whole_truth_table(table):
    rows = [l for l in table if "->" in l]
    assert len(rows) == 3 * 2 * 2 * 2 * 2 * 2 and f"{len(rows)} lines" in table
    seen = set()
    for l in rows:
        args, got = l.split("->")
        mode, tiny, split, pairs, single, arith = (int(v) for v in args.split())
        want = mode == MODE_RENDER and tiny == 1 and split == 1 and pairs == 1 and single == 1 and arith == ARITH_EXACT
        assert int(got) == int(want), l
        seen.add((mode, tiny, split, pairs, single, arith))
    assert len(seen) == len(rows)
    assert sum(int(l.split("->")[1]) for l in rows) == 1   # one combination: the four kernels are all there is


def test_each_condition_alone_keeps_the_general_kernels(table):
    """from the one row that takes the walk-only pair, flipping any single input leaves it"""
    rows = {tuple(int(v) for v in l.split("->")[0].split()): int(l.split("->")[1]) for l in table if "->" in l}
    yes = (MODE_RENDER, 1, 1, 1, 1, ARITH_EXACT)
    assert rows[yes] == 1
    for i in range(6):
        for other in ((1, 2) if i == 0 else (1 - yes[i],)):
            flipped = yes[:i] + (other,) + yes[i + 1:]
            assert rows[flipped] == 0, flipped


def test_the_selection_it_is_fed(table):
    """a split one-sample render on pair records with one draw: mk_variant_select's head carries the fields the launch
    passes on"""
    assert "select 2 1 1 0" in table
