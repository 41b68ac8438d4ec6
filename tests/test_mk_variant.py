"""The megakernel's instances and their selection on the CPU (wc-path-tracer_amd/csrc/mk_variant.h, compiled here with
g++ from the product header through tests/mk_variant_shim.cpp): which of the field combinations are compiled -- 136
pt_megakernel and 8 pt_mk_tail instances, written out here a second time, independently of the header -- every rule
that bounds them, and that the instance a launch takes follows the launch's inputs field by field. No image test sees
the last: an instance picked with the wrong stack kind renders the same bits."""
import ctypes
import itertools
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RENDER, COUNT, DIAG = 0, 1, 2                 # launch modes
NONE, WRITE, READ = 0, 1, 2                   # primary-cache modes
EXACT, FAST = 0, 1                            # arithmetic
WHOLE, HEAD, TAIL = 0, 1, 2                   # stages
FIELDS = ("count", "diag", "stack", "pairs", "single", "reuse", "pcache", "arith", "stage")


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    out = tmp_path_factory.mktemp("mkv") / "libmk_variant_shim.so"
    src = os.path.join(ROOT, "tests", "mk_variant_shim.cpp")
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-shared", "-fPIC", src, "-o", str(out)], check=True)
    lib = ctypes.CDLL(str(out))
    u32, i = ctypes.c_uint32, ctypes.c_int
    ints = ctypes.POINTER(ctypes.c_int)
    lib.mkv_codes.restype = u32
    lib.mkv_decode.argtypes = [u32, ints]
    lib.mkv_decode.restype = None
    lib.mkv_code.argtypes = [ints]
    lib.mkv_code.restype = u32
    lib.mkv_built.argtypes = [ints]
    lib.mkv_built.restype = i
    lib.mkv_select.argtypes = [i, i, i, u32, u32, i, i, i, ints]
    lib.mkv_select.restype = u32
    return lib


def _arr(fields):
    return (ctypes.c_int * 9)(*[int(f) for f in fields])


def _built(shim, v):
    return shim.mkv_built(_arr([v[f] for f in FIELDS])) == 1


def _select(shim, mode=RENDER, stack=1, pairs=1, draws=1, samples=1, pcmode=NONE, arith=EXACT, split=0):
    out = (ctypes.c_int * 18)()
    n = shim.mkv_select(mode, stack, pairs, draws, samples, pcmode, arith, split, out)
    return [dict(zip(FIELDS, out[9 * k:9 * k + 9])) for k in range(n)]


@pytest.fixture(scope="module")
def every(shim):
    """Every field combination once, as the header numbers them."""
    out = []
    for code in range(shim.mkv_codes()):
        a = (ctypes.c_int * 9)()
        shim.mkv_decode(code, a)
        assert shim.mkv_code(a) == code
        out.append(dict(zip(FIELDS, a)))
    assert len({tuple(v.values()) for v in out}) == len(out) == 2 ** 6 * 3 * 2 * 3
    return out


def _kind(v):
    if v["stage"] == TAIL:
        return "tail"
    if v["count"] or v["diag"]:
        return "count"
    return "head" if v["stage"] == HEAD else "render"


def test_exactly_the_instances_of_the_code_object(shim, every):
    built = [v for v in every if _built(shim, v)]
    kinds = [_kind(v) for v in built]
    assert len(built) == 136 + 8
    assert kinds.count("tail") == 8
    assert (kinds.count("render"), kinds.count("head"), kinds.count("count")) == (96, 24, 16)
    # the same set, written out: (count, diag, stack, pairs, single, reuse, pcache, arith, stage)
    b2 = (0, 1)
    want = set()
    for stack, pairs, single, arith, reuse, pc in itertools.product(b2, b2, b2, (EXACT, FAST), b2, (NONE, WRITE, READ)):
        want.add((0, 0, stack, pairs, single, reuse, pc, arith, WHOLE))
    for pairs, single, arith, pc in itertools.product(b2, b2, (EXACT, FAST), (NONE, WRITE, READ)):
        want.add((0, 0, 1, pairs, single, 0, pc, arith, HEAD))
    for diag, stack, pairs, single in itertools.product(b2, b2, b2, b2):
        want.add((1, diag, stack, pairs, single, 0, NONE, EXACT, WHOLE))
    for pairs, single, arith in itertools.product(b2, b2, (EXACT, FAST)):
        want.add((0, 0, 1, pairs, single, 0, NONE, arith, TAIL))
    assert len(want) == 144
    assert {tuple(v[f] for f in FIELDS) for v in built} == want


def test_out_of_range_fields_are_not_built(shim):
    ok = dict(count=0, diag=0, stack=1, pairs=1, single=1, reuse=0, pcache=NONE, arith=EXACT, stage=WHOLE)
    assert _built(shim, ok)
    for f, bad in (("stack", 2), ("stack", -1), ("pcache", 3), ("pcache", -1), ("arith", 2), ("arith", -1), ("stage", 3),
                   ("stage", -1)):
        assert not _built(shim, dict(ok, **{f: bad}))


def test_counting_builds_are_exact_uncached_whole(shim, every):
    counting = [v for v in every if _built(shim, v) and (v["count"] or v["diag"])]
    assert len(counting) == 16
    for v in counting:
        assert v["count"] == 1                   # the diagnostics are counters: never diag alone
        assert v["arith"] == EXACT
        assert v["pcache"] == NONE
        assert v["stage"] == WHOLE
        assert v["reuse"] == 0                   # they trace every sample's primary segment, as the reference does


def test_a_head_is_lds_stack_and_one_sample(shim, every):
    heads = [v for v in every if _built(shim, v) and v["stage"] == HEAD]
    assert len(heads) == 24
    for v in heads:
        assert v["stack"] == 1
        assert v["reuse"] == 0


def test_a_tail_has_no_cache(shim, every):
    tails = [v for v in every if _built(shim, v) and v["stage"] == TAIL]
    assert len(tails) == 8
    for v in tails:
        assert v["pcache"] == NONE
        assert (v["count"], v["diag"], v["reuse"], v["stack"]) == (0, 0, 0, 1)


def test_the_read_form_follows_the_sample_count(shim):
    for stack, pairs, draws, arith in itertools.product((0, 1), (0, 1), (0, 1, 2), (EXACT, FAST)):
        kw = dict(stack=stack, pairs=pairs, draws=draws, arith=arith, pcmode=READ)
        (one,) = _select(shim, samples=1, **kw)
        assert (one["pcache"], one["reuse"]) == (READ, 0)   # its sample count is the constant 1
        for samples in (2, 3, 16):
            (many,) = _select(shim, samples=samples, **kw)
            assert (many["pcache"], many["reuse"]) == (READ, 1)
    for pcmode in (NONE, WRITE):
        assert _select(shim, samples=1, pcmode=pcmode)[0]["reuse"] == 0
        assert _select(shim, samples=2, pcmode=pcmode)[0]["reuse"] == 1


def test_fast_only_in_render_mode(shim):
    for mode, split, pcmode in itertools.product((COUNT, DIAG), (0, 1), (NONE, WRITE, READ)):
        (v,) = _select(shim, mode=mode, arith=FAST, split=split, pcmode=pcmode)
        assert v["arith"] == EXACT and v["count"] == 1
    assert _select(shim, mode=RENDER, arith=FAST)[0]["arith"] == FAST
    assert _select(shim, mode=RENDER, arith=EXACT)[0]["arith"] == EXACT


CROSS = list(itertools.product((RENDER, COUNT, DIAG), (0, 1), (0, 1), (0, 1, 2), (1, 2, 16), (NONE, WRITE, READ),
                               (EXACT, FAST), (0, 1)))


def test_every_selection_is_built_and_follows_its_inputs(shim):
    assert len(CROSS) == 3 * 2 * 2 * 3 * 3 * 3 * 2 * 2
    for mode, stack, pairs, draws, samples, pcmode, arith, split in CROSS:
        sel = _select(shim, mode, stack, pairs, draws, samples, pcmode, arith, split)
        assert len(sel) in (1, 2)
        for v in sel:
            assert _built(shim, v), (mode, stack, pairs, draws, samples, pcmode, arith, split, v)
            assert v["stack"] == stack          # the option, whatever else is chosen
            assert v["pairs"] == pairs
            assert v["single"] == (1 if draws == 1 else 0)
            assert v["count"] == (0 if mode == RENDER else 1)
            assert v["diag"] == (1 if mode == DIAG else 0)
            assert v["arith"] == (arith if mode == RENDER else EXACT)
        assert sel[0]["pcache"] == (pcmode if mode == RENDER else NONE)
        splits = bool(split) and mode == RENDER and stack == 1 and samples == 1
        assert len(sel) == (2 if splits else 1)
        if not splits:
            assert sel[0]["stage"] == WHOLE
            if mode == RENDER:
                assert sel[0]["reuse"] == (1 if samples > 1 else 0)
            else:
                assert sel[0]["reuse"] == 0


def test_a_split_request_is_head_then_tail(shim):
    for pairs, draws, pcmode, arith in itertools.product((0, 1), (0, 1, 2), (NONE, WRITE, READ), (EXACT, FAST)):
        head, tail = _select(shim, stack=1, pairs=pairs, draws=draws, samples=1, pcmode=pcmode, arith=arith, split=1)
        assert head["stage"] == HEAD and tail["stage"] == TAIL
        for f in ("pairs", "single", "arith", "stack"):
            assert head[f] == tail[f]
        assert head["pcache"] == pcmode and tail["pcache"] == NONE
        assert head["reuse"] == 0 and tail["reuse"] == 0
    # what has no head stays whole: the scratch stack, more than one sample, the counting runs
    assert len(_select(shim, stack=0, split=1)) == 1
    assert len(_select(shim, samples=2, split=1)) == 1
    assert len(_select(shim, mode=COUNT, split=1)) == 1
    assert len(_select(shim, mode=DIAG, split=1)) == 1


def test_any_nonzero_stack_kind_is_the_lds_stack(shim):
    """launch_megakernel's stack_kind is 0 for the scratch stack and anything else for the LDS stack."""
    assert _select(shim, stack=0)[0]["stack"] == 0
    for kind in (1, 2, 7):
        assert _select(shim, stack=kind)[0]["stack"] == 1
