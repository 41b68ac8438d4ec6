"""The wavefront renderer's launch rules on the CPU (wc-path-tracer_amd/csrc/wf_plan.h, compiled here with g++ from the
product header through tests/wf_plan_shim.cpp): the twelve wf_trace instances, the instance a launch selects, and the
frame's plan -- persistent trace or not, the pipeline count, the grids, each pipeline's share, fetch rounds and
iterations -- against pinned cases and against tests/wf_plan_cases.py, a plain Python model written from the host code
that held these rules before. A wrong rule here renders no wrong pixel: it is a silent slowdown, or a test that quietly
runs another instance, so this is where it is caught."""
import ctypes

import pytest

import wf_plan_cases as model
import wf_record
from wf_plan_cases import RENDER, COUNT, DIAG

HEAD = ("ok", "empty", "persist", "W", "rows", "K", "trace_grid", "shade_grid", "persist_grid")
PIPE = ("tiles", "total", "paths", "init_grid", "geo", "iters")


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    """tests/wf_plan_shim.cpp built with g++ and loaded: once per process, also for the GPU modules that import this."""
    return wf_record.shim_library(lambda: tmp_path_factory.mktemp("wfp"))


def _v(fields):
    return (ctypes.c_int * 5)(*[int(f) for f in fields])


def _select(shim, mode=RENDER, draws=1, fast=1, lds_stack=0):
    out = (ctypes.c_int * 5)()
    shim.wfp_select(mode, draws, fast, lds_stack, out)
    return tuple(out)


# the pinned cases' setting: 256 CUs, 32 and 16 blocks per CU, one draw on the fast layout, one sample, render mode,
# every option automatic, overlap on
BASE = dict(mode=RENDER, draws=1, fast=1, lds_stack=0, W=1920, rows=1080, samples=1, max_bounce=4, wf_fetch=-1,
            wf_persist=-1, pipes=0, sort=0, overlap=1, cus=256, trace_bpc=32, persist_bpc=16)


def _words(shim, kw):
    """the shim's 18 input words: what launch_wavefront hands wf_frame_plan"""
    base = _select(shim, kw["mode"], kw["draws"], kw["fast"], kw["lds_stack"])
    sort = 1 if (kw["sort"] and kw["draws"] > 0) else 0   # the sort as it runs
    return (ctypes.c_int64 * 18)(*base, kw["mode"], kw["W"], kw["rows"], kw["samples"], kw["max_bounce"], kw["wf_fetch"],
                                 kw["wf_persist"], kw["pipes"], sort, kw["overlap"], kw["cus"], kw["trace_bpc"],
                                 kw["persist_bpc"])


def _plan(shim, **over):
    kw = dict(BASE, **over)
    out = (ctypes.c_int64 * (9 + 11 * 4))()
    shim.wfp_plan(_words(shim, kw), out)
    p = dict(zip(HEAD, out[:9]))
    for f in ("ok", "empty", "persist"):
        p[f] = bool(p[f])
    p["pipe"] = []
    for j in range(4):
        o = out[9 + 11 * j:9 + 11 * (j + 1)]
        if j < p["K"]:
            p["pipe"].append(dict(zip(PIPE, o[:6]), variant=tuple(o[6:])))
        else:
            assert list(o) == [0] * 11   # nothing past the last pipeline
    return p


def _share(shim, W, rows, j, K):
    out = (ctypes.c_uint32 * 3)()
    shim.wfp_share(W, rows, j, K, out)
    return tuple(out)


@pytest.fixture(scope="module")
def every(shim):
    """Every field combination once, as the header numbers them."""
    out = []
    for code in range(shim.wfp_codes()):
        a = (ctypes.c_int * 5)()
        shim.wfp_decode(code, a)
        assert shim.wfp_code(a) == code
        out.append(tuple(a))
    assert len(set(out)) == len(out) == 2 * 2 * 4 * 3 * 2
    return out


# ---- the instance list -------------------------------------------------------------------------------------------

def test_exactly_the_twelve_instances(shim, every):
    built = {v for v in every if shim.wfp_built(_v(v)) == 1}
    assert len(built) == 12
    assert built == model.BUILT
    # by kind: (count, diag, geo, ldsn, persist)
    assert {v for v in built if not v[0] and not v[4]} == {(0, 0, 0, 10, 0), (0, 0, 1, 10, 0), (0, 0, 1, 16, 0),
                                                           (0, 0, 1, 24, 0), (0, 0, 2, 10, 0), (0, 0, 3, 10, 0)}
    assert {v[2] for v in built if v[0] and not v[1]} == {0, 1}
    assert {v[2] for v in built if v[1]} == {0, 1}
    assert {v[2] for v in built if v[4]} == {2, 3}
    assert all(v[3] == 10 for v in built if v[2] != 1)


def test_out_of_range_fields_are_not_built(shim):
    assert shim.wfp_built(_v((0, 0, 1, 16, 0))) == 1
    for bad in ((0, 0, 4, 10, 0), (0, 0, -1, 10, 0), (0, 0, 1, 12, 0), (0, 0, 1, 0, 0), (0, 1, 1, 10, 0), (1, 0, 2, 10, 0),
                (1, 0, 1, 16, 0), (0, 0, 1, 10, 1), (1, 0, 2, 10, 1), (0, 0, 2, 16, 0)):
        assert shim.wfp_built(_v(bad)) == 0, bad


def test_the_persistent_instance(shim):
    out = (ctypes.c_int * 5)()
    shim.wfp_persist_variant(out)
    assert tuple(out) == (0, 0, model.PERSIST_GEO, 10, 1)
    assert shim.wfp_built(out) == 1


# ---- the selection -----------------------------------------------------------------------------------------------

def test_selection_follows_the_old_ladder(shim):
    for mode in (RENDER, COUNT, DIAG):
        for draws in (0, 1, 2, 3):
            for fast in (0, 1):
                for stack in (-1, 0, 7, 10, 16, 24, 32):
                    got = _select(shim, mode, draws, fast, stack)
                    assert got == model.select(mode, draws, fast, stack), (mode, draws, fast, stack)
                    assert shim.wfp_built(_v(got)) == 1
                    assert got[4] == 0


def test_selection_rules(shim):
    assert _select(shim) == (0, 0, 2, 10, 0)
    assert _select(shim, fast=0) == (0, 0, 1, 10, 0)
    assert _select(shim, lds_stack=16) == (0, 0, 1, 16, 0)      # a deeper stack leaves the fast layout
    assert _select(shim, lds_stack=24, fast=0) == (0, 0, 1, 24, 0)
    assert _select(shim, lds_stack=12) == (0, 0, 2, 10, 0)      # normalised to 10
    assert _select(shim, draws=2, lds_stack=24) == (0, 0, 0, 10, 0)
    assert _select(shim, draws=0) == (0, 0, 0, 10, 0)
    assert _select(shim, mode=COUNT, draws=2, lds_stack=16) == (1, 0, 0, 10, 0)   # counting runs ignore the stack option
    assert _select(shim, mode=COUNT, lds_stack=16) == (1, 0, 1, 10, 0)
    assert _select(shim, mode=DIAG, lds_stack=24) == (1, 1, 1, 10, 0)


def test_persist_eligibility(shim):
    fast, plain = _v((0, 0, 2, 10, 0)), _v((0, 0, 1, 10, 0))
    assert shim.wfp_persist_eligible(fast, 1, 0, -1) == 1
    assert shim.wfp_persist_eligible(fast, 1, 0, 1) == 1
    assert shim.wfp_persist_eligible(fast, 1, 0, 0) == 0        # the option
    assert shim.wfp_persist_eligible(fast, 2, 0, 1) == 0        # one sample only
    assert shim.wfp_persist_eligible(fast, 1, 1, 1) == 0        # unsorted only
    assert shim.wfp_persist_eligible(plain, 1, 0, 1) == 0       # the fast layout only
    assert shim.wfp_persist_eligible(_v((1, 0, 1, 10, 0)), 1, 0, 1) == 0


# ---- pinned plans ------------------------------------------------------------------------------------------------

def test_pinned_1080p(shim):
    p = _plan(shim)
    assert (p["ok"], p["empty"], p["persist"]) == (True, False, False)
    assert (p["K"], p["trace_grid"], p["shade_grid"], p["persist_grid"]) == (3, 2730, 1024, 0)
    for q in p["pipe"]:
        assert (q["paths"], q["total"], q["init_grid"], q["geo"]) == (691200, 691200, 2700, 3)
        assert q["variant"] == (0, 0, 3, 10, 0)


def test_pinned_4k(shim):
    p = _plan(shim, W=3840, rows=2160)
    assert (p["K"], p["trace_grid"], p["persist"]) == (2, 4096, False)
    for q in p["pipe"]:
        assert (q["paths"], q["geo"]) == (4147200, 2)
        assert q["init_grid"] == 4096           # capped at 16 blocks per CU
        assert q["variant"] == (0, 0, 2, 10, 0)


def test_pinned_row_block_persists(shim):
    p = _plan(shim, rows=135)
    assert (p["persist"], p["K"], p["persist_grid"]) == (True, 2, 2048)
    assert [q["paths"] for q in p["pipe"]] == [130560, 130560]
    assert all(q["variant"] == (0, 0, model.PERSIST_GEO, 10, 1) and q["geo"] == model.PERSIST_GEO for q in p["pipe"])
    p = _plan(shim, rows=135, overlap=0)
    assert (p["persist"], p["K"], p["persist_grid"]) == (True, 1, 4096)
    assert (p["pipe"][0]["total"], p["pipe"][0]["paths"]) == (261120, 259200)


def test_pinned_persist_threshold(shim):
    assert 345600 * 5 <= 64 * 7 * 4096 < 414720 * 5
    assert _plan(shim, rows=180, overlap=0)["persist"] is True
    p = _plan(shim, rows=216, overlap=0)
    assert (p["persist"], p["K"], p["trace_grid"]) == (False, 3, 2730)


def test_pinned_small_frames(shim):
    p = _plan(shim, W=8, rows=8, pipes=4)
    assert (p["K"], p["pipe"][0]["paths"]) == (1, 64)
    p = _plan(shim, W=9, rows=8, pipes=4, samples=2)
    assert (p["K"], p["persist"]) == (2, False)
    assert [q["paths"] for q in p["pipe"]] == [64, 64]


def test_pinned_sort_and_count(shim):
    p = _plan(shim, sort=1, pipes=3, wf_persist=1)
    assert (p["K"], p["persist"]) == (1, False)
    p = _plan(shim, mode=COUNT, draws=2, lds_stack=16)
    assert all(q["geo"] == 0 and q["variant"] == (1, 0, 0, 10, 0) for q in p["pipe"])


# ---- options -----------------------------------------------------------------------------------------------------

def test_fetch_option_overrides_the_pipeline_geo(shim):
    assert {q["geo"] for q in _plan(shim, wf_fetch=0)["pipe"]} == {2}                  # 1080p: short queues, yet two rounds
    assert {q["geo"] for q in _plan(shim, W=3840, rows=2160, wf_fetch=1)["pipe"]} == {3}   # 4K: long queues, yet one
    assert {q["geo"] for q in _plan(shim, fast=0, wf_fetch=1)["pipe"]} == {1}              # only on the fast layout
    # the threshold's second use compares one pipeline's paths with the divided grid: 8 * 64 * 2730 = 1397760
    assert shim.wfp_short_queue(1397760, 2730) == 1 and shim.wfp_short_queue(1397761, 2730) == 0


def test_persist_option(shim):
    assert _plan(shim, wf_persist=0, rows=135)["persist"] is False
    p = _plan(shim, wf_persist=1)                       # the whole frame, far past 1.4 paths per lane
    assert (p["persist"], p["K"], p["persist_grid"]) == (True, 2, 2048)
    assert _plan(shim, wf_persist=1, samples=2)["persist"] is False
    assert _plan(shim, wf_persist=1, fast=0)["persist"] is False
    assert _plan(shim, wf_persist=1, mode=COUNT)["persist"] is False
    assert _plan(shim, wf_persist=1, pipes=3)["persist_grid"] == 4096 // 3


def test_pipes_option(shim):
    for pipes, K in ((1, 1), (2, 2), (3, 3), (4, 4), (5, 4), (100, 4)):
        p = _plan(shim, pipes=pipes)
        assert p["K"] == K == len(p["pipe"])
        assert p["trace_grid"] == 8192 // K
    assert _plan(shim, pipes=-3)["K"] == 3              # below 1: by queue length
    assert _plan(shim, pipes=4, mode=DIAG)["K"] == 1    # one diagnostics block
    assert _plan(shim, pipes=4, mode=COUNT)["K"] == 4
    assert _plan(shim, pipes=4, sort=1)["K"] == 1
    assert _plan(shim, pipes=4, sort=1, draws=0)["K"] == 4   # nothing to sort by: the sort does not run
    # the threshold's first use compares the whole frame with the undivided grid: 8 * 64 * 8192 = 4194304 paths
    assert _plan(shim, W=2048, rows=2048)["K"] == 3 and _plan(shim, W=2048, rows=2049)["K"] == 2


def test_iterations(shim):
    assert {q["iters"] for q in _plan(shim, samples=1, max_bounce=4)["pipe"]} == {5}
    assert {q["iters"] for q in _plan(shim, samples=3, max_bounce=4)["pipe"]} == {5 + 2 * 4}   # primary records reused
    assert {q["iters"] for q in _plan(shim, mode=COUNT, samples=3, max_bounce=4)["pipe"]} == {15}
    assert {q["iters"] for q in _plan(shim, mode=COUNT, samples=1, max_bounce=4)["pipe"]} == {5}
    assert shim.wfp_iterations(RENDER, 1, (1 << 20) - 1) == 1 << 20
    assert shim.wfp_iterations(RENDER, 1, 1 << 20) == 1 << 20
    assert shim.wfp_iterations(RENDER, 2, 0) == 1
    assert shim.wfp_iterations(COUNT, 0xFFFFFFFF, 0xFFFFFFFF) == 1 << 20
    assert shim.wfp_iterations(RENDER, 0xFFFFFFFF, 0xFFFFFFFF) == 1 << 20
    assert shim.wfp_iterations(RENDER, 0, 7) == 0


# ---- edges -------------------------------------------------------------------------------------------------------

def test_empty_frames(shim):
    for W, rows in ((0, 0), (0, 1080), (1920, 0), (0, 0xFFFFFFFF), (0xFFFFFFFF, 0)):
        p = _plan(shim, W=W, rows=rows)
        assert (p["ok"], p["empty"], p["K"], p["pipe"]) == (True, True, 0, [])


def test_lane_count_limit(shim):
    # 2^26 - 1 tiles: 0xFFFFFFC0 lanes, the last count accepted
    p = _plan(shim, W=8, rows=8 * (2 ** 26 - 1), pipes=1)
    assert (p["ok"], p["empty"], p["K"]) == (True, False, 1)
    assert (p["pipe"][0]["tiles"], p["pipe"][0]["total"], p["pipe"][0]["paths"]) == (2 ** 26 - 1, 0xFFFFFFC0, 0xFFFFFFC0)
    assert p["pipe"][0]["init_grid"] == 4096
    p = _plan(shim, W=1, rows=8 * (2 ** 26 - 1), pipes=4)
    assert p["ok"] and sum(q["tiles"] for q in p["pipe"]) == 2 ** 26 - 1
    assert all(q["paths"] == 8 * (2 ** 26 - 1) for q in p["pipe"])   # a share's lanes exceed the frame's pixels: the bound
    # one tile more: 2^32 lanes, with fewer than 2^32 pixels
    assert 65529 * 65529 < 2 ** 32
    assert _plan(shim, W=65529, rows=65529)["ok"] is False
    assert _plan(shim, W=1, rows=8 * (2 ** 26 - 1) + 1)["ok"] is False


def test_pixel_count_limit(shim):
    assert _plan(shim, W=65536, rows=65536)["ok"] is False           # 2^32 pixels
    assert _plan(shim, W=0xFFFFFFFF, rows=0xFFFFFFFF)["ok"] is False  # every product in 64 bits
    assert _plan(shim, W=0xFFFFFFFF, rows=2)["ok"] is False
    assert _plan(shim, W=0x80000000, rows=2)["ok"] is False
    # the most pixels a frame can have within the lane limit, as one row and as one column
    for W, rows in ((0xFFFFFFC0 // 8, 8), (8, 0xFFFFFFC0 // 8)):
        p = _plan(shim, W=W, rows=rows, pipes=2)
        assert p["ok"] and [q["paths"] for q in p["pipe"]] == [0x80000000, 0x7FFFFFC0]


# ---- the sweep ---------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def swept(shim):
    cases = list(model.sweep())
    assert len(cases) >= 20000
    return [(kw, _plan(shim, **kw)) for kw in cases]


def test_sweep_against_the_model(shim, swept):
    seen = set()
    for kw, got in swept:
        want = model.plan(**kw)
        for f in HEAD:
            assert got[f] == want[f], (f, kw, got, want)
        assert len(got["pipe"]) == len(want["pipe"]) == want["K"]
        for q, r in zip(got["pipe"], want["pipe"]):
            assert q == r, (kw, q, r)
        base = _select(shim, kw["mode"], kw["draws"], kw["fast"], kw["lds_stack"])
        assert base == model.select(kw["mode"], kw["draws"], kw["fast"], kw["lds_stack"])
        seen.add(base)
        seen.update(q["variant"] for q in got["pipe"])
    # whatever a launch can take is built, and the sweep reaches every instance
    assert all(shim.wfp_built(_v(v)) == 1 for v in seen)
    assert seen == model.BUILT - ({(0, 0, 2, 10, 1), (0, 0, 3, 10, 1)} - {(0, 0, model.PERSIST_GEO, 10, 1)})


def test_sweep_properties(shim, swept):
    persisted = 0
    for kw, p in swept:
        assert p["ok"] and not p["empty"]
        W, rows = kw["W"], kw["rows"]
        tiles = ((W + 7) // 8) * ((rows + 7) // 8)
        assert 1 <= p["K"] <= min(shim.wfp_max_pipes(), tiles)
        assert sum(q["tiles"] for q in p["pipe"]) == tiles          # the shares partition the tiles ...
        assert max(q["tiles"] for q in p["pipe"]) - min(q["tiles"] for q in p["pipe"]) <= 1   # ... evenly
        assert sum(q["paths"] for q in p["pipe"]) >= W * rows
        for j, q in enumerate(p["pipe"]):
            assert q["total"] == 64 * q["tiles"] and q["tiles"] >= 1
            assert q["paths"] <= q["total"] and q["paths"] <= W * rows
            assert q["init_grid"] >= 1
            assert (q["tiles"], q["total"], q["paths"]) == _share(shim, W, rows, j, p["K"])
        assert p["trace_grid"] >= 1 and p["shade_grid"] >= 1
        assert (p["persist_grid"] != 0) == p["persist"]
        if p["persist"]:
            persisted += 1
            base = _select(shim, kw["mode"], kw["draws"], kw["fast"], kw["lds_stack"])
            assert kw["mode"] == RENDER and kw["samples"] == 1 and not kw["sort"] and base[2] == 2
    assert persisted > 50   # the sweep reaches the persistent trace often enough to mean something
    # past the last pipeline, and past the last tile, there is no share
    assert _share(shim, 9, 8, 2, 2) == (0, 0, 0) and _share(shim, 8, 8, 1, 4) == (0, 0, 0) and _share(shim, 8, 8, 0, 0) == (0, 0, 0)


# ---- the continuation predicate ----------------------------------------------------------------------------------

def _continues(shim, kw, mode, overlap, pending):
    return shim.wfp_continues(_words(shim, kw), mode, overlap, (ctypes.c_uint32 * 5)(*pending)) == 1


def test_continuation_needs_every_condition(shim):
    for over, persist in ((dict(), 0), (dict(rows=135), 1)):
        kw = dict(BASE, **over)
        p = _plan(shim, **over)
        assert p["K"] > 1 and p["persist"] == bool(persist)
        ok = (1, p["K"], kw["W"], kw["rows"], persist)
        assert _continues(shim, kw, RENDER, 1, ok)
        assert _continues(shim, kw, RENDER, 2, ok)
        assert not _continues(shim, kw, RENDER, 0, ok)                      # overlap off
        assert not _continues(shim, kw, COUNT, 1, ok)                       # not a render
        assert not _continues(shim, kw, DIAG, 1, ok)
        assert not _continues(shim, kw, RENDER, 1, (0,) + ok[1:])           # nothing pending
        assert not _continues(shim, kw, RENDER, 1, (1, p["K"] + 1) + ok[2:])
        assert not _continues(shim, kw, RENDER, 1, (1, p["K"] - 1) + ok[2:])
        assert not _continues(shim, kw, RENDER, 1, ok[:2] + (kw["W"] + 8,) + ok[3:])
        assert not _continues(shim, kw, RENDER, 1, ok[:3] + (kw["rows"] + 8, persist))
        assert not _continues(shim, kw, RENDER, 1, ok[:4] + (1 - persist,))
        one = dict(kw, pipes=1)                                             # K == 1: nothing runs beside the stream
        assert not _continues(shim, one, RENDER, 1, (1, 1, kw["W"], kw["rows"], persist))
    # and it agrees with the model over pending states of the sweep's plans
    for kw in list(model.sweep())[::37]:
        want = model.plan(**kw)
        for pending in ((1, want["K"], kw["W"], kw["rows"], int(want["persist"])), (1, 2, kw["W"], kw["rows"], 0),
                        (1, 3, kw["W"], kw["rows"], 1), (0, want["K"], kw["W"], kw["rows"], int(want["persist"]))):
            assert _continues(shim, kw, kw["mode"], kw["overlap"], pending) == \
                model.continues(want, kw["mode"], kw["overlap"], *pending)


# ---- the launch record (wcpt_wf_last_plan) and the model the GPU tests hold it against ------------------------------

def _record(shim, launches=1, continued=0, **over):
    """A record as launch_wavefront would fill it for the plan of these inputs: made up, no device involved."""
    kw = dict(BASE, **over)
    p = _plan(shim, **over)
    base = _select(shim, kw["mode"], kw["draws"], kw["fast"], kw["lds_stack"])
    rec = dict(launches=launches, mode=kw["mode"], ok=int(p["ok"]), empty=int(p["empty"]), persist=int(p["persist"]),
               K=p["K"], trace_grid=p["trace_grid"], shade_grid=p["shade_grid"], persist_grid=p["persist_grid"],
               continued=continued, sort=1 if (kw["sort"] and kw["draws"] > 0) else 0,
               base_code=wf_record.code_of(shim, base), width=kw["W"], rows=kw["rows"], samples=kw["samples"],
               max_bounce=kw["max_bounce"], wf_fetch=kw["wf_fetch"], wf_persist=kw["wf_persist"], pipes=kw["pipes"],
               overlap=kw["overlap"], cus=kw["cus"], trace_bpc=kw["trace_bpc"], persist_bpc=kw["persist_bpc"])
    rec["pipe"] = [dict(variant_code=wf_record.code_of(shim, q["variant"]), dispatches=1 if p["persist"] else q["iters"],
                        tiles=q["tiles"], paths=q["paths"], iters=q["iters"]) for q in p["pipe"]]
    return rec


RECORDS = (dict(), dict(W=3840, rows=2160), dict(rows=135), dict(rows=135, overlap=0), dict(W=52, rows=44, pipes=4, samples=2),
           dict(W=52, rows=44, wf_persist=1, pipes=2), dict(W=52, rows=44, mode=DIAG, draws=2, pipes=3),
           dict(W=52, rows=44, mode=COUNT, pipes=3), dict(W=52, rows=44, lds_stack=24, pipes=3),
           dict(W=52, rows=44, draws=0, pipes=4), dict(W=9, rows=8, pipes=4), dict(sort=1, pipes=3))


def test_record_layout_matches_the_mirror(shim):
    """wcpt_wf_plan_info as g++ lays it out is the ctypes mirror's: size and the offsets of a field of every group."""
    import ctypes as C
    from wcpt._lib import WfPipeInfo, WfPlanInfo
    out = (C.c_uint32 * 9)()
    shim.wfp_record_layout(out)
    assert list(out) == [C.sizeof(WfPlanInfo), WfPlanInfo.launches.offset, WfPlanInfo.mode.offset, WfPlanInfo.K.offset,
                         WfPlanInfo.continued.offset, WfPlanInfo.pipe.offset, WfPlanInfo.pipe.offset + C.sizeof(WfPipeInfo),
                         WfPlanInfo.base_code.offset, WfPlanInfo.persist_bpc.offset]
    assert C.sizeof(WfPlanInfo) == 176 and C.sizeof(WfPipeInfo) == 20 and shim.wfp_max_pipes() == 4


def test_record_round_trip(shim):
    """dict -> C record -> dict keeps every field (what the helpers rely on)."""
    rec = _record(shim, launches=7, continued=1, W=52, rows=44, pipes=3)
    assert wf_record.to_struct(rec).as_dict() == rec


@pytest.mark.parametrize("over", RECORDS, ids=[str(i) for i in range(len(RECORDS))])
def test_record_model_accepts_a_true_record(shim, over):
    rec = _record(shim, **over)
    assert wf_record.mismatches(shim, rec) == []
    codes = wf_record.check(shim, rec, launches=1)
    assert codes == [q["variant"] for q in _plan(shim, **over)["pipe"]]


@pytest.mark.parametrize("over", RECORDS, ids=[str(i) for i in range(len(RECORDS))])
def test_record_model_names_every_wrong_field(shim, over):
    """One field at a time made wrong -- a plan field, a pipeline's field, an input the plan depends on: the model says
    which (for an input: the plan fields that no longer follow from it)."""
    good = _record(shim, **over)
    for f in wf_record.PLAN_FIELDS:
        bad = dict(good, **{f: good[f] + 1})
        assert f in wf_record.mismatches(shim, bad), f
    for j in range(good["K"]):
        for f in wf_record.PIPE_FIELDS:
            bad = dict(good, pipe=[dict(q) for q in good["pipe"]])
            bad["pipe"][j][f] += 1
            assert wf_record.mismatches(shim, bad) == [f"pipe[{j}].{f}"], (j, f)
    # another built instance in one pipeline: the slip between plan and launch this record exists to show
    for other in sorted(wf_record.built_codes(shim) - {good["pipe"][0]["variant_code"]}):
        bad = dict(good, pipe=[dict(q) for q in good["pipe"]])
        bad["pipe"][0]["variant_code"] = other
        assert wf_record.mismatches(shim, bad) == ["pipe[0].variant_code"]
        with pytest.raises(AssertionError):
            wf_record.check(shim, bad)
    # a pipeline too few or too many
    assert "pipe" in wf_record.mismatches(shim, dict(good, pipe=good["pipe"][:-1]))
    # inputs: the grids follow cus and the occupancy, the iterations the bounces, the shares the frame
    assert "shade_grid" in wf_record.mismatches(shim, dict(good, cus=good["cus"] + 1))
    assert "trace_grid" in wf_record.mismatches(shim, dict(good, trace_bpc=good["trace_bpc"] * 2 + 1))
    assert any(m.endswith(".iters") for m in wf_record.mismatches(shim, dict(good, max_bounce=good["max_bounce"] + 1)))
    assert any(m.endswith(".paths") for m in wf_record.mismatches(shim, dict(good, width=good["width"] + 64)))
    if good["persist"]:
        assert "persist_grid" in wf_record.mismatches(shim, dict(good, persist_bpc=good["persist_bpc"] + 8))
        assert "persist" in wf_record.mismatches(shim, dict(good, samples=2))
        assert "persist" in wf_record.mismatches(shim, dict(good, sort=1))
        assert "persist" in wf_record.mismatches(shim, dict(good, wf_persist=0))
    # a base instance no launch selects
    assert wf_record.mismatches(shim, dict(good, base_code=wf_record.persist_code(shim))) == ["base_code"]
    assert wf_record.mismatches(shim, dict(good, base_code=shim.wfp_codes())) == ["base_code"]


def test_record_mode_and_sort_fix_the_pipelines(shim):
    rec = _record(shim, W=52, rows=44, pipes=3)
    assert rec["K"] == 3
    assert "K" in wf_record.mismatches(shim, dict(rec, mode=DIAG))
    assert "K" in wf_record.mismatches(shim, dict(rec, sort=1))
    assert "K" in wf_record.mismatches(shim, dict(rec, pipes=2))


def test_record_decoder_and_the_unreachable_instance(shim, every):
    for code, v in enumerate(every):
        assert wf_record.decode(shim, code) == v and wf_record.code_of(shim, v) == code
    built = wf_record.built_codes(shim)
    assert {wf_record.decode(shim, c) for c in built} == model.BUILT
    geo = shim.wfp_persist_geo()
    assert geo in (2, 3) and wf_record.decode(shim, wf_record.persist_code(shim)) == (0, 0, geo, 10, 1)
    # the persistent GEO is a compile-time choice: the other persistent instance is built and never launched
    assert {wf_record.decode(shim, c) for c in wf_record.unreachable_codes(shim)} == {(0, 0, 5 - geo, 10, 1)}
    assert len(built - wf_record.unreachable_codes(shim)) == 11


def test_record_continuation_model(shim):
    """wfp_record_continues: pending exactly after a render of several pipelines under the overlap, and then
    wf_frame_continues' conditions."""
    a = _record(shim, W=52, rows=44, pipes=3, overlap=2)
    assert not wf_record.continues(shim, a, None)                          # nothing pending
    assert wf_record.continues(shim, a, a)
    assert not wf_record.continues(shim, a, dict(a, overlap=0))            # the frame before joined at its end
    assert not wf_record.continues(shim, dict(a, overlap=0), a)
    assert not wf_record.continues(shim, a, _record(shim, W=52, rows=44, pipes=2, overlap=2))   # K changed
    assert not wf_record.continues(shim, a, _record(shim, W=60, rows=44, pipes=3, overlap=2))   # resized
    assert not wf_record.continues(shim, a, _record(shim, W=52, rows=44, pipes=3, overlap=2, mode=COUNT))
    assert not wf_record.continues(shim, _record(shim, W=52, rows=44, pipes=3, overlap=2, mode=COUNT), a)
    one = _record(shim, W=52, rows=44, pipes=1, overlap=2)
    assert not wf_record.continues(shim, one, one)
    p = _record(shim, W=52, rows=44, pipes=2, overlap=2, wf_persist=1)
    assert p["persist"] == 1 and wf_record.continues(shim, p, p)
    assert not wf_record.continues(shim, p, _record(shim, W=52, rows=44, pipes=2, overlap=2, wf_persist=0))
