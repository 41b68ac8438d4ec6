"""Every wf_trace instance of the wavefront renderer on the GPU, each asserted as taken (csrc/wf_plan.h lists the
instances and makes the plan; tests/test_wf_plan.py checks both on the CPU). All instances render the same bits by design,
so an image cannot say which one ran: every cell here also reads the launch record (wcpt_wf_last_plan) after the render
and asserts that

- the record is of this render (`launches`), and holds exactly the plan wf_frame_plan makes of the inputs it reports --
  among them the three values only the device knows: the compute-unit count and the two occupancies (wf_record.check,
  through the product header compiled by tests/wf_plan_shim.cpp);
- every pipeline's instance, noted where the dispatcher was called, is the one the cell is here for.

52x44 leaves partial 8x8 tiles at both edges (42 tiles); 3 bounces; frames 0, 1, 2 of a still camera, accumulated. No
tolerance anywhere: the image after each frame equals the oracle's accumulation bit for bit, NaN patterns included, and
counters equal the oracle's exactly. The last test states the coverage: the instances the module reached are the built
ones minus the one no launch can select.

Source mutation this module was checked against (a scratch build, unable to write out of bounds): pipe_iterate handing
pipeline 1 the launch's base instance instead of wf_pipe_variant's -- GEO 2 where the plan says GEO 3, the same bits in
every image -- fails test_render_instance[geo3], test_persistent_instance, test_continuation[per-bounce-3] and the
coverage test, and the one-round cases of test_gpu_parity.py's fetch-round test.

The cells are run once each and kept (_once), so the coverage test can name them all without depending on test order."""
import ctypes as C

import numpy as np
import pytest

import oracle
import wcpt
import wf_record
from wf_record import COUNT, DIAG, RENDER

from test_gpu_primary_cache import H, W, _Run, _bits, _scene
from test_wf_plan import shim  # noqa: F401  (fixture: wf_plan.h through its CPU shim)

pytestmark = pytest.mark.gpu

T = wcpt._lib
BOUNCES = 3
FRAMES = (0, 1, 2)
TILES = ((W + 7) // 8) * ((H + 7) // 8)
OVERLAP_FORCED = 2            # what tests/test_gpu_overlap.py sets

_want = {}
_done = {}
_seen = {}                    # instance code -> the cells that launched it


def _once(key, fn):
    if key not in _done:
        _done[key] = fn()
    return _done[key]


def _oracle_frames(name, samples):
    """The oracle's accumulated image after each of FRAMES, once per (scene, samples); read-only."""
    key = (name, samples)
    if key not in _want:
        s = _scene(name)
        acc, out = None, []
        for f in FRAMES:
            acc, _ = oracle.render_scene(s, W, H, sd=s.scene_data(W, H, max_bounce=BOUNCES, samples=samples, frame=f),
                                         image=acc, threads=8)
            keep = acc.copy()
            keep.setflags(write=False)
            out.append(keep)
        _want[key] = out
    return _want[key]


def _oracle_counters(name, frame=1):
    key = (name, "counters", frame)
    if key not in _want:
        s = _scene(name)
        _want[key] = oracle.render_scene(s, W, H, sd=s.scene_data(W, H, max_bounce=BOUNCES, samples=1, frame=frame),
                                         threads=8)[1]
    return _want[key]


def _note(shim, rec, cell):
    for q in rec["pipe"]:
        _seen.setdefault(q["variant_code"], []).append(cell)


def _assert_image(r, name, samples, i, cell):
    img = r.image()
    want = _oracle_frames(name, samples)[i]
    assert img.shape == want.shape, cell
    assert np.array_equal(_bits(img), _bits(want)), f"{cell}: frame {FRAMES[i]} differs from the oracle's accumulation"


def _wf_run(name, **options):
    """A context on the wavefront kernel, forced, with the scene resident and the options set."""
    r = _Run(_scene(name), cache=False)
    r.ctx.set_kernel(wcpt.KERNEL_WAVEFRONT)
    for opt, v in options.items():
        r.ctx.set_option(getattr(T, "OPTION_" + opt), v)
    return r


def _frames(shim, r, name, samples, cell, launches, each):
    """Frames 0, 1, 2: after every render the record (before the readback joins anything) passes wf_record.check and
    `each(rec, variants)`, and the image equals the oracle's. Returns the launch count."""
    for i, f in enumerate(FRAMES):
        r.render(f, BOUNCES, samples)
        rec = r.ctx.wf_last_plan()
        launches += 1
        variants = wf_record.check(shim, rec, launches=launches)
        assert r.ctx.last_kernel() == wcpt.KERNEL_WAVEFRONT
        assert (rec["mode"], rec["width"], rec["rows"], rec["samples"], rec["max_bounce"]) == (RENDER, W, H, samples, BOUNCES), cell
        _note(shim, rec, cell)
        each(rec, variants)
        _assert_image(r, name, samples, i, f"{cell} frame {f}")
    return launches


# ---- the six render instances: pipelines 1..4 x samples 1, 2 ---------------------------------------------------------
# (scene, options, the instance every pipeline must launch)
RENDER_CELLS = {
    "geo0-two_draws": ("two_draws", {}, (0, 0, 0, 10, 0)),
    "geo0-no_draws": ("empty", {}, (0, 0, 0, 10, 0)),
    "geo1-lds10": ("cornell", {"PACKED_REFS": 0}, (0, 0, 1, 10, 0)),
    "geo1-lds16": ("cornell", {"WF_STACK": 16}, (0, 0, 1, 16, 0)),
    "geo1-lds24": ("cornell", {"WF_STACK": 24}, (0, 0, 1, 24, 0)),
    "geo2": ("cornell", {"WF_PERSIST": 0, "WF_FETCH": 0}, (0, 0, 2, 10, 0)),
    "geo3": ("cornell", {"WF_PERSIST": 0, "WF_FETCH": 1}, (0, 0, 3, 10, 0)),
}


def _render_cell(shim, key):
    name, options, instance = RENDER_CELLS[key]
    r = _wf_run(name, **options)
    try:
        launches = 0
        for samples in (1, 2):
            iters = shim.wfp_iterations(RENDER, samples, BOUNCES)
            for pipes in (1, 2, 3, 4):
                cell = f"{key} pipes {pipes} samples {samples}"
                r.ctx.set_option(T.OPTION_WF_PIPES, pipes)

                def each(rec, variants):
                    assert variants == [instance] * pipes, (cell, variants)
                    assert rec["K"] == min(pipes, TILES) == pipes and rec["pipes"] == pipes, cell
                    assert rec["persist"] == 0 and rec["persist_grid"] == 0 and rec["sort"] == 0, cell
                    assert wf_record.decode(shim, rec["base_code"])[3] == instance[3], cell
                    assert sum(q["tiles"] for q in rec["pipe"]) == TILES, cell
                    assert all(q["iters"] == q["dispatches"] == iters for q in rec["pipe"]), (cell, rec["pipe"])

                launches = _frames(shim, r, name, samples, cell, launches, each)
        assert launches == 2 * 4 * len(FRAMES)
    finally:
        r.close()
    return True


@pytest.mark.parametrize("key", list(RENDER_CELLS))
def test_render_instance(shim, key):
    """One per-bounce render instance with WF_PIPES 1, 2, 3, 4 and samples 1, 2 (the second sample reuses sample 0's
    primary record in wf_shade, and 3 + 1 + 3 iterations replace 2 x 4): every pipeline launches that instance, K is
    min(option, tiles), every pipeline makes wf_iterations' launches, and never the persistent trace."""
    assert _once(("render", key), lambda: _render_cell(shim, key))


# ---- the persistent instance -----------------------------------------------------------------------------------------
def _persist_cells(shim):
    code = wf_record.persist_code(shim)
    out = {"ran": 0}
    for wf_persist in (1, -1):
        r = _wf_run("cornell", WF_PERSIST=wf_persist)
        try:
            launches = 0
            for pipes in (0, 1, 2):
                cell = f"persist {wf_persist} pipes {pipes}"
                r.ctx.set_option(T.OPTION_WF_PIPES, pipes)

                def each(rec, variants):
                    # wf_record.check has held `persist`, K and the grids against the model for the reported cus and
                    # persist_bpc: that is the whole expectation where the option is -1
                    assert rec["wf_persist"] == wf_persist and rec["persist_bpc"] >= 1 and rec["cus"] >= 1, cell
                    if wf_persist == 1:
                        assert rec["persist"] == 1, cell
                    if pipes:
                        assert rec["K"] == pipes, cell
                    if rec["persist"]:
                        out["ran"] += 1
                        assert rec["persist_grid"] == max(1, rec["persist_bpc"] * rec["cus"] // rec["K"]), cell
                        assert [q["variant_code"] for q in rec["pipe"]] == [code] * rec["K"], cell
                        assert all(q["dispatches"] == 1 for q in rec["pipe"]), cell
                    else:
                        assert rec["persist_grid"] == 0 and all(v[4] == 0 and v[2] in (2, 3) for v in variants), cell

                launches = _frames(shim, r, "cornell", 1, cell, launches, each)
        finally:
            r.close()
    # ineligible whatever the option says: a sorted render, and more than one sample
    for extra, samples in (({"SORT_RAYS": 1}, 1), ({}, 2)):
        r = _wf_run("cornell", WF_PERSIST=1, WF_PIPES=2, **extra)
        try:
            cell = f"persist 1 {extra} samples {samples}"

            def each(rec, variants):
                assert rec["persist"] == 0 and rec["persist_grid"] == 0 and rec["wf_persist"] == 1, cell
                assert rec["sort"] == (1 if extra else 0) and rec["K"] == (1 if extra else 2), cell
                assert all(v[4] == 0 for v in variants), cell

            _frames(shim, r, "cornell", samples, cell, 0, each)
        finally:
            r.close()
    assert out["ran"] >= 3 * len(FRAMES)       # WF_PERSIST 1: every frame of every pipeline count
    return True


def test_persistent_instance(shim):
    """The path-persistent trace on Cornell, one sample: forced (WF_PERSIST 1) it runs with WF_PIPES 0, 1 and 2; left
    to the rule (-1) it runs exactly where the plan of the reported compute units and occupancy says. Its grid is
    max(1, persist_bpc * cus / K), its instance wf_persist_variant(), one launch per pipeline. Sorted, or with two
    samples, the render is per-bounce although the option says 1."""
    assert _once("persist", lambda: _persist_cells(shim))


# ---- the counting and diagnostics instances ----------------------------------------------------------------------------
def _counters(ctx, sd, addrs, diagnostics):
    """wcpt_render_counters with every field of wcpt_counters, the SIMD ones included whether asked for or not."""
    sd = np.ascontiguousarray(sd, dtype=T.SCENE_DATA_DTYPE)
    c = T.Counters()
    ctx.set_option(T.OPTION_DIAGNOSTICS, 1 if diagnostics else 0)
    try:
        T.check(T.lib.wcpt_render_counters(ctx.h, T.ptr(sd), *addrs, C.byref(c)), ctx.h)
    finally:
        ctx.set_option(T.OPTION_DIAGNOSTICS, 0)
    return c.as_dict(True)


def _count_cells(shim, name, diagnostics):
    want = _oracle_counters(name)
    geo = 1 if name == "cornell" else 0
    instance = (1, 1 if diagnostics else 0, geo, 10, 0)
    r = _wf_run(name)
    try:
        sd = r.sd(1, BOUNCES, 1)
        launches = 0
        for pipes in (1, 3):
            cell = f"{name} diagnostics {diagnostics} pipes {pipes}"
            r.ctx.set_option(T.OPTION_WF_PIPES, pipes)
            got = _counters(r.ctx, sd, r.dev.addresses(), diagnostics)
            rec = r.ctx.wf_last_plan()
            launches += 1
            variants = wf_record.check(shim, rec, launches=launches)
            _note(shim, rec, cell)
            K = 1 if diagnostics else pipes        # one diagnostics block
            assert rec["mode"] == (DIAG if diagnostics else COUNT) and rec["K"] == K and rec["pipes"] == pipes, cell
            assert variants == [instance] * K, (cell, variants)
            assert rec["persist"] == 0 and rec["continued"] == 0, cell
            iters = shim.wfp_iterations(COUNT, 1, BOUNCES)
            assert all(q["iters"] == q["dispatches"] == iters for q in rec["pipe"]), cell
            # the reference's work, exactly -- with three pipelines three streams add into one block
            assert {k: got[k] for k in T.COUNTER_FIELDS} == want, cell
            if diagnostics:
                # wf_trace calls simd_step beside interior_visits++, beside triangle_tests++ and where a lane takes a
                # queued ray (one per Intersect call): the lane steps are those counters
                assert got["lane_interior_steps"] == want["interior_visits"] > 0, cell
                assert got["lane_triangle_steps"] == want["triangle_tests"] > 0, cell
                assert got["lane_segment_steps"] == want["segments"] > 0, cell
                for phase in ("interior", "triangle", "segment"):
                    wave, lane = got[f"wave_{phase}_steps"], got[f"lane_{phase}_steps"]
                    assert 0 < wave <= lane <= 64 * wave, (cell, phase, wave, lane)
            else:
                assert all(got[k] == 0 for k in T.DIAG_FIELDS), (cell, got)
    finally:
        r.close()
    return True


@pytest.mark.parametrize("diagnostics", [False, True], ids=["count", "diag"])
@pytest.mark.parametrize("name", ["cornell", "two_draws"])
def test_counting_instance(shim, name, diagnostics):
    """wcpt_render_counters with WF_PIPES 1 and 3: the counting instance (GEO 1 on Cornell, GEO 0 on two draws) counts
    the oracle's work exactly on one and on three pipelines; the diagnostics instance runs one pipeline whatever the
    option says, and its lane steps are the work counters they stand beside."""
    assert _once(("count", name, diagnostics), lambda: _count_cells(shim, name, diagnostics))


# ---- continuation under the frame overlap ----------------------------------------------------------------------------
def _continuation(shim, persist):
    pipes = 2 if persist else 3
    other = 3 if persist else 2
    r = _wf_run("cornell", WF_PERSIST=1 if persist else 0, WF_PIPES=pipes, FRAME_OVERLAP=OVERLAP_FORCED)
    state = {"prev": None, "launches": 0}
    what = "persistent" if persist else "per-bounce"

    def render(f, K, continued, cell):
        r.render(f, BOUNCES, 1)
        rec = r.ctx.wf_last_plan()                  # joins nothing: the pipelines run on
        state["launches"] += 1
        wf_record.check(shim, rec, launches=state["launches"])
        _note(shim, rec, cell)
        assert rec["K"] == K and rec["persist"] == (1 if persist else 0), (cell, rec)
        assert rec["continued"] == (1 if continued else 0), (cell, rec)
        assert wf_record.continues(shim, rec, state["prev"]) == continued, (cell, rec, state["prev"])   # the CPU model agrees
        state["prev"] = rec
        return rec

    def sequence(K, cell):
        """frames 0, 1, 2 with nothing in between: the first behind a join (or a changed plan) stands alone, the
        others continue; then the image"""
        render(0, K, False, f"{cell} frame 0")
        render(1, K, True, f"{cell} frame 1")
        render(2, K, True, f"{cell} frame 2")
        _assert_image(r, "cornell", 1, 2, cell)     # sync + readback: joins
        state["prev"] = None

    try:
        # The first render of a context prepares the scene's records on the stream, and the runtime runs such a frame
        # without the overlap (wcpt_render.hip: prep_missed): it joins at its end, so nothing is pending behind it.
        rec = render(0, pipes, False, f"{what}: the preparing render")
        assert rec["overlap"] == 0
        rec = render(0, pipes, False, f"{what} frame 0")
        assert rec["overlap"] == OVERLAP_FORCED
        render(1, pipes, True, f"{what} frame 1")
        render(2, pipes, True, f"{what} frame 2")
        _assert_image(r, "cornell", 1, 2, f"{what} frames 0, 1, 2")
        state["prev"] = None
        # another pipeline count between two frames: other tiles per pipeline, so the frames before are joined first
        render(0, pipes, False, f"{what}: before WF_PIPES {other}")
        render(1, pipes, True, f"{what}: before WF_PIPES {other}")
        r.ctx.set_option(T.OPTION_WF_PIPES, other)
        sequence(other, f"{what}: after WF_PIPES {other}")
        r.ctx.set_option(T.OPTION_WF_PIPES, pipes)
        # a resize between two frames
        render(0, pipes, False, f"{what}: before the resize")
        render(1, pipes, True, f"{what}: before the resize")
        r.ctx.resize(W, H)
        state["prev"] = None
        sequence(pipes, f"{what}: after wcpt_resize")
        # a counting render between two frames
        render(0, pipes, False, f"{what}: before the counters")
        render(1, pipes, True, f"{what}: before the counters")
        got = _counters(r.ctx, r.sd(1, BOUNCES, 1), r.dev.addresses(), False)
        assert {k: got[k] for k in T.COUNTER_FIELDS} == _oracle_counters("cornell")
        rec = r.ctx.wf_last_plan()
        state["launches"] += 1
        assert rec["launches"] == state["launches"] and rec["mode"] == COUNT and rec["continued"] == 0
        state["prev"] = None
        sequence(pipes, f"{what}: after wcpt_render_counters")
    finally:
        r.close()
    return True


@pytest.mark.parametrize("persist", [False, True], ids=["per-bounce-3", "persistent-2"])
def test_continuation(shim, persist):
    """WCPT_OPTION_FRAME_OVERLAP forced: frame 0 stands alone, frames 1 and 2 continue behind the frame before on their
    pipelines' own streams; after another WF_PIPES, a wcpt_resize or a wcpt_render_counters the next render does not.
    What the record says is what wf_frame_continues says of the record before (wf_record.continues), and the images
    are the oracle's throughout."""
    assert _once(("continuation", persist), lambda: _continuation(shim, persist))


# ---- the coverage statement --------------------------------------------------------------------------------------------
def test_every_reachable_instance_was_launched(shim):
    """The instances this module launched, by the records: the built set minus what no launch can select.
    wf_persist_variant() fixes the persistent trace's GEO at compile time (WCPT_WF_PERSIST_GEO), so the persistent instance
    of the other GEO is compiled and unreachable at run time; the expectation comes from the shim, so another value
    of the macro moves it."""
    for key in RENDER_CELLS:
        _once(("render", key), lambda: _render_cell(shim, key))
    _once("persist", lambda: _persist_cells(shim))
    for name in ("cornell", "two_draws"):
        for diagnostics in (False, True):
            _once(("count", name, diagnostics), lambda: _count_cells(shim, name, diagnostics))
    for persist in (False, True):
        _once(("continuation", persist), lambda: _continuation(shim, persist))
    built = wf_record.built_codes(shim)
    unreachable = wf_record.unreachable_codes(shim)
    geo = shim.wfp_persist_geo()
    assert len(built) == 12
    assert {wf_record.decode(shim, c) for c in unreachable} == {(0, 0, 5 - geo, 10, 1)}
    seen = set(_seen)
    assert seen == built - unreachable, ({wf_record.decode(shim, c) for c in seen ^ (built - unreachable)})
    assert len(seen) == 11 and not (seen & unreachable)
