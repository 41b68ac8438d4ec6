"""The traversal stack's last entry and its refusal (WCPT_ERROR_STACK_OVERFLOW), in every stack the kernels have.

The chain of tests/deep_tree.py defers one far leaf per level, so a ray that reaches its bottom holds `levels` entries
(the reference pushes both children: the oracle's ref_stack_max is levels + 1). The stacks hold 48: levels = 48 fills
the last entry, levels = 49 is the first tree that does not fit.

This is a check of a designed return code, not a provoked fault. Read in the code before the overflowing case was
ever run: PrivateStack<48>::push returns false at sp >= 48 before it stores; LdsStack<N, SPILL>::push (the megakernel's
<16, 32>, the wavefront's <LDSN, 48 - LDSN>) stores to LDS at sp < N, to the spill at sp < N + SPILL, and otherwise
returns false having stored nothing and left sp alone (pt_stacks.h). The callers (pt_traversal.h interior_step,
pt_wavefront.hip wf_trace's interior step) only set a flag on a refused push and go on; every pop is behind empty().
The refused subtree is simply not visited, the kernels atomicOr the context's status word at their end, and the next
wcpt_sync / wcpt_readback / wcpt_render_counters reports WCPT_ERROR_STACK_OVERFLOW once and clears the word
(wcpt_runtime.hip read_status).

Which instance a one-draw hand-made chain selects (wf_plan.h wf_variant_select, wf_frame_plan, wf_pipe_geo and
wf_pipe_variant, which tests/test_wf_plan.py evaluates on the CPU; pt_wavefront.hip wf_dispatch launches it): uploaded through wcpt_buffer_upload it gets the fast layout (packed refs, 24-bit offsets, 3-index leaves on records, a
known node count), so at WCPT_OPTION_WF_STACK 10 a 48x32 one-sample frame takes the path-persistent trace
wf_trace<false, false, 3, 10, true> (1536 paths fit the resident lanes), with WCPT_OPTION_WF_PERSIST 0 the one-round
trace <.., 3, 10> (WCPT_OPTION_WF_FETCH 1 or auto at this size) or the two-round <.., 2, 10> (WF_FETCH 0); with
WCPT_OPTION_PACKED_REFS 0 the layout is not fast and it takes <.., 1, 10>; WF_STACK 16 / 24 take <.., 1, 16> / <.., 1, 24>;
the same mesh drawn twice takes <.., 0, 10>. Counting runs take <true, false, 1, 10> (two draws: <true, false, 0, 10>)
whatever the options say. The megakernel takes PrivateStack<48> with WCPT_OPTION_STACK 0 and LdsStack<16, 32> with 1, in
its render and its counting instances alike. The wavefront cases do not take this paragraph's word for it: every
render and counting run asserts, from the launch record (wcpt_wf_last_plan), the instance each pipeline launched."""
import copy

import numpy as np
import pytest

import wcpt
import oracle

import wf_record
from deep_tree import deep_chain_scene
from test_gpu_parity import assert_close, get_scene
from test_wf_plan import shim  # noqa: F401  (fixture: wf_plan.h through its CPU shim)

pytestmark = pytest.mark.gpu

T = wcpt._lib
MK, WF = wcpt.KERNEL_MEGAKERNEL, wcpt.KERNEL_WAVEFRONT
W, H, BOUNCES = 48, 32, 2

# name -> (kernel, {option: value}, draws of the chain)
CONFIGS = {
    "mk_scratch": (MK, {T.OPTION_STACK: 0}, 1),
    "mk_lds": (MK, {T.OPTION_STACK: 1}, 1),
    "wf10_persist": (WF, {T.OPTION_WF_STACK: 10, T.OPTION_WF_PERSIST: 1}, 1),
    "wf10_one_round": (WF, {T.OPTION_WF_STACK: 10, T.OPTION_WF_PERSIST: 0, T.OPTION_WF_FETCH: 1}, 1),
    "wf10_two_rounds": (WF, {T.OPTION_WF_STACK: 10, T.OPTION_WF_PERSIST: 0, T.OPTION_WF_FETCH: 0}, 1),
    "wf10_plain": (WF, {T.OPTION_WF_STACK: 10, T.OPTION_PACKED_REFS: 0}, 1),
    "wf16": (WF, {T.OPTION_WF_STACK: 16}, 1),
    "wf24": (WF, {T.OPTION_WF_STACK: 24}, 1),
    "wf_two_draws": (WF, {}, 2),
}

# the wf_trace instance (count, diag, geo, ldsn, persist) each wavefront configuration's renders must launch;
# "persist": wf_persist_variant()
WF_RENDERS = {
    "wf10_persist": "persist",
    "wf10_one_round": (0, 0, 3, 10, 0),
    "wf10_two_rounds": (0, 0, 2, 10, 0),
    "wf10_plain": (0, 0, 1, 10, 0),
    "wf16": (0, 0, 1, 16, 0),
    "wf24": (0, 0, 1, 24, 0),
    "wf_two_draws": (0, 0, 0, 10, 0),
}
assert set(WF_RENDERS) == {n for n, c in CONFIGS.items() if c[0] == WF}

_cache = {}


def chain(levels, draws=1):
    key = ("scene", levels, draws)
    if key not in _cache:
        s = deep_chain_scene(get_scene("default"), levels=levels)
        s.meshes = s.meshes * draws
        _cache[key] = s
    return _cache[key]


def ref(levels, draws=1):
    key = ("ref", levels, draws)
    if key not in _cache:
        img, cnt = oracle.render_scene(chain(levels, draws), W, H, max_bounce=BOUNCES, threads=8)
        img.setflags(write=False)
        _cache[key] = (img, cnt)
    return _cache[key]


def untouched(levels):
    """Pixels whose path never meets the chain: bit-equal in the oracle's frames with the mesh and without it."""
    key = ("mask", levels)
    if key not in _cache:
        bare = copy.copy(chain(levels))
        bare.meshes = []
        without, _ = oracle.render_scene(bare, W, H, max_bounce=BOUNCES, threads=8)
        _cache[key] = (without.view(np.uint32) == ref(levels)[0].view(np.uint32)).all(axis=2)
    return _cache[key]


class Chains:
    """A context of its own set up as CONFIGS[name] says, with the chains it has uploaded."""

    def __init__(self, name, shim):
        self.name, self.shim = name, shim
        self.kernel, self.options, self.draws = CONFIGS[name]
        self.ctx = wcpt.Context(0)
        self.devs = {}
        self.launches = 0

    def __enter__(self):
        self.ctx.set_kernel(self.kernel)
        for o, v in self.options.items():
            self.ctx.set_option(o, v)
        self.ctx.create_screen(W, H)
        return self

    def __exit__(self, *exc):
        self.ctx.close()

    def args(self, levels):
        s = chain(levels, self.draws)
        if levels not in self.devs:
            self.devs[levels] = wcpt.DeviceScene(self.ctx, s)
        return (s.scene_data(W, H, max_bounce=BOUNCES),) + self.devs[levels].addresses()

    def launched(self, want):
        """the record of the wavefront launch just made: this launch's, the plan of its inputs, and every pipeline on
        the instance `want`"""
        if self.kernel != WF:
            return
        rec = self.ctx.wf_last_plan()
        got = wf_record.check(self.shim, rec, launches=self.launches)
        assert got == [want] * rec["K"], (self.name, got, want)
        assert rec["persist"] == want[4] and (rec["width"], rec["rows"]) == (W, H)

    def render(self, levels):
        args = self.args(levels)
        self.launches += 1
        self.ctx.render(*args)                   # raises if the render call itself reports anything
        want = WF_RENDERS.get(self.name)
        self.launched(wf_record.decode(self.shim, wf_record.persist_code(self.shim)) if want == "persist" else want)

    def counters(self, levels):
        args = self.args(levels)
        self.launches += 1
        try:
            return self.ctx.render_counters(*args)
        finally:                                 # also when the call reports the overflow: the launch was made
            self.launched((1, 0, 1 if self.draws == 1 else 0, 10, 0))


def overflows(call):
    with pytest.raises(wcpt.WcptError) as e:
        call()
    assert e.value.code == T.WCPT_ERROR_STACK_OVERFLOW


@pytest.mark.parametrize("name", list(CONFIGS))
def test_last_entry_fits(shim, name):
    """levels = 48: the 48th entry is stored and popped; no status, image and counters exact."""
    with Chains(name, shim) as c:
        c.render(48)
        c.ctx.sync()
        img = c.ctx.readback()
        cnt = c.counters(48)
    rimg, rcnt = ref(48, c.draws)
    assert_close(img, rimg, exact=True)
    assert cnt == rcnt
    assert rcnt["ref_stack_max"] == 49 and rcnt["ref_stack_overflow_segments"] > 0
    assert 0 < untouched(48).sum() < W * H     # the chain is in view, and so is the sky around it


@pytest.mark.parametrize("name", list(CONFIGS))
def test_first_entry_that_does_not_fit_is_refused(shim, name):
    """levels = 49: the render returns success, the next sync reports the overflow once, pixels away from the chain are the
    oracle's, a 40-level frame afterwards is exact; the same through readback and through render_counters, which
    returns the error too (its counters are those of the cut-short traversal)."""
    with Chains(name, shim) as c:
        ctx = c.ctx
        c.render(49)
        overflows(ctx.sync)
        ctx.sync()                               # reported once: the word was cleared
        img = ctx.readback()
        c.render(40)
        ctx.sync()
        after = ctx.readback()
        after_cnt = c.counters(40)
        c.render(49)
        overflows(ctx.readback)                  # readback as the reporting call
        ctx.sync()
        overflows(lambda: c.counters(49))        # the counting instance refuses and reports in the same call
        ctx.sync()
        c.render(40)
        ctx.sync()
        again = ctx.readback()
    keep = untouched(49)
    assert 0 < keep.sum() < keep.size
    assert np.array_equal(img.view(np.uint32)[keep], ref(49, c.draws)[0].view(np.uint32)[keep])
    assert np.isfinite(img).all()
    rimg, rcnt = ref(40, c.draws)
    assert_close(after, rimg, exact=True)
    assert after_cnt == rcnt and rcnt["ref_stack_max"] == 41
    assert_close(again, rimg, exact=True)


def test_oracle_depths():
    """The chain's depth as the oracle counts it: levels + 1 reference entries, one more per level."""
    assert [ref(n)[1]["ref_stack_max"] for n in (40, 48, 49)] == [41, 49, 50]
