"""Every render instance of the megakernel on the GPU (csrc/mk_variant.h lists them; tests/test_mk_variant.py checks
the selection on the CPU): stack kind x pair records x one or two draw commands x one or two samples x exact or fast
arithmetic x whole or split, and in each cell frames 0, 1, 2 of a still camera with the primary cache on and no upload
in between, which take the cache's none, write and read forms. That is all 96 render, all 24 head and all 8 tail
instances. 52x44 leaves partial 8x8 tiles at both edges.

No tolerance anywhere: an exact cell equals the oracle's accumulation of the three frames bit for bit; a fast cell
equals, bit for bit, the fast render of the same scene, samples and records on the LDS stack, unsplit and uncached
("Defined arithmetic": fast against fast does not depend on stack, split or cache). Every cell asserts from
wcpt_primary_cache_stats and wcpt_mk_split_stats that it took the forms it is here for."""
import itertools

import numpy as np
import pytest

import wcpt

from test_gpu_primary_cache import H, W, _Run, _bits, _oracle_acc, _scene

pytestmark = pytest.mark.gpu

T = wcpt._lib
BOUNCES = 3
FRAMES = (0, 1, 2)
CUT = 2                       # WCPT_OPTION_MK_SPLIT: forced, before segment 2 of 0..3


def _cell(s, samples, stack, pairs, arith, split, cache=True):
    """The accumulated image after the three frames, and what the context says it ran."""
    r = _Run(s, cache)
    try:
        r.ctx.set_kernel(wcpt.KERNEL_MEGAKERNEL)      # singles would otherwise go to the wavefront kernels
        r.ctx.set_option(T.OPTION_STACK, stack)
        r.ctx.set_option(T.OPTION_PAIR_RECORDS, pairs)
        r.ctx.set_option(T.OPTION_ARITH, arith)
        r.ctx.set_option(T.OPTION_MK_SPLIT, split)
        for f in FRAMES:
            r.render(f, BOUNCES, samples)
        img = r.image()
        assert r.ctx.last_kernel() == wcpt.KERNEL_MEGAKERNEL
        assert r.ctx.last_arith() == arith
        return img, r.stats(), r.ctx.mk_split_stats()
    finally:
        r.close()


@pytest.mark.parametrize("samples", [1, 2])
@pytest.mark.parametrize("name", ["cornell", "two_draws"])
def test_every_render_instance(name, samples):
    s = _scene(name)
    want_exact = _oracle_acc(s, W, H, [(f, BOUNCES, samples) for f in FRAMES])
    want_fast = {}
    for pairs in (0, 1):
        img, stats, splits = _cell(s, samples, 1, pairs, T.ARITH_FAST, 0, cache=False)
        assert stats == (0, 0) and splits == 0
        want_fast[pairs] = img
    for stack, pairs, arith, split in itertools.product((0, 1), (0, 1), (T.ARITH_EXACT, T.ARITH_FAST), (0, CUT)):
        cell = f"stack {stack} pairs {pairs} arith {arith} split {split}"
        img, stats, splits = _cell(s, samples, stack, pairs, arith, split)
        assert stats == (1, 1), cell                 # frame 1 wrote the records, frame 2 read them
        can_split = split != 0 and stack == 1 and samples == 1
        assert splits == (len(FRAMES) if can_split else 0), cell
        want = want_exact if arith == T.ARITH_EXACT else want_fast[pairs]
        assert img.shape == want.shape, cell
        assert np.array_equal(_bits(img), _bits(want)), cell
