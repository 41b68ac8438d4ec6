"""The composite device functions of the render kernels, one at a time, in both arithmetic modes (wcpt_selftest_geometry).

The whole-frame statistics of test_gpu_arith.py cannot tell a slightly wrong formula from a flipped path: both move a few
pixels. Here each function -- the three triangle tests, the sphere test, the sphere's hit epilogue, reflect / refract /
Fresnel, normalize and the reciprocals, one scatter step of path_shade -- runs alone on the input sets of tests/arith_ref.py:

  exact mode  bit for bit the binary32 restatement in the exact mode's operation order (arith_ref flavour (a)), and for the
              triangle and the sphere test also oracle/pt_f64.py's functions run in binary32. This proves the hook and the
              restatement, so that a failure in the fast mode is the kernel's.
  fast mode   every value within its derived bound of the binary64 value, every decision equal to the binary64 decision
              where that one is further from its threshold than the bound (arith_ref.check). The bounds come from the
              rounding of the formulas alone; tests/test_arith_ref_cpu.py checks them, and that six wrong formulas break
              them, without a GPU.

The traversal's child-pair decision and root cull (fn 8: child_pair, root_survives, the one definition the megakernel's
loop and its tiny walk use) have no fast form and no bound: bit for bit the oracle's expressions in numpy
binary32 (arith_ref.child_pair_model, itself checked against the oracle's C on the CPU), the same in both modes.
"""
import numpy as np
import pytest

import wcpt
import arith_ref as R

pytestmark = pytest.mark.gpu

T = wcpt._lib
FAST, EXACT = T.ARITH_FAST, T.ARITH_EXACT
SETS = R.all_sets()
KEYS = sorted(SETS)


def _run(ctx, fn, arith, x):
    return ctx.selftest_geometry(fn, arith, np.ascontiguousarray(x, np.float32).view(np.uint32))


def _same_bits(got, want, what):
    """Equal bit patterns, a NaN matching any NaN (numpy and the GPU may give different payloads)."""
    assert got.shape == want.shape
    both_nan = np.isnan(got.view(np.float32)) & np.isnan(want.view(np.float32))
    differ = (got != want) & ~both_nan
    assert not differ.any(), f"{what}: {int(differ.any(axis=1).sum())} of {len(got)} items differ, first " \
                             f"{int(np.flatnonzero(differ.any(axis=1))[0])}"


def test_arguments(gpu_ctx):
    x = np.zeros((4, 15), np.uint32)
    for fn, arith, iw, ow in ((0, 2, 15, 1), (0, -1, 15, 1), (8, EXACT, 15, 1), (9, EXACT, 19, 6), (-1, FAST, 15, 1), (0, EXACT, 14, 1),
                              (0, FAST, 15, 2), (6, FAST, 15, 6)):
        out = np.zeros((4, ow), np.uint32)
        rc = wcpt.lib.wcpt_selftest_geometry(gpu_ctx.h, fn, arith, wcpt.renderer.ptr(x), iw, wcpt.renderer.ptr(out), ow, 4)
        assert rc == T.WCPT_ERROR_INVALID_ARGUMENT, (fn, arith, iw, ow)
    assert _run(gpu_ctx, 0, EXACT, np.zeros((0, 15), np.float32)).shape == (0, 1)
    for fn, (iw, ow) in R.WORDS.items():
        assert gpu_ctx.GEOMETRY_WORDS[fn] == (iw, ow)
        n = 257                                                    # a second, partial block; the last item ends the array
        out = _run(gpu_ctx, fn, FAST, np.ones((n, iw), np.float32))
        assert out.shape == (n, ow) and (out == out[0]).all()


@pytest.mark.parametrize("fn,name", KEYS)
def test_exact_mode_is_the_unfused_restatement(gpu_ctx, fn, name):
    x = SETS[fn, name]
    got = _run(gpu_ctx, fn, EXACT, x)
    _same_bits(got, R.model(fn, R.F32(), x), "exact kernel against flavour (a)")
    if fn in (0, 3):
        _same_bits(got, R.reference_f32(fn, x).view(np.uint32).reshape(-1, 1), "exact kernel against pt_f64 in binary32")
    rep = R.check(fn, x, got)
    print(f"fn {fn} {name} exact: {rep}")
    assert not rep.bad.any(), str(rep)


@pytest.mark.parametrize("fn,name", KEYS)
def test_fast_mode_within_the_bounds(gpu_ctx, fn, name):
    """fn 2 and fn 1 see the same rays and triangles and both stay within the bounds of the same binary64 values; they are
    not bit-equal in the fast mode, because the records' origin terms (oa, q, tq) are built unfused (primary_terms) while
    rayTrianglePair fuses them."""
    x = SETS[fn, name]
    rep = R.check(fn, x, _run(gpu_ctx, fn, FAST, x))
    print(f"fn {fn} {name} fast: {rep}")
    assert not rep.bad.any(), str(rep)
    assert rep.share_undecided <= R.MAX_UNDECIDED, str(rep)


def test_scatter_step_draws_the_same_stream(gpu_ctx):
    """The fast mode draws what the exact mode draws: after one path_shade step the rng state is the exact mode's wherever
    both took the same branch -- everywhere but the few items whose k < 0 or rand <= reflectProb decision lies inside its
    bound (arith_ref.check marks those undecided) -- and the transmittance, plain binary32 code in both modes, has the same
    bits there."""
    x = SETS[7, "scatter"]
    fast, exact = _run(gpu_ctx, 7, FAST, x), _run(gpu_ctx, 7, EXACT, x)
    decided = ~R.check(7, x, fast).undecided
    assert decided.mean() >= 1 - R.MAX_UNDECIDED
    assert np.array_equal(fast[decided, 9], exact[decided, 9])
    assert np.array_equal(fast[decided, 6:9], exact[decided, 6:9])
    assert (fast[:, 3:6] != exact[:, 3:6]).any(), "the fast step is bit-identical to the exact one"


@pytest.mark.parametrize("arith", [EXACT, FAST])
@pytest.mark.parametrize("name", sorted(R.never_accepted_sets()))
def test_zero_determinant_is_a_miss(gpu_ctx, name, arith):
    """det is exactly 0 (a ray parallel to the plane, or a triangle with two equal vertices): t, u and v are infinite or
    NaN in either mode, and the triangle must not be accepted."""
    x = R.never_accepted_sets()[name]
    assert (_run(gpu_ctx, 0, arith, x).view(np.float32) == -1.0).all()
    for fn in (1, 2):
        out = _run(gpu_ctx, fn, arith, R.pair_items(x, x))
        assert not out[:, 2:].any(), f"fn {fn}"
        t = out[:, :2].view(np.float32)
        assert not np.isfinite(t).any(), "t = tn * rcp(0) is infinite or NaN"
    if arith == EXACT:
        _same_bits(_run(gpu_ctx, 0, EXACT, x), R.model(0, R.F32(), x), "exact kernel against flavour (a)")


def test_sliver_triangles_exact(gpu_ctx):
    """c = b: det is zero only up to rounding, so no bound says anything; the exact mode still has the restatement's bits."""
    x = R.sliver_set()
    _same_bits(_run(gpu_ctx, 0, EXACT, x), R.model(0, R.F32(), x), "exact kernel against flavour (a)")
    pair = R.pair_items(x)
    _same_bits(_run(gpu_ctx, 1, EXACT, pair), R.model(1, R.F32(), pair), "exact pair kernel against flavour (a)")
    assert _run(gpu_ctx, 0, FAST, x).shape == (len(x), 1)


@pytest.mark.parametrize("arith", [EXACT, FAST])
@pytest.mark.parametrize("name", ["inside", "edges", "vertices", "grazing", "negative_t"])
def test_pair_halves_agree(gpu_ctx, name, arith):
    """The two halves of a packed pair are the same formula: one triangle in both halves gives the same bits twice, two
    triangles swapped between the halves give swapped results, and a half gives rayTriangleE's bits (fn 0: t when accepted
    and t > 0, else -1) -- in the fast mode too, where all three use the same fused helpers."""
    x = SETS[0, name]
    single = _run(gpu_ctx, 0, arith, x)[:, 0]
    same = _run(gpu_ctx, 1, arith, R.pair_items(x, x))
    assert np.array_equal(same[:, 0], same[:, 1]) and np.array_equal(same[:, 2], same[:, 3])
    taken = (same[:, 2] != 0) & (same[:, 0].view(np.float32) > 0)
    want = np.where(taken, same[:, 0], np.float32(-1.0).view(np.uint32))
    assert np.array_equal(single, want), f"{int((single != want).sum())} items differ between fn 0 and a pair half"
    if name in ("edges", "vertices"):
        assert 0 < taken.sum() < len(x)                          # hits and misses both go through the comparison
    ab = R.pair_items(x)
    ba = np.concatenate([ab[:, :6], ab[:, 15:24], ab[:, 6:15]], axis=1)
    out_ab, out_ba = _run(gpu_ctx, 1, arith, ab), _run(gpu_ctx, 1, arith, ba)
    _same_bits(out_ab[:, [0, 1, 2, 3]], out_ba[:, [1, 0, 3, 2]], "swapped halves")
    assert np.array_equal(out_ab[:, 0], same[:, 0]) and np.array_equal(out_ab[:, 2], same[:, 2])


def test_child_pair_decision_bit_for_bit(gpu_ctx):
    """Every word of every item: which child is popped first, each box's pass, each entry distance t0 (as bits; two NaNs
    compare equal) and the root cull against rec.t -- on random boxes, invDirection components of +-inf with the origin on
    and off the slab planes, equal boxes, boxes behind the ray, rec.t equal to a t0, rec.t = kInfinity and NaN box words
    (arith_ref.child_pair_set)."""
    x = R.child_pair_set()
    want = R.child_pair_model(x)
    exact, fast = _run(gpu_ctx, 8, EXACT, x), _run(gpu_ctx, 8, FAST, x)
    _same_bits(exact, want, "child_pair / root_survives against the oracle's expressions")
    _same_bits(fast, exact, "the fast mode's words against the exact mode's")
