"""The bounds of tests/arith_ref.py checked on the CPU, before any kernel is held to them.

  1. The binary64 values are the ones oracle/pt_f64.py's independent functions give.
  2. Three binary32 restatements of every formula stay inside the bounds on every input set the GPU tests use: (a) unfused,
     the exact mode's order; (b) fused as pt_device.h writes it; (c) as (b) with every rcp / sqrt result one ULP up, and one
     ULP down.
  3. At most 2 % of any set is undecided (nearer to a decision threshold than its bound).
  4. The bounds are tight enough to be worth having: six deliberately wrong formulas each violate them on some set.
  5. The traversal's child-pair decision (fn 8, no bound: bit for bit) as numpy states it is the oracle's C on every item.
"""
import functools

import numpy as np
import pytest

import arith_ref as R


@functools.lru_cache(maxsize=None)
def _sets():
    return R.all_sets()


KEYS = sorted(R.all_sets())
FLAVOURS = {"unfused": R.F32(), **R.fast_flavours()}


@pytest.mark.parametrize("fn,name", KEYS)
def test_flavours_stay_inside_the_bounds(fn, name):
    x = _sets()[fn, name]
    assert len(x) >= 512 and x.shape[1] == R.WORDS[fn][0]
    for label, ar in FLAVOURS.items():
        rep = R.check(fn, x, R.model(fn, ar, x))
        print(f"fn {fn} {name} ({label}): {rep}")
        assert not rep.bad.any(), f"{label}: {rep}"
        assert rep.share_undecided <= R.MAX_UNDECIDED, f"{label}: {rep}"


@pytest.mark.parametrize("name", sorted(R.never_accepted_sets()))
def test_zero_determinant_is_a_miss_in_every_flavour(name):
    x = R.never_accepted_sets()[name]
    for label, ar in FLAVOURS.items():
        assert (R.model(0, ar, x).view(np.float32) == -1.0).all(), label
        pair = R.model(1, ar, R.pair_items(x, x))
        assert not pair[:, 2:].any(), label


def test_binary64_values_are_pt_f64s():
    """The reference values inside check() against oracle/pt_f64.py on the same binary32 inputs: a binary32 evaluation that
    is pt_f64's own (run in binary32) must pass check(), and the binary64 results must agree to binary64 rounding."""
    sets = _sets()
    for (fn, name), x in sets.items():
        if fn in (0, 3):
            out = R.reference_f32(fn, x).view(np.uint32).reshape(-1, 1)
            assert np.array_equal(out, R.model(fn, R.F32(), x)), (fn, name)     # flavour (a) is pt_f64 in binary32, bit for bit
        if fn == 3:
            t, disc = R.sphere_terms(R.E64, R._cols(R.E64, x, 0), R._cols(R.E64, x, 3), R._cols(R.E64, x, 6), R.E64.inp(x[:, 9]))
            ref = R.reference_values(3, x)
            hit = disc.v >= 0
            assert np.array_equal(ref[~hit], np.full((~hit).sum(), -1.0))
            assert np.allclose(ref[hit], t.v[hit], rtol=1e-13, atol=0)
        if fn == 5:
            ar = R.E64
            i, n, ia, ib = R._cols(ar, x, 0), R._cols(ar, x, 3), ar.inp(x[:, 6]), ar.inp(x[:, 7])
            refl, refr, prob = R.reference_values(5, x)
            mine = np.stack([c.v for c in R.reflect_terms(ar, i, n)], axis=1)
            assert np.allclose(refl, mine, rtol=1e-12, atol=1e-15)
            t, k = R.refract_terms(ar, i, n, V_div(ia, ib))
            ok = k.v > 1e-9                                   # away from k = 0, where sqrt(k) amplifies the last bit
            assert np.allclose(refr[ok], np.stack([c.v for c in t], axis=1)[ok], rtol=1e-9, atol=1e-12)
            f, sin2, d_perp, d_par = R.reflectance_terms(ar, i, n, ia, ib)
            ok = (sin2.v < 1 - 1e-9) & (np.fmin(d_perp.v, d_par.v) > 1e-7)
            assert np.allclose(prob[ok], f.v[ok], rtol=1e-6, atol=1e-12)
            assert (prob[sin2.v >= 1] == 1.0).all()


def V_div(a, b):
    """the binary64 quotient as a value without error (eta as pt_f64 forms it)"""
    return R.V(a.v / b.v, np.zeros_like(a.v))


MUTANTS = {
    "cross_term": (0, 1, 2),          # swapped operands in one term of cross(d, e2)
    "dot_oa_p": (0, 1, 2),            # dot(oa, p) with e1 in place of oa
    "rpar_iors": (5, 7),                # rPar's numerator with iorA and iorB exchanged
    "refract_sign": (5, 7),             # refract's c with the wrong sign
    "reflect_factor": (5, 7),           # reflect with the factor -1 instead of -2
    "far_root": (3,),                 # the sphere's far root
}


@pytest.mark.parametrize("mutant", sorted(MUTANTS))
def test_mutants_are_caught(mutant):
    """A wrong formula, evaluated as the fast mode would (flavour (b)), violates a bound or a decision on at least one set
    of each function it sits in."""
    for fn in MUTANTS[mutant]:
        caught = {}
        for (f, name), x in _sets().items():
            if f == fn:
                rep = R.check(fn, x, R.model(fn, R.F32(True, True), x, mut=mutant))
                caught[name] = int(rep.bad.sum())
        print(f"{mutant} in fn {fn}: violations per set {caught}")
        assert max(caught.values()) > 0, f"{mutant} passes every set of fn {fn}"


def test_child_pair_model_is_the_oracles():
    """arith_ref.child_pair_model against oracle/pt_oracle.c's own box test and Intersect's own decisions
    (oracle_child_pair) on the items the GPU test uses: every word equal, a NaN distance matching a NaN. The set holds what
    it claims to: NaN distances, both pop orders, passing and failing boxes, roots that survive and roots that do not."""
    import oracle
    x = R.child_pair_set()
    assert 300 <= len(x) <= 1000 and x.shape[1] == R.WORDS[8][0]
    got, want = R.child_pair_model(x), oracle.child_pair(x)
    assert got.shape == want.shape == (len(x), R.WORDS[8][1])
    both_nan = np.isnan(got.view(np.float32)) & np.isnan(want.view(np.float32))
    differ = ((got != want) & ~both_nan).any(axis=1)
    assert not differ.any(), f"{int(differ.sum())} of {len(x)} items differ, first {int(np.flatnonzero(differ)[0])}"
    t0 = got[:, 3:5].view(np.float32)
    nan_l, nan_r = np.isnan(t0[:, 0]), np.isnan(t0[:, 1])
    assert (nan_l & nan_r).any() and (nan_l & ~nan_r).any() and (~nan_l & nan_r).any()
    for k in (0, 1, 2, 5):
        assert 0 < got[:, k].sum() < len(x), f"word {k} is the same for every item"
    assert (t0 == x[:, 18:19]).any() and np.isinf(x[:, 3:6]).any() and np.isnan(x[:, 6:18]).any()
