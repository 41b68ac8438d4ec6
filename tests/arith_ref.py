"""binary64 references, derived error bounds, binary32 models and input sets for the composite device functions that
wcpt_selftest_geometry exposes (wcpt.h: fn 0..7; fn 8, the traversal's child-pair decision, has no fast form and no bound:
child_pair_model and child_pair_set at the end). numpy only; shared by tests/test_arith_ref_cpu.py (which checks the
bounds themselves, without a GPU) and tests/test_gpu_arith_functions.py (which checks the kernels against them).

One text per formula, several arithmetics. Each formula below is written once, in the operation order of pt_device.h,
on an arithmetic object `ar`; evaluating it with
  E64                           gives the binary64 value of every quantity together with a running error bound,
  F32()                         flavour (a): the exact mode's binary32 operations, unfused, correctly rounded 1/x and sqrt,
  F32(fuse=True, fast=True)     flavour (b): the fast mode as pt_device.h writes it: fma(a, b, c) where kFuse<A> fuses
                                (modelled as float32(float64(a) * float64(b) + float64(c))), a * rcp(b) for a / b,
  F32(True, True, nudge=+-1)    flavour (c): as (b) with every rcp / sqrt result moved one ULP up or down.
Sharing the text does not make the check circular: the binary64 values are compared with oracle/pt_f64.py's independent
functions (test_arith_ref_cpu.py), flavour (a) is compared bit for bit with the exact kernels, and the bound is a
property of the arithmetic object, not of the formula.

The bound (E64). Every quantity carries (v, e): its binary64 value from the binary32 inputs, and a bound e on the
absolute error of any binary32 evaluation of the same unfused formula. With u = 2^-24 (binary32 unit roundoff):
  inputs                 e = 0
  a + b, a - b           e = ea + eb + u |v|                    (one rounding)
  a * b                  e = |a| eb + |b| ea + ea eb + u |v|    (one rounding)
  rcp(a)                 e = ea / (|a| (|a| - ea)) + 2u |v|     (2^-23: the 1 ULP of a bare v_rcp_f32; inf if ea >= |a|)
  sqrt(a)                e = min(ea / (2 sqrt a), sqrt ea) + 2u |v|   (2^-23: v_sqrt_f32; |sqrt(a + d) - sqrt a| <= sqrt |d|)
  a / b                  a * rcp(b)                             (3u |v|: covers the correctly rounded quotient's u |v|)
A fused multiply-add rounds once where the unfused form rounds twice, so it stays inside the same bound. Expanded over a
dot or cross product this is the classic bound from the absolute sums of the terms: e.g. for t = tn * rcp(det) of the
triangle test, with T_abs and D_abs the sums of |term| of tn and det (each term itself a product of rounded factors),
  |dt| <= k u (T_abs + |t| D_abs) / |det| + 4u |t|,
k the roundings on the longest chain (o - a, two products and a subtraction in the cross product, three products and two
additions in the dot product). Every comparison uses SAFETY * e (the factor covers the u^2 terms left out and, in
flavour (c), the half ULP by which a nudged correctly rounded result exceeds 2^-23), plus the smallest normal binary32
number, below which a result may be flushed. No number here was read off a kernel's output.

Decisions (accept / miss, t > 0, discriminant < 0, front, k < 0, sinSqr >= 1, min(dPerp, dPar) < 1e-8, rand <=
reflectProb, the side of the next origin) must equal the
binary64 decision wherever the binary64 quantity is further from its threshold than SAFETY * e; nearer items are
undecided and skipped for that decision and for the values that depend on it. At most MAX_UNDECIDED of a set may be
undecided (asserted on the CPU for every set).
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "oracle"))
import pt_f64  # noqa: E402  (the independent binary64 restatement: cross-checks the values below)

U = 2.0 ** -24
SAFETY = 2.0
TINY = 2.0 ** -126
MAX_UNDECIDED = 0.02
WORDS = {0: (15, 1), 1: (24, 4), 2: (24, 4), 3: (10, 1), 4: (11, 7), 5: (8, 7), 6: (3, 6), 7: (33, 10),
         8: (19, 6)}
K_BIAS = np.float32(1e-5)
_ERR = dict(divide="ignore", invalid="ignore", over="ignore", under="ignore")


# ---- arithmetics ------------------------------------------------------------------------------------------------------
class _Arith:
    """The helpers of pt_device.h (mad_a, msub_a, nmad_a, madn_a, dot_a, cross_a, axpy_a, div_a, div3_a) on the
    primitives add, sub, mul, neg, rcp, sqrt, truediv and fma that each arithmetic defines."""
    fuse = False
    fast = False

    def mad(self, a, b, c):
        return self.fma(a, b, c) if self.fuse else self.add(self.mul(a, b), c)

    def msub(self, a, b, c, d):                      # a * b - c * d; fused: fma(a, b, -(c * d))
        return self.fma(a, b, self.neg(self.mul(c, d))) if self.fuse else self.sub(self.mul(a, b), self.mul(c, d))

    def nmad(self, c, a, b):                         # c - a * b; fused: fma(-a, b, c)
        return self.fma(self.neg(a), b, c) if self.fuse else self.sub(c, self.mul(a, b))

    def madn(self, a, b, c):                         # a * b - c; fused: fma(a, b, -c)
        return self.fma(a, b, self.neg(c)) if self.fuse else self.sub(self.mul(a, b), c)

    def dot(self, a, b):                             # (x x' + y y') + z z'; fused: fma(z, z', fma(y, y', x x'))
        if self.fuse:
            return self.fma(a[2], b[2], self.fma(a[1], b[1], self.mul(a[0], b[0])))
        return self.add(self.add(self.mul(a[0], b[0]), self.mul(a[1], b[1])), self.mul(a[2], b[2]))

    def cross(self, a, b):
        return (self.msub(a[1], b[2], b[1], a[2]), self.msub(a[2], b[0], b[2], a[0]), self.msub(a[0], b[1], b[0], a[1]))

    def axpy(self, a, b, s):                         # a + b * s; fused: fma(b, s, a)
        if self.fuse:
            return tuple(self.fma(b[i], s, a[i]) for i in range(3))
        return tuple(self.add(a[i], self.mul(b[i], s)) for i in range(3))

    def div(self, a, b):                             # div_a: the IEEE quotient, or a * rcp(b)
        return self.mul(a, self.rcp(b)) if self.fast else self.truediv(a, b)

    def sub3(self, a, b):
        return tuple(self.sub(a[i], b[i]) for i in range(3))

    def scale3(self, a, s):
        return tuple(self.mul(a[i], s) for i in range(3))

    def neg3(self, a):
        return tuple(self.neg(a[i]) for i in range(3))

    def div3(self, a, s):                            # GLSL v / s as the kernels evaluate it in both modes: v * rcp(s)
        return self.scale3(a, self.rcp(s))


class F32(_Arith):
    """binary32 evaluation. fuse: the formulas' fused forms; fast: a * rcp(b) for a / b; nudge: rcp and sqrt results moved
    by that many ULPs (0: correctly rounded, the exact mode's)."""

    def __init__(self, fuse=False, fast=False, nudge=0):
        self.fuse, self.fast, self.nudge = fuse, fast, nudge

    def unfused(self):
        return F32(False, self.fast, self.nudge)

    @staticmethod
    def const(x):
        return np.float32(x)

    @staticmethod
    def inp(x):
        return np.asarray(x, np.float32)

    def add(self, a, b):
        with np.errstate(**_ERR):
            return np.float32(a) + np.float32(b)

    def sub(self, a, b):
        with np.errstate(**_ERR):
            return np.float32(a) - np.float32(b)

    def mul(self, a, b):
        with np.errstate(**_ERR):
            return np.float32(a) * np.float32(b)

    @staticmethod
    def neg(a):
        return -np.float32(a)

    def fma(self, a, b, c):
        with np.errstate(**_ERR):
            return (np.float64(a) * np.float64(b) + np.float64(c)).astype(np.float32)

    def _nudged(self, r):
        if self.nudge:
            moved = np.nextafter(r, np.float32(np.inf if self.nudge > 0 else -np.inf)).astype(np.float32)
            r = np.where(np.isfinite(r), moved, r)      # rcp(+-0) = +-inf has no neighbour one ULP away
        return r

    def rcp(self, a):
        with np.errstate(**_ERR):
            return self._nudged(np.float32(1.0) / np.asarray(a, np.float32))

    def sqrt(self, a):
        with np.errstate(**_ERR):
            return self._nudged(np.sqrt(np.asarray(a, np.float32)))

    def truediv(self, a, b):
        with np.errstate(**_ERR):
            return np.float32(a) / np.float32(b)


class V:
    """A binary64 value with its running error bound."""
    __slots__ = ("v", "e")

    def __init__(self, v, e):
        self.v, self.e = v, e


class _E64(_Arith):
    fuse, fast = False, True        # unfused (most roundings); a / b as a * rcp(b) (the wider of the two)

    def unfused(self):
        return self

    @staticmethod
    def const(x):
        return V(np.float64(np.float32(x)), 0.0)

    @staticmethod
    def inp(x):
        x = np.asarray(x, np.float32).astype(np.float64)
        return V(x, np.zeros_like(x))

    def add(self, a, b):
        v = a.v + b.v
        return V(v, a.e + b.e + U * np.abs(v))

    def sub(self, a, b):
        v = a.v - b.v
        return V(v, a.e + b.e + U * np.abs(v))

    def mul(self, a, b):
        with np.errstate(**_ERR):
            v = a.v * b.v
            return V(v, np.abs(a.v) * b.e + np.abs(b.v) * a.e + a.e * b.e + U * np.abs(v))

    @staticmethod
    def neg(a):
        return V(-a.v, a.e)

    def rcp(self, a):
        with np.errstate(**_ERR):
            v = 1.0 / a.v
            av = np.abs(a.v)
            e = np.where(a.e < av, a.e / (av * (av - a.e)), np.inf)
            return V(v, e + 2.0 * U * np.abs(v))

    def sqrt(self, a):
        with np.errstate(**_ERR):
            v = np.sqrt(np.maximum(a.v, 0.0))
            e = np.fmin(a.e / (2.0 * v), np.sqrt(a.e))
            return V(v, e + 2.0 * U * v)


    # The fast mode's transcendentals (RandomDirection), bounded by the precision the Vulkan specification grants GLSL's
    # log and cos, which is what tests/test_gpu_arith.py holds v_log_f32 and v_cos_f32 to: log within 3 ULP outside
    # [0.5, 2] and 2^-21 absolute inside, plus the rounding of the multiplication by ln 2; cos within 2^-11 absolute.
    # The exact mode's software log and cos are far inside both.
    def ln(self, a):
        with np.errstate(**_ERR):
            v = np.log(a.v)
            return V(v, np.fmax(6.0 * U * np.abs(v), 2.0 ** -21) + U * np.abs(v))

    def cos2pi(self, a):
        return V(np.cos(2.0 * np.pi * a.v), np.full_like(a.v, 2.0 ** -11))


E64 = _E64()


def fast_flavours():
    """(b), (c+), (c-)"""
    return {"fused": F32(True, True), "nudged up": F32(True, True, +1), "nudged down": F32(True, True, -1)}


# ---- the formulas (pt_device.h) -----------------------------------------------------------------------------------------
def _cols(ar, x, k):
    return tuple(ar.inp(x[:, k + i]) for i in range(3))


def tri_terms(ar, o, d, a, e1, e2, mut=None, primary=False):
    """rayTriangleE and one half of rayTrianglePair: (t, u, v, w = 1 - (u + v), det). primary: the origin terms oa,
    q = cross(oa, e1), tq = dot(e2, q) come unfused from the record (primary_terms), as in rayTrianglePairP."""
    og = ar.unfused() if primary else ar
    oa = og.sub3(o, a)
    p = ar.cross(d, e2)
    if mut == "cross_term":                          # first component with b.y and b.z exchanged
        p = (ar.msub(d[1], e2[1], e2[2], d[2]), p[1], p[2])
    det = ar.dot(e1, p)
    inv = ar.rcp(det)
    q = og.cross(oa, e1)
    un = ar.dot(e1 if mut == "dot_oa_p" else oa, p)
    tn = og.dot(e2, q)
    u = ar.mul(un, inv)
    v = ar.dot(d, ar.scale3(q, inv))
    t = ar.mul(tn, inv)
    w = ar.sub(ar.const(1.0), ar.add(u, v))
    return t, u, v, w, det


def sphere_terms(ar, o, d, c, r, mut=None):
    """raySphereNear: (t, discriminant). The sphere test is never fused (kSphereA)."""
    s = ar.unfused()
    oc = s.sub3(o, c)
    b = s.dot(oc, d)
    cc = s.nmad(s.dot(oc, oc), r, r)
    disc = s.madn(b, b, cc)
    root = s.sqrt(disc)
    t = s.add(s.neg(b), root) if mut == "far_root" else s.sub(s.neg(b), root)
    return t, disc


def resolve_terms(ar, o, d, t, c, r):
    """resolve_hit on a sphere: (p, outward normal, dot(d, normal))."""
    p = ar.axpy(o, d, t)
    n = ar.div3(ar.sub3(p, c), r)
    return p, n, ar.dot(d, n)


def reflect_terms(ar, i, n, mut=None):
    f = 1.0 if mut == "reflect_factor" else 2.0
    if ar.fuse:
        return ar.axpy(i, n, ar.mul(ar.const(-f), ar.dot(n, i)))
    return ar.sub3(i, ar.scale3(n, ar.mul(ar.const(f), ar.dot(n, i))))


def refract_terms(ar, i, n, eta, mut=None):
    """(T when k >= 0, k)."""
    one = ar.const(1.0)
    dn = ar.dot(n, i)
    if ar.fuse:
        k = ar.nmad(one, ar.mul(eta, eta), ar.nmad(one, dn, dn))
        c = ar.mad(eta, dn, ar.sqrt(k))
        if mut != "refract_sign":
            c = ar.neg(c)
        return ar.axpy(ar.scale3(i, eta), n, c), k
    k = ar.sub(one, ar.mul(ar.mul(eta, eta), ar.sub(one, ar.mul(dn, dn))))
    c = ar.add(ar.mul(eta, dn), ar.sqrt(k))
    if mut == "refract_sign":
        c = ar.neg(c)
    return ar.sub3(ar.scale3(i, eta), ar.scale3(n, c)), k


def reflectance_terms(ar, i, n, ia, ib, mut=None):
    """CalculateReflectance: (value past both exits, sinSqr, dPerp, dPar)."""
    one = ar.const(1.0)
    ratio = ar.div(ia, ib)
    cos_in = ar.neg(ar.dot(i, n))
    sin2 = ar.mul(ar.mul(ratio, ratio), ar.nmad(one, cos_in, cos_in))
    cos_r = ar.sqrt(ar.sub(one, sin2))
    d_perp = ar.mad(ia, cos_in, ar.mul(ib, cos_r))
    d_par = ar.mad(ib, cos_in, ar.mul(ia, cos_r))
    r_perp = ar.div(ar.msub(ia, cos_in, ib, cos_r), d_perp)
    r_perp = ar.mul(r_perp, r_perp)
    if mut == "rpar_iors":
        r_par = ar.div(ar.msub(ia, cos_in, ib, cos_r), d_par)
    else:
        r_par = ar.div(ar.msub(ib, cos_in, ia, cos_r), d_par)
    r_par = ar.mul(r_par, r_par)
    return ar.mul(ar.add(r_perp, r_par), ar.const(0.5)), sin2, d_perp, d_par      # x / 2 == x * 0.5 exactly


def normalize_terms(ar, v):
    return ar.div3(v, ar.sqrt(ar.dot(v, v)))


def random_direction_terms(state):
    """RandomDirection in E64 from the rng state (uint32 array, advanced in place by its six draws): the binary64 direction
    with a bound that covers the fast mode's v_log_f32 / v_cos_f32 / bare sqrt and rcp (and so the exact mode's)."""
    ar, comp = E64, []
    for _ in range(3):
        u0 = ar.inp(pt_f64.rand(state).astype(np.float32))       # rand() is a binary32 value: exact here
        u1 = ar.inp(pt_f64.rand(state).astype(np.float32))
        rho = ar.sqrt(ar.mul(ar.const(-2.0), ar.ln(u1)))
        comp.append(ar.mul(rho, ar.cos2pi(u0)))
    return normalize_terms(ar, tuple(comp))


def shade_terms(ar, d, nrm, ior, front, rough, rd_a, rd_b, mut=None):
    """The arithmetic of one path_shade step past the material fetch: reflect, and for a dielectric Fresnel and refract
    with etaI / etaT chosen by `front`; then the three directions the step can end on -- normalize(base + roughness * rd)
    for base = R with the direction drawn straight away (rd_a: metal, or total reflection: no rand drawn before it), R
    after the Fresnel draw (rd_b) and T after it -- each with dot(direction, normal), whose sign places the next origin."""
    one = ar.const(1.0)
    eta_i = _where(ar, front, one, ior)
    eta_t = _where(ar, front, ior, one)
    r = reflect_terms(ar, d, nrm, mut)
    prob = reflectance_terms(ar, d, nrm, eta_i, eta_t, mut)
    t, k = refract_terms(ar, d, nrm, ar.div(eta_i, eta_t), mut)
    ends = {}
    for name, base, rd in (("RA", r, rd_a), ("RB", r, rd_b), ("TB", t, rd_b)):
        direction = normalize_terms(ar, ar.axpy(base, rd, rough))
        ends[name] = (direction, ar.dot(direction, nrm))
    return r, prob, k, ends


def _where(ar, cond, a, b):
    if isinstance(a, V) or isinstance(b, V):
        return V(np.where(cond, a.v, b.v), np.where(cond, a.e, b.e))
    return np.where(cond, a, b).astype(np.float32)


def _shade_inputs(ar, x):
    m = np.ascontiguousarray(x[:, 14:29])
    return dict(o=_cols(ar, x, 0), d=_cols(ar, x, 3), p=_cols(ar, x, 6), nrm=_cols(ar, x, 9), t=x[:, 12],
                front=np.ascontiguousarray(x[:, 13]).view(np.uint32) != 0,
                metal=np.ascontiguousarray(m[:, 0]).view(np.uint32) == 0, albedo=m[:, 1:4], rough=ar.inp(m[:, 9]),
                absorption=m[:, 10:13], strength=m[:, 13], ior=ar.inp(m[:, 14]),
                rng=np.ascontiguousarray(x[:, 29]).view(np.uint32).copy(), trans=x[:, 30:33])


def _shade_streams(rng):
    """The rng states and draws of a step: state after RandomDirection drawn straight away (A), the Fresnel draw u, and
    the state after u and RandomDirection (B)."""
    state_a = rng.copy()
    for _ in range(6):
        pt_f64.rand(state_a)
    state_b = rng.copy()
    u = pt_f64.rand(state_b).astype(np.float32)
    after_u = state_b.copy()
    for _ in range(6):
        pt_f64.rand(state_b)
    return state_a, u, after_u, state_b


def _oracle_directions(states):
    """The exact mode's RandomDirection (the C oracle's, bit-identical to the kernels') from each rng state."""
    import oracle
    return tuple(np.array(c, np.float32) for c in zip(*[oracle.random_direction(int(st))[0] for st in states]))


def _transmittances(i):
    """The two transmittances a step can leave, in the binary32 operations both modes share: times the albedo (metal), or
    times exp(-absorption * strength * t) (a refracted back hit); a dielectric otherwise leaves it unchanged."""
    import oracle
    e = ((i["absorption"] * np.float32(-1.0)) * i["strength"][:, None]) * i["t"][:, None]
    ex = np.array([[oracle.expf(float(v)) for v in row] for row in e], np.float32)
    return (i["trans"] * i["albedo"]).astype(np.float32), (i["trans"] * ex).astype(np.float32)


# ---- binary32 models in the hook's output layout ------------------------------------------------------------------------
def _u32(*cols):
    out = np.empty((len(cols[0]), len(cols)), np.uint32)
    for k, c in enumerate(cols):
        c = np.asarray(c)
        out[:, k] = c.astype(np.float32).view(np.uint32) if c.dtype != np.uint32 else c
    return out


def _flag(b):
    return np.asarray(b).astype(np.uint32)


def model(fn, ar, x, mut=None):
    """What wcpt_selftest_geometry(fn) returns for the items x[n, in_words] (float32) under the binary32 arithmetic ar."""
    x = np.asarray(x, np.float32)
    with np.errstate(**_ERR):
        if fn == 0:
            a, b, c = _cols(ar, x, 6), _cols(ar, x, 9), _cols(ar, x, 12)
            ex = F32()                                  # the edges are plain subtractions in both modes
            t, u, v, w, _ = tri_terms(ar, _cols(ar, x, 0), _cols(ar, x, 3), a, ex.sub3(b, a), ex.sub3(c, a), mut)
            ok = (t > 0) & (u >= 0) & (v >= 0) & (ar.add(u, v) <= 1)
            return _u32(np.where(ok, t, np.float32(-1.0)))
        if fn in (1, 2):
            o, d = _cols(ar, x, 0), _cols(ar, x, 3)
            res = [tri_terms(ar, o, d, _cols(ar, x, k), _cols(ar, x, k + 3), _cols(ar, x, k + 6), mut, primary=fn == 2)
                   for k in (6, 15)]
            hit = [_flag((u >= 0) & (v >= 0) & (w >= 0)) for _, u, v, w, _ in res]
            return _u32(res[0][0], res[1][0], hit[0], hit[1])
        if fn == 3:
            t, disc = sphere_terms(ar, _cols(ar, x, 0), _cols(ar, x, 3), _cols(ar, x, 6), ar.inp(x[:, 9]), mut)
            return _u32(np.where(disc < 0, np.float32(-1.0), t))
        if fn == 4:
            d = _cols(ar, x, 3)
            p, n, dn = resolve_terms(ar, _cols(ar, x, 0), d, ar.inp(x[:, 6]), _cols(ar, x, 7), ar.inp(x[:, 10]))
            front = dn < 0
            n = [np.where(front, c, c * np.float32(-1.0)) for c in n]
            return _u32(*p, *n, _flag(front))
        if fn == 5:
            i, n, ia, ib = _cols(ar, x, 0), _cols(ar, x, 3), ar.inp(x[:, 6]), ar.inp(x[:, 7])
            r = reflect_terms(ar, i, n, mut)
            t, k = refract_terms(ar, i, n, ar.div(ia, ib), mut)
            t = [np.where(k < 0, np.float32(0.0), c) for c in t]
            f, sin2, d_perp, d_par = reflectance_terms(ar, i, n, ia, ib, mut)
            f = np.where(np.fmin(d_perp, d_par) < np.float32(1e-8), np.float32(1.0), f)
            f = np.where(sin2 >= 1, np.float32(1.0), f)
            return _u32(*r, *t, f)
        if fn == 6:
            v = _cols(ar, x, 0)
            return _u32(*normalize_terms(ar, v), *[ar.rcp(c) for c in v])
        if fn == 7:
            # RandomDirection is the exact mode's in every flavour: the fast mode's v_log_f32 / v_cos_f32 have no binary32
            # model, and enter the bound as terms of their own (random_direction_terms)
            i = _shade_inputs(ar, x)
            state_a, u, after_u, state_b = _shade_streams(i["rng"])
            rd_a, rd_b = _oracle_directions(i["rng"]), _oracle_directions(after_u)
            r, prob, k, ends = shade_terms(ar, i["d"], i["nrm"], i["ior"], i["front"], i["rough"], rd_a, rd_b, mut)
            f, sin2, d_perp, d_par = prob
            f = np.where(np.fmin(d_perp, d_par) < np.float32(1e-8), np.float32(1.0), f)
            f = np.where(sin2 >= 1, np.float32(1.0), f)
            metal, total = i["metal"], ~i["metal"] & (k < 0)
            straight = metal | total                                  # no Fresnel draw
            follow = straight | (u <= f)
            pick = lambda a, rb, tb: np.where(straight, a, np.where(follow, rb, tb))      # noqa: E731
            direction = [pick(ends["RA"][0][c], ends["RB"][0][c], ends["TB"][0][c]) for c in range(3)]
            dn = pick(ends["RA"][1], ends["RB"][1], ends["TB"][1])
            sign = np.where(dn > 0, np.float32(1.0), np.where(dn < 0, np.float32(-1.0), np.float32(0.0)))
            o_metal = ar.axpy(i["p"], i["nrm"], K_BIAS)
            origin = [np.where(metal, o_metal[c], i["p"][c] + (K_BIAS * i["nrm"][c]) * sign) for c in range(3)]
            t_metal, t_absorb = _transmittances(i)
            trans = np.where(metal[:, None], t_metal, np.where((~follow & ~i["front"])[:, None], t_absorb, i["trans"]))
            return _u32(*origin, *direction, *trans.T, np.where(straight, state_a, state_b).astype(np.uint32))
    raise ValueError(fn)


# ---- the check: outputs against the binary64 values within the bounds --------------------------------------------------
class Report:
    """bad: items that violate a bound or a decision; undecided: items skipped for some decision; ratio: the largest
    |error| / (SAFETY * e + TINY) over the checked values (<= 1 passes)."""

    def __init__(self, n):
        self.bad = np.zeros(n, bool)
        self.undecided = np.zeros(n, bool)
        self.ratio = 0.0
        self.why = []

    def value(self, name, got, ref, where):
        """got within the bound of ref.v on the items `where`; a non-finite bound leaves the item undecided."""
        got = np.asarray(got, np.float32).astype(np.float64)
        tol = SAFETY * ref.e + TINY
        known = where & np.isfinite(tol) & np.isfinite(ref.v)
        self.undecided |= where & ~known
        with np.errstate(**_ERR):
            ratio = np.where(known, np.abs(got - ref.v) / tol, 0.0)
        ratio = np.where(known & ~np.isfinite(got), np.inf, ratio)
        self._mark(name, ratio > 1.0)
        self.ratio = max(self.ratio, float(ratio.max(initial=0.0)))

    def equal(self, name, got, want, where):
        self._mark(name, where & (np.asarray(got, np.float32) != np.float32(want)))

    def decision(self, name, got, q, thr, where=True, at_threshold=False):
        """got (bool) against q.v < thr (at_threshold: q.v <= thr). Returns (surely true, surely false)."""
        with np.errstate(**_ERR):
            margin = np.abs(q.v - thr)
            sure = np.isfinite(q.e) & np.isfinite(q.v) & (margin > SAFETY * q.e + TINY)
        ref = (q.v <= thr) if at_threshold else (q.v < thr)
        where = np.broadcast_to(where, sure.shape)
        self.undecided |= where & ~sure
        if got is not None:
            self._mark(name, where & sure & (np.asarray(got, bool) != ref))
        return sure & ref, sure & ~ref

    def _mark(self, name, mask):
        if mask.any():
            self.why.append(f"{name}: {int(mask.sum())} items, first {int(np.flatnonzero(mask)[0])}")
        self.bad |= mask

    @property
    def share_undecided(self):
        return float(self.undecided.mean()) if self.undecided.size else 0.0

    def __str__(self):
        return (f"{int(self.bad.sum())} violations of {self.bad.size}, {100 * self.share_undecided:.2f} % undecided, "
                f"largest error / bound {self.ratio:.3f}" + ("; " + "; ".join(self.why) if self.why else ""))


def _f(out, k):
    return np.ascontiguousarray(out[:, k]).view(np.float32)


def _tri_check(rep, tag, terms, got_hit, with_t):
    """The acceptance u >= 0, v >= 0, w >= 0 (and t > 0 when with_t) as one decision: surely accepted when every term
    is surely on the accepting side, surely missed when one is surely on the other. Returns (accepted, missed)."""
    t, u, v, w, _ = terms
    n = len(t.v)
    yes, no = np.ones(n, bool), np.zeros(n, bool)
    for q in (u, v, w):
        neg, pos = rep.decision(tag, None, q, 0.0, where=False)      # q < 0 rejects; -0 and +0 accept
        yes &= pos
        no |= neg
    if with_t:
        neg, pos = rep.decision(tag, None, t, 0.0, where=False, at_threshold=True)   # t <= 0 rejects
        yes &= pos
        no |= neg
    rep.undecided |= ~(yes | no)
    if got_hit is not None:
        rep._mark(tag + " accept", (yes & ~got_hit) | (no & got_hit))
    return yes, no


def check(fn, x, out):
    """The outputs out[n, out_words] (uint32) of fn on the items x against the binary64 reference."""
    x = np.asarray(x, np.float32)
    out = np.asarray(out, np.uint32)
    assert out.shape == (len(x), WORDS[fn][1]) and x.shape[1] == WORDS[fn][0]
    ar, rep, n = E64, Report(len(x)), len(x)
    every = np.ones(n, bool)
    with np.errstate(**_ERR):
        if fn == 0:
            a, b, c = x[:, 6:9], x[:, 9:12], x[:, 12:15]
            e1, e2 = (b - a).astype(np.float32), (c - a).astype(np.float32)   # the function's inputs: rounded edges
            terms = tri_terms(ar, _cols(ar, x, 0), _cols(ar, x, 3), _cols(ar, a, 0), _cols(ar, e1, 0), _cols(ar, e2, 0))
            got = _f(out, 0)
            yes, no = _tri_check(rep, "fn0", terms, None, with_t=True)
            rep.equal("miss gives -1", got, -1.0, no)
            rep.value("t", got, terms[0], yes)
        elif fn in (1, 2):
            o, d = _cols(ar, x, 0), _cols(ar, x, 3)
            for h, k in enumerate((6, 15)):
                terms = tri_terms(ar, o, d, _cols(ar, x, k), _cols(ar, x, k + 3), _cols(ar, x, k + 6), primary=fn == 2)
                _tri_check(rep, f"half {h}", terms, out[:, 2 + h] != 0, with_t=False)
                rep.value(f"t{h}", _f(out, h), terms[0], every)      # the raw quotient: its sign is part of the value
        elif fn == 3:
            t, disc = sphere_terms(ar, _cols(ar, x, 0), _cols(ar, x, 3), _cols(ar, x, 6), ar.inp(x[:, 9]))
            got = _f(out, 0)
            miss, hit = rep.decision("disc < 0", None, disc, 0.0)
            rep.equal("miss gives -1", got, -1.0, miss)
            rep.value("t", got, t, hit)
        elif fn == 4:
            d = _cols(ar, x, 3)
            p, nrm, dn = resolve_terms(ar, _cols(ar, x, 0), d, ar.inp(x[:, 6]), _cols(ar, x, 7), ar.inp(x[:, 10]))
            front, back = rep.decision("front", out[:, 6] != 0, dn, 0.0)
            for k in range(3):
                rep.value("p", _f(out, k), p[k], every)
                rep.value("normal", _f(out, 3 + k), nrm[k], front)
                rep.value("normal", _f(out, 3 + k), ar.neg(nrm[k]), back)
        elif fn == 5:
            i, nrm, ia, ib = _cols(ar, x, 0), _cols(ar, x, 3), ar.inp(x[:, 6]), ar.inp(x[:, 7])
            r = reflect_terms(ar, i, nrm)
            t, k = refract_terms(ar, i, nrm, ar.div(ia, ib))
            total, refr = rep.decision("k < 0", None, k, 0.0)
            for c in range(3):
                rep.value("R", _f(out, c), r[c], every)
                rep.equal("T = 0 on total reflection", _f(out, 3 + c), 0.0, total)
                rep.value("T", _f(out, 3 + c), t[c], refr)
            f, sin2, d_perp, d_par = reflectance_terms(ar, i, nrm, ia, ib)
            below, above = rep.decision("sinSqr >= 1", None, sin2, 1.0)
            eps = float(np.float32(1e-8))
            small_a, big_a = rep.decision("dPerp < 1e-8", None, d_perp, eps, where=below)
            small_b, big_b = rep.decision("dPar < 1e-8", None, d_par, eps, where=below)
            one = above | (below & (small_a | small_b))
            rep.equal("reflectProb = 1", _f(out, 6), 1.0, one)
            rep.value("reflectProb", _f(out, 6), f, below & big_a & big_b)
        elif fn == 6:
            v = _cols(ar, x, 0)
            nv = normalize_terms(ar, v)
            for c in range(3):
                rep.value("normalize", _f(out, c), nv[c], every)
                rep.value("rcp", _f(out, 3 + c), ar.rcp(v[c]), every)
        elif fn == 7:
            i = _shade_inputs(ar, x)
            state_a, u, after_u, state_b = _shade_streams(i["rng"])
            rd_a, rd_b = random_direction_terms(i["rng"].copy()), random_direction_terms(after_u.copy())
            r, prob, k, ends = shade_terms(ar, i["d"], i["nrm"], i["ior"], i["front"], i["rough"], rd_a, rd_b)
            f, sin2, d_perp, d_par = prob
            metal, glass = i["metal"], ~i["metal"]
            total, refr = rep.decision("k < 0", None, k, 0.0, where=glass)
            below, above = rep.decision("sinSqr >= 1", None, sin2, 1.0, where=glass & refr)
            eps = float(np.float32(1e-8))
            small_a, big_a = rep.decision("dPerp < 1e-8", None, d_perp, eps, where=glass & refr & below)
            small_b, big_b = rep.decision("dPar < 1e-8", None, d_par, eps, where=glass & refr & below)
            sure_one = above | (below & (small_a | small_b))             # reflectProb = 1: every rand() <= 1 follows
            known = below & big_a & big_b
            gap = V(f.v - u.astype(np.float64), f.e)                      # rand <= reflectProb: gap >= 0
            away, toward = rep.decision("rand <= reflectProb", None, gap, 0.0, where=glass & refr & known)
            ends_in = {"RA": metal | (glass & total), "RB": glass & refr & (sure_one | (known & toward)),
                       "TB": glass & refr & known & away}
            t_metal, t_absorb = _transmittances(i)
            got_trans = np.stack([_f(out, 6 + c) for c in range(3)], axis=1)
            for name, mask in ends_in.items():
                direction, dn = ends[name]
                for c in range(3):
                    rep.value(f"direction {name}", _f(out, 3 + c), direction[c], mask)
                rep._mark(f"rng state {name}", mask & (out[:, 9] != (state_a if name == "RA" else state_b)))
                want = np.where(metal[:, None], t_metal, t_absorb if name == "TB" else i["trans"])
                want = np.where((glass & i["front"])[:, None], i["trans"], want)
                rep._mark(f"transmittance {name}", mask & (got_trans.view(np.uint32) != want.view(np.uint32)).any(axis=1))
                neg, pos = rep.decision(f"side {name}", None, dn, 0.0, where=mask & glass)
                for c in range(3):
                    bias = ar.mul(ar.const(K_BIAS), i["nrm"][c])
                    rep.value(f"origin {name}", _f(out, c), ar.add(i["p"][c], bias), mask & ((glass & pos) | metal))
                    rep.value(f"origin {name}", _f(out, c), ar.sub(i["p"][c], bias), mask & glass & neg)
        else:
            raise ValueError(fn)
    return rep


def reference_values(fn, x):
    """pt_f64's own binary64 functions on the same inputs, where it has them (fn 0, 3, 5): the values check() must agree
    with, from code that shares nothing with this module."""
    x = np.asarray(x, np.float32).astype(np.float64)
    with np.errstate(**_ERR):
        if fn == 0:
            return pt_f64.ray_triangle(x[:, 0:3], x[:, 3:6], x[:, 6:9], x[:, 9:12], x[:, 12:15])
        if fn == 3:
            return pt_f64.ray_sphere_near(x[:, 0:3], x[:, 3:6], x[:, 6:9], x[:, 9])
        if fn == 5:
            eta = x[:, 6] / x[:, 7]
            return (pt_f64._reflect(x[:, 0:3], x[:, 3:6]), pt_f64._refract(x[:, 0:3], x[:, 3:6], eta),
                    pt_f64.reflectance(x[:, 0:3], x[:, 3:6], x[:, 6], x[:, 7]))
    raise ValueError(fn)


def reference_f32(fn, x):
    """pt_f64's functions evaluated in binary32 (they take the type of their arguments): fn 0 and 3."""
    x = np.asarray(x, np.float32)
    with np.errstate(**_ERR):
        if fn == 0:
            return pt_f64.ray_triangle(x[:, 0:3], x[:, 3:6], x[:, 6:9], x[:, 9:12], x[:, 12:15]).astype(np.float32)
        if fn == 3:
            return pt_f64.ray_sphere_near(x[:, 0:3], x[:, 3:6], x[:, 6:9], x[:, 9]).astype(np.float32)
    raise ValueError(fn)


# ---- input sets ---------------------------------------------------------------------------------------------------------
# Every set is a float32 array [n, in_words] in the hook's layout, built in binary64 and rounded once; the same arrays go
# to the CPU checks of the bounds and to the kernels. The sizes and ranges are chosen so that the cases the kernels can get
# wrong are present while at most 2 % of a set lies nearer to a decision threshold than the bound (see each comment).
def _unit(rng, n):
    v = rng.normal(size=(n, 3))
    return v / np.linalg.norm(v, axis=1, keepdims=True)


def _tri_rays(rng, n, uv, centre=0.0, size=1.0, dist=(1.0, 5.0), origin=None, backwards=False, fat=0.2):
    """Triangles of edge length ~size around `centre`, each with a ray through a + u e1 + v e2 for the given (u, v)[n, 2],
    from an origin `dist` away (or the given one): (o, d, a, b, c) as float64."""
    a = centre + size * rng.uniform(-1, 1, (n, 3))
    b = a + size * rng.uniform(0.3, 1.0, (n, 1)) * _unit(rng, n)
    c = a + size * rng.uniform(0.3, 1.0, (n, 1)) * _unit(rng, n)
    bad = np.linalg.norm(np.cross(b - a, c - a), axis=1) < fat * np.linalg.norm(b - a, axis=1) * np.linalg.norm(c - a, axis=1)
    c[bad] = a[bad] + np.cross(b[bad] - a[bad], _unit(rng, int(bad.sum())))        # no slivers here: own set below
    hit = a + uv[:, :1] * (b - a) + uv[:, 1:] * (c - a)
    if origin is None:
        origin = hit + rng.uniform(*dist, (n, 1)) * size * _unit(rng, n)
    d = hit - origin
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return origin, (-d if backwards else d), a, b, c


def _inside(rng, n, margin=0.02):
    u = rng.uniform(margin, 1 - 2 * margin, n)
    v = rng.uniform(margin, 1 - margin - u)
    return np.stack([u, v], axis=1)


def _pack0(o, d, a, b, c):
    return np.concatenate([o, d, a, b, c], axis=1).astype(np.float32)


def _graze(rng, n, lo, hi, axis_plane):
    """Rays at a sine of lo..hi (log-uniform, either side) to the plane of a triangle, through a point inside it, so
    |det| = that sine times |e1 x e2|. axis_plane: the triangle lies in z = 0 and the terms of u, v and t stay small with
    det; in a general position the terms of dot(oa, p) stay O(|oa| |p|) while det shrinks, and u is known only to ~1e-7 /
    sine, and v (a sum of terms ~|q| / det) worse -- which is why that variant stops at 3e-3."""
    uv = _inside(rng, n, 0.15)
    o, d, a, b, c = _tri_rays(rng, n, uv, fat=0.5)
    if axis_plane:
        a[:, 2] = b[:, 2] = c[:, 2] = 0.0
    hit = a + uv[:, :1] * (b - a) + uv[:, 1:] * (c - a)
    nrm = np.cross(b - a, c - a)
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    g = np.cross(nrm, _unit(rng, n))
    g /= np.linalg.norm(g, axis=1, keepdims=True)
    s = 10.0 ** rng.uniform(np.log10(lo), np.log10(hi), (n, 1)) * rng.choice([-1.0, 1.0], (n, 1))
    d = g + s * nrm
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    o = hit - rng.uniform(0.5, 2.0, (n, 1)) * d
    return _pack0(o, d, a, b, c)


def _steep(x, n, cos=0.3):
    """The first n items whose ray meets the triangle's plane at |cos| >= 0.3 to the normal (grazing has its own sets)."""
    x64 = x.astype(np.float64)
    nrm = np.cross(x64[:, 9:12] - x64[:, 6:9], x64[:, 12:15] - x64[:, 6:9])
    c = np.abs((nrm * x64[:, 3:6]).sum(1)) / np.linalg.norm(nrm, axis=1) / np.linalg.norm(x64[:, 3:6], axis=1)
    x = x[c >= cos][:n]
    assert len(x) == n
    return x


def triangle_sets(n=1024):
    """fn 0 items (origin, direction, a, b, c) by case."""
    rng = np.random.default_rng(401)
    sets = {}
    sets["inside"] = _pack0(*_tri_rays(rng, n, _inside(rng, n)))
    # 1e-4 .. 1e-3 (barycentric) to either side of an edge, from an origin within an edge length: there u, v and u + v
    # are known to ~1e-5 (the bound grows with |oa|), so nearer points could not be decided
    near = lambda: 10.0 ** rng.uniform(-4, -3, n) * rng.choice([-1.0, 1.0], n)        # noqa: E731
    k, off, s = rng.integers(0, 3, n), near(), rng.uniform(0.1, 0.8, n)
    uv = np.where((k == 0)[:, None], np.stack([off, s], 1),
                  np.where((k == 1)[:, None], np.stack([s, off], 1), np.stack([s, 1 - s - off], 1)))
    sets["edges"] = _pack0(*_tri_rays(rng, n, uv, dist=(0.3, 1.0), fat=0.5))
    # the same distances from both edges that meet in a vertex, in all four quadrants around it
    k, p, q = rng.integers(0, 3, n), near(), near()
    uv = np.where((k == 0)[:, None], np.stack([p, q], 1),
                  np.where((k == 1)[:, None], np.stack([1 - p - q, p], 1), np.stack([p, 1 - p - q], 1)))
    sets["vertices"] = _pack0(*_tri_rays(rng, n, uv, dist=(0.3, 1.0), fat=0.5))
    sets["grazing_axis_plane"] = _graze(rng, n, 1e-6, 1e-2, True)
    sets["grazing"] = _graze(rng, n, 3e-3, 1e-1, False)
    # the origin (nearly) on the plane. Under a point inside the triangle t ~ 0 is all rounding error and t > 0 cannot be
    # decided, so for fn 0 the origin sits 1e-4 .. 1e-2 to either side of the plane (half the items), or in the plane under a
    # point outside the triangle (the other half: a miss whatever t is)
    uv = _inside(rng, n)
    uv[n // 2:, 0] = -rng.uniform(0.2, 1.0, n - n // 2)
    o, d, a, b, c = _tri_rays(rng, n, uv)
    nrm = np.cross(b - a, c - a)
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    h = 10.0 ** rng.uniform(-4, -2, (n, 1)) * rng.choice([-1.0, 1.0], (n, 1))
    h[n // 2:] = 0.0
    o = a + uv[:, :1] * (b - a) + uv[:, 1:] * (c - a) + h * nrm
    d = np.where(h != 0, -np.sign(h) * nrm, _unit(rng, n)) + 0.3 * _unit(rng, n)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    sets["origin_on_plane"] = _pack0(o, d, a, b, c)
    # 1e3 units between origin and triangle: u, v and t are known to ~1e-3 (|oa| times the near cases' bound)
    m = 2 * n
    far = 1e3 * _unit(rng, m)
    sets["far_triangle"] = _steep(_pack0(*_tri_rays(rng, m, _inside(rng, m, 0.15), centre=far,
                                                    origin=rng.uniform(-1, 1, (m, 3)), fat=0.5)), n)
    sets["far_origin"] = _steep(_pack0(*_tri_rays(rng, m, _inside(rng, m, 0.15), origin=far + rng.uniform(-1, 1, (m, 3)),
                                                  fat=0.5)), n)
    sets["negative_t"] = _pack0(*_tri_rays(rng, n, _inside(rng, n), backwards=True))
    return sets


def never_accepted_sets(n=256):
    """fn 0 items whose det is exactly zero in every arithmetic (each term has a zero factor), so t, u and v are
    infinite or NaN and no bound applies: the item must be a miss. parallel: triangle and direction in z = const;
    degenerate: b = a (e1 = 0) or c = a (e2 = 0)."""
    rng = np.random.default_rng(402)
    o, d, a, b, c = _tri_rays(rng, n, _inside(rng, n))
    z = rng.uniform(-1, 1, n)
    a[:, 2] = b[:, 2] = c[:, 2] = z
    d[:, 2] = 0.0
    o[: n // 2, 2] = z[: n // 2]                       # half of them with the origin in the plane too
    sets = {"parallel": _pack0(o, d, a, b, c)}
    o, d, a, b, c = _tri_rays(rng, n, _inside(rng, n))
    b[: n // 2] = a[: n // 2]
    c[n // 2:] = a[n // 2:]
    sets["degenerate"] = _pack0(o, d, a, b, c)
    return sets


def sliver_set(n=256):
    """fn 0 items with c = b (e1 = e2): det is zero only up to rounding, so nothing can be said beyond the exact mode's
    bits."""
    rng = np.random.default_rng(403)
    o, d, a, b, c = _tri_rays(rng, n, _inside(rng, n))
    return _pack0(o, d, a, b, b)


def pair_items(x0, other=None):
    """fn 1 / fn 2 items from fn 0 items: the ray and triangle of x0 in half 0, the triangle of `other` (default: the next
    item's, which the ray mostly misses) in half 1. The edges are the binary32 differences the records hold."""
    x0 = np.asarray(x0, np.float32)
    other = np.roll(x0, 1, axis=0) if other is None else np.asarray(other, np.float32)

    def rec(x):
        return np.concatenate([x[:, 6:9], x[:, 9:12] - x[:, 6:9], x[:, 12:15] - x[:, 6:9]], axis=1).astype(np.float32)

    return np.concatenate([x0[:, :6], rec(x0), rec(other)], axis=1)


def _aim(rng, c, r, o, impact):
    """Unit directions from o that pass the centre c at `impact` times the radius."""
    to = c - o
    dist = np.linalg.norm(to, axis=1, keepdims=True)
    to /= dist
    side = np.cross(to, _unit(rng, len(c)))
    side /= np.linalg.norm(side, axis=1, keepdims=True)
    sin = impact * r / dist
    d = np.sqrt(np.maximum(1 - sin * sin, 0.0)) * to + sin * side
    return d / np.linalg.norm(d, axis=1, keepdims=True)


def sphere_sets(n=1024):
    """fn 3 items (origin, direction, centre, radius) by case."""
    rng = np.random.default_rng(404)
    col = lambda lo, hi: rng.uniform(lo, hi, (n, 1))                      # noqa: E731
    pack = lambda o, d, c, r: np.concatenate([o, d, c, r], axis=1).astype(np.float32)   # noqa: E731
    sets = {}
    c, r = rng.uniform(-1, 1, (n, 3)), np.ones((n, 1))
    o = c + col(2, 5) * _unit(rng, n)
    impact = np.where(rng.uniform(size=(n, 1)) < 0.75, col(0, 0.95), col(1.05, 2.0))   # three hits to one miss
    sets["unit"] = pack(o, _aim(rng, c, r, o, impact), c, r)
    # the ground sphere of the reference's scene seen from 0.5 .. 3 above it: dot(oc, oc) and b * b are ~1e4, c ~1e2
    c, r = np.tile([0.0, -100.0, 0.0], (n, 1)), np.full((n, 1), 100.0)
    up = _unit(rng, n) * [0.3, 0.0, 0.3] + [0.0, 1.0, 0.0]
    up /= np.linalg.norm(up, axis=1, keepdims=True)
    o = c + (r + col(0.5, 3.0)) * up
    sets["ground"] = pack(o, _aim(rng, c, r, o, np.where(rng.uniform(size=(n, 1)) < 0.75, col(0, 0.9), col(1.001, 1.02))), c, r)
    c, r = rng.uniform(-1, 1, (n, 3)), col(0.5, 2.0)
    sets["inside"] = pack(c + col(0, 0.9) * r * _unit(rng, n), _unit(rng, n), c, r)
    # tangent rays: the impact parameter within 1e-4 .. 1e-2 of the radius on either side (the discriminant 2 r^2 off is
    # known to ~1e-5 |oc|^2); one item in 64 within 1e-9, where the discriminant lies inside its bound (undecided by
    # construction, and kept under the cap by their number)
    o = c + col(1.5, 3) * r * _unit(rng, n)
    off = 10.0 ** rng.uniform(-4, -2, (n, 1)) * rng.choice([-1.0, 1.0], (n, 1))
    off[::64] = 1e-9 * rng.choice([-1.0, 1.0], (len(off[::64]), 1))
    sets["tangent"] = pack(o, _aim(rng, c, r, o, 1.0 + off), c, r)
    sets["behind"] = pack(o, -_aim(rng, c, r, o, col(0, 0.9)), c, r)
    return sets


def resolve_sets(n=1024):
    """fn 4 items (origin, direction, t, centre, radius): a hit from outside (front, the near root) and from inside (back,
    the far root) with t the rounded binary64 root, at impact parameters up to 0.95 r."""
    rng = np.random.default_rng(405)
    sets = {}
    for name, radius, inside in (("unit_front", 1.0, False), ("unit_back", 1.0, True), ("ground_front", 100.0, False)):
        c = rng.uniform(-1, 1, (n, 3)) if radius == 1.0 else np.tile([0.0, -100.0, 0.0], (n, 1))
        r = np.full((n, 1), radius)
        if inside:
            o, d = c + rng.uniform(0, 0.9, (n, 1)) * r * _unit(rng, n), _unit(rng, n)
        else:
            o = c + (r + rng.uniform(0.5, 3.0, (n, 1))) * _unit(rng, n)
            d = _aim(rng, c, r, o, rng.uniform(0, 0.95, (n, 1)))
        o, d, c, r = (v.astype(np.float32).astype(np.float64) for v in (o, d, c, r))
        oc = o - c
        b = (oc * d).sum(1, keepdims=True)
        disc = b * b - ((oc * oc).sum(1, keepdims=True) - r * r) * (d * d).sum(1, keepdims=True)
        t = (-b + (1 if inside else -1) * np.sqrt(disc)) / (d * d).sum(1, keepdims=True)
        sets[name] = np.concatenate([o, d, t, c, r], axis=1).astype(np.float32)
    return sets


IORS = (1.0, 1.0000001, 1.33, 1.5, 2.5)


def _optics(rng, cos, ia, ib):
    """(direction, normal, iorA, iorB) with dot(direction, normal) = -cos."""
    n = len(cos)
    nrm = _unit(rng, n)
    tang = np.cross(nrm, _unit(rng, n))
    tang /= np.linalg.norm(tang, axis=1, keepdims=True)
    cos = np.asarray(cos, np.float64)[:, None]
    d = -cos * nrm + np.sqrt(np.maximum(1 - cos * cos, 0.0)) * tang
    return np.concatenate([d, nrm, np.asarray(ia)[:, None], np.asarray(ib)[:, None]], axis=1).astype(np.float32)


def optics_sets(n=2048):
    """fn 5 items by case."""
    rng = np.random.default_rng(406)
    pairs = [(1.0, i) for i in IORS] + [(i, 1.0) for i in IORS]
    sets = {}
    # cos in {1, 0.5, 1e-3, 1e-6} x every ior pair, 4 directions each (160 items). At cos = 1e-6 with a ratio within 1e-6 of
    # 1 sinSqr lies inside its bound of 1 whatever the kernel does, so the grid is filled up with random incidences (cos
    # uniform in (0, 1)) until those few combinations are under the cap.
    grid = [(cs, a, b) for cs in (1.0, 0.5, 1e-3, 1e-6) for a, b in pairs for _ in range(4)]
    fill = [(cs, *pairs[k]) for cs, k in zip(rng.uniform(0.01, 1.0, n), rng.integers(0, len(pairs), n))]
    cs, a, b = (np.array(v) for v in zip(*(grid + fill)))
    sets["incidence"] = _optics(rng, cs, a, b)
    # around the critical angle of the dense -> thin pairs: sin^2 = eta^2 (1 - cos^2) within 1e-5 .. 1e-2 of 1
    ior = rng.choice([1.33, 1.5, 2.5], n)
    sin2 = 1.0 + 10.0 ** rng.uniform(-5, -2, n) * rng.choice([-1.0, 1.0], n)
    sets["critical_angle"] = _optics(rng, np.sqrt(1 - sin2 / ior ** 2), ior, np.ones(n))
    # the denominators' exit. With cos >= 0 it cannot be taken in binary32: sinSqr < 1 means 1 - sinSqr >= 2^-24, so
    # cosRefr >= 2^-12 and both denominators exceed 1e-8. A direction on the normal's side (cos < 0) takes it: dPerp or
    # dPar is then negative for most angles, positive for some (ratio 1 would leave them at 0 +- rounding: left out).
    k = rng.integers(0, 6, n)
    ior = np.array([1.33, 1.5, 2.5])[k % 3]
    sets["small_denominators"] = _optics(rng, -rng.uniform(0.05, 1.0, n), np.where(k < 3, 1.0, ior), np.where(k < 3, ior, 1.0))
    return sets


def vector_sets(n=1024):
    """fn 6 items: vectors of length 1e-3 .. 1e3, nearly unit vectors (what path_shade normalises), and vectors along an axis
    up to a 1e-4 part (the reciprocal of a small component)."""
    rng = np.random.default_rng(407)
    v = _unit(rng, n)
    axis = np.eye(3)[rng.integers(0, 3, n)] + 1e-4 * v
    return {"lengths": (v * 10.0 ** rng.uniform(-3, 3, (n, 1))).astype(np.float32),
            "near_unit": (v * (1 + rng.uniform(-0.3, 0.3, (n, 1)))).astype(np.float32),
            "near_axis": axis.astype(np.float32)}


def origin_in_plane_set(n=512):
    """fn 0 items with the origin in the triangle's plane under a point inside it: t ~ 0 is rounding error only, so fn 0's
    acceptance is undecided, but the raw t of fn 1 / fn 2 must still lie within its bound of zero."""
    rng = np.random.default_rng(408)
    uv = _inside(rng, n, 0.1)
    o, d, a, b, c = _tri_rays(rng, n, uv)
    return _pack0(a + uv[:, :1] * (b - a) + uv[:, 1:] * (c - a), _unit(rng, n), a, b, c)


def scatter_sets(n=1536):
    """fn 7 items: metal and dielectric x roughness 0 / 0.3 / 1 x front and back hits, incidence cos 0.05 .. 1 against the
    (already flipped) normal, ior 1.33 / 1.5 / 2.5 (a back hit inside the denser medium reflects totally past its critical
    angle), nonzero absorption (applied on a refracted back hit), seeds pcg_hash(pixel index)."""
    rng = np.random.default_rng(409)
    k = np.arange(n)
    geo = _optics(rng, rng.uniform(0.05, 1.0, n), np.ones(n), np.ones(n))
    d, nrm = geo[:, 0:3].astype(np.float64), geo[:, 3:6].astype(np.float64)
    t = rng.uniform(0.5, 3.0, (n, 1))
    p = rng.uniform(-2, 2, (n, 3))
    mat = np.zeros((n, 15), np.float32)
    mat[:, 1:4] = rng.uniform(0.1, 1.0, (n, 3))                          # albedo
    mat[:, 9] = np.array([0.0, 0.3, 1.0])[(k // 2) % 3]                  # roughness
    mat[:, 10:13] = rng.uniform(0.1, 1.0, (n, 3))                        # absorption
    mat[:, 13] = 0.7
    mat[:, 14] = np.array([1.33, 1.5, 2.5])[(k // 12) % 3]
    mat = mat.view(np.uint32)
    mat[:, 0] = k % 2                                                    # type: metal, dielectric
    words = np.zeros((n, 33), np.uint32)
    words[:, 0:13] = np.concatenate([p - t * d, d, p, nrm, t], axis=1).astype(np.float32).view(np.uint32)
    words[:, 13] = (k // 6) % 2                                          # front
    words[:, 14:29] = mat
    words[:, 29] = pt_f64.pcg_hash(k.astype(np.uint32) + np.uint32(719393))
    words[:, 30:33] = rng.uniform(0.2, 1.0, (n, 3)).astype(np.float32).view(np.uint32)
    return {"scatter": words.view(np.float32)}


def all_sets():
    """{(fn, name): items} for every set that is checked against the bounds, fn 1 and 2 on the triangles of fn 0."""
    out = {}
    tris = triangle_sets()
    for name, x in tris.items():
        out[0, name] = x
        for fn in (1, 2):
            out[fn, name] = pair_items(x)
    for fn in (1, 2):
        out[fn, "origin_in_plane_inside"] = pair_items(origin_in_plane_set())
    for fn, sets in ((3, sphere_sets()), (4, resolve_sets()), (5, optics_sets()), (6, vector_sets()), (7, scatter_sets())):
        for name, x in sets.items():
            out[fn, name] = x
    return out


# ---- fn 8: the child-pair decision and the root cull -------------------------------------------------------------------
# No arithmetic object here: the box test is the same binary32 operations in both modes, and every output is a decision or
# a distance that decisions read, so the check is bit for bit (a NaN distance matching any NaN).
def _ray_box32(o, inv, bmin, bmax):
    """rayBoxIntersect (pathTracer.comp:97-108, oracle/pt_oracle.c) in binary32: (t0, t1). GLSL min / max are IEEE minNum /
    maxNum -- a NaN operand gives the other one -- which is np.fmin / np.fmax."""
    tbot = [(bmin[k] - o[k]) * inv[k] for k in range(3)]
    ttop = [(bmax[k] - o[k]) * inv[k] for k in range(3)]
    tmin = [np.fmin(ttop[k], tbot[k]) for k in range(3)]
    tmax = [np.fmax(ttop[k], tbot[k]) for k in range(3)]
    t0 = np.fmax(np.fmax(tmin[0], tmin[1]), np.fmax(tmin[0], tmin[2]))
    t1 = np.fmin(np.fmin(tmax[0], tmax[1]), np.fmin(tmax[0], tmax[2]))
    assert t0.dtype == np.float32 and t1.dtype == np.float32
    return t0, t1


def child_pair_model(x):
    """What wcpt_selftest_geometry(8) returns for the items x[n, 19] (float32: origin, invDirection, left box min, max, right
    box min, max, rec.t), in the oracle's expressions (pt_oracle.c Intersect): left popped first iff leftDist < rightDist
    with dist = t0 > 0 ? t0 : t1; a box passes unless t0 > t1 || t1 < 0; a root survives unless that or t0 > rec.t. Every
    comparison with a NaN is false, as in C."""
    x = np.asarray(x, np.float32)
    c = lambda k: tuple(x[:, k + i] for i in range(3))                   # noqa: E731
    with np.errstate(**_ERR):
        l0, l1 = _ray_box32(c(0), c(3), c(6), c(9))
        r0, r1 = _ray_box32(c(0), c(3), c(12), c(15))
        left_dist, right_dist = np.where(l0 > 0, l0, l1), np.where(r0 > 0, r0, r1)
        culled_l, culled_r = (l0 > l1) | (l1 < 0), (r0 > r1) | (r1 < 0)
        return _u32(_flag(left_dist < right_dist), _flag(~culled_l), _flag(~culled_r), l0, r0,
                    _flag(~(culled_l | (l0 > x[:, 18]))))


def child_pair_set():
    """fn 8 items by case, a few dozen of each (a few hundred in all). The one thing left out on purpose: a min or max of
    two zeros of different sign, whose sign IEEE 754-2008 leaves open (v_min_f32, C's compare-select and numpy differ) and
    no decision reads; so no finite invDirection meets an origin on a slab plane here (with an infinite one the product is
    NaN, which is the case that matters)."""
    rng = np.random.default_rng(410)
    inf, nan, big = np.float32(np.inf), np.float32(np.nan), np.float32(3.402823466e+38)
    n = 32

    def boxes(k):
        lo = rng.uniform(-2, 2, (k, 3))
        return lo, lo + rng.uniform(0.1, 2, (k, 3))

    def items(k, o=None, d=None, lb=None, rb=None, rt=None):
        o = rng.uniform(-3, 3, (k, 3)) if o is None else o
        d = _unit(rng, k) if d is None else d
        lb, rb = boxes(k) if lb is None else lb, boxes(k) if rb is None else rb
        rt = 10.0 ** rng.uniform(-1, 1.5, (k, 1)) if rt is None else rt
        with np.errstate(**_ERR):
            inv = np.float32(1.0) / np.asarray(d, np.float32)           # 1 / +-0 = +-inf, as rcp3 gives
        return np.concatenate([np.asarray(o, np.float32), inv, *[np.asarray(v, np.float32) for v in (*lb, *rb)],
                               np.asarray(rt, np.float32)], axis=1).astype(np.float32)

    def near(lb):
        """a box that overlaps lb: the same ray mostly meets both, so the pop order is a real decision"""
        shift = rng.uniform(-0.5, 0.5, lb[0].shape)
        return lb[0] + shift, lb[1] + shift

    def through(lb, k, d=None):
        """origins 1 .. 4 behind a point inside the box lb along the direction d (default: random unit vectors)"""
        p = lb[0] + rng.uniform(0.1, 0.9, (k, 3)) * (lb[1] - lb[0])
        d = _unit(rng, k) if d is None else d
        return p - rng.uniform(1, 4, (k, 1)) * d, d

    def hitting(k):
        lb = boxes(k)
        return (*through(lb, k), lb, near(lb))

    row = np.arange(n)
    sets = [items(2 * n), items(2 * n, *hitting(2 * n))]                # random boxes and rays; rays through the left box
    # invDirection components of +-inf (direction components +-0; a quarter of the items have two): the origin inside the
    # slab, outside it, and on one of the four planes of the two boxes (0 * inf = NaN for that plane)
    for where in ("inside", "outside", "plane"):
        lb = boxes(n)
        rb = near(lb)
        d = _unit(rng, n)
        axis = rng.integers(0, 3, n)
        d[row, axis] = 0.0 * rng.choice([-1.0, 1.0], n)
        two = rng.uniform(size=n) < 0.25
        d[two, (axis[two] + 1) % 3] = 0.0 * rng.choice([-1.0, 1.0], int(two.sum()))
        o, d = through(lb, n, d)                                        # inside the left box's slab on the zero axes
        if where == "outside":
            o[row, axis] += rng.choice([-3.0, 3.0], n)
        elif where == "plane":
            planes = np.stack([*lb, *rb])[:, row, axis]                 # left min, left max, right min, right max
            o[row, axis] = np.float32(planes[rng.integers(0, 4, n), row])   # the binary32 plane itself
        sets.append(items(n, o, d, lb, rb))
    # every distance NaN: a box of no extent that holds the origin, and no direction at all (0 * inf on all six planes)
    o = rng.uniform(-3, 3, (n, 3)).astype(np.float32)
    flat, zero = (o, o), 0.0 * rng.choice([-1.0, 1.0], (n, 3))
    sets += [items(n, o, zero, flat, flat), items(n, o, zero, flat, boxes(n)), items(n, o, zero, boxes(n), flat)]
    lb = boxes(n)
    sets.append(items(n, *through(lb, n), lb, lb))                      # equal boxes: leftDist == rightDist
    x = items(n, *hitting(n))
    x[:, 12:15], x[:, 15:18] = 2 * x[:, 0:3] - x[:, 9:12], 2 * x[:, 0:3] - x[:, 6:9]
    sets.append(x)                                                      # the right box is the left one mirrored at the origin
    o, d, lb, rb = hitting(n)
    sets.append(items(n, o, -d, lb, rb))                                # both boxes behind the ray
    sets.append(items(n, *through(lb, n, -d), boxes(n), lb))            # the right one alone
    x = items(n, *hitting(n))
    with np.errstate(**_ERR):
        x[:, 18] = _ray_box32(*[tuple(x[:, k + i] for i in range(3)) for k in (0, 3, 6, 9)])[0]
    sets.append(x)                                                      # rec.t equal to the left box's t0: survives
    below = x.copy()
    below[:, 18] = np.nextafter(x[:, 18], -inf)
    sets.append(below)                                                  # and one ULP below it: culled
    x = items(n, *hitting(n))
    x[:, 18] = big
    x[n // 2:, 18] = inf
    sets.append(x)                                                      # rec.t = kInfinity (and +inf)
    x = np.concatenate([items(n), items(n, *hitting(n))])
    x[np.arange(2 * n), 6 + rng.integers(0, 12, 2 * n)] = nan
    sets.append(x)                                                      # NaN in a box word
    x = items(n, *hitting(n))
    x[row, 6 + rng.integers(0, 12, n)] = rng.choice([-inf, inf], n)
    sets.append(x)                                                      # an infinite box word
    return np.concatenate(sets).astype(np.float32)
