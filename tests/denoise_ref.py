"""Numpy restatement of the guided a-trous denoise (wc-path-tracer_amd/csrc/wcpt_denoise.h), from the rule's words and not
from the header's code: float32 with one rounding per operation, oracle.expf for the exponential, the guide taken from
the primary-hit records as they are (no packing). Test input, no product code. A tap is one whole-frame array operation,
so a frame of 37x23 pixels costs 25 of them (and as many exponentials as taps) per iteration."""
import numpy as np

import oracle
import wcpt

T = wcpt._lib
F = np.float32
H3 = (F(3.0 / 8.0), F(1.0 / 4.0), F(1.0 / 16.0))


def _expf(a):
    flat = np.ascontiguousarray(a, F).ravel()
    return np.array([oracle.expf(float(v)) for v in flat], F).reshape(a.shape)


def guide_of(rec, sigma_depth):
    """hit, kind, key, n, P, izt2 of the records [H, W] (PRIMARY_HIT_DTYPE)."""
    kind = rec["kind"] & T.HIT_KIND_MASK
    hit = kind != T.HIT_MISS
    key = np.where(kind == T.HIT_SPHERE, rec["index"], np.where(kind == T.HIT_TRIANGLE, rec["draw"], 0)).astype(np.uint32)
    t = rec["t"].astype(F)
    with np.errstate(all="ignore"):
        P = (t[..., None] * rec["direction"].astype(F)).astype(F)
        st = F(sigma_depth) * t
        izt2 = (F(1.0) / (st * st)).astype(F)
    n = rec["normal"].astype(F).copy()
    P[~hit] = 0
    n[~hit] = 0
    izt2[~hit] = 0
    return hit, kind, key, n, P, izt2


def _dist2(a, b):
    d = a - b
    return (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]


def iteration(c, guide, step, isc2, isn2):
    """One iteration of step `step` over the float4 image `c` [H, W, 4]."""
    hit, kind, key, n, P, izt2 = guide
    Hh, Ww = c.shape[:2]
    acc = np.zeros((Hh, Ww, 3), F)
    ws = np.zeros((Hh, Ww), F)
    for dy in range(-2, 3):
        for dx in range(-2, 3):
            oy, ox = step * dy, step * dx
            # the pixels p whose tap q = p + (ox, oy) lies inside the frame
            y0, y1 = max(0, -oy), min(Hh, Hh - oy)
            x0, x1 = max(0, -ox), min(Ww, Ww - ox)
            if y0 >= y1 or x0 >= x1:
                continue
            p = (slice(y0, y1), slice(x0, x1))
            q = (slice(y0 + oy, y1 + oy), slice(x0 + ox, x1 + ox))
            k = H3[abs(dx)] * H3[abs(dy)]
            same = (kind[p] == kind[q]) & (key[p] == key[q])
            with np.errstate(all="ignore"):
                e = _dist2(c[p][..., :3], c[q][..., :3]) * isc2
                eh = e + _dist2(n[p], n[q]) * isn2
                d = P[q] - P[p]
                dz = (n[p][..., 0] * d[..., 0] + n[p][..., 1] * d[..., 1]) + n[p][..., 2] * d[..., 2]
                eh = eh + dz * dz * izt2[p]
                e = np.where(hit[p], eh, e).astype(F)
                w = k * _expf(-e)
                take = same & (w > 0)
                w = np.where(take, w, F(0))
                cq = np.where(take[..., None], c[q][..., :3], F(0))     # a skipped tap adds nothing, not 0 * inf
                acc[p] = acc[p] + w[..., None] * cq
                ws[p] = ws[p] + w
    out = c.copy()
    ok = ws > 0
    with np.errstate(all="ignore"):
        out[..., :3] = np.where(ok[..., None], acc / np.where(ok, ws, F(1))[..., None], c[..., :3])
    return out


def filtered(img, rec, iterations=5, sigma_color=4.0, sigma_normal=0.5, sigma_depth=0.05):
    """The last iteration's float4 image."""
    c = np.ascontiguousarray(img, F)
    with np.errstate(all="ignore"):
        isc2 = F(1.0) / (F(sigma_color) * F(sigma_color))
        isn2 = F(1.0) / (F(sigma_normal) * F(sigma_normal))
    guide = guide_of(rec, sigma_depth)
    for i in range(iterations):
        c = iteration(c, guide, 1 << i, isc2, isn2)
    return c


def denoise(img, rec, iterations=5, sigma_color=4.0, sigma_normal=0.5, sigma_depth=0.05):
    """(rgba32f, rgba8): the display step (the existing oracle's composite) of the filtered image."""
    return oracle.composite(filtered(img, rec, iterations, sigma_color, sigma_normal, sigma_depth))
