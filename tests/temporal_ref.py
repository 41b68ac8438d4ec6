"""Numpy restatement of the temporal reprojection (wc-path-tracer_amd/csrc/wcpt_temporal.h), from the rule's words and not
from the header's code: float32 with one rounding per operation, the records taken as they are (no packing), the camera's F
formed in float64 by the elimination the rule spells out. Test input, no product code. A tap is one whole-frame array
operation."""
import math

import numpy as np

import wcpt

T = wcpt._lib
F = np.float32


# ---- the camera: float64 -------------------------------------------------------------------------------------------------
def inverse(m):
    """Gauss-Jordan on [M | I] with the rule's pivoting; None when singular. Python floats are binary64."""
    n = len(m)
    t = [[float(m[r][c]) for c in range(n)] + [1.0 if c == r else 0.0 for c in range(n)] for r in range(n)]
    for col in range(n):
        piv = col
        for r in range(col + 1, n):
            if abs(t[r][col]) > abs(t[piv][col]):
                piv = r
        if not abs(t[piv][col]) >= 1e-300:
            return None
        t[piv], t[col] = t[col], t[piv]
        d = t[col][col]
        t[col] = [v / d for v in t[col]]
        for r in range(n):
            f = t[r][col]
            if r == col or f == 0.0:
                continue
            t[r] = [a - f * b for a, b in zip(t[r], t[col])]
    return [row[n:] for row in t]


def _project64(Fm, r, w, h):
    cx, cy, cw = ((float(Fm[i][0]) * r[0] + float(Fm[i][1]) * r[1]) + float(Fm[i][2]) * r[2] for i in range(3))
    if not cw > 0.0:
        return None
    return (cx / cw * 0.5 + 0.5) * w - 0.5, (1.0 - (cy / cw * 0.5 + 0.5)) * h - 0.5


def camera(sd, w, h):
    """(F [3, 3] float32, position [3] float32) of the scene data for a w x h frame, or None where the rule refuses it."""
    ip = np.asarray(sd["inverseProjection"], np.float64).reshape(4, 4).T.tolist()      # column-major
    a = np.asarray(sd["inverseView"], np.float64).reshape(4, 4).T[:3, :3].tolist()
    with np.errstate(all="ignore"):
        try:
            P, ai = inverse(ip), inverse(a)
        except (OverflowError, ZeroDivisionError):
            return None
    if P is None or ai is None or w == 0 or h == 0:
        return None
    R = [P[0][:3], P[1][:3], P[3][:3]]
    with np.errstate(all="ignore"):
        Fm = np.array([[(R[i][0] * ai[0][j] + R[i][1] * ai[1][j]) + R[i][2] * ai[2][j] for j in range(3)] for i in range(3)],
                      np.float64).astype(F)
    for x in (0.0, w - 1.0):
        for y in (0.0, h - 1.0):
            try:
                cx = x / w + (1.0 / w) * 0.5
                cy = 1.0 - (y / h + (1.0 / h) * 0.5)
                cx, cy = cx * 2.0 - 1.0, cy * 2.0 - 1.0
                tg = [((ip[r][0] * cx + ip[r][1] * cy) + ip[r][2]) + ip[r][3] for r in range(4)]
                d = [tg[c] / tg[3] for c in range(3)]
                dl = math.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2])
                d = [v / dl for v in d]
                wd = [(a[r][0] * d[0] + a[r][1] * d[1]) + a[r][2] * d[2] for r in range(3)]
                wl = math.sqrt((wd[0] * wd[0] + wd[1] * wd[1]) + wd[2] * wd[2])
                wd = [v / wl for v in wd]
                p = _project64(Fm, wd, float(w), float(h))
            except (OverflowError, ZeroDivisionError, ValueError):
                return None
            if p is None or not (abs(p[0] - x) <= 1e-3 and abs(p[1] - y) <= 1e-3):
                return None
    return Fm, np.asarray(sd["position"], F).reshape(3).copy()


# ---- per pixel: float32 ----------------------------------------------------------------------------------------------------
def guide_of(rec, o):
    """hit, kind, key, n, W, t, direction of the records [H, W] for the camera position o."""
    kind = (rec["kind"] & T.HIT_KIND_MASK).astype(np.uint32)
    t = rec["t"].astype(F)
    hit = ((kind == T.HIT_SPHERE) | (kind == T.HIT_TRIANGLE)) & ~np.isnan(t)
    kind = np.where(hit, kind, 0).astype(np.uint32)
    key = np.where(kind == T.HIT_SPHERE, rec["index"], np.where(kind == T.HIT_TRIANGLE, rec["draw"], 0)).astype(np.uint32)
    d = rec["direction"].astype(F)
    with np.errstate(all="ignore"):
        Wp = (np.asarray(o, F)[None, None, :] + (t[..., None] * d).astype(F)).astype(F)
    n = rec["normal"].astype(F).copy()
    Wp[~hit] = 0
    n[~hit] = 0
    return hit, kind, key, n, Wp, t, d


def _dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def positions(rec, o, cam, w, h):
    """Steps 2 to 4: (valid, fx, fy) of every pixel of the records in the frame of the camera `cam`."""
    Fm, oh = cam
    hit, kind, key, n, Wp, t, d = guide_of(rec, o)
    with np.errstate(all="ignore"):
        r = np.where(hit[..., None], (Wp - oh[None, None, :]).astype(F), d)
        cx, cy, cw = (((Fm[i, 0] * r[..., 0] + Fm[i, 1] * r[..., 1]) + Fm[i, 2] * r[..., 2]).astype(F) for i in range(3))
        nx, ny = (cx / cw).astype(F), (cy / cw).astype(F)
        fx = ((nx * F(0.5) + F(0.5)) * F(w) - F(0.5)).astype(F)
        fy = ((F(1.0) - (ny * F(0.5) + F(0.5))) * F(h) - F(0.5)).astype(F)
        valid = (cw > 0) & (fx >= F(-1.0)) & (fx < F(w)) & (fy >= F(-1.0)) & (fy < F(h))
    return valid, fx, fy


def reproject(rec, sd, history, w, h, normal_min, depth_tol):
    """Steps 1 to 6 of a restart call: (base [H, W, 3], n_b [H, W]). `history` is None or (rgba, length, records, sd)."""
    base = np.zeros((h, w, 3), F)
    n_b = np.zeros((h, w), F)
    if history is None:
        return base, n_b
    hrgba, hlen, hrec, hsd = history
    o = np.asarray(sd["position"], F).reshape(3)
    cam = camera(hsd, w, h)
    hit, kind, key, n, Wp, t, _ = guide_of(rec, o)
    qhit, qkind, qkey, qn, qW, _, _ = guide_of(hrec, cam[1])
    valid, fx, fy = positions(rec, o, cam, w, h)
    fx = np.where(valid, fx, F(0))
    fy = np.where(valid, fy, F(0))
    flx, fly = np.floor(fx), np.floor(fy)
    x0, y0 = flx.astype(np.int64), fly.astype(np.int64)
    ax, ay = (fx - flx).astype(F), (fy - fly).astype(F)
    bx, by = F(1.0) - ax, F(1.0) - ay
    weights = [bx * by, ax * by, bx * ay, ax * ay]
    hc = np.asarray(hrgba, F)[..., :3]
    hl = np.asarray(hlen, F)
    acc = np.zeros((h, w, 3), F)
    nacc = np.zeros((h, w), F)
    ws = np.zeros((h, w), F)
    with np.errstate(all="ignore"):
        tol = (F(depth_tol) * t).astype(F)
        for j, wt in enumerate(weights):
            qx, qy = x0 + (j & 1), y0 + (j >> 1)
            inside = valid & (qx >= 0) & (qx < w) & (qy >= 0) & (qy < h)
            cxq, cyq = np.clip(qx, 0, w - 1), np.clip(qy, 0, h - 1)
            c, ln = hc[cyq, cxq], hl[cyq, cxq]
            take = inside & (ln > 0) & (qkind[cyq, cxq] == kind) & (qkey[cyq, cxq] == key) & np.isfinite(c).all(axis=-1) & (wt > 0)
            nd = _dot(n, qn[cyq, cxq]).astype(F)
            dz = np.abs(_dot(n, (qW[cyq, cxq] - Wp).astype(F))).astype(F)
            take &= ~hit | ((nd >= F(normal_min)) & (dz <= tol))
            acc = np.where(take[..., None], acc + wt[..., None] * np.where(take[..., None], c, F(0)), acc).astype(F)
            nacc = np.where(take, nacc + wt * np.where(take, ln, F(0)), nacc).astype(F)
            ws = np.where(take, ws + wt, ws).astype(F)
        ok = ws > 0
        den = np.where(ok, ws, F(1))
        base = np.where(ok[..., None], acc / den[..., None], F(0)).astype(F)
        n_b = np.where(ok, nacc / den, F(0)).astype(F)
    return base, n_b


def blend(img, base, n_b, frames, max_history):
    """(rgba [H, W, 4], length [H, W]) of every call."""
    cur = np.ascontiguousarray(img, F)
    f = F(frames)
    with np.errstate(all="ignore"):
        tot = (n_b + f).astype(F)
        a = (f / tot).astype(F)
        mixed = (base + ((cur[..., :3] - base).astype(F) * a[..., None]).astype(F)).astype(F)
    out = cur.copy()
    out[..., :3] = np.where((n_b == 0)[..., None], cur[..., :3], mixed)
    return out, np.minimum(tot, F(max_history)).astype(F)


def call(img, frames, rec, sd, restart=True, history=None, state=None, max_history=32, normal_min=0.9, depth_tol=0.05):
    """One call as wcpt.temporal_host makes it: (base, n_b, rgba, length)."""
    h, w = np.asarray(img).shape[:2]
    if restart:
        base, n_b = reproject(rec, sd, history, w, h, normal_min, depth_tol)
    else:
        base, n_b = state
    out, length = blend(img, base, n_b, frames, max_history)
    return base, n_b, out, length
