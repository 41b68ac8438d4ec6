"""An independent numpy restatement, in binary32, of the reference's bloom.comp and of the Bloom branch of composite.comp
(test infrastructure; not a test module).

Written from the two shaders and from the protocol the project fixes for what they leave open, not from
csrc/wcpt_bloom.h:

* min(x, y) = y < x ? y : x, max(x, y) = x < y ? y : x, clamp(x, lo, hi) = min(max(x, lo), hi) (GLSL's definitions);
* the sampler: linear, clamp to edge, RGB only. For a level of (w, h) texels: px = uv.x * w - 0.5, x0 = floor(px),
  fx = px - x0 (the same in y), the indices x0, x0 + 1, y0, y0 + 1 each clamped to [0, size - 1], and per channel
  (t00 * (1 - fx) + t10 * fx) * (1 - fy) + (t01 * (1 - fx) + t11 * fx) * fy;
* the coordinate of output texel x of a level ow texels wide: float(x) / ow + (1 / ow) * 0.5 (bloom.comp:111-115);
* `existing` (bloom.comp:130, :139) is the destination-sized texel itself;
* the chain: level l of a W x H frame has max(1, W >> (l + 1)) x max(1, H >> (l + 1)) texels, L = the request clipped to
  1 + floor(log2(min(w_0, h_0))), at least 2;
  D[0] = Prefilter(Box13(image)), D[l] = Box13(D[l-1]), U[L-2] = D[L-2] + Tent9(D[L-1]), U[l] = D[l] + Tent9(U[l+1]),
  display = composite(image.rgb + sample(U[0])) with the existing oracle's composite (gamma 1/2.2 + PBR Neutral).

Every numpy operation on float32 arrays is one correctly rounded binary32 operation, so the order of the operations
written here is the order compared.
"""
import math

import numpy as np

import oracle

F = np.float32


def gmin(x, y):
    return np.where(y < x, y, x)


def gmax(x, y):
    return np.where(x < y, y, x)


def gclamp(x, lo, hi):
    return gmin(gmax(x, lo), hi)


def level_sizes(width, height, requested):
    """The levels' (w, h); None where the chain is refused."""
    if not 2 <= requested <= 12:
        return None
    w0, h0 = max(1, width >> 1), max(1, height >> 1)
    n = min(requested, 1 + int(math.floor(math.log2(min(w0, h0)))))
    if n < 2:
        return None
    return [(max(1, width >> (l + 1)), max(1, height >> (l + 1))) for l in range(n)]


def texel_coords(ow, oh):
    """texCoords of every output texel of an (ow, oh) image: (u[1, ow], v[oh, 1])."""
    u = np.arange(ow).astype(F) / F(ow) + (F(1.0) / F(ow)) * F(0.5)
    v = np.arange(oh).astype(F) / F(oh) + (F(1.0) / F(oh)) * F(0.5)
    return u[None, :], v[:, None]


def sample(tex, u, v):
    """textureLod(tex, (u, v)).rgb for tex[h, w, 3] and broadcastable coordinate arrays -> [.., .., 3]."""
    h, w = tex.shape[:2]

    def axis(c, n):
        p = c * F(n) - F(0.5)
        fl = np.floor(p)
        frac = p - fl
        i0 = fl.astype(np.int64)
        return np.clip(i0, 0, n - 1), np.clip(i0 + 1, 0, n - 1), frac

    x0, x1, fx = axis(u, w)
    y0, y1, fy = axis(v, h)
    x0, x1, fx, y0, y1, fy = np.broadcast_arrays(x0, x1, fx, y0, y1, fy)
    fx = fx[..., None]
    fy = fy[..., None]
    t00, t10, t01, t11 = tex[y0, x0], tex[y0, x1], tex[y1, x0], tex[y1, x1]
    one = F(1.0)
    return (t00 * (one - fx) + t10 * fx) * (one - fy) + (t01 * (one - fx) + t11 * fx) * fy


def box13(tex, u, v):
    """DownsampleBox13(tex, lod, uv, 1 / textureSize) (bloom.comp:25-65)."""
    h, w = tex.shape[:2]
    tx = (F(1.0) / F(w)) * F(0.5)
    ty = (F(1.0) / F(h)) * F(0.5)

    def tap(dx, dy):
        return sample(tex, u + tx * F(dx), v + ty * F(dy))

    a = sample(tex, u, v)
    b, c, d, e = tap(-1, -1), tap(-1, 1), tap(1, 1), tap(1, -1)
    f, g, hh = tap(-2, -2), tap(-2, 0), tap(0, 2)
    i, j, k = tap(2, 2), tap(2, 2), tap(2, 0)
    l, m = tap(-2, -2), tap(0, -2)
    r = np.zeros_like(a)
    r = r + (b + c + d + e) * F(0.5)
    r = r + (f + g + a + m) * F(0.125)
    r = r + (g + hh + i + a) * F(0.125)
    r = r + (a + i + j + k) * F(0.125)
    r = r + (m + a + k + l) * F(0.125)
    return r * F(0.25)


def prefilter(color, params):
    """Prefilter + QuadraticThreshold (bloom.comp:69-86); params = (threshold, threshold - knee, knee * 2, 0.25 / knee)."""
    color = gmin(F(20.0), color)
    br = gmax(gmax(color[..., 0], color[..., 1]), color[..., 2])
    rq = gclamp(br - params[1], F(0.0), params[2])
    rq = (rq * rq) * params[3]
    s = gmax(rq, br - params[0]) / gmax(br, F(1.0e-4))
    return color * s[..., None]


def tent9(tex, u, v):
    """UpsampleTent9(tex, lod, uv, 1 / textureSize, 1) (bloom.comp:88-107)."""
    h, w = tex.shape[:2]
    radius = F(1.0)
    tsx, tsy = F(1.0) / F(w), F(1.0) / F(h)
    ox, oy, oz, ow = tsx * F(1.0) * radius, tsy * F(1.0) * radius, tsx * F(-1.0) * radius, tsy * F(0.0) * radius
    r = sample(tex, u, v) * F(4.0)
    r = r + sample(tex, u - ox, v - oy)
    r = r + sample(tex, u - ow, v - oy) * F(2.0)
    r = r + sample(tex, u - oz, v - oy)
    r = r + sample(tex, u + oz, v + ow) * F(2.0)
    r = r + sample(tex, u + ox, v + ow) * F(2.0)
    r = r + sample(tex, u + oz, v + oy)
    r = r + sample(tex, u + ow, v + oy) * F(2.0)
    r = r + sample(tex, u + ox, v + oy)
    return r * (F(1.0) / F(16.0))


def pyramid(img, threshold=1.0, knee=0.1, levels=6):
    """U[0] (the texture composite.comp samples) for a float image [H, W, >= 3], or None where the chain is refused."""
    rgb = np.ascontiguousarray(img, dtype=F)[..., :3]
    height, width = rgb.shape[:2]
    sizes = level_sizes(width, height, levels)
    if sizes is None:
        return None
    threshold, knee = F(threshold), F(knee)
    params = (threshold, threshold - knee, knee * F(2.0), F(0.25) / knee)
    with np.errstate(all="ignore"):
        down = []
        for l, (w, h) in enumerate(sizes):
            u, v = texel_coords(w, h)
            if l == 0:
                down.append(prefilter(box13(rgb, u, v), params))
            else:
                down.append(box13(down[l - 1], u, v))
        up = down[-1]
        for l in range(len(sizes) - 2, -1, -1):
            u, v = texel_coords(*sizes[l])
            up = down[l] + tent9(up, u, v)
    assert up.dtype == F
    return up


def bloom(img, threshold=1.0, knee=0.1, levels=6):
    """(rgba32f, rgba8) of composite.comp with Bloom set, or None where the chain is refused."""
    a = np.ascontiguousarray(img, dtype=F)
    u0 = pyramid(a, threshold, knee, levels)
    if u0 is None:
        return None
    height, width = a.shape[:2]
    u, v = texel_coords(width, height)
    with np.errstate(all="ignore"):
        s = a.copy()
        s[..., :3] = a[..., :3] + sample(u0, u, v)
    return oracle.composite(s)
