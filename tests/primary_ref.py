"""CPU reference of the primary-hit buffer (wcpt_trace_primary, wcpt_pick): segment 0 of every pixel, restated so that
it keeps the primitive. Test input, no product code.

- Direction: oracle/pt_oracle.c shade_pixel (:375-391) in numpy float32, one rounding per operation, in the same operand
  order; div3s (v * RN(1 / s)) and normalize3 as that file defines them.
- Hit: the traversal of oracle/pt_f64.py intersect, per ray, with a stack as the reference has it (both children pushed,
  the nearer last; a popped node culled by t0 > t1, t1 < 0 or t0 > rec.t; a leaf's triangles in index order; strict `<`
  everywhere). The arithmetic is the C oracle's own exported functions -- oracle_ray_sphere, oracle_ray_box,
  oracle_child_pair, oracle_ray_triangle, the functions behind oracle.ray_sphere / ray_box / child_pair / ray_triangle,
  called on raw pointers because a frame makes some 10^5 calls. It tracks (prim, draw) and counts node pops, triangle tests,
  sphere tests and hits.
- Normals: pt_oracle.c's expressions (:227-228, :260, :292-293) in float32.

tests/test_primary_ref.py pins this restatement to the C oracle's frames. CPU-cheap only at small frames (70x44)."""
import ctypes as C

import numpy as np

import oracle
import wcpt

T = wcpt._lib
F = np.float32
K_INFINITY = F(3.402823466e38)
MISS, SPHERE, TRIANGLE, FRONT = T.HIT_MISS, T.HIT_SPHERE, T.HIT_TRIANGLE, T.HIT_FRONT
WORDS = 12
COUNTERS = ("segments", "sphere_tests", "node_pops", "interior_visits", "triangle_tests", "hits", "draw_fetches")

_olib = oracle.lib


def _dot3(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def _div3s(v, s):
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        r = F(1.0) / s
        return v * np.asarray(r)[..., None]


def _normalize3(v):
    with np.errstate(invalid="ignore", over="ignore"):
        return _div3s(v, np.sqrt(_dot3(v, v)))


def _cross3(a, b):
    return np.array([a[1] * b[2] - b[1] * a[2], a[2] * b[0] - b[2] * a[0], a[0] * b[1] - b[0] * a[1]], F)


def directions(sd, W, H, xs, ys):
    """pt_oracle.c:375-391 for the pixels (xs[i], ys[i]) of a W x H frame: float32 [n, 3]."""
    xs = np.asarray(xs, np.uint32)
    ys = np.asarray(ys, np.uint32)
    imgW, imgH = F(W), F(H)
    one, half, two = F(1.0), F(0.5), F(2.0)
    cx = xs.astype(F) / imgW
    cy = ys.astype(F) / imgH
    cx = cx + (one / imgW) * half
    cy = cy + (one / imgH) * half
    cy = one - cy
    cx = cx * two - one
    cy = cy * two - one
    P = np.asarray(sd["inverseProjection"], F).reshape(16)
    tg = [((P[0 * 4 + r] * cx + P[1 * 4 + r] * cy) + P[2 * 4 + r] * one) + P[3 * 4 + r] * one for r in range(4)]
    d = _normalize3(_div3s(np.stack(tg[:3], axis=-1), tg[3]))
    V = np.asarray(sd["inverseView"], F).reshape(16)
    wd = [((V[0 * 4 + r] * d[..., 0] + V[1 * 4 + r] * d[..., 1]) + V[2 * 4 + r] * d[..., 2]) + V[3 * 4 + r] * F(0.0)
          for r in range(3)]
    return np.ascontiguousarray(_normalize3(np.stack(wd, axis=-1)), F)


class _Draw:
    def __init__(self, mesh):
        self.pos = np.ascontiguousarray(mesh.positions, F).reshape(-1, 3)
        self.idx = np.ascontiguousarray(mesh.indices, np.uint32)
        self.nodes = np.ascontiguousarray(mesh.nodes, T.NODE_DTYPE)
        self.nodesf = self.nodes.view(F).reshape(-1, 8)          # min(3) max(3) | two u32
        self.left = [int(v) for v in self.nodes["leftNodeOrTriangleIndex"]]
        self.count = [int(v) for v in self.nodes["triangleCount"]]
        self.vtx = [int(v) for v in self.idx]
        self.pp = self.pos.ctypes.data
        self.np_ = self.nodes.ctypes.data


def _closest(o, d, spheres, sph_pos, draws, cnt):
    """Intersect's record for one ray: (t, kind, index, draw)."""
    op, dp = o.ctypes.data, d.ctypes.data
    rec_t, kind, index, draw = K_INFINITY, MISS, 0, 0
    cnt["segments"] += 1
    for i in range(len(spheres)):
        ts = F(_olib.oracle_ray_sphere(op, dp, sph_pos.ctypes.data + 12 * i, F(spheres["radius"][i])))
        cnt["sphere_tests"] += 1
        if ts > 0.0 and ts < rec_t:
            rec_t, kind, index, draw = ts, SPHERE, i, 0
    with np.errstate(divide="ignore"):
        inv = F(1.0) / d
    item = np.zeros(19, F)
    item[0:3] = o
    item[3:6] = inv
    out6 = np.zeros(6, np.uint32)
    t01 = np.zeros(2, F)
    ip, o6p, tp = item.ctypes.data, out6.ctypes.data, t01.ctypes.data
    for di, g in enumerate(draws):
        cnt["draw_fetches"] += 1
        stack = [0]
        while stack:
            node = stack.pop()
            nptr = g.np_ + 32 * node
            _olib.oracle_ray_box(op, dp, nptr, nptr + 12, tp)
            cnt["node_pops"] += 1
            t0, t1 = t01[0], t01[1]
            if t0 > t1 or t1 < 0.0 or t0 > rec_t:
                continue
            count, left = g.count[node], g.left[node]
            if count > 0:
                for k in range(0, count, 3):
                    first = k + left
                    tt = F(_olib.oracle_ray_triangle(op, dp, g.pp + 12 * g.vtx[first], g.pp + 12 * g.vtx[first + 1],
                                                     g.pp + 12 * g.vtx[first + 2]))
                    cnt["triangle_tests"] += 1
                    if tt != -1.0 and tt < rec_t:
                        rec_t, kind, index, draw = tt, TRIANGLE, first // 3, di
            else:
                cnt["interior_visits"] += 1
                item[6:12] = g.nodesf[left, :6]
                item[12:18] = g.nodesf[left + 1, :6]
                _olib.oracle_child_pair(ip, o6p)
                if out6[0]:
                    stack += [left + 1, left]    # left is nearer: pushed last, popped first
                else:
                    stack += [left, left + 1]
    if kind != MISS:
        cnt["hits"] += 1
    return rec_t, kind, index, draw


def _bits(v):
    return np.asarray(v, F).view(np.uint32)


def trace(scene, W, H, sd=None, pixels=None):
    """The records of a W x H frame of `scene` (a wcpt.scene.HostScene): a PRIMARY_HIT_DTYPE array [H, W] and the
    counters' sums. With `pixels` (a list of (x, y)) only those are traced: [n] records."""
    if sd is None:
        sd = scene.scene_data(W, H, max_bounce=0, samples=1, frame=0)
    if pixels is None:
        ys, xs = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
        xs, ys = xs.reshape(-1), ys.reshape(-1)
    else:
        xs, ys = np.array([p[0] for p in pixels]), np.array([p[1] for p in pixels])
    dirs = directions(sd, W, H, xs, ys)
    origin = np.ascontiguousarray(sd["position"], F).reshape(3)
    nsph = int(sd["sphereCount"])
    spheres = np.ascontiguousarray(scene.spheres[:nsph])
    sph_pos = np.ascontiguousarray(spheres["position"], F).reshape(-1, 3) if nsph else np.zeros((1, 3), F)
    draws = [_Draw(m) for m in scene.meshes[: int(sd["drawCommandCount"])]]
    cnt = {k: 0 for k in COUNTERS}
    words = np.zeros((len(xs), WORDS), np.uint32)
    for i in range(len(xs)):
        d = np.ascontiguousarray(dirs[i])
        t, kind, index, draw = _closest(origin, d, spheres, sph_pos, draws, cnt)
        words[i, 0:3] = _bits(d)
        words[i, 3] = _bits(t)
        if kind == MISS:
            continue
        if kind == SPHERE:
            with np.errstate(over="ignore", invalid="ignore"):
                p = origin + t * d                                             # :227
                n = _div3s(p - sph_pos[index], F(spheres["radius"][index]))    # :228
            material = int(spheres["material"][index])
        else:
            g = draws[draw]
            a, b, c = (g.pos[g.vtx[3 * index + j]] for j in range(3))
            with np.errstate(over="ignore", invalid="ignore"):
                n = _normalize3(_cross3(b - a, c - a))                         # :260
            material = 0
        with np.errstate(over="ignore", invalid="ignore"):
            front = bool(_dot3(d, n) < 0.0)                                    # :292
        if not front:
            n = n * F(-1.0)                                                    # :293
        words[i, 4:7] = _bits(n)
        words[i, 7] = kind | (FRONT if front else 0)
        words[i, 8] = material
        words[i, 9] = index
        words[i, 10] = draw
    rec = words.view(T.PRIMARY_HIT_DTYPE).reshape(-1)
    if pixels is None:
        rec = rec.reshape(H, W)
    return rec, cnt


_cache = {}


def reference(key, scene, W, H):
    """trace(scene, W, H), computed once per `key` and left unchanged (shared by the tests of a session)."""
    k = (key, W, H)
    if k not in _cache:
        rec, cnt = trace(scene, W, H)
        rec.setflags(write=False)
        _cache[k] = (rec, cnt)
    return _cache[k]


def kind_of(rec):
    return rec["kind"] & T.HIT_KIND_MASK


def front_of(rec):
    return (rec["kind"] & T.HIT_FRONT) != 0


def synthesize(rec, materials):
    """The image the oracle renders with maxBounceCount 0 at frame 0 from these records (pt_oracle.c:318-323, :332-335,
    :404-410): a hit shows emission * emissionStrength of its material, a miss the sky of direction.y."""
    h, w = rec.shape
    img = np.zeros((h, w, 4), F)
    img[..., 3] = 1.0
    hit = kind_of(rec) != MISS
    em = np.asarray(materials["emission"], F) * np.asarray(materials["emissionStrength"], F)[:, None]
    zero, one = F(0.0), F(1.0)
    lit = (zero + em * one) * one                      # totalLight + emission * transmittance, then / samples
    a = F(0.5) * (rec["direction"][..., 1] + one)
    ia = one - a
    sky = np.stack([F(0.5) * ia + one * a, F(0.7) * ia + one * a, one * ia + one * a], axis=-1)
    sky = (zero + sky * one) * one
    img[..., :3] = np.where(hit[..., None], lit[rec["material"]], sky)
    return img
