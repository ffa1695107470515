"""The yardstick of the ray-query tests (spira_scene_cast_* / spira_scene_occluded_*): the reference's closest-hit scan
hit(world, ray, t_min, t_max) (examples/julia-raytracer.jl:242-258) in Python over the oracle's oracle_hit_sphere_* / oracle_hit_triangle_* — spheres
[0..) then triangles [0..) in the caller's order with a shrinking t_max — on rays prepared by spira_hip.query.normalize_rays, plus the ray sets, the
invalid kinds, the tree frame and the normals restated in numpy.  Argtypes are set and every pointer is built once: a scan is one C call per object."""
import ctypes as C
import functools

import numpy as np

from spira_hip import query, scenes

MISS, INVALID = -1, -3


def dtype_of(prec):
    return np.float32 if prec == "f32" else np.float64


def mesh_frame(triangles10, prec):
    """(centre[3], scale) of the normalised frame a fresh build gives the mesh (spira_bvh.h): the box centre rounded to T, the power of two that
    brings the largest extent into [0.5, 1).  None for a mesh without a tree (at most 32 triangles)."""
    if triangles10 is None or len(triangles10) <= 32:
        return None
    T = dtype_of(prec)
    v = np.asarray(triangles10, dtype=T).astype(np.float64)[:, :9].reshape(-1, 3)
    lo, hi = v.min(axis=0), v.max(axis=0)
    centre = (lo * 0.5 + hi * 0.5).astype(T).astype(np.float64)
    ext = float(np.maximum(hi - centre, centre - lo).max() * 2)
    _, e2 = np.frexp(ext)
    return centre, float(np.ldexp(1.0, -int(e2)))


class Scan:
    """The reference scan over one scene in one precision."""

    def __init__(self, oracle, scene, prec, frame=None):
        """frame: the (centre[3], scale) the validity rule is restated with where it is not a fresh build's of this mesh — after an update the tree keeps
        the frame it was built in, after a rebuild it has the one the device made."""
        self.prec, self.T = prec, dtype_of(prec)
        cdt = C.c_float if prec == "f32" else C.c_double
        lib = oracle.lib()
        suf = "_" + prec
        self._hs, self._ht = getattr(lib, "oracle_hit_sphere" + suf), getattr(lib, "oracle_hit_triangle" + suf)
        for fn in (self._hs, self._ht):
            fn.restype = C.c_int
            fn.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, cdt, cdt, C.c_void_p, C.c_void_p]
        self.sp = np.ascontiguousarray(scene["spheres5"], dtype=self.T).reshape(-1, 5)
        tri = scene.get("triangles10")
        self.tri = np.ascontiguousarray(tri if tri is not None else np.zeros((0, 10)), dtype=self.T).reshape(-1, 10)
        isz = self.T().itemsize
        self._objs = [(self._hs, self.sp.ctypes.data + 5 * isz * i) for i in range(len(self.sp))]
        self._objs += [(self._ht, self.tri.ctypes.data + 10 * isz * i) for i in range(len(self.tri))]
        self.ns = len(self.sp)
        self.frame = frame if frame is not None else mesh_frame(tri, prec)
        self._t = cdt()
        self._n = (cdt * 3)()

    def cast(self, rays8):
        """prim int32 [n], t [n], valid [n], rays (prepared): the contract of spira_scene_cast_* (miss: -1 and t_max copied; invalid: -3 and 0)."""
        rays, valid = query.normalize_rays(rays8, self.T, self.frame)
        rays = np.ascontiguousarray(rays)
        n, isz = len(rays), self.T().itemsize
        prim, t = np.full(n, INVALID, dtype=np.int32), np.zeros(n, dtype=self.T)
        tp, npp = C.addressof(self._t), C.addressof(self._n)
        base = rays.ctypes.data
        for i in range(n):
            if not valid[i]:
                continue
            o, d = base + 8 * isz * i, base + (8 * i + 4) * isz
            t_min, closest, best = float(rays[i, 3]), float(rays[i, 7]), MISS
            for k, (fn, ptr) in enumerate(self._objs):
                if fn(ptr, o, d, t_min, closest, tp, npp):
                    closest, best = self._t.value, k
            prim[i] = best
            t[i] = rays[i, 7] if best < 0 else self.T(closest)
        return prim, t, valid, rays

    def normals(self, rays, prim, t, TN):
        """The library's normal (feature_normal of spira_denoise.h) restated in TN from T-valued inputs: outward normalize(pos - centre) for a sphere, the
        unflipped normalize(cross(e1, e2)) for a triangle (the edges are differences in T), at pos = o + d t; 0 for a miss or an invalid ray."""
        hit = prim >= 0
        is_sph = hit & (prim < self.ns)
        with np.errstate(all="ignore"):
            pos = rays[:, :3].astype(TN) + rays[:, 4:7].astype(TN) * t.astype(TN)[:, None]
            sp = self.sp if len(self.sp) else np.zeros((1, 5), dtype=self.T)
            n_s = _normalize(pos - sp[np.where(is_sph, prim, 0)][:, :3].astype(TN))
            if len(self.tri):
                tr = self.tri[np.where(hit & ~is_sph, prim - self.ns, 0)]
                e1, e2 = (tr[:, 3:6] - tr[:, 0:3]).astype(TN), (tr[:, 6:9] - tr[:, 0:3]).astype(TN)
                n_s = np.where(is_sph[:, None], n_s, _normalize(_cross(e1, e2)))
        return np.where(hit[:, None], n_s, TN(0)).astype(TN)


def _dot(a, b):
    return a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1] + a[..., 2] * b[..., 2]


def _normalize(a):
    return a / np.sqrt(_dot(a, a))[..., None]


def _cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2], a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], axis=-1)


def target_box(scene):
    """(lo, hi, centre, ext) of what the rays aim at: the mesh's box, or — a scene without triangles — the box of its spheres of radius < 10."""
    tri = scene.get("triangles10")
    if tri is not None and len(tri):
        v = np.asarray(tri, dtype=np.float64)[:, :9].reshape(-1, 3)
        lo, hi = v.min(axis=0), v.max(axis=0)
    else:
        s = np.asarray(scene["spheres5"], dtype=np.float64)
        s = s[s[:, 3] < 10]
        lo, hi = (s[:, :3] - s[:, 3:4]).min(axis=0), (s[:, :3] + s[:, 3:4]).max(axis=0)
    return lo, hi, (lo + hi) / 2, float((hi - lo).max())


def _unit(rng, n):
    u = rng.normal(size=(n, 3))
    return u / np.linalg.norm(u, axis=1)[:, None]


def _targets(rng, scene, n):
    lo, hi, c, _ = target_box(scene)
    return c + (rng.random((n, 3)) - 0.5) * (hi - lo) * 1.3


def rays_a(rng, scene, n):
    """From (0, 1, 3) to targets uniform in the box grown by 1.3; t_min 0.001, t_max +Inf."""
    o = np.tile([0.0, 1.0, 3.0], (n, 1))
    return np.concatenate([o, np.full((n, 1), 0.001), _targets(rng, scene, n) - o, np.full((n, 1), np.inf)], axis=1)


def rays_b(rng, scene, n):
    """From c + 1.5 ext u, u random unit vectors, to such targets; the direction scaled by 3.7 so that normalisation matters."""
    _, _, c, ext = target_box(scene)
    o = c + 1.5 * ext * _unit(rng, n)
    return np.concatenate([o, np.full((n, 1), 0.001), 3.7 * (_targets(rng, scene, n) - o), np.full((n, 1), np.inf)], axis=1)


def rays_c(rng, scene, n):
    """From c +- 0.05 ext in random directions (inside a closed mesh); t_min 0."""
    _, _, c, ext = target_box(scene)
    o = c + 0.05 * ext * (2.0 * rng.random((n, 3)) - 1.0)
    return np.concatenate([o, np.zeros((n, 1)), _unit(rng, n), np.full((n, 1), np.inf)], axis=1)


def rays_d(rays, prim, t, ns, T, n=64):
    """For the first n mesh hits (any hits in a scene without triangles) of `rays`: the same ray with t_max = t, with t_max = nextafter(t, 0) and with
    t_min = nextafter(t, +Inf).  rays: as given to the scan (directions NOT normalised); t: the scan's, in T."""
    sel = np.flatnonzero(prim >= ns)[:n]
    r = np.asarray(rays, dtype=np.float64)[sel]
    tt = np.asarray(t, dtype=T)[sel]
    same, below, beyond = r.copy(), r.copy(), r.copy()
    same[:, 7] = tt
    below[:, 7] = np.nextafter(tt, T(0))
    beyond[:, 3] = np.nextafter(tt, T(np.inf))
    return same, below, beyond, sel


def aim_at_triangles(rng, rays, scene):
    """Every second ray of `rays` (the odd ones) redirected, from its own origin, at an interior point of a triangle drawn at random: for scenes whose
    triangles are too sparse for rays_a / rays_b to hit often."""
    tri = np.asarray(scene["triangles10"], dtype=np.float64)
    n = len(rays)
    v = tri[rng.integers(0, len(tri), n), :9].reshape(-1, 3, 3)
    a, b = rng.uniform(0.1, 0.4, (n, 1)), rng.uniform(0.1, 0.4, (n, 1))
    out = np.array(rays, dtype=np.float64)
    out[1::2, 4:7] = (v[:, 0] + a * (v[:, 1] - v[:, 0]) + b * (v[:, 2] - v[:, 0]) - out[:, :3])[1::2]
    return out


def invalid_kinds(T, frame):
    """One ray per invalidity cause of the contract, each otherwise harmless.  frame given: the origin rule's ray too."""
    good = np.array([0.0, 1.0, 3.0, 0.001, 0.0, -0.3, -1.0, np.inf])
    kinds = []
    for k, v in ((0, np.nan), (3, np.nan), (5, np.nan), (7, np.nan), (1, np.inf), (6, -np.inf), (3, -1e-3)):
        r = good.copy(); r[k] = v; kinds.append(r)
    r = good.copy(); r[4:7] = 0.0; kinds.append(r)                                    # s = 0
    r = good.copy(); r[4:7] = [0.0, float(np.finfo(T).max) / 2, float(np.finfo(T).max)]; kinds.append(r)      # s overflows
    r = good.copy(); r[4:7] = [0.0, 0.0, float(np.sqrt(float(np.finfo(T).tiny))) / 4]; kinds.append(r)        # s below the smallest normal
    r = good.copy(); r[3], r[7] = 2.0, 1.0; kinds.append(r)                           # t_max < t_min
    if frame is not None:
        r = good.copy(); r[0] = float(frame[0][0]) + 65.0 / frame[1]; kinds.append(r)      # beyond the origin rule
    return np.array(kinds)


# ------------------------------------------------------------------ the scenes and ray sets of the edge tests (test_cast_edges_cpu.py, test_gpu_cast_edges.py)
# (scale, shift) of the four placements the far-origin rule is tested at: as built, a thousand times larger, far from the origin, and small and far.
FRAMES = ((1.0, (0.0, 0.0, 0.0)), (1e3, (0.0, 0.0, 0.0)), (1.0, (300.0, -200.0, 150.0)), (0.05, (-40.0, 7.0, 90.0)))


@functools.lru_cache(maxsize=None)
def _blob_triangles(level):
    v, f = scenes.bumpy_blob(level)
    v = scenes.transform_vertices(v, scale=(0.5, 0.5, 0.5), rotation=(0.0, 90.0, 0.0), translation=(0.0, 0.0, -1.0), center=True, normalize_size=True)
    t = scenes.mesh_triangles10(v, f, 3)
    t.setflags(write=False)
    return t


def blob_scene(level, scale=1.0, shift=(0.0, 0.0, 0.0)):
    """The objects of scenes.scene_s4(level) — ground sphere, light sphere, the bumpy_blob mesh under scene_s4's transform — without a camera (no native
    library is needed), everything scaled by `scale` and then moved by `shift` together, the spheres' radii included.  At (1, 0): scene_s4's own values."""
    materials8 = np.array([[0.8, 0.8, 0.2, 0, 0, 0, 0.0, 1.0], [0.8, 0.8, 0.8, 4, 4, 4, 0.0, 1.0], [0.7, 0.3, 0.2, 0, 0, 0, 0.2, 0.4]], dtype=np.float64)
    sp = np.array([[0, -100.5, -1, 100, 1], [0, 2, 0, 0.5, 2]], dtype=np.float64)
    tri = np.array(_blob_triangles(level))
    sh = np.asarray(shift, dtype=np.float64)
    if scale != 1.0 or sh.any():
        for v in range(3):
            tri[:, 3 * v:3 * v + 3] = tri[:, 3 * v:3 * v + 3] * scale + sh
        sp[:, :3] = sp[:, :3] * scale + sh
        sp[:, 3] *= scale
    return dict(spheres5=sp, materials8=materials8, triangles10=tri)


def quad_scene():
    """600 axis-aligned triangles, no spheres: 300 little squares of side 0.2 at random places (default_rng(4)), normal axes cycling — many boxes of zero
    extent along one axis.  Triangles 2q and 2q + 1 are the halves of square q: (c, c + u, c + v) and (c + u, c + u + v, c + v)."""
    rng = np.random.default_rng(4)
    quads = []
    for k in range(300):
        c = rng.uniform(-1, 1, 3)
        ax = k % 3
        u, v = np.roll(np.eye(3), ax, axis=1)[0] * 0.2, np.roll(np.eye(3), ax, axis=1)[1] * 0.2
        quads.append(list(c) + list(c + u) + list(c + v) + [1.0])
        quads.append(list(c + u) + list(c + u + v) + list(c + v) + [1.0])
    return dict(spheres5=np.zeros((0, 5)), materials8=np.array([[0.8, 0.8, 0.8, 0, 0, 0, 0.5, 0.0]]), triangles10=np.array(quads))


def duplicate_scene(s, rng):
    """Ties: the triangles of scene `s` and their copies under another material (the next of six), interleaved by a permutation drawn from rng, no
    spheres.  Returns the scene and pair[i], the index of the other triangle with triangle i's vertices."""
    t = np.asarray(s["triangles10"], dtype=np.float64)
    n = len(t)
    dup = t.copy()
    dup[:, 9] = (t[:, 9] % 6) + 1
    order = rng.permutation(2 * n)
    where = np.empty(2 * n, dtype=np.int64)
    where[order] = np.arange(2 * n)                                 # where[j]: the place of row j of [t; dup]
    pair = np.empty(2 * n, dtype=np.int64)
    pair[where[:n]], pair[where[n:]] = where[n:], where[:n]
    return dict(s, spheres5=np.zeros((0, 5)), triangles10=np.concatenate([t, dup])[order]), pair


def _mesh_vertices(scene, T):
    """[nt, 3, 3] the mesh's vertices rounded to T (what the library and the scan hold), as Float64."""
    return np.asarray(scene["triangles10"], dtype=T).astype(np.float64)[:, :9].reshape(-1, 3, 3)


def _box_T(scene, T):
    v = _mesh_vertices(scene, T).reshape(-1, 3)
    lo, hi = v.min(axis=0), v.max(axis=0)
    return lo, hi, float((hi - lo).max())


def rays_far(rng, scan, scene, n, lo=60.0):
    """Valid rays from the edge of the origin rule: o = centre + off / scale in the tree's frame, off uniform in [-64, 64]^3 with one axis (chosen at
    random) forced to +-uniform(lo, 64) and off_y >= 0 (above the ground sphere); the origin rounded to T and widened again, so both sides see the value
    the library sees.  Even rays aim at a vertex of the mesh rounded to T, odd rays at the midpoint of a triangle's edge: the leaf boxes are the
    triangles' own boxes, so an entry point in the wrong place prunes a real hit exactly there.  t_min 0, t_max +Inf, directions not normalised.
    Returns (rays, axis, sign): the forced axis and its side, for rays_far_outside."""
    centre, scale = np.asarray(scan.frame[0], dtype=np.float64), float(scan.frame[1])
    off = rng.uniform(-64.0, 64.0, (n, 3))
    axis, sign = rng.integers(0, 3, n), np.where(rng.random(n) < 0.5, -1.0, 1.0)
    off[np.arange(n), axis] = sign * rng.uniform(lo, 64.0, n)
    off[:, 1] = np.abs(off[:, 1])
    sign = np.where(axis == 1, 1.0, sign)
    o = (centre + off / scale).astype(scan.T).astype(np.float64)
    v = _mesh_vertices(scene, scan.T)
    ti, vi = rng.integers(0, len(v), n), rng.integers(0, 3, n)
    target = np.where((np.arange(n) % 2 == 0)[:, None], v[ti, vi], 0.5 * (v[ti, vi] + v[ti, (vi + 1) % 3]))
    return np.concatenate([o, np.zeros((n, 1)), target - o, np.full((n, 1), np.inf)], axis=1), axis, sign


def rays_far_outside(rays, axis, sign, scan):
    """The invalid twins of rays_far: the forced coordinate moved to the first value of T beyond centre +- 64 / scale that the rule, evaluated in T as the
    library evaluates it, rejects — one ulp beyond the bound where o - centre is exact there, a few where that difference rounds back onto 64."""
    T = scan.T
    c, scale = np.asarray(scan.frame[0], dtype=T), T(scan.frame[1])
    out = np.array(rays, dtype=np.float64)
    for i in range(len(out)):
        k, s = int(axis[i]), T(sign[i])
        x = T(c[k] + s * T(64) / scale)
        for _ in range(64):
            if not abs((x - c[k]) * scale) <= T(64):
                break
            x = np.nextafter(x, s * T(np.inf))
        out[i, k] = float(x)
    return out


def rays_axis(rng, scene, n, T=np.float64, away=None):
    """Axis-parallel rays: direction +-e_k, k cycling, the other two components 0.0 / -0.0 alternating; the line runs through a point uniform in the mesh's
    box.  The first half starts outside the box, 2 extents before the face it enters by (away given: at that distance from the box centre along the axis
    instead); the second half starts inside, 0.01 extents before the point.  t_min 0, t_max +Inf."""
    lo, hi, ext = _box_T(scene, T)
    p = lo + rng.random((n, 3)) * (hi - lo)
    i = np.arange(n)
    k, s = i % 3, np.where((i // 3) % 2 == 0, 1.0, -1.0)
    d = np.where((i[:, None] + np.arange(3)[None, :]) % 2 == 0, 0.0, -0.0)
    d[i, k] = s
    o = p.copy()
    if away is None:
        start = np.where(s > 0, lo[k] - 2.0 * ext, hi[k] + 2.0 * ext)
    else:
        start = 0.5 * (lo[k] + hi[k]) - s * away
    o[i, k] = np.where(i < n // 2, start, p[i, k] - 0.01 * ext * s)
    return np.concatenate([o, np.zeros((n, 1)), d, np.full((n, 1), np.inf)], axis=1)


PLANE_IN, PLANE_INWARD, PLANE_OUTWARD = 0, 1, 2


def rays_on_planes(scene, T):
    """Origins ON the six bounding planes of the mesh: for each axis k and each of the two extreme vertex coordinates of the mesh rounded to T, 8 rays
    whose origin has exactly that k-coordinate, spread over the face — four in the plane along +-e_j, +-e_l from outside the face, one in the plane from
    inside the face, two along e_k into the box and one out of it.  Returns (rays, kind) with kind PLANE_IN / PLANE_INWARD / PLANE_OUTWARD."""
    lo, hi, ext = _box_T(scene, T)
    frac = [(0.5, 0.5), (0.25, 0.75), (0.4, 0.1), (0.9, 0.6), (0.3, 0.3), (0.5, 0.5), (0.7, 0.2), (0.15, 0.85)]
    rays, kind = [], []
    for k in range(3):
        j, l = (k + 1) % 3, (k + 2) % 3
        for side, plane in ((-1.0, lo[k]), (1.0, hi[k])):
            for r, (fj, fl) in enumerate(frac):
                o, d = np.zeros(3), np.array([0.0, -0.0, 0.0])
                o[k], o[j], o[l] = plane, lo[j] + fj * (hi[j] - lo[j]), lo[l] + fl * (hi[l] - lo[l])
                if r < 4:
                    a, s = (j, l)[r // 2], (1.0, -1.0)[r % 2]
                    d[a] = s
                    o[a] = (lo[a] - 0.5 * ext) if s > 0 else (hi[a] + 0.5 * ext)
                    kind.append(PLANE_IN)
                elif r == 4:
                    d[j] = 1.0
                    kind.append(PLANE_IN)
                elif r == 7:
                    d[k] = side
                    kind.append(PLANE_OUTWARD)
                else:
                    d[k] = -side
                    kind.append(PLANE_INWARD)
                rays.append(list(o) + [0.0] + list(d) + [np.inf])
    return np.array(rays), np.array(kind)


def rays_quads(rng, quads, T, n):
    """Against quad_scene's triangles.  n rays along a square's normal axis from 3 units away, direction of length 2.5 with a signed zero in the other two
    components, at one of three points of a triangle picked at random: an interior point, the midpoint of its square's diagonal (u + v == 1 for the
    square's first triangle: the edge both halves share) and its corner v0.  Then n rays lying IN a square's plane: the origin has the plane's coordinate
    exactly and lies 0.5 before an interior point of the square, the direction is +-e along one of the square's two in-plane axes.
    Returns rays [2 n, 8]; the first n are the normal-axis ones."""
    v = np.asarray(quads, dtype=T).astype(np.float64)[:, :9].reshape(-1, 3, 3)
    out = []
    for part in range(2):
        ti = rng.integers(0, len(v), n)
        what, sgn = rng.integers(0, 3, n), np.where(rng.random(n) < 0.5, -1.0, 1.0)
        a, b = rng.uniform(0.1, 0.4, n), rng.uniform(0.1, 0.4, n)
        for i in range(n):
            t, q = v[ti[i]], ti[i] // 2
            ax = q % 3                                            # u along e_ax, v along e_(ax + 1), the normal along e_(ax + 2)
            nrm = (ax + 2) % 3
            inner = t[0] + a[i] * (t[1] - t[0]) + b[i] * (t[2] - t[0])
            d = np.array([0.0, 0.0, 0.0])
            if part == 0:
                p = (inner, 0.5 * (v[2 * q][1] + v[2 * q][2]), t[0])[what[i]]
                o = p.copy()
                o[nrm] = p[nrm] + 3.0 * sgn[i]
                d[(nrm + 1) % 3], d[(nrm + 2) % 3] = (0.0, -0.0) if i % 2 == 0 else (-0.0, 0.0)
                d[nrm] = -2.5 * sgn[i]
            else:
                along = (ax, (ax + 1) % 3)[what[i] % 2]
                o = inner.copy()
                o[nrm] = t[0][nrm]
                o[along] -= 0.5 * sgn[i]
                d[nrm] = -0.0 if i % 2 else 0.0
                d[along] = sgn[i]
            out.append(list(o) + [0.0] + list(d) + [np.inf])
    return np.array(out)


def rays_windows(rays, prim, t, scan, n):
    """For the first n mesh hits of `rays` (as given to the scan; prim, t: the scan's): rays_d's triple — t_max = t, t_max one ulp below, t_min one ulp
    beyond — and three more windows: `before` t_max = 0.5 (|o - box centre| - ext), which ends before the mesh's box; `hit` t_min = t_max = t, the hit
    itself; `behind` t_min = |o - box centre| + 2 ext, which starts behind the mesh.  Returns (same, below, beyond, before, hit, behind, sel)."""
    same, below, beyond, sel = rays_d(rays, prim, t, scan.ns, scan.T, n)
    vv = scan.tri.astype(np.float64)[:, :9].reshape(-1, 3)
    lo, hi = vv.min(axis=0), vv.max(axis=0)
    ext = float((hi - lo).max())
    dist = np.linalg.norm(same[:, :3] - (lo + hi) / 2, axis=1)
    before, hit, behind = same.copy(), same.copy(), same.copy()
    before[:, 7] = np.maximum(0.5 * (dist - ext), 0.0)
    hit[:, 3] = hit[:, 7]
    behind[:, 3], behind[:, 7] = dist + 2.0 * ext, np.inf
    return same, below, beyond, before, hit, behind, sel


# ------------------------------------------------------------------ the sets themselves with the scan's answers: built once per process, left unchanged,
# shared by test_cast_edges_cpu.py (which asserts what they reach) and test_gpu_cast_edges.py (which runs them on the device)
N_FAR, N_WIN, N_AXIS, N_QUADS, N_TIES = 256, 64, 192, 300, 128


def _oracle():
    import oracle_py
    oracle_py.lib()
    return oracle_py


def _freeze(d):
    for a in d.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return d


def scanned(sc, rays, **more):
    """`rays` with the scan's answers, read-only: dict(sc, rays, prim, t, valid, prepared)."""
    prim, t, valid, prepared = sc.cast(rays)
    return _freeze(dict(more, sc=sc, rays=rays, prim=prim, t=t, valid=valid, prepared=prepared))


def far_rays_in(sc, scene, seed=7, n=N_FAR, n_win=N_WIN):
    """rays_far in the scan's frame, the six windows of its first n_win mesh hits and the invalid twins, each scanned: a dict of parts."""
    rays, axis, sign = rays_far(np.random.default_rng(seed), sc, scene, n)
    far = scanned(sc, rays)
    *wins, sel = rays_windows(rays, far["prim"], far["t"], sc, n_win)
    out = dict(far=far, sel=sel, twins=scanned(sc, rays_far_outside(rays, axis, sign, sc)))
    for name, w in zip(("same", "below", "beyond", "before", "hit", "behind"), wins):
        out[name] = scanned(sc, w)
    return out


def join(parts):
    """Several scanned parts as one set for a device comparison: dict(rays, prim, t, prepared)."""
    return _freeze({k: np.concatenate([p[k] for p in parts]) for k in ("rays", "prim", "t", "prepared")})


def far_joined(fs):
    """The far rays and their invalid twins interleaved (ray, twin, ray, twin, ...), then the six windows."""
    a, b = fs["far"], fs["twins"]
    head = {k: np.stack([a[k], b[k]], axis=1).reshape((-1,) + a[k].shape[1:]) for k in ("rays", "prim", "t", "prepared")}
    return join([head] + [fs[k] for k in ("same", "below", "beyond", "before", "hit", "behind")])


@functools.lru_cache(maxsize=None)
def far_set(prec, fi):
    scene = blob_scene(2, *FRAMES[fi])
    sc = Scan(_oracle(), scene, prec)
    return dict(far_rays_in(sc, scene), scene=scene, sc=sc)


@functools.lru_cache(maxsize=None)
def axis_set(prec, level=2):
    scene = blob_scene(level)
    sc = Scan(_oracle(), scene, prec)
    planes, kind = rays_on_planes(scene, sc.T)
    return dict(scene=scene, sc=sc, axis=scanned(sc, rays_axis(np.random.default_rng(11), scene, N_AXIS, sc.T)), planes=scanned(sc, planes), kind=kind)


@functools.lru_cache(maxsize=None)
def quad_set(prec):
    scene = quad_scene()
    sc = Scan(_oracle(), scene, prec)
    away = 60.0 / sc.frame[1]
    return dict(scene=scene, sc=sc, quads=scanned(sc, rays_quads(np.random.default_rng(8), scene["triangles10"], sc.T, N_QUADS)),
                axis_far=scanned(sc, rays_axis(np.random.default_rng(12), scene, N_AXIS, sc.T, away=away)))


@functools.lru_cache(maxsize=None)
def ties_set(prec):
    from test_gpu_parity import random_scene
    rng = np.random.default_rng(9)
    scene, pair = duplicate_scene(random_scene(rng, 0, 100, n_mats=6), rng)
    sc = Scan(_oracle(), scene, prec)
    # rays_a alone hits these sparse triangles with 28 rays of 128: every second ray is aimed at an interior point of a triangle drawn at random instead
    rays = aim_at_triangles(rng, rays_a(rng, scene, N_TIES), scene)
    return dict(scene=scene, sc=sc, pair=pair, rays=scanned(sc, rays))
