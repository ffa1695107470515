"""The yardstick of the ray-query tests (spira_scene_cast_* / spira_scene_occluded_*): the reference's closest-hit scan
hit(world, ray, t_min, t_max) (examples/julia-raytracer.jl:242-258) in Python over the oracle's oracle_hit_sphere_* / oracle_hit_triangle_* — spheres
[0..) then triangles [0..) in the caller's order with a shrinking t_max — on rays prepared by spira_hip.query.normalize_rays, plus the ray sets, the
invalid kinds, the tree frame and the normals restated in numpy.  Argtypes are set and every pointer is built once: a scan is one C call per object."""
import ctypes as C

import numpy as np

from spira_hip import query

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

    def __init__(self, oracle, scene, prec):
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
        self.frame = mesh_frame(tri, prec)
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
