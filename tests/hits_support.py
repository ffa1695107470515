"""The yardstick of the multi-hit tests (spira_scene_cast_hits_*): for each valid ray the oracle's oracle_hit_sphere_* / oracle_hit_triangle_* called on
EVERY object with the ray's own t_min and t_max (cast_support.Scan's functions and pointers, imported and not edited), the accepted (t, k) sorted by
(t ascending, k descending), cut to K, and all of them counted.  Plus the nested-shells scene: concentric copies of cast_support.blob_scene's mesh."""
import ctypes as C
import functools

import numpy as np

import cast_support as S
from spira_hip import query

MISS, INVALID = S.MISS, S.INVALID


def candidates(sc, rays8):
    """Per ray the sorted list of (t, k) of all candidates (None for an invalid ray), valid [n] and the prepared rays.  sc: a cast_support.Scan."""
    rays, valid = query.normalize_rays(rays8, sc.T, sc.frame)
    rays = np.ascontiguousarray(rays)
    isz = sc.T().itemsize
    tp, npp = C.addressof(sc._t), C.addressof(sc._n)
    base = rays.ctypes.data
    out = []
    for i in range(len(rays)):
        if not valid[i]:
            out.append(None)
            continue
        o, d = base + 8 * isz * i, base + (8 * i + 4) * isz
        t_min, t_max = float(rays[i, 3]), float(rays[i, 7])
        got = []
        for k, (fn, ptr) in enumerate(sc._objs):
            if fn(ptr, o, d, t_min, t_max, tp, npp):
                got.append((sc.T(sc._t.value), k))
        got.sort(key=lambda e: (e[0], -e[1]))
        out.append(got)
    return out, valid, rays


def cut(cands, rays, T, K):
    """The contract's outputs from candidates(): prim int32 [n, K], t [n, K], count [n] (slots filled), total [n] (all candidates)."""
    n = len(cands)
    prim, t = np.full((n, K), INVALID, dtype=np.int32), np.zeros((n, K), dtype=T)
    count, total = np.zeros(n, dtype=np.uint32), np.zeros(n, dtype=np.uint32)
    for i, c in enumerate(cands):
        if c is None:
            continue
        prim[i], t[i] = MISS, rays[i, 7]
        for j, (tt, k) in enumerate(c[:K]):
            prim[i, j], t[i, j] = k, tt
        count[i], total[i] = min(len(c), K), len(c)
    return prim, t, count, total


def shells_scene(level, n_shells=10, max_tris=None):
    """Nested shells: n_shells concentric copies of blob_scene(level)'s mesh about its box centre at scales 1.0, 0.9, ... and its two spheres; a ray
    through the centre has about 2 n_shells triangle candidates.  max_tris: the triangles taken round-robin from the shells and cut to that many (<= 32:
    they stay in LDS)."""
    b = S.blob_scene(level)
    tri = np.asarray(b["triangles10"], dtype=np.float64)
    v = tri[:, :9].reshape(-1, 3)
    c = (v.min(axis=0) + v.max(axis=0)) / 2
    parts = []
    for s in range(n_shells):
        k = 1.0 - 0.1 * s
        p = tri.copy()
        for j in range(3):
            p[:, 3 * j:3 * j + 3] = c + (p[:, 3 * j:3 * j + 3] - c) * k
        parts.append(p)
    if max_tris is None:
        all_t = np.concatenate(parts)
    else:
        all_t = np.stack(parts, axis=1).reshape(-1, 10)[:max_tris]      # triangle 0 of every shell, then triangle 1, ...
    return dict(b, triangles10=all_t)


def rays_through(rng, scene, n):
    """Rays for a shells scene: a third from outside through a point near the centre (many candidates), a third from the centre outwards (t_min 0), a third
    cast_support.rays_b (some miss everything); t_max +Inf except every fifth ray, cut to 1.2 extents."""
    lo, hi, c, ext = S.target_box(scene)
    k = n // 3
    o = c + 1.5 * ext * S._unit(rng, k)
    a = np.concatenate([o, np.full((k, 1), 0.001), (c + 0.1 * ext * (rng.random((k, 3)) - 0.5)) - o, np.full((k, 1), np.inf)], axis=1)
    b = np.concatenate([c + 0.02 * ext * (rng.random((k, 3)) - 0.5), np.zeros((k, 1)), S._unit(rng, k), np.full((k, 1), np.inf)], axis=1)
    r = np.concatenate([a, b, S.rays_b(rng, scene, n - 2 * k)])
    r[::5, 7] = 1.2 * ext
    return r


@functools.lru_cache(maxsize=None)
def _oracle():
    import oracle_py
    oracle_py.lib()
    return oracle_py


def reference(scene, prec, rays, frame=None):
    """dict(sc, rays, cands, valid, prepared), computed once by the caller and left unchanged."""
    sc = S.Scan(_oracle(), scene, prec, frame)
    cands, valid, prepared = candidates(sc, rays)
    rays = np.array(rays)
    rays.setflags(write=False); prepared.setflags(write=False); valid.setflags(write=False)
    return dict(sc=sc, rays=rays, cands=cands, valid=valid, prepared=prepared)


def warp(tri, amp=0.3):
    """A moved mesh for the update / rebuild cases: a twist about the vertical axis through the mesh's middle plus a sine displacement of amp x the
    extent (the deformation tests/test_gpu_refit.py moves its meshes by); the material column is kept."""
    t = np.array(tri, dtype=np.float64)
    v = t[:, :9].reshape(-1, 3)
    lo, hi = v.min(axis=0), v.max(axis=0)
    c, ext = (lo + hi) / 2.0, float((hi - lo).max())
    x, y, z = (v - c).T
    ang = 5.0 * y / ext
    out = np.stack([np.cos(ang) * x - np.sin(ang) * z + amp * ext * np.sin(5.0 * y / ext), y + 0.1 * ext * np.sin(7.0 * x / ext), np.sin(ang) * x + np.cos(ang) * z], axis=1) + c
    t[:, :9] = out.reshape(-1, 9)
    return t


def device_frame(binding, h):
    """(centre[3], scale) of the tree a handle holds on the device (spira_debug_scene_tree): after a rebuild the frame is the one the device made."""
    fn = binding.lib().spira_debug_scene_tree
    fn.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64)]
    fn.restype = C.c_int
    buf, need = np.zeros(1024, dtype=np.uint8), C.c_uint64()
    assert fn(h._h, 0, buf.ctypes.data_as(C.c_void_p), buf.nbytes, C.byref(need)) == 0
    f = buf[16:48].view(np.float64)
    return f[:3].copy(), float(f[3])
