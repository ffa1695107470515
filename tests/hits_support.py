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


def shells_scene(level, n_shells=10, max_tris=None, scale=1.0, shift=(0.0, 0.0, 0.0)):
    """Nested shells: n_shells concentric copies of blob_scene(level)'s mesh about its box centre at scales 1.0, 0.9, ... and its two spheres; a ray
    through the centre has about 2 n_shells triangle candidates.  max_tris: the triangles taken round-robin from the shells and cut to that many (<= 32:
    they stay in LDS).  scale, shift: blob_scene's placement of everything (cast_support.FRAMES)."""
    b = S.blob_scene(level, scale, shift)
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


# ------------------------------------------------------------------ the sets of the edge tests (test_hits_edges_cpu.py, test_gpu_hits_edges.py): built once
# per process, left unchanged, shared by the module that asserts what they reach and the module that runs them on the device
N_SHELLS_FAR = 96
DUP_SEED, N_DUP = 43, 96


def totals(ref):
    """Candidates per ray, -1 for an invalid ray."""
    return np.array([-1 if c is None else len(c) for c in ref["cands"]])


def straddles(cands, K):
    """The rays whose candidates at slots K - 1 and K have bit-equal t: a list of K is cut between two candidates that only their index tells apart."""
    return sum(1 for c in cands if c is not None and len(c) > K and c[K - 1][0] == c[K][0])


def interleave(a, b):
    """a[0], b[0], a[1], b[1], ..."""
    return np.stack([a, b], axis=1).reshape((-1,) + a.shape[1:])


@functools.lru_cache(maxsize=None)
def nan_rays(n, prec):
    r = np.full((n, 8), np.nan, dtype=S.dtype_of(prec))
    r.setflags(write=False)
    return r


def poison(h, n, K, inplace=False):
    """The host form stages [rays | t | prim | count] in a workspace that outlives the call: after a call with the same n and K it holds that call's
    answers, and a slot the next call never stores would go unnoticed.  n invalid rays (NaN) with the same K through the same organisation leave
    -3 / 0 / 0 in every staged slot first.  K = 0 (count only): through a K = 1 call of the same n."""
    prim, t, count = h.cast_hits(nan_rays(n, h.prec), max(int(K), 1), inplace=inplace)
    for e in (0, -1):
        assert (prim[e] == INVALID).all() and not t[e].any() and count[e] == 0


@functools.lru_cache(maxsize=None)
def far_ref(prec, fi):
    """cast_support.far_set(prec, fi) as far_joined lays it out — 256 far rays interleaved with their invalid twins, then the six t windows of the first
    64 mesh hits — under the multi-hit yardstick."""
    fs = S.far_set(prec, fi)
    return reference(fs["scene"], prec, S.far_joined(fs)["rays"])


@functools.lru_cache(maxsize=None)
def shells_far_ref(prec, fi):
    """Long lists at far origins: the ten nested shells (800 triangles) in placement FRAMES[fi], 96 rays from 60 .. 64 normalised units away — the odd ones
    re-aimed near the centre, through every shell — interleaved with their invalid twins."""
    scene = shells_scene(1, n_shells=10, scale=S.FRAMES[fi][0], shift=S.FRAMES[fi][1])
    sc = S.Scan(_oracle(), scene, prec)
    rng = np.random.default_rng(29 + fi)
    rays, axis, sign = S.rays_far(rng, sc, scene, N_SHELLS_FAR)
    lo, hi, c, ext = S.target_box(scene)
    rays[1::2, 4:7] = (c + 0.1 * ext * (rng.random((N_SHELLS_FAR, 3)) - 0.5))[1::2] - rays[1::2, :3]
    return dict(reference(scene, prec, interleave(rays, S.rays_far_outside(rays, axis, sign, sc))), scene=scene)


@functools.lru_cache(maxsize=None)
def axis_ref(prec):
    """cast_support.axis_set(prec, 3), parts axis and planes: signed-zero directions, origins on the root box's planes."""
    a = S.axis_set(prec, 3)
    return dict(reference(a["scene"], prec, S.join([a["axis"], a["planes"]])["rays"]), scene=a["scene"])


@functools.lru_cache(maxsize=None)
def quad_ref(prec):
    """cast_support.quad_set(prec), parts quads and axis_far: leaf boxes of zero extent, rays in their planes, axis rays from 60 units away."""
    q = S.quad_set(prec)
    return dict(reference(q["scene"], prec, S.join([q["quads"], q["axis_far"]])["rays"]), scene=q["scene"])


@functools.lru_cache(maxsize=None)
def dup_ref(prec):
    """Ties at every slot: nearest_support's `dup` scene — blob level 3 with every triangle twice, no spheres — so that candidates come in pairs of
    bit-equal t.  pair[i]: the other triangle with triangle i's vertices (duplicate_scene's own, drawn again from the same seed)."""
    import nearest_support as N
    scene = N.scene("dup")
    twin, pair = S.duplicate_scene(S.blob_scene(3), np.random.default_rng(21))
    assert np.array_equal(twin["triangles10"], scene["triangles10"])
    rng = np.random.default_rng(DUP_SEED)
    rays = S.aim_at_triangles(rng, S.rays_b(rng, scene, N_DUP), scene)
    pair.setflags(write=False)
    return dict(reference(scene, prec, rays), scene=scene, pair=pair)


def pairs_hold(ref):
    """Every ray's candidates are whole pairs: entries 2m and 2m + 1 have bit-equal t and are (later index, earlier index) of one duplicated triangle."""
    pair = ref["pair"]
    for c in ref["cands"]:
        if c is None or len(c) % 2:
            return False
        for m in range(0, len(c), 2):
            if not (c[m][0] == c[m + 1][0] and c[m][1] > c[m + 1][1] and pair[c[m][1]] == c[m + 1][1]):
                return False
    return True
