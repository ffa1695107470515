"""GPU: spira_scene_cast_* / spira_scene_occluded_* (spira_query.h: k_cast, k_cast_session) against the reference's closest-hit scan restated over the
oracle's hit functions (tests/cast_support.py).  The leaf test is the scan's own arithmetic and the tree only prunes, so prim and t are compared with
numpy.array_equal in both precisions, for the refilled sessions and for SPIRA_CAST_INPLACE; normals as tests/test_gpu_denoise.py compares them (bit for
bit in Float64, within 4 x the Float32 restatement's own distance from the Float64 one in Float32).

The ray set R (default_rng(5), scene_s4(level=3): 2 spheres, 1 280 triangles, a tree of 4 levels), c = the mesh's box centre, ext its largest dimension:
  (a) 128 rays from (0, 1, 3) to targets uniform in the mesh box grown by 1.3, t_min 0.001, t_max +Inf
  (b) 128 rays from c + 1.5 ext u (u random unit vectors) to such targets, the direction scaled by 3.7
  (c) 64 rays from c +- 0.05 ext in random directions, t_min 0
  (d) for the first 64 mesh hits of (a)-(c) the same ray with t_max = t (the same hit), with t_max = nextafter(t, 0) (a miss) and with
      t_min = nextafter(t, +Inf) (the next object along the ray)"""
import ctypes as C
import functools

import numpy as np
import pytest

import cast_support as S
from spira_hip import query, scenes

pytestmark = pytest.mark.gpu

NA, NB, NC, ND = 128, 128, 64, 64


def _mesh_only(level):
    s = scenes.scene_s4(level=level)
    return dict(s, spheres5=np.zeros((0, 5)))


SCENES = {"s4_3": lambda: scenes.scene_s4(level=3), "s4_4": lambda: scenes.scene_s4(level=4), "s1": scenes.scene_s1, "s2": scenes.scene_s2,
          "mesh_only": lambda: _mesh_only(3)}


@functools.lru_cache(maxsize=None)
def _scene(name):
    return SCENES[name]()


@functools.lru_cache(maxsize=None)
def _scan(name, prec):
    import oracle_py
    oracle_py.lib()
    return S.Scan(oracle_py, _scene(name), prec)


@functools.lru_cache(maxsize=None)
def _reference(name, prec, na=NA, nb=NB, nc=NC, nd=ND):
    """The ray set on a scene and the scan's answers, computed once and left unchanged: dict(rays, prim, t, valid, prepared, parts)."""
    sc, T = _scan(name, prec), S.dtype_of(prec)
    rng = np.random.default_rng(5)
    s = _scene(name)
    abc = np.concatenate([S.rays_a(rng, s, na), S.rays_b(rng, s, nb), S.rays_c(rng, s, nc)])
    prim, t, _, _ = sc.cast(abc)
    ns = sc.ns if len(sc.tri) else 0
    same, below, beyond, sel = S.rays_d(abc, prim, t, ns, T, nd)
    rays = np.concatenate([abc, same, below, beyond])
    prim, t, valid, prepared = sc.cast(rays)
    assert valid.all()
    out = dict(rays=rays, prim=prim, t=t, valid=valid, prepared=prepared, sel=sel, n_abc=len(abc), n_d=len(sel))
    for a in (rays, prim, t, prepared):
        a.setflags(write=False)
    return out


def _handle(gpu, name, prec):
    s = _scene(name)
    return gpu.Scene(s["spheres5"] if len(s["spheres5"]) else None, s["materials8"], s["triangles10"], prec)


def _check_against(h, sc, ref, rays=None, prim=None, t=None, prepared=None, inplace=(False, True), normals=True):
    """One handle against the scan: prim and t array_equal for both organisations, occluded == (prim >= 0), the normals' criterion."""
    T = sc.T
    rays = ref["rays"] if rays is None else rays
    prim = ref["prim"] if prim is None else prim
    t = ref["t"] if t is None else t
    prepared = ref["prepared"] if prepared is None else prepared
    for ip in inplace:
        g_prim, g_t, g_n = h.cast(rays, want_normal=True, inplace=ip)
        bad = np.flatnonzero((g_prim != prim) | (g_t.view(np.uint32 if T == np.float32 else np.uint64) != t.view(np.uint32 if T == np.float32 else np.uint64)))
        assert np.array_equal(g_prim, prim) and np.array_equal(g_t, t), (ip, bad[:8], g_prim[bad[:8]], prim[bad[:8]], g_t[bad[:8]], t[bad[:8]])
        occ = h.occluded(rays, inplace=ip)
        want_occ = np.where(prim == S.INVALID, 255, prim >= 0).astype(np.uint8)
        assert np.array_equal(occ, want_occ), (ip, np.flatnonzero(occ != want_occ)[:8])
        if normals:
            e_n = sc.normals(prepared, prim, t, T)
            if T == np.float64:
                assert np.array_equal(g_n, e_n), ip
            else:
                n64 = sc.normals(prepared, prim, t, np.float64)
                floor = float(np.abs(e_n.astype(np.float64) - n64).max())
                err = float(np.abs(g_n.astype(np.float64) - n64).max())
                print("normal floor: restatement f32 vs f64 %.3e, gpu f32 vs f64 %.3e, bitwise equal to the f32 restatement: %s" % (floor, err, bool(np.array_equal(g_n, e_n))))
                assert floor > 0 and err <= 4 * floor, ip
            assert not g_n[prim < 0].any()


def test_the_ray_set_covers_what_it_is_for():
    """Asserted from the scan's answers alone, before any device result is looked at."""
    counts = {}
    for prec in ("f32", "f64"):
        ref, sc = _reference("s4_3", prec), _scan("s4_3", prec)
        prim, t = ref["prim"], ref["t"]
        mesh = prim >= sc.ns
        a, b, c = mesh[:NA], mesh[NA:NA + NB], mesh[NA + NB:NA + NB + NC]
        b_miss = int((prim[NA:NA + NB] < 0).sum())
        print(prec, "mesh hits of (a), (b), (c):", int(a.sum()), int(b.sum()), int(c.sum()), "misses of (b):", b_miss)
        assert 4 * a.sum() >= NA and 4 * b.sum() >= NB and 10 * b_miss >= NB and c.all()
        assert ref["n_d"] == ND
        k = ref["n_abc"]
        sel = ref["sel"]
        same, below, beyond = slice(k, k + ND), slice(k + ND, k + 2 * ND), slice(k + 2 * ND, k + 3 * ND)
        assert np.array_equal(prim[same], prim[sel]) and np.array_equal(t[same], t[sel])            # a hit at exactly t_max counts
        assert (prim[below] == S.MISS).all() and np.array_equal(t[below], ref["rays"][below, 7].astype(sc.T))
        assert (prim[beyond] != prim[sel]).all() and (prim[beyond] >= 0).sum() >= ND // 2 and (t[beyond][prim[beyond] >= 0] > t[sel][prim[beyond] >= 0]).all()
        counts[prec] = (int(a.sum()), int(b.sum()), int(c.sum()), b_miss)
    assert counts["f32"] == counts["f64"]


def _device_frame(gpu, h):
    fn = gpu.lib().spira_debug_scene_tree
    fn.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64)]
    fn.restype = C.c_int
    buf, need = np.zeros(1024, dtype=np.uint8), C.c_uint64()
    assert fn(h._h, 0, buf.ctypes.data_as(C.c_void_p), buf.nbytes, C.byref(need)) == 0
    f = buf[16:48].view(np.float64)
    return f[:3].copy(), float(f[3])


@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_r_against_the_oracle(gpu, prec):
    ref, sc = _reference("s4_3", prec), _scan("s4_3", prec)
    with _handle(gpu, "s4_3", prec) as h:
        centre, scale = _device_frame(gpu, h)
        assert np.array_equal(centre, sc.frame[0]) and scale == sc.frame[1]      # the frame the validity rule is restated with is the tree's
        _check_against(h, sc, ref)


@pytest.mark.parametrize("name,prec", [("s1", "f32"), ("s1", "f64"), ("s2", "f32"), ("s2", "f64"), ("s4_4", "f32"), ("mesh_only", "f32"), ("mesh_only", "f64")])
def test_other_scene_shapes(gpu, name, prec):
    """Spheres only, LDS triangles, one more tree level, and the mesh alone where a scene without spheres can be created."""
    ref, sc = _reference(name, prec, 48, 48, 24, 24), _scan(name, prec)
    assert (ref["prim"] >= 0).sum() >= 24 and (ref["prim"] < 0).sum() >= 12
    if name in ("s2", "s4_4", "mesh_only"):
        assert (ref["prim"] >= sc.ns).sum() >= 12
    if name == "s4_4":
        assert len(sc.tri) == 5120
    with _handle(gpu, name, prec) as h:
        _check_against(h, sc, ref)


@pytest.mark.parametrize("prec", ["f32", "f64"])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 129])
def test_ragged_sizes(gpu, prec, n):
    ref, sc = _reference("s4_3", prec), _scan("s4_3", prec)
    pick = np.arange(n) * 3 % len(ref["rays"])                 # rays of every kind
    with _handle(gpu, "s4_3", prec) as h:
        _check_against(h, sc, ref, ref["rays"][pick], ref["prim"][pick], ref["t"][pick], ref["prepared"][pick])


N_REFILL = 20011


@functools.lru_cache(maxsize=None)
def _refill_rays():
    return S.rays_b(np.random.default_rng(6), _scene("s4_4"), N_REFILL)


@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_refills(gpu, prec):
    """20 011 incoherent rays on the 5 120-triangle scene: every wave of the session kernel owns more rays than it has lanes, so it refills."""
    plan = gpu.cast_plan(N_REFILL, 256)
    assert plan["base"] > 64 and plan["waves"] > 4 and plan["base"] * plan["waves"] + plan["rem"] == N_REFILL
    rays, sc = _refill_rays(), _scan("s4_4", prec)
    with _handle(gpu, "s4_4", prec) as h:
        d_prim, d_t, d_n = h.cast(rays, want_normal=True)
        i_prim, i_t, i_n = h.cast(rays, want_normal=True, inplace=True)
        assert np.array_equal(d_prim, i_prim) and np.array_equal(d_t, i_t) and np.array_equal(d_n, i_n)
        d_occ, i_occ = h.occluded(rays), h.occluded(rays, inplace=True)
        assert np.array_equal(d_occ, i_occ) and np.array_equal(d_occ, (d_prim >= 0).astype(np.uint8))
    assert (d_prim >= sc.ns).sum() > N_REFILL // 4 and (d_prim < 0).sum() > N_REFILL // 10
    sub = np.arange(256) * 78 + 5                               # a fixed subsample across the whole list
    prim, t, valid, _ = sc.cast(rays[sub])
    assert valid.all() and np.array_equal(d_prim[sub], prim) and np.array_equal(d_t[sub], t)


@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_invalid_rays_interleaved(gpu, prec):
    ref, sc = _reference("s4_3", prec), _scan("s4_3", prec)
    kinds = S.invalid_kinds(sc.T, sc.frame)
    rays = np.array(ref["rays"])
    at = np.arange(0, len(rays), 7)
    rays[at] = kinds[np.arange(len(at)) % len(kinds)]
    assert len(at) >= 2 * len(kinds)
    _, valid = query.normalize_rays(rays, sc.T, sc.frame)
    assert not valid[at].any() and valid.sum() == len(rays) - len(at)
    prim, t, prepared = np.array(ref["prim"]), np.array(ref["t"]), np.array(ref["prepared"])
    prim[at], t[at] = S.INVALID, 0
    with _handle(gpu, "s4_3", prec) as h:
        _check_against(h, sc, ref, rays, prim, t, prepared)
        g_prim, g_t, g_n = h.cast(rays, want_normal=True)
        assert (g_prim[at] == -3).all() and not g_t[at].any() and not g_n[at].any() and (h.occluded(rays)[at] == 255).all()


@functools.lru_cache(maxsize=None)
def _deformed(prec):
    from test_gpu_refit import deform
    A = _scene("s4_3")
    B = dict(A, triangles10=deform(A["triangles10"]))
    import oracle_py
    sc = S.Scan(oracle_py, B, prec)
    rays = np.array(_reference("s4_3", prec)["rays"][:NA + NB + NC])
    prim, t, valid, prepared = sc.cast(rays)
    assert valid.all()
    return B, sc, rays, prim, t


@pytest.mark.parametrize("how", ["update", "rebuild"])
@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_after_an_update_and_after_a_rebuild(gpu, prec, how):
    """The new tree on one stream, the cast on another, no host synchronisation in between; host and device forms give the same bytes."""
    import torch
    B, sc, rays, prim, t = _deformed(prec)
    ref = _reference("s4_3", prec)
    assert not np.array_equal(prim, ref["prim"][:len(rays)])
    tdt = torch.float32 if prec == "f32" else torch.float64
    d_tri = torch.tensor(B["triangles10"], dtype=tdt, device="cuda:0").contiguous()
    d_rays = torch.tensor(rays, dtype=tdt, device="cuda:0").contiguous()
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()
    with _handle(gpu, "s4_3", prec) as h:
        on_a = h.cast(rays)
        assert np.array_equal(on_a[0], ref["prim"][:len(rays)]) and np.array_equal(on_a[1], ref["t"][:len(rays)])
        (h.update_device if how == "update" else h.rebuild_device)(d_tri, s1)
        g_prim, g_t, g_n = query.cast_rays(h, d_rays, want_normal=True, stream=s2)
        g_occ = query.cast_rays(h, d_rays, occlusion=True, stream=s2)
        s2.synchronize()
        g_prim, g_t, g_n, g_occ = g_prim.cpu().numpy(), g_t.cpu().numpy(), g_n.cpu().numpy(), g_occ.cpu().numpy()
        assert np.array_equal(g_prim, prim) and np.array_equal(g_t, t) and np.array_equal(g_occ, (prim >= 0).astype(np.uint8))
        assert not np.array_equal(g_prim, on_a[0])
        h_prim, h_t, h_n = h.cast(rays, want_normal=True)
        assert np.array_equal(h_prim, g_prim) and np.array_equal(h_t, g_t) and np.array_equal(h_n, g_n)
        i_prim, i_t, _ = h.cast(rays, inplace=True)
        assert np.array_equal(i_prim, prim) and np.array_equal(i_t, t)


@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_refusals_with_a_live_handle(gpu, prec):
    ref, sc = _reference("s4_3", prec), _scan("s4_3", prec)
    other = "f64" if prec == "f32" else "f32"
    lib = gpu.lib()
    rays = np.ascontiguousarray(ref["rays"], dtype=sc.T)
    rays_o = np.ascontiguousarray(ref["rays"], dtype=S.dtype_of(other))
    n = len(rays)
    out = np.zeros(4 * n, dtype=np.float64)
    rp, rpo, op = rays.ctypes.data_as(C.c_void_p), rays_o.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p)
    cast, cast_o = getattr(lib, "spira_scene_cast_" + prec), getattr(lib, "spira_scene_cast_" + other)
    occ = getattr(lib, "spira_scene_occluded_" + prec)
    h = _handle(gpu, "s4_3", prec)
    try:
        assert cast_o(h._h, rpo, C.c_uint32(n), C.c_uint32(0), op, op, None) == -1 and b"other precision" in lib.spira_last_error()
        assert cast(h._h, rp, C.c_uint32(n), C.c_uint32(0), None, None, None) == -1 and b"every output is NULL" in lib.spira_last_error()
        assert occ(h._h, rp, C.c_uint32(n), C.c_uint32(0), None) == -1
        assert cast(h._h, rp, C.c_uint32(n), C.c_uint32(2), op, op, None) == -1 and b"unknown flag bits" in lib.spira_last_error()
        assert cast(h._h, rp, C.c_uint32(n), C.c_uint32(0x101), op, op, None) == -1
        _check_against(h, sc, ref, normals=False)                 # a following valid cast still answers
        dead = C.c_void_p(h._h.value)
    finally:
        h.destroy()
    assert cast(dead, rp, C.c_uint32(n), C.c_uint32(0), op, op, None) == -1 and b"NULL or was destroyed" in lib.spira_last_error()
    with _handle(gpu, "s4_3", prec) as h2:
        _check_against(h2, sc, ref, inplace=(False,), normals=False)
