"""GPU: spira_scene_sweep_* / spira_scene_sweep_blocked_* (spira_sweep.h: k_sweep, k_sweep_session) against the brute-force scan over the numpy twins
(tests/sweep_support.py).  The leaf test is the scan's own function on the record's own values and the tree only prunes, so prim, t, point and normal are
compared bit for bit in both precisions, for the refilled sessions and for SPIRA_CAST_INPLACE; blocked == (prim >= 0), 255 for invalid sweeps.

The sweep set of a scene (sweep_support.build_set, about 2 000 sweeps — several waves with ranges beyond 128 sweeps, so the sessions refill): head-on
sweeps toward the surface and grazing ones; sweeps starting in overlap, with several triangles, so that ties go to the later index; r = 0, along rays and
on vertices and edge midpoints; axis-parallel directions; sweeps inside the scene's spheres (the R - r root); origins at 60 .. 64 frame units with their
twins just beyond; balls of 1 .. 4 frame units, and at the radius bound the last valid radius and the first invalid one, and that radius from
origins at 60 .. 64 units on every axis; t_max equal to the found t, one
ulp below it, and t_min past the first contact; every invalid kind interleaved with valid neighbours."""
import ctypes as C
import functools

import numpy as np
import pytest

import cast_support as S
import nearest_support as N
import sweep_support as W
from spira_hip import query

pytestmark = pytest.mark.gpu


def _open(gpu, scene, prec):
    return gpu.Scene(scene["spheres5"] if len(scene["spheres5"]) else None, scene["materials8"], scene["triangles10"], prec)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def _poison(h, n):
    """The host form stages its outputs in a workspace that outlives the call: n invalid sweeps (NaN) leave -3 / 0 / 0 / 0 and 255 in every staged element
    first, so an element the next call fails to write cannot pass for a right answer left over from the call before."""
    bad, rad = np.full((n, 8), np.nan), np.zeros(n)
    prim = h.sweep(bad, rad, want_t=False, want_point=False, want_normal=False)[0]
    assert prim[0] == -3 and prim[-1] == -3
    hit = h.sweep_blocked(bad, rad)
    assert hit[0] == 255 and hit[-1] == 255


def _check(h, rays, radii, prim, t, point, normal, inplace=(False, True)):
    """One handle against the scan: prim, t, point and normal bit for bit and blocked == (prim >= 0) under both organisations.  Returns the trips of each."""
    trips = []
    want_hit = np.where(prim == W.INVALID, 255, prim >= 0).astype(np.uint8)
    for ip in inplace:
        _poison(h, len(rays))
        g_prim, g_t, g_point, g_normal, g_trips = h.sweep(rays, radii, inplace=ip, want_trips=True)
        bad = np.flatnonzero((g_prim != prim) | (_bits(g_t) != _bits(t)) | (_bits(g_point) != _bits(point)).any(axis=1) | (_bits(g_normal) != _bits(normal)).any(axis=1))
        assert len(bad) == 0, (ip, len(bad), bad[:6], g_prim[bad[:6]], prim[bad[:6]], g_t[bad[:6]], t[bad[:6]], g_point[bad[:6]], point[bad[:6]], g_normal[bad[:6]], normal[bad[:6]])
        _poison(h, len(rays))
        g_hit = h.sweep_blocked(rays, radii, inplace=ip)
        bad = np.flatnonzero(g_hit != want_hit)
        assert len(bad) == 0, (ip, "blocked", len(bad), bad[:6], g_hit[bad[:6]], want_hit[bad[:6]])
        trips.append(g_trips)
    return trips


def _check_ref(h, ref, **kw):
    return _check(h, ref["rays"], ref["radii"], ref["prim"], ref["t"], ref["point"], ref["normal"], **kw)


@pytest.mark.parametrize("prec", ["f32", "f64"])
@pytest.mark.parametrize("name", ["s1", "quad", "ico32", "ico33", "ico80", "s4_3", "dup"])
def test_against_the_scan(gpu, name, prec):
    """Spheres only, a tree of flat boxes, LDS triangles, the smallest tree, 80 triangles, the 4-level tree of scene_s4(level=3), and its duplicate
    scene, where exact ties must go to the later index under pruning."""
    ref, ss = W.reference(name, prec), W.scan_of(name, prec)
    assert (ss.frame is not None) == (name not in ("s1", "ico32"))
    assert (ref["prim"] >= 0).sum() > 500 and (ref["prim"] == W.MISS).sum() > 100 and (ref["prim"] == W.INVALID).sum() >= 20
    with _open(gpu, N.scene(name), prec) as h:
        trips = _check_ref(h, ref)
    for t in trips:
        if ss.frame is None:
            assert not t.any()                                       # no tree: no trips
        else:
            assert t[ref["prim"] >= ss.ns].min() >= 2                # a triangle winner: at least the root and its leaf test
            assert not t[ref["prim"] == W.INVALID].any()


@pytest.mark.parametrize("prec", ["f32", "f64"])
@pytest.mark.parametrize("n", [1, 63, 64, 65])
def test_ragged_sizes(gpu, prec, n):
    ref = W.reference("s4_3", prec)
    pick = np.arange(n) * 37 % len(ref["rays"])                      # sweeps of every kind
    with _open(gpu, N.scene("s4_3"), prec) as h:
        _check(h, ref["rays"][pick], ref["radii"][pick], ref["prim"][pick], ref["t"][pick], ref["point"][pick], ref["normal"][pick])


@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_invalid_sweeps_never_disturb_their_neighbours(gpu, prec):
    ref, ss = W.reference("s4_3", prec), W.scan_of("s4_3", prec)
    at = ref["invalid_at"]
    assert len(at) >= len(W.invalid_kinds(ss.T, ss.frame)[1])
    with _open(gpu, N.scene("s4_3"), prec) as h:
        for ip in (False, True):
            prim, t, point, normal, trips = h.sweep(ref["rays"], ref["radii"], inplace=ip, want_trips=True)
            assert (prim[at] == -3).all() and not t[at].any() and not point[at].any() and not normal[at].any() and not trips[at].any()
            assert np.array_equal(prim[at[:-1] + 1], ref["prim"][at[:-1] + 1]) and (prim[at[:-1] + 1] != -3).all()
            hit = h.sweep_blocked(ref["rays"], ref["radii"], inplace=ip)
            assert (hit[at] == 255).all() and (hit[at[:-1] + 1] != 255).all()


@pytest.mark.parametrize("refill", [1, 64])
@pytest.mark.parametrize("n", [1000, 999])
@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_session_refills_at_both_ends_of_the_threshold(gpu, prec, n, refill):
    """k_sweep_session against its in-place twin, by bytes, on the smallest tree (33 triangles) at the two ends of the walk loop's exit condition:
    SPIRA_CAST_REFILL 64 refills only when the whole wave is free, 1 after every finished lane.  SPIRA_CAST_WAVES_PER_CU 1 and 128 sweeps per wave at the
    least leave 4 waves of about 250 sweeps: every wave refills.  1 000 divides among them evenly; 999 leaves rem = 3, so the ranges of base + 1 sweeps are
    walked as well.  Both organisations are also held to the scan."""
    from test_gpu_bvh import _with_env
    ref = W.reference("ico33", prec)
    pick = np.arange(n) * 37 % len(ref["rays"])                      # sweeps of every kind
    rays, radii = ref["rays"][pick], ref["radii"][pick]

    def go():
        plan = gpu.cast_plan(n, 256)
        assert plan["refill_free"] == refill and plan["base"] > 64 and plan["base"] * plan["waves"] + plan["rem"] == n and (plan["rem"] != 0) == (n == 999), plan
        with _open(gpu, N.scene("ico33"), prec) as h:
            _check(h, rays, radii, ref["prim"][pick], ref["t"][pick], ref["point"][pick], ref["normal"][pick])
            _poison(h, n)
            return h.sweep(rays, radii), h.sweep(rays, radii, inplace=True), h.sweep_blocked(rays, radii), h.sweep_blocked(rays, radii, inplace=True)
    session, inplace, b_session, b_inplace = _with_env(gpu, {"SPIRA_CAST_REFILL": str(refill), "SPIRA_CAST_WAVES_PER_CU": "1"}, go)
    for a, b in zip(session[:4], inplace[:4]):                       # prim, t, point, normal
        assert a.dtype == b.dtype and np.array_equal(_bits(a), _bits(b))
    assert np.array_equal(b_session, b_inplace)
    assert (session[0] >= 1).sum() > n // 4                          # triangle winners: lanes that walked


@functools.lru_cache(maxsize=None)
def _frame_case(prec, fi, how):
    """The blob mesh in placement fi; how = create: as built; update: twisted (test_gpu_refit.deform), the validity frame stays the creation frame;
    rebuild: twisted, then scaled by 1.7 and moved, the frame is the fresh build's of that mesh.  Returns (A, B, scan of B in the frame that holds, set)."""
    from test_gpu_refit import deform
    A = S.blob_scene(2, *S.FRAMES[fi])
    if how == "create":
        B, frame = A, None
    else:
        tri = deform(A["triangles10"])
        if how == "rebuild":
            tri = np.array(tri)
            for v in range(3):
                tri[:, 3 * v:3 * v + 3] = tri[:, 3 * v:3 * v + 3] * 1.7 + np.array([0.5, -0.25, 1.0]) * S.FRAMES[fi][0]
        B = dict(A, triangles10=tri)
        frame = S.mesh_frame(A["triangles10"], prec) if how == "update" else S.mesh_frame(tri, prec)
    ss = W.SweepScan(B, prec, frame=frame)
    return A, B, ss, W.build_set(ss, B, seed=73 + fi, n_head=160, n_graze=96, n_over=64, n_box=96, n_axis=48, n_far=48, n_big=48, n_bound=32, n_in=32, n_win=32, n_zero=32, n_corner=32)


@pytest.mark.parametrize("how", ["create", "update", "rebuild"])
@pytest.mark.parametrize("fi", range(len(S.FRAMES)))
@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_frames_updates_and_rebuilds(gpu, prec, fi, how):
    """The four placements of cast_support.FRAMES, each as built, after an update and after a rebuild: far sweeps at 60 .. 64 units of the frame that
    holds stay valid and exact, their twins come back INVALID; so do the radii on either side of the radius bound."""
    A, B, ss, ref = _frame_case(prec, fi, how)
    far, bound = ref["prim"][ref["parts"]["far"]], ref["prim"][ref["parts"]["bound"]]
    assert (far[0::2] != W.INVALID).all() and (far[0::2] >= 0).any() and (far[1::2] == W.INVALID).all()
    assert (bound[0::2] != W.INVALID).all() and (bound[1::2] == W.INVALID).all()
    with _open(gpu, A, prec) as h:
        if how != "create":
            (h.update if how == "update" else h.rebuild)(triangles10=B["triangles10"])
        _check_ref(h, ref)


@pytest.mark.parametrize("how", ["update", "rebuild"])
@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_device_form_sees_the_new_tree(gpu, prec, how):
    """The new tree on one stream, the sweep on another non-default one, no host synchronisation in between; then every output pointer NULL in turn."""
    import torch
    A, B, ss, ref = _frame_case(prec, 0, how)
    before = W.SweepScan(A, prec).sweep(ref["rays"], ref["radii"])
    assert not np.array_equal(before[0], ref["prim"])
    tdt = torch.float32 if prec == "f32" else torch.float64
    d_tri = torch.tensor(B["triangles10"], dtype=tdt, device="cuda:0").contiguous()
    d_rays = torch.tensor(ref["rays"], dtype=tdt, device="cuda:0").contiguous()
    d_rad = torch.tensor(ref["radii"], dtype=tdt, device="cuda:0").contiguous()
    want = (ref["prim"], ref["t"], ref["point"], ref["normal"])
    want_hit = np.where(ref["prim"] == W.INVALID, 255, ref["prim"] >= 0).astype(np.uint8)
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()
    with _open(gpu, A, prec) as h:
        (h.update_device if how == "update" else h.rebuild_device)(d_tri, s1)
        for ip in (False, True):
            g = query.sweep_spheres(h, d_rays, d_rad, inplace=ip, want_trips=True, stream=s2)
            b = query.sweep_spheres(h, d_rays, d_rad, blocked=True, inplace=ip, stream=s2)
            s2.synchronize()
            for k in range(4):
                assert np.array_equal(_bits(g[k].cpu().numpy()), _bits(want[k])), (ip, k)
            assert np.array_equal(b.cpu().numpy(), want_hit), ip
        n = len(ref["rays"])
        for skip in range(4):
            outs = [torch.full((n,), -7, dtype=torch.int32, device="cuda:0"), torch.full((n,), -7, dtype=tdt, device="cuda:0"),
                    torch.full((n, 3), -7, dtype=tdt, device="cuda:0"), torch.full((n, 3), -7, dtype=tdt, device="cuda:0")]
            ptrs = [0 if k == skip else o.data_ptr() for k, o in enumerate(outs)]
            h.sweep_device(d_rays.data_ptr(), d_rad.data_ptr(), n, ptrs[0], ptrs[1], ptrs[2], ptrs[3], s2.cuda_stream)
            s2.synchronize()
            got = [o.cpu().numpy() for o in outs]
            for k in range(4):
                if k == skip:
                    assert (got[k] == -7).all()
                else:
                    assert np.array_equal(_bits(got[k]), _bits(want[k])), (skip, k)


@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_multi_device_handle_and_refusals(gpu, prec):
    ref = W.reference("ico80", prec)
    s = N.scene("ico80")
    with gpu.Scene(s["spheres5"], s["materials8"], s["triangles10"], prec, n_devices=1) as h:
        _check_ref(h, ref, inplace=(False,))
    other = "f64" if prec == "f32" else "f32"
    lib = gpu.lib()
    with np.errstate(over="ignore"):                                 # (Float64's invalid kinds overflow Float32)
        rays = np.ascontiguousarray(ref["rays"], dtype=S.dtype_of(other))
        rad = np.ascontiguousarray(ref["radii"], dtype=S.dtype_of(other))
    out = np.zeros(4 * len(rays), dtype=np.float64).ctypes.data_as(C.c_void_p)
    with _open(gpu, s, prec) as h:
        fn = getattr(lib, "spira_scene_sweep_" + other)
        rc = fn(h._h, rays.ctypes.data_as(C.c_void_p), rad.ctypes.data_as(C.c_void_p), C.c_uint32(len(rays)), C.c_uint32(0), out, out, out, out, None)
        assert rc == -1 and b"other precision" in lib.spira_last_error()
        fn = getattr(lib, "spira_scene_sweep_blocked_" + other)
        assert fn(h._h, rays.ctypes.data_as(C.c_void_p), rad.ctypes.data_as(C.c_void_p), C.c_uint32(len(rays)), C.c_uint32(0), out) == -1 and b"other precision" in lib.spira_last_error()
        _check_ref(h, ref, inplace=(False,))                         # a following valid call still answers


@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_blocked_at_the_start_is_count_within(gpu, prec):
    """t_min = t_max = 0: the sweep is blocked exactly where the existing K-nearest entry counts an object within r of the origin."""
    sc, ss = N.scene("s4_3"), W.scan_of("s4_3", prec)
    rng = np.random.default_rng(81)
    n = 1024
    ext = S.target_box(sc)[3]
    p = np.array(N.near_surface(rng, sc, n, frac=0.1)[:, :3], dtype=ss.T).astype(np.float64)
    r = np.array(rng.uniform(0.0, 0.1, n) * ext, dtype=ss.T).astype(np.float64)
    rays = np.concatenate([p, np.zeros((n, 1)), S._unit(rng, n), np.zeros((n, 1))], axis=1)
    with _open(gpu, sc, prec) as h:
        count = query.count_within(h, p, r)
        for ip in (False, True):
            hit = h.sweep_blocked(rays, r, inplace=ip)
            assert np.array_equal(hit, (count > 0).astype(np.uint8)), ip
    assert 0.2 < (count > 0).mean() < 0.8


@functools.lru_cache(maxsize=None)
def _pruning_set(prec):
    sc, ss = N.scene("s4_4"), W.scan_of("s4_4", prec)
    rng = np.random.default_rng(82)
    ext = S.target_box(sc)[3]
    rays, radii = W.head_on(rng, sc, 256, lo=0.01, hi=0.01)
    rays, radii = np.array(rays, dtype=ss.T).astype(np.float64), np.array(radii, dtype=ss.T).astype(np.float64)
    return (rays, radii) + ss.sweep(rays, radii)[:4]


@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_the_walk_prunes(gpu, prec):
    """scene_s4(level=4)'s 5 120 triangles, sweeps toward the surface with r of 1 % of the extent: a walk that visits everything takes more than
    n_triangles trips, a working one tens.  The bound is a condition, not a measurement: mean out_trips below n_triangles / 16 for both organisations, the
    trips equal between them.  The sphere-only scene takes no trips."""
    rays, radii, prim, t, point, normal = _pruning_set(prec)
    ss = W.scan_of("s4_4", prec)
    assert len(ss.tri) == 5120 and (prim >= ss.ns).mean() > 0.75     # (origins below the ground meet the ground sphere first)
    with _open(gpu, N.scene("s4_4"), prec) as h:
        t_session, t_inplace = _check(h, rays, radii, prim, t, point, normal)
    print(prec, "mean trips: sessions %.1f, in place %.1f; max %d" % (t_session.mean(), t_inplace.mean(), t_session.max()))
    assert np.array_equal(t_session, t_inplace)                      # the same walk, whatever the organisation
    assert t_session.mean() < len(ss.tri) / 16 and t_inplace.mean() < len(ss.tri) / 16
    ref = W.reference("s1", prec)
    with _open(gpu, N.scene("s1"), prec) as h:
        assert not h.sweep(ref["rays"], ref["radii"], want_trips=True)[4].any()


@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_sweep_segments_reproduce_the_scan(gpu, prec):
    """query.sweep_segments on ico80: the fractions are the scan's t / |b - a| on the rays the helper builds."""
    sc, ss = N.scene("ico80"), W.scan_of("ico80", prec)
    rng = np.random.default_rng(83)
    n = 96
    _, _, c, ext = S.target_box(sc)
    a = c + 1.5 * ext * S._unit(rng, n)
    b = N.surface_points(rng, sc, n) + (N.surface_points(rng, sc, n) - a) * rng.uniform(-0.3, 0.5, (n, 1))
    b[-1] = a[-1]                                                    # a segment of no length: invalid
    radius = 0.04 * ext
    d = b - a
    length = np.sqrt((d * d).sum(axis=1))
    rays = np.concatenate([a, np.zeros((n, 1)), d, length[:, None]], axis=1).astype(ss.T)
    prim, t, point, _, _ = ss.sweep(rays, np.full(n, radius, dtype=ss.T))
    with _open(gpu, sc, prec) as h:
        g_prim, g_frac, g_point = query.sweep_segments(h, a, b, radius)
    assert np.array_equal(g_prim, prim) and np.array_equal(_bits(g_point), _bits(point))
    with np.errstate(all="ignore"):
        want = np.where(prim == W.INVALID, ss.T(0), t / rays[:, 7])
    assert np.array_equal(_bits(g_frac.astype(ss.T)), _bits(want.astype(ss.T)))
    assert g_prim[-1] == W.INVALID and (g_prim[:-1] >= 0).sum() > n // 3 and (g_prim[:-1] == W.MISS).sum() > 4 and (g_frac[g_prim == W.MISS] == 1).all()
