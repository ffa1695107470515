"""GPU: spira_scene_closest_point_* (spira_nearest.h: k_nearest, k_nearest_session) against the brute-force scan over the numpy twins
(tests/nearest_support.py).  The leaf test is the scan's own function on the record's own values and the tree only prunes, so prim, dist and point are
compared bit for bit in both precisions, for the refilled sessions and for SPIRA_CAST_INPLACE.

The point set of a scene (nearest_support.build_set, about 2 100 points — several waves with ranges beyond 128 points, so the sessions refill):
near-surface points, points uniform in the box grown by 1.5, the box centre and the mesh's vertex mean, points exactly on vertices and edge midpoints,
points at 60 .. 64 frame units interleaved with their twins just outside the bound, r_max = the found distance, r_max one ulp below it, r_max = 0 on
vertex and edge points, and every invalid kind interleaved with valid neighbours; r_max = +Inf elsewhere."""
import ctypes as C
import functools

import numpy as np
import pytest

import cast_support as S
import nearest_support as N
from spira_hip import bake, query

pytestmark = pytest.mark.gpu


def _open(gpu, scene, prec):
    return gpu.Scene(scene["spheres5"] if len(scene["spheres5"]) else None, scene["materials8"], scene["triangles10"], prec)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def _poison(h, n):
    """The host form stages its outputs in a workspace that outlives the call: n invalid points (NaN) leave -3 / 0 / 0 in every staged element first, so
    an element the next call fails to write cannot pass for a right answer left over from the call before."""
    bad = np.full((n, 4), np.nan)
    prim = h.closest_point(bad, want_dist=False, want_point=False)[0]
    assert prim[0] == -3 and prim[-1] == -3


def _check(h, points, prim, dist, point, inplace=(False, True)):
    """One handle against the scan: prim, dist and point bit for bit under both organisations.  Returns the trips of each."""
    trips = []
    for ip in inplace:
        _poison(h, len(points))
        g_prim, g_dist, g_point, g_trips = h.closest_point(points, inplace=ip, want_trips=True)
        bad = np.flatnonzero((g_prim != prim) | (_bits(g_dist) != _bits(dist)) | (_bits(g_point) != _bits(point)).any(axis=1))
        assert len(bad) == 0, (ip, len(bad), bad[:6], g_prim[bad[:6]], prim[bad[:6]], g_dist[bad[:6]], dist[bad[:6]], g_point[bad[:6]], point[bad[:6]])
        trips.append(g_trips)
    return trips


def _check_ref(h, ref, **kw):
    return _check(h, ref["points"], ref["prim"], ref["dist"], ref["point"], **kw)


@pytest.mark.parametrize("prec", ["f32", "f64"])
@pytest.mark.parametrize("name", ["s1", "quad", "ico32", "ico33", "ico80", "s4_3", "dup"])
def test_against_the_scan(gpu, name, prec):
    """Spheres only, a tree of flat boxes, LDS triangles, the smallest tree, 80 triangles, the 4-level tree of scene_s4(level=3), and its duplicate
    scene, where exact ties must go to the later index under pruning."""
    ref, ns = N.reference(name, prec), N.scan_of(name, prec)
    assert (ns.frame is not None) == (name not in ("s1", "ico32"))
    with _open(gpu, N.scene(name), prec) as h:
        trips = _check_ref(h, ref)
    for t in trips:
        if ns.frame is None:
            assert not t.any()                                       # no tree: no trips
        else:
            assert t[ref["prim"] >= ns.ns].min() >= 2                # a triangle winner: at least the root and its leaf test
            assert not t[ref["prim"] == N.INVALID].any()


@pytest.mark.parametrize("prec", ["f32", "f64"])
@pytest.mark.parametrize("n", [1, 63, 64, 65])
def test_ragged_sizes(gpu, prec, n):
    ref = N.reference("s4_3", prec)
    pick = np.arange(n) * 37 % len(ref["points"])                    # points of every kind
    with _open(gpu, N.scene("s4_3"), prec) as h:
        _check(h, ref["points"][pick], ref["prim"][pick], ref["dist"][pick], ref["point"][pick])


@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_invalid_points_never_disturb_their_neighbours(gpu, prec):
    ref, ns = N.reference("s4_3", prec), N.scan_of("s4_3", prec)
    at = ref["invalid_at"]
    assert len(at) >= 2 * len(N.invalid_kinds(ns.T, ns.frame))
    with _open(gpu, N.scene("s4_3"), prec) as h:
        for ip in (False, True):
            prim, dist, point, trips = h.closest_point(ref["points"], inplace=ip, want_trips=True)
            assert (prim[at] == -3).all() and not dist[at].any() and not point[at].any() and not trips[at].any()
            assert np.array_equal(prim[at[:-1] + 1], ref["prim"][at[:-1] + 1]) and (prim[at[:-1] + 1] >= 0).all()


@pytest.mark.parametrize("refill", [1, 64])
@pytest.mark.parametrize("n", [1000, 999])
@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_session_refills_at_both_ends_of_the_threshold(gpu, prec, n, refill):
    """k_nearest_session against its in-place twin, by bytes, on the smallest tree (33 triangles) at the two ends of the walk loop's exit condition:
    SPIRA_CAST_REFILL 64 refills only when the whole wave is free, 1 after every finished lane.  SPIRA_CAST_WAVES_PER_CU 1 and 128 points per wave at the
    least leave 4 waves of about 250 points: every wave refills.  1 000 divides among them evenly; 999 leaves rem = 3, so the ranges of base + 1 points are
    walked as well.  Both organisations are also held to the scan."""
    from test_gpu_bvh import _with_env
    ref = N.reference("ico33", prec)
    pick = np.arange(n) * 37 % len(ref["points"])                    # points of every kind
    pts = ref["points"][pick]

    def go():
        plan = gpu.cast_plan(n, 256)
        assert plan["refill_free"] == refill and plan["base"] > 64 and plan["base"] * plan["waves"] + plan["rem"] == n and (plan["rem"] != 0) == (n == 999), plan
        with _open(gpu, N.scene("ico33"), prec) as h:
            _check(h, pts, ref["prim"][pick], ref["dist"][pick], ref["point"][pick])
            _poison(h, n)
            return h.closest_point(pts), h.closest_point(pts, inplace=True)
    session, inplace = _with_env(gpu, {"SPIRA_CAST_REFILL": str(refill), "SPIRA_CAST_WAVES_PER_CU": "1"}, go)
    for a, b in zip(session[:3], inplace[:3]):                       # prim, dist, point
        assert a.dtype == b.dtype and np.array_equal(_bits(a), _bits(b))
    assert (session[0] >= 1).sum() > n // 4                          # triangle winners: lanes that walked


@functools.lru_cache(maxsize=None)
def _frame_case(prec, fi, how):
    """The blob mesh in placement fi; how = create: as built; update: twisted (test_gpu_refit.deform), the validity frame stays the creation frame;
    rebuild: twisted, then scaled by 1.7 and moved, the frame is the fresh build's of that mesh.  Returns (A, B, scan of B in the frame that holds, set)."""
    A, B, frame = N.frame_mesh(prec, fi, how)                        # (shared with the K-nearest and the overlap edge tests)
    ns = N.NearScan(B, prec, frame=frame)
    return A, B, ns, N.build_set(ns, B, seed=33 + fi, n_near=256, n_box=192, n_edge=64, n_far=48, n_r=32)


@pytest.mark.parametrize("how", ["create", "update", "rebuild"])
@pytest.mark.parametrize("fi", range(len(S.FRAMES)))
@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_frames_updates_and_rebuilds(gpu, prec, fi, how):
    """The four placements of cast_support.FRAMES, each as built, after an update and after a rebuild: far points at 60 .. 64 units of the frame that
    holds stay valid and exact, their twins come back INVALID."""
    A, B, ns, ref = _frame_case(prec, fi, how)
    far = ref["prim"][ref["parts"]["far"]]
    assert (far[0::2] >= 0).all() and (far[1::2] == N.INVALID).all()
    with _open(gpu, A, prec) as h:
        if how != "create":
            (h.update if how == "update" else h.rebuild)(triangles10=B["triangles10"])
        _check_ref(h, ref)


@pytest.mark.parametrize("how", ["update", "rebuild"])
@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_device_form_sees_the_new_tree(gpu, prec, how):
    """The new tree on one stream, the query on another non-default one, no host synchronisation in between; then every output pointer NULL in turn."""
    import torch
    A, B, ns, ref = _frame_case(prec, 0, how)
    before = N.NearScan(A, prec).query(ref["points"])
    assert not np.array_equal(before[0], ref["prim"])
    tdt = torch.float32 if prec == "f32" else torch.float64
    d_tri = torch.tensor(B["triangles10"], dtype=tdt, device="cuda:0").contiguous()
    d_pts = torch.tensor(ref["points"], dtype=tdt, device="cuda:0").contiguous()
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()
    with _open(gpu, A, prec) as h:
        (h.update_device if how == "update" else h.rebuild_device)(d_tri, s1)
        for ip in (False, True):
            g = query.closest_points(h, d_pts, inplace=ip, want_trips=True, stream=s2)
            s2.synchronize()
            g_prim, g_dist, g_point = g[0].cpu().numpy(), g[1].cpu().numpy(), g[2].cpu().numpy()
            assert np.array_equal(g_prim, ref["prim"]) and np.array_equal(_bits(g_dist), _bits(ref["dist"])) and np.array_equal(_bits(g_point), _bits(ref["point"])), ip
        n = len(ref["points"])
        for skip in range(3):
            outs = [torch.full((n,), -7, dtype=torch.int32, device="cuda:0"), torch.full((n,), -7, dtype=tdt, device="cuda:0"), torch.full((n, 3), -7, dtype=tdt, device="cuda:0")]
            ptrs = [0 if k == skip else o.data_ptr() for k, o in enumerate(outs)]
            h.closest_point_device(d_pts.data_ptr(), n, ptrs[0], ptrs[1], ptrs[2], s2.cuda_stream)
            s2.synchronize()
            got = [o.cpu().numpy() for o in outs]
            for k, want in enumerate((ref["prim"], ref["dist"], ref["point"])):
                if k == skip:
                    assert (got[k] == -7).all()
                else:
                    assert np.array_equal(got[k], want), (skip, k)


@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_multi_device_handle_and_refusals(gpu, prec):
    ref, ns = N.reference("ico80", prec), N.scan_of("ico80", prec)
    s = N.scene("ico80")
    with gpu.Scene(s["spheres5"], s["materials8"], s["triangles10"], prec, n_devices=1) as h:
        _check_ref(h, ref, inplace=(False,))
    other = "f64" if prec == "f32" else "f32"
    lib = gpu.lib()
    pts = np.ascontiguousarray(ref["points"], dtype=S.dtype_of(other))
    out = np.zeros(4 * len(pts), dtype=np.float64).ctypes.data_as(C.c_void_p)
    with _open(gpu, s, prec) as h:
        fn = getattr(lib, "spira_scene_closest_point_" + other)
        assert fn(h._h, pts.ctypes.data_as(C.c_void_p), C.c_uint32(len(pts)), C.c_uint32(0), out, out, out, None) == -1 and b"other precision" in lib.spira_last_error()
        _check_ref(h, ref, inplace=(False,))                         # a following valid call still answers


@functools.lru_cache(maxsize=None)
def _pruning_set(prec):
    sc, ns = N.scene("s4_4"), N.scan_of("s4_4", prec)
    pts = np.array(N.near_surface(np.random.default_rng(51), sc, 1024), dtype=ns.T).astype(np.float64)
    prim, dist, point, valid = ns.query(pts)
    return pts, prim, dist, point


@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_the_walk_prunes(gpu, prec):
    """scene_s4(level=4)'s 5 120 triangles, near-surface points: a walk that visits everything takes more than n_triangles trips, a working one tens.
    The bound is a condition, not a measurement: mean out_trips below n_triangles / 16 for both organisations.  The sphere-only scene takes no trips."""
    pts, prim, dist, point = _pruning_set(prec)
    ns = N.scan_of("s4_4", prec)
    assert len(ns.tri) == 5120 and (prim >= ns.ns).mean() > 0.95
    with _open(gpu, N.scene("s4_4"), prec) as h:
        t_session, t_inplace = _check(h, pts, prim, dist, point)
    print(prec, "mean trips: sessions %.1f, in place %.1f; max %d" % (t_session.mean(), t_inplace.mean(), t_session.max()))
    assert np.array_equal(t_session, t_inplace)                      # the same walk, whatever the organisation
    assert t_session.mean() < len(ns.tri) / 16 and t_inplace.mean() < len(ns.tri) / 16
    ref = N.reference("s1", prec)
    with _open(gpu, N.scene("s1"), prec) as h:
        assert not h.closest_point(ref["points"], want_trips=True)[3].any()


@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_bake_snaps_points_to_the_surface(gpu, prec):
    """bake.snap_to_surface: positions become the scan's closest points, normals the winning triangle's."""
    sc, ns = N.scene("ico80"), N.scan_of("ico80", prec)
    rng = np.random.default_rng(61)
    p4 = N.near_surface(rng, sc, 96, frac=0.05)
    p6 = np.concatenate([p4[:, :3], np.tile([0.0, 1.0, 0.0], (len(p4), 1))], axis=1)
    prim, _, point, _ = ns.query(np.array(p4, dtype=ns.T).astype(np.float64))                  # the values the library sees
    with _open(gpu, sc, prec) as h:
        out, g_prim = bake.snap_to_surface(h, p6, sc["triangles10"])
    assert np.array_equal(g_prim, prim) and np.array_equal(out[:, :3], point)
    on_tri = prim >= ns.ns
    assert on_tri.sum() > 48
    nrm = bake.triangle_points(sc["triangles10"], prec)[:, 3:6]
    assert np.array_equal(out[on_tri, 3:6], nrm[prim[on_tri] - ns.ns]) and np.array_equal(out[~on_tri, 3:6], p6[~on_tri, 3:6].astype(ns.T))
