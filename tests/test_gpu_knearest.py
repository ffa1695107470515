"""GPU: spira_scene_nearest_k_* (spira_knearest.h: k_knear, k_knear_session) against the contract's order by brute force (tests/knearest_support.py: every
object's d2 and q from the numpy twins, those within r_max sorted by d2 ascending and index descending, cut at K).  A leaf's d2 and q are the scan's own
functions on the record's own values and the tree only prunes, so prim, dist, point and count are compared bit for bit in both precisions, for the
refilled sessions and for SPIRA_CAST_INPLACE.  The point sets are nearest_support's (about 2 100 points per scene: the sessions refill)."""
import functools

import numpy as np
import pytest

import cast_support as S
import knearest_support as KS
import nearest_support as N
from spira_hip import query

pytestmark = pytest.mark.gpu

KS_ALL = (1, 2, 3, 4, 5, 15, 16)      # the three capacities (1, 4, 16) and both sides of each capacity edge


def _open(gpu, scene, prec):
    return gpu.Scene(scene["spheres5"] if len(scene["spheres5"]) else None, scene["materials8"], scene["triangles10"], prec)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def _poison(h, n, K, count_all=False):
    """The host form stages its outputs in a workspace that outlives the call: n invalid points (NaN) at the same K leave -3 / 0 / 0 / count 0 in every
    staged element first, so an element the next call fails to write cannot pass for a right answer left over from the call before."""
    prim, _, _, count, _ = h.nearest_k(np.full((n, 4), np.nan), K, count_all=count_all, want_trips=True)
    assert not count.any() and (K == 0 or ((prim[0] == -3).all() and (prim[-1] == -3).all()))


def _check(h, ref, K, pick=None, inplace=(False, True), count_all=False):
    """One handle against the order cut at K: prim, dist, point and count bit for bit under both organisations.  Returns the trips of each."""
    prim, dist, point, count = KS.cut(ref, K)
    points = ref["points"]
    if count_all:
        count = ref["total"]
    if pick is not None:
        points, prim, dist, point, count = points[pick], prim[pick], dist[pick], point[pick], count[pick]
    trips = []
    for ip in inplace:
        _poison(h, len(points), K, count_all)
        g_prim, g_dist, g_point, g_count, g_trips = h.nearest_k(points, K, inplace=ip, count_all=count_all, want_trips=True)
        assert g_prim.shape == prim.shape and g_dist.shape == dist.shape and g_point.shape == point.shape and g_count.shape == count.shape
        bad = np.flatnonzero((g_prim != prim).any(axis=1) | (_bits(g_dist) != _bits(dist)).any(axis=1) | (_bits(g_point) != _bits(point)).any(axis=(1, 2)) | (g_count != count))
        assert len(bad) == 0, (K, ip, len(bad), bad[:4], g_prim[bad[:4]], prim[bad[:4]], g_dist[bad[:4]], dist[bad[:4]], g_count[bad[:4]], count[bad[:4]])
        trips.append(g_trips)
    return trips


def _check_slots_of_the_contract(ref, K):
    """The yardstick's own cut: unused slots hold MISS, r_max and 0; invalid points INVALID, 0, 0 and count 0 — so equality with it checks exactly that."""
    prim, dist, point, count = KS.cut(ref, K)
    unused = np.arange(K)[None, :] >= count[:, None]
    v = ref["valid"]
    assert unused[v].any() and (prim[v][unused[v]] == N.MISS).all() and not point[v][unused[v]].any()
    assert np.array_equal(dist[v][unused[v]], np.broadcast_to(ref["r_max"][v][:, None], dist[v].shape)[unused[v]])
    assert (~v).any() and (prim[~v] == N.INVALID).all() and not dist[~v].any() and not point[~v].any() and not count[~v].any()


@pytest.mark.parametrize("prec", ["f32", "f64"])
@pytest.mark.parametrize("name", ["s1", "ico32", "ico33", "ico80", "s4_3", "dup"])
def test_against_the_scan(gpu, name, prec):
    """Spheres only, LDS triangles, the smallest tree, 80 triangles, the 4-level tree of scene_s4(level=3) and its duplicate scene (exact ties), at K = 4."""
    ref, ns = KS.reference(name, prec), N.scan_of(name, prec)
    KS.conditions(ref, 4, ties=(name == "dup"))
    _check_slots_of_the_contract(ref, 4)
    with _open(gpu, N.scene(name), prec) as h:
        trips = _check(h, ref, 4)
    for t in trips:
        if ns.frame is None:
            assert not t.any()                                       # spheres only, LDS triangles: no tree, no trips
        else:
            assert t[ref["prim"][:, 0] >= ns.ns].min() >= 2 and not t[~ref["valid"]].any()
    if ns.frame is not None:
        assert np.array_equal(trips[0], trips[1])                    # the same walk, whatever the organisation


@pytest.mark.parametrize("prec", ["f32", "f64"])
@pytest.mark.parametrize("K", KS_ALL)
@pytest.mark.parametrize("name", ["ico33", "dup"])
def test_every_k(gpu, name, K, prec):
    ref = KS.reference(name, prec)
    KS.conditions(ref, K, ties=(name == "dup"))
    _check_slots_of_the_contract(ref, K)
    with _open(gpu, N.scene(name), prec) as h:
        _check(h, ref, K)


@pytest.mark.parametrize("prec", ["f32", "f64"])
@pytest.mark.parametrize("name", ["s1", "ico32", "s4_3", "dup"])
def test_one_nearest_is_closest_point(gpu, name, prec):
    """max_near = 1: prim, dist and point are spira_scene_closest_point_*'s bytes, and the trips are equal — the walk makes the same decisions from the
    same values."""
    pts = N.reference(name, prec)["points"]
    with _open(gpu, N.scene(name), prec) as h:
        for ip in (False, True):
            c_prim, c_dist, c_point, c_trips = h.closest_point(pts, inplace=ip, want_trips=True)
            _poison(h, len(pts), 1)
            prim, dist, point, count, trips = h.nearest_k(pts, 1, inplace=ip, want_trips=True)
            assert np.array_equal(prim[:, 0], c_prim) and np.array_equal(_bits(dist[:, 0]), _bits(c_dist)) and np.array_equal(_bits(point[:, 0]), _bits(c_point))
            assert np.array_equal(count, (c_prim >= 0).astype(np.uint32)) and np.array_equal(trips, c_trips)
    assert (c_prim >= 0).sum() > 1000 and (c_prim == N.MISS).sum() > 8 and (c_prim == N.INVALID).sum() > 8


@functools.lru_cache(maxsize=None)
def _radius_set(prec):
    """256 points of s4_3's grown box with a finite r_max each, 1 % .. 45 % of the extent: some objects within, most not."""
    sc, ns = N.scene("s4_3"), N.scan_of("s4_3", prec)
    rng = np.random.default_rng(71)
    p = N.in_box(rng, sc, 256)
    p[:, 3] = S.target_box(sc)[3] * 10.0 ** rng.uniform(-2.0, -0.35, len(p))
    return KS.order_of(ns, np.array(p, dtype=ns.T).astype(np.float64))


@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_count_all(gpu, prec):
    """SPIRA_NEAR_COUNT_ALL: the count is the scan's number of candidates — for finite r_max, and for +Inf, where it is the object count; the slots are
    what they are without the flag; max_near = 0 counts only, with NULL lists."""
    ns = N.scan_of("s4_3", prec)
    n_obj = ns.ns + len(ns.tri)
    fin, ref = _radius_set(prec), KS.reference("s4_3", prec)
    t = fin["total"].astype(np.int64)
    assert (t > 16).sum() > 32 and ((t > 0) & (t < 16)).sum() >= 4 and (t == 0).sum() >= 4 and t.max() < n_obj
    inf = ref["valid"] & np.isinf(ref["r_max"])
    assert inf.sum() > 1000 and (ref["total"][inf] == n_obj).all()
    with _open(gpu, N.scene("s4_3"), prec) as h:
        for r in (fin, ref):
            for K in (4, 16):
                _check(h, r, K, count_all=True)                      # the slots of the cut, the count of all
            for ip in (False, True):
                _poison(h, len(r["points"]), 0, count_all=True)
                prim, dist, point, count, _ = h.nearest_k(r["points"], 0, inplace=ip, count_all=True)
                assert prim is None and dist is None and point is None and np.array_equal(count, r["total"])
        assert np.array_equal(query.count_within(h, fin["points"]), fin["total"])
        assert np.array_equal(query.count_within(h, fin["points"][:, :3], radius=fin["points"][:, 3]), fin["total"])


@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_pruning_happens(gpu, prec):
    """On the 4-level tree with r_max = +Inf the walk at K = 4 takes fewer trips than under SPIRA_NEAR_COUNT_ALL, which must meet every triangle; scenes
    without a tree take none."""
    ref, ns = KS.reference("s4_3", prec), N.scan_of("s4_3", prec)
    pick = np.flatnonzero(ref["valid"] & np.isinf(ref["r_max"]))
    assert len(pick) > 1000
    with _open(gpu, N.scene("s4_3"), prec) as h:
        pruned = _check(h, ref, 4, pick=pick)
        everything = _check(h, ref, 4, pick=pick, count_all=True)
    for a, b in zip(pruned, everything):
        print(prec, "mean trips: K = 4 %.1f, COUNT_ALL %.1f of %d triangles" % (a.mean(), b.mean(), len(ns.tri)))
        assert (b > len(ns.tri)).all()                               # a trip per triangle and the nodes above them
        assert a.mean() < b.mean()
    for name in ("s1", "ico32"):
        with _open(gpu, N.scene(name), prec) as h:
            for t in _check(h, KS.reference(name, prec), 4, count_all=True):
                assert not t.any()


@pytest.mark.parametrize("prec", ["f32", "f64"])
@pytest.mark.parametrize("name,K", [("s4_3", 4), ("dup", 3), ("dup", 16)])
def test_r_max_at_the_kth_distance(gpu, name, K, prec):
    """r_max = the K-th distance keeps the K-th object (where r_max * r_max does not round below its d2: the scan decides), one ulp below drops it —
    K - 1 slots are filled, fewer where it was tied — and r_max = 0 finds the vertex a point lies on."""
    ref = KS.edge_set(name, prec, K)
    with _open(gpu, N.scene(name), prec) as h:
        _check(h, ref, K)
        _check(h, ref, K, count_all=True)


@pytest.mark.parametrize("prec", ["f32", "f64"])
@pytest.mark.parametrize("n", [1, 63, 64, 65])
def test_ragged_sizes(gpu, prec, n):
    ref = KS.reference("s4_3", prec)
    pick = np.arange(n) * 37 % len(ref["points"])                    # points of every kind
    with _open(gpu, N.scene("s4_3"), prec) as h:
        for K in (4, 16):
            _check(h, ref, K, pick=pick)


@pytest.mark.parametrize("refill", [1, 64])
@pytest.mark.parametrize("n", [1000, 999])
@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_session_refills_at_both_ends_of_the_threshold(gpu, prec, n, refill):
    """k_knear_session against its in-place twin, by bytes, on the smallest tree at the two ends of the walk loop's exit condition (SPIRA_CAST_REFILL 64: a
    refill only when the whole wave is free; 1: after every finished lane), with SPIRA_CAST_WAVES_PER_CU 1: 4 waves of about 250 points, every wave
    refills; 999 leaves rem = 3.  Both organisations are also held to the scan."""
    from test_gpu_bvh import _with_env
    ref = KS.reference("ico33", prec)
    pick = np.arange(n) * 37 % len(ref["points"])
    pts = ref["points"][pick]

    def go():
        plan = gpu.cast_plan(n, 256)
        assert plan["refill_free"] == refill and plan["base"] > 64 and plan["base"] * plan["waves"] + plan["rem"] == n and (plan["rem"] != 0) == (n == 999), plan
        out = []
        with _open(gpu, N.scene("ico33"), prec) as h:
            for K in (4, 16):
                _check(h, ref, K, pick=pick)
                _poison(h, n, K)
                out.append((h.nearest_k(pts, K), h.nearest_k(pts, K, inplace=True)))
        return out
    for session, inplace in _with_env(gpu, {"SPIRA_CAST_REFILL": str(refill), "SPIRA_CAST_WAVES_PER_CU": "1"}, go):
        for a, b in zip(session[:4], inplace[:4]):                   # prim, dist, point, count
            assert a.dtype == b.dtype and np.array_equal(_bits(a), _bits(b))
        assert (session[0][:, 0] >= 1).sum() > n // 4                # triangle winners: lanes that walked


@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_invalid_points_never_disturb_their_neighbours(gpu, prec):
    sup, ref, ns = N.reference("s4_3", prec), KS.reference("s4_3", prec), N.scan_of("s4_3", prec)
    at = sup["invalid_at"]
    assert len(at) >= 2 * len(N.invalid_kinds(ns.T, ns.frame)) and (np.diff(at) == 7).all() and not ref["valid"][at].any()
    with _open(gpu, N.scene("s4_3"), prec) as h:
        for K in (1, 4, 16):
            w_prim, w_dist, w_point, w_count = KS.cut(ref, K)
            for ip in (False, True):
                _poison(h, len(ref["points"]), K)
                prim, dist, point, count, trips = h.nearest_k(ref["points"], K, inplace=ip, want_trips=True)
                assert (prim[at] == -3).all() and not dist[at].any() and not point[at].any() and not count[at].any() and not trips[at].any()
                nb = at[:-1] + 1
                assert np.array_equal(prim[nb], w_prim[nb]) and np.array_equal(_bits(dist[nb]), _bits(w_dist[nb])) and (prim[nb, 0] >= 0).all()


@functools.lru_cache(maxsize=None)
def _moved(prec, how):
    """ico80 in a new pose.  update: turned about its own centre and moved a little (the tree is refitted and keeps the frame it was built in); rebuild:
    turned, scaled by 1.7 and moved away (the frame is a fresh build's of the new mesh).  Returns (A, B, the order of a point set of B in the frame that holds)."""
    A = N.scene("ico80")
    tri = np.array(A["triangles10"], dtype=np.float64)
    v = tri[:, :9].reshape(-1, 3)
    c = v.mean(axis=0)
    a = 0.4
    R = np.array([[np.cos(a), -np.sin(a), 0.0], [np.sin(a), np.cos(a), 0.0], [0.0, 0.0, 1.0]])
    if how == "update":
        w = (v - c) @ R.T * 0.9 + c + np.array([0.05, -0.03, 0.04])
    else:
        w = (v - c) @ R.T * 1.7 + c + np.array([0.5, -0.25, 1.0])
    B = dict(A, triangles10=np.concatenate([w.reshape(-1, 9), tri[:, 9:]], axis=1))
    frame = S.mesh_frame(A["triangles10"], prec) if how == "update" else S.mesh_frame(B["triangles10"], prec)
    ns = N.NearScan(B, prec, frame=frame)
    pts = N.build_set(ns, B, seed=35, n_near=256, n_box=192, n_edge=64, n_far=48, n_r=32)
    return A, B, KS.order_of(ns, pts["points"]), pts


@pytest.mark.parametrize("how", ["update", "rebuild"])
@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_after_update_and_rebuild(gpu, prec, how):
    """The refitted and the rebuilt tree, through the device forms of update and rebuild: the scan of the new arrays, in the frame that holds."""
    import torch
    A, B, ref, pts = _moved(prec, how)
    KS.conditions(ref, 4)
    far = ref["prim"][pts["parts"]["far"], 0]
    assert (far[0::2] >= 0).all() and not ref["valid"][pts["parts"]["far"]][1::2].any()
    before = KS.order_of(N.scan_of("ico80", prec), ref["points"])
    assert not np.array_equal(before["prim"], ref["prim"])
    tdt = torch.float32 if prec == "f32" else torch.float64
    d_tri = torch.tensor(B["triangles10"], dtype=tdt, device="cuda:0").contiguous()
    with _open(gpu, A, prec) as h:
        st = torch.cuda.current_stream()
        (h.update_device if how == "update" else h.rebuild_device)(d_tri, st)
        for K in (4, 16):
            _check(h, ref, K)


@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_device_form(gpu, prec):
    """Torch tensors on a non-default stream: the bytes of the host form, lists and counts; then every output pointer NULL in turn."""
    import torch
    ref = KS.reference("s4_3", prec)
    tdt = torch.float32 if prec == "f32" else torch.float64
    d_pts = torch.tensor(ref["points"], dtype=tdt, device="cuda:0").contiguous()
    n = len(ref["points"])
    s2 = torch.cuda.Stream()
    torch.cuda.synchronize()
    with _open(gpu, N.scene("s4_3"), prec) as h:
        for K in (1, 4, 16):
            want = KS.cut(ref, K)
            for ip in (False, True):
                host = h.nearest_k(ref["points"], K, inplace=ip)
                g = query.k_nearest(h, d_pts, K, inplace=ip, want_trips=True, stream=s2)
                s2.synchronize()
                for k in range(4):
                    got = g[k].cpu().numpy()
                    assert np.array_equal(_bits(got), _bits(host[k])) and np.array_equal(_bits(got), _bits(want[k])), (K, ip, k)
        cnt = query.count_within(h, d_pts, stream=s2)
        s2.synchronize()
        assert np.array_equal(cnt.cpu().numpy().astype(np.uint32), ref["total"])
        K = 4
        want = KS.cut(ref, K)
        for skip in range(4):
            outs = [torch.full((n, K), -7, dtype=torch.int32, device="cuda:0"), torch.full((n, K), -7, dtype=tdt, device="cuda:0"),
                    torch.full((n, K, 3), -7, dtype=tdt, device="cuda:0"), torch.full((n,), -7, dtype=torch.int32, device="cuda:0")]
            ptrs = [0 if k == skip else o.data_ptr() for k, o in enumerate(outs)]
            h.nearest_k_device(d_pts.data_ptr(), n, K, ptrs[0], ptrs[1], ptrs[2], ptrs[3], s2.cuda_stream)
            s2.synchronize()
            for k, o in enumerate(outs):
                got = o.cpu().numpy()
                if k == skip:
                    assert (got == -7).all()
                else:
                    assert np.array_equal(_bits(got), _bits(want[k].astype(got.dtype))), (skip, k)
