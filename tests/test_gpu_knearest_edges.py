"""GPU: the claims of spira_knearest.h that tests/test_gpu_knearest.py never reaches, each against the yardstick of tests/knearest_support.py (order_of,
cut) and always on the bytes of prim, dist, point and count (the total under count_all) — no tolerance, no measurement:
  * the four placements of cast_support.FRAMES, as built, after an update and after a rebuild: the walk prunes in Float32 in the tree's frame against a
    bound converted from the caller's units every time the K-th d2 moves; far points at 60 .. 64 frame units with their invalid twins;
  * r_max at the K-th distance FROM those far points, where d2 is in the thousands of normalised units and the bound starts at a candidate's distance;
  * a list full of one d2 while further candidates with that d2 keep arriving in the tree's order (17 coincident copies of every triangle), for every K
    of the three forms of near_insert and knear_store, on the host builder's tree and on the device rebuild's, which meets the copies in another order;
  * r_max whose square is the largest finite value, +Inf, 0 and subnormal, through k-nearest and closest-point alike;
  * the 5 120-triangle tree with the 16-entry list in scratch beside the walk's stack, and a bound on its trips;
  * every subset of the device form's outputs at capacity 16 (q is computed again at the store, with `point` present and absent).
Before every compared host-form call the staging is poisoned (test_gpu_knearest._poison).  The sets come from knearest_support.py;
tests/test_knearest_edges_cpu.py asserts without a device that they reach what they are for."""
import numpy as np
import pytest

import cast_support as S
import knearest_support as KS
import nearest_support as N
from test_gpu_knearest import _bits, _check, _open, _poison
from test_gpu_nearest import _check as _check_closest

pytestmark = pytest.mark.gpu

PRECS = ["f32", "f64"]


def _same_walk(trips):
    assert np.array_equal(trips[0], trips[1])                        # the same walk, whatever the organisation


# ------------------------------------------------------------------------------------------------ 1: placements, updates, rebuilds
@pytest.mark.parametrize("how", ["create", "update", "rebuild"])
@pytest.mark.parametrize("fi", range(len(S.FRAMES)))
@pytest.mark.parametrize("prec", PRECS)
def test_frames_updates_and_rebuilds(gpu, prec, fi, how):
    """The bound is the K-th d2 of the moment, converted to normalised units whenever it changes (near_bestn in knear_step): where amax_n is large (far
    from the origin), where the caller's units are a thousand times the frame's, and in a frame that is not a fresh build's (after an update)."""
    A, B, ns, pts, ref = KS.frame_case(prec, fi, how)
    far, twins = KS.far_valid(pts)
    assert ref["valid"][far].all() and (ref["total"][far] == ns.ns + len(ns.tri)).all() and not ref["valid"][twins].any()
    with _open(gpu, A, prec) as h:
        if how != "create":
            (h.update if how == "update" else h.rebuild)(triangles10=B["triangles10"])
        for K in (4, 16):
            KS.conditions(ref, K)
            prim, dist, point, count = KS.cut(ref, K)
            assert (prim[twins] == N.INVALID).all() and not dist[twins].any() and not point[twins].any() and not count[twins].any()
            assert (prim[far] >= 0).all() and (count[far] == K).all()
            trips = _check(h, ref, K)
            _same_walk(trips)
            assert trips[0][far].min() >= 2 and not trips[0][twins].any()


# ------------------------------------------------------------------------------------------------ 2: r_max at the K-th distance, far away
@pytest.mark.parametrize("fi", range(len(S.FRAMES)))
@pytest.mark.parametrize("prec", PRECS)
def test_r_max_at_the_kth_distance_from_far_points(gpu, prec, fi):
    """r_max = the K-th distance from 60 .. 64 frame units: the first bestn is made from a candidate's own d2, thousands of normalised units, and must
    not round below it; one ulp below drops the K-th object and all tied with it."""
    A = KS.frame_case(prec, fi, "create")[0]
    with _open(gpu, A, prec) as h:
        for K in (4, 16):
            ref = KS.far_edge_set(prec, fi, K)
            _same_walk(_check(h, ref, K))
            _same_walk(_check(h, ref, K, count_all=True))


# ------------------------------------------------------------------------------------------------ 3: lists full of one distance
@pytest.mark.parametrize("K", range(1, 17))
@pytest.mark.parametrize("prec", PRECS)
def test_ties_fill_the_list_at_every_k(gpu, prec, K):
    """Every triangle 17 times: once the list holds K copies at one d2, every further copy is a candidate AT the bound (the node test is strict, the leaf
    test d2 <= bound) and near_insert keeps it only by its index.  A `<` for that `<=`, or a reversed index comparison, gives another list.  The same
    handle after a rebuild of the same triangles: the Morton-order tree meets the copies in another order and the bytes must stay."""
    sc, ref = KS.pile_scene(), KS.pile_ref(prec)
    KS.pile_conditions(ref, K)
    pts = ref["points"]
    with _open(gpu, sc, prec) as h:
        _same_walk(_check(h, ref, K))
        _poison(h, len(pts), K)
        before = h.nearest_k(pts, K)
        h.rebuild(triangles10=sc["triangles10"])
        _same_walk(_check(h, ref, K))
        _poison(h, len(pts), K)
        after = h.nearest_k(pts, K)
        for a, b in zip(before[:4], after[:4]):
            assert a.dtype == b.dtype and np.array_equal(_bits(a), _bits(b))
        if K == 16:
            _same_walk(_check(h, ref, K, count_all=True))            # the count is the scan's total


@pytest.mark.parametrize("prec", PRECS)
def test_one_nearest_on_the_pile_is_closest_point(gpu, prec):
    """max_near = 1 on the pile: spira_scene_closest_point_*'s bytes and trips — both walks decide 17-fold ties alike."""
    pts = KS.pile_set(prec)["points"]
    with _open(gpu, KS.pile_scene(), prec) as h:
        for ip in (False, True):
            c_prim, c_dist, c_point, c_trips = h.closest_point(pts, inplace=ip, want_trips=True)
            _poison(h, len(pts), 1)
            prim, dist, point, count, trips = h.nearest_k(pts, 1, inplace=ip, want_trips=True)
            assert np.array_equal(prim[:, 0], c_prim) and np.array_equal(_bits(dist[:, 0]), _bits(c_dist)) and np.array_equal(_bits(point[:, 0]), _bits(c_point))
            assert np.array_equal(count, (c_prim >= 0).astype(np.uint32)) and np.array_equal(trips, c_trips)
    assert (c_prim >= 1).sum() > 500 and (c_prim == N.MISS).sum() >= 32 and (c_prim == N.INVALID).sum() > 8


# ------------------------------------------------------------------------------------------------ 4: r_max * r_max outside the normal range
@pytest.mark.parametrize("prec", PRECS)
def test_extreme_radii(gpu, prec):
    """near_load's best0 = r_max * r_max in T: the largest finite square, +Inf, 0 and a subnormal number.  Unused slots carry r_max itself back."""
    for name in ("pile", "ico32"):
        sc = KS.pile_scene() if name == "pile" else N.scene(name)
        ns = KS.pile_scan(prec) if name == "pile" else N.scan_of(name, prec)
        ref = KS.extreme_radius_set(name, prec)
        pts = ref["points"]
        with _open(gpu, sc, prec) as h:
            for K in (1, 4, 16):
                prim, dist, point, count = KS.cut(ref, K)
                unused = np.arange(K)[None, :] >= count[:, None]
                for key in "cd":
                    s = ref["parts"][key]
                    assert unused[s].any() and np.array_equal(_bits(dist[s][unused[s]]), _bits(np.broadcast_to(ref["r_max"][s][:, None], dist[s].shape)[unused[s]]))
                trips = _check(h, ref, K)
                _check(h, ref, K, count_all=True)
                if ns.frame is not None:
                    _same_walk(trips)
            c_prim, c_dist, c_point, valid = ns.query(pts)
            assert valid.all() and (c_prim == N.MISS).any()
            _check_closest(h, pts, c_prim, c_dist, c_point)


# ------------------------------------------------------------------------------------------------ 5: the deep tree under a scratch list
@pytest.mark.parametrize("prec", PRECS)
def test_deep_tree_long_list(gpu, prec):
    """scene_s4(level=4)'s 5 120 triangles, one level deeper than any tree k-nearest ran on, with the 16-entry list in scratch beside the walk's stack and
    with the smallest scratch list (K = 5).  A walk that follows its bound takes fewer trips than one that must meet every triangle (count_all): a
    bestn that stops following the K-th d2 still answers right, and fails here."""
    ref, ns = KS.deep_set(prec), N.scan_of("s4_4", prec)
    v = ref["valid"]
    with _open(gpu, N.scene("s4_4"), prec) as h:
        t16 = _check(h, ref, 16)
        t5 = _check(h, ref, 5)
        tall = _check(h, ref, 16, count_all=True)
    for t in (t16, t5, tall):
        _same_walk(t)
    print(prec, "mean trips of valid points: K = 5 %.1f, K = 16 %.1f, COUNT_ALL %.1f of %d triangles" % (t5[0][v].mean(), t16[0][v].mean(), tall[0][v].mean(), len(ns.tri)))
    assert (tall[0][v] > len(ns.tri)).all() and not t16[0][~v].any()
    assert t16[0][v].mean() < tall[0][v].mean()
    assert t5[0][v].mean() <= t16[0][v].mean()                       # the 5th d2 of what was met is never beyond the 16th: K = 5 prunes no less


# ------------------------------------------------------------------------------------------------ 6: output subsets at capacity 16
@pytest.mark.parametrize("prec", PRECS)
def test_output_subsets_on_the_pile(gpu, prec):
    """The device form on a non-default stream at K = 16, each of the four output pointers NULL in turn: capacity 16 keeps a record index per entry and
    computes q again at the store — with `point` absent that code must not run, with it present and `dist` or `prim` absent it must not depend on them."""
    import torch
    ref = KS.pile_ref(prec)
    K, n = 16, len(ref["points"])
    tdt = torch.float32 if prec == "f32" else torch.float64
    d_pts = torch.tensor(ref["points"], dtype=tdt, device="cuda:0").contiguous()
    want = KS.cut(ref, K)
    st = torch.cuda.Stream()
    torch.cuda.synchronize()
    with _open(gpu, KS.pile_scene(), prec) as h:
        for ip in (False, True):
            for skip in (None, 0, 1, 2, 3):
                outs = [torch.full((n, K), -7, dtype=torch.int32, device="cuda:0"), torch.full((n, K), -7, dtype=tdt, device="cuda:0"),
                        torch.full((n, K, 3), -7, dtype=tdt, device="cuda:0"), torch.full((n,), -7, dtype=torch.int32, device="cuda:0")]
                ptrs = [0 if k == skip else o.data_ptr() for k, o in enumerate(outs)]
                torch.cuda.synchronize()
                h.nearest_k_device(d_pts.data_ptr(), n, K, ptrs[0], ptrs[1], ptrs[2], ptrs[3], st.cuda_stream, inplace=ip)
                st.synchronize()
                for k, o in enumerate(outs):
                    got = o.cpu().numpy()
                    if k == skip:
                        assert (got == -7).all(), (ip, skip)
                    else:
                        assert np.array_equal(_bits(got), _bits(want[k].astype(got.dtype))), (ip, skip, k)
