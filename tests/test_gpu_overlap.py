"""GPU: spira_scene_overlap_box_* / spira_scene_overlap_any_* (spira_overlap.h: k_overlap, k_overlap_session) against the brute-force scan over the numpy
twins (tests/overlap_support.py).  The leaf test is the scan's own function on the record's own values and the tree only prunes, so out_prim, out_count and
out_hit are compared byte for byte in both precisions, for the refilled sessions and for SPIRA_CAST_INPLACE, for the host and the device form.

The box set of a scene (overlap_support.build_set, about 2 000 boxes — several waves with ranges beyond 128 boxes, so the sessions refill): small boxes at
the surface; boxes containing the whole mesh (every object a candidate, the count far above 16); flat and needle boxes; identity, quarter-turn and random
quaternions throughout; h = 0 on vertices and edge midpoints; centres at 60 .. 64 frame units with extents just under the bound and their twins just over
it, small boxes there with twins beyond the origin rule; every invalid kind interleaved every 7th with valid neighbours."""
import ctypes as C
import functools

import numpy as np
import pytest

import cast_support as S
import nearest_support as N
import overlap_support as V
from spira_hip import query

pytestmark = pytest.mark.gpu
KS = (0, 1, 4, 5, 16)


def _open(gpu, scene, prec):
    return gpu.Scene(scene["spheres5"] if len(scene["spheres5"]) else None, scene["materials8"], scene["triangles10"], prec)


def _poison(h, n, k):
    """The host form stages its outputs in a workspace that outlives the call: n invalid boxes (NaN) leave -3 / 0 and 255 in every staged element first, so
    an element the next call fails to write cannot pass for a right answer left over from the call before."""
    bad = np.full((n, 10), np.nan)
    prim, count, _ = h.overlap_box(bad, max(k, 1))
    assert prim[0, 0] == -3 and prim[-1, -1] == -3 and not count.any()
    hit = h.overlap_any(bad)
    assert hit[0] == 255 and hit[-1] == 255


def _check(h, ref, pick=None, inplace=(False, True), ks=KS):
    """One handle against the scan: lists, counts and the any form under both organisations.  Returns the trips of each."""
    boxes = ref["boxes"] if pick is None else ref["boxes"][pick]
    sub = ref if pick is None else dict(cand=ref["cand"][pick], valid=ref["valid"][pick])
    count = ref["count"] if pick is None else ref["count"][pick]
    want_hit = ref["hit"] if pick is None else ref["hit"][pick]
    trips = []
    for ip in inplace:
        for k in ks:
            _poison(h, len(boxes), k)
            g_prim, g_count, g_trips = h.overlap_box(boxes, k, inplace=ip, want_trips=True)
            assert g_count.dtype == np.uint32 and np.array_equal(g_count, count), (ip, k, np.flatnonzero(g_count != count)[:6])
            if k == 0:
                assert g_prim is None
            else:
                want = V.lists(sub, k)
                bad = np.flatnonzero((g_prim != want).any(axis=1))
                assert g_prim.dtype == np.int32 and g_prim.shape == want.shape and len(bad) == 0, (ip, k, len(bad), bad[:4], g_prim[bad[:4]], want[bad[:4]])
        _poison(h, len(boxes), 1)
        g_hit = h.overlap_any(boxes, inplace=ip)
        bad = np.flatnonzero(g_hit != want_hit)
        assert len(bad) == 0, (ip, "any", len(bad), bad[:6], g_hit[bad[:6]], want_hit[bad[:6]])
        trips.append(g_trips)
    return trips


@pytest.mark.parametrize("prec", ["f32", "f64"])
@pytest.mark.parametrize("name", ["ico20", "ico33", "torus"])
def test_against_the_scan(gpu, name, prec):
    """3 spheres + 20 triangles (no tree: the LDS scan), 2 spheres + 33 triangles (the smallest tree), the torus of 2 048 triangles + 3 spheres."""
    ref, ss = V.reference(name, prec), V.scan_of(name, prec)
    assert (ss.frame is not None) == (name != "ico20")
    assert (ref["count"] > 16).sum() >= 20 and (ref["count"] == 0).sum() > 100 and (~ref["valid"]).sum() >= 20 and ((ref["count"] > 0) & (ref["count"] <= 4)).sum() > 100
    with _open(gpu, V.scene(name), prec) as h:
        trips = _check(h, ref)
    for t in trips:
        if ss.frame is None:
            assert not t.any()                                       # no tree: no trips
        else:
            assert t[ref["valid"]].min() >= 1 and not t[~ref["valid"]].any()
            assert t[ref["cand"][:, ss.ns:].any(axis=1)].min() >= 2  # a triangle candidate: at least the root and its leaf test
    if ss.frame is not None:
        assert np.array_equal(trips[0], trips[1])                    # the same walk, whatever the organisation


@pytest.mark.parametrize("prec", ["f32", "f64"])
@pytest.mark.parametrize("n", [1, 63, 65])
def test_ragged_sizes(gpu, prec, n):
    ref = V.reference("ico33", prec)
    pick = np.arange(n) * 37 % len(ref["boxes"])                     # boxes of every kind
    with _open(gpu, V.scene("ico33"), prec) as h:
        _check(h, ref, pick=pick)


@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_invalid_boxes_never_disturb_their_neighbours(gpu, prec):
    ref, ss = V.reference("torus", prec), V.scan_of("torus", prec)
    at = ref["invalid_at"]
    assert len(at) >= len(V.invalid_kinds(ss.T, ss.frame))
    with _open(gpu, V.scene("torus"), prec) as h:
        for ip in (False, True):
            prim, count, trips = h.overlap_box(ref["boxes"], 4, inplace=ip, want_trips=True)
            assert (prim[at] == -3).all() and not count[at].any() and not trips[at].any()
            assert np.array_equal(count[at[:-1] + 1], ref["count"][at[:-1] + 1]) and (prim[at[:-1] + 1] != -3).all()
            hit = h.overlap_any(ref["boxes"], inplace=ip)
            assert (hit[at] == 255).all() and (hit[at[:-1] + 1] != 255).all()


@pytest.mark.parametrize("refill", [1, 8])
@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_session_refills_several_times(gpu, prec, refill):
    """k_overlap_session against its in-place twin and the scan on the smallest tree with the knobs the cast tests use: SPIRA_CAST_WAVES_PER_CU 1 and 128
    boxes per wave at the least leave 4 waves of about 250 boxes of 999 (rem = 3: ranges of base + 1 too); a small SPIRA_CAST_REFILL refills each wave many
    times."""
    from test_gpu_bvh import _with_env
    ref = V.reference("ico33", prec)
    n = 999
    pick = np.arange(n) * 37 % len(ref["boxes"])

    def go():
        plan = gpu.cast_plan(n, 256)
        assert plan["refill_free"] == refill and plan["base"] > 64 and plan["base"] * plan["waves"] + plan["rem"] == n and plan["rem"] != 0, plan
        with _open(gpu, V.scene("ico33"), prec) as h:
            t_session, t_inplace = _check(h, ref, pick=pick, ks=(0, 4, 16))
        return t_session, t_inplace
    t_session, t_inplace = _with_env(gpu, {"SPIRA_CAST_REFILL": str(refill), "SPIRA_CAST_WAVES_PER_CU": "1"}, go)
    assert np.array_equal(t_session, t_inplace) and (t_session >= 2).sum() > n // 4          # lanes that walked


@functools.lru_cache(maxsize=None)
def _moved(prec, how):
    """The torus as built (A) and twisted (test_gpu_refit.deform); how = update: the validity frame stays the creation frame; rebuild: twisted, then scaled
    by 1.7 and moved, the frame is the fresh build's of that mesh.  Returns (A, B, the scan of B in the frame that holds, its box set)."""
    from test_gpu_refit import deform
    A = V.scene("torus")
    tri = np.array(deform(A["triangles10"]))
    if how == "rebuild":
        for v in range(3):
            tri[:, 3 * v:3 * v + 3] = tri[:, 3 * v:3 * v + 3] * 1.7 + np.array([0.5, -0.25, 1.0])
    B = dict(A, triangles10=tri)
    frame = S.mesh_frame(A["triangles10"], prec) if how == "update" else S.mesh_frame(tri, prec)
    ss = V.OverlapScan(B, prec, frame=frame)
    return A, B, ss, V.build_set(ss, B, seed=93, n_surf=512, n_whole=8, n_thin=128, n_zero=64, n_far=16, n_small=24, n_mixed=70)


@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_the_same_handle_after_update_and_after_rebuild(gpu, prec):
    """The torus as built, the same handle after an update with a twist (the refitted tree) and after a rebuild (the Morton-order tree, a new frame)."""
    A, B_up, _, ref_up = _moved(prec, "update")
    _, B_re, _, ref_re = _moved(prec, "rebuild")
    far = ref_re["valid"][ref_re["parts"]["far"]]
    assert far[0::2].all() and not far[1::2].any()
    with _open(gpu, A, prec) as h:
        _check(h, V.reference("torus", prec), ks=(4,))
        h.update(triangles10=B_up["triangles10"])
        _check(h, ref_up, ks=(0, 5, 16))
        h.rebuild(triangles10=B_re["triangles10"])
        _check(h, ref_re, ks=(0, 5, 16))


@pytest.mark.parametrize("how", ["update", "rebuild"])
@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_device_form_sees_the_new_tree(gpu, prec, how):
    """The new tree on one stream, the query on another non-default one, no host synchronisation in between; then each output pointer NULL in turn."""
    import torch
    A, B, ss, ref = _moved(prec, how)
    before = V.OverlapScan(A, prec).overlap(ref["boxes"])
    assert not np.array_equal(before["count"], ref["count"])
    tdt = torch.float32 if prec == "f32" else torch.float64
    d_tri = torch.tensor(B["triangles10"], dtype=tdt, device="cuda:0").contiguous()
    d_boxes = torch.tensor(ref["boxes"], dtype=tdt, device="cuda:0").contiguous()
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()
    n = len(ref["boxes"])
    with _open(gpu, A, prec) as h:
        (h.update_device if how == "update" else h.rebuild_device)(d_tri, s1)
        for ip in (False, True):
            for k in (0, 4, 16):
                prim, count, trips = query.overlap_boxes(h, d_boxes, k, inplace=ip, want_trips=True, stream=s2)
                hit = query.overlap_boxes(h, d_boxes, 0, any=True, inplace=ip, stream=s2)
                s2.synchronize()
                assert np.array_equal(count.cpu().numpy().astype(np.uint32), ref["count"]), (ip, k)
                assert np.array_equal(hit.cpu().numpy(), ref["hit"]), (ip, k)
                assert (prim is None) if k == 0 else np.array_equal(prim.cpu().numpy(), V.lists(ref, k)), (ip, k)
        want = (V.lists(ref, 4), ref["count"].astype(np.int32))
        for skip in range(2):
            outs = [torch.full((n, 4), -7, dtype=torch.int32, device="cuda:0"), torch.full((n,), -7, dtype=torch.int32, device="cuda:0")]
            ptrs = [0 if k == skip else o.data_ptr() for k, o in enumerate(outs)]
            h.overlap_box_device(d_boxes.data_ptr(), n, 4, ptrs[0], ptrs[1], s2.cuda_stream)
            s2.synchronize()
            for k in range(2):
                got = outs[k].cpu().numpy()
                assert (got == -7).all() if k == skip else np.array_equal(got, want[k]), (skip, k)


@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_multi_device_handle_and_refusals(gpu, prec):
    ref = V.reference("ico33", prec)
    s = V.scene("ico33")
    with gpu.Scene(s["spheres5"], s["materials8"], s["triangles10"], prec, n_devices=1) as h:
        _check(h, ref, inplace=(False,), ks=(4,))
    other = "f64" if prec == "f32" else "f32"
    lib = gpu.lib()
    with np.errstate(over="ignore"):                                 # (Float64's invalid kinds overflow Float32)
        boxes = np.ascontiguousarray(ref["boxes"], dtype=S.dtype_of(other))
    out = np.zeros(16 * len(boxes), dtype=np.int32).ctypes.data_as(C.c_void_p)
    with _open(gpu, s, prec) as h:
        fn = getattr(lib, "spira_scene_overlap_box_" + other)
        assert fn(h._h, boxes.ctypes.data_as(C.c_void_p), C.c_uint32(len(boxes)), C.c_uint32(4), C.c_uint32(0), out, out, None) == -1 and b"other precision" in lib.spira_last_error()
        fn = getattr(lib, "spira_scene_overlap_any_" + other)
        assert fn(h._h, boxes.ctypes.data_as(C.c_void_p), C.c_uint32(len(boxes)), C.c_uint32(0), out) == -1 and b"other precision" in lib.spira_last_error()
        _check(h, ref, inplace=(False,), ks=(4,))                    # a following valid call still answers


@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_voxelize_equals_the_twin(gpu, prec):
    """An 8 x 8 x 8 surface voxelisation of the torus scene: the cells made on the device are voxel_boxes' and the grid is the twin scan's any form."""
    import torch
    sc, ss = V.scene("torus"), V.scan_of("torus", prec)
    lo, hi, _, _ = S.target_box(sc)
    lo, hi = lo - 0.13, hi + 0.21
    boxes = query.voxel_boxes(lo, hi, (8, 8, 8), ss.T)
    ref = ss.overlap(boxes.astype(np.float64))
    assert ref["valid"].all() and 0.2 < (ref["count"] > 0).mean() < 0.9
    with _open(gpu, sc, prec) as h:
        grid = query.voxelize(h, lo, hi, (8, 8, 8))
        torch.cuda.synchronize()
        assert grid.dtype == torch.bool and tuple(grid.shape) == (8, 8, 8)
        assert np.array_equal(grid.cpu().numpy().reshape(-1), ref["count"] > 0)
        assert np.array_equal(h.overlap_any(boxes), ref["hit"])
