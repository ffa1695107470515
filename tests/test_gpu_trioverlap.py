"""GPU: spira_scene_overlap_tri_* / spira_scene_overlap_tri_any_* (spira_trioverlap.h: k_trioverlap, k_trioverlap_session) against the brute-force scan over
the numpy twins (tests/trioverlap_support.py).  The leaf test is the scan's own function on the record's own values and the tree only prunes, so out_prim,
out_count and out_hit are compared byte for byte in both precisions, for the refilled sessions and for SPIRA_CAST_INPLACE, for the host and the device form.

The query set of a scene (trioverlap_support.build_set, about 1 900 triangles — several waves with ranges beyond 128 queries, so the sessions refill): small
triangles straddling the surface; the scene's own triangles shifted in their plane, and copies sharing exactly a vertex or an edge; large triangles slicing
the whole mesh in the planes that cut the most objects (counts above 16); needles and tiny far triangles; vertices at 60 .. 64 frame units with twins just
beyond the origin rule; every invalid kind interleaved every 7th with valid neighbours; the tenth value of every third query NaN."""
import functools

import numpy as np
import pytest

import cast_support as S
import trioverlap_support as W
from spira_hip import query

pytestmark = pytest.mark.gpu
KS = (0, 1, 4, 5, 16)


def _open(gpu, scene, prec):
    return gpu.Scene(scene["spheres5"] if len(scene["spheres5"]) else None, scene["materials8"], scene["triangles10"], prec)


def _poison(h, n, k):
    """The host form stages its outputs in a workspace that outlives the call: n invalid queries (NaN) leave -3 / 0 and 255 in every staged element first,
    so an element the next call fails to write cannot pass for a right answer left over from the call before."""
    bad = np.full((n, 10), np.nan)
    prim, count, _ = h.overlap_tri(bad, max(k, 1))
    assert prim[0, 0] == -3 and prim[-1, -1] == -3 and not count.any()
    hit = h.overlap_tri_any(bad)
    assert hit[0] == 255 and hit[-1] == 255


def _check(h, ref, pick=None, inplace=(False, True), ks=KS, tris=None):
    """One handle against the scan: lists, counts and the any form under both organisations.  Returns the trips of each."""
    if tris is None:
        tris = ref["tris"] if pick is None else ref["tris"][pick]
    sub = ref if pick is None else dict(cand=ref["cand"][pick], valid=ref["valid"][pick])
    count = ref["count"] if pick is None else ref["count"][pick]
    want_hit = ref["hit"] if pick is None else ref["hit"][pick]
    trips = []
    for ip in inplace:
        for k in ks:
            _poison(h, len(tris), k)
            g_prim, g_count, g_trips = h.overlap_tri(tris, k, inplace=ip, want_trips=True)
            assert g_count.dtype == np.uint32 and np.array_equal(g_count, count), (ip, k, np.flatnonzero(g_count != count)[:6])
            if k == 0:
                assert g_prim is None
            else:
                want = W.lists(sub, k)
                bad = np.flatnonzero((g_prim != want).any(axis=1))
                assert g_prim.dtype == np.int32 and g_prim.shape == want.shape and len(bad) == 0, (ip, k, len(bad), bad[:4], g_prim[bad[:4]], want[bad[:4]])
        _poison(h, len(tris), 1)
        g_hit = h.overlap_tri_any(tris, inplace=ip)
        bad = np.flatnonzero(g_hit != want_hit)
        assert len(bad) == 0, (ip, "any", len(bad), bad[:6], g_hit[bad[:6]], want_hit[bad[:6]])
        trips.append(g_trips)
    return trips


@pytest.mark.parametrize("prec", ["f32", "f64"])
@pytest.mark.parametrize("name", ["ico20", "ico33", "torus"])
def test_against_the_scan(gpu, name, prec):
    """3 spheres + 20 triangles (no tree: the LDS scan), 2 spheres + 33 triangles (the smallest tree), the torus of 2 048 triangles + 3 spheres."""
    ref, ss = W.reference(name, prec), W.scan_of(name, prec)
    assert (ss.frame is not None) == (name != "ico20")
    W.conditions(ref)
    with _open(gpu, W.scene(name), prec) as h:
        trips = _check(h, ref)
    for t in trips:
        if ss.frame is None:
            assert not t.any()                                       # no tree: no trips
        else:
            assert t[ref["valid"]].min() >= 1 and not t[~ref["valid"]].any()
            assert t[ref["cand"][:, ss.ns:].any(axis=1)].min() >= 2  # a triangle candidate: at least the root and its leaf test
    if ss.frame is not None:
        assert np.array_equal(trips[0], trips[1])                    # the same walk, whatever the organisation


@pytest.mark.parametrize("how", ["none", "update", "rebuild"])
@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_device_form_on_another_stream_equals_the_host_form(gpu, prec, how):
    """Torch tensors on a non-default stream; after a device-form update or rebuild enqueued on ANOTHER stream the query sees the new tree with no host
    synchronisation in between; then each output pointer NULL in turn."""
    import torch
    if how == "none":
        A = B = W.scene("torus")
        ref = W.reference("torus", prec)
    else:
        A, B, _, ref = _moved(prec, how)
    tdt = torch.float32 if prec == "f32" else torch.float64
    d_tri = torch.tensor(B["triangles10"], dtype=tdt, device="cuda:0").contiguous()
    with np.errstate(over="ignore"):
        d_q = torch.tensor(np.asarray(ref["tris"], dtype=S.dtype_of(prec)), device="cuda:0").contiguous()
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()
    n = len(ref["tris"])
    with _open(gpu, A, prec) as h:
        if how != "none":
            (h.update_device if how == "update" else h.rebuild_device)(d_tri, s1)
        for ip in (False, True):
            for k in (0, 4, 16):
                prim, count, trips = query.overlap_triangles(h, d_q, k, inplace=ip, want_trips=True, stream=s2)
                hit = query.overlap_triangles(h, d_q, 0, any=True, inplace=ip, stream=s2)
                s2.synchronize()
                assert np.array_equal(count.cpu().numpy().astype(np.uint32), ref["count"]), (ip, k)
                assert np.array_equal(hit.cpu().numpy(), ref["hit"]), (ip, k)
                assert (prim is None) if k == 0 else np.array_equal(prim.cpu().numpy(), W.lists(ref, k)), (ip, k)
        h_prim, h_count, h_trips = h.overlap_tri(ref["tris"], 16, want_trips=True)
        assert np.array_equal(h_prim, prim.cpu().numpy()) and np.array_equal(h_count, count.cpu().numpy().astype(np.uint32))
        assert np.array_equal(h_trips, trips.cpu().numpy().astype(np.uint32))
        want = (W.lists(ref, 4), ref["count"].astype(np.int32))
        for skip in range(2):
            outs = [torch.full((n, 4), -7, dtype=torch.int32, device="cuda:0"), torch.full((n,), -7, dtype=torch.int32, device="cuda:0")]
            ptrs = [0 if k == skip else o.data_ptr() for k, o in enumerate(outs)]
            h.overlap_tri_device(d_q.data_ptr(), n, 4, ptrs[0], ptrs[1], s2.cuda_stream)
            s2.synchronize()
            for k in range(2):
                got = outs[k].cpu().numpy()
                assert (got == -7).all() if k == skip else np.array_equal(got, want[k]), (skip, k)


@pytest.mark.parametrize("prec", ["f32", "f64"])
@pytest.mark.parametrize("n", [1, 63, 65])
def test_ragged_sizes(gpu, prec, n):
    ref = W.reference("ico33", prec)
    pick = np.arange(n) * 37 % len(ref["tris"])                      # queries of every kind
    with _open(gpu, W.scene("ico33"), prec) as h:
        _check(h, ref, pick=pick)


@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_invalid_queries_never_disturb_their_neighbours(gpu, prec):
    ref, ss = W.reference("torus", prec), W.scan_of("torus", prec)
    at = ref["invalid_at"]
    assert len(at) >= len(W.invalid_kinds(ss.T, ss.frame))
    with _open(gpu, W.scene("torus"), prec) as h:
        for ip in (False, True):
            prim, count, trips = h.overlap_tri(ref["tris"], 4, inplace=ip, want_trips=True)
            assert (prim[at] == -3).all() and not count[at].any() and not trips[at].any()
            assert np.array_equal(count[at[:-1] + 1], ref["count"][at[:-1] + 1]) and (prim[at[:-1] + 1] != -3).all()
            hit = h.overlap_tri_any(ref["tris"], inplace=ip)
            assert (hit[at] == 255).all() and (hit[at[:-1] + 1] != 255).all()


@pytest.mark.parametrize("refill", [1, 8])
@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_session_refills_several_times(gpu, prec, refill):
    """k_trioverlap_session against its in-place twin and the scan on the smallest tree with the knobs the cast tests use: SPIRA_CAST_WAVES_PER_CU 1 and 128
    queries per wave at the least leave 4 waves of about 250 queries of 999 (rem = 3: ranges of base + 1 too); a small SPIRA_CAST_REFILL refills each wave
    many times."""
    from test_gpu_bvh import _with_env
    ref = W.reference("ico33", prec)
    n = 999
    pick = np.arange(n) * 37 % len(ref["tris"])

    def go():
        plan = gpu.cast_plan(n, 256)
        assert plan["refill_free"] == refill and plan["base"] > 64 and plan["base"] * plan["waves"] + plan["rem"] == n and plan["rem"] != 0, plan
        with _open(gpu, W.scene("ico33"), prec) as h:
            t_session, t_inplace = _check(h, ref, pick=pick, ks=(0, 4, 16))
        return t_session, t_inplace
    t_session, t_inplace = _with_env(gpu, {"SPIRA_CAST_REFILL": str(refill), "SPIRA_CAST_WAVES_PER_CU": "1"}, go)
    assert np.array_equal(t_session, t_inplace) and (t_session >= 2).sum() > n // 4          # lanes that walked


@functools.lru_cache(maxsize=None)
def _moved(prec, how):
    """The torus as built (A) and twisted (test_gpu_refit.deform); how = update: the validity frame stays the creation frame; rebuild: twisted, then scaled
    by 1.7 and moved, the frame is the fresh build's of that mesh.  Returns (A, B, the scan of B in the frame that holds, its query set)."""
    from test_gpu_refit import deform
    A = W.scene("torus")
    tri = np.array(deform(A["triangles10"]))
    if how == "rebuild":
        for v in range(3):
            tri[:, 3 * v:3 * v + 3] = tri[:, 3 * v:3 * v + 3] * 1.7 + np.array([0.5, -0.25, 1.0])
    B = dict(A, triangles10=tri)
    frame = S.mesh_frame(A["triangles10"], prec) if how == "update" else S.mesh_frame(tri, prec)
    ss = W.TriScan(B, prec, frame=frame)
    return A, B, ss, W.build_set(ss, B, seed=193, n_straddle=420, n_shift=96, n_share=96, n_slice=16, n_needle=64, n_far=24, n_mixed=70)


@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_the_same_handle_after_update_and_after_rebuild(gpu, prec):
    """The torus as built, the same handle after an update with a twist (the refitted tree) and after a rebuild (the Morton-order tree, a new frame): the
    answers are the scan's of the new mesh and, byte for byte, a fresh handle's."""
    A, B_up, _, ref_up = _moved(prec, "update")
    _, B_re, _, ref_re = _moved(prec, "rebuild")
    far = ref_re["valid"][ref_re["parts"]["far"]]
    assert far[0::2].all() and not far[1::2].any()
    with _open(gpu, A, prec) as h:
        _check(h, W.reference("torus", prec), ks=(4,))
        h.update(triangles10=B_up["triangles10"])
        _check(h, ref_up, ks=(0, 5, 16))
        h.rebuild(triangles10=B_re["triangles10"])
        _check(h, ref_re, ks=(0, 5, 16))
        prim, count, _ = h.overlap_tri(ref_re["tris"], 16)
        hit = h.overlap_tri_any(ref_re["tris"])
    with _open(gpu, B_re, prec) as fresh:
        f_prim, f_count, _ = fresh.overlap_tri(ref_re["tris"], 16)
        assert prim.tobytes() == f_prim.tobytes() and count.tobytes() == f_count.tobytes() and hit.tobytes() == fresh.overlap_tri_any(ref_re["tris"]).tobytes()


@pytest.mark.parametrize("prec", ["f32", "f64"])
@pytest.mark.parametrize("name", ["ico33", "torus"])
def test_a_mesh_against_itself(gpu, name, prec):
    """The scene's own triangles10 as the query list, untouched, and a copy whose mat column is NaN: every query lists itself, every answer is the scan's,
    and the pair list and the verdict of spira_hip.query come from the same bytes."""
    sc, ss = W.scene(name), W.scan_of(name, prec)
    tris = sc["triangles10"]
    ref = ss.overlap(tris)
    assert ref["valid"].all() and ref["cand"][np.arange(len(tris)), ss.ns + np.arange(len(tris))].all()      # (exactly: u0 = 0, e = g)
    poisoned = np.array(tris, dtype=np.float64)
    poisoned[:, 9] = np.nan
    with _open(gpu, sc, prec) as h:
        _check(h, ref, ks=(0, 4, 16), tris=tris)
        _check(h, ref, ks=(16,), tris=poisoned)
        prim, count, _ = h.overlap_tri(poisoned, 16)
        assert ((prim == (ss.ns + np.arange(len(tris)))[:, None]).any(axis=1) | (count > 16)).all()
        pairs, over = query.mesh_pairs(h, tris, 16)
        want = W.lists(ref, 16)
        qi, slot = np.nonzero(want >= 0)
        assert np.array_equal(pairs, np.stack([qi, want[qi, slot]], axis=1)) and np.array_equal(over, ref["count"] > 16)
        assert query.meshes_intersect(h, tris) is True
        away = np.array(tris, dtype=np.float64)
        away[:, :9] += np.tile(np.array([0.0, 3.0 * S.target_box(sc)[3], 0.0]), 3)
        top = max(float(tris[:, 1:9:3].max()), float((sc["spheres5"][:, 1] + sc["spheres5"][:, 3]).max()))
        assert away[:, 1:9:3].min() > top + 1.0 and query.meshes_intersect(h, away) is False      # beyond everything along y: the world axis rejects
