"""CPU: the ray sets of tests/test_gpu_cast_edges.py reach what they are for — asserted from the reference scan's answers alone (tests/cast_support.py),
in both precisions and with fixed seeds, before any device is involved.  Every assertion is a condition on the inputs of the device tests, not a
measurement: origins at 60 .. 64 normalised units that are valid and still hit the mesh, their twins just beyond the bound that are not, axis-parallel
directions that keep their signed zeros through the preparation, rays in the planes of axis-aligned squares, duplicate triangles whose later copy wins.
The sets are built once per process in cast_support.py (lru_cache) and left unchanged; the device module uses the same ones."""
import numpy as np
import pytest

import cast_support as S
from spira_hip import query

def test_blob_scene_is_the_s4_objects():
    s = S.blob_scene(2)
    assert s["triangles10"].shape == (320, 10) and s["spheres5"].shape == (2, 5) and "camera12" not in s
    big = S.blob_scene(2, 1e3, (1.0, 2.0, 3.0))
    assert np.array_equal(big["triangles10"][:, 9], s["triangles10"][:, 9]) and np.array_equal(big["spheres5"][:, 3], s["spheres5"][:, 3] * 1e3)
    assert np.array_equal(big["triangles10"][:, 3:6], s["triangles10"][:, 3:6] * 1e3 + [1.0, 2.0, 3.0])
    assert np.array_equal(big["spheres5"][:, :3], s["spheres5"][:, :3] * 1e3 + [1.0, 2.0, 3.0])


@pytest.mark.parametrize("fi", range(len(S.FRAMES)))
@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_far_origins_are_valid_hit_the_mesh_and_their_twins_are_invalid(oracle, prec, fi):
    fs = S.far_set(prec, fi)
    sc, far = fs["sc"], fs["far"]
    T = sc.T
    centre, scale = np.asarray(sc.frame[0], dtype=T), T(sc.frame[1])
    x = np.abs((far["rays"][:, :3].astype(T) - centre) * scale)
    assert far["valid"].all() and (x <= 64).all() and (x.max(axis=1) >= 60).all() and not np.isin(far["prim"], [S.INVALID]).any()
    mesh = int((far["prim"] >= sc.ns).sum())
    print(prec, S.FRAMES[fi], "frame", sc.frame, "mesh hits of rays_far:", mesh, "of", S.N_FAR)
    assert 4 * mesh >= 3 * S.N_FAR
    # the twins differ from their rays in one coordinate alone and fail the origin rule, nothing else
    tw = fs["twins"]
    assert not tw["valid"].any() and (tw["prim"] == S.INVALID).all() and not tw["t"].any()
    assert ((tw["rays"] != far["rays"]).sum(axis=1) == 1).all() and query.normalize_rays(tw["rays"], T, None)[1].all()
    xt = np.abs((tw["rays"][:, :3].astype(T) - centre) * scale).max(axis=1)
    assert (xt > 64).all() and (xt < 64.001).all()
    # the windows
    sel = fs["sel"]
    assert len(sel) == S.N_WIN
    prim, t = far["prim"][sel], far["t"][sel]
    same, below, beyond, before, hit, behind = (fs[k] for k in ("same", "below", "beyond", "before", "hit", "behind"))
    for w in (same, below, beyond, before, hit, behind):
        assert w["valid"].all()
    assert np.array_equal(same["prim"], prim) and np.array_equal(same["t"], t)                    # a hit at exactly t_max counts
    assert (below["prim"] == S.MISS).all() and np.array_equal(below["t"], below["rays"][:, 7].astype(T))
    later = beyond["prim"] >= 0
    print("   beyond: hits", int(later.sum()), " before / behind: mesh hits", int((before["prim"] >= sc.ns).sum()), int((behind["prim"] >= sc.ns).sum()))
    assert (beyond["prim"] != prim).all() and later.sum() >= S.N_WIN // 2 and (beyond["t"][later] > t[later]).all()
    assert (before["rays"][:, 7] > 0).all() and (before["prim"] < sc.ns).all()                      # the window ends before the mesh's box
    assert np.array_equal(hit["prim"], prim) and np.array_equal(hit["t"], t)                       # t_min = t_max = t: the hit itself
    assert (behind["prim"] < sc.ns).all()                                                          # the window starts behind the mesh


@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_axis_rays_keep_their_signed_zeros_and_split_into_hits_and_misses(oracle, prec):
    a = S.axis_set(prec)
    sc, ax = a["sc"], a["axis"]
    U = np.uint32 if prec == "f32" else np.uint64
    assert ax["valid"].all() and len(ax["rays"]) == S.N_AXIS
    d = ax["prepared"][:, 4:7]
    assert np.array_equal(np.ascontiguousarray(d).view(U), np.ascontiguousarray(ax["rays"][:, 4:7].astype(sc.T)).view(U))      # +-e_k, the zeros' signs kept
    k = np.arange(S.N_AXIS) % 3
    assert (np.abs(d[np.arange(S.N_AXIS), k]) == 1).all() and (np.abs(d).sum(axis=1) == 1).all()
    assert np.signbit(d).sum() > S.N_AXIS and (d == 0).sum() == 2 * S.N_AXIS and 0 < (np.signbit(d) & (d == 0)).sum() < 2 * S.N_AXIS
    mesh, miss = int((ax["prim"] >= sc.ns).sum()), int((ax["prim"] < 0).sum())
    inside = int((ax["prim"][S.N_AXIS // 2:] >= sc.ns).sum())
    print(prec, "rays_axis: mesh hits", mesh, "misses", miss, "mesh hits of the half that starts inside the box", inside)
    assert 3 * mesh >= S.N_AXIS and 10 * miss >= S.N_AXIS and inside > 0


@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_rays_on_the_bounding_planes(oracle, prec):
    """These inputs pin pruning, not hits: an origin exactly on a bounding plane makes one slab distance of the root box 0, and a direction in the plane
    makes it 0 x Inf.  What the scan says (blob_scene(2), both precisions): every ray is valid; no ray that lies in a bounding plane touches the mesh — the
    plane holds one extreme vertex and no ray is aimed at it; no outward ray does; all 12 inward rays do."""
    a = S.axis_set(prec)
    sc, pl, kind = a["sc"], a["planes"], a["kind"]
    assert len(kind) == 48 and pl["valid"].all()
    lo, hi, _ = S._box_T(a["scene"], sc.T)
    o = pl["rays"][:, :3].astype(sc.T).astype(np.float64)
    on = np.array([o[i, i // 16] == (lo, hi)[(i // 8) % 2][i // 16] for i in range(48)])
    assert on.all()                                                                                # exactly on the plane, in T
    mesh = pl["prim"] >= sc.ns
    counts = [int(mesh[kind == k].sum()) for k in (S.PLANE_IN, S.PLANE_INWARD, S.PLANE_OUTWARD)]
    print(prec, "rays_on_planes: mesh hits in-plane / inward / outward:", counts, "of", [int((kind == k).sum()) for k in range(3)])
    assert counts[0] == 0 and counts[2] == 0 and counts[1] == 12


@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_quad_rays_hit_along_the_normal_and_split_in_the_plane(oracle, prec):
    q = S.quad_set(prec)
    sc, r = q["sc"], q["quads"]
    assert sc.ns == 0 and r["valid"].all() and len(r["rays"]) == 2 * S.N_QUADS
    d = r["prepared"][:, 4:7]
    assert (np.abs(d).sum(axis=1) == 1).all() and (np.signbit(d) & (d == 0)).sum() >= S.N_QUADS      # unit axis directions after a length of 2.5, -0.0 kept
    normal, plane = r["prim"][:S.N_QUADS], r["prim"][S.N_QUADS:]
    hit, miss = int((plane >= 0).sum()), int((plane < 0).sum())
    print(prec, "rays_quads: normal-axis hits", int((normal >= 0).sum()), "in-plane hits", hit, "misses", miss)
    assert (normal >= 0).all() and 4 * hit > S.N_QUADS and 4 * miss > S.N_QUADS
    far = q["axis_far"]
    assert far["valid"].all() and (far["prim"] >= 0).sum() >= S.N_AXIS // 4 and (far["prim"] < 0).sum() >= S.N_AXIS // 10
    x = np.abs((far["rays"][:S.N_AXIS // 2, :3].astype(sc.T) - np.asarray(sc.frame[0], dtype=sc.T)) * sc.T(sc.frame[1])).max(axis=1)
    assert (x >= 59).all() and (x <= 64).all()


@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_ties_go_to_the_later_copy(binding, oracle, prec):
    s = S.ties_set(prec)
    sc, pair, r = s["sc"], s["pair"], s["rays"]
    assert sc.ns == 0 and len(sc.tri) == 200 and np.array_equal(pair[pair], np.arange(200))
    assert np.array_equal(sc.tri[pair][:, :9], sc.tri[:, :9]) and (sc.tri[pair][:, 9] != sc.tri[:, 9]).all()
    hit = r["prim"] >= 0
    print(prec, "duplicate triangles: hits", int(hit.sum()), "of", S.N_TIES)
    assert r["valid"].all() and hit.sum() >= 50 and (r["prim"][hit] > pair[r["prim"][hit]]).all()
