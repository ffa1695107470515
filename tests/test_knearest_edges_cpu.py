"""CPU: the point sets of tests/test_gpu_knearest_edges.py reach what they are for — asserted from the K-nearest yardstick alone (tests/knearest_support.py),
in both precisions and with fixed seeds, for every parameter the device tests use, before any device is involved, so that no device case can pass on an
empty premise.  Every assertion is a condition on the inputs of the device tests, not a measurement; every count is printed.  The sets are built once per
process in knearest_support.py (lru_cache) and left unchanged; the device module uses the same ones."""
import hashlib

import numpy as np
import pytest

import cast_support as S
import knearest_support as KS
import nearest_support as N

PRECS = ["f32", "f64"]
HOWS = ["create", "update", "rebuild"]
PILE_SHA256 = "122e7241e40ffa4fff8895076260973b16a88f20dddf147449ef25941f5dc5f2"


@pytest.mark.parametrize("how", HOWS)
@pytest.mark.parametrize("fi", range(len(S.FRAMES)))
@pytest.mark.parametrize("prec", PRECS)
def test_frame_cases_hold_every_kind_of_point(prec, fi, how):
    """The blob mesh (320 triangles, 2 spheres) in the four placements, as built, updated and rebuilt: points with more than K candidates, with fewer, with
    none and with ties across the K-th place at K = 4 and K = 16; every valid far point has every object as a candidate, every twin is invalid."""
    A, B, ns, pts, ref = KS.frame_case(prec, fi, how)
    m = ns.ns + len(ns.tri)
    assert m == 322 and (ns.frame is not None) and len(ref["points"]) == len(pts["points"])
    if how != "create":
        fa = S.mesh_frame(A["triangles10"], prec)
        same = np.array_equal(ns.frame[0], fa[0]) and ns.frame[1] == fa[1]
        assert same == (how == "update")                             # an update keeps the creation frame, a rebuild has its own
        assert not np.array_equal(A["triangles10"], B["triangles10"])
    for K in (4, 16):
        more, fewer, none, tied = KS.conditions(ref, K)
        print(prec, fi, how, "K", K, "more", more, "fewer", fewer, "none", none, "tied across the K-th place", tied)
        assert more >= 682 and fewer >= 35 and none >= 38 and tied >= 155
    far, twins = KS.far_valid(pts)
    assert len(far) == 48 and ref["valid"][far].all() and (ref["total"][far] == m).all() and not ref["valid"][twins].any()
    p1 = KS.cut(ref, 1)[0][:, 0]
    assert np.array_equal(p1, pts["prim"])                           # the order's head is the closest-point scan's answer on the same set


@pytest.mark.parametrize("K", [4, 16])
@pytest.mark.parametrize("fi", range(len(S.FRAMES)))
@pytest.mark.parametrize("prec", PRECS)
def test_far_edge_sets_put_r_max_at_the_kth_distance(prec, fi, K):
    """From the order alone, what edge_set asserts near the mesh: one ulp below the K-th distance always fills fewer than K slots; at it, at least K
    candidates remain on more than half the points (r_max * r_max rounds)."""
    e = KS.far_edge_set(prec, fi, K)
    t = e["total"].astype(np.int64)
    same, below = t[e["parts"]["same"]], t[e["parts"]["below"]]
    print(prec, fi, K, "same: >= K on", int((same >= K).sum()), "of", len(same), "below: K - 1 on", int((below == K - 1).sum()), "fewer on", int((below < K - 1).sum()))
    assert len(same) == len(below) == 48 and e["valid"].all()
    assert (below < K).all() and (same >= K).mean() > 0.5
    _, _, ns, _, _ = KS.frame_case(prec, fi, "create")
    centre, scale = ns.frame
    d_n = np.abs((e["points"][:, :3] - centre) * scale).max(axis=1)
    assert (d_n >= 59.9).all() and (d_n <= 64.0).all()               # 60 .. 64 frame units (60 before the origin was rounded to T)
    assert ((e["r_max"].astype(np.float64) * scale) ** 2 > 1000.0).all()      # d2 in normalised units: in the thousands


def test_pile_scene_keeps_its_bytes():
    sc = KS.pile_scene()
    tri = sc["triangles10"]
    assert tri.shape == (33 * KS.PILE_COPIES, 10) == (561, 10) and tri.dtype == np.float64 and len(sc["spheres5"]) == 1
    assert hashlib.sha256(np.ascontiguousarray(tri).tobytes()).hexdigest() == PILE_SHA256
    rows, counts = np.unique(tri, axis=0, return_counts=True)
    assert len(rows) == 33 and (counts == KS.PILE_COPIES).all() and KS.PILE_COPIES > KS.MAX_NEAR
    assert np.array_equal(rows, np.unique(N.ico_scene(33)["triangles10"], axis=0))
    assert not np.array_equal(tri[:33], N.ico_scene(33)["triangles10"])      # interleaved, not stacked
    assert S.mesh_frame(tri, "f32") is not None                      # a tree


@pytest.mark.parametrize("K", range(1, 17))
@pytest.mark.parametrize("prec", PRECS)
def test_pile_fills_every_list_with_one_distance(prec, K):
    ref = KS.pile_ref(prec)
    more, tied, run, none = KS.pile_conditions(ref, K)
    print(prec, "K", K, "more than K", more, "tied across the K-th place", tied, "one run of equal d2", run, "valid without a candidate", none)
    assert more >= 700 and (K == 1 or tied == more) and run >= 600 and none >= 32
    # the order among the copies: index descending
    prim, dist, point, count = KS.cut(ref, K)
    full = count == K
    eq = np.diff(ref["d2"][full, :K], axis=1) == 0
    assert (np.diff(prim[full], axis=1)[eq] < 0).all()


@pytest.mark.parametrize("prec", PRECS)
def test_pile_at_one_is_the_closest_point_scan(prec):
    ref, scan = KS.pile_ref(prec), KS.pile_set(prec)
    prim, dist, point, count = KS.cut(ref, 1)
    assert np.array_equal(prim[:, 0], scan["prim"]) and np.array_equal(dist[:, 0], scan["dist"]) and np.array_equal(point[:, 0], scan["point"])


@pytest.mark.parametrize("name", ["pile", "ico32"])
@pytest.mark.parametrize("prec", PRECS)
def test_extreme_radii_square_out_of_range(prec, name):
    T = S.dtype_of(prec)
    r = KS.extreme_radii(T)
    fi = np.finfo(T)
    with np.errstate(all="ignore"):
        assert np.isfinite(r["a"] * r["a"]) and np.nextafter(r["a"], T(np.inf)) == r["b"] and np.isinf(r["b"] * r["b"]) and np.isfinite(r["b"])
        assert r["c"] > 0 and r["c"] * r["c"] == 0 and 0 < r["d"] * r["d"] < fi.tiny
    e = KS.extreme_radius_set(name, prec)
    ns = KS.pile_scan(prec) if name == "pile" else N.scan_of(name, prec)
    m = ns.ns + len(ns.tri)
    t = e["total"].astype(np.int64)
    assert len(t) == 128 and e["valid"].all() and (ns.frame is not None) == (name == "pile")
    for key in "abcd":
        s = e["parts"][key]
        print(prec, name, key, "r_max", r[key], "candidates", int(t[s].min()), "..", int(t[s].max()), "points with some", int((t[s] > 0).sum()))
        assert (e["r_max"][s] == r[key]).all()
    for key in "ab":
        assert (t[e["parts"][key]] == m).all()
    for key in "cd":
        s = e["parts"][key]
        assert (t[s] > 0).any() and (t[s] == 0).any() and t[s].max() <= (102 if name == "pile" else 6)
        used = np.arange(KS.TOP)[None, :] < np.minimum(t[s], KS.TOP)[:, None]
        assert not e["d2"][s][used].any()                            # only the objects AT the point
    if name == "pile":
        assert (t[e["parts"]["c"]] % KS.PILE_COPIES == 0).all()      # 17 per coincident vertex
    # the closest-point scan on the same points: its answer is the order's head
    prim, dist, point, valid = ns.query(e["points"])
    k_prim, k_dist, k_point, _ = KS.cut(e, 1)
    assert valid.all() and np.array_equal(prim, k_prim[:, 0]) and np.array_equal(dist, k_dist[:, 0]) and np.array_equal(point, k_point[:, 0])
    miss = prim == N.MISS
    assert miss.any() and np.array_equal(dist[miss], e["r_max"][miss])          # a miss carries r_max back, the subnormal-squared one included
    assert (miss[e["parts"]["d"]]).any()


@pytest.mark.parametrize("prec", PRECS)
def test_deep_set(prec):
    d = KS.deep_set(prec)
    ns = N.scan_of("s4_4", prec)
    far = d["valid"][d["parts"]["far"]]
    assert len(ns.tri) == 5120 and len(d["points"]) == 256 and far[0::2].all() and not far[1::2].any()
    assert (d["total"][d["valid"]] == ns.ns + len(ns.tri)).all() and d["valid"].sum() == 240
