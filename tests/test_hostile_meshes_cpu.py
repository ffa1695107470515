"""CPU: the premises of tests/test_gpu_hostile_meshes.py, asserted from the yardsticks alone (tests/hostile_support.py) before any device result is looked
at.  They are conditions, not measurements: where a mesh misses one, the mesh changes and the condition stays.

Every (mesh, precision, frame, query) set holds at least 100 items answered by a triangle, 30 valid items answered by nothing and 20 invalid ones; each
mesh's sets reach what makes the mesh hostile (collapsed triangles as winners where the query can return one and never where it cannot, the tiny cluster
and the rest, the needles, the last copy and the tie rule's order, many octaves); the host twin of the tree builds every mesh through both builders, the
geometric mesh at least 7 levels deep; and sweep_support.grazing draws what it drew before on every scene whose reference other tests hold."""
import numpy as np
import pytest

import cast_support as S
import hostile_support as X
import knearest_support as KS
import nearest_support as N
import sweep_support as W
import tree_twin_support as TW

PRECS = ["f32", "f64"]
FRAMES = [(n, "create") for n in X.MESHES] + [(n, "update") for n in X.UPDATES]      # rebuild shares create's set


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("name,how", FRAMES)
def test_every_set_mixes_winners_misses_and_invalid_items(name, how, prec):
    st = X.sets(name, prec, how)
    for q in X.QUERIES:
        tri, empty, invalid = X.winners(st, q)
        got = (int((tri >= 0).any(axis=1).sum()), int(empty.sum()), int(invalid.sum()))
        print(name, how, prec, q, "items %d: triangle winners %d, empty %d, invalid %d" % ((len(tri),) + got))
        assert got[0] >= 100 and got[1] >= 30 and got[2] >= 20, (q, got)
        assert len(tri) <= 640


def ns_of(st):
    return st["ns"]


def _rows_with(tri, mask):
    """Items with a winner among the triangles of `mask`."""
    return int((np.where(tri >= 0, mask[np.maximum(tri, 0)], False)).any(axis=1).sum())


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("how", ["create", "update"])
def test_zero_area_triangles_win_where_a_query_can_return_them(how, prec):
    st = X.sets("zero_area", prec, how)
    flat = X.zero_area_mask(X.mesh("zero_area"), S.dtype_of(prec))
    assert flat.sum() == 24
    for q in ("near", "knear", "sweep"):
        assert _rows_with(X.winners(st, q)[0], flat) >= 16, q
    assert _rows_with(X.winners(st, "cast")[0], flat) == 0           # the scan's |a| < 1e-8 excludes them
    # box overlap: spira_overlap.h makes a triangle whose computed normal is exactly 0 NO candidate, wherever it lies — so none is ever listed, although
    # the first 24 target boxes are centred on a point of a collapsed triangle each
    boxes = st["boxes"]
    assert not boxes["cand"][:, ns_of(st):][:, flat].any()
    at = np.arange(boxes["targets"].start, boxes["targets"].start + X.N_SPOTS)
    assert boxes["valid"][at].all() and np.array_equal(boxes["boxes"][at, :3].astype(S.dtype_of(prec)), X.spots("zero_area", prec)[0].astype(S.dtype_of(prec)))
    ns = st["ns"]
    assert not any(flat[k - ns] for c in st["hits"]["cands"] if c for _, k in c if k >= ns)
    assert not np.isnan(st["sweep"]["rays"][st["sweep"]["parts"]["graze"]]).any()      # grazing drew triangles with a normal


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("how", ["create", "update"])
def test_mixed_scales_answers_come_from_the_cluster_and_from_outside_it(how, prec):
    st = X.sets("mixed_scales", prec, how)
    cluster = (np.arange(160) % 2 == 0) & (np.arange(160) > 0)
    v = np.asarray(X.mesh("mixed_scales"))[:, :9].reshape(-1, 3)
    assert np.abs(v.reshape(160, 3, 3)[cluster] - X.CLUSTER_AT).max() < 1e-3 and (v.max(axis=0) - v.min(axis=0) == 1.0).all()
    for q in X.QUERIES:
        tri = X.winners(st, q)[0]
        assert _rows_with(tri, cluster) >= 16 and _rows_with(tri, ~cluster) >= 16, q


@pytest.mark.parametrize("prec", PRECS)
def test_needles_win_in_every_query(prec):
    st = X.sets("needles", prec, "create")
    needle = np.arange(96) % 3 == 0
    for q in X.QUERIES:
        assert _rows_with(X.winners(st, q)[0], needle) >= 16, q


@pytest.mark.parametrize("prec", PRECS)
def test_copies_answer_with_the_last_copy_and_in_the_tie_rules_order(prec):
    st = X.sets("copies", prec, "create")
    for q in ("cast", "near", "sweep"):
        tri = X.winners(st, q)[0]
        assert set(tri[tri >= 0].tolist()) == {199}, q
    prim = KS.cut(st["order"], 16)[0]
    ns = st["ns"]
    full = 0
    for row in prim:
        t = row[row >= ns] - ns
        assert np.array_equal(t, 199 - np.arange(len(t)))            # equal d2: index descending, from the last copy down
        full += len(t) >= 15
    assert full >= 100


@pytest.mark.parametrize("how", ["create", "update"])
def test_geometric_answers_come_from_many_octaves(how):
    alive = {p: X.surviving_clusters(p) for p in PRECS}
    print("geometric: clusters with a triangle of three distinct vertices: f32 %d, f64 %d" % (len(alive["f32"]), len(alive["f64"])))
    assert len(alive["f64"]) == X.N_CLUSTERS and 12 <= len(alive["f32"]) < len(alive["f64"])
    st = X.sets("geometric", "f64", how)
    for q in X.QUERIES:
        tri = X.winners(st, q)[0]
        clusters = np.unique(tri[tri >= 0] // 4)
        print(how, q, "winners from %d clusters" % len(clusters))
        # a ray's determinant a = e1 . (d x e2) is at most twice the area, about 0.04 * 4^-k in cluster k, and the scan takes no triangle with
        # |a| < 1e-8: no ray hits anything beyond cluster 10, however it is aimed.  Rays must still reach 8 octaves; every other query 12
        assert len(clusters) >= (8 if q in ("cast", "hits") else 12), q


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("name", X.MESHES + ("scrambled",))
def test_render_windows_meet_the_mesh(oracle, name, prec):
    """The paths the render-walk test starts meet at least 100 triangles per mesh, by the oracle alone."""
    s, r = X.render_scene(name), X.RENDER
    hits = 0
    for k, window in enumerate(X.RENDER_WINDOWS[name]):
        po = oracle.make_params(r["W"], r["H"], r["spp"], r["depth"], len(s["spheres5"]), len(s["materials8"]), len(s["triangles10"]), seed=r["seed"] + k)
        for i, j, smp in X.render_paths(k, window):
            cnt, prims, _, _, _ = oracle.trace_path(s["spheres5"], s["materials8"], s["triangles10"], s["camera12"], po, int(i), int(j), int(smp), prec)
            hits += int((prims[:cnt] >= len(s["spheres5"])).sum())
    print(name, prec, "triangle hits of %d paths: %d" % (3 * r["n"], hits))
    assert hits >= 100


# ------------------------------------------------------------------ the tree the walks will meet, from the host twin
@pytest.fixture(scope="module")
def dump(tmp_path_factory):
    d = tmp_path_factory.mktemp("hostile_twin")
    return d, TW.build_dump(d)


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("name", X.MESHES + ("scrambled",))
def test_both_builders_take_every_mesh(dump, name, prec):
    d, exe = dump
    first, target = X.poses(name, "rebuild" if name in X.MESHES else "update")
    chain = [("create", target), ("rebuild", first), ("rebuild", target)]
    if name in X.UPDATES:
        chain += [("create", first), ("update", target)]
    steps, _, _ = TW.run_dump(exe, d, name + "_" + prec, prec, 3, False, chain)
    assert [s.status for s in steps] == [0] * len(chain)
    sm = [TW.summary(s.blobs["summary"]) for s in steps]
    for kind, k in (("create", 0), ("rebuild", 2)) + ((("update", 4),) if name in X.UPDATES else ()):
        print("%s %s %s: depth %d, slots %d, level widths %s" % (name, prec, kind, sm[k].depth, sm[k].n_slots, TW.level_widths(sm[k])))
    assert all(s.n == len(target) for s in sm)
    floor = 7 if name == "geometric" else 3
    assert sm[0].depth >= floor and sm[2].depth >= floor, (sm[0].depth, sm[2].depth)
    if name in X.UPDATES:
        assert sm[4].depth == sm[3].depth and sm[4].n_slots == sm[3].n_slots      # a refit keeps the topology of the pose it was built on


# ------------------------------------------------------------------ sweep_support.grazing draws what it drew before
def _grazing_before(rng, sc, n):
    """sweep_support.grazing as it stood before it learned to leave out triangles without a normal, kept to compare with."""
    ext = S.target_box(sc)[3]
    tri = sc.get("triangles10")
    if tri is not None and len(tri):
        v = np.asarray(tri, dtype=np.float64)[rng.integers(0, len(tri), n), :9].reshape(-1, 3, 3)
        a = rng.uniform(0.05, 0.9, (n, 1)); b = rng.uniform(0.02, 0.95, (n, 1)) * (1 - a)
        p = v[:, 0] + a * (v[:, 1] - v[:, 0]) + b * (v[:, 2] - v[:, 0])
        nrm = np.cross(v[:, 1] - v[:, 0], v[:, 2] - v[:, 0])
    else:
        sp = np.asarray(sc["spheres5"], dtype=np.float64)
        sp = sp[sp[:, 3] < 10][rng.integers(0, (sp[:, 3] < 10).sum(), n)]
        nrm = S._unit(rng, n)
        p = sp[:, :3] + sp[:, 3:4] * nrm
    nrm = nrm / np.linalg.norm(nrm, axis=1)[:, None]
    tau = np.cross(nrm, S._unit(rng, n))
    tau /= np.linalg.norm(tau, axis=1)[:, None]
    r = rng.uniform(0.01, 0.10, n) * ext
    off = r * rng.uniform(0.9, 1.1, n) * np.where(rng.random(n) < 0.5, -1.0, 1.0)
    return W._rays(p + off[:, None] * nrm - 1.5 * ext * tau, 2.3 * tau, t_max=3.0 * ext), r


def _existing_scenes():
    import test_gpu_refit
    out = {name: N.scene(name) for name in N.SCENES}
    for fi in range(len(S.FRAMES)):
        A = S.blob_scene(2, *S.FRAMES[fi])
        out["frame%d" % fi] = A
        out["frame%d_moved" % fi] = dict(A, triangles10=test_gpu_refit.deform(A["triangles10"]))
    return out


def test_grazing_draws_what_it_drew_before_on_every_existing_scene():
    """The sweep references other tests hold (sweep_support.reference and the frame cases) are functions of grazing's output and of the generator's state
    after it: both are equal, byte for byte, to the former code's on every one of their scenes."""
    for name, sc in _existing_scenes().items():
        for seed, n in ((71, 256), (73, 96)):
            r0, r1 = np.random.default_rng(seed), np.random.default_rng(seed)
            was, now = _grazing_before(r0, sc, n), W.grazing(r1, sc, n)
            assert np.isfinite(was[0][:, :7]).all(), name
            assert was[0].tobytes() == now[0].tobytes() and was[1].tobytes() == now[1].tobytes(), name
            assert r0.bit_generator.state == r1.bit_generator.state, name
    with np.errstate(all="ignore"):
        was = _grazing_before(np.random.default_rng(71), X.scene_of(X.mesh("zero_area")), 48)
    assert np.isnan(was[0]).any()                                    # what the change is for
