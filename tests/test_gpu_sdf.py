"""GPU: spira_scene_signed_distance_* (spira_sdf.h: k_sdf, k_sdf_session) against the yardstick of tests/sdf_support.py — nearest_support's scan for the
nearest surface, the oracle's triangle test on every triangle for the three rays, the vote and the sphere rule in numpy.  A leaf's distance and a ray's
candidate test are the scans' own functions on the records' own values and the tree only prunes, so prim, dist (sign bit included), point, inside and
crossings are compared bit for bit in both precisions, for the refilled sessions and SPIRA_CAST_INPLACE, in the host form and the device form.
tests/test_sdf_cpu.py holds the premises of the sets used here (ground truth on the convex mesh, both vote outcomes, the Lipschitz property)."""
import numpy as np
import pytest

import cast_support as S
import hits_support as H
import nearest_support as N
import sdf_support as D
from spira_hip import query

pytestmark = pytest.mark.gpu

PRECS = ["f32", "f64"]


def _open(gpu, scene, prec):
    return gpu.Scene(scene["spheres5"] if len(scene["spheres5"]) else None, scene["materials8"], scene.get("triangles10"), prec)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def _poison(h, n):
    """The host form stages its outputs in a workspace that outlives the call: n invalid points (NaN) leave -3 / 0 / 0 / 255 / 0 in every staged element
    first, so an element the next call fails to write cannot pass for a right answer left over from the call before."""
    prim, dist, point, inside, cr, _ = h.signed_distance(np.full((n, 4), np.nan), want_crossings=True, want_trips=True)
    assert (prim == -3).all() and (inside == 255).all() and not cr.any() and not dist.any() and not point.any()


def _equal(got, ref, sel=slice(None)):
    """prim, dist, point, inside, crossings of one call against the reference's rows `sel`, bit for bit."""
    prim, dist, point, inside, cr = got
    T = S.dtype_of(ref["scan"].prec)
    want = (ref["prim"][sel], ref["dist"][sel].astype(T), ref["point"][sel].astype(T), ref["inside"][sel], ref["crossings"][sel])
    assert prim.dtype == np.int32 and dist.dtype == T and point.dtype == T and inside.dtype == np.uint8
    bad = np.flatnonzero((prim != want[0]) | (_bits(dist) != _bits(want[1])) | (_bits(point) != _bits(want[2])).any(axis=1) | (inside != want[3])
                         | (cr.astype(np.uint32) != want[4]).any(axis=1))
    assert len(bad) == 0, (len(bad), bad[:4], prim[bad[:4]], want[0][bad[:4]], dist[bad[:4]], want[1][bad[:4]], inside[bad[:4]], want[3][bad[:4]], cr[bad[:4]], want[4][bad[:4]])


def _device_call(h, points, prec, inplace, want_trips=False):
    import torch
    tdt = torch.float32 if prec == "f32" else torch.float64
    d_pts = torch.tensor(points, dtype=tdt, device="cuda:0").contiguous()
    g = query.signed_distance(h, d_pts, inplace=inplace, want_crossings=True, want_trips=want_trips)
    torch.cuda.synchronize()
    out = [x.cpu().numpy() for x in g[:5]]
    out[4] = out[4].view(np.uint32)
    return out + [g[5].cpu().numpy().view(np.uint32) if want_trips else None]


def _check(h, ref, prec, sel=slice(None)):
    """One handle against the reference: sessions and in-place, host form and device form.  Returns the trips of the host calls."""
    pts = ref["points"][sel]
    trips = []
    for ip in (False, True):
        _poison(h, len(pts))
        g = h.signed_distance(pts, inplace=ip, want_crossings=True, want_trips=True)
        _equal(g[:5], ref, sel)
        trips.append(g[5])
        _equal(_device_call(h, pts, prec, ip)[:5], ref, sel)
    return trips


@pytest.mark.parametrize("prec", PRECS)
def test_blob_scene_against_the_yardstick(gpu, prec):
    """blob_scene(2): the mesh (a tree) plus the ground and light spheres, points inside the light sphere included; and the same points through
    closest_point on the same handle: prim and point equal, |dist| equal bit for bit."""
    ref = D.blob_ref(prec)
    with _open(gpu, ref["scene"], prec) as h:
        trips = _check(h, ref, prec)
        c_prim, c_dist, c_point, _ = h.closest_point(ref["points"])
        prim, dist, point, inside, _, _ = h.signed_distance(ref["points"])
    assert np.array_equal(prim, c_prim) and np.array_equal(_bits(point), _bits(c_point)) and np.array_equal(_bits(np.abs(dist)), _bits(np.abs(c_dist)))
    assert np.array_equal(np.signbit(dist), inside == 1) and (inside == 1).sum() >= 64 and (inside == 0).sum() >= 64
    v = ref["valid"]
    for t in trips:
        assert t[ref["prim"] >= ref["scan"].ns].min() >= 2 and not t[~v].any()      # a triangle winner was reached through the tree
    assert np.array_equal(trips[0], trips[1])                        # the same walks, whatever the organisation


@pytest.mark.parametrize("prec", PRECS)
def test_crossings_and_sign_against_the_existing_entries(gpu, prec):
    """out_crossings against cast_hits(count_all, K = 0) on a handle created from the triangles alone, with SKIPPED applied; the mesh's verdict against
    query.inside_mesh on that handle (a scene without spheres here, so inside is the mesh's verdict)."""
    ref = D.lipschitz_ref(prec)                                      # blob_scene(2)'s mesh alone
    pts = ref["points"]
    with _open(gpu, ref["scene"], prec) as h:
        counts = np.stack([query.count_hits(h, D.rays_of(pts[:, :3], j)) for j in range(3)], axis=1)
        votes = query.inside_mesh(h, pts[:, :3])
        _, _, _, inside, cr, _ = h.signed_distance(pts, want_crossings=True)
    assert np.array_equal(counts, ref["counts"])
    agree = (counts[:, 0] % 2) == (counts[:, 1] % 2)
    want = counts.astype(np.uint32)
    want[agree, 2] = D.SKIPPED
    assert np.array_equal(cr, want) and 16 <= agree.sum()
    assert np.array_equal(inside == 1, votes)
    full = D.blob_ref(prec)                                          # with the spheres: crossings still count triangles alone
    with _open(gpu, D.triangles_only(full["scene"]), prec) as h:
        counts = np.stack([query.count_hits(h, D.rays_of(full["points"][:, :3], j)) for j in range(3)], axis=1)
    assert np.array_equal(counts[full["valid"]], full["counts"][full["valid"]])


@pytest.mark.parametrize("prec", PRECS)
def test_lds_triangles_and_spheres_only(gpu, prec):
    """At most 32 triangles stay in LDS (no tree: sdf_count_local); a spheres-only scene has every slot SKIPPED and the sign from step 2 alone."""
    lds, sph = D.lds_ref(prec), D.spheres_ref(prec)
    with _open(gpu, lds["scene"], prec) as h:
        for t in _check(h, lds, prec):
            assert not t.any()                                       # no tree, no trips
    with _open(gpu, sph["scene"], prec) as h:
        _check(h, sph, prec)
        _, _, _, inside, cr, _ = h.signed_distance(sph["points"], want_crossings=True)
    v = sph["valid"]
    assert (cr[v] == D.SKIPPED).all() and not cr[~v].any()
    assert np.array_equal(inside[v] == 1, D.in_spheres(sph["scene"], S.dtype_of(prec), sph["points"][v, :3]))


@pytest.mark.parametrize("prec", PRECS)
def test_open_mesh_both_vote_outcomes(gpu, prec):
    """quad_scene with the set of test_sdf_cpu's (b): ray 2 walked for at least a quarter, SKIPPED for at least a quarter, in the GPU's own output."""
    ref = D.quad_ref(prec)
    with _open(gpu, ref["scene"], prec) as h:
        _check(h, ref, prec)
        cr = h.signed_distance(ref["points"], want_crossings=True)[4]
    sk = cr[:, 2] == D.SKIPPED
    assert sk.sum() >= 75 and (~sk).sum() >= 75
    assert ((cr[~sk, 0] ^ cr[~sk, 1]) & 1).all() and not ((cr[sk, 0] ^ cr[sk, 1]) & 1).any()


@pytest.mark.parametrize("how", ["create", "update", "rebuild"])
@pytest.mark.parametrize("fi", range(len(S.FRAMES)))
@pytest.mark.parametrize("prec", PRECS)
def test_frames_updates_and_rebuilds(gpu, prec, fi, how):
    """The four placements of cast_support.FRAMES, each as built, after an update and after a rebuild; far points stay valid, their twins are invalid."""
    A, B, ref = D.frame_case(prec, fi, how)
    assert (~ref["valid"]).sum() >= 10 and (ref["inside"] == 1).sum() >= 16 and (ref["inside"] == 0).sum() >= 16
    with _open(gpu, A, prec) as h:
        if how != "create":
            (h.update if how == "update" else h.rebuild)(triangles10=B["triangles10"])
        _check(h, ref, prec)


@pytest.mark.parametrize("prec", PRECS)
def test_invalid_points_never_disturb_their_neighbours(gpu, prec):
    """One invalid point per cause of nearest_point_prepare, interleaved with valid ones: -3, 0, 0, 255, crossings 0; the neighbours are the yardstick's."""
    ref = D.blob_ref(prec)
    at = ref["invalid_at"]
    assert len(at) >= len(N.invalid_kinds(S.dtype_of(prec), ref["scan"].frame)) == 10
    sel = slice(int(at[0]) - 3, len(ref["points"]))
    with _open(gpu, ref["scene"], prec) as h:
        _check(h, ref, prec, sel)
        prim, dist, point, inside, cr, trips = h.signed_distance(ref["points"], want_crossings=True, want_trips=True)
    assert (prim[at] == -3).all() and not dist[at].any() and not point[at].any() and (inside[at] == 255).all() and not cr[at].any() and not trips[at].any()


@pytest.mark.parametrize("refill", [1, 64])
@pytest.mark.parametrize("n", [1000, 999])
@pytest.mark.parametrize("prec", PRECS)
def test_phase_machine_under_refills_at_both_ends(gpu, prec, n, refill):
    """k_sdf_session at the two ends of the walk loop's exit condition: SPIRA_CAST_REFILL 64 refills only when the whole wave is free, 1 after every
    finished lane — lanes of one wave then sit in every phase at once.  SPIRA_CAST_WAVES_PER_CU 1 leaves 4 waves of about 250 points; 999 leaves rem = 3."""
    from test_gpu_bvh import _with_env
    ref = D.blob_ref(prec)
    pick = np.arange(n) * 37 % len(ref["points"])                    # points of every kind

    def go():
        plan = gpu.cast_plan(n, 256)
        assert plan["refill_free"] == refill and plan["base"] > 64 and plan["base"] * plan["waves"] + plan["rem"] == n and (plan["rem"] != 0) == (n == 999), plan
        with _open(gpu, ref["scene"], prec) as h:
            _poison(h, n)
            full = h.signed_distance(ref["points"][pick], want_crossings=True)
            _equal(full[:5], ref, pick)
            _poison(h, n)
            sign = h.signed_distance(ref["points"][pick], want_prim=False, want_dist=False, want_point=False, want_crossings=True)
            return full, sign
    full, sign = _with_env(gpu, {"SPIRA_CAST_REFILL": str(refill), "SPIRA_CAST_WAVES_PER_CU": "1"}, go)
    assert sign[0] is None and np.array_equal(sign[3], full[3]) and np.array_equal(sign[4], full[4])


@pytest.mark.parametrize("prec", PRECS)
def test_sign_only_form(gpu, prec):
    """out_prim, out_dist and out_point all NULL: no nearest walk (fewer trips), inside and crossings equal the full form's — sessions and in-place, host
    and device form, on the tree scene and the LDS scene; query.inside_points is that form."""
    import torch
    tdt = torch.float32 if prec == "f32" else torch.float64
    for ref in (D.blob_ref(prec), D.lds_ref(prec)):
        pts = ref["points"]
        with _open(gpu, ref["scene"], prec) as h:
            for ip in (False, True):
                full = h.signed_distance(pts, inplace=ip, want_crossings=True, want_trips=True)
                _poison(h, len(pts))
                sign = h.signed_distance(pts, inplace=ip, want_prim=False, want_dist=False, want_point=False, want_crossings=True, want_trips=True)
                assert sign[0] is None and sign[1] is None and sign[2] is None
                assert np.array_equal(sign[3], ref["inside"]) and np.array_equal(sign[4], ref["crossings"]) and np.array_equal(sign[3], full[3])
                if ref["scan"].frame is not None:
                    assert (sign[5] <= full[5]).all() and sign[5].sum() < full[5].sum()
                d_pts = torch.tensor(pts, dtype=tdt, device="cuda:0").contiguous()
                d_in = torch.full((len(pts),), 7, dtype=torch.uint8, device="cuda:0")
                d_cr = torch.full((len(pts), 3), 7, dtype=torch.int32, device="cuda:0")
                h.signed_distance_device(d_pts.data_ptr(), len(pts), 0, 0, 0, d_in.data_ptr(), torch.cuda.current_stream().cuda_stream, inplace=ip,
                                         d_crossings_ptr=d_cr.data_ptr())
                torch.cuda.synchronize()
                assert np.array_equal(d_in.cpu().numpy(), ref["inside"]) and np.array_equal(d_cr.cpu().numpy().view(np.uint32), ref["crossings"])
            assert np.array_equal(query.inside_points(h, pts[:, :3]), ref["inside"] == 1)
            assert np.array_equal(query.inside_points(h, d_pts).cpu().numpy(), ref["inside"] == 1)


@pytest.mark.parametrize("prec", PRECS)
def test_convex_ground_truth_and_lipschitz_on_the_device(gpu, prec):
    """The sets (a) and (c) of tests/test_sdf_cpu.py: on the icosphere the device's sign is |p - c| < r_in for all 400 points; on the closed blob mesh
    |sd(a) - sd(b)| <= |a - b| + tol for all 300 pairs, on the device's own distances."""
    conv, lip = D.convex_ref(prec), D.lipschitz_ref(prec)
    with _open(gpu, conv["scene"], prec) as h:
        _check(h, conv, prec)
        _, dist, _, inside, _, _ = h.signed_distance(conv["points"])
    assert np.array_equal(inside == 1, conv["truth"]) and np.array_equal(np.signbit(dist), conv["truth"])
    with _open(gpu, lip["scene"], prec) as h:
        _check(h, lip, prec)
        dist = h.signed_distance(lip["points"])[1]
    assert len(D.lipschitz_failures(lip["points"], dist, lip["tol"])) == 0


@pytest.mark.parametrize("band", [None, 0.05])
@pytest.mark.parametrize("prec", PRECS)
def test_distance_field_is_signed_distance_at_the_cell_centres(gpu, prec, band):
    """distance_field on an 8 x 8 x 8 grid equals signed_distance on voxel_boxes(...)[:, :3] with r_max = band (or +Inf); invalid cells are NaN."""
    import torch
    scene = S.blob_scene(2)
    T = S.dtype_of(prec)
    lo, hi, c, ext = S.target_box(scene)
    lo, hi = lo - 0.1 * ext, hi + 0.1 * ext
    dims = (8, 8, 8)
    cells = query.voxel_boxes(lo, hi, dims, T)[:, :3]
    pts = np.concatenate([cells, np.full((len(cells), 1), np.inf if band is None else T(band), dtype=T)], axis=1)
    with _open(gpu, scene, prec) as h:
        field = query.distance_field(h, lo, hi, dims, band=band)
        assert field.is_cuda and tuple(field.shape) == dims and field.dtype == (torch.float32 if prec == "f32" else torch.float64)
        field = field.cpu().numpy()
        _, dist, _, inside, _, _ = h.signed_distance(pts)
        assert np.array_equal(_bits(field.reshape(-1)), _bits(dist)) and (inside != 255).all()
        assert (dist < 0).sum() >= 8 and (dist > 0).sum() >= 64
        if band is not None:
            assert (np.abs(dist) == T(band)).sum() >= 64 and (np.abs(dist) < T(band)).sum() >= 4
        far = query.distance_field(h, lo + 200.0, hi + 200.0, (2, 2, 2), band=band).cpu().numpy()      # beyond the origin rule: invalid cells
        assert np.isnan(far).all()
