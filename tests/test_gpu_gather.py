"""GPU: the hemisphere gather at surface points — spira_scene_gather_* (radiance sums), spira_scene_gather_visible_* (counts of unoccluded directions)
and spira_gather_rays_device_*.

Every number the gather gives is, by construction, what the existing entries give for the ray lists of gather_rays: the anchors compare by bytes with
Scene.radiance (one call per sample on the generated list) and with Scene.occluded (the count of zeros over the generated lists).  Two extremes need no
twin (open sky: every sample visible; inside the closed box: none).  The contracts of the entries — sample ranges, adding, chunks keyed by key0, pass
splits, one workgroup, both organisations, host against device form, invalid points, stream order — are all compared by bytes.  32-bit and 64-bit,
depth 6, the smallest scenes that reach every kernel: S1 (spheres), S2 (its LDS triangle), S3 (the closed box) and the 320-triangle mesh (a tree)."""
import functools

import numpy as np
import pytest

from spira_hip import bake, scenes

pytestmark = pytest.mark.gpu

DEPTH, SEED = 6, 3


@functools.lru_cache(maxsize=None)
def _scene(name):
    return {"s1": scenes.scene_s1, "s2": scenes.scene_s2, "s3": scenes.scene_s3, "s2_glass": scenes.scene_s2_glass,
            "mesh": lambda: scenes.scene_s4(level=2)}[name]()


def _handle(gpu, s, prec):
    return gpu.Scene(s["spheres5"], s["materials8"], s["triangles10"], prec=prec)


def _T(prec):
    return np.float32 if prec == "f32" else np.float64


def _sphere_points(sphere, n, rng, cap=1.0):
    """n points on a sphere [cx cy cz r ..] with outward normals, within `cap` radians of its top."""
    c, r = np.asarray(sphere[0:3], dtype=np.float64), float(sphere[3])
    th, ph = rng.uniform(0, cap, n), rng.uniform(0, 2 * np.pi, n)
    nrm = np.stack([np.sin(th) * np.cos(ph), np.cos(th), np.sin(th) * np.sin(ph)], axis=1)
    return np.concatenate([c + r * nrm, nrm * rng.uniform(0.5, 3.0, (n, 1))], axis=1)      # non-unit normals: the library normalises


@functools.lru_cache(maxsize=None)
def _points(name, n=None):
    """Sphere scenes: points on the ground sphere around the objects and on a small sphere, plus the triangles' centroids.  The mesh: triangle_points
    of its 320 triangles; with n, those lifted off the surface by three offsets and ground points, n in all."""
    s = _scene(name)
    rng = np.random.default_rng({"s1": 1, "s2": 2, "s3": 3, "s2_glass": 4, "mesh": 5}[name])
    tri = bake.triangle_points(s["triangles10"]) if s["triangles10"] is not None else np.zeros((0, 6))
    ground, small = s["spheres5"][0] if name != "s1" and name != "s3" else s["spheres5"][1], s["spheres5"][-1 if name == "mesh" else 2]
    if n is None:
        return np.concatenate([_sphere_points(ground, 40, rng, cap=0.03), _sphere_points(small, 40, rng, cap=np.pi), tri])
    lifted = [np.concatenate([tri[:, 0:3] + off * tri[:, 3:6], tri[:, 3:6]], axis=1) for off in (0.0, 0.01, 0.1)]
    pts = np.concatenate(lifted + [_sphere_points(ground, n - 3 * len(tri), rng, cap=0.03)])
    assert len(pts) == n
    return pts


def _radiance_twin(gpu, h, pts, spp, prec, sample0=0, key0=0, flags=0, sums=None):
    """zeros (or sums) plus, for every sample, Scene.radiance at one sample per ray along gather_rays' list."""
    sums = np.zeros((len(pts), 3), dtype=_T(prec)) if sums is None else sums
    valid = None
    for s in range(sample0, sample0 + spp):
        rays = gpu.gather_rays(pts, s, SEED, key0, prec)
        _, v = h.radiance(rays, 1, DEPTH, seed=SEED, sample0=s, key0=key0, flags=flags, sums=sums, want_valid=True)
        valid = v if valid is None else valid
        assert np.array_equal(v, valid)
    return sums, valid


def _visible_twin(gpu, h, pts, spp, prec, t_min, t_max, sample0=0, key0=0):
    T = _T(prec)
    counts = np.zeros(len(pts), dtype=np.uint32)
    valid = None
    for s in range(sample0, sample0 + spp):
        r6 = gpu.gather_rays(pts, s, SEED, key0, prec)
        r8 = np.concatenate([r6[:, 0:3], np.full((len(pts), 1), T(t_min)), r6[:, 3:6], np.full((len(pts), 1), T(t_max))], axis=1).astype(T)
        occ = h.occluded(r8)
        counts += (occ == 0).astype(np.uint32)
        v = (occ != 255).astype(np.uint8)
        valid = v if valid is None else valid
        assert np.array_equal(v, valid)                             # the origin rule reads the origin only: all samples of a point or none
    return counts, valid


# ---------------------------------------------------------------------------------- the anchors
@pytest.mark.parametrize("prec", ["f32", "f64"])
@pytest.mark.parametrize("name", ["s1", "s2", "s3", "mesh"])
def test_gather_is_radiance_along_the_generated_rays(gpu, name, prec):
    pts = _points(name)
    with _handle(gpu, _scene(name), prec) as h:
        got, valid = h.gather(pts, 4, DEPTH, seed=SEED, key0=1000, want_valid=True)
        want, v_want = _radiance_twin(gpu, h, pts, 4, prec, key0=1000)
        one, v_one = h.gather(pts, 1, DEPTH, seed=SEED, key0=1000, want_valid=True)      # the direct pass: the lanes add themselves
        first, _ = _radiance_twin(gpu, h, pts, 1, prec, key0=1000)
        irr = bake.irradiance(h, pts, 4, DEPTH, seed=SEED, key0=1000)
    assert got.dtype == _T(prec) and np.array_equal(got, want) and np.array_equal(valid, v_want) and valid.all()
    assert np.array_equal(one, first) and np.array_equal(v_one, v_want)
    assert np.array_equal(irr, (got * _T(prec)(np.pi)) / _T(prec)(4))
    assert np.isfinite(got).all() and got.max() > 0 and len(np.unique(got)) > 16


@pytest.mark.parametrize("flag,name", [("EXT_DIELECTRIC", "s2_glass"), ("EXT_SPECTRAL", "s1")])
def test_gather_with_an_extension(gpu, flag, name):
    prec, ext, pts = "f32", getattr(gpu, flag), _points(name)
    with _handle(gpu, _scene(name), prec) as h:
        got = h.gather(pts, 4, DEPTH, seed=SEED, flags=ext)
        want, _ = _radiance_twin(gpu, h, pts, 4, prec, flags=ext)
        plain = h.gather(pts, 4, DEPTH, seed=SEED)
    assert np.array_equal(got, want) and not np.array_equal(got, plain)


def _far_points(gpu, h, k=6):
    """k points 65 normalised units from the mesh's centre along +-x, +-y, +-z (beyond the ray queries' origin bound of 64), each followed by its twin at
    60 units; normals towards the mesh."""
    from test_gpu_cast import _device_frame
    centre, scale = _device_frame(gpu, h)
    out = []
    for a in range(k):
        e = np.zeros(3); e[a % 3] = 1.0 if a < 3 else -1.0
        for units in (65.0, 60.0):
            out.append(np.concatenate([centre + e * (units / scale), -e]))
    return np.array(out)


@pytest.mark.parametrize("prec", ["f32", "f64"])
@pytest.mark.parametrize("name,t_max", [("s2", np.inf), ("s2", 0.5), ("mesh", np.inf), ("mesh", 0.05), ("mesh", 0.5)])
def test_gather_visible_counts_what_occluded_answers_zero_for(gpu, name, t_max, prec):
    t_min = 1e-3
    with _handle(gpu, _scene(name), prec) as h:
        pts = _points(name)
        if name == "mesh":
            pts = np.concatenate([pts[:100], _far_points(gpu, h), pts[100:]])
        prefill = np.arange(len(pts), dtype=np.uint32) * 3 + 1
        got, valid = h.gather_visible(pts, 8, t_min=t_min, t_max=t_max, seed=SEED, key0=7, counts=prefill.copy(), want_valid=True)
        inpl, v_inpl = h.gather_visible(pts, 8, t_min=t_min, t_max=t_max, seed=SEED, key0=7, counts=prefill.copy(), want_valid=True, inplace=True)
        want, v_want = _visible_twin(gpu, h, pts, 8, prec, t_min, t_max, key0=7)
        ao = bake.ambient_occlusion(h, pts, 8, t_max, t_min=t_min, seed=SEED, key0=7)
    assert got.dtype == np.uint32 and np.array_equal(got, prefill + want) and np.array_equal(valid, v_want)
    assert np.array_equal(inpl, got) and np.array_equal(v_inpl, valid)
    assert np.array_equal(ao, want.astype(np.float64) / 8.0)
    print(name, prec, t_max, "histogram of the counts:", np.bincount(want, minlength=9))
    assert want.max() == 8 and (want.min() < 8 or t_max != np.inf)      # open sky above some points; with no t_max, the ground below others
    if name == "mesh":
        far, twin = np.arange(100, 112, 2), np.arange(101, 112, 2)
        assert not valid[far].any() and np.array_equal(got[far], prefill[far])        # beyond the bound: valid 0, the count untouched
        assert valid[twin].all() and (want[twin] > 0).any() and valid.sum() == len(pts) - 6
    else:
        assert valid.all()


@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_open_sky_is_all_visible_and_the_closed_box_is_all_occluded(gpu, prec):
    from test_gpu_cast import _device_frame
    up = np.array([[0.0, 50.0, -1.0, 0.0, 2.0, 0.0], [3.0, 40.0, 2.0, 0.1, 1.0, -0.1]])
    with _handle(gpu, _scene("s2"), prec) as h:
        assert np.array_equal(h.gather_visible(up, 64, seed=SEED), [64, 64])
    with _handle(gpu, _scene("mesh"), prec) as h:                                      # a tree: the point stays within the origin bound
        centre, scale = _device_frame(gpu, h)
        high = np.array([np.concatenate([centre + [0.0, 30.0 / scale, 0.0], [0.0, 1.0, 0.0]])])
        for inplace in (False, True):
            counts, valid = h.gather_visible(high, 64, seed=SEED, want_valid=True, inplace=inplace)
            assert counts[0] == 64 and valid[0] == 1
    inside = np.array([[3.0, 4.0, 3.0, 0.0, 1.0, 0.0], [-5.0, 7.0, -6.0, 1.0, -1.0, 0.5], [0.0, 2.5, 0.0, 0.0, 0.0, 1.0]])
    with _handle(gpu, _scene("s3"), prec) as h:
        counts, valid = h.gather_visible(inside, 64, t_max=np.inf, seed=SEED, want_valid=True)
        assert np.array_equal(counts, [0, 0, 0]) and valid.all()
        assert (h.gather_visible(inside, 64, t_max=0.5, seed=SEED) == 64).all()         # ... and nothing within half a unit of them


@pytest.mark.parametrize("refill", ["1", "64"])
@pytest.mark.parametrize("n_points,spp", [(125, 8), (111, 9)])
@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_visible_session_refills_at_both_ends_of_the_threshold(gpu, prec, n_points, spp, refill, monkeypatch):
    """k_gather_visible_session against its in-place twin, by bytes, on the smallest tree (the 33-triangle shell of tests/nearest_support.py) at the two ends
    of the walk loop's exit condition: SPIRA_CAST_REFILL 64 refills only when the whole wave is free, 1 after every finished lane.  SPIRA_CAST_WAVES_PER_CU 1
    and 128 items per wave at the least leave 4 waves of about 250 items: every wave refills.  125 x 8 = 1 000 items divide among them evenly; 111 x 9 = 999
    leave rem = 3, so the ranges of base + 1 items are walked as well.  Points on and off the shell, normals outward and inward: rays that miss the mesh's
    box, rays that walk and escape, rays that hit."""
    from nearest_support import ico_scene
    s = ico_scene(33)
    tri = bake.triangle_points(s["triangles10"])
    lifted = [np.concatenate([tri[:, 0:3] + off * tri[:, 3:6], sign * tri[:, 3:6]], axis=1) for off, sign in ((0.01, 1.0), (0.01, -1.0), (0.3, -1.0), (-0.3, 1.0))]
    pts = np.concatenate(lifted)[:n_points]
    n = n_points * spp
    monkeypatch.setenv("SPIRA_CAST_REFILL", refill)
    monkeypatch.setenv("SPIRA_CAST_WAVES_PER_CU", "1")
    plan = gpu.cast_plan(n, 256)
    assert plan["refill_free"] == int(refill) and plan["base"] > 64 and plan["base"] * plan["waves"] + plan["rem"] == n and (plan["rem"] != 0) == (n == 999), plan
    with _handle(gpu, s, prec) as h:
        got, valid = h.gather_visible(pts, spp, t_min=1e-3, seed=SEED, key0=7, want_valid=True)
        inpl, v_inpl = h.gather_visible(pts, spp, t_min=1e-3, seed=SEED, key0=7, want_valid=True, inplace=True)
    assert got.dtype == np.uint32 and got.tobytes() == inpl.tobytes() and valid.tobytes() == v_inpl.tobytes() and valid.all()
    assert got.max() == spp and got.min() < spp // 2                 # open sky above some points, the shell or the ground around others


# ---------------------------------------------------------------------------------- contracts, bitwise
@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_sample_ranges_passes_and_grids(gpu, prec, monkeypatch):
    pts = _points("mesh", 1000)
    with _handle(gpu, _scene("mesh"), prec) as h:
        pl = gpu.gather_plan(1000, 8, 256)
        assert pl["n_pass"] == 1 and pl["spp_pass"] == 8 and not pl["direct"] and pl["grid"] > 1
        one = h.gather(pts, 8, DEPTH, seed=SEED)
        vis = h.gather_visible(pts, 8, seed=SEED)
        part = h.gather(pts, 3, DEPTH, seed=SEED)
        h.gather(pts, 5, DEPTH, seed=SEED, sample0=3, sums=part)
        assert np.array_equal(part, one)                            # spp 8 = 3 + 5 through sample0
        vpart = h.gather_visible(pts, 3, seed=SEED)
        h.gather_visible(pts, 5, seed=SEED, sample0=3, counts=vpart)
        assert np.array_equal(vpart, vis)

        def both():
            return (np.array_equal(h.gather(pts, 8, DEPTH, seed=SEED), one) and np.array_equal(h.gather_visible(pts, 8, seed=SEED), vis)
                    and np.array_equal(h.gather_visible(pts, 8, seed=SEED, inplace=True), vis))
        monkeypatch.setenv("SPIRA_GATHER_MAX_ITEMS", "3000")        # 3 samples of 1000 points per pass: 3 + 3 + 2
        pl = gpu.gather_plan(1000, 8, 256)
        assert pl["n_pass"] == 3 and pl["spp_pass"] == 3 and pl["ws_entries"] == 3000
        assert both()
        monkeypatch.setenv("SPIRA_GATHER_MAX_ITEMS", "1000")        # one sample per pass: eight direct passes, no workspace
        pl = gpu.gather_plan(1000, 8, 256)
        assert pl["n_pass"] == 8 and pl["direct"] and pl["ws_entries"] == 0
        assert both()
        monkeypatch.delenv("SPIRA_GATHER_MAX_ITEMS")
        monkeypatch.setenv("SPIRA_GATHER_WAVES_PER_CU", "0")        # one workgroup: 8 000 items on 256 lanes, every lane regenerates / refills ~31 times
        assert gpu.gather_plan(1000, 8, 256)["grid"] == 1 and gpu.gather_plan(1000, 8, 256)["n_pass"] == 1
        assert both()
        monkeypatch.delenv("SPIRA_GATHER_WAVES_PER_CU")
    assert np.isfinite(one).all() and len(np.unique(one[:, 0])) > 500 and vis.max() == 8 and vis.min() < 4


@pytest.mark.parametrize("prec", ["f32", "f64"])
@pytest.mark.parametrize("name", ["s2", "mesh"])
def test_host_form_equals_device_form_and_sums_are_added(gpu, name, prec):
    import torch
    T = _T(prec)
    tdt = torch.float32 if prec == "f32" else torch.float64
    pts = (_points("mesh", 1000)[::4][:250] if name == "mesh" else _points(name)[:81]).astype(T)
    n = len(pts)
    prefill = np.random.default_rng(4).uniform(0, 2, (n, 3)).astype(T)
    cfill = np.arange(n, dtype=np.uint32) + 5
    with _handle(gpu, _scene(name), prec) as h:
        d_pts = torch.tensor(pts, dtype=tdt, device="cuda:0").contiguous()
        st = torch.cuda.Stream()
        for spp in (1, 5):
            fresh, valid = h.gather(pts, spp, DEPTH, seed=SEED, want_valid=True)
            d_sums = torch.zeros((n, 3), dtype=tdt, device="cuda:0")
            d_valid = torch.full((n,), 7, dtype=torch.uint8, device="cuda:0")
            torch.cuda.synchronize()
            h.gather_device(d_pts.data_ptr(), n, spp, DEPTH, d_sums.data_ptr(), seed=SEED, d_valid_ptr=d_valid.data_ptr(), stream_ptr=st.cuda_stream)
            st.synchronize()
            assert np.array_equal(d_sums.cpu().numpy(), fresh) and np.array_equal(d_valid.cpu().numpy(), valid) and valid.all()
            # sums are added to, not stored: a prefilled array plus the same samples, one addition per sample in order
            got = h.gather(pts, spp, DEPTH, seed=SEED, sums=prefill.copy())
            want = prefill.copy()
            for smp in range(spp):
                want = want + h.gather(pts, 1, DEPTH, seed=SEED, sample0=smp)
            assert np.array_equal(got, want) and not np.array_equal(got, fresh)
        for inplace in (False, True):
            counts, cvalid = h.gather_visible(pts, 8, t_max=0.5, seed=SEED, want_valid=True, inplace=inplace)
            d_counts = torch.tensor(cfill.astype(np.int64), device="cuda:0").to(torch.int32).contiguous()      # (uint32 storage, viewed as int32)
            d_valid = torch.full((n,), 7, dtype=torch.uint8, device="cuda:0")
            torch.cuda.synchronize()
            h.gather_visible_device(d_pts.data_ptr(), n, 8, d_counts.data_ptr(), t_max=0.5, seed=SEED, d_valid_ptr=d_valid.data_ptr(),
                                    stream_ptr=st.cuda_stream, inplace=inplace)
            st.synchronize()
            assert np.array_equal(d_counts.cpu().numpy().astype(np.uint32), cfill + counts) and np.array_equal(d_valid.cpu().numpy(), cvalid)
        # the generator's device form writes the host form's list
        for sample, key0 in ((0, 0), (9, 12345)):
            d_rays = torch.full((n, 6), -1.0, dtype=tdt, device="cuda:0")
            torch.cuda.synchronize()
            gpu.gather_rays_device(d_pts.data_ptr(), n, d_rays.data_ptr(), sample, SEED, key0, st.cuda_stream, prec)
            st.synchronize()
            assert np.array_equal(d_rays.cpu().numpy(), gpu.gather_rays(pts, sample, SEED, key0, prec))


@pytest.mark.parametrize("prec", ["f32", "f64"])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_chunks_of_the_point_list_keyed_by_key0(gpu, prec, n):
    pts = _points("mesh", 1000)
    with _handle(gpu, _scene("mesh"), prec) as h:
        whole = h.gather(pts, 2, DEPTH, seed=SEED)
        assert np.array_equal(h.gather(pts[:n], 2, DEPTH, seed=SEED), whole[:n])
        assert np.array_equal(h.gather(pts[n:], 2, DEPTH, seed=SEED, key0=n), whole[n:])      # the tail as a chunk of its own
        vis = h.gather_visible(pts, 8, seed=SEED)
        assert np.array_equal(h.gather_visible(pts[:n], 8, seed=SEED), vis[:n])
        assert np.array_equal(h.gather_visible(pts[n:], 8, seed=SEED, key0=n), vis[n:])


@pytest.mark.parametrize("prec", ["f32", "f64"])
@pytest.mark.parametrize("spp", [1, 3])
def test_invalid_points_interleaved(gpu, prec, spp):
    T = _T(prec)
    pts = _points("mesh", 1000)[::5].astype(T)                                        # 200 points
    tiny = np.sqrt(np.finfo(T).tiny) / 4                                              # n.n = 3 tiny^2 / 16 < the smallest normal
    kinds = [np.array([np.nan, 0, 0, 0, 1, 0]), np.array([0, 1, 0, 0, np.nan, 0]), np.array([np.inf, 0, 0, 0, 1, 0]), np.array([0, 1, 0, -np.inf, 0, 0]),
             np.array([0, 1, 0, 0, 0, 0]), np.array([0, 1, 0, tiny, tiny, tiny]), np.array([0, 1, 0, np.finfo(T).max, np.finfo(T).max, 0])]
    bad = np.array(pts)
    at = np.arange(3, 200, 9)
    assert len(at) >= 3 * len(kinds)
    for i, k in enumerate(at):
        bad[k] = kinds[i % len(kinds)].astype(T)
    ok = np.setdiff1d(np.arange(200), at)
    prefill = np.random.default_rng(8).uniform(0, 1, (200, 3)).astype(T)
    cfill = np.arange(200, dtype=np.uint32) + 11
    with _handle(gpu, _scene("mesh"), prec) as h:
        clean = h.gather(pts, spp, DEPTH, seed=SEED, sums=prefill.copy())
        got, valid = h.gather(bad, spp, DEPTH, seed=SEED, sums=prefill.copy(), want_valid=True)
        assert not valid[at].any() and valid[ok].all()
        assert np.array_equal(got[at], prefill[at])                                  # untouched
        assert np.array_equal(got[ok], clean[ok]) and not np.array_equal(clean[at], prefill[at])
        for inplace in (False, True):
            vclean = h.gather_visible(pts, 8 * spp, seed=SEED, counts=cfill.copy(), inplace=inplace)
            vgot, vvalid = h.gather_visible(bad, 8 * spp, seed=SEED, counts=cfill.copy(), want_valid=True, inplace=inplace)
            assert np.array_equal(vvalid, valid) and np.array_equal(vgot[at], cfill[at]) and np.array_equal(vgot[ok], vclean[ok])
            assert not np.array_equal(vclean[at], cfill[at])


@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_a_gather_after_update_device_on_another_stream_sees_the_moved_mesh(gpu, prec):
    import torch
    from test_gpu_refit import deform
    A = _scene("mesh")
    moved = dict(A, triangles10=deform(A["triangles10"]))
    tdt = torch.float32 if prec == "f32" else torch.float64
    pts = _points("mesh", 1000)[:600].astype(_T(prec))
    with _handle(gpu, moved, prec) as hb:
        want = hb.gather(pts, 2, DEPTH, seed=SEED)
        vwant = hb.gather_visible(pts, 8, seed=SEED)
    d_tri = torch.tensor(moved["triangles10"], dtype=tdt, device="cuda:0").contiguous()
    d_pts = torch.tensor(pts, dtype=tdt, device="cuda:0").contiguous()
    d_sums = torch.zeros((600, 3), dtype=tdt, device="cuda:0")
    d_counts = torch.zeros((600,), dtype=torch.int32, device="cuda:0")
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()
    with _handle(gpu, A, prec) as h:
        before = h.gather(pts, 2, DEPTH, seed=SEED)
        vbefore = h.gather_visible(pts, 8, seed=SEED)
        h.update_device(d_tri, s1)
        h.gather_device(d_pts.data_ptr(), 600, 2, DEPTH, d_sums.data_ptr(), seed=SEED, stream_ptr=s2.cuda_stream)
        h.gather_visible_device(d_pts.data_ptr(), 600, 8, d_counts.data_ptr(), seed=SEED, stream_ptr=s2.cuda_stream)
        s2.synchronize()
        got, vgot = d_sums.cpu().numpy(), d_counts.cpu().numpy().astype(np.uint32)
    assert np.array_equal(got, want) and not np.array_equal(got, before)
    assert np.array_equal(vgot, vwant) and not np.array_equal(vgot, vbefore)
