"""GPU: light probes — spira_scene_probe_sh_* (nine SH terms of the radiance arriving at free points) and spira_probe_rays_device_*.

Every number the probe entry gives is, by construction, what the existing entries give for the ray lists of probe_rays: the anchor compares by bytes with
Scene.radiance (one call per sample on the generated list) times bake.sh9 of cameras.ray_prepare's unit direction, added in sample order in T.  The
contracts of the entry — sample ranges, adding, chunks keyed by key0, pass splits, one workgroup, the direct pass, host against device form, invalid
points, stream order — are all compared by bytes.  One case needs no twin: under the open sky the coefficients are known in closed form (bands 0 and 1).
32-bit and 64-bit, depth 4, the scenes of test_gpu_gather.py: S1 (spheres), S2 (its LDS triangle), S3 (the closed box) and the 320-triangle mesh (a tree)."""
import numpy as np
import pytest

from spira_hip import bake, cameras
from test_gpu_gather import _T, _handle, _points, _scene

pytestmark = pytest.mark.gpu

DEPTH, SEED = 4, 3
_TWINS = {}


def _probes(name, n=200):
    """n free points: around the objects of a sphere scene (some inside a sphere, some below the ground: every one is a valid probe); for the mesh, points on
    its triangles, lifted off them by two offsets, and on the ground."""
    if name == "mesh":
        pts = _points("mesh", 1000)[:, 0:3]
        return np.ascontiguousarray(pts[np.linspace(0, len(pts) - 1, n).astype(int)])
    rng = np.random.default_rng({"s1": 11, "s2": 12, "s3": 13, "s2_glass": 14}[name])
    return rng.uniform([-2.5, -0.45, -3.0], [2.5, 3.0, 1.5], (n, 3))


def _twin(gpu, h, pts, spp, prec, sample0=0, key0=0, flags=0, start=None, depth=DEPTH):
    """start (or zeros) plus, for every sample in order, Scene.radiance at one sample per ray along probe_rays' list, times bake.sh9 of the unit direction
    cameras.ray_prepare gives for that list: one product, one addition, in T.  Rows of invalid points are left alone."""
    T = _T(prec)
    sums = np.zeros((len(pts), 9, 3), dtype=T) if start is None else start.copy()
    valid = None
    for s in range(sample0, sample0 + spp):
        rays = gpu.probe_rays(pts, s, SEED, key0, prec)
        L, v = h.radiance(rays, 1, depth, seed=SEED, sample0=s, key0=key0, flags=flags, want_valid=True)
        ok, d = cameras.ray_prepare(rays, prec)
        assert np.array_equal(v, ok.astype(np.uint8)) and L.dtype == T and d.dtype == T
        valid = v if valid is None else valid
        assert np.array_equal(v, valid)
        Y = bake.sh9(d)
        term = Y[:, :, None] * L[:, None, :]
        assert term.dtype == T
        keep = v.astype(bool)
        sums[keep] = sums[keep] + term[keep]
    return sums, valid


def _shared_twin(gpu, h, name, prec, spp):
    """The reference of the mesh contracts: computed once per precision and sample count, read by every test, never written."""
    key = (name, prec, spp)
    if key not in _TWINS:
        sums, valid = _twin(gpu, h, _probes(name), spp, prec)
        sums.setflags(write=False)
        _TWINS[key] = (sums, valid)
    return _TWINS[key]


# ---------------------------------------------------------------------------------- the anchor
@pytest.mark.parametrize("prec", ["f32", "f64"])
@pytest.mark.parametrize("name", ["s1", "s2", "s3", "mesh"])
def test_probe_sh_is_radiance_along_the_generated_rays_times_the_basis(gpu, name, prec):
    pts = _probes(name)
    with _handle(gpu, _scene(name), prec) as h:
        got, valid = h.probe_sh(pts, 5, DEPTH, seed=SEED, key0=1000, want_valid=True)
        want, v_want = _twin(gpu, h, pts, 5, prec, key0=1000)
        one, v_one = h.probe_sh(pts, 1, DEPTH, seed=SEED, key0=1000, want_valid=True)    # the direct pass: the lanes add themselves
        first, _ = _twin(gpu, h, pts, 1, prec, key0=1000)
        coeffs = bake.light_probes(h, pts, 5, DEPTH, seed=SEED, key0=1000)
    T = _T(prec)
    assert got.dtype == T and got.shape == (200, 9, 3) and np.array_equal(got, want) and np.array_equal(valid, v_want) and valid.all()
    assert np.array_equal(one, first) and np.array_equal(v_one, v_want)
    assert np.array_equal(coeffs, (got * T(4.0 * np.pi)) / T(5))
    assert np.isfinite(got).all() and got[:, 0].max() > 0 and len(np.unique(got)) > 100
    assert (got[:, 1:] < 0).any() and (got[:, 0] >= 0).all()                             # Y0 > 0 and L >= 0; the other bands change sign


@pytest.mark.parametrize("flag,name", [("EXT_DIELECTRIC", "s2_glass"), ("EXT_SPECTRAL", "s1")])
def test_probe_sh_with_an_extension(gpu, flag, name):
    prec, ext, pts = "f32", getattr(gpu, flag), _probes(name)
    with _handle(gpu, _scene(name), prec) as h:
        got = h.probe_sh(pts, 5, DEPTH, seed=SEED, flags=ext)
        want, _ = _twin(gpu, h, pts, 5, prec, flags=ext)
        plain = h.probe_sh(pts, 5, DEPTH, seed=SEED)
    assert np.array_equal(got, want) and not np.array_equal(got, plain)


# ---------------------------------------------------------------------------------- contracts, bitwise
@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_sample_ranges_passes_and_grids(gpu, prec, monkeypatch):
    pts = _probes("mesh")
    with _handle(gpu, _scene("mesh"), prec) as h:
        want, _ = _shared_twin(gpu, h, "mesh", prec, 9)
        pl = gpu.gather_plan(200, 9, 256)
        assert pl["n_pass"] == 1 and pl["spp_pass"] == 9 and not pl["direct"] and pl["grid"] > 1
        one = h.probe_sh(pts, 9, DEPTH, seed=SEED)
        assert np.array_equal(one, want)
        part = h.probe_sh(pts, 4, DEPTH, seed=SEED)
        h.probe_sh(pts, 5, DEPTH, seed=SEED, sample0=4, sums=part)
        assert np.array_equal(part, want)                           # spp 9 = 4 + 5 through sample0
        monkeypatch.setenv("SPIRA_GATHER_MAX_ITEMS", "600")         # 3 samples of 200 points per pass: 3 + 3 + 3
        pl = gpu.gather_plan(200, 9, 256)
        assert pl["n_pass"] == 3 and pl["spp_pass"] == 3 and pl["ws_entries"] == 600
        assert np.array_equal(h.probe_sh(pts, 9, DEPTH, seed=SEED), want)
        monkeypatch.setenv("SPIRA_GATHER_MAX_ITEMS", "1000")        # 5 per pass: 5 + 4
        pl = gpu.gather_plan(200, 9, 256)
        assert pl["n_pass"] == 2 and pl["spp_pass"] == 5
        assert np.array_equal(h.probe_sh(pts, 9, DEPTH, seed=SEED), want)
        monkeypatch.setenv("SPIRA_GATHER_MAX_ITEMS", "200")         # one sample per pass: nine direct passes, no workspace
        pl = gpu.gather_plan(200, 9, 256)
        assert pl["n_pass"] == 9 and pl["direct"] and pl["ws_entries"] == 0
        assert np.array_equal(h.probe_sh(pts, 9, DEPTH, seed=SEED), want)
        monkeypatch.delenv("SPIRA_GATHER_MAX_ITEMS")
        monkeypatch.setenv("SPIRA_GATHER_WAVES_PER_CU", "0")        # one workgroup: 1 800 items on 256 lanes, every lane regenerates ~7 times
        assert gpu.gather_plan(200, 9, 256)["grid"] == 1 and gpu.gather_plan(200, 9, 256)["n_pass"] == 1
        assert np.array_equal(h.probe_sh(pts, 9, DEPTH, seed=SEED), want)
        direct = h.probe_sh(pts, 1, DEPTH, seed=SEED)               # ... and the direct pass on one workgroup
        monkeypatch.delenv("SPIRA_GATHER_WAVES_PER_CU")
        first, _ = _shared_twin(gpu, h, "mesh", prec, 1)
        assert np.array_equal(direct, first) and np.array_equal(h.probe_sh(pts, 1, DEPTH, seed=SEED), first)      # spp 1: the lanes add themselves
    assert np.isfinite(want).all() and len(np.unique(want[:, 0, 0])) > 100


@pytest.mark.parametrize("prec", ["f32", "f64"])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_chunks_of_the_point_list_keyed_by_key0(gpu, prec, n):
    pts = _probes("mesh", 320)
    with _handle(gpu, _scene("mesh"), prec) as h:
        whole = h.probe_sh(pts, 2, DEPTH, seed=SEED)
        assert np.array_equal(h.probe_sh(pts[:n], 2, DEPTH, seed=SEED), whole[:n])
        assert np.array_equal(h.probe_sh(pts[n:], 2, DEPTH, seed=SEED, key0=n), whole[n:])      # the tail as a chunk of its own
        assert not np.array_equal(h.probe_sh(pts[n:], 2, DEPTH, seed=SEED, key0=n + 1), whole[n:])


@pytest.mark.parametrize("prec", ["f32", "f64"])
@pytest.mark.parametrize("name", ["s2", "mesh"])
def test_host_form_equals_device_form_and_sums_are_added(gpu, name, prec):
    import torch
    T = _T(prec)
    tdt = torch.float32 if prec == "f32" else torch.float64
    pts = _probes(name).astype(T)
    n = len(pts)
    prefill = np.random.default_rng(4).uniform(-1, 2, (n, 9, 3)).astype(T)
    with _handle(gpu, _scene(name), prec) as h:
        d_pts = torch.tensor(pts, dtype=tdt, device="cuda:0").contiguous()
        st = torch.cuda.Stream()
        for spp in (1, 5):
            fresh, valid = h.probe_sh(pts, spp, DEPTH, seed=SEED, want_valid=True)
            d_sums = torch.zeros((n, 9, 3), dtype=tdt, device="cuda:0")
            d_valid = torch.full((n,), 7, dtype=torch.uint8, device="cuda:0")
            torch.cuda.synchronize()
            h.probe_sh_device(d_pts.data_ptr(), n, spp, DEPTH, d_sums.data_ptr(), seed=SEED, d_valid_ptr=d_valid.data_ptr(), stream_ptr=st.cuda_stream)
            st.synchronize()
            assert np.array_equal(d_sums.cpu().numpy(), fresh) and np.array_equal(d_valid.cpu().numpy(), valid) and valid.all()
            # sums are added to, not stored: non-zero starting sums against the twin started from them
            got = h.probe_sh(pts, spp, DEPTH, seed=SEED, sums=prefill.copy())
            want, _ = _twin(gpu, h, pts, spp, prec, start=prefill)
            assert np.array_equal(got, want) and not np.array_equal(got, fresh)
            d_sums = torch.tensor(prefill, dtype=tdt, device="cuda:0").contiguous()
            torch.cuda.synchronize()
            h.probe_sh_device(d_pts.data_ptr(), n, spp, DEPTH, d_sums.data_ptr(), seed=SEED, stream_ptr=st.cuda_stream)      # no valid bytes wanted
            st.synchronize()
            assert np.array_equal(d_sums.cpu().numpy(), want)
        # the generator's device form writes the host form's list
        for sample, key0 in ((0, 0), (9, 12345)):
            d_rays = torch.full((n, 6), -1.0, dtype=tdt, device="cuda:0")
            torch.cuda.synchronize()
            gpu.probe_rays_device(d_pts.data_ptr(), n, d_rays.data_ptr(), sample, SEED, key0, st.cuda_stream, prec)
            st.synchronize()
            host = gpu.probe_rays(pts, sample, SEED, key0, prec)
            assert np.array_equal(d_rays.cpu().numpy(), host) and np.array_equal(host, bake.sphere_rays(pts, sample, SEED, key0, prec))


@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_probe_rays_device_on_more_than_one_workgroup_with_invalid_points(gpu, prec):
    import torch
    T = _T(prec)
    tdt = torch.float32 if prec == "f32" else torch.float64
    pts = np.random.default_rng(6).normal(size=(777, 3)).astype(T) * 5            # four workgroups, the last one 9 points
    pts[5, 1], pts[256, 0], pts[776, 2] = np.nan, np.inf, -np.inf
    d_pts = torch.tensor(pts, dtype=tdt, device="cuda:0").contiguous()
    d_rays = torch.full((778, 6), -1.0, dtype=tdt, device="cuda:0")
    torch.cuda.synchronize()
    gpu.probe_rays_device(d_pts.data_ptr(), 777, d_rays.data_ptr(), 4, SEED, 99, 0, prec)
    torch.cuda.synchronize()
    got = d_rays.cpu().numpy()
    assert np.array_equal(got[:777], gpu.probe_rays(pts, 4, SEED, 99, prec)) and (got[777] == -1).all()      # nothing written past the list
    assert (got[[5, 256, 776]] == 0).all()


@pytest.mark.parametrize("prec", ["f32", "f64"])
@pytest.mark.parametrize("spp", [1, 3])
def test_invalid_points_interleaved(gpu, prec, spp):
    T = _T(prec)
    pts = _probes("mesh").astype(T)
    kinds = [np.array([np.nan, 0, 0]), np.array([0, np.nan, 0]), np.array([0, 1, np.nan]), np.array([np.inf, 0, 0]), np.array([0, -np.inf, 0]), np.array([0, 1, np.inf])]
    bad = np.array(pts)
    at = np.arange(3, 200, 9)
    assert len(at) >= 3 * len(kinds)
    for i, k in enumerate(at):
        bad[k] = kinds[i % len(kinds)].astype(T)
    ok = np.setdiff1d(np.arange(200), at)
    prefill = np.random.default_rng(8).uniform(0, 1, (200, 9, 3)).astype(T)
    with _handle(gpu, _scene("mesh"), prec) as h:
        clean = h.probe_sh(pts, spp, DEPTH, seed=SEED, sums=prefill.copy())
        got, valid = h.probe_sh(bad, spp, DEPTH, seed=SEED, sums=prefill.copy(), want_valid=True)
    assert not valid[at].any() and valid[ok].all()
    assert np.array_equal(got[at], prefill[at])                                      # untouched
    assert np.array_equal(got[ok], clean[ok]) and not np.array_equal(clean[at], prefill[at])


@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_a_probe_call_after_update_device_on_another_stream_sees_the_moved_mesh(gpu, prec):
    import torch
    from test_gpu_refit import deform
    A = _scene("mesh")
    moved = dict(A, triangles10=deform(A["triangles10"]))
    tdt = torch.float32 if prec == "f32" else torch.float64
    pts = _probes("mesh", 320).astype(_T(prec))
    with _handle(gpu, moved, prec) as hb:
        want = hb.probe_sh(pts, 2, DEPTH, seed=SEED)
    d_tri = torch.tensor(moved["triangles10"], dtype=tdt, device="cuda:0").contiguous()
    d_pts = torch.tensor(pts, dtype=tdt, device="cuda:0").contiguous()
    d_sums = torch.zeros((320, 9, 3), dtype=tdt, device="cuda:0")
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()
    with _handle(gpu, A, prec) as h:
        before = h.probe_sh(pts, 2, DEPTH, seed=SEED)
        h.update_device(d_tri, s1)
        h.probe_sh_device(d_pts.data_ptr(), 320, 2, DEPTH, d_sums.data_ptr(), seed=SEED, stream_ptr=s2.cuda_stream)
        s2.synchronize()
        got = d_sums.cpu().numpy()
    assert np.array_equal(got, want) and not np.array_equal(got, before)


# ---------------------------------------------------------------------------------- the open sky: bands 0 and 1 only
@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_the_sky_is_band_0_and_1_only(gpu, prec):
    """One sphere of radius 1e-3 at distance 1e3 from 4 probes; no generated ray meets it (asserted in numpy on bake.sphere_rays' directions: every
    discriminant is negative), so at depth 1 every path is one sky lookup, L(d) = a + b d.y per channel with a = (1 + c) / 2, b = (c - 1) / 2,
    c = (0.5, 0.7, 1.0) — sky_term of csrc/spira_device.h.  Its coefficients are a sqrt(4 pi) at j = 0, b c1 4 pi / 3 at j = 1 and 0 elsewhere.
    light_probes at spp 4096 is within 6 standard errors of them.  The standard error is the list route's: the sample deviation of the 4096 products
    4 pi Y_j(d_s) L_s[c] of every point, L from Scene.radiance on the generated rays (at depth 1 the sky depends on the direction alone, so one call on the
    whole list serves), over sqrt(4096).  Where those products are constant (c = 1: L = 1, and Y0 is a constant) the standard error is 0 and what remains is
    the rounding of the entry's sum of 4096 terms in T, (N - 1) eps / 2 of the mean magnitude of the terms at the worst (the bound on recursive summation),
    which is added to the bound: 9e-4 relative in Float32, nothing to speak of in Float64."""
    T = _T(prec)
    N = 4096
    s1 = _scene("s1")
    scene = dict(spheres5=np.array([[1000.0, 0.0, 0.0, 1e-3, 1]]), materials8=s1["materials8"][:1], triangles10=None)
    pts = np.array([[0.0, 0.0, 0.0], [0.5, -0.25, 0.125], [-0.75, 2.0, 0.5], [0.0, -3.0, 1.0]])
    rays = np.stack([bake.sphere_rays(pts, s, SEED, 0, prec) for s in range(N)])         # [N, 4, 6]
    o, qh = rays[..., 0:3].astype(np.float64), rays[..., 3:6].astype(np.float64)
    oc = o - np.array([1000.0, 0.0, 0.0])
    b = (oc * qh).sum(axis=-1)
    disc = b * b - (qh * qh).sum(axis=-1) * ((oc * oc).sum(axis=-1) - 1e-6)
    assert (disc < 0).all(), "a generated ray meets the far sphere"
    with _handle(gpu, scene, prec) as h:
        got = bake.light_probes(h, pts, N, 1, seed=SEED)
        L = h.radiance(rays.reshape(-1, 6), 1, 1, seed=SEED).reshape(N, 4, 3)
    valid, d = cameras.ray_prepare(rays.reshape(-1, 6), prec)
    assert valid.all()
    c = np.array([0.5, 0.7, 1.0])
    a, bb = (1 + c) / 2, (c - 1) / 2
    assert np.abs(L.astype(np.float64) - (a + bb * d.reshape(N, 4, 3).astype(np.float64)[..., 1:2])).max() <= 8 * np.finfo(T).eps      # every path was one sky lookup
    prod = 4 * np.pi * bake.sh9(d).astype(np.float64).reshape(N, 4, 9)[..., None] * L.astype(np.float64)[:, :, None, :]      # [N, 4, 9, 3]
    se = prod.std(axis=0, ddof=1) / np.sqrt(N)
    floor = (N - 1) * (np.finfo(T).eps / 2) * np.abs(prod).mean(axis=0) + 4 * np.finfo(T).eps
    want = np.zeros((9, 3))
    want[0] = a * np.sqrt(4 * np.pi)
    want[1] = bb * bake.SH9_C[1] * 4 * np.pi / 3
    err = np.abs(got.astype(np.float64) - want[None])
    print(prec, "worst |coefficient - analytic| / (6 se + rounding):", (err / (6 * se + floor)).max(), " largest se:", se.max(), " largest rounding term:", floor.max())
    assert got.shape == (4, 9, 3) and got.dtype == T
    assert (err <= 6 * se + floor).all(), (err / (6 * se + floor)).max()
    # ... and it IS the mean of those products, up to the rounding of the products, of the sum and of the scaling in T: (N + 2) eps / 2 of the mean magnitude
    assert (np.abs(got.astype(np.float64) - prod.mean(axis=0)) <= 2 * floor).all()
