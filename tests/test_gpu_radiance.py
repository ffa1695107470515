"""GPU: spira_scene_radiance_* — path-traced radiance along the caller's rays on a scene handle.

Anchor: a ray list made from the pinhole camera reproduces spira_accumulate_* and Scene.render bit for bit (32 x 18, spp 4, depth 6, both precisions,
S1, S2 with its LDS triangle, the closed box S3 and the 320-triangle mesh, which has a tree).  Arbitrary rays are held to the oracle through a degenerate
camera per ray: camera = [o, llc, 0, 0] makes every pixel's ray normalize(llc - o) from o, and pixel i = k + 1 of row j = 1 has the RNG key k.
The contracts of the entry (sample ranges, passes, grids, forms, ragged sizes, adding, invalid rays, stream order) are all compared by bytes."""
import functools

import numpy as np
import pytest

from spira_hip import cameras, scenes

pytestmark = pytest.mark.gpu

RTOL, ATOL = 1e-5, 1e-6      # test_gpu_parity's: |gpu - oracle| <= ATOL + RTOL*|oracle| per ray and channel
W, H, SPP, DEPTH, SEED = 32, 18, 4, 6, 3
N_OR = 24                    # rays per scene against the oracle


@functools.lru_cache(maxsize=None)
def _scene(name):
    if name == "random":
        from test_gpu_parity import random_scene
        return random_scene(np.random.default_rng(11), 40, 25)
    return {"s1": scenes.scene_s1, "s2": scenes.scene_s2, "s3": scenes.scene_s3, "s2_glass": scenes.scene_s2_glass,
            "mesh": lambda: scenes.scene_s4(level=2)}[name]()


def _handle(gpu, s, prec):
    return gpu.Scene(s["spheres5"], s["materials8"], s["triangles10"], prec=prec)


def _npdt(prec):
    return np.float32 if prec == "f32" else np.float64


def _frame(sums, width, height):
    """[n, 3] sums in reference pixel order (bottom row first) -> planar [3, H, W], row 0 = top."""
    return np.ascontiguousarray(np.moveaxis(sums.reshape(height, width, 3)[::-1], -1, 0))


def _pinhole_sums(gpu, h, cam, prec, spp=SPP, flags=0, row0=0, rows=0, sums=None):
    n = (rows or H) * W
    sums = np.zeros((n, 3), dtype=_npdt(prec)) if sums is None else sums
    for s in range(spp):
        rays = gpu.camera_rays(cam, gpu.CAM_PINHOLE, W, H, s, SEED, row0, rows, 0.0, prec)
        h.radiance(rays, 1, DEPTH, seed=SEED, sample0=s, key0=row0 * W, flags=flags, sums=sums)
    return sums


# ---------------------------------------------------------------------------------- the anchor
@pytest.mark.parametrize("prec", ["f32", "f64"])
@pytest.mark.parametrize("name", ["s1", "s2", "s3", "mesh"])
def test_pinhole_list_is_the_renderer_bit_for_bit(gpu, name, prec):
    s = _scene(name)
    nt = 0 if s["triangles10"] is None else len(s["triangles10"])
    assert nt > 32 if name == "mesh" else nt <= 32
    p = gpu.make_params(W, H, SPP, DEPTH, len(s["spheres5"]), len(s["materials8"]), nt, seed=SEED)
    acc = np.zeros((3, H, W), dtype=_npdt(prec))
    gpu.accumulate(s["spheres5"], s["materials8"], s["triangles10"], s["camera12"], p, 0, acc, prec=prec)
    with _handle(gpu, s, prec) as h:
        hdr, _ = h.render(s["camera12"], p)
        sums = _pinhole_sums(gpu, h, s["camera12"], prec)
        assert np.array_equal(_frame(sums, W, H), acc)
        assert np.array_equal(_frame(sums / _npdt(prec)(SPP), W, H), hdr)
        # rows 0-6 and rows 7-17 with their key0 are the whole frame
        lo = _pinhole_sums(gpu, h, s["camera12"], prec, row0=0, rows=7)
        hi = _pinhole_sums(gpu, h, s["camera12"], prec, row0=7, rows=11)
        assert np.array_equal(np.concatenate([lo, hi]), sums)
        assert np.array_equal(cameras.render(h, cameras.Pinhole(s["camera12"]), W, H, SPP, DEPTH, seed=SEED), hdr)
    assert np.isfinite(acc).all() and acc.max() > 0 and len(np.unique(acc)) > 50


@pytest.mark.parametrize("flag", ["EXT_DIELECTRIC", "EXT_SPECTRAL"])
def test_pinhole_list_with_an_extension(gpu, flag):
    s, prec, ext = _scene("s2_glass"), "f32", getattr(gpu, flag)
    nt = 0 if s["triangles10"] is None else len(s["triangles10"])
    p = gpu.make_params(W, H, SPP, DEPTH, len(s["spheres5"]), len(s["materials8"]), nt, flags=ext, seed=SEED)
    with _handle(gpu, s, prec) as h:
        hdr, _ = h.render(s["camera12"], p)
        plain, _ = h.render(s["camera12"], gpu.make_params(W, H, SPP, DEPTH, len(s["spheres5"]), len(s["materials8"]), nt, seed=SEED))
        sums = _pinhole_sums(gpu, h, s["camera12"], prec, flags=ext)
    assert np.array_equal(_frame(sums / np.float32(SPP), W, H), hdr) and not np.array_equal(hdr, plain)


# ---------------------------------------------------------------------------------- arbitrary rays against the oracle
@functools.lru_cache(maxsize=None)
def _probe_rays(name):
    """24 seeded rays: origins uniform in a 6-unit box above the scene, aimed at points inside it.  (o, llc) in Float64, exactly representable in Float32."""
    rng = np.random.default_rng({"s1": 1, "s2": 2, "s2_glass": 3, "random": 4, "mesh": 5}[name])
    centre = np.array([0.0, 0.0, -4.0]) if name == "random" else np.array([0.0, 0.0, -1.0])
    o = rng.uniform(-3, 3, (N_OR, 3)) + centre + [0, 4, 0]
    llc = rng.uniform(-1.5, 1.5, (N_OR, 3)) + centre
    f32 = lambda a: a.astype(np.float32).astype(np.float64)
    return f32(o), f32(llc)


@functools.lru_cache(maxsize=None)
def _oracle_radiance(name, prec, flags):
    import oracle_py as O
    s = _scene(name)
    o, llc = _probe_rays(name)
    nt = 0 if s["triangles10"] is None else len(s["triangles10"])
    p = O.make_params(max(N_OR, 2), 2, SPP, DEPTH, len(s["spheres5"]), len(s["materials8"]), nt, flags=flags, seed=SEED)
    out = np.zeros((SPP, N_OR, 3), dtype=_npdt(prec))
    for k in range(N_OR):
        cam = np.concatenate([o[k], llc[k], np.zeros(6)])
        for smp in range(SPP):
            out[smp, k] = O.trace_path(s["spheres5"], s["materials8"], s["triangles10"], cam, p, k + 1, 1, smp, prec)[4]
    return out


@pytest.mark.parametrize("prec", ["f32", "f64"])
@pytest.mark.parametrize("name,ext", [("s1", 0), ("s2", 0), ("s2_glass", 0x20000), ("random", 0), ("mesh", 0)])
def test_arbitrary_rays_against_the_oracle(gpu, oracle, name, ext, prec):
    T = _npdt(prec)
    o, llc = _probe_rays(name)
    rays = np.concatenate([o.astype(T), llc.astype(T) - o.astype(T)], axis=1)      # d = llc - o computed in T
    want = _oracle_radiance(name, prec, ext)
    with _handle(gpu, _scene(name), prec) as h:
        per = np.stack([h.radiance(rays, 1, DEPTH, seed=SEED, sample0=smp, flags=ext) for smp in range(SPP)])
        once, valid = h.radiance(rays, SPP, DEPTH, seed=SEED, flags=ext, want_valid=True)
    err = np.abs(per.astype(np.float64) - want)
    print(name, prec, "max |gpu - oracle| =", err.max(), "max rel =", (err / np.maximum(np.abs(want), 1e-30)).max())
    assert valid.all() and np.isfinite(per).all()
    assert len(np.unique(per.sum(axis=(0, 2)))) == N_OR            # 24 distinct radiances
    assert np.all(err <= ATOL + RTOL * np.abs(want))
    total = np.zeros((N_OR, 3), dtype=T)
    for smp in range(SPP):
        total = total + per[smp]
    assert np.array_equal(total, once)


# ---------------------------------------------------------------------------------- contracts, bitwise
def _list(name, n, seed=21):
    """n rays into the scene from a box above it, rays of every fate (sky, spheres, the mesh)."""
    rng = np.random.default_rng(seed)
    o = rng.uniform(-3, 3, (n, 3)) + [0, 4, -1]
    d = rng.uniform(-1.5, 1.5, (n, 3)) + [0, 0, -1] - o
    return np.concatenate([o, d], axis=1)


@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_sample_ranges_passes_and_grids(gpu, prec, monkeypatch):
    rays = _list("mesh", 1000)
    with _handle(gpu, _scene("mesh"), prec) as h:
        pl = gpu.radiance_plan(1000, 8, 256)
        assert pl["n_pass"] == 1 and pl["spp_pass"] == 8 and not pl["direct"] and pl["grid"] > 1
        one = h.radiance(rays, 8, DEPTH, seed=SEED)
        part = h.radiance(rays, 3, DEPTH, seed=SEED)
        h.radiance(rays, 5, DEPTH, seed=SEED, sample0=3, sums=part)
        assert np.array_equal(part, one)                            # spp 8 = 3 + 5 through sample0
        monkeypatch.setenv("SPIRA_RADIANCE_MAX_ITEMS", "3000")      # 3 samples of 1000 rays per pass: 3 + 3 + 2
        pl = gpu.radiance_plan(1000, 8, 256)
        assert pl["n_pass"] == 3 and pl["spp_pass"] == 3 and pl["ws_entries"] == 3000
        assert np.array_equal(h.radiance(rays, 8, DEPTH, seed=SEED), one)
        monkeypatch.setenv("SPIRA_RADIANCE_MAX_ITEMS", "1000")      # one sample per pass: eight direct passes, no workspace
        pl = gpu.radiance_plan(1000, 8, 256)
        assert pl["n_pass"] == 8 and pl["direct"] and pl["ws_entries"] == 0
        assert np.array_equal(h.radiance(rays, 8, DEPTH, seed=SEED), one)
        monkeypatch.delenv("SPIRA_RADIANCE_MAX_ITEMS")
        monkeypatch.setenv("SPIRA_RADIANCE_WAVES_PER_CU", "0")      # one workgroup: 8 000 items on 256 lanes, every lane regenerates ~31 times
        assert gpu.radiance_plan(1000, 8, 256)["grid"] == 1 and gpu.radiance_plan(1000, 8, 256)["n_pass"] == 1
        assert np.array_equal(h.radiance(rays, 8, DEPTH, seed=SEED), one)
        monkeypatch.delenv("SPIRA_RADIANCE_WAVES_PER_CU")
    assert np.isfinite(one).all() and len(np.unique(one[:, 0])) > 500


@pytest.mark.parametrize("prec", ["f32", "f64"])
@pytest.mark.parametrize("name", ["s2", "mesh"])
def test_host_form_equals_device_form_and_sums_are_added(gpu, name, prec):
    import torch
    tdt = torch.float32 if prec == "f32" else torch.float64
    rays = _list(name, 257).astype(_npdt(prec))
    prefill = np.random.default_rng(4).uniform(0, 2, (257, 3)).astype(_npdt(prec))
    with _handle(gpu, _scene(name), prec) as h:
        for spp in (1, 5):
            fresh, valid = h.radiance(rays, spp, DEPTH, seed=SEED, want_valid=True)
            d_rays = torch.tensor(rays, dtype=tdt, device="cuda:0").contiguous()
            d_sums = torch.zeros((257, 3), dtype=tdt, device="cuda:0")
            d_valid = torch.full((257,), 7, dtype=torch.uint8, device="cuda:0")
            st = torch.cuda.Stream()
            torch.cuda.synchronize()
            h.radiance_device(d_rays.data_ptr(), 257, spp, DEPTH, d_sums.data_ptr(), seed=SEED, d_valid_ptr=d_valid.data_ptr(), stream_ptr=st.cuda_stream)
            st.synchronize()
            assert np.array_equal(d_sums.cpu().numpy(), fresh) and np.array_equal(d_valid.cpu().numpy(), valid) and valid.all()
            # sums are added to, not stored: a prefilled array plus the same samples, one addition per sample in order
            got = h.radiance(rays, spp, DEPTH, seed=SEED, sums=prefill.copy())
            want = prefill.copy()
            for smp in range(spp):
                want = want + h.radiance(rays, 1, DEPTH, seed=SEED, sample0=smp)
            assert np.array_equal(got, want) and not np.array_equal(got, fresh)


@pytest.mark.parametrize("prec", ["f32", "f64"])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 1000])
def test_ragged_sizes(gpu, prec, n):
    rays = _list("mesh", 1000)
    with _handle(gpu, _scene("mesh"), prec) as h:
        whole = h.radiance(rays, 2, DEPTH, seed=SEED)
        assert np.array_equal(h.radiance(rays[:n], 2, DEPTH, seed=SEED), whole[:n])
        if n < 1000:       # the tail as a chunk of its own, keyed by key0
            assert np.array_equal(h.radiance(rays[n:], 2, DEPTH, seed=SEED, key0=n), whole[n:])


@pytest.mark.parametrize("prec", ["f32", "f64"])
@pytest.mark.parametrize("spp", [1, 3])
def test_invalid_rays_interleaved(gpu, prec, spp):
    T = _npdt(prec)
    rays = _list("s2", 200).astype(T)
    tiny = np.sqrt(np.finfo(T).tiny) / 4                            # s = 3 tiny^2 / 16 < the smallest normal
    kinds = [np.array([np.nan, 0, 0, 0, -1, 0]), np.array([0, 4, 0, 0, np.nan, 0]), np.array([np.inf, 0, 0, 0, -1, 0]), np.array([0, 4, 0, -np.inf, 0, 0]),
             np.array([0, 4, 0, 0, 0, 0]), np.array([0, 4, 0, tiny, tiny, tiny]), np.array([0, 4, 0, np.finfo(T).max, np.finfo(T).max, 0])]
    bad = np.array(rays)
    at = np.arange(3, 200, 9)
    assert len(at) >= 3 * len(kinds)
    for i, k in enumerate(at):
        bad[k] = kinds[i % len(kinds)].astype(T)
    v_np, _ = cameras.ray_prepare(bad, prec)
    assert not v_np[at].any() and v_np.sum() == 200 - len(at)
    prefill = np.random.default_rng(8).uniform(0, 1, (200, 3)).astype(T)
    with _handle(gpu, _scene("s2"), prec) as h:
        clean = h.radiance(rays, spp, DEPTH, seed=SEED, sums=prefill.copy())
        got, valid = h.radiance(bad, spp, DEPTH, seed=SEED, sums=prefill.copy(), want_valid=True)
    assert np.array_equal(valid, v_np.astype(np.uint8))
    assert np.array_equal(got[at], prefill[at])                    # untouched
    ok = np.setdiff1d(np.arange(200), at)
    assert np.array_equal(got[ok], clean[ok]) and not np.array_equal(clean[at], prefill[at])


@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_a_call_after_update_device_on_another_stream_sees_the_moved_mesh(gpu, prec):
    import torch
    from test_gpu_refit import deform
    A = _scene("mesh")
    moved = dict(A, triangles10=deform(A["triangles10"]))
    tdt = torch.float32 if prec == "f32" else torch.float64
    rays = _list("mesh", 600).astype(_npdt(prec))
    with _handle(gpu, moved, prec) as hb:
        want = hb.radiance(rays, 2, DEPTH, seed=SEED)
    d_tri = torch.tensor(moved["triangles10"], dtype=tdt, device="cuda:0").contiguous()
    d_rays = torch.tensor(rays, dtype=tdt, device="cuda:0").contiguous()
    d_sums = torch.zeros((600, 3), dtype=tdt, device="cuda:0")
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()
    with _handle(gpu, A, prec) as h:
        before = h.radiance(rays, 2, DEPTH, seed=SEED)
        h.update_device(d_tri, s1)
        h.radiance_device(d_rays.data_ptr(), 600, 2, DEPTH, d_sums.data_ptr(), seed=SEED, stream_ptr=s2.cuda_stream)
        s2.synchronize()
        got = d_sums.cpu().numpy()
    assert np.array_equal(got, want) and not np.array_equal(got, before)
