"""CPU: spira_hip.cameras — the numpy restatements the product uses (counter RNG, ray preparation, the three generator models) against the oracle and
against their own geometry, and raytracer.render's default path left as it was."""
import numpy as np
import pytest

from spira_hip import _binding as B
from spira_hip import cameras, raytracer, scenes

W, H, SEED = 33, 17, 5


@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_rng3_is_the_oracles(oracle, prec):
    pixels = np.array([0, 1, 560, 99999, 2 ** 31 - 1, 2 ** 32 - 1], dtype=np.uint64)
    for seed in (0, 5, 0x1234567890ABCDEF):
        for sample, bounce, t in ((0, 0, 0), (3, 0, 0), (7, 2, 1), (2 ** 24 - 1, 255, 64), (11, 254, 17)):
            got = cameras.rng3(seed, pixels, sample, bounce, t, prec)
            for k, px in enumerate(pixels):
                assert np.array_equal(got[k], oracle.rng_try(seed, int(px), sample, bounce, t, prec)), (seed, px, sample, bounce, t)
    assert cameras.rng3(5, pixels, 3, 0, 0, prec).dtype == (np.float32 if prec == "f32" else np.float64)


@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_numpy_pinhole_rays_are_the_oracles_first_segment(oracle, prec):
    for s in (scenes.scene_s1(), scenes.scene_s2()):
        nt = 0 if s["triangles10"] is None else len(s["triangles10"])
        p = oracle.make_params(W, H, 4, 3, len(s["spheres5"]), len(s["materials8"]), nt, seed=SEED)
        for sample in (0, 3):
            rays = cameras.generate_rays(s["camera12"], B.CAM_PINHOLE, W, H, sample, SEED, prec=prec)
            valid, d = cameras.ray_prepare(rays, prec)
            assert valid.all()
            for i, j in ((1, 1), (W, 1), (1, H), (W, H), (17, 9), (2, 16), (30, 5), (9, 12), (25, 3), (12, 14)):
                dirs = oracle.trace_path(s["spheres5"], s["materials8"], s["triangles10"], s["camera12"], p, i, j, sample, prec)[3]
                k = (j - 1) * W + (i - 1)
                assert np.array_equal(d[k], dirs[0]), (i, j, sample)
                assert np.array_equal(rays[k, 0:3], np.asarray(s["camera12"][0:3], dtype=rays.dtype))


@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_thin_lens(prec):
    T = np.float32 if prec == "f32" else np.float64
    cam = np.ascontiguousarray(scenes.scene_s1()["camera12"], dtype=T)
    pin = cameras.generate_rays(cam, B.CAM_PINHOLE, W, H, 2, SEED, prec=prec)
    assert np.array_equal(cameras.generate_rays(cam, B.CAM_THIN_LENS, W, H, 2, SEED, lens_radius=0.0, prec=prec), pin)      # radius 0 IS the pinhole
    R = 0.25
    lens = cameras.generate_rays(cam, B.CAM_THIN_LENS, W, H, 2, SEED, lens_radius=R, prec=prec)
    assert lens.dtype == T and not np.array_equal(lens, pin)
    c64 = cam.astype(np.float64)
    eu, ev = c64[6:9] / np.linalg.norm(c64[6:9]), c64[9:12] / np.linalg.norm(c64[9:12])
    axis = np.cross(eu, ev)
    off = lens[:, 0:3].astype(np.float64) - c64[0:3]
    eps = float(np.finfo(T).eps)
    scale = np.abs(c64[0:3]).max() + R
    assert np.abs(off @ axis).max() <= 8 * eps * scale                              # the lens points lie in the lens plane
    assert np.linalg.norm(off, axis=1).max() <= R * (1 + 8 * eps) + 8 * eps * scale        # ... within the lens
    assert np.linalg.norm(off, axis=1).max() > 0.8 * R and len(np.unique(off[:, 0])) > W * H // 2      # ... and fill it
    # every ray of a pixel sample meets the focus plane at the pinhole's point P = origin + d_pinhole
    P = c64[0:3] + pin[:, 3:6].astype(np.float64)
    hit = lens[:, 0:3].astype(np.float64) + lens[:, 3:6].astype(np.float64)
    assert np.abs(hit - P).max() <= 8 * eps * max(scale, np.abs(P).max())


@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_ortho_and_row_chunks(prec):
    cam = scenes.scene_s1()["camera12"]
    rays = cameras.generate_rays(cam, B.CAM_ORTHO, W, H, 1, SEED, prec=prec)
    assert (rays[:, 3:6] == rays[0, 3:6]).all() and len(np.unique(rays[:, 0])) > W      # one direction, many origins
    pin = cameras.generate_rays(cam, B.CAM_PINHOLE, W, H, 1, SEED, prec=prec)
    T = rays.dtype.type
    c = np.ascontiguousarray(cam, dtype=T)
    assert np.abs(rays[:, 0:3].astype(np.float64) - (c[0:3].astype(np.float64) + pin[:, 3:6])).max() <= 8 * float(np.finfo(T).eps) * 4      # the origins are the pinhole's focus-plane points
    axis = (c[3:6].astype(np.float64) + c[6:9] / 2.0 + c[9:12] / 2.0) - c[0:3]
    assert np.abs(rays[0, 3:6] - axis).max() <= 8 * float(np.finfo(T).eps) * 4
    for model in (B.CAM_PINHOLE, B.CAM_THIN_LENS, B.CAM_ORTHO):
        whole = cameras.generate_rays(cam, model, W, H, 1, SEED, lens_radius=0.1, prec=prec)
        parts = [cameras.generate_rays(cam, model, W, H, 1, SEED, row0=r0, rows=n, lens_radius=0.1, prec=prec) for r0, n in ((0, 6), (6, 10), (16, 1))]
        assert np.array_equal(np.concatenate(parts), whole)


def test_equirect_is_a_ray_list():
    e = cameras.Equirect([0.0, 1.0, 3.0], forward=(0, 0, -1), up=(0, 1, 0))
    for prec in ("f32", "f64"):
        rays = e.rays(16, 8, sample=1, seed=SEED, prec=prec)
        valid, d = cameras.ray_prepare(rays, prec)
        assert rays.shape == (128, 6) and valid.all() and (rays[:, 0:3] == rays[0, 0:3]).all()
        assert d[:16, 1].max() < -0.8 and d[-16:, 1].min() > 0.8                       # bottom row looks down, top row up
        assert np.array_equal(e.rays(16, 8, 1, SEED, prec, row0=3, rows=2), rays[48:80])


def test_render_without_defocus_takes_the_old_path(monkeypatch):
    calls = []

    def fake_render(spheres5, materials8, triangles10, camera12, params, prec="f32", want_hdr=True, want_img=False):
        calls.append((params.width, params.height, params.spp, params.max_depth, params.flags, prec))
        z = np.zeros((3, params.height, params.width), dtype=np.float64)
        return z, z

    def no_ray_lists(*a, **k):
        raise AssertionError("the ray-list route was taken")
    monkeypatch.setattr(B, "render", fake_render)
    monkeypatch.setattr(cameras, "render", no_ray_lists)
    monkeypatch.setattr(B, "Scene", no_ray_lists)
    world, _ = raytracer.create_scene()
    sharp = raytracer.Camera(position=raytracer.Vec3(0, 1, 3), look_at=raytracer.Vec3(0, 0, -1), up=raytracer.Vec3(0, 1, 0), fov=45.0)
    wide = raytracer.Camera(position=raytracer.Vec3(0, 1, 3), look_at=raytracer.Vec3(0, 0, -1), up=raytracer.Vec3(0, 1, 0), fov=45.0, aperture=0.1, focus_dist=4.0)
    assert sharp.lens_radius == 0 and wide.lens_radius == 0.05
    for cam, kw in ((sharp, {}), (wide, {}), (wide, {"defocus": False}), (sharp, {"defocus": True})):      # (defocus with aperture 0 is the pinhole: old path too)
        img, hdr = raytracer.render(world, cam, 16, 9, samples_per_pixel=2, max_depth=3, **kw)
        assert img.shape == (9, 16, 3) and hdr.shape == (9, 16, 3)
    assert calls == [(16, 9, 2, 3, B.SEM_A | B.KERNEL_WAVEFRONT | B.POST_ACES, "f64")] * 4
    with pytest.raises(AssertionError, match="ray-list route"):
        raytracer.render(world, wide, 16, 9, samples_per_pixel=2, max_depth=3, defocus=True)
