"""GPU: spira_camera_rays_device_* against the numpy restatement (bytes), and a thin-lens frame through cameras.render."""
import numpy as np
import pytest

from spira_hip import cameras, scenes

pytestmark = pytest.mark.gpu

W, H = 33, 17


@pytest.mark.parametrize("prec", ["f32", "f64"])
@pytest.mark.parametrize("model,radius", [("CAM_PINHOLE", 0.0), ("CAM_THIN_LENS", 0.07), ("CAM_THIN_LENS", 0.0), ("CAM_ORTHO", 0.0)])
def test_device_generator_equals_the_numpy_restatement(gpu, model, radius, prec):
    import torch
    tdt = torch.float32 if prec == "f32" else torch.float64
    cam = scenes.scene_s1()["camera12"]
    m = getattr(gpu, model)
    for row0, rows in ((0, 0), (0, 6), (6, 11), (16, 1)):
        n = (rows or H) * W
        d = torch.full((n + 1, 6), -7.0, dtype=tdt, device="cuda:0")           # one guard row behind the list
        st = torch.cuda.Stream()
        torch.cuda.synchronize()
        gpu.camera_rays_device(cam, m, W, H, d.data_ptr(), sample=3, seed=9, row0=row0, rows=rows, lens_radius=radius, stream_ptr=st.cuda_stream, prec=prec)
        st.synchronize()
        got = d.cpu().numpy()
        want = cameras.generate_rays(cam, m, W, H, 3, 9, row0, rows, radius, prec)
        assert np.array_equal(got[:n], want) and (got[n] == -7).all()
        assert np.array_equal(gpu.camera_rays(cam, m, W, H, 3, 9, row0, rows, radius, prec), want)
    whole = cameras.generate_rays(cam, m, W, H, 3, 9, 0, 0, radius, prec)
    assert np.array_equal(cameras.generate_rays(cam, m, W, H, 3, 9, 6, 11, radius, prec), whole[6 * W:])


@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_thin_lens_frame(gpu, prec):
    s = scenes.scene_s2()
    w, h, spp, depth = 48, 27, 8, 6
    with gpu.Scene(s["spheres5"], s["materials8"], s["triangles10"], prec=prec) as sc:
        lens = cameras.render(sc, cameras.ThinLens(s["camera12"], 0.1), w, h, spp, depth, seed=2)
        again = cameras.render(sc, cameras.ThinLens(s["camera12"], 0.1), w, h, spp, depth, seed=2)
        pin = cameras.render(sc, cameras.Pinhole(s["camera12"]), w, h, spp, depth, seed=2)
        hdr, _ = sc.render(s["camera12"], sc.params(w, h, spp, depth, seed=2))
        pano = cameras.render(sc, cameras.Equirect([0.0, 1.0, 3.0]), w, h, 2, depth, seed=2)
    assert lens.shape == (3, h, w) and np.isfinite(lens).all() and lens.max() > 0
    assert lens.tobytes() == again.tobytes()
    assert np.array_equal(pin, hdr) and not np.array_equal(lens, pin)
    assert abs(float(lens.mean()) - float(pin.mean())) < 0.25 * float(pin.mean())      # the same scene, blurred: not another image
    assert np.isfinite(pano).all() and pano.max() > 0
