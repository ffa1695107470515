"""GPU: spira_scene_update_* — new contents for a live scene handle, the mesh's tree refitted on the device (spira_refit.h; k_refit_check, k_refit_tris,
k_refit_level).  The tree only prunes (spira_bvh.h: the leaf test is the linear scan's own arithmetic on the caller's coordinates), so the test of a refit
is equality: a render through an updated handle is, bit for bit, the render of a fresh handle built on the same arrays — image and segment count — and
agrees with the oracle like every render.  The deformation (twist + sine, 0.3 of the extent) moves every triangle out of its old leaf box
(tests/native/refit_plan.cpp counts them), so a refit that skipped the node pass would lose hits and fail these tests.  All at 128 x 72, spp 4, depth 5."""
import numpy as np
import pytest

from spira_hip import scenes

pytestmark = pytest.mark.gpu

W, H, SPP, DEPTH, SEED = 128, 72, 4, 5, 11
RTOL, ATOL = 1e-5, 1e-6      # test_gpu_parity's: |gpu - oracle| <= ATOL + RTOL*|oracle| per pixel and channel


def deform(tri, amp=0.3):
    """Twist about the vertical axis through the mesh's middle + a sine displacement of amp x the extent; the material column changes too."""
    t = np.array(tri, dtype=np.float64)
    v = t[:, :9].reshape(-1, 3)
    lo, hi = v.min(axis=0), v.max(axis=0)
    c, ext = (lo + hi) / 2.0, float((hi - lo).max())
    x, y, z = (v - c).T
    ang = 5.0 * y / ext
    out = np.stack([np.cos(ang) * x - np.sin(ang) * z + amp * ext * np.sin(5.0 * y / ext), y + 0.1 * ext * np.sin(7.0 * x / ext), np.sin(ang) * x + np.cos(ang) * z], axis=1) + c
    t[:, :9] = out.reshape(-1, 9)
    t[:, 9] = 1.0 + (np.arange(len(t)) % 3)
    return t


_cache = {}


def _scene(level):
    """(A, B): scene_s4(level) and the same scene with the deformed mesh."""
    if level not in _cache:
        a = scenes.scene_s4(level=level)
        b = dict(a, triangles10=deform(a["triangles10"]))
        _cache[level] = (a, b)
    return _cache[level]


def _params(gpu, s, **kw):
    return gpu.make_params(W, H, SPP, DEPTH, len(s["spheres5"]), len(s["materials8"]), len(s["triangles10"]), seed=SEED, **kw)


def _fresh(gpu, s, prec):
    """Render of a fresh handle on s: (hdr, segments); computed once per (scene, precision)."""
    key = ("fresh", id(s["triangles10"]), prec)
    if key not in _cache:
        with gpu.Scene(s["spheres5"], s["materials8"], s["triangles10"], prec) as h:
            hdr, _ = h.render(s["camera12"], _params(gpu, s))
            _cache[key] = (hdr, gpu.counters()["segments"])
    return _cache[key]


@pytest.mark.parametrize("prec,level", [("f32", 3), ("f64", 3), ("f32", 4)])
def test_render_after_update_is_the_render_of_a_fresh_handle(gpu, oracle, prec, level):
    A, B = _scene(level)
    assert len(A["triangles10"]) == 20 * 4 ** level
    p = _params(gpu, A)
    with gpu.Scene(A["spheres5"], A["materials8"], A["triangles10"], prec) as h:
        first, _ = h.render(A["camera12"], p)
        h.update(triangles10=B["triangles10"])
        second, _ = h.render(A["camera12"], p)
        seg = gpu.counters()["segments"]
    want, want_seg = _fresh(gpu, B, prec)
    assert np.array_equal(first, _fresh(gpu, A, prec)[0])
    assert not np.array_equal(first, second)
    assert np.array_equal(second, want) and seg == want_seg
    ohdr, _, oseg = oracle.render(B["spheres5"], B["materials8"], B["triangles10"], B["camera12"],
                                  oracle.make_params(W, H, SPP, DEPTH, len(B["spheres5"]), len(B["materials8"]), len(B["triangles10"]), seed=SEED), prec)
    err = np.abs(second.astype(np.float64) - ohdr.astype(np.float64))
    print("max |gpu - oracle| = %.3e" % err.max())
    assert np.all(err <= ATOL + RTOL * np.abs(ohdr)) and seg == oseg


@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_device_form_matches_the_host_form_and_is_ordered_across_streams(gpu, prec):
    import torch
    A, B = _scene(3)
    p = _params(gpu, A)
    tdt = torch.float32 if prec == "f32" else torch.float64
    d_tri = torch.tensor(B["triangles10"], dtype=tdt, device="cuda:0").contiguous()
    want, want_seg = _fresh(gpu, B, prec)
    with gpu.Scene(A["spheres5"], A["materials8"], A["triangles10"], prec) as h:
        h.render(A["camera12"], p)
        h.update_device(d_tri)
        got, _ = h.render(A["camera12"], p)
        assert np.array_equal(got, want) and gpu.counters()["segments"] == want_seg
    # the refit on one stream, the render at once on another, no host synchronisation in between: the library's own ordering has to hold
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    out = torch.zeros((3, H, W), dtype=tdt, device="cuda:0")
    torch.cuda.synchronize()
    with gpu.Scene(A["spheres5"], A["materials8"], A["triangles10"], prec) as h:
        h.render(A["camera12"], p)
        h.update_device(d_tri, s1)
        h.render_device(A["camera12"], p, out.data_ptr(), 0, s2.cuda_stream)
        s2.synchronize()
        assert np.array_equal(out.cpu().numpy(), want)


@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_a_to_b_to_a_returns_to_the_first_image(gpu, prec):
    A, B = _scene(3)
    p = _params(gpu, A)
    with gpu.Scene(A["spheres5"], A["materials8"], A["triangles10"], prec) as h:
        first, _ = h.render(A["camera12"], p)
        h.update(triangles10=B["triangles10"])
        h.render(A["camera12"], p)
        h.update(triangles10=A["triangles10"])
        third, _ = h.render(A["camera12"], p)
    assert np.array_equal(third, first)


def test_spheres_and_materials_alone(gpu):
    A, _ = _scene(3)
    sph = A["spheres5"].copy()
    sph[1, :3] = [0.6, 1.4, -0.4]
    sph[1, 3] = 0.35
    mats = A["materials8"].copy()
    mats[2, :3] = [0.2, 0.4, 0.8]
    mats[0, 7] = 0.3
    S = dict(A, spheres5=sph, materials8=mats)
    p = _params(gpu, A)
    with gpu.Scene(A["spheres5"], A["materials8"], A["triangles10"], "f32") as h:
        first, _ = h.render(A["camera12"], p)
        h.update(spheres5=sph, materials8=mats)
        got, _ = h.render(A["camera12"], p)
        h.update(materials8=A["materials8"])
        h.update(spheres5=A["spheres5"])
        back, _ = h.render(A["camera12"], p)
    with gpu.Scene(S["spheres5"], S["materials8"], S["triangles10"], "f32") as h:
        want, _ = h.render(A["camera12"], p)
    assert np.array_equal(got, want) and not np.array_equal(got, first) and np.array_equal(back, first)


@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_small_mesh_without_a_tree(gpu, prec):
    """Twelve triangles stay in LDS: no tree, no frame — the update is the array, in both forms, and the mesh may go anywhere."""
    import torch
    s = scenes.scene_s2()
    tri = np.array(s["triangles10"], dtype=np.float64)
    tri = np.concatenate([tri] * (12 // len(tri) + 1))[:12].copy()
    tri[:, :9] += np.repeat(np.arange(12), 9).reshape(12, 9) * 0.05
    moved = tri.copy()
    moved[:, :9] = moved[:, :9] * 1.7 + 0.4
    p = gpu.make_params(W, H, SPP, DEPTH, len(s["spheres5"]), len(s["materials8"]), 12, seed=SEED)
    with gpu.Scene(s["spheres5"], s["materials8"], moved, prec) as h:
        want, _ = h.render(s["camera12"], p)
    with gpu.Scene(s["spheres5"], s["materials8"], tri, prec) as h:
        first, _ = h.render(s["camera12"], p)
        h.update(triangles10=moved)
        got, _ = h.render(s["camera12"], p)
        h.update_device(torch.tensor(tri, dtype=torch.float32 if prec == "f32" else torch.float64, device="cuda:0"))
        back, _ = h.render(s["camera12"], p)
    assert np.array_equal(got, want) and not np.array_equal(first, want) and np.array_equal(back, first)


def _code(gpu, fn, *a, **kw):
    with pytest.raises(gpu.SpiraError) as e:
        fn(*a, **kw)
    return str(e.value)


@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_refused_updates_leave_the_handle_as_it_was(gpu, prec):
    import torch
    A, B = _scene(3)
    p = _params(gpu, A)
    tdt = torch.float32 if prec == "f32" else torch.float64
    tri = np.array(A["triangles10"])
    v = tri[:, :9].reshape(-1, 3)
    c, ext = (v.min(axis=0) + v.max(axis=0)) / 2.0, float((v.max(axis=0) - v.min(axis=0)).max())
    out_of_frame = tri.copy()
    out_of_frame[700, 3:6] = c + [0.0, 3.0 * ext, 0.0]          # the frame reaches at most 2 x the extent from the centre
    nan = tri.copy()
    nan[5, 2] = np.nan
    bad_material = tri.copy()
    bad_material[1279, 9] = 0.0
    with gpu.Scene(A["spheres5"], A["materials8"], A["triangles10"], prec) as h:
        before, _ = h.render(A["camera12"], p)
        for bad, code in ((out_of_frame, "error -4"), (nan, "error -1"), (bad_material, "error -1")):
            msg = _code(gpu, h.update, triangles10=bad)
            assert code in msg, msg
            after, _ = h.render(A["camera12"], p)
            assert np.array_equal(after, before)
            msg = _code(gpu, h.update_device, torch.tensor(bad, dtype=tdt, device="cuda:0"))
            assert code in msg, msg
            after, _ = h.render(A["camera12"], p)
            assert np.array_equal(after, before)
        assert "create a new handle" in _code(gpu, h.update, triangles10=out_of_frame)
        bad_sphere = A["spheres5"].copy()
        bad_sphere[0, 4] = 9.0
        assert "error -1" in _code(gpu, h.update, spheres5=bad_sphere, triangles10=B["triangles10"])      # nothing of a refused update is applied
        after, _ = h.render(A["camera12"], p)
        assert np.array_equal(after, before)
        # all-NULL, the other precision, a device pointer that is NULL
        assert "error -1" in _code(gpu, h.update)
        assert "error -1" in _code(gpu, h.update_device, 0)
        other = "f64" if prec == "f32" else "f32"
        fn = getattr(gpu.lib(), "spira_scene_update_" + other)
        arr = np.ascontiguousarray(B["triangles10"], dtype=np.float32 if other == "f32" else np.float64)
        assert fn(h._h, None, None, arr.ctypes.data_as(gpu.C.c_void_p)) == -1
        fn = getattr(gpu.lib(), "spira_scene_update_device_" + other)
        assert fn(h._h, gpu.C.c_void_p(1 << 20), None) == -1
        # and after all that the handle still takes a good update
        h.update(triangles10=B["triangles10"])
        got, _ = h.render(A["camera12"], p)
        assert np.array_equal(got, _fresh(gpu, B, prec)[0])
    with gpu.Scene(A["spheres5"], A["materials8"], A["triangles10"], prec, n_devices=1) as h:
        assert "error -5" in _code(gpu, h.update, triangles10=B["triangles10"])
        assert "error -5" in _code(gpu, h.update_device, torch.tensor(B["triangles10"], dtype=tdt, device="cuda:0"))
    assert gpu.lib().spira_scene_update_f32(None, None, None, None) == -1


def test_feature_buffers_and_adaptive_render_through_an_updated_handle(gpu):
    A, B = _scene(3)
    p = _params(gpu, A)
    pa = _params(gpu, A)
    pa.spp = 16
    ad = gpu.make_adaptive(4, 4, 0.05, 0.01)
    with gpu.Scene(B["spheres5"], B["materials8"], B["triangles10"], "f32") as h:
        want_f = h.render_features(A["camera12"], p)
        want_a = h.render_adaptive(A["camera12"], pa, ad)
    with gpu.Scene(A["spheres5"], A["materials8"], A["triangles10"], "f32") as h:
        h.render(A["camera12"], p)
        h.update(triangles10=B["triangles10"])
        got_f = h.render_features(A["camera12"], p)
        got_a = h.render_adaptive(A["camera12"], pa, ad)
    for g, w in zip(got_f, want_f):
        assert np.array_equal(g, w)
    for g, w in zip(got_a, want_a):
        assert (g is None and w is None) or np.array_equal(g, w)
    assert want_f[2].max() > 0 and want_a[2].min() < want_a[2].max()      # the mesh is in view; the adaptive render did stop pixels at different counts
