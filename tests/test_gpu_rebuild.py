"""GPU: spira_scene_rebuild_* — a new triangle array for a live scene handle, the mesh's tree built anew on the device (spira_lbvh.h; k_lbvh_* and the refit
passes).  The tree only prunes, so the test of a rebuild is the refit's: a render through a rebuilt handle is, bit for bit, the render of a fresh handle on
the same arrays — image and segment count — and agrees with the oracle like every render.  A rebuilt tree that lost a triangle, or whose boxes did not hold
what lies beneath them, would lose hits and fail these tests.  All at 128 x 72, spp 4, depth 5, seed 11."""
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


def _with(s, tri):
    return dict(s, triangles10=np.array(tri, dtype=np.float64))


def _params(gpu, s, **kw):
    return gpu.make_params(W, H, SPP, DEPTH, len(s["spheres5"]), len(s["materials8"]), len(s["triangles10"]), seed=SEED, **kw)


def _fresh(gpu, s, prec):
    """Render of a fresh handle on s: (hdr, segments); computed once per (mesh, precision)."""
    key = ("fresh", s["triangles10"].tobytes(), prec)
    if key not in _cache:
        with gpu.Scene(s["spheres5"], s["materials8"], s["triangles10"], prec) as h:
            hdr, _ = h.render(s["camera12"], _params(gpu, s))
            _cache[key] = (hdr, gpu.counters()["segments"])
    return _cache[key]


def _tdt(prec):
    import torch
    return torch.float32 if prec == "f32" else torch.float64


def _bounds(tri):
    v = np.asarray(tri)[:, :9].reshape(-1, 3)
    lo, hi = v.min(axis=0), v.max(axis=0)
    return (lo + hi) / 2.0, float((hi - lo).max())


@pytest.mark.parametrize("prec,level", [("f32", 3), ("f64", 3), ("f32", 4)])
def test_render_after_rebuild_is_the_render_of_a_fresh_handle(gpu, oracle, prec, level):
    A, B = _scene(level)
    assert len(A["triangles10"]) == 20 * 4 ** level
    p = _params(gpu, A)
    with gpu.Scene(A["spheres5"], A["materials8"], A["triangles10"], prec) as h:
        first, _ = h.render(A["camera12"], p)
        h.rebuild(B["triangles10"])
        second, _ = h.render(A["camera12"], p)
        seg = gpu.counters()["segments"]
    want, want_seg = _fresh(gpu, B, prec)
    assert not np.array_equal(first, second)
    assert np.array_equal(second, want) and seg == want_seg
    ohdr, _, oseg = oracle.render(B["spheres5"], B["materials8"], B["triangles10"], B["camera12"],
                                  oracle.make_params(W, H, SPP, DEPTH, len(B["spheres5"]), len(B["materials8"]), len(B["triangles10"]), seed=SEED), prec)
    err = np.abs(second.astype(np.float64) - ohdr.astype(np.float64))
    print("max |gpu - oracle| = %.3e" % err.max())
    assert np.all(err <= ATOL + RTOL * np.abs(ohdr)) and seg == oseg


def _code(gpu, fn, *a, **kw):
    with pytest.raises(gpu.SpiraError) as e:
        fn(*a, **kw)
    return str(e.value)


@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_the_frame_rule_is_gone(gpu, prec):
    """The mesh moved by three times its extent along y and scaled by 2.5: an update is refused (-4), a rebuild takes it, and a following update with the
    deformed version of the moved mesh is inside the NEW frame."""
    A, _ = _scene(3)
    p = _params(gpu, A)
    c, ext = _bounds(A["triangles10"])
    moved = np.array(A["triangles10"], dtype=np.float64)
    v = moved[:, :9].reshape(-1, 3)
    moved[:, :9] = ((v - c) * 2.5 + c + [0.0, 3.0 * ext, 0.0]).reshape(-1, 9)
    M = _with(A, moved)
    MD = _with(A, deform(moved))
    with gpu.Scene(A["spheres5"], A["materials8"], A["triangles10"], prec) as h:
        before, _ = h.render(A["camera12"], p)
        assert "error -4" in _code(gpu, h.update, triangles10=moved)
        h.rebuild(moved)
        got, _ = h.render(A["camera12"], p)
        assert np.array_equal(got, _fresh(gpu, M, prec)[0]) and gpu.counters()["segments"] == _fresh(gpu, M, prec)[1]
        h.update(triangles10=MD["triangles10"])
        got2, _ = h.render(A["camera12"], p)
        assert np.array_equal(got2, _fresh(gpu, MD, prec)[0]) and gpu.counters()["segments"] == _fresh(gpu, MD, prec)[1]
        # ... and the OLD mesh is now outside the new frame's reach for an update only if it left it; a rebuild always takes it back
        h.rebuild(A["triangles10"])
        back, _ = h.render(A["camera12"], p)
        assert np.array_equal(back, before)


@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_device_form_matches_the_host_form_and_is_ordered_across_streams(gpu, prec):
    import torch
    A, B = _scene(3)
    p = _params(gpu, A)
    d_tri = torch.tensor(B["triangles10"], dtype=_tdt(prec), device="cuda:0").contiguous()
    want, want_seg = _fresh(gpu, B, prec)
    with gpu.Scene(A["spheres5"], A["materials8"], A["triangles10"], prec) as h:
        h.render(A["camera12"], p)
        h.rebuild_device(d_tri)
        got, _ = h.render(A["camera12"], p)
        assert np.array_equal(got, want) and gpu.counters()["segments"] == want_seg
    # the rebuild on one stream, the render at once on another, no host synchronisation in between: the library's own ordering has to hold
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    out = torch.zeros((3, H, W), dtype=_tdt(prec), device="cuda:0")
    torch.cuda.synchronize()
    with gpu.Scene(A["spheres5"], A["materials8"], A["triangles10"], prec) as h:
        h.render(A["camera12"], p)
        h.rebuild_device(d_tri, s1)
        h.render_device(A["camera12"], p, out.data_ptr(), 0, s2.cuda_stream)
        s2.synchronize()
        assert np.array_equal(out.cpu().numpy(), want)


def _awkward(name):
    """(first, target): two triangle arrays of one size in view of scene_s4's camera; the handle is created on `first` and rebuilt to `target`."""
    A, _ = _scene(3)
    base = np.array(A["triangles10"], dtype=np.float64)
    c, ext = _bounds(base)
    if name == "33":
        target = deform(base)[:1280:39][:33].copy()              # 33 triangles from all over the deformed mesh
    elif name == "copies200":
        one = np.concatenate([c + [-0.4 * ext, -0.3 * ext, 0.1 * ext], c + [0.45 * ext, -0.2 * ext, 0.0], c + [0.0, 0.5 * ext, -0.1 * ext], [2.0]])
        target = np.repeat(one[None, :], 200, axis=0)
    elif name == "flat512":
        q = 16
        xs, ys = np.linspace(c[0] - 0.5 * ext, c[0] + 0.5 * ext, q + 1), np.linspace(c[1] - 0.5 * ext, c[1] + 0.5 * ext, q + 1)
        rows = []
        for j in range(q):
            for i in range(q):
                p00, p10, p11, p01 = [xs[i], ys[j], c[2]], [xs[i + 1], ys[j], c[2]], [xs[i + 1], ys[j + 1], c[2]], [xs[i], ys[j + 1], c[2]]
                rows.append(p00 + p10 + p11 + [1.0 + (i + j) % 3])
                rows.append(p00 + p11 + p01 + [1.0 + (i + 2 * j) % 3])
        target = np.array(rows)
    else:
        assert name == "12"
        target = deform(base)[:1280:100][:12].copy()
    assert len(target) == {"33": 33, "copies200": 200, "flat512": 512, "12": 12}[name]
    first = target.copy()
    v = first[:, :9].reshape(-1, 3)
    first[:, :9] = ((v - c) * 0.6 + c + [0.3 * ext, -0.2 * ext, 0.1 * ext]).reshape(-1, 9)
    return _with(A, first), _with(A, target)


@pytest.mark.parametrize("prec", ["f32", "f64"])
@pytest.mark.parametrize("name", ["33", "copies200", "flat512", "12"])
def test_awkward_meshes(gpu, name, prec):
    """33 triangles (the smallest mesh with a tree), 200 copies of one triangle (every Morton key equal), a flat grid (one axis without extent) and 12
    triangles (no tree: the rebuild is the array), through both forms."""
    import torch
    F, T = _awkward(name)
    p = _params(gpu, T)
    want, want_seg = _fresh(gpu, T, prec)
    first_want, _ = _fresh(gpu, F, prec)
    assert not np.array_equal(want, first_want)      # the mesh is in view and the two poses differ
    with gpu.Scene(F["spheres5"], F["materials8"], F["triangles10"], prec) as h:
        first, _ = h.render(F["camera12"], p)
        h.rebuild(T["triangles10"])
        got, _ = h.render(F["camera12"], p)
        seg = gpu.counters()["segments"]
        h.rebuild_device(torch.tensor(F["triangles10"], dtype=_tdt(prec), device="cuda:0"))
        back, _ = h.render(F["camera12"], p)
    assert np.array_equal(first, first_want) and np.array_equal(got, want) and seg == want_seg and np.array_equal(back, first_want)


@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_refused_rebuilds_leave_the_handle_as_it_was(gpu, prec):
    import torch
    A, B = _scene(3)
    p = _params(gpu, A)
    tri = np.array(A["triangles10"])
    nan = tri.copy()
    nan[5, 2] = np.nan
    bad_material = tri.copy()
    bad_material[1279, 9] = 0.0
    with gpu.Scene(A["spheres5"], A["materials8"], A["triangles10"], prec) as h:
        before, _ = h.render(A["camera12"], p)
        for bad in (nan, bad_material):
            msg = _code(gpu, h.rebuild, bad)
            assert "error -1" in msg, msg
            after, _ = h.render(A["camera12"], p)
            assert np.array_equal(after, before)
            msg = _code(gpu, h.rebuild_device, torch.tensor(bad, dtype=_tdt(prec), device="cuda:0"))
            assert "error -1" in msg, msg
            after, _ = h.render(A["camera12"], p)
            assert np.array_equal(after, before)
        # the other precision's entries, a device pointer that is NULL
        assert "error -1" in _code(gpu, h.rebuild_device, 0)
        other = "f64" if prec == "f32" else "f32"
        arr = np.ascontiguousarray(B["triangles10"], dtype=np.float32 if other == "f32" else np.float64)
        assert getattr(gpu.lib(), "spira_scene_rebuild_" + other)(h._h, arr.ctypes.data_as(gpu.C.c_void_p)) == -1
        assert getattr(gpu.lib(), "spira_scene_rebuild_device_" + other)(h._h, gpu.C.c_void_p(1 << 20), None) == -1
        after, _ = h.render(A["camera12"], p)
        assert np.array_equal(after, before)
        # and after all that the handle still takes a good rebuild
        h.rebuild(B["triangles10"])
        got, _ = h.render(A["camera12"], p)
        assert np.array_equal(got, _fresh(gpu, B, prec)[0])
    with gpu.Scene(A["spheres5"], A["materials8"], A["triangles10"], prec, n_devices=1) as h:
        assert "error -5" in _code(gpu, h.rebuild, B["triangles10"])
        assert "error -5" in _code(gpu, h.rebuild_device, torch.tensor(B["triangles10"], dtype=_tdt(prec), device="cuda:0"))
    assert gpu.lib().spira_scene_rebuild_f32(None, None) == -1
    assert gpu.lib().spira_scene_rebuild_device_f64(None, None, None) == -1


def test_feature_buffers_and_adaptive_render_through_a_rebuilt_handle(gpu):
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
        h.rebuild(B["triangles10"])
        got_f = h.render_features(A["camera12"], p)
        got_a = h.render_adaptive(A["camera12"], pa, ad)
    for g, w in zip(got_f, want_f):
        assert np.array_equal(g, w)
    for g, w in zip(got_a, want_a):
        assert (g is None and w is None) or np.array_equal(g, w)
    assert want_f[2].max() > 0 and want_a[2].min() < want_a[2].max()      # the mesh is in view; the adaptive render did stop pixels at different counts


@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_a_to_b_to_a_returns_to_the_first_image(gpu, prec):
    A, B = _scene(3)
    p = _params(gpu, A)
    with gpu.Scene(B["spheres5"], B["materials8"], B["triangles10"], prec) as h:
        h.rebuild(A["triangles10"])
        first, _ = h.render(A["camera12"], p)
        h.rebuild(B["triangles10"])
        h.render(A["camera12"], p)
        h.rebuild(A["triangles10"])
        third, _ = h.render(A["camera12"], p)
    assert np.array_equal(third, first) and np.array_equal(first, _fresh(gpu, A, prec)[0])
