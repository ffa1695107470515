"""GPU (MI355X): first-hit feature buffers (spira_render_features_*) and the a-trous denoiser (spira_denoise_*).
Features are held to bounce 0 of spira_trace_paths_* (itself held bitwise to the oracle in tests/test_gpu_parity.py) — depth and albedo bit for bit,
normals bit for bit in Float64 and within 4 x the Float32 restatement's own distance from the Float64 one in Float32 — and to oracle.trace_path
directly on a small frame.  The denoiser is held bit for bit to its numpy restatement (spira_hip/denoise.py, whose known answers are pinned in
tests/test_denoise_cpu.py), and on rendered frames it has to halve the relative MSE against a 2048-spp reference."""
import copy
import functools

import numpy as np
import pytest

from spira_hip import denoise as dnz
from spira_hip import scenes

pytestmark = pytest.mark.gpu

K = np.array([1 / 16, 1 / 4, 3 / 8, 1 / 4, 1 / 16])


def _T(prec):
    return np.float32 if prec == "f32" else np.float64


@functools.lru_cache(maxsize=None)
def _scene(name):
    s = {"s1": scenes.scene_s1, "s2": scenes.scene_s2, "s4": lambda: scenes.scene_s4(level=3)}[name]()
    return s["spheres5"], s["materials8"], s["triangles10"], s["camera12"]


def _params(mod, name, W, H, spp, depth=6, seed=31, flags=None, **tile):
    sp, ma, tr, _ = _scene(name)
    return mod.make_params(W, H, spp, depth, len(sp), len(ma), 0 if tr is None else len(tr), flags=0x300 if flags is None else flags, seed=seed, **tile)


# ---------------------------------------------------------------- features
def _ijs(W, H, spp):
    j, i, s = np.meshgrid(np.arange(H, 0, -1), np.arange(1, W + 1), np.arange(spp), indexing="ij")      # output row r (top first) is loop row j = H - r
    return np.stack([i, j, s], axis=-1).reshape(-1, 3).astype(np.uint32)


@functools.lru_cache(maxsize=None)
def _traces(name, W, H, spp, prec):
    """Bounce 0 of every (pixel, sample) from spira_trace_paths_*: prims [H, W, spp], ts [H, W, spp], dirs [H, W, spp, 3]."""
    from spira_hip import _binding as B
    prims, ts, dirs, _ = B.trace_paths(*_scene(name), _params(B, name, W, H, spp, depth=1), _ijs(W, H, spp), prec)
    return prims[:, 0].reshape(H, W, spp), ts[:, 0].reshape(H, W, spp), dirs[:, 0].reshape(H, W, spp, 3)


def _dot(a, b):
    return a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1] + a[..., 2] * b[..., 2]


def _normalize(a):
    return a / np.sqrt(_dot(a, a))[..., None]


def _cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2], a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], axis=-1)


def _expected(name, prims, ts, dirs, T, TN):
    """Feature buffers from bounce-0 traces.  Depth and albedo are summed in T; normals are restated in TN from the T-valued traces
    (TN = T: the kernel's statements; TN = float64 on Float32 traces: the yardstick of the Float32 floor)."""
    sp, ma, tr, cam = _scene(name)
    H, W, spp = prims.shape
    ns = len(sp)
    hit = prims >= 0
    mat_of = np.concatenate([np.asarray(sp)[:, 4], np.asarray(tr)[:, 9] if tr is not None else np.zeros(0)]).astype(np.int64) - 1
    alb_rows = np.asarray(ma, dtype=T)[:, :3][mat_of]
    alb_s = np.where(hit[..., None], alb_rows[np.where(hit, prims, 0)], T(1)).astype(T)
    spT, camN = np.asarray(sp, dtype=T), np.asarray(cam, dtype=T).astype(TN)
    with np.errstate(all="ignore"):
        pos = camN[:3] + dirs.astype(TN) * ts.astype(TN)[..., None]
        is_sph = hit & (prims < ns)
        ctr = spT[np.where(is_sph, prims, 0)][..., :3].astype(TN)
        n_s = _normalize(pos - ctr)
        if tr is not None:
            trT = np.asarray(tr, dtype=T)
            tri = trT[np.where(hit & ~is_sph, prims - ns, 0)]
            e1 = (tri[..., 3:6] - tri[..., 0:3]).astype(TN)          # the edges are differences in the scene's precision (stage_scene, the BVH build)
            e2 = (tri[..., 6:9] - tri[..., 0:3]).astype(TN)
            n_s = np.where(is_sph[..., None], n_s, _normalize(_cross(e1, e2)))
        n_s = np.where(hit[..., None], n_s, TN(0)).astype(TN)
    alb, nrm, dep = np.zeros((H, W, 3), dtype=T), np.zeros((H, W, 3), dtype=TN), np.zeros((H, W), dtype=T)
    for s in range(spp):
        alb = alb + alb_s[:, :, s]
        nrm = nrm + n_s[:, :, s]
        dep = dep + np.where(hit[:, :, s], ts[:, :, s], T(0)).astype(T)
    return (alb / T(spp)).transpose(2, 0, 1), (nrm / TN(spp)).transpose(2, 0, 1), dep / T(spp), hit.any(axis=2)


@pytest.mark.parametrize("prec", ["f32", "f64"])
@pytest.mark.parametrize("W,H,spp", [(67, 35, 1), (160, 90, 4)])
@pytest.mark.parametrize("name", ["s1", "s2", "s4"])
def test_features_against_bounce_zero_of_the_traces(gpu, name, W, H, spp, prec):
    T = _T(prec)
    alb, nrm, dep = gpu.render_features(*_scene(name), _params(gpu, name, W, H, spp), prec)
    prims, ts, dirs = _traces(name, W, H, spp, prec)
    e_alb, e_nrm, e_dep, any_hit = _expected(name, prims, ts, dirs, T, T)
    assert any_hit.any() and (~any_hit).any() and (prims.max() >= len(_scene(name)[0]) or name == "s1")      # hits, sky, and the scene's triangles
    assert np.array_equal(dep > 0, any_hit)
    assert np.array_equal(dep, e_dep)
    assert np.array_equal(alb, e_alb)
    if prec == "f64":
        assert np.array_equal(nrm, e_nrm)
    else:
        _, n64, _, _ = _expected(name, prims, ts, dirs, T, np.float64)
        floor = float(np.abs(e_nrm.astype(np.float64) - n64).max())
        err = float(np.abs(nrm.astype(np.float64) - n64).max())
        print("normal floor", name, "%dx%d spp %d" % (W, H, spp), "restatement f32 vs f64: %.3e" % floor, "gpu f32 vs f64: %.3e" % err,
              "gpu bitwise equal to the f32 restatement:", bool(np.array_equal(nrm, e_nrm)))
        assert floor > 0 and err <= 4 * floor


@pytest.mark.parametrize("prec", ["f32", "f64"])
@pytest.mark.parametrize("name", ["s1", "s2", "s4"])
def test_features_against_the_oracle_directly(gpu, oracle, name, prec):
    T = _T(prec)
    W, H, spp = 48, 27, 2
    alb, nrm, dep = gpu.render_features(*_scene(name), _params(gpu, name, W, H, spp), prec)
    op = _params(oracle, name, W, H, spp, depth=1)
    prims, ts, dirs = np.zeros((H, W, spp), dtype=np.int32), np.zeros((H, W, spp), dtype=T), np.zeros((H, W, spp, 3), dtype=T)
    for r in range(H):
        for x in range(W):
            for s in range(spp):
                _, pr, t, d, _ = oracle.trace_path(*_scene(name), op, x + 1, H - r, s, prec)
                prims[r, x, s], ts[r, x, s], dirs[r, x, s] = pr[0], t[0], d[0]
    e_alb, e_nrm, e_dep, any_hit = _expected(name, prims, ts, dirs, T, T)
    assert np.array_equal(dep > 0, any_hit) and np.array_equal(dep, e_dep) and np.array_equal(alb, e_alb)
    if prec == "f64":
        assert np.array_equal(nrm, e_nrm)
    else:
        _, n64, _, _ = _expected(name, prims, ts, dirs, T, np.float64)
        floor = float(np.abs(e_nrm.astype(np.float64) - n64).max())
        assert floor > 0 and float(np.abs(nrm.astype(np.float64) - n64).max()) <= 4 * floor


@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_feature_entry_forms_and_tiling(gpu, prec):
    import torch
    T = _T(prec)
    W, H, spp = 160, 90, 4
    args = _scene("s4")
    full = gpu.render_features(*args, _params(gpu, "s4", W, H, spp), prec)
    # rows / row0
    for k in range(3):
        parts = [gpu.render_features(*args, _params(gpu, "s4", W, H, spp, row0=r0, rows=n), prec)[k] for r0, n in ((0, 37), (37, 1), (38, 52))]
        assert np.array_equal(np.concatenate(parts, axis=-2), full[k]), k
    # 3 interleaved stripes of 4 rows
    out = [np.empty_like(f) for f in full]
    for rank in range(3):
        rows = gpu.stripe_rows(H, 4, 3, rank)
        tile = gpu.render_features(*args, _params(gpu, "s4", W, H, spp, rows=rows, stripe_h=4, stripe_count=3, stripe_rank=rank), prec)
        ys = [y for y0 in range(rank * 4, H, 12) for y in range(y0, min(y0 + 4, H))]
        assert len(ys) == rows
        for k in range(3):
            out[k][..., ys, :] = tile[k]
    for k in range(3):
        assert np.array_equal(out[k], full[k]), k
    # bottom-up rows
    up = gpu.render_features(*args, _params(gpu, "s4", W, H, spp, flags=0x300 | gpu.ROWS_BOTTOM_UP), prec)
    for k in range(3):
        assert np.array_equal(up[k], full[k][..., ::-1, :]), k
    # the three entry forms; single outputs
    with gpu.Scene(args[0], args[1], args[2], prec=prec) as sc:
        p = sc.params(W, H, spp, 6, flags=0x300, seed=31)
        via_scene = sc.render_features(args[3], p)
        tt = torch.float32 if prec == "f32" else torch.float64
        d = [torch.empty(s, dtype=tt, device="cuda") for s in ((3, H, W), (3, H, W), (H, W))]
        st = torch.cuda.Stream()
        sc.render_features_device(args[3], p, d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), st.cuda_stream)
        st.synchronize()
        for k in range(3):
            assert np.array_equal(via_scene[k], full[k]) and np.array_equal(d[k].cpu().numpy(), full[k]), k
        only_depth = sc.render_features(args[3], p, want_albedo=False, want_normal=False)
        assert only_depth[0] is None and only_depth[1] is None and np.array_equal(only_depth[2], full[2])
    assert full[0].dtype == T


# ---------------------------------------------------------------- denoiser
def _random_inputs(W, H, T, seed):
    rng = np.random.default_rng(seed)
    color = (rng.random((3, H, W)) * 2.0).astype(T)
    variance = (rng.random((H, W)) * 0.05).astype(T)
    albedo = rng.random((3, H, W)).astype(T)
    n = rng.normal(size=(3, H, W))
    n /= np.sqrt((n * n).sum(axis=0))
    yy, xx = np.mgrid[0:H, 0:W]
    base = np.where(xx + yy > (W + H) // 2, n[:, :1, :1] * np.ones((1, H, W)), n)        # a flat region (equal normals) beside a rough one
    depth = (5.0 + 0.02 * xx + 0.05 * rng.random((H, W))).astype(T)
    miss = ((xx // 5 + yy // 3) % 4 == 0)                                                  # sky patches: depth 0, normal 0
    depth[miss] = 0
    normal = np.where(miss, 0.0, base).astype(T)
    return color, variance, albedo, normal, depth


def _both(gpu, prec, color, dn_kw, **guides):
    T = _T(prec)
    H, W = color.shape[1:]
    dn = gpu.make_denoise(W, H, post=gpu.POST_NONE, **dn_kw)
    got, _ = gpu.denoise(color, dn, prec=prec, **guides)
    want = dnz.denoise(color, prec=prec, **dn_kw, **guides)
    assert got.dtype == T and want.dtype == T
    return got, want


@pytest.mark.parametrize("prec", ["f32", "f64"])
@pytest.mark.parametrize("W,H,iterations", [(19, 13, 1), (19, 13, 5), (19, 13, 6), (67, 35, 5), (67, 35, 3)])
def test_denoise_bitwise_random_inputs(gpu, W, H, iterations, prec):
    color, variance, albedo, normal, depth = _random_inputs(W, H, _T(prec), 100 * W + iterations)
    got, want = _both(gpu, prec, color, dict(iterations=iterations, sigma_l=4.0, sigma_z=0.1), variance=variance, albedo=albedo, normal=normal, depth=depth)
    assert np.isfinite(want).all() and not np.array_equal(want, color)
    assert np.array_equal(got, want)


@pytest.mark.parametrize("prec", ["f32", "f64"])
@pytest.mark.parametrize("combo", ["all", "none", "variance", "features", "normal_no_depth", "depth_only", "albedo_only"])
def test_denoise_bitwise_guide_combinations(gpu, combo, prec):
    color, variance, albedo, normal, depth = _random_inputs(67, 35, _T(prec), 7)
    # (without a depth plane nothing marks a miss, and a zero normal would zero every weight, the centre's included: unit normals everywhere there)
    unit = np.where((normal == 0).all(axis=0), np.array([0.0, 0.0, 1.0], dtype=normal.dtype)[:, None, None], normal)
    g = {"all": dict(variance=variance, albedo=albedo, normal=normal, depth=depth), "none": {}, "variance": dict(variance=variance),
         "features": dict(albedo=albedo, normal=normal, depth=depth), "normal_no_depth": dict(variance=variance, normal=unit),
         "depth_only": dict(depth=depth), "albedo_only": dict(albedo=albedo)}[combo]
    got, want = _both(gpu, prec, color, dict(iterations=4, sigma_l=2.0, sigma_z=0.3), **g)
    assert np.isfinite(want).all()
    assert np.array_equal(got, want)


@functools.lru_cache(maxsize=None)
def _pipeline(name, W, H, seed, prec):
    """Noisy frame (adaptive, tolerance 0, cap 8), its variance of the mean, features at spp 8 — host arrays from the GPU."""
    from spira_hip import _binding as B
    hdr, _, spp, q = B.render_adaptive(*_scene(name), _params(B, name, W, H, 8, seed=seed), B.make_adaptive(4, 4, 0.0, 0.0), prec)
    assert (spp == 8).all()
    alb, nrm, dep = B.render_features(*_scene(name), _params(B, name, W, H, 8, seed=seed), prec)
    return hdr, dnz.variance_of_mean(hdr, q, spp, prec), alb, nrm, dep


@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_denoise_bitwise_on_the_real_pipeline(gpu, prec):
    hdr, var, alb, nrm, dep = _pipeline("s1", 160, 90, 31, prec)
    got, want = _both(gpu, prec, hdr, dict(iterations=5, sigma_l=4.0, sigma_z=0.1), variance=var, albedo=alb, normal=nrm, depth=dep)
    assert np.isfinite(want).all() and np.array_equal(got, want)
    assert float(np.abs(want - hdr).max()) > 1e-3                    # it filtered
    # the frame holds what the centre-tap rule is for: silhouette pixels whose mean normal is so short that |n|^128 is 0 in Float32
    n2 = (nrm.astype(np.float64) ** 2).sum(axis=0)
    assert ((dep > 0) & (n2 ** 64 < 1.4e-45)).sum() >= 10


@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_denoise_in_place_device_form_and_display_transforms(gpu, prec):
    import torch
    T = _T(prec)
    W, H = 67, 35
    color, variance, albedo, normal, depth = _random_inputs(W, H, T, 11)
    g = dict(variance=variance, albedo=albedo, normal=normal, depth=depth)
    dn = gpu.make_denoise(W, H, iterations=5, post=gpu.POST_NONE)
    ref, _ = gpu.denoise(color, dn, prec=prec, **g)
    # out_hdr aliasing color (host form)
    c2 = color.copy()
    out, _ = gpu.denoise(c2, dn, prec=prec, in_place=True, **g)
    assert out is c2 and np.array_equal(c2, ref)
    # the device form on a non-null stream, out_hdr aliasing color there too
    tt = torch.float32 if prec == "f32" else torch.float64
    st = torch.cuda.Stream()
    d = {k: torch.from_numpy(v).cuda() for k, v in dict(color=color, **g).items()}
    d_out = torch.empty((3, H, W), dtype=tt, device="cuda")
    torch.cuda.synchronize()
    gpu.denoise_device(d["color"].data_ptr(), dn, d_out.data_ptr(), 0, st.cuda_stream, d["variance"].data_ptr(), d["albedo"].data_ptr(),
                       d["normal"].data_ptr(), d["depth"].data_ptr(), prec=prec)
    gpu.denoise_device(d["color"].data_ptr(), dn, d["color"].data_ptr(), 0, st.cuda_stream, d["variance"].data_ptr(), d["albedo"].data_ptr(),
                       d["normal"].data_ptr(), d["depth"].data_ptr(), prec=prec)
    st.synchronize()
    assert np.array_equal(d_out.cpu().numpy(), ref) and np.array_equal(d["color"].cpu().numpy(), ref)
    # out_img: every display transform of out_hdr (Float32: the library's own host transform)
    for post in (gpu.POST_ACES, gpu.POST_ACES_GAMMA, gpu.POST_CLAMP_GAMMA, gpu.POST_NONE):
        dnp = gpu.make_denoise(W, H, iterations=5, post=post)
        hdr, img = gpu.denoise(color, dnp, prec=prec, want_img=True, **g)
        only_img = gpu.denoise(color, dnp, prec=prec, want_hdr=False, want_img=True, **g)
        assert np.array_equal(hdr, ref) and only_img[0] is None and np.array_equal(only_img[1], img)
        if prec == "f32":
            assert np.array_equal(img, gpu.tonemap(hdr, post).reshape(hdr.shape)), hex(post)
        elif post == gpu.POST_NONE:
            assert np.array_equal(img, hdr)


@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_known_answers_on_the_device(gpu, prec):
    T = _T(prec)
    H, W = 13, 19
    run = lambda c, it, **g: gpu.denoise(c, gpu.make_denoise(W, H, iterations=it, post=gpu.POST_NONE), prec=prec, **g)[0]
    c = np.zeros((3, H, W), dtype=T)
    c[:, 6, 9] = 1.0
    want = np.zeros((H, W))
    want[4:9, 7:12] = np.outer(K, K)
    out = run(c, 1)
    for ch in range(3):
        assert np.array_equal(out[ch].astype(np.float64), want)
    for it in range(1, 7):
        assert np.array_equal(run(np.ones((3, H, W), dtype=T), it), np.ones((3, H, W), dtype=T)), it
    depth = np.zeros((H, W), dtype=T)
    depth[:, :9] = 1.0
    split = np.where(depth > 0, T(1.0), T(0.25)).astype(T)[None].repeat(3, axis=0)
    for it in (1, 5):
        assert np.array_equal(run(split, it, depth=depth), split), it
    # variance == 1, constant colour: the filtered variance is not an output, so it is observed through the next iteration's weights —
    # the restatement gives (70/256)^2 at interior pixels (tests/test_denoise_cpu.py) and the device agrees with it bit for bit on a frame
    # whose second iteration depends on that value
    rng = np.random.default_rng(3)
    noisy = (0.5 + 0.2 * rng.random((3, H, W))).astype(T)
    ones = np.ones((H, W), dtype=T)
    got = run(noisy, 2, variance=ones)
    want2, v = dnz.denoise(noisy, variance=ones, iterations=2, prec=prec, return_variance=True)
    assert np.array_equal(got, want2)
    _, v1 = dnz.denoise(np.full((3, H, W), 0.5, dtype=T), variance=ones, iterations=1, prec=prec, return_variance=True)
    assert v1[6, 9] == T((70 / 256) ** 2)


# ---------------------------------------------------------------- it denoises
def _relmse(x, ref):
    x, ref = x.astype(np.float64), ref.astype(np.float64)
    return float((((x - ref) ** 2).sum(axis=0) / ((ref ** 2).sum(axis=0) + 0.01)).mean())


@functools.lru_cache(maxsize=None)
def _reference(name, W, H, seed):
    from spira_hip import _binding as B
    return B.render(*_scene(name), _params(B, name, W, H, 2048, seed=seed + 1000), "f64")[0]


@pytest.mark.parametrize("prec", ["f32", "f64"])
@pytest.mark.parametrize("name,seed", [("s1", 31), ("s2", 32)])
def test_it_denoises(gpu, name, seed, prec):
    W, H = 96, 54
    hdr, var, alb, nrm, dep = _pipeline(name, W, H, seed, prec)
    ref = _reference(name, W, H, seed)
    out, _ = gpu.denoise(hdr, gpu.make_denoise(W, H, iterations=5, post=gpu.POST_NONE, sigma_l=4.0, sigma_z=0.1), variance=var, albedo=alb, normal=nrm, depth=dep, prec=prec)
    noisy, clean = _relmse(hdr, ref), _relmse(out, ref)
    print("denoise ratio", name, prec, "noisy relMSE %.4f" % noisy, "denoised relMSE %.4f" % clean, "ratio %.3f" % (clean / noisy))
    assert clean <= 0.5 * noisy


# ---------------------------------------------------------------- the chain, streams, shutdown
@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_render_denoised_twice_on_two_streams_then_after_shutdown(gpu, prec):
    import torch
    args = _scene("s1")
    W, H = 96, 54
    with gpu.Scene(args[0], args[1], args[2], prec=prec) as sc:
        p = sc.params(W, H, 8, 6, flags=gpu.POST_NONE, seed=31)
        ad = gpu.make_adaptive(4, 4, 0.0, 0.0)
        s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
        a = dnz.render_denoised(sc, args[3], p, ad, feature_spp=8, stream=s1)
        b = dnz.render_denoised(sc, args[3], copy.copy(p), ad, feature_spp=8, stream=s2, want_img=True)
        s1.synchronize(); s2.synchronize()
        ra, rb = a["hdr"].cpu().numpy(), b["hdr"].cpu().numpy()
        gpu.lib().spira_shutdown()
        c = dnz.render_denoised(sc, args[3], p, ad, feature_spp=8)
        torch.cuda.synchronize()
        rc = c["hdr"].cpu().numpy()
    assert np.isfinite(ra).all() and np.array_equal(ra, rb) and np.array_equal(ra, rc)
    assert np.array_equal(b["img"].cpu().numpy(), rb)                 # POST_NONE
    # and the chain is the three entries: the host forms give the same frame
    hdr, var, alb, nrm, dep = _pipeline("s1", W, H, 31, prec)
    assert np.array_equal(a["noisy"].cpu().numpy(), hdr) and np.array_equal(a["depth"].cpu().numpy(), dep)
    var_t = a["variance"].cpu().numpy()
    assert np.allclose(var_t, var, rtol=1e-5 if prec == "f32" else 1e-12, atol=0)
    host, _ = gpu.denoise(hdr, gpu.make_denoise(W, H, iterations=5, post=gpu.POST_NONE), variance=var_t, albedo=alb, normal=nrm, depth=dep, prec=prec)
    assert np.array_equal(host, ra)
