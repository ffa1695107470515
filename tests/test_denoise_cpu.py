"""CPU: first-hit feature buffers (spira_render_features_*) and the a-trous denoiser (spira_denoise_*) without a device — the library exports the
new symbols and the struct mirror has the header's layout, the numpy restatement of the filter (spira_hip/denoise.py, which the GPU tests hold the
kernels to bit for bit) meets hand-made known answers exactly, the plan arithmetic of spira_plan.h survives a sweep under ASan + UBSan, and every
documented argument error comes back before a device is looked for."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from spira_hip import scenes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["spira_render_features_f32", "spira_render_features_f64", "spira_render_features_scene_f32", "spira_render_features_scene_f64",
       "spira_render_features_scene_device_f32", "spira_render_features_scene_device_f64",
       "spira_denoise_f32", "spira_denoise_f64", "spira_denoise_device_f32", "spira_denoise_device_f64"]
K = np.array([1 / 16, 1 / 4, 3 / 8, 1 / 4, 1 / 16])


def test_library_exports_the_new_symbols_and_the_struct_mirror(binding):
    lib = binding.lib()
    for name in NEW:
        assert hasattr(lib, name), name
        assert name in binding.EXPORTS, name
    assert C.sizeof(binding.Denoise) == 32
    assert [n for n, _ in binding.Denoise._fields_] == ["width", "height", "iterations", "post", "sigma_l", "sigma_z"]
    hdr = open(os.path.join(ROOT, "include", "spira_hip.h")).read()
    assert "typedef struct spira_denoise {" in hdr and "uint32_t width, height, iterations, post;" in hdr and "double   sigma_l, sigma_z;" in hdr
    assert lib.spira_abi_version() == 3               # no existing struct grew
    mk = open(os.path.join(ROOT, "julia-spira_amd", "csrc", "Makefile")).read()
    assert "spira_denoise.h" in mk.split("DEPS", 1)[1].split("\n", 1)[0]      # hashed into spira_build_id


def test_kernels_live_in_the_unit_of_their_precision():
    import re
    csrc = os.path.join(ROOT, "julia-spira_amd", "csrc")
    objs = {n: os.path.join(csrc, "spira_tu_%s.o" % n) for n in ("main", "f32", "f64mesh")}
    if not all(os.path.exists(o) for o in objs.values()):
        pytest.skip("objects not present (library built elsewhere)")
    syms = {n: subprocess.run(["nm", o], capture_output=True, text=True, check=True).stdout for n, o in objs.items()}
    for kern in ("10k_features", "17k_denoise_prepare", "14k_denoise_iter"):
        assert len(re.findall(kern + "If", syms["f32"])) > 0 and len(re.findall(kern + "Id", syms["f32"])) == 0, kern
        assert len(re.findall(kern + "Id", syms["main"])) > 0 and len(re.findall(kern + "If", syms["main"])) == 0, kern
        assert len(re.findall(kern + "I[fd]", syms["f64mesh"])) == 0, kern
    # three feature launches per precision: spheres alone, LDS triangles, a BVH mesh
    assert len(set(re.findall(r"10k_featuresIfLb[01]ELb[01]E", syms["f32"]))) == 3
    for fn in ("_ZN8spira_tu4ImplIfE8featuresE", "_ZN8spira_tu4ImplIfE7denoiseE"):
        assert re.search(r" W %s" % fn, syms["f32"]) and re.search(r" U %s" % fn, syms["main"]), fn


# ---- the numpy restatement against known answers (exact: every weight is a dyadic rational)
@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_impulse_gives_the_kernel(prec):
    from spira_hip import denoise
    T = np.float32 if prec == "f32" else np.float64
    c = np.zeros((3, 13, 19), dtype=T)
    c[:, 6, 9] = 1.0
    out = denoise.denoise(c, iterations=1, prec=prec)
    assert out.dtype == T
    want = np.zeros((13, 19))
    want[4:9, 7:12] = np.outer(K, K)
    for ch in range(3):
        assert np.array_equal(out[ch].astype(np.float64), want)


@pytest.mark.parametrize("prec", ["f32", "f64"])
@pytest.mark.parametrize("iterations", [1, 2, 3, 4, 5, 6])
def test_constant_stays_constant_borders_included(prec, iterations):
    from spira_hip import denoise
    T = np.float32 if prec == "f32" else np.float64
    out = denoise.denoise(np.ones((3, 13, 19), dtype=T), iterations=iterations, prec=prec)      # 19 x 13: smaller than the reach 2 * 16 of step 16
    assert np.array_equal(out, np.ones((3, 13, 19), dtype=T))


@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_hit_miss_split_keeps_each_side(prec):
    from spira_hip import denoise
    T = np.float32 if prec == "f32" else np.float64
    depth = np.zeros((13, 19), dtype=T)
    depth[:, :9] = 1.0
    c = np.where(depth > 0, T(1.0), T(0.25)).astype(T)[None].repeat(3, axis=0)
    for it in (1, 5):
        out = denoise.denoise(c, depth=depth, iterations=it, prec=prec)
        assert np.array_equal(out, c), it


@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_unit_variance_shrinks_by_the_kernels_energy(prec):
    from spira_hip import denoise
    T = np.float32 if prec == "f32" else np.float64
    c = np.full((3, 13, 19), 0.5, dtype=T)
    out, v = denoise.denoise(c, variance=np.ones((13, 19), dtype=T), iterations=1, prec=prec, return_variance=True)
    assert np.array_equal(out, c)
    assert v[6, 9] == T((70 / 256) ** 2) and (70 / 256) ** 2 == float(T((70 / 256) ** 2))       # sum k^2 = 70/256; exact in both formats
    assert np.array_equal(v[2:11, 2:17], np.full((9, 15), (70 / 256) ** 2, dtype=T))


@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_centre_tap_keeps_its_weight_under_a_short_normal(prec):
    """A normal averaged over samples that partly missed is short: with one hit in eight |n|^2 = 1/64 and |n|^128 = 2^-384, which is 0 in Float32.
    The centre tap takes no factor, so a silhouette pixel whose neighbours are all cut by the edge keeps its own value instead of becoming 0 / 0."""
    from spira_hip import denoise
    T = np.float32 if prec == "f32" else np.float64
    H, W = 13, 19
    rng = np.random.default_rng(9)
    c = (0.2 + rng.random((3, H, W))).astype(T)
    normal = np.zeros((3, H, W), dtype=T)
    normal[2] = 1.0                                   # everybody faces +z ...
    normal[:, 6, 9] = (0.125, 0.0, 0.0)               # ... except one pixel: the mean of one +x normal and seven misses
    depth = np.ones((H, W), dtype=T)
    var = np.full((H, W), 0.01, dtype=T)
    for guides in (dict(normal=normal, depth=depth), dict(normal=normal), dict(normal=normal, depth=depth, variance=var)):
        out = denoise.denoise(c, iterations=5, prec=prec, **guides)
        assert np.isfinite(out).all(), sorted(guides)
        # every other tap of that pixel weighs 0: five times (9/64 c) / (9/64), a rounding or two each
        assert np.allclose(out[:, 6, 9], c[:, 6, 9], rtol=16 * np.finfo(T).eps, atol=0), sorted(guides)
    # and a pixel of unit normal among equals is filtered as before: the centre's factors were 1 there anyway
    flat = denoise.denoise(c, normal=np.broadcast_to(np.array([0, 0, 1], dtype=T)[:, None, None], (3, H, W)), depth=depth, iterations=1, prec=prec)
    assert np.array_equal(flat, denoise.denoise(c, iterations=1, prec=prec))


def test_restatement_refuses_bad_settings():
    from spira_hip import denoise
    c = np.ones((3, 4, 4))
    for kw in (dict(iterations=0), dict(iterations=7), dict(sigma_l=0.0), dict(sigma_z=-1.0)):
        with pytest.raises(ValueError):
            denoise.denoise(c, **kw)


@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_variance_of_mean(prec):
    from spira_hip import adaptive, denoise
    T = np.float32 if prec == "f32" else np.float64
    rng = np.random.default_rng(5)
    n = 8
    samples = rng.random((n, 3, 6, 7)).astype(T)
    s = np.zeros((3, 6, 7), dtype=T)
    q = np.zeros((6, 7), dtype=T)
    for k in range(n):
        s = s + samples[k]
        y = adaptive.luma(samples[k, 0], samples[k, 1], samples[k, 2], prec)
        q = q + y * y
    hdr = s / T(n)
    v = denoise.variance_of_mean(hdr, q, np.full((6, 7), n, dtype=np.uint32), prec)
    assert v.dtype == T
    ys = adaptive.luma(samples[:, 0], samples[:, 1], samples[:, 2], "f64").astype(np.float64)
    want = ys.var(axis=0, ddof=1) / n
    assert np.allclose(v, want, rtol=2e-4 if prec == "f32" else 1e-10, atol=1e-7 if prec == "f32" else 1e-15)
    # the written order: Y = n * luma(hdr); max(n q - Y Y, 0) / ((n n) (n - 1))
    nn = T(n)
    Y = nn * adaptive.luma(hdr[0], hdr[1], hdr[2], prec)
    d = nn * q - Y * Y
    assert np.array_equal(v, np.where(d > 0, d, T(0)) / ((nn * nn) * (nn - T(1))))


def test_denoise_plan_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "denoise_plan")
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g", "-O1"]
    subprocess.run(["g++", "-std=c++17", "-ffp-contract=off", os.path.join(ROOT, "tests", "native", "denoise_plan.cpp"), "-o", exe] + san, check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-6000:]
    assert "all checks passed" in r.stdout and "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr


def test_feature_argument_validation_runs_before_the_device(binding):
    s = scenes.scene_s1()
    sp, ma, cam = s["spheres5"], s["materials8"], s["camera12"]

    def err(params, prec="f32", **kw):
        with pytest.raises(binding.SpiraError) as e:
            binding.render_features(sp, ma, None, cam, params, prec, **kw)
        return str(e.value)
    P = lambda **kw: binding.make_params(16, 9, kw.pop("spp", 4), kw.pop("depth", 4), 5, 5, **kw)
    for prec in ("f32", "f64"):
        assert "error -1" in err(P(), prec, want_albedo=False, want_normal=False, want_depth=False)      # no output at all
        assert "error -1" in err(P(rows=4, row0=8), prec)                                                # row0 + rows > height
        assert "error -1" in err(P(rows=4, stripe_h=2, stripe_count=3, stripe_rank=3), prec)             # bad stripe parameters
        assert "error -4" in err(P(spp=0), prec) and "error -4" in err(P(spp=(1 << 24) + 1), prec)       # the limits of every entry
        for flags in (binding.SEM_CPU, binding.SEM_METAL, binding.SEM_HYBRID, binding.KERNEL_MEGA, binding.KERNEL_BOUNCE, binding.KERNEL_WAVEFRONT,
                      binding.EXT_DIELECTRIC, binding.EXT_SPECTRAL):
            assert "error -5" in err(P(flags=flags), prec), hex(flags)
        if binding.device_count() == 0:               # max_depth is not used: 0 is a valid call, and a valid call fails loudly without a device
            assert "error -2" in err(P(depth=0), prec)
            assert "error -2" in err(P(), prec, want_albedo=False, want_normal=False)
    lib = binding.lib()
    assert lib.spira_render_features_f32(None, None, None, None, None, None, None, None) == -1
    assert lib.spira_render_features_scene_f64(None, None, None, None, None, None) == -1
    assert lib.spira_render_features_scene_device_f32(None, None, None, None, None, None, None) == -1


def test_denoise_argument_validation_runs_before_the_device(binding):
    def err(dn, prec="f32", color=True, **kw):
        T = np.float32 if prec == "f32" else np.float64
        c = np.ones((3, max(dn.height, 1), max(dn.width, 1)), dtype=T)
        fn = binding.lib().spira_denoise_f32 if prec == "f32" else binding.lib().spira_denoise_f64
        out = np.empty_like(c)
        want_hdr, want_img = kw.get("want_hdr", True), kw.get("want_img", False)
        return fn(c.ctypes.data_as(C.c_void_p) if color else None, None, None, None, None, C.byref(dn),
                  out.ctypes.data_as(C.c_void_p) if want_hdr else None, out.ctypes.data_as(C.c_void_p) if want_img else None)
    D = binding.make_denoise
    for prec in ("f32", "f64"):
        for bad in (D(0, 9), D(16, 0), D(16, 9, iterations=0), D(16, 9, iterations=7), D(16, 9, sigma_l=0.0), D(16, 9, sigma_l=-1.0),
                    D(16, 9, sigma_l=float("nan")), D(16, 9, sigma_z=0.0), D(16, 9, sigma_z=float("nan")), D(16, 9, post=0x400), D(16, 9, post=1),
                    D(16, 9, post=binding.ROWS_BOTTOM_UP)):
            assert err(bad, prec) == -1, (bad.width, bad.height, bad.iterations, bad.post, bad.sigma_l, bad.sigma_z)
        assert err(D(16, 9), prec, color=False) == -1                            # color is required
        assert err(D(16, 9), prec, want_hdr=False, want_img=False) == -1         # both outputs NULL
        for post in (binding.POST_ACES, binding.POST_ACES_GAMMA, binding.POST_CLAMP_GAMMA, binding.POST_NONE):
            for it in (1, 6):
                rc = err(D(16, 9, iterations=it, post=post), prec)
                assert rc == (-2 if binding.device_count() == 0 else 0), (post, it, rc)
        assert err(D(1, 1), prec, want_hdr=False, want_img=True) == (-2 if binding.device_count() == 0 else 0)      # width, height >= 1 is all it asks
    lib = binding.lib()
    assert lib.spira_denoise_f32(None, None, None, None, None, None, None, None) == -1
    assert lib.spira_denoise_device_f64(None, None, None, None, None, None, None, None, None) == -1
    # the device form checks the same things in the same place
    one = np.ones(1, dtype=np.float32)
    ptr = one.ctypes.data_as(C.c_void_p)          # never dereferenced: the argument error comes first
    assert lib.spira_denoise_device_f32(ptr, None, None, None, None, C.byref(D(16, 9, iterations=7)), ptr, None, None) == -1
    assert lib.spira_denoise_device_f32(ptr, None, None, None, None, C.byref(D(16, 9)), None, None, None) == -1
