"""CPU: light probes (spira_scene_probe_sh_*, spira_probe_rays_*, spira_sh9_basis_*) without a device — header, binding and library agree; the host
generator and the host basis equal their numpy twins (spira_hip.bake.sphere_rays, bake.sh9) bit for bit; an invalid point of every kind gives six zeros
and leaves the neighbours alone; the directions are uniform on the sphere (the basis comes out orthonormal under them); sh9_radiance and sh9_irradiance
reproduce the closed forms of the analytic sky; every argument error comes back as documented, never as SPIRA_E_NO_DEVICE; and the generator and the
basis pass tests/native/probe_plan.cpp under ASan + UBSan, bit for bit against the twins."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from spira_hip import bake, cameras

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RAYS = ["spira_probe_rays_f32", "spira_probe_rays_f64", "spira_probe_rays_device_f32", "spira_probe_rays_device_f64"]
PROBE = ["spira_scene_probe_sh_f32", "spira_scene_probe_sh_f64", "spira_scene_probe_sh_device_f32", "spira_scene_probe_sh_device_f64"]
BASIS = ["spira_sh9_basis_f32", "spira_sh9_basis_f64"]
TUPLES = ((0, 0, 0), (5, 0x1234567890, 77), ((1 << 24) - 1, 3, 0xFFFFFFFF - 999), (17, 2 ** 64 - 1, 1 << 31))      # (sample, seed, key0): test_gather_cpu.py's


def _T(prec):
    return np.float32 if prec == "f32" else np.float64


def _random_points(n, seed=0):
    rng = np.random.default_rng(seed)
    return rng.normal(size=(n, 3)) * 3 * rng.uniform(0.01, 50, size=(n, 1))


def test_library_header_and_binding_name_the_entries(binding):
    lib = binding.lib()
    hdr = open(os.path.join(ROOT, "include", "spira_hip.h")).read()
    for name in RAYS:
        assert hasattr(lib, name) and name in binding.EXPORTS and re.search(r"^int %s\(const (float|double) \*(d_)?points3, uint32_t n_points, uint32_t sample, " % name, hdr, flags=re.M), name
    for name in PROBE:
        assert hasattr(lib, name) and name in binding.EXPORTS and re.search(r"^int %s\(const spira_scene \*scene, const (float|double) \*(d_)?points3, " % name, hdr, flags=re.M), name
    for name in BASIS:
        assert hasattr(lib, name) and name in binding.EXPORTS and re.search(r"^void %s\(const (float|double) d_unit\[3\], (float|double) out9\[9\]\);" % name, hdr, flags=re.M), name
    assert "#define SPIRA_ABI_VERSION 3 " in hdr and lib.spira_abi_version() == 3
    assert C.sizeof(binding.Radiance) == 32                                            # the probe entry reuses spira_radiance unchanged
    for m in ("probe_sh", "probe_sh_device"):
        assert hasattr(binding.Scene, m), m
    for f in ("probe_rays", "probe_rays_device", "sh9_basis"):
        assert hasattr(binding, f), f
    for f in ("sphere_rays", "sh9", "light_probes", "probe_grid", "probes_outside", "sh9_radiance", "sh9_irradiance"):
        assert hasattr(bake, f), f


def test_the_probe_methods_of_the_handle_keep_their_signatures(binding):
    """The two public methods this surface adds to a handle, with their parameters, their order and their defaults (they live in the base class
    _SceneProbes of Scene, and reach a handle through it)."""
    import inspect
    want = {"probe_sh": "(self, points3, spp, max_depth, seed=0, sample0=0, key0=0, flags=0, sums=None, want_valid=False)",
            "probe_sh_device": "(self, d_points_ptr, n_points, spp, max_depth, d_sums_ptr, seed=0, sample0=0, key0=0, flags=0, d_valid_ptr=0, stream_ptr=0)"}
    have = {name: str(inspect.signature(f)) for name, f in vars(binding._SceneProbes).items() if not name.startswith("_") and callable(f)}
    assert have == want and issubclass(binding.Scene, binding._SceneProbes)
    for name in want:
        assert getattr(binding.Scene, name) is getattr(binding._SceneProbes, name)
    sig = {"probe_rays": "(points3, sample=0, seed=0, key0=0, prec='f32')",
           "probe_rays_device": "(d_points_ptr, n_points, d_rays_ptr, sample=0, seed=0, key0=0, stream_ptr=0, prec='f32')", "sh9_basis": "(d, prec='f32')"}
    assert {n: str(inspect.signature(getattr(binding, n))) for n in sig} == sig


def test_the_header_is_hashed_into_the_build_id_and_included_behind_the_gather():
    mk = open(os.path.join(ROOT, "julia-spira_amd", "csrc", "Makefile")).read()
    assert "spira_probe.h" in mk.split("DEPS", 1)[1].split("\n", 1)[0]
    src = open(os.path.join(ROOT, "julia-spira_amd", "csrc", "spira_hip.hip")).read()
    assert src.index('#include "spira_gather.h"') < src.index('#include "spira_probe.h"')


def test_the_kernels_sit_in_the_unit_of_their_precision():
    csrc = os.path.join(ROOT, "julia-spira_amd", "csrc")
    objs = {n: os.path.join(csrc, "spira_tu_%s.o" % n) for n in ("main", "f32", "f64mesh")}
    if not all(os.path.exists(o) for o in objs.values()):
        pytest.skip("objects not present (library built elsewhere)")
    syms = {n: subprocess.run(["nm", o], capture_output=True, text=True, check=True).stdout for n, o in objs.items()}
    count = lambda text, pat: len(re.findall(pat, text))
    for kern in ("7k_probe", "11k_probe_sum", "12k_probe_rays"):
        assert count(syms["main"], kern + "If") == 0 and count(syms["main"], kern + "Id") > 0, kern
        assert count(syms["f32"], kern + "Id") == 0 and count(syms["f32"], kern + "If") > 0, kern
        assert count(syms["f64mesh"], kern + "I[fd]") == 0, kern
    for unit, t in (("main", "d"), ("f32", "f")):
        assert len(set(re.findall(r"_ZN5spira7k_probeI%sLb[01]ELb[01]EEEvNS_9ProbeArgsIT_EE" % t, syms[unit]))) == 4      # BVH x EXT
    for fn in ("_ZN8spira_tu4ImplIfE8probe_shE", "_ZN8spira_tu4ImplIfE10probe_raysE"):
        assert re.search(r" W %s" % fn, syms["f32"]) and re.search(r" U %s" % fn, syms["main"]), fn


@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_the_host_generator_equals_its_twin(binding, prec):
    pts = _random_points(1000, 1)
    for sample, seed, key0 in TUPLES:
        got = binding.probe_rays(pts, sample, seed, key0, prec)
        want = bake.sphere_rays(pts, sample, seed, key0, prec)
        assert got.dtype == _T(prec) and got.shape == (1000, 6) and np.array_equal(got, want), (sample, seed, key0)
        assert np.array_equal(got[:, 0:3], pts.astype(_T(prec)))
        valid, d = cameras.ray_prepare(got, prec)                                      # the radiance entry's own classification: every ray valid
        assert valid.all() and np.abs((d.astype(np.float64) ** 2).sum(axis=1) - 1).max() <= 4 * np.finfo(_T(prec)).eps
    # the key is key0 + k: a chunk of the list with key0 advanced is the same rays; another sample, seed or key is another direction
    whole = binding.probe_rays(pts, 3, 9, 100, prec)
    assert np.array_equal(binding.probe_rays(pts[300:], 3, 9, 400, prec), whole[300:])
    for other in (binding.probe_rays(pts, 4, 9, 100, prec), binding.probe_rays(pts, 3, 10, 100, prec), binding.probe_rays(pts, 3, 9, 101, prec)):
        assert (other[:, 3:6] != whole[:, 3:6]).any(axis=1).mean() > 0.99
    # the draw is the gather's q: with the normal taken away, the gather's direction is the probe's
    p6 = np.concatenate([pts, np.tile([0.0, 1.0, 0.0], (1000, 1))], axis=1)
    hemi = bake.hemisphere_rays(p6, 3, 9, 100, prec)
    assert np.array_equal((hemi[:, 3:6] - np.array([0, 1, 0], dtype=_T(prec)))[:, [0, 2]], whole[:, [3, 5]])


@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_the_host_basis_equals_its_twin(binding, prec):
    T = _T(prec)
    rays = binding.probe_rays(_random_points(1000, 2), 1, 7, 0, prec)
    _, d = cameras.ray_prepare(rays, prec)
    axes = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]], dtype=T)
    d = np.concatenate([d, axes])
    got = binding.sh9_basis(d, prec)
    want = bake.sh9(d)
    assert got.dtype == T and want.dtype == T and got.shape == (1006, 9) and np.array_equal(got, want)
    assert np.array_equal(binding.sh9_basis(d[5], prec), want[5])
    c0, c1, c2, c3, c4 = (T(c) for c in bake.SH9_C)
    assert np.array_equal(want[-6:, 0], np.full(6, c0)) and np.array_equal(want[-6:, [3, 1, 2]][[0, 2, 4]], np.diag([c1, c1, c1]))
    assert (want[-6:, [4, 5, 7]] == 0).all() and np.array_equal(want[-6:, 6], [-c3, -c3, -c3, -c3, c3 * T(2), c3 * T(2)])
    assert np.array_equal(want[-6:, 8], [c4, c4, -c4, -c4, 0, 0])
    with pytest.raises(ValueError):
        binding.sh9_basis(np.zeros((4, 2)), prec)


def _invalid_rows(T):
    good = np.array([0.25, 1.0, 3.0], dtype=T)
    rows = []
    for k in range(3):
        for v in (np.nan, np.inf, -np.inf):
            r = good.copy(); r[k] = v; rows.append(r)
    return np.array(rows, dtype=T)


@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_invalid_points_give_six_zeros_and_leave_their_neighbours_alone(binding, prec):
    T = _T(prec)
    bad = _invalid_rows(T)
    good = _random_points(len(bad) + 1, 2).astype(T)
    mixed = np.empty((2 * len(bad) + 1, 3), dtype=T)
    mixed[0::2] = good
    mixed[1::2] = bad
    got = binding.probe_rays(mixed, 2, 11, 50, prec)
    assert np.array_equal(got, bake.sphere_rays(mixed, 2, 11, 50, prec))
    assert (got[1::2] == 0).all() and not np.signbit(got[1::2]).any()
    valid, _ = cameras.ray_prepare(got, prec)                                          # the radiance entry's own classification of the generated list
    assert valid[0::2].all() and not valid[1::2].any()
    # the neighbours: what the same points give at the same keys with every invalid point replaced by a valid one
    clean = mixed.copy()
    clean[1::2] = good[:-1]
    assert np.array_equal(binding.probe_rays(clean, 2, 11, 50, prec)[0::2], got[0::2])
    # there is no origin rule and no rule on magnitude: the largest finite point is valid
    edge = np.full((1, 3), np.finfo(T).max, dtype=T)
    assert cameras.ray_prepare(binding.probe_rays(edge, 0, 0, 0, prec), prec)[0].all()


@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_the_directions_are_uniform_on_the_sphere(binding, prec):
    """Under the uniform density 1 / (4 pi) the nine functions are orthonormal: (4 pi / N) sum_k Y_i(d_k) Y_j(d_k) -> delta_ij.  N = 2^16 directions of one
    point list (point k draws under key k), seed fixed.  The bound on every entry is 6 standard errors of its own mean, the standard error from the sample
    variance of the N products 4 pi Y_i Y_j — a derived bound, nothing measured — plus the rounding of the basis, which is all that is left where a product
    is constant (i = j = 0: variance 0): a Y is at most three operations in T on values below 1.1, a product 4 pi Y_i Y_j stays below 5.1 (Y6 = 2 c3 on the
    z axis), so its error is below 5.1 * 2 * 3 * eps / 2 < 16 eps."""
    T = _T(prec)
    N = 1 << 16
    pts = np.tile([1.0, -2.0, 0.5], (N, 1))
    valid, d = cameras.ray_prepare(binding.probe_rays(pts, 1, 42, 0, prec), prec)
    assert valid.all()
    Y = bake.sh9(d).astype(np.float64)
    floor = 16 * np.finfo(T).eps
    worst = 0.0
    for i in range(9):
        for j in range(i, 9):
            prod = 4 * np.pi * Y[:, i] * Y[:, j]
            se = prod.std(ddof=1) / np.sqrt(N)
            err = abs(prod.mean() - (1.0 if i == j else 0.0))
            worst = max(worst, err / (6 * se + floor))
            assert err <= 6 * se + floor, (i, j, err, se)
    print(prec, "worst |mean - delta| / bound:", worst)
    # the samples of ONE point (samples 0 .. 2^12 - 1 at one key) obey the same law
    M = 1 << 12
    one = np.stack([binding.probe_rays(pts[:1], s, 42, 5, prec)[0] for s in range(M)])
    Y1 = bake.sh9(cameras.ray_prepare(one, prec)[1]).astype(np.float64)
    for i in range(9):
        for j in range(i, 9):
            prod = 4 * np.pi * Y1[:, i] * Y1[:, j]
            assert abs(prod.mean() - (1.0 if i == j else 0.0)) <= 6 * prod.std(ddof=1) / np.sqrt(M) + floor, (i, j)


def test_irradiance_and_radiance_of_the_analytic_sky():
    """The sky of sky_term (csrc/spira_device.h) is L(d) = a + b d.y per channel, a = (1 + c) / 2, b = (c - 1) / 2, c = (0.5, 0.7, 1.0): bands 0 and 1 only.
    Its coefficients are a sqrt(4 pi) at j = 0 and b c1 4 pi / 3 at j = 1; they give back L(d) = a + b d.y and E(n) = pi a + (2 pi / 3) b n.y."""
    c = np.array([0.5, 0.7, 1.0])
    a, b = (1 + c) / 2, (c - 1) / 2
    coeffs = np.zeros((9, 3))
    coeffs[0] = a * np.sqrt(4 * np.pi)
    coeffs[1] = b * bake.SH9_C[1] * 4 * np.pi / 3
    rng = np.random.default_rng(5)
    dirs = rng.normal(size=(500, 3))
    dirs /= np.linalg.norm(dirs, axis=1)[:, None]
    L = bake.sh9_radiance(coeffs, dirs)
    E = bake.sh9_irradiance(coeffs, dirs)
    L_want = a[None, :] + b[None, :] * dirs[:, 1:2]
    E_want = np.pi * a[None, :] + (2 * np.pi / 3) * b[None, :] * dirs[:, 1:2]
    assert L.shape == E.shape == (500, 3)
    assert np.abs(L - L_want).max() <= 1e-12 * np.abs(L_want).max() and np.abs(E - E_want).max() <= 1e-12 * np.abs(E_want).max()
    assert np.abs(L / L_want - 1).max() <= 1e-12 and np.abs(E / E_want - 1).max() <= 1e-12
    # one set of coefficients per direction, and a single direction
    many = np.tile(coeffs, (500, 1, 1))
    assert np.array_equal(bake.sh9_irradiance(many, dirs), E) and np.array_equal(bake.sh9_radiance(coeffs, dirs[3]), L[3])
    # the bands above 1 carry their own factor: a pure Y6 of unit weight towards +z gives (pi / 4) Y6(z)
    only6 = np.zeros((9, 3)); only6[6] = 1.0
    z = np.array([0.0, 0.0, 1.0])
    assert np.allclose(bake.sh9_irradiance(only6, z), (np.pi / 4) * 2 * bake.SH9_C[3], rtol=1e-15)


def test_probe_grid_is_the_voxel_centres():
    from spira_hip import query
    for prec in ("f32", "f64"):
        g = bake.probe_grid([-1.0, 0.0, 2.0], [3.0, 1.0, 2.5], (4, 2, 3), prec)
        assert g.shape == (24, 3) and g.dtype == _T(prec) and g.flags["C_CONTIGUOUS"]
        assert np.array_equal(g, query.voxel_boxes([-1.0, 0.0, 2.0], [3.0, 1.0, 2.5], (4, 2, 3), _T(prec))[:, 0:3])
        assert np.allclose(g[0], [-0.5, 0.25, 2.0 + 0.5 / 6]) and np.allclose(g[-1], [2.5, 0.75, 2.5 - 0.5 / 6])
        assert g[1, 2] > g[0, 2] and g[1, 0] == g[0, 0]                                # x slowest, z fastest


def test_return_codes_without_a_device(binding):
    """Every argument error that needs no handle is decided before any device is touched: its own code, never SPIRA_E_NO_DEVICE (-2)."""
    lib = binding.lib()
    buf = np.zeros(128, dtype=np.float64)
    p = buf.ctypes.data_as(C.c_void_p)
    u32, u64 = C.c_uint32, C.c_uint64
    err = lambda: lib.spira_last_error()
    R = binding.Radiance

    def rp(spp=1, depth=4, flags=0, sample0=0, seed=0, key0=0, reserved=0):
        return C.byref(R(spp, depth, flags, sample0, seed, key0, reserved))
    for name in PROBE:
        fn = getattr(lib, name)
        tail = (None,) if "device" in name else ()
        call = lambda pts, n, r, sums: fn(None, pts, u32(n), r, sums, None, *tail)
        assert call(None, 4, rp(), p) == -1 and b"point array is NULL" in err(), name
        assert call(p, 4, None, p) == -1 and b"struct is NULL" in err(), name
        assert call(p, 4, rp(), None) == -1 and b"sum_sh is NULL" in err(), name
        assert call(None, 4, None, None) == -1 and b"point array is NULL" in err(), name
        assert call(p, 0, rp(), p) == -1 and b"n_points is 0" in err(), name
        assert call(p, 4, rp(spp=0), p) == -1 and b"spp is 0" in err(), name
        assert call(p, 4, rp(depth=0), p) == -1 and call(p, 4, rp(depth=256), p) == -1 and b"max_depth" in err(), name
        assert call(p, 4, rp(reserved=1), p) == -1 and b"reserved" in err(), name
        for bad in (binding.KERNEL_MEGA, binding.SEM_CPU, binding.POST_NONE, binding.ROWS_BOTTOM_UP, 0x80000000):
            assert call(p, 4, rp(flags=bad), p) == -5 and b"probe entries" in err(), (name, bad)
        assert call(p, (1 << 26) + 1, rp(), p) == -4 and b"SPIRA_MAX_RAYS" in err(), name
        assert call(p, 4, rp(key0=0xFFFFFFFD), p) == -4 and b"key0" in err(), name
        assert call(p, 4, rp(spp=8, sample0=(1 << 24) - 7), p) == -4 and b"sample0" in err(), name
        # everything in order — 2^26 points x 2^24 samples included: the call gets as far as the handle
        for flags in (0, binding.EXT_DIELECTRIC, binding.EXT_SPECTRAL, binding.EXT_DIELECTRIC | binding.EXT_SPECTRAL):
            assert call(p, 4, rp(flags=flags, depth=255, key0=0xFFFFFFFC, spp=8, sample0=(1 << 24) - 8), p) == -1 and b"scene handle is NULL" in err(), name
        assert call(p, 1 << 26, rp(spp=1 << 24), p) == -1 and b"scene handle is NULL" in err(), name
    for name in RAYS:
        fn = getattr(lib, name)
        tail = (None,) if "device" in name else ()
        call = lambda pts, n, sample, key0, out: fn(pts, u32(n), u32(sample), u64(0), u32(key0), out, *tail)
        assert call(None, 4, 0, 0, p) == -1 and b"point array is NULL" in err(), name
        assert call(p, 4, 0, 0, None) == -1 and b"ray array is NULL" in err(), name
        assert call(p, 0, 0, 0, p) == -1 and b"n_points is 0" in err(), name
        assert call(p, (1 << 26) + 1, 0, 0, p) == -4 and b"SPIRA_MAX_RAYS" in err(), name
        assert call(p, 4, 0, 0xFFFFFFFD, p) == -4 and b"key0" in err(), name
        assert call(p, 4, 1 << 24, 0, p) == -4 and b"sample" in err(), name


def test_python_wrappers_refuse_misshapen_arrays(binding):
    class _NoHandle(binding.Scene):
        def __init__(self):
            self.prec, self._h = "f32", None
    s = _NoHandle()
    with pytest.raises(ValueError):
        s.probe_sh(np.zeros((4, 6)), 1, 4)
    with pytest.raises(ValueError):
        s.probe_sh(np.zeros((4, 3)), 1, 4, sums=np.zeros((4, 9, 3), dtype=np.float64))
    with pytest.raises(ValueError):
        s.probe_sh(np.zeros((4, 3)), 1, 4, sums=np.zeros((4, 27), dtype=np.float32))
    with pytest.raises(ValueError):
        binding.probe_rays(np.zeros((4, 6)))
    with pytest.raises(binding.SpiraError) as e:                                       # a NULL handle: the library's own refusal, no device touched
        s.probe_sh(np.zeros((4, 3)), 1, 4)
    assert "error -1" in str(e.value)


@pytest.fixture(scope="module")
def probe_plan_exe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("probe") / "probe_plan")
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g", "-O1"]
    subprocess.run(["g++", "-std=c++17", "-ffp-contract=off", os.path.join(ROOT, "tests", "native", "probe_plan.cpp"), "-o", exe] + san, check=True)
    return exe


def _run(exe, text):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], input=text, capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-6000:]
    assert "rules checked" in r.stdout and "all checks passed" in r.stdout and "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr
    return r.stdout


@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_generator_and_basis_under_asan_ubsan(probe_plan_exe, prec):
    T = _T(prec)
    U = np.uint32 if prec == "f32" else np.uint64
    hexrow = lambda a: " ".join("%x" % int(w) for w in np.ascontiguousarray(a, dtype=T).view(U))
    pts = np.concatenate([_random_points(200, 3).astype(T), _invalid_rows(T)])
    sample, seed, key0 = 6, 0xABCDEF0123, 4000
    text = prec + "\n" + "".join("gen %x %x %x %s\n" % (sample, seed, key0 + k, hexrow(r)) for k, r in enumerate(pts))
    out = _run(probe_plan_exe, text)
    got = re.findall(r"^gen (\d)" + r" ([0-9a-f]+)" * 18 + "$", out, flags=re.M)
    assert len(got) == len(pts)
    want = bake.sphere_rays(pts, sample, seed, key0, prec)
    valid, d = cameras.ray_prepare(want, prec)
    verdicts = np.array([int(g[0]) for g in got], dtype=bool)
    assert np.array_equal(verdicts, valid) and valid[:200].all() and not valid[200:].any()
    bits = np.array([[int(x, 16) for x in g[1:]] for g in got], dtype=U)
    assert np.array_equal(bits[:, 0:6], want.view(U))
    assert np.array_equal(bits[valid, 6:9], np.ascontiguousarray(d[valid]).view(U))    # the direction the kernels trace along: radiance_ray_prepare's
    assert np.array_equal(bits[valid, 9:18], np.ascontiguousarray(bake.sh9(d[valid])).view(U))
