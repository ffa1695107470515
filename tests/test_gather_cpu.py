"""CPU: the hemisphere gather (spira_gather_rays_*, spira_scene_gather_*, spira_scene_gather_visible_*) without a device — header, binding and library
agree; the host generator equals its numpy twin (spira_hip.bake.hemisphere_rays) bit for bit, writes six zeros for every kind of invalid point and
leaves the neighbours alone; its directions are cosine-weighted about the normal; every argument error comes back as documented, never as
SPIRA_E_NO_DEVICE; and the launch plan and the generator pass tests/native/gather_plan.cpp under ASan + UBSan, the generator bit for bit against the twin."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from spira_hip import bake, cameras

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RAYS = ["spira_gather_rays_f32", "spira_gather_rays_f64", "spira_gather_rays_device_f32", "spira_gather_rays_device_f64"]
GATHER = ["spira_scene_gather_f32", "spira_scene_gather_f64", "spira_scene_gather_device_f32", "spira_scene_gather_device_f64"]
VISIBLE = ["spira_scene_gather_visible_f32", "spira_scene_gather_visible_f64", "spira_scene_gather_visible_device_f32", "spira_scene_gather_visible_device_f64"]


def _T(prec):
    return np.float32 if prec == "f32" else np.float64


def _random_points(n, seed=0):
    rng = np.random.default_rng(seed)
    pts = rng.normal(size=(n, 6)) * np.array([3, 3, 3, 1, 1, 1]) * rng.uniform(0.01, 50, size=(n, 1))      # non-unit normals of many lengths
    return pts


def test_library_header_and_binding_name_the_entries(binding):
    lib = binding.lib()
    hdr = open(os.path.join(ROOT, "include", "spira_hip.h")).read()
    for name in RAYS:
        assert hasattr(lib, name) and name in binding.EXPORTS and re.search(r"^int %s\(const (float|double) \*(d_)?points6, uint32_t n_points, uint32_t sample, " % name, hdr, flags=re.M), name
    for name in GATHER + VISIBLE:
        assert hasattr(lib, name) and name in binding.EXPORTS and re.search(r"^int %s\(const spira_scene \*scene, " % name, hdr, flags=re.M), name
    assert hasattr(lib, "spira_debug_gather_plan") and "spira_debug_gather_plan" not in hdr
    assert "#define SPIRA_ABI_VERSION 3 " in hdr and lib.spira_abi_version() == 3
    for m in ("gather", "gather_device", "gather_visible", "gather_visible_device"):
        assert hasattr(binding.Scene, m), m
    for f in ("gather_rays", "gather_rays_device", "gather_plan"):
        assert hasattr(binding, f), f
    for f in ("hemisphere_rays", "triangle_points", "irradiance", "ambient_occlusion"):
        assert hasattr(bake, f), f


def test_struct_mirror_matches_the_header_field_by_field(binding):
    from test_abi_cpu import _header_struct_fields
    ctype_of = {"uint32_t": C.c_uint32, "uint64_t": C.c_uint64, "double": C.c_double}
    fields = _header_struct_fields("spira_gather_visible")
    mirror = binding.GatherVisible
    assert [n for _, n in fields] == [n for n, _ in mirror._fields_]
    assert [ctype_of[t] for t, _ in fields] == [t for _, t in mirror._fields_]
    assert C.sizeof(mirror) == 40 == sum(C.sizeof(ctype_of[t]) for t, _ in fields)      # no padding either side
    assert (mirror.seed.offset, mirror.key0.offset, mirror.t_min.offset, mirror.t_max.offset) == (8, 16, 24, 32)
    assert C.sizeof(binding.Radiance) == 32      # the radiance gather reuses spira_radiance unchanged


def test_the_header_is_hashed_into_the_build_id_and_included_behind_radiance():
    mk = open(os.path.join(ROOT, "julia-spira_amd", "csrc", "Makefile")).read()
    assert "spira_gather.h" in mk.split("DEPS", 1)[1].split("\n", 1)[0]
    src = open(os.path.join(ROOT, "julia-spira_amd", "csrc", "spira_hip.hip")).read()
    assert src.index('#include "spira_radiance.h"') < src.index('#include "spira_gather.h"')


def test_the_kernels_sit_in_the_unit_of_their_precision():
    csrc = os.path.join(ROOT, "julia-spira_amd", "csrc")
    objs = {n: os.path.join(csrc, "spira_tu_%s.o" % n) for n in ("main", "f32", "f64mesh")}
    if not all(os.path.exists(o) for o in objs.values()):
        pytest.skip("objects not present (library built elsewhere)")
    syms = {n: subprocess.run(["nm", o], capture_output=True, text=True, check=True).stdout for n, o in objs.items()}
    count = lambda text, pat: len(re.findall(pat, text))
    for kern in ("8k_gather", "12k_gather_sum", "13k_gather_rays", "16k_gather_visible", "24k_gather_visible_session"):
        assert count(syms["main"], kern + "If") == 0 and count(syms["main"], kern + "Id") > 0, kern
        assert count(syms["f32"], kern + "Id") == 0 and count(syms["f32"], kern + "If") > 0, kern
        assert count(syms["f64mesh"], kern + "I[fd]") == 0, kern
    for unit, t in (("main", "d"), ("f32", "f")):
        assert len(set(re.findall(r"_ZN5spira8k_gatherI%sLb[01]ELb[01]EEEvNS_10GatherArgsIT_EE" % t, syms[unit]))) == 4      # BVH x EXT
        assert len(set(re.findall(r"_ZN5spira16k_gather_visibleI%sLb[01]ELb[01]EEEvNS_17GatherVisibleArgsIT_EE" % t, syms[unit]))) == 3
    for fn in ("_ZN8spira_tu4ImplIfE6gatherE", "_ZN8spira_tu4ImplIfE14gather_visibleE", "_ZN8spira_tu4ImplIfE11gather_raysE"):
        assert re.search(r" W %s" % fn, syms["f32"]) and re.search(r" U %s" % fn, syms["main"]), fn


@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_the_host_generator_equals_its_twin(binding, prec):
    pts = _random_points(1000, 1)
    for sample, seed, key0 in ((0, 0, 0), (5, 0x1234567890, 77), ((1 << 24) - 1, 3, 0xFFFFFFFF - 999), (17, 2 ** 64 - 1, 1 << 31)):
        got = binding.gather_rays(pts, sample, seed, key0, prec)
        want = bake.hemisphere_rays(pts, sample, seed, key0, prec)
        assert got.dtype == _T(prec) and got.shape == (1000, 6) and np.array_equal(got, want), (sample, seed, key0)
        assert np.array_equal(got[:, 0:3], pts[:, 0:3].astype(_T(prec)))
    # the key is key0 + k: a chunk of the list with key0 advanced is the same rays; another sample, seed or key is another direction
    whole = binding.gather_rays(pts, 3, 9, 100, prec)
    assert np.array_equal(binding.gather_rays(pts[300:], 3, 9, 400, prec), whole[300:])
    for other in (binding.gather_rays(pts, 4, 9, 100, prec), binding.gather_rays(pts, 3, 10, 100, prec), binding.gather_rays(pts, 3, 9, 101, prec)):
        assert (other[:, 3:6] != whole[:, 3:6]).any(axis=1).mean() > 0.99


def _invalid_rows(T):
    fi = np.finfo(T)
    good = np.array([0.25, 1.0, 3.0, 0.3, -0.4, -1.2], dtype=T)
    rows = []
    for k in range(6):
        for v in (np.nan, np.inf, -np.inf):
            r = good.copy(); r[k] = v; rows.append(r)
    r = good.copy(); r[3:6] = 0; rows.append(r)                                        # a zero normal
    r = good.copy(); r[3:6] = fi.smallest_subnormal; rows.append(r)                    # a subnormal-length normal: n.n underflows to 0
    r = good.copy(); r[3:6] = [0, T(np.sqrt(np.float64(fi.tiny)) * 0.5), 0]; rows.append(r)      # n.n just below the smallest normal
    r = good.copy(); r[3:6] = fi.max; rows.append(r)                                   # an overflowing normal: n.n = Inf
    r = good.copy(); r[3:6] = [T(np.sqrt(np.float64(fi.max)) * 2), 0, 0]; rows.append(r)
    return np.array(rows, dtype=T)


@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_invalid_points_give_six_zeros_and_leave_their_neighbours_alone(binding, prec):
    T = _T(prec)
    bad = _invalid_rows(T)
    good = _random_points(len(bad) + 1, 2).astype(T)
    mixed = np.empty((2 * len(bad) + 1, 6), dtype=T)
    mixed[0::2] = good
    mixed[1::2] = bad
    got = binding.gather_rays(mixed, 2, 11, 50, prec)
    assert np.array_equal(got, bake.hemisphere_rays(mixed, 2, 11, 50, prec))
    assert (got[1::2] == 0).all() and not np.signbit(got[1::2]).any()
    valid, _ = cameras.ray_prepare(got, prec)                                          # the radiance entry's own classification of the generated list
    assert valid[0::2].all() and not valid[1::2].any()
    # the neighbours: what the same points give at the same keys with every invalid point replaced by a valid one
    clean = mixed.copy()
    clean[1::2] = good[:-1]
    assert np.array_equal(binding.gather_rays(clean, 2, 11, 50, prec)[0::2], got[0::2])
    # a normal whose length is just above the smallest normal is valid
    edge = np.array([[0, 0, 0, 0, T(np.sqrt(np.float64(np.finfo(T).tiny)) * 1.001), 0]], dtype=T)
    assert cameras.ray_prepare(binding.gather_rays(edge, 0, 0, 0, prec), prec)[0].all()


@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_the_directions_are_cosine_weighted_about_the_normal(binding, prec):
    """2^16 samples at one point with a tilted normal.  Under the cosine density p(w) = cos / pi: E[cos] = 2/3, Var[cos] = 1/2 - 4/9 = 1/18, and a
    tangent component has mean 0 and variance 1/4; the bounds are 5 sigma / sqrt(N): 4.6e-3 and 9.8e-3."""
    T = _T(prec)
    N = 1 << 16
    n = np.array([0.3, -0.5, 0.81]) * 7.0
    pts = np.tile(np.concatenate([[1.0, -2.0, 0.5], n]), (N, 1))
    rays = binding.gather_rays(pts, 1, 42, 0, prec)                                   # point k draws under key k: N independent directions
    valid, d = cameras.ray_prepare(rays, prec)
    assert valid.all()
    _, nh = cameras.ray_prepare(pts[:1], prec)
    nh = nh[0].astype(np.float64)
    d = d.astype(np.float64)
    cos = d @ nh
    assert cos.min() >= -4 * np.finfo(T).eps
    assert abs(cos.mean() - 2.0 / 3.0) <= 5 * np.sqrt(1.0 / 18.0 / N)
    t1 = np.cross(nh, [1.0, 0.0, 0.0]); t1 /= np.linalg.norm(t1)
    t2 = np.cross(nh, t1)
    for t in (t1, t2, (t1 + t2) / np.sqrt(2.0)):
        assert abs((d @ t).mean()) <= 5 * np.sqrt(0.25 / N)
    # the same samples of ONE point (samples 0 .. 2^12 - 1 at one key) obey the same law
    M = 1 << 12
    one = np.stack([binding.gather_rays(pts[:1], s, 42, 5, prec)[0] for s in range(M)])
    _, d1 = cameras.ray_prepare(one, prec)
    assert abs((d1.astype(np.float64) @ nh).mean() - 2.0 / 3.0) <= 5 * np.sqrt(1.0 / 18.0 / M)


def test_return_codes_without_a_device(binding):
    """Every argument error that needs no handle is decided before any device is touched: its own code, never SPIRA_E_NO_DEVICE (-2)."""
    lib = binding.lib()
    buf = np.zeros(64, dtype=np.float64)
    p = buf.ctypes.data_as(C.c_void_p)
    u32, u64 = C.c_uint32, C.c_uint64
    err = lambda: lib.spira_last_error()
    R, V = binding.Radiance, binding.GatherVisible

    def rp(spp=1, depth=4, flags=0, sample0=0, seed=0, key0=0, reserved=0):
        return C.byref(R(spp, depth, flags, sample0, seed, key0, reserved))

    def gv(spp=8, sample0=0, seed=0, key0=0, flags=0, t_min=1e-3, t_max=float("inf")):
        return C.byref(V(spp, sample0, seed, key0, flags, t_min, t_max))
    for name in GATHER:
        fn = getattr(lib, name)
        tail = (None,) if "device" in name else ()
        call = lambda pts, n, r, sums: fn(None, pts, u32(n), r, sums, None, *tail)
        assert call(None, 4, rp(), p) == -1 and b"point array is NULL" in err(), name
        assert call(p, 4, None, p) == -1 and b"struct is NULL" in err(), name
        assert call(p, 4, rp(), None) == -1 and b"sum_rgb is NULL" in err(), name
        assert call(p, 0, rp(), p) == -1 and b"n_points is 0" in err(), name
        assert call(p, 4, rp(spp=0), p) == -1 and b"spp is 0" in err(), name
        assert call(p, 4, rp(depth=0), p) == -1 and call(p, 4, rp(depth=256), p) == -1 and b"max_depth" in err(), name
        assert call(p, 4, rp(reserved=1), p) == -1 and b"reserved" in err(), name
        for bad in (binding.KERNEL_MEGA, binding.SEM_CPU, binding.POST_NONE, binding.ROWS_BOTTOM_UP, 0x80000000):
            assert call(p, 4, rp(flags=bad), p) == -5, (name, bad)
        assert call(p, (1 << 26) + 1, rp(), p) == -4 and b"SPIRA_MAX_RAYS" in err(), name
        assert call(p, 4, rp(key0=0xFFFFFFFD), p) == -4 and b"key0" in err(), name
        assert call(p, 4, rp(spp=8, sample0=(1 << 24) - 7), p) == -4 and b"sample0" in err(), name
        # everything in order — 2^26 points x 2^24 samples included: the call gets as far as the handle
        for flags in (0, binding.EXT_DIELECTRIC, binding.EXT_SPECTRAL, binding.EXT_DIELECTRIC | binding.EXT_SPECTRAL):
            assert call(p, 4, rp(flags=flags, depth=255, key0=0xFFFFFFFC, spp=8, sample0=(1 << 24) - 8), p) == -1 and b"scene handle is NULL" in err(), name
        assert call(p, 1 << 26, rp(spp=1 << 24), p) == -1 and b"scene handle is NULL" in err(), name
    for name in VISIBLE:
        fn = getattr(lib, name)
        tail = (None,) if "device" in name else ()
        call = lambda pts, n, g, counts: fn(None, pts, u32(n), g, counts, None, *tail)
        assert call(None, 4, gv(), p) == -1 and b"point array is NULL" in err(), name
        assert call(p, 4, None, p) == -1 and b"struct is NULL" in err(), name
        assert call(p, 4, gv(), None) == -1 and b"visible_u32 is NULL" in err(), name
        assert call(p, 0, gv(), p) == -1 and b"n_points is 0" in err(), name
        assert call(p, 4, gv(spp=0), p) == -1 and b"spp is 0" in err(), name
        for t_min, t_max in ((float("nan"), 1.0), (0.0, float("nan")), (-1e-9, 1.0), (1.0, 0.5), (float("inf"), 1.0), (-float("inf"), 1.0)):
            assert call(p, 4, gv(t_min=t_min, t_max=t_max), p) == -1 and b"t_min" in err(), (name, t_min, t_max)
        for bad in (0x2, 0x3, binding.EXT_SPECTRAL, 0x80000000):
            assert call(p, 4, gv(flags=bad), p) == -1 and b"flag" in err(), (name, bad)
        assert call(p, (1 << 26) + 1, gv(), p) == -4 and b"SPIRA_MAX_RAYS" in err(), name
        assert call(p, 4, gv(key0=0xFFFFFFFD), p) == -4 and b"key0" in err(), name
        assert call(p, 4, gv(spp=8, sample0=(1 << 24) - 7), p) == -4 and b"sample0" in err(), name
        for flags, t_min, t_max in ((0, 1e-3, float("inf")), (binding.CAST_INPLACE, 0.0, 0.0), (0, 0.5, 0.5)):
            assert call(p, 4, gv(flags=flags, t_min=t_min, t_max=t_max, key0=0xFFFFFFFC, sample0=(1 << 24) - 8), p) == -1 and b"scene handle is NULL" in err(), name
        assert call(p, 1 << 26, gv(spp=1 << 24), p) == -1 and b"scene handle is NULL" in err(), name
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
        s.gather(np.zeros((4, 5)), 1, 4)
    with pytest.raises(ValueError):
        s.gather(np.zeros((4, 6)), 1, 4, sums=np.zeros((4, 3), dtype=np.float64))
    with pytest.raises(ValueError):
        s.gather_visible(np.zeros((4, 6)), 1, counts=np.zeros(4, dtype=np.int64))
    with pytest.raises(ValueError):
        binding.gather_rays(np.zeros((4, 8)))
    with pytest.raises(binding.SpiraError) as e:                                       # a NULL handle: the library's own refusal, no device touched
        s.gather(np.zeros((4, 6)), 1, 4)
    assert "error -1" in str(e.value)


def test_gather_plan_through_the_library(binding, monkeypatch):
    monkeypatch.delenv("SPIRA_GATHER_MAX_ITEMS", raising=False)
    monkeypatch.delenv("SPIRA_GATHER_WAVES_PER_CU", raising=False)
    pl = binding.gather_plan(1000, 8, 256)
    assert pl == {"grid": 32, "wpb": 4, "spp_pass": 8, "n_pass": 1, "direct": False, "ws_entries": 8000, "max_items": 1 << 26}
    assert binding.gather_plan(1 << 20, 1, 256)["direct"] and binding.gather_plan(1 << 20, 1, 256)["grid"] == 256 * 64 // 4
    # more than 2^32 items in a call: split into passes of at most 2^26 items, nothing overflowed
    big = binding.gather_plan(1 << 26, 1 << 24, 256)
    assert (big["spp_pass"], big["n_pass"], big["direct"], big["ws_entries"]) == (1, 1 << 24, True, 0)
    big = binding.gather_plan(1 << 20, 1 << 16, 256)
    assert (big["spp_pass"], big["n_pass"], big["direct"], big["ws_entries"]) == (64, 1024, False, 1 << 26)
    assert big["n_pass"] * big["ws_entries"] == (1 << 20) * (1 << 16) > 1 << 32
    # the gather's own knobs, read per call — not the radiance entries'
    monkeypatch.setenv("SPIRA_RADIANCE_MAX_ITEMS", "500")
    assert binding.gather_plan(1000, 8, 256)["n_pass"] == 1
    monkeypatch.setenv("SPIRA_GATHER_MAX_ITEMS", "3000")
    monkeypatch.setenv("SPIRA_GATHER_WAVES_PER_CU", "0")
    pl = binding.gather_plan(1000, 8, 256)
    assert (pl["grid"], pl["spp_pass"], pl["n_pass"], pl["ws_entries"], pl["max_items"]) == (1, 3, 3, 3000, 3000)
    monkeypatch.setenv("SPIRA_GATHER_MAX_ITEMS", "1000")
    pl = binding.gather_plan(1000, 8, 256)
    assert (pl["spp_pass"], pl["n_pass"], pl["direct"], pl["ws_entries"]) == (1, 8, True, 0)


def test_triangle_points_are_centroids_with_the_unit_geometric_normal():
    tri = np.array([[0, 0, 0, 2, 0, 0, 0, 3, 0, 1], [1, 1, 1, 1, 1, 2, 1, 2, 1, 1], [0, 0, 0, 1, 1, 1, 2, 2, 2, 1]], dtype=np.float64)
    pts = bake.triangle_points(tri)
    assert pts.shape == (3, 6) and pts.dtype == np.float64
    assert np.allclose(pts[0], [2 / 3, 1, 0, 0, 0, 1]) and np.allclose(pts[1], [1, 4 / 3, 4 / 3, -1, 0, 0])
    assert (pts[2, 3:6] == 0).all()                                                   # a degenerate triangle: an invalid point
    assert bake.triangle_points(tri, "f32").dtype == np.float32


@pytest.fixture(scope="module")
def gather_plan_exe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("gather") / "gather_plan")
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g", "-O1"]
    subprocess.run(["g++", "-std=c++17", "-ffp-contract=off", os.path.join(ROOT, "tests", "native", "gather_plan.cpp"), "-o", exe] + san, check=True)
    return exe


def _run(exe, text):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], input=text, capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-6000:]
    assert "plans checked" in r.stdout and "all checks passed" in r.stdout and "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr
    return r.stdout


@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_plan_and_generator_under_asan_ubsan(gather_plan_exe, prec):
    T = _T(prec)
    U = np.uint32 if prec == "f32" else np.uint64
    hexrow = lambda a: " ".join("%x" % int(w) for w in np.ascontiguousarray(a, dtype=T).view(U))
    pts = np.concatenate([_random_points(200, 3).astype(T), _invalid_rows(T)])
    sample, seed, key0 = 6, 0xABCDEF0123, 4000
    text = prec + "\n" + "".join("gen %x %x %x %s\n" % (sample, seed, key0 + k, hexrow(r)) for k, r in enumerate(pts))
    out = _run(gather_plan_exe, text)
    got = re.findall(r"^gen (\d)" + r" ([0-9a-f]+)" * 9 + "$", out, flags=re.M)
    assert len(got) == len(pts)
    want = bake.hemisphere_rays(pts, sample, seed, key0, prec)
    valid, d = cameras.ray_prepare(want, prec)
    verdicts = np.array([int(g[0]) for g in got], dtype=bool)
    assert np.array_equal(verdicts, valid) and valid[:200].all() and not valid[200:].any()
    bits = np.array([[int(x, 16) for x in g[1:]] for g in got], dtype=U)
    assert np.array_equal(bits[:, 0:6], want.view(U))
    assert np.array_equal(bits[valid, 6:9], np.ascontiguousarray(d[valid]).view(U))    # the direction the kernels trace along: radiance_ray_prepare's
