"""CPU: spira_scene_radiance_* and spira_camera_rays_* without a device — header, binding and library agree; the struct mirrors match field by field; the
header is hashed into the build id; the kernels sit in the translation unit of their precision; every argument error that needs no handle comes back as
documented, not as SPIRA_E_NO_DEVICE; and the launch plan, the ray preparation and the generator pass tests/native/radiance_plan.cpp under ASan + UBSan,
the last two bit for bit against the numpy restatements of spira_hip.cameras."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from spira_hip import cameras, scenes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RADIANCE = ["spira_scene_radiance_f32", "spira_scene_radiance_f64", "spira_scene_radiance_device_f32", "spira_scene_radiance_device_f64"]
CAMERA = ["spira_camera_rays_f32", "spira_camera_rays_f64", "spira_camera_rays_device_f32", "spira_camera_rays_device_f64"]


def test_library_header_and_binding_name_the_entries(binding):
    lib = binding.lib()
    hdr = open(os.path.join(ROOT, "include", "spira_hip.h")).read()
    for name in RADIANCE:
        assert hasattr(lib, name) and name in binding.EXPORTS and re.search(r"^int %s\(const spira_scene \*scene, " % name, hdr, flags=re.M), name
    for name in CAMERA:
        assert hasattr(lib, name) and name in binding.EXPORTS and re.search(r"^int %s\(const (float|double) camera12\[12\], const spira_lens \*lens, " % name, hdr, flags=re.M), name
    assert hasattr(lib, "spira_debug_radiance_plan") and "spira_debug_radiance_plan" not in hdr
    assert "#define SPIRA_ABI_VERSION 3 " in hdr and lib.spira_abi_version() == 3
    for const, val in (("SPIRA_CAM_PINHOLE", "0u"), ("SPIRA_CAM_THIN_LENS", "1u"), ("SPIRA_CAM_ORTHO", "2u")):
        assert re.search(r"^#define %s\s+%s" % (const, re.escape(val)), hdr, flags=re.M), const
    assert (binding.CAM_PINHOLE, binding.CAM_THIN_LENS, binding.CAM_ORTHO) == (0, 1, 2)
    for m in ("radiance", "radiance_device"):
        assert hasattr(binding.Scene, m), m
    assert hasattr(binding, "camera_rays") and hasattr(binding, "camera_rays_device")


def test_struct_mirrors_match_the_header_field_by_field(binding):
    from test_abi_cpu import _header_struct_fields
    ctype_of = {"uint32_t": C.c_uint32, "uint64_t": C.c_uint64, "double": C.c_double}
    for struct, mirror, size in (("spira_radiance", binding.Radiance, 32), ("spira_lens", binding.Lens, 40)):
        fields = _header_struct_fields(struct)
        assert [n for _, n in fields] == [n for n, _ in mirror._fields_], struct
        assert [ctype_of[t] for t, _ in fields] == [t for _, t in mirror._fields_], struct
        assert C.sizeof(mirror) == size == sum(C.sizeof(ctype_of[t]) for t, _ in fields), struct      # no padding either side
        assert ("%s;" % struct) in open(os.path.join(ROOT, "include", "spira_hip.h")).read()
    assert binding.Radiance.seed.offset == 16 and binding.Lens.seed.offset == 16 and binding.Lens.lens_radius.offset == 32


def test_the_header_is_hashed_into_the_build_id():
    mk = open(os.path.join(ROOT, "julia-spira_amd", "csrc", "Makefile")).read()
    assert "spira_radiance.h" in mk.split("DEPS", 1)[1].split("\n", 1)[0]
    src = open(os.path.join(ROOT, "julia-spira_amd", "csrc", "spira_hip.hip")).read()
    assert '#include "spira_radiance.h"' in src


def test_the_kernels_sit_in_the_unit_of_their_precision():
    csrc = os.path.join(ROOT, "julia-spira_amd", "csrc")
    objs = {n: os.path.join(csrc, "spira_tu_%s.o" % n) for n in ("main", "f32", "f64mesh")}
    if not all(os.path.exists(o) for o in objs.values()):
        pytest.skip("objects not present (library built elsewhere)")
    syms = {n: subprocess.run(["nm", o], capture_output=True, text=True, check=True).stdout for n, o in objs.items()}
    count = lambda text, pat: len(re.findall(pat, text))
    for kern in ("10k_radiance", "14k_radiance_sum", "13k_camera_rays"):
        assert count(syms["main"], kern + "If") == 0 and count(syms["main"], kern + "Id") > 0, kern
        assert count(syms["f32"], kern + "Id") == 0 and count(syms["f32"], kern + "If") > 0, kern
        assert count(syms["f64mesh"], kern + "I[fd]") == 0, kern
    # four instantiations of k_radiance per precision: BVH x EXT
    for unit, t in (("main", "d"), ("f32", "f")):
        assert len(set(re.findall(r"_ZN5spira10k_radianceI%sLb[01]ELb[01]EEEvNS_12RadianceArgsIT_EE" % t, syms[unit]))) == 4
    for fn in ("_ZN8spira_tu4ImplIfE8radianceE", "_ZN8spira_tu4ImplIfE11camera_raysE"):
        assert re.search(r" W %s" % fn, syms["f32"]) and re.search(r" U %s" % fn, syms["main"]), fn


def test_return_codes_without_a_device(binding):
    """Every argument error that needs no handle is decided before any device is touched: its own code, never SPIRA_E_NO_DEVICE (-2)."""
    lib = binding.lib()
    buf = np.zeros(64, dtype=np.float64)
    p = buf.ctypes.data_as(C.c_void_p)
    u32 = C.c_uint32
    R = binding.Radiance

    def rp(spp=1, depth=4, flags=0, sample0=0, seed=0, key0=0, reserved=0):
        return C.byref(R(spp, depth, flags, sample0, seed, key0, reserved))
    for name in RADIANCE:
        fn = getattr(lib, name)
        tail = (None,) if "device" in name else ()
        call = lambda rays, n, r, sums: fn(None, rays, u32(n), r, sums, None, *tail)
        err = lambda: lib.spira_last_error()
        assert call(None, 4, rp(), p) == -1 and b"ray array is NULL" in err(), name
        assert call(p, 4, None, p) == -1 and b"struct is NULL" in err(), name
        assert call(p, 4, rp(), None) == -1 and b"sum_rgb is NULL" in err(), name
        assert call(p, 0, rp(), p) == -1 and b"n_rays is 0" in err(), name
        assert call(p, 4, rp(spp=0), p) == -1 and b"spp is 0" in err(), name
        assert call(p, 4, rp(depth=0), p) == -1 and call(p, 4, rp(depth=256), p) == -1 and b"max_depth" in err(), name
        assert call(p, 4, rp(reserved=1), p) == -1 and b"reserved" in err(), name
        for bad in (binding.KERNEL_MEGA, binding.SEM_CPU, binding.POST_NONE, binding.ROWS_BOTTOM_UP, 0x80000000):
            assert call(p, 4, rp(flags=bad), p) == -5, (name, bad)
        assert call(p, (1 << 26) + 1, rp(), p) == -4 and b"SPIRA_MAX_RAYS" in err(), name
        assert call(p, 4, rp(key0=0xFFFFFFFD), p) == -4 and b"key0" in err(), name
        assert call(p, 4, rp(spp=8, sample0=(1 << 24) - 7), p) == -4 and b"sample0" in err(), name
        # everything in order: the call gets as far as the handle
        for flags in (0, binding.EXT_DIELECTRIC, binding.EXT_SPECTRAL, binding.EXT_DIELECTRIC | binding.EXT_SPECTRAL):
            assert call(p, 4, rp(flags=flags, depth=255, key0=0xFFFFFFFC, spp=8, sample0=(1 << 24) - 8), p) == -1 and b"scene handle is NULL" in err(), name
    cam = scenes.scene_s1()["camera12"]
    L = binding.Lens
    for name in CAMERA:
        fn = getattr(lib, name)
        T = np.float32 if name.endswith("f32") else np.float64
        c = np.ascontiguousarray(cam, dtype=T)
        cp = c.ctypes.data_as(C.c_void_p)
        tail = (None,) if "device" in name else ()
        call = lambda camp, lens, out: fn(camp, lens, out, *tail)
        ok = L(0, 33, 17, 0, 0, 0, 0, 0.0)
        assert call(None, C.byref(ok), p) == -1 and call(cp, None, p) == -1 and call(cp, C.byref(ok), None) == -1, name
        for bad in (L(3, 33, 17, 0, 0, 0, 0, 0.0), L(0, 1, 17, 0, 0, 0, 0, 0.0), L(0, 33, 1, 0, 0, 0, 0, 0.0), L(1, 33, 17, 0, 0, 0, 0, -0.5),
                    L(1, 33, 17, 0, 0, 0, 0, float("nan")), L(0, 33, 17, 0, 0, 7, 11, 0.0), L(0, 33, 17, 0, 0, 17, 1, 0.0)):
            assert call(cp, C.byref(bad), p) == -1, (name, bad.model, bad.width, bad.height, bad.row0, bad.rows, bad.lens_radius)
        for lim in (L(0, 65536, 65536, 0, 0, 0, 1, 0.0), L(0, 33, 17, 1 << 24, 0, 0, 0, 0.0), L(0, 16384, 8192, 0, 0, 0, 0, 0.0)):
            assert call(cp, C.byref(lim), p) == -4, name


def test_the_host_generator_needs_no_device(binding):
    cam = scenes.scene_s1()["camera12"]
    for prec in ("f32", "f64"):
        for model, radius in ((binding.CAM_PINHOLE, 0.0), (binding.CAM_THIN_LENS, 0.07), (binding.CAM_ORTHO, 0.0)):
            got = binding.camera_rays(cam, model, 33, 17, 2, 7, 3, 5, radius, prec)
            assert got.shape == (5 * 33, 6) and np.array_equal(got, cameras.generate_rays(cam, model, 33, 17, 2, 7, 3, 5, radius, prec))


def test_radiance_plan_through_the_library(binding, monkeypatch):
    pl = binding.radiance_plan(1000, 8, 256)
    assert pl == {"grid": 32, "wpb": 4, "spp_pass": 8, "n_pass": 1, "direct": False, "ws_entries": 8000, "max_items": 1 << 26}
    assert binding.radiance_plan(1920 * 1080, 1, 256)["direct"] and binding.radiance_plan(1920 * 1080, 1, 256)["grid"] == 256 * 64 // 4
    monkeypatch.setenv("SPIRA_RADIANCE_MAX_ITEMS", "3000")
    monkeypatch.setenv("SPIRA_RADIANCE_WAVES_PER_CU", "0")
    pl = binding.radiance_plan(1000, 8, 256)
    assert (pl["grid"], pl["spp_pass"], pl["n_pass"], pl["ws_entries"], pl["max_items"]) == (1, 3, 3, 3000, 3000)


@pytest.fixture(scope="module")
def radiance_plan_exe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("radiance") / "radiance_plan")
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g", "-O1"]
    subprocess.run(["g++", "-std=c++17", "-ffp-contract=off", os.path.join(ROOT, "tests", "native", "radiance_plan.cpp"), "-o", exe] + san, check=True)
    return exe


def _run(exe, text):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], input=text, capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-6000:]
    assert "plans checked" in r.stdout and "all checks passed" in r.stdout and "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr
    return r.stdout


def _ray_table(T):
    """Rays for radiance_ray_prepare: ordinary ones, each invalidity cause alone, and s around the smallest normal."""
    fi = np.finfo(T)
    good = np.array([0.25, 1.0, 3.0, 0.3, -0.4, -1.2], dtype=T)
    rows = [good, np.array([1, 2, 3, 0, 0, 5], dtype=T), np.array([-1e6, 0.5, 2e6, 1e-3, 2e-3, -3e-3], dtype=T), np.array([0, 0, 0, -0.0, 1, -0.0], dtype=T)]
    for k in range(6):
        for v in (np.nan, np.inf, -np.inf):
            r = good.copy(); r[k] = v; rows.append(r)
    r = good.copy(); r[3:6] = 0; rows.append(r)                                        # a zero direction
    r = good.copy(); r[3:6] = fi.max; rows.append(r)                                   # s overflows
    r = good.copy(); r[3:6] = fi.smallest_subnormal; rows.append(r)                    # s underflows to 0
    x = np.sqrt(np.float64(fi.tiny))
    for f in (1.0 + 1e-3, 1.0 - 1e-3, 2.0, 0.5):                                       # s = x x, one product: just above / below the smallest normal
        r = good.copy(); r[3:6] = [0, T(x * f), 0]; rows.append(r)
    return np.array(rows, dtype=T)


@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_plan_preparation_and_generator_under_asan_ubsan(radiance_plan_exe, prec):
    T = np.float32 if prec == "f32" else np.float64
    U = np.uint32 if prec == "f32" else np.uint64
    hexrow = lambda a: " ".join("%x" % int(w) for w in np.ascontiguousarray(a, dtype=T).view(U))
    rays = _ray_table(T)
    text = prec + "\n" + "".join("ray " + hexrow(r) + "\n" for r in rays)
    cam = np.ascontiguousarray(scenes.scene_s1()["camera12"], dtype=T)
    cases = []
    for model, radius in ((0, 0.0), (1, 0.07), (1, 0.0), (2, 0.0)):
        for row0, rows in ((0, 0), (0, 6), (6, 11)):
            cases.append((model, radius, row0, rows))
            text += "cam %x %x %x %x %x %x %x %s %s\n" % (model, 33, 17, 5, 0x1234567890, row0, rows, hexrow([radius]), hexrow(cam))
    out = _run(radiance_plan_exe, text)
    got = re.findall(r"^ray (\d) ([0-9a-f]+) ([0-9a-f]+) ([0-9a-f]+)$", out, flags=re.M)
    assert len(got) == len(rays)
    valid, d = cameras.ray_prepare(rays, prec)
    verdicts = np.array([int(g[0]) for g in got], dtype=bool)
    assert np.array_equal(verdicts, valid), np.flatnonzero(verdicts != valid)
    bits = np.array([[int(x, 16) for x in g[1:]] for g in got], dtype=U)
    assert np.array_equal(bits[valid], np.ascontiguousarray(d[valid]).view(U))
    assert valid[:4].all() and not valid[4:4 + 18 + 3].any() and list(valid[4 + 21:]) == [True, False, True, False]
    assert np.abs(np.linalg.norm(d[valid].astype(np.float64), axis=1) - 1).max() < 4 * np.finfo(T).eps
    gen = re.findall(r"^gen (\d+) ([0-9a-f]+) ([0-9a-f]+) ([0-9a-f]+) ([0-9a-f]+) ([0-9a-f]+) ([0-9a-f]+)$", out, flags=re.M)
    at = 0
    for model, radius, row0, rows in cases:
        n = (rows or 17) * 33
        blk = gen[at:at + n]
        assert [int(g[0]) for g in blk] == list(range(n))
        bits = np.array([[int(x, 16) for x in g[1:]] for g in blk], dtype=U)
        want = cameras.generate_rays(cam, model, 33, 17, 5, 0x1234567890, row0, rows, float(T(radius)), prec)
        assert np.array_equal(bits, want.view(U)), (model, radius, row0, rows)
        at += n
    assert at == len(gen)
