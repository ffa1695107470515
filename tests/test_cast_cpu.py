"""CPU: spira_scene_cast_* / spira_scene_occluded_* without a device — the library exports the eight symbols and the header and the binding name them; the
launch plan (spira_plan.h, make_cast_plan) and the ray preparation the kernels call (spira_query.h, cast_ray_prepare) pass tests/native/cast_plan.cpp
under ASan + UBSan, the latter bit for bit against spira_hip.query.normalize_rays; the argument errors that need no device come back as documented; the
kernels sit in the translation unit of their precision; and normalize_rays fed to the oracle's hit functions reproduces hand-checked answers."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import cast_support as S
from spira_hip import query

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["spira_scene_cast_f32", "spira_scene_cast_f64", "spira_scene_cast_device_f32", "spira_scene_cast_device_f64",
       "spira_scene_occluded_f32", "spira_scene_occluded_f64", "spira_scene_occluded_device_f32", "spira_scene_occluded_device_f64"]


def test_library_header_and_binding_name_the_query_entries(binding):
    lib = binding.lib()
    hdr = open(os.path.join(ROOT, "include", "spira_hip.h")).read()
    for name in NEW:
        assert hasattr(lib, name) and name in binding.EXPORTS and re.search(r"^int %s\(const spira_scene \*scene, " % name, hdr, flags=re.M), name
    assert "#define SPIRA_ABI_VERSION 3 " in hdr and lib.spira_abi_version() == 3
    for const, val in (("SPIRA_MAX_RAYS", "(1u << 26)"), ("SPIRA_RAY_MISS", "-1"), ("SPIRA_RAY_INVALID", "-3"), ("SPIRA_CAST_INPLACE", "0x1u")):
        assert re.search(r"^#define %s\s+%s" % (const, re.escape(val)), hdr, flags=re.M), const
    assert (binding.MAX_RAYS, binding.RAY_MISS, binding.RAY_INVALID, binding.CAST_INPLACE) == (1 << 26, -1, -3, 1)
    for m in ("cast", "occluded", "cast_device", "occluded_device"):
        assert hasattr(binding.Scene, m), m
    mk = open(os.path.join(ROOT, "julia-spira_amd", "csrc", "Makefile")).read()
    assert "spira_query.h" in mk.split("DEPS", 1)[1].split("\n", 1)[0]      # hashed into spira_build_id


def _table(T, frame):
    """Rays for cast_ray_prepare: ordinary ones, each invalidity cause alone, and the edges of the rules."""
    fi = np.finfo(T)
    good = np.array([0.25, 1.0, 3.0, 0.001, 0.3, -0.4, -1.2, np.inf], dtype=T)
    rows = [good, np.array([1, 2, 3, 0, 0, 0, 5, 7], dtype=T), np.array([-1, 0.5, 2, 0.5, 1e-3, 2e-3, -3e-3, 0.5], dtype=T)]      # (the last: t_min == t_max)
    rows += [r.astype(T) for r in S.invalid_kinds(T, frame)]
    # s just above and just below the smallest normal: one component of sqrt(tiny) scaled up / down a little (s = x x exactly one product)
    x = np.sqrt(np.float64(fi.tiny))
    for f in (1.0 + 1e-3, 1.0 - 1e-3, 2.0, 0.5):
        r = good.copy(); r[4:7] = [0, T(x * f), 0]; rows.append(r)
    r = good.copy(); r[7] = r[3]; rows.append(r)                                  # t_min == t_max
    r = good.copy(); r[7] = np.nextafter(r[3], T(0)); rows.append(r)              # t_max one ulp under t_min
    r = good.copy(); r[3] = 0; rows.append(r)
    r = good.copy(); r[3] = -0.0; rows.append(r)                                  # -0 is not < 0
    r = good.copy(); r[3] = np.inf; rows.append(r)                                # t_min = t_max = +Inf: nothing can be hit, but nothing is malformed
    if frame is not None:
        c, scale = np.asarray(frame[0], dtype=T), T(frame[1])
        for k in range(3):
            for sign in ((1, -1) if c[k] == 0 else (int(np.sign(c[k])),)):        # (away from 0: o - c is then exact for o one ulp off the bound)
                on = T(c[k] + T(sign * 64) / scale)                                # exactly on the bound (a power-of-two scale: exact)
                r = good.copy(); r[k] = on; rows.append(r)
                r = good.copy(); r[k] = np.nextafter(on, T(sign * np.inf)); rows.append(r)      # one ulp outside
                r = good.copy(); r[k] = np.nextafter(on, T(0) if c[k] == 0 else c[k]); rows.append(r)
    return np.array(rows, dtype=T)


@pytest.fixture(scope="module")
def cast_plan_exe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("cast") / "cast_plan")
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g", "-O1"]
    subprocess.run(["g++", "-std=c++17", "-ffp-contract=off", os.path.join(ROOT, "tests", "native", "cast_plan.cpp"), "-o", exe] + san, check=True)
    return exe


def _run(exe, text):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], input=text, capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-6000:]
    assert "plans checked" in r.stdout and "all checks passed" in r.stdout and "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr
    return r.stdout


@pytest.mark.parametrize("prec", ["f32", "f64"])
@pytest.mark.parametrize("frame", [None, ((0.0, 0.0, 0.0), 1.0), ((0.5, -2.0, 8.0), 0.25)])
def test_plan_and_ray_preparation_under_asan_ubsan(cast_plan_exe, prec, frame):
    T = S.dtype_of(prec)
    U = np.uint32 if prec == "f32" else np.uint64
    rays = _table(T, frame)
    head = "%s %d %r %r %r %r\n" % ((prec, 1) + tuple(float(x) for x in frame[0]) + (float(frame[1]),)) if frame else "%s 0 0 0 0 1\n" % prec
    body = "".join(" ".join("%x" % int(w) for w in row.view(U)) + "\n" for row in rays)
    out = _run(cast_plan_exe, head + body)
    got = re.findall(r"^ray (\d) ([0-9a-f]+) ([0-9a-f]+) ([0-9a-f]+)$", out, flags=re.M)
    assert len(got) == len(rays)
    want, valid = query.normalize_rays(rays, T, frame)
    verdicts = np.array([int(g[0]) for g in got], dtype=bool)
    assert np.array_equal(verdicts, valid), np.flatnonzero(verdicts != valid)
    bits = np.array([[int(x, 16) for x in g[1:]] for g in got], dtype=U)
    assert np.array_equal(bits[valid], np.ascontiguousarray(want[valid, 4:7]).view(U))
    # the verdicts are the contract's, cause by cause
    n_inv = len(S.invalid_kinds(T, frame))
    assert valid[:3].all() and not valid[3:3 + n_inv].any()
    k = 3 + n_inv
    assert list(valid[k:k + 4]) == [True, False, True, False]                      # s around the smallest normal
    assert list(valid[k + 4:k + 9]) == [True, False, True, True, True]
    if frame is not None:
        assert len(valid) - (k + 9) in (9, 18) and list(valid[k + 9:]) == [True, False, True] * ((len(valid) - k - 9) // 3)      # on the bound, one ulp outside, one inside
    # unit length to rounding, and the direction kept
    d = want[valid, 4:7].astype(np.float64)
    assert np.abs(np.linalg.norm(d, axis=1) - 1).max() < 4 * np.finfo(T).eps


def test_return_codes_without_a_device(binding):
    """Every argument error of the query entries is decided before any device is touched: it returns its own code, not SPIRA_E_NO_DEVICE (-2)."""
    lib = binding.lib()
    rays = np.zeros((4, 8), dtype=np.float64)
    rp, out = rays.ctypes.data_as(C.c_void_p), np.zeros(64, dtype=np.float64).ctypes.data_as(C.c_void_p)
    u32 = C.c_uint32
    for name in NEW:
        fn = getattr(lib, name)
        occ, dev = "occluded" in name, "device" in name
        tail = (None,) if dev else ()

        def call(scene, r, n, flags, outs):
            return fn(scene, r, u32(n), u32(flags), *(outs + tail))
        outs = (out,) if occ else (out, out, out)
        none = (None,) if occ else (None, None, None)
        assert call(None, None, 4, 0, outs) == -1 and b"ray array is NULL" in lib.spira_last_error(), name
        assert call(None, rp, 0, 0, outs) == -1 and b"n_rays is 0" in lib.spira_last_error(), name
        assert call(None, rp, 4, 2, outs) == -1 and b"unknown flag bits" in lib.spira_last_error(), name
        assert call(None, rp, 4, 0x80000001, outs) == -1, name
        assert call(None, rp, 4, 0, none) == -1 and b"every output is NULL" in lib.spira_last_error(), name
        assert call(None, rp, (1 << 26) + 1, 0, outs) == -4 and b"SPIRA_MAX_RAYS" in lib.spira_last_error(), name
        assert call(None, rp, 4, 0, outs) == -1 and b"scene handle is NULL or was destroyed" in lib.spira_last_error(), name
        assert call(None, rp, 4, 1, outs) == -1 and b"scene handle is NULL" in lib.spira_last_error(), name
        if not occ:      # out_prim and out_t may each be NULL: with the normal alone the call gets as far as the handle
            assert call(None, rp, 4, 0, (None, None, out)) == -1 and b"scene handle is NULL" in lib.spira_last_error(), name


def test_cast_plan_helper(binding):
    p = binding.cast_plan(20011, 256)
    assert p["waves"] == p["grid"] * p["wpb"] and p["base"] * p["waves"] + p["rem"] == 20011 and p["base"] > 64 and p["refill_free"] == 16
    p = binding.cast_plan(1 << 26, 256)
    assert p["waves"] == 256 * 20 and p["base"] * p["waves"] + p["rem"] == 1 << 26
    with pytest.raises(binding.SpiraError):
        binding.cast_plan(0, 256)


def test_query_kernels_live_in_the_unit_of_their_precision():
    csrc = os.path.join(ROOT, "julia-spira_amd", "csrc")
    objs = {n: os.path.join(csrc, "spira_tu_%s.o" % n) for n in ("main", "f32", "f64mesh")}
    if not all(os.path.exists(o) for o in objs.values()):
        pytest.skip("objects not present (library built elsewhere)")
    syms = {n: subprocess.run(["nm", o], capture_output=True, text=True, check=True).stdout for n, o in objs.items()}
    for kern in ("6k_cast", "14k_cast_session"):
        assert len(re.findall(kern + "If", syms["f32"])) > 0 and len(re.findall(kern + "Id", syms["f32"])) == 0, kern
        assert len(re.findall(kern + "Id", syms["main"])) > 0 and len(re.findall(kern + "If", syms["main"])) == 0, kern
        assert len(re.findall(kern + "I[fd]", syms["f64mesh"])) == 0, kern
    assert re.search(r" W _ZN8spira_tu4ImplIfE4castE", syms["f32"]) and re.search(r" U _ZN8spira_tu4ImplIfE4castE", syms["main"])


@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_normalize_rays_against_the_oracle_on_known_answers(oracle, prec):
    T = S.dtype_of(prec)
    eps = float(np.finfo(T).eps)
    # an axis ray at a unit sphere hits at t = |o| - 1, whatever the length of the direction given
    sph = dict(spheres5=np.array([[0.0, 0.0, 0.0, 1.0, 1.0]]), triangles10=None)
    rays = np.array([[0, 0, 5, 0.001, 0, 0, -7.5, np.inf], [-3, 0, 0, 0, 0.125, 0, 0, np.inf], [0, 4, 0, 0, 0, -2, 0, 2.5], [0, 4, 0, 0, 0, -2, 0, 3.0],
                     [0, 0, 5, 4.5, 0, 0, -1, np.inf], [0, 0, 5, 0, 0, 0, 1, np.inf]])
    prim, t, valid, prepared = S.Scan(oracle, sph, prec).cast(rays)
    assert valid.all() and np.array_equal(prepared[:, 4:7], np.array([[0, 0, -1], [1, 0, 0], [0, -1, 0], [0, -1, 0], [0, 0, -1], [0, 0, 1]], dtype=T))
    assert list(prim) == [0, 0, -1, 0, 0, -1]                   # (ray 2: the hit at 3 lies beyond t_max 2.5; ray 4: t_min 4.5 skips the near root, the far one is 6)
    assert np.allclose(t[[0, 1, 3, 4]], [4, 2, 3, 6], rtol=8 * eps, atol=0) and t[2] == T(2.5) and t[5] == T(np.inf)
    # a triangle is hit at its centroid, from a skew direction of length 3.7; beside it the ray misses
    tri = np.array([[1.0, 0.0, -2.0, 0.0, 2.0, -2.5, -1.0, 0.5, -3.0, 1.0]])
    cen = tri[0, :9].reshape(3, 3).mean(axis=0)
    o = np.array([0.3, 0.4, 3.0])
    dist = float(np.linalg.norm(cen - o))
    rays = np.array([list(o) + [0.001] + list(3.7 * (cen - o) / dist) + [np.inf], list(o) + [0.001] + list(cen + [5, 0, 0] - o) + [np.inf],
                     list(o) + [0.001] + list(cen - o) + [dist * 0.999]])
    sc = S.Scan(oracle, dict(spheres5=np.zeros((0, 5)), triangles10=tri), prec)
    prim, t, valid, prepared = sc.cast(rays)
    assert valid.all() and list(prim) == [0, -1, -1] and abs(float(t[0]) - dist) <= 16 * eps * dist and t[2] == T(dist * 0.999)
    n = sc.normals(prepared, prim, t, T)
    e1, e2 = tri[0, 3:6] - tri[0, 0:3], tri[0, 6:9] - tri[0, 0:3]
    want = np.cross(e1, e2) / np.linalg.norm(np.cross(e1, e2))
    assert np.abs(n[0] - want).max() <= 8 * eps and not n[1:].any()
    # an invalid ray answers -3 and 0 and is left alone
    bad = rays.copy(); bad[0, 4:7] = 0
    prim, t, valid, _ = sc.cast(bad)
    assert list(valid) == [False, True, True] and prim[0] == -3 and t[0] == 0
