"""CPU: spira_scene_sweep_* without a device — the library exports the entries and the header and the binding name them; the functions the kernels call
(spira_sweep.h: sweep_prepare, sweep_sphere_triangle, sweep_sphere_sphere, sweep_normal) and sweep_check pass tests/native/sweep_plan.cpp under ASan +
UBSan bit for bit against the numpy twins of spira_hip.query; the exported host arithmetic equals the twin; with t_min = t_max = 0 the twin's start-overlap
verdict is the K-nearest candidate rule; the twin has the properties of a first contact whatever its formulas (an independent sample-and-bisect reference
in Float64); the argument errors that need no device come back as documented."""
import ctypes as C
import os
import re
import subprocess
import types

import numpy as np
import pytest

import cast_support as S
import nearest_support as N
import sweep_support as W
from spira_hip import query

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ["spira_scene_sweep_f32", "spira_scene_sweep_f64", "spira_scene_sweep_device_f32", "spira_scene_sweep_device_f64"]
BLOCKED = ["spira_scene_sweep_blocked_f32", "spira_scene_sweep_blocked_f64", "spira_scene_sweep_blocked_device_f32", "spira_scene_sweep_blocked_device_f64"]
HOST = ["spira_sweep_sphere_triangle_f32", "spira_sweep_sphere_triangle_f64"]


def test_library_header_and_binding_name_the_entries(binding):
    lib = binding.lib()
    hdr = open(os.path.join(ROOT, "include", "spira_hip.h")).read()
    for name in ENTRIES + BLOCKED:
        assert hasattr(lib, name) and name in binding.EXPORTS and re.search(r"^int %s\(const spira_scene \*scene, " % name, hdr, flags=re.M), name
    for name in HOST:
        assert hasattr(lib, name) and name in binding.EXPORTS and re.search(r"^void %s\(const " % name, hdr, flags=re.M), name
    assert "#define SPIRA_ABI_VERSION 3 " in hdr and lib.spira_abi_version() == 3
    for m in ("sweep", "sweep_device", "sweep_blocked", "sweep_blocked_device"):
        assert hasattr(binding.Scene, m), m
    for f in ("sweep_spheres", "sweep_sphere_triangle", "sweep_sphere_sphere", "prepare_sweeps", "sweep_segments"):
        assert hasattr(query, f), f
    mk = open(os.path.join(ROOT, "julia-spira_amd", "csrc", "Makefile")).read()
    assert "spira_sweep.h" in mk.split("DEPS", 1)[1].split("\n", 1)[0]      # hashed into spira_build_id


def test_kernels_live_in_the_unit_of_their_precision():
    csrc = os.path.join(ROOT, "julia-spira_amd", "csrc")
    objs = {n: os.path.join(csrc, "spira_tu_%s.o" % n) for n in ("main", "f32", "f64mesh")}
    if not all(os.path.exists(o) for o in objs.values()):
        pytest.skip("objects not present (library built elsewhere)")
    syms = {n: subprocess.run(["nm", o], capture_output=True, text=True, check=True).stdout for n, o in objs.items()}
    for kern in ("7k_sweep", "15k_sweep_session"):
        assert len(re.findall(kern + "If", syms["f32"])) > 0 and len(re.findall(kern + "Id", syms["f32"])) == 0, kern
        assert len(re.findall(kern + "Id", syms["main"])) > 0 and len(re.findall(kern + "If", syms["main"])) == 0, kern
        assert len(re.findall(kern + "I[fd]", syms["f64mesh"])) == 0, kern


# ------------------------------------------------------------------ the table
A_, B_, C_ = np.array([0.0, 0.0, 0.0]), np.array([2.0, 0.0, 0.0]), np.array([0.0, 1.0, 0.0])
# (origin, direction, r, t_min, t_max, the t geometry gives or None for a miss) against the triangle A B C: the face, each edge, each vertex, a face proposal
# outside the triangle falling through to an edge, start overlap, windows
_S5 = float(np.sqrt(5.0))
PLAIN = [
    ([0.5, 0.25, 3.0], [0, 0, -1], 0.5, 0.0, np.inf, 2.5),                               # the face
    ([0.5, 0.25, -3.0], [0, 0, 2], 0.25, 0.0, np.inf, 2.75),                             # the face from below, the direction not of unit length
    ([1.0, -3.0, 0.0], [0, 1, 0], 0.5, 0.0, np.inf, 2.5),                                # edge A B, in the plane
    ([-3.0, 0.5, 0.0], [1, 0, 0], 0.5, 0.0, np.inf, 2.5),                                # edge A C
    ([1.0 + 3 / _S5, 0.5 + 6 / _S5, 0.0], [-1, -2, 0], 0.5, 0.0, np.inf, 2.5),           # edge B C, along its normal at its midpoint
    ([-2.0, -2.0, 0.0], [1, 1, 0], 0.5, 0.0, np.inf, float(np.sqrt(8.0)) - 0.5),         # vertex A
    ([5.0, -1.0, 0.0], [-3, 1, 0], 0.5, 0.0, np.inf, float(np.sqrt(10.0)) - 0.5),        # vertex B
    ([-1.0, 4.0, 0.0], [1, -3, 0], 0.5, 0.0, np.inf, float(np.sqrt(10.0)) - 0.5),        # vertex C
    ([1.0, -0.3, 3.0], [0, 0, -1], 0.5, 0.0, np.inf, 3.0 - 0.4),                         # the face proposal lands outside: edge A B at height sqrt(0.25 - 0.09)
    ([0.5, 0.25, 0.3], [0, 0, 1], 0.5, 0.0, np.inf, 0.0),                                # start overlap
    ([0.5, 0.25, 0.3], [1, 0, 0], 0.5, 0.125, 4.0, 0.125),                               # start overlap at t_min > 0
    ([0.5, 0.25, 3.0], [0, 0, -1], 0.5, 0.0, 2.0, None),                                 # t_max before the contact
    ([0.5, 0.25, 3.0], [0, 0, -1], 0.5, 3.75, np.inf, None),                             # t_min past the first contact and past the overlap: the ball has gone through
    ([0.5, 0.25, 3.0], [0, 0, 1], 0.5, 0.0, np.inf, None),                               # moving away
    ([0.5, 0.25, 3.0], [0, 0, -1], 0.0, 0.0, np.inf, 3.0),                               # r = 0: the ray's own hit
    ([3.0, 3.0, 1.0], [1, 0, 0], 0.5, 0.0, np.inf, None),                                # parallel to the plane, beside the triangle
]


def _tri_rows(T):
    """(v0, v1, v2, o, d, r, t_min, t_max) rows in T with unit directions: PLAIN, PLAIN shifted, a needle, triangles of zero area, subnormal offsets, and a
    triangle so large that its products overflow (NaN: never a candidate)."""
    fi = np.finfo(T)
    rows = [(A_, B_, C_) + tuple(p[:5]) for p in PLAIN]
    shift = np.array([10.25, -3.5, 7.125])
    rows += [(a + shift, b + shift, c + shift, np.asarray(o) + shift, d, r, t0, t1) for a, b, c, o, d, r, t0, t1 in rows[:len(PLAIN)]]
    N1, N2, N3 = np.array([0.0, 0.0, 0.0]), np.array([1000.0, 0.0, 0.0]), np.array([500.0, 1e-4, 0.0])                            # a needle
    for o, d, r in (([500, 1, 3.0], [0, -0.3, -1], 0.25), ([-3, 0, 0], [1, 0, 0], 0.5), ([250, 2, 0], [0, -1, 0], 0.5), ([700, 0.05, -2], [0.1, 0, 1], 0.125)):
        rows.append((N1, N2, N3, o, d, r, 0.0, np.inf))
    for o, d in (([0.5, 0.5, 0.5], [0, -1, -1]), ([1, 3, 0], [0, -1, 0])):                                                       # zero area: a segment, a point
        rows.append((A_, B_, 0.5 * (A_ + B_), o, d, 0.5, 0.0, np.inf))
        rows.append((B_, B_, B_, o, d, 0.5, 0.0, np.inf))
    sub = float(fi.tiny) / 8                                                                                                     # subnormal offsets and radii
    rows.append((A_, B_, C_, [0.5, 0.25, sub], [0, 0, 1], 0.0, 0.0, np.inf))
    rows.append((A_, B_, C_, [0.5, 0.25, sub], [0, 0, -1], sub, 0.0, np.inf))
    rows.append((A_, B_, C_, [0.5, 0.25, 1.0], [0, 0, -1], sub, 0.0, np.inf))
    rows.append((A_, B_, C_, [sub, -sub, 0.5], [0, 0, -1], 0.25, 0.0, np.inf))
    big = float(np.sqrt(np.float64(fi.max))) * 4                                                                                # products overflow
    rows.append((A_, np.array([big, 0.0, 0.0]), np.array([0.0, big, 0.0]), [big / 4, big / 4, 1.0], [0, 0, -1], 0.5, 0.0, np.inf))
    out = []
    for a, b, c, o, d, r, t0, t1 in rows:
        ray, ok = query.normalize_rays(np.concatenate([o, [t0], d, [t1]])[None], T)
        assert ok[0]
        out.append(np.concatenate([np.asarray(a, dtype=T), np.asarray(b, dtype=T), np.asarray(c, dtype=T), ray[0, 0:3], ray[0, 4:7], [T(r), ray[0, 3], ray[0, 7]]]).astype(T))
    return np.array(out, dtype=T)


def _ray_sphere(o, d, c, radius):
    """The near root of |o + d t - c| = radius for the normalised d, in Float64."""
    o, d, c = (np.asarray(x, dtype=np.float64) for x in (o, d, c))
    d = d / np.linalg.norm(d)
    b = np.dot(o - c, d)
    return float(-b - np.sqrt(b * b - (np.dot(o - c, o - c) - radius * radius)))


# (centre, R, origin, direction, r, t_min, t_max, t or None): from outside, from the shell, from inside (the R - r root), a ball larger than the sphere
SPHERES = [
    ([0.5, -1.0, 2.0], 1.5, [0.5, -1.0, 7.0], [0, 0, -1], 0.5, 0.0, np.inf, 3.0),
    ([0.5, -1.0, 2.0], 1.5, [0.5, -1.0, 7.0], [0, 0, -1], 0.0, 0.0, np.inf, 3.5),
    ([0.5, -1.0, 2.0], 1.5, [0.5, -1.0, 3.5], [0, 1, 0], 0.25, 0.0, np.inf, 0.0),       # on the shell: overlap
    ([0.5, -1.0, 2.0], 1.5, [0.5, -1.0, 2.0], [0, 1, 0], 0.25, 0.0, np.inf, 1.25),      # from the centre: R - r
    ([0.5, -1.0, 2.0], 1.5, [0.5, -0.5, 2.0], [0, -1, 0], 0.5, 0.0, np.inf, 1.5),       # inside, through the centre to the far side
    ([0.5, -1.0, 2.0], 1.5, [0.5, -1.0, 2.0], [0, 1, 0], 2.0, 0.0, np.inf, 0.0),        # the ball holds the whole sphere: the shell is within r of its centre, overlap
    ([0.5, -1.0, 2.0], 1.5, [0.5, -1.0, 7.0], [0, 0, 1], 0.5, 0.0, np.inf, None),       # moving away
    ([0.5, -1.0, 2.0], 1.5, [0.5, -1.0, 7.0], [0, 0, -1], 0.5, 0.0, 2.5, None),         # t_max before the contact
    ([0.5, -1.0, 2.0], 1.5, [0.5, -1.0, 7.0], [0, 0, -1], 0.5, 4.5, np.inf, 6.0),       # t_min inside the shell: the far side from within (R - r)
    ([0.0, -100.5, -1.0], 100.0, [0.3, 2.0, -0.7], [0.1, -1, 0.05], 0.3, 0.0, np.inf, _ray_sphere([0.3, 2.0, -0.7], [0.1, -1, 0.05], [0.0, -100.5, -1.0], 100.3)),
    ([0.0, 0.0, 0.0], 0.0, [1.0, 2.0, 3.0], [-1, -2, -3], 0.5, 0.0, np.inf, float(np.sqrt(14.0)) - 0.5),      # a sphere of radius 0: a point
]


def _sph_rows(T):
    out = []
    for c, R, o, d, r, t0, t1, _ in SPHERES:
        ray, ok = query.normalize_rays(np.concatenate([o, [t0], d, [t1]])[None], T)
        assert ok[0]
        out.append(np.concatenate([np.asarray(c, dtype=T), [T(R)], ray[0, 0:3], ray[0, 4:7], [T(r), ray[0, 3], ray[0, 7]]]).astype(T))
    return np.array(out, dtype=T)


def _sweep_rows(T, frame):
    """Rays with radii: good ones, every invalid kind, and the radius bound (the last valid radius, the first invalid one) in a frame."""
    k_rays, k_rad = W.invalid_kinds(T, frame)
    c0 = np.zeros(3) if frame is None else np.asarray(frame[0], dtype=np.float64)
    u = 1.0 if frame is None else 1.0 / float(frame[1])
    good = np.concatenate([c0 + np.array([0.25, 1.0, 3.0]) * u, [0.0], [0.1, -0.4, -1.0], [np.inf]])
    rows, rad = [good, good, good], [0.0, -0.0, 0.5 * u]
    rows += list(k_rays); rad += list(k_rad)
    if frame is not None:
        r_in, r_out = W.radius_bound(types.SimpleNamespace(T=T, frame=frame))
        rows += [good, good]; rad += [float(r_in), float(r_out)]
    else:
        rows += [good]; rad += [float(np.finfo(T).max)]                # no tree: no radius rule (rs overflows to Inf: still no rule)
    return np.concatenate([np.array(rows), np.array(rad)[:, None]], axis=1).astype(T)


@pytest.fixture(scope="module")
def sweep_exe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("sweep") / "sweep_plan")
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g", "-O1"]
    subprocess.run(["g++", "-std=c++17", "-ffp-contract=off", os.path.join(ROOT, "tests", "native", "sweep_plan.cpp"), "-o", exe] + san, check=True)
    return exe


def _frames(prec):
    return [None, ((0.0, 0.0, 0.0), 1.0), ((0.5, -2.0, 8.0), 0.25)] + [S.mesh_frame(S.blob_scene(2, *f)["triangles10"], prec) for f in S.FRAMES]


def _twin_outputs(t, q, hit, o, d, T):
    """The harness's line from the twin's answer: hit, t, q, normal (0 for a miss)."""
    with np.errstate(all="ignore"):
        rv = (o + d * t[:, None]) - q
        l = np.sqrt(query._dot3(rv, rv))
        nrm = np.where((l >= np.finfo(T).tiny)[:, None], rv / l[:, None], -d)
    return np.concatenate([t[:, None], q, np.where(hit[:, None], nrm, T(0))], axis=1).astype(T)


def _same_bits(got, want, T, U):
    nan = np.isnan(want)
    return got.shape == want.shape and np.array_equal(np.isnan(got.view(T)), nan) and np.array_equal(got[~nan], np.ascontiguousarray(want).view(U)[~nan])


@pytest.mark.parametrize("prec", ["f32", "f64"])
@pytest.mark.parametrize("fi", range(7))
def test_the_kernels_functions_under_asan_ubsan_equal_the_twins(sweep_exe, prec, fi):
    T = S.dtype_of(prec)
    U = np.uint32 if prec == "f32" else np.uint64
    frame = _frames(prec)[fi]
    sw, tri, sph = _sweep_rows(T, frame), _tri_rows(T), _sph_rows(T)
    if fi > 0:
        tri, sph = tri[:4], sph[:2]              # the arithmetic does not depend on the frame: once in full is enough
    e = np.concatenate([tri[:, 0:3], tri[:, 3:6] - tri[:, 0:3], tri[:, 6:9] - tri[:, 0:3], tri[:, 9:]], axis=1)
    head = "%s %d %r %r %r %r\n" % ((prec, 1) + tuple(float(x) for x in frame[0]) + (float(frame[1]),)) if frame else "%s 0 0 0 0 1\n" % prec
    hexrow = lambda row: " ".join("%x" % int(w) for w in np.ascontiguousarray(row).view(U))
    body = "".join("P " + hexrow(r) + "\n" for r in sw) + "".join("T " + hexrow(r) + "\n" for r in e) + "".join("S " + hexrow(r) + "\n" for r in sph)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([sweep_exe], input=head + body, capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0 and "all checks passed" in r.stdout and "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stdout[-2000:] + r.stderr[-4000:]
    assert "%d lines answered" % (len(sw) + len(e) + len(sph)) in r.stdout
    # ---- validity
    verdicts = np.array([int(x) for x in re.findall(r"^sw (\d)$", r.stdout, flags=re.M)], dtype=bool)
    _, _, valid = query.prepare_sweeps(sw[:, :8], sw[:, 8], T, frame)
    assert np.array_equal(verdicts, valid), np.flatnonzero(verdicts != valid)
    n_inv = len(W.invalid_kinds(T, frame)[1])
    assert valid[:3].all() and not valid[3:3 + n_inv].any()                                      # every invalidity cause alone
    assert list(valid[3 + n_inv:]) == ([True, False] if frame is not None else [True])           # the last valid radius and the first invalid one
    # ---- the two sweep functions, bit for bit
    pat = r"^%s (\d) ([0-9a-f]+) ([0-9a-f]+) ([0-9a-f]+) ([0-9a-f]+) ([0-9a-f]+) ([0-9a-f]+) ([0-9a-f]+)$"
    rows = re.findall(pat % "tri", r.stdout, flags=re.M)
    g_hit, got = np.array([int(g[0]) for g in rows], dtype=bool), np.array([[int(x, 16) for x in g[1:]] for g in rows], dtype=U)
    t, q, hit = query.sweep_sphere_triangle(e[:, 0:3], e[:, 3:6], e[:, 6:9], e[:, 9:12], e[:, 12:15], e[:, 15], e[:, 16], e[:, 17])
    assert np.array_equal(g_hit, hit), np.flatnonzero(g_hit != hit)
    assert _same_bits(got, _twin_outputs(t, q, hit, e[:, 9:12], e[:, 12:15], T), T, U)
    rows = re.findall(pat % "sph", r.stdout, flags=re.M)
    g_hit, got = np.array([int(g[0]) for g in rows], dtype=bool), np.array([[int(x, 16) for x in g[1:]] for g in rows], dtype=U)
    ts, qs, hs = query.sweep_sphere_sphere(sph[:, 0:3], sph[:, 3], sph[:, 4:7], sph[:, 7:10], sph[:, 10], sph[:, 11], sph[:, 12])
    assert np.array_equal(g_hit, hs), np.flatnonzero(g_hit != hs)
    assert _same_bits(got, _twin_outputs(ts, qs, hs, sph[:, 4:7], sph[:, 7:10], T), T, U)
    if fi == 0:
        # what the table is for: every feature answers what geometry says
        tol = 64 * float(np.finfo(T).eps)
        n0 = len(PLAIN)
        for k in (0, n0):                                                                       # plain and shifted
            for i, p in enumerate(PLAIN):
                want = p[5]
                assert bool(hit[k + i]) == (want is not None), (k, i)
                if want is not None:
                    assert abs(float(t[k + i]) - want) <= tol * 16, (k, i, float(t[k + i]), want)
        assert np.abs(q[0].astype(np.float64) - [0.5, 0.25, 0.0]).max() <= tol and np.abs(q[2].astype(np.float64) - [1.0, 0.0, 0.0]).max() <= tol      # face, edge A B
        assert np.abs(q[8].astype(np.float64) - [1.0, 0.0, 0.0]).max() <= tol and np.abs(q[6].astype(np.float64) - B_).max() <= tol                    # fallen through to the edge; vertex B
        needle = slice(2 * n0, 2 * n0 + 4)
        assert hit[needle].all()
        zero = slice(2 * n0 + 4, 2 * n0 + 8)
        # zero area: where the closest-point function answers (vertex and edge regions) the triangle is the segment or the point it has collapsed to —
        # both sweeps meet the segment A B, neither comes within r of the point B; the overflowing triangle is NaN throughout: never a candidate
        assert list(hit[zero]) == [True, False, True, False] and not hit[-1]
        for i, s in enumerate(SPHERES):
            assert bool(hs[i]) == (s[7] is not None), i
            if s[7] is not None:
                assert abs(float(ts[i]) - s[7]) <= tol * 16, (i, float(ts[i]), s[7])


@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_the_exported_triangle_function_equals_the_twin(binding, prec):
    T = S.dtype_of(prec)
    U = np.uint32 if prec == "f32" else np.uint64
    tri = _tri_rows(T)
    rng = np.random.default_rng(43)
    n = 256
    v = rng.normal(size=(n, 9))
    o = v.reshape(n, 3, 3).mean(axis=1) + 3.0 * S._unit(rng, n)
    d = v.reshape(n, 3, 3).mean(axis=1) + 0.5 * rng.normal(size=(n, 3)) - o
    rays, ok = query.normalize_rays(np.concatenate([o, np.zeros((n, 1)), d, np.full((n, 1), np.inf)], axis=1), T)
    assert ok.all()
    rnd = np.concatenate([v.astype(T), rays[:, 0:3], rays[:, 4:7], rng.uniform(0.0, 0.6, (n, 1)).astype(T), rays[:, 3:4], rays[:, 7:8]], axis=1).astype(T)
    rows = np.concatenate([tri, rnd])
    v0, e1, e2 = rows[:, 0:3], rows[:, 3:6] - rows[:, 0:3], rows[:, 6:9] - rows[:, 0:3]
    t, q, hit = query.sweep_sphere_triangle(v0, e1, e2, rows[:, 9:12], rows[:, 12:15], rows[:, 15], rows[:, 16], rows[:, 17])
    assert 0.2 < hit[len(tri):].mean() < 0.98
    for i in range(len(rows)):
        gt, gq, gh = binding.sweep_sphere_triangle(v0[i], e1[i], e2[i], rows[i, 9:12], rows[i, 12:15], rows[i, 15], rows[i, 16], rows[i, 17], prec)
        assert gh == bool(hit[i]), i
        assert np.array([gt]).view(U)[0] == np.array([t[i]]).view(U)[0] and np.array_equal(gq.view(U), np.ascontiguousarray(q[i]).view(U)), i
    fn = getattr(binding.lib(), "spira_sweep_sphere_triangle_" + prec)
    ct = C.c_float if prec == "f32" else C.c_double
    a = [np.ascontiguousarray(x[0]).ctypes.data_as(C.c_void_p) for x in (v0, e1, e2, rows[:, 9:12], rows[:, 12:15])]
    fn(*a, ct(0.5), ct(0.0), ct(10.0), None, None, None)             # every output may be NULL


@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_start_overlap_is_the_k_nearest_candidate_rule(prec):
    """t_min = t_max = 0: object k is a candidate of the sweep exactly where d2_k <= r r — knearest_support's rule on NearScan.d2_all — bit for bit: the
    same function on the same values.  (A proposal could only add a candidate by being exactly 0 and verified within rs; none does here.)"""
    ss = W.scan_of("ico80", prec)
    T = ss.T
    rng = np.random.default_rng(44)
    n = 512
    sc = N.scene("ico80")
    ext = S.target_box(sc)[3]
    p = np.array(N.near_surface(rng, sc, n, frac=0.2)[:, :3], dtype=T)
    r = (rng.uniform(0.0, 0.3, n) * ext).astype(T)
    d = np.array(S._unit(rng, n), dtype=T)
    rays, ok = query.normalize_rays(np.concatenate([p, np.zeros((n, 1)), d, np.zeros((n, 1))], axis=1), T)
    assert ok.all()
    tk, qk, hit = ss.contacts(rays[:, 0:3], rays[:, 4:7], r, rays[:, 3], rays[:, 7])
    q, d2 = ss.d2_all(rays[:, 0:3])
    want = d2 <= (r * r)[:, None]
    assert np.array_equal(hit, want) and 0.02 < want.mean() < 0.9
    import knearest_support as K
    order = K.order_of(ss, np.concatenate([rays[:, 0:3], r[:, None]], axis=1).astype(np.float64))      # the yardstick's own candidates: r_max = r
    assert order["valid"].all() and np.array_equal(order["total"], hit.sum(axis=1).astype(np.uint32))
    few = np.flatnonzero(order["total"] <= K.TOP)
    assert len(few) > n // 2 and all(set(order["prim"][i][:order["total"][i]]) == set(np.flatnonzero(hit[i])) for i in few)
    assert np.array_equal(qk[want].view(np.uint32 if prec == "f32" else np.uint64), q[want].view(np.uint32 if prec == "f32" else np.uint64)) and not tk[want].any()


# ------------------------------------------------------------------ properties of the twin, whatever its formulas
def _first_contact_reference(ns, o, d, r, t_max, n_samples=512):
    """An independent first contact in Float64: f(t) = dist(c(t), scene) - r from the closest-point twins, sampled at n_samples + 1 points of [0, t_max];
    f is 1-Lipschitz in t (|d| = 1), so an interval of width h can hold f <= band only if f_i + f_(i+1) <= h + 2 band: those are searched for their
    minimum (golden section), the first point with f <= 0 is bracketed with the positive point before it and bisected to 1e-12.  Objects whose bounding
    sphere stays further than r + 3 h from the path cannot bring f below 2 h: left out.  Returns (t or None, min f over the path)."""
    h = t_max / n_samples
    band = 1e-3 * r
    cen = np.concatenate([ns.sp[:, 0:3], ns.v0 + (ns.e1 + ns.e2) / 3.0])
    rad = np.concatenate([ns.sp[:, 3], np.sqrt(np.maximum(np.maximum(((ns.e1 * 2 - ns.e2) ** 2).sum(1), ((ns.e2 * 2 - ns.e1) ** 2).sum(1)), ((ns.e1 + ns.e2) ** 2).sum(1))) / 3.0])
    s = np.clip(((cen - o) * d).sum(1), 0.0, t_max)
    gap = np.sqrt(((o + d * s[:, None] - cen) ** 2).sum(1))
    inside = np.arange(len(cen)) < ns.ns                             # (a sphere is a shell: the path may be inside it)
    near = inside | (gap - rad <= r + 3 * h)
    sph, tri = np.flatnonzero(near[:ns.ns]), np.flatnonzero(near[ns.ns:])

    def f(t):
        t = np.atleast_1d(np.asarray(t, dtype=np.float64))
        p = o + d * t[:, None]
        best = np.full(len(t), np.inf)
        if len(sph):
            best = np.minimum(best, query.closest_point_sphere(ns.sp[None, sph, 0:3], ns.sp[None, sph, 3], p[:, None, :])[1].min(axis=1))
        if len(tri):
            d2 = query.closest_point_triangle(ns.v0[None, tri], ns.e1[None, tri], ns.e2[None, tri], p[:, None, :])[1]
            best = np.minimum(best, np.where(np.isnan(d2), np.inf, d2).min(axis=1))
        return np.sqrt(best) - r
    ts = np.linspace(0.0, t_max, n_samples + 1)
    fs = f(ts)
    pts = [(ts[i], fs[i]) for i in range(len(ts))]
    g = (np.sqrt(5.0) - 1) / 2
    for i in np.flatnonzero((fs[:-1] > 0) & (fs[1:] > 0) & (fs[:-1] + fs[1:] <= h * 1.001 + 2 * band)):
        a, b = ts[i], ts[i + 1]
        x1, x2 = b - g * (b - a), a + g * (b - a)
        f1, f2 = f(x1)[0], f(x2)[0]
        for _ in range(48):
            if f1 < f2:
                b, x2, f2 = x2, x1, f1
                x1 = b - g * (b - a); f1 = f(x1)[0]
            else:
                a, x1, f1 = x1, x2, f2
                x2 = a + g * (b - a); f2 = f(x2)[0]
        pts.append((x1, f1) if f1 < f2 else (x2, f2))
    pts.sort()
    f_min = min(v for _, v in pts)
    k = next((k for k, (_, v) in enumerate(pts) if v <= 0), None)
    if k is None:
        return None, f_min
    if k == 0:
        return 0.0, f_min
    a, b = pts[k - 1][0], pts[k][0]
    while b - a > 1e-12:
        m = 0.5 * (a + b)
        if f(m)[0] <= 0:
            b = m
        else:
            a = m
    return b, f_min


@pytest.mark.parametrize("name", ["ico80", "s4_3"])
def test_the_twin_returns_the_first_contact(name):
    """Float64, 512 sweeps whose origins lie within 3 extents, r from 1 % to 30 % of the extent, directions toward random surface points with jitter.
    Sweeps whose minimum path distance lies within r (1 +- 1e-3) are left out — rounding decides those (and rs = r (1 + 2^-10) lies inside that band) — at
    most 5 % of the set.  For the rest the verdicts are equal and |t - t_ref| <= 1e-9 max(1, extent): outside the grazing band the approach rate is at
    least sqrt(2e-3), so Float64 rounding of about 100 operations gives about 1e-13; the factor 1e4 is margin."""
    sc = N.scene(name)
    ss = W.SweepScan(dict(sc, triangles10=np.asarray(sc["triangles10"], dtype=np.float64)), "f64", frame=False)
    ss.frame = None                                                  # the twin alone: no origin rule, no radius rule
    rng = np.random.default_rng(45)
    n = 512
    _, _, c, ext = S.target_box(sc)
    o = c + ext * rng.uniform(0.6, 3.0, (n, 1)) * S._unit(rng, n)
    target = N.surface_points(rng, sc, n) + 0.3 * ext * rng.normal(size=(n, 3)) * (rng.random((n, 1)) < 0.6)
    to = target - o
    length = np.linalg.norm(to, axis=1)
    t_max = length + ext
    r = rng.uniform(0.01, 0.30, n) * ext
    rays, ok = query.normalize_rays(np.concatenate([o, np.zeros((n, 1)), to, t_max[:, None]], axis=1), np.float64)
    assert ok.all()
    prim, t, point, normal, valid = ss.sweep(rays, r)
    assert valid.all()
    left_out, hits, worst = 0, 0, 0.0
    for i in range(n):
        t_ref, f_min = _first_contact_reference(ss, rays[i, 0:3], rays[i, 4:7], r[i], t_max[i])
        if abs(f_min) <= 1e-3 * r[i]:
            left_out += 1
            continue
        assert (prim[i] >= 0) == (t_ref is not None), (i, prim[i], t_ref, f_min, r[i])
        if t_ref is not None:
            hits += 1
            worst = max(worst, abs(float(t[i]) - t_ref))
            assert abs(float(t[i]) - t_ref) <= 1e-9 * max(1.0, ext), (i, float(t[i]), t_ref, r[i])
            # the outputs are those of a contact: the point is on the winner, at rs at the most from the centre, and the normal is of unit length
            cdist = np.linalg.norm(rays[i, 0:3] + rays[i, 4:7] * t[i] - point[i])
            assert cdist <= r[i] * (1 + 2.0 ** -10) * (1 + 1e-12) and abs(np.linalg.norm(normal[i]) - 1) <= 1e-12, i
    print(name, "left out %d of %d, hits %d, worst |t - t_ref| %.3g" % (left_out, n, hits, worst))
    assert left_out <= 0.05 * n and hits >= n // 4 and n - hits - left_out >= n // 16


def test_return_codes_without_a_device(binding):
    """Every argument error of the entries is decided before any device is touched: it returns its own code, not SPIRA_E_NO_DEVICE (-2)."""
    lib = binding.lib()
    rays, rad = np.zeros((4, 8), dtype=np.float64), np.zeros(4, dtype=np.float64)
    rp, dp, out = rays.ctypes.data_as(C.c_void_p), rad.ctypes.data_as(C.c_void_p), np.zeros(64, dtype=np.float64).ctypes.data_as(C.c_void_p)
    u32 = C.c_uint32
    for name in ENTRIES + BLOCKED:
        fn = getattr(lib, name)
        tail = (None,) if "device" in name else ()
        blocked = "blocked" in name

        def call(scene, r, d, n, flags, outs):
            return fn(scene, r, d, u32(n), u32(flags), *(outs + tail))
        outs = (out,) if blocked else (out, out, out, out, None)
        none = (None,) if blocked else (None, None, None, None, out)      # trips alone is no output
        assert call(None, None, dp, 4, 0, outs) == -1 and b"ray array is NULL" in lib.spira_last_error(), name
        assert call(None, rp, None, 4, 0, outs) == -1 and b"radius array is NULL" in lib.spira_last_error(), name
        assert call(None, rp, dp, 0, 0, outs) == -1 and b"n is 0" in lib.spira_last_error(), name
        assert call(None, rp, dp, 4, 2, outs) == -1 and b"unknown flag bits" in lib.spira_last_error(), name
        assert call(None, rp, dp, 4, 0x80000001, outs) == -1, name
        assert call(None, rp, dp, 4, 0, none) == -1 and b"every output is NULL" in lib.spira_last_error(), name
        assert call(None, rp, dp, (1 << 26) + 1, 0, outs) == -4 and b"SPIRA_MAX_RAYS" in lib.spira_last_error(), name
        assert call(None, rp, dp, 4, 0, outs) == -1 and b"scene handle is NULL or was destroyed" in lib.spira_last_error(), name
        assert call(None, rp, dp, 4, 1, outs) == -1 and b"scene handle is NULL" in lib.spira_last_error(), name


def test_the_sweep_sets_reach_what_they_are_for():
    """Asserted from the scan's answers alone, on the small scenes (the sets the GPU tests run): every part does what it is there for."""
    for prec in ("f32", "f64"):
        for name in ("ico33", "ico80"):
            r, ss = W.reference(name, prec), W.scan_of(name, prec)
            prim, t, parts = r["prim"], r["t"], r["parts"]
            assert 1800 <= len(prim) <= 2600, len(prim)
            assert (prim[parts["head"]] >= ss.ns).mean() > 0.6                             # (origins below the ground meet the ground sphere)
            g = prim[parts["graze"]]
            assert (g >= 0).mean() > 0.2 and (g == W.MISS).mean() > 0.1
            over = parts["over"]
            assert (prim[over] >= 0).all() and not t[over].any()                                 # start overlap: t = t_min = 0
            tk, _, hit = ss.contacts(*[np.asarray(x, dtype=ss.T) for x in (r["rays"][over][:64, 0:3], query.normalize_rays(r["rays"][over][:64], ss.T)[0][:, 4:7],
                                                                           r["radii"][over][:64], r["rays"][over][:64, 3], r["rays"][over][:64, 7])])
            several = (hit & (tk == 0)).sum(axis=1)
            assert (several >= 2).mean() > 0.5                                                    # ... with several objects: ties
            last = hit.shape[1] - 1 - np.argmax((hit & (tk == 0))[:, ::-1], axis=1)
            assert np.array_equal(prim[over][:64], last)                                          # ... that go to the later index
            assert (prim[parts["same"]] == prim[r["sel"]]).all() and np.array_equal(t[parts["same"]], t[r["sel"]])
            assert (prim[parts["below"]] != prim[r["sel"]]).mean() > 0.9 and (t[parts["below"]] <= r["rays"][parts["below"], 7].astype(ss.T)).all()
            assert ((prim[parts["beyond"]] == W.MISS) | (t[parts["beyond"]] > t[r["sel"]]) | (t[parts["beyond"]] == r["rays"][parts["beyond"], 3].astype(ss.T))).all()
            assert (prim[parts["zero_on"]] >= ss.ns).any()
            assert (prim[parts["axis"]] >= 0).mean() > 0.3
            assert (prim[parts["inside"]] >= 0).mean() > 0.9 and (t[parts["inside"]] > 0).mean() > 0.5       # the R - r root
            far = prim[parts["far"]]
            assert (far[0::2] != W.INVALID).all() and (far[0::2] >= 0).mean() > 0.5 and (far[1::2] == W.INVALID).all()
            b = prim[parts["bound"]]
            assert (b[0::2] != W.INVALID).all() and (b[1::2] == W.INVALID).all()
            assert (prim[parts["big"]] >= 0).mean() > 0.5
            assert (prim[parts["corner"]] != W.INVALID).mean() > 0.9 and (prim[parts["corner"]] >= 0).mean() > 0.5
            assert (prim[r["invalid_at"]] == W.INVALID).all() and (prim[r["invalid_at"][:-1] + 1] != W.INVALID).all()
            assert len(r["invalid_at"]) >= len(W.invalid_kinds(ss.T, ss.frame)[1])
            assert not t[prim == W.INVALID].any() and not r["point"][prim < 0].any() and not r["normal"][prim < 0].any()
