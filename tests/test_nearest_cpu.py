"""CPU: spira_scene_closest_point_* without a device — the library exports the entries and the header and the binding name them; the functions the
kernels call (spira_nearest.h: nearest_point_prepare, closest_point_triangle, closest_point_sphere) pass tests/native/nearest_plan.cpp under ASan + UBSan
bit for bit against the numpy twins of spira_hip.query; the twin has the properties of a closest point whatever its formulas; the exported host
arithmetic equals the twin; the argument errors that need no device come back as documented."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import cast_support as S
import nearest_support as N
from spira_hip import query

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ["spira_scene_closest_point_f32", "spira_scene_closest_point_f64", "spira_scene_closest_point_device_f32", "spira_scene_closest_point_device_f64"]
HOST = ["spira_closest_point_triangle_f32", "spira_closest_point_triangle_f64"]


def test_library_header_and_binding_name_the_entries(binding):
    lib = binding.lib()
    hdr = open(os.path.join(ROOT, "include", "spira_hip.h")).read()
    for name in ENTRIES:
        assert hasattr(lib, name) and name in binding.EXPORTS and re.search(r"^int %s\(const spira_scene \*scene, " % name, hdr, flags=re.M), name
    for name in HOST:
        assert hasattr(lib, name) and name in binding.EXPORTS and re.search(r"^void %s\(const " % name, hdr, flags=re.M), name
    assert "#define SPIRA_ABI_VERSION 3 " in hdr and lib.spira_abi_version() == 3
    for m in ("closest_point", "closest_point_device"):
        assert hasattr(binding.Scene, m), m
    mk = open(os.path.join(ROOT, "julia-spira_amd", "csrc", "Makefile")).read()
    assert "spira_nearest.h" in mk.split("DEPS", 1)[1].split("\n", 1)[0]      # hashed into spira_build_id


def test_kernels_live_in_the_unit_of_their_precision():
    csrc = os.path.join(ROOT, "julia-spira_amd", "csrc")
    objs = {n: os.path.join(csrc, "spira_tu_%s.o" % n) for n in ("main", "f32", "f64mesh")}
    if not all(os.path.exists(o) for o in objs.values()):
        pytest.skip("objects not present (library built elsewhere)")
    syms = {n: subprocess.run(["nm", o], capture_output=True, text=True, check=True).stdout for n, o in objs.items()}
    for kern in ("9k_nearest", "17k_nearest_session"):
        assert len(re.findall(kern + "If", syms["f32"])) > 0 and len(re.findall(kern + "Id", syms["f32"])) == 0, kern
        assert len(re.findall(kern + "Id", syms["main"])) > 0 and len(re.findall(kern + "If", syms["main"])) == 0, kern
        assert len(re.findall(kern + "I[fd]", syms["f64mesh"])) == 0, kern


# ------------------------------------------------------------------ the table
def _tri_rows(T):
    """(v0, v1, v2, p) rows in T: all seven regions of a plain triangle from above its plane, points exactly on vertices, edges and the face, a point in
    the plane outside the triangle, a needle, triangles of zero area, subnormal offsets, and a triangle so large that its products overflow (the answer is NaN)."""
    fi = np.finfo(T)
    A, B, Cc = np.array([0.0, 0.0, 0.0]), np.array([2.0, 0.0, 0.0]), np.array([0.0, 1.0, 0.0])
    rows = []
    for p in ([-1, -1, 0.5], [3, -0.5, 0.5], [1, -1, 0.5], [-0.5, 2.5, 0.5], [-1, 0.5, 0.5], [2, 1.5, 0.5], [0.5, 0.25, 0.5]):      # regions 1 .. 7
        rows.append((A, B, Cc, np.array(p, dtype=np.float64)))
    for p in (A, B, Cc, 0.5 * (A + B), 0.5 * (A + Cc), 0.5 * (B + Cc), A + 0.25 * (B - A) + 0.25 * (Cc - A), [3.0, 3.0, 0.0], [-2.0, 0.3, 0.0]):
        rows.append((A, B, Cc, np.array(p, dtype=np.float64)))
    shift = np.array([10.25, -3.5, 7.125])
    rows += [(a + shift, b + shift, c + shift, p + shift) for a, b, c, p in rows[:16]]
    N1, N2, N3 = np.array([0.0, 0.0, 0.0]), np.array([1000.0, 0.0, 0.0]), np.array([500.0, 1e-4, 0.0])                            # a needle
    for p in ([500, 1, 0.2], [-3, 0, 0], [1200, -1, 0], [250, 5e-5, 0], [700, 0, -2]):
        rows.append((N1, N2, N3, np.array(p, dtype=np.float64)))
    for p in ([0.5, 0.5, 0.5], [1, 1, 1], [-1, 0, 0]):                                                                            # zero area: a segment, a point
        rows.append((A, B, 0.5 * (A + B), np.array(p, dtype=np.float64)))
        rows.append((B, B, B, np.array(p, dtype=np.float64)))
    sub = float(fi.tiny) / 8                                                                                                     # subnormal offsets
    for p in ([sub, sub, 0], [0.5, 0.25, sub], [-sub, 0.5, 0], [1, -sub, sub]):
        rows.append((A, B, Cc, np.array(p, dtype=np.float64)))
    big = float(np.sqrt(np.float64(fi.max))) * 4                                                                                # products overflow: Inf - Inf, a NaN answer
    rows.append((A, np.array([big, 0.0, 0.0]), np.array([0.0, big, 0.0]), np.array([big / 4, big / 4, 1.0])))
    return np.array([np.concatenate(r) for r in rows]).astype(T)


def _sph_rows(T):
    fi = np.finfo(T)
    sub = float(fi.tiny) / 8
    c = [0.5, -1.0, 2.0]
    rows = [c + [1.5] + c,                                   # the sphere's centre
            c + [1.5] + [0.5 + sub, -1.0, 2.0],             # a subnormal offset: l below the smallest normal
            c + [1.5] + [0.5, -1.0 + float(fi.tiny) * 4, 2.0],
            c + [1.5] + [3.0, 1.0, 2.5], c + [1.5] + [0.6, -1.1, 2.2], c + [1.5] + [2.0, -1.0, 2.0],
            [0, -100.5, -1, 100] + [0.3, 0.1, -0.7], [-0.0, -0.0, -0.0, 0.0] + [-0.0, -0.0, -0.0], [0, 0, 0, 0] + [1, 2, 3]]
    return np.array(rows, dtype=np.float64).astype(T)


def _point_rows(T, frame):
    c0 = np.zeros(3) if frame is None else np.asarray(frame[0], dtype=np.float64)
    u = 1.0 if frame is None else 1.0 / float(frame[1])              # one frame unit
    good = np.concatenate([c0 + np.array([0.25, 1.0, 3.0]) * u, [np.inf]]).astype(T)
    rows = [good, np.concatenate([c0 + np.array([1, 2, 3]) * u, [0]]).astype(T), np.concatenate([c0 + np.array([-1, 0.5, 2]) * u, [-0.0]]).astype(T),
            np.concatenate([c0, [float(np.finfo(T).max)]]).astype(T)]
    rows += [r.astype(T) for r in N.invalid_kinds(T, frame)]
    if frame is not None:
        c, scale = np.asarray(frame[0], dtype=T), T(frame[1])
        for k in range(3):
            for sign in ((1, -1) if c[k] == 0 else (int(np.sign(c[k])),)):        # (away from 0: p - c is then exact for p one ulp off the bound)
                on = T(c[k] + T(sign * 64) / scale)
                r = good.copy(); r[k] = on; rows.append(r)
                r = good.copy(); r[k] = np.nextafter(on, T(sign * np.inf)); rows.append(r)
                r = good.copy(); r[k] = np.nextafter(on, T(0) if c[k] == 0 else c[k]); rows.append(r)
    return np.array(rows, dtype=T)


@pytest.fixture(scope="module")
def nearest_exe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("nearest") / "nearest_plan")
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g", "-O1"]
    subprocess.run(["g++", "-std=c++17", "-ffp-contract=off", os.path.join(ROOT, "tests", "native", "nearest_plan.cpp"), "-o", exe] + san, check=True)
    return exe


def _frames(prec):
    """No tree, two hand-made frames, and the fresh build's frame of the blob mesh in the four placements of cast_support.FRAMES."""
    return [None, ((0.0, 0.0, 0.0), 1.0), ((0.5, -2.0, 8.0), 0.25)] + [S.mesh_frame(S.blob_scene(2, *f)["triangles10"], prec) for f in S.FRAMES]


@pytest.mark.parametrize("prec", ["f32", "f64"])
@pytest.mark.parametrize("fi", range(7))
def test_the_kernels_functions_under_asan_ubsan_equal_the_twins(nearest_exe, prec, fi):
    T = S.dtype_of(prec)
    U = np.uint32 if prec == "f32" else np.uint64
    frame = _frames(prec)[fi]
    pts, tri, sph = _point_rows(T, frame), _tri_rows(T), _sph_rows(T)
    if fi > 0:
        tri, sph = tri[:4], sph[:2]              # the arithmetic does not depend on the frame: once in full is enough
    e = np.concatenate([tri[:, 0:3], tri[:, 3:6] - tri[:, 0:3], tri[:, 6:9] - tri[:, 0:3], tri[:, 9:12]], axis=1)
    head = "%s %d %r %r %r %r\n" % ((prec, 1) + tuple(float(x) for x in frame[0]) + (float(frame[1]),)) if frame else "%s 0 0 0 0 1\n" % prec
    hexrow = lambda row: " ".join("%x" % int(w) for w in np.ascontiguousarray(row).view(U))
    body = "".join("P " + hexrow(r) + "\n" for r in pts) + "".join("T " + hexrow(r) + "\n" for r in e) + "".join("S " + hexrow(r) + "\n" for r in sph)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([nearest_exe], input=head + body, capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0 and "all checks passed" in r.stdout and "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stdout[-2000:] + r.stderr[-4000:]
    assert "%d lines answered" % (len(pts) + len(e) + len(sph)) in r.stdout
    # ---- validity
    verdicts = np.array([int(x) for x in re.findall(r"^pt (\d)$", r.stdout, flags=re.M)], dtype=bool)
    _, valid = query.prepare_points(pts, T, frame)
    assert np.array_equal(verdicts, valid), np.flatnonzero(verdicts != valid)
    n_inv = len(N.invalid_kinds(T, frame))
    assert valid[:4].all() and not valid[4:4 + n_inv].any()                                      # every invalidity cause alone
    if frame is not None:
        rest = valid[4 + n_inv:]
        assert len(rest) in (9, 12, 15, 18) and list(rest) == [True, False, True] * (len(rest) // 3)     # on the bound, one ulp outside, one ulp inside
    # ---- the two closest-point functions, bit for bit
    got = np.array([[int(x, 16) for x in g] for g in re.findall(r"^tri ([0-9a-f]+) ([0-9a-f]+) ([0-9a-f]+) ([0-9a-f]+)$", r.stdout, flags=re.M)], dtype=U)
    q, d2 = query.closest_point_triangle(e[:, 0:3], e[:, 3:6], e[:, 6:9], e[:, 9:12])
    want = np.concatenate([q, d2[:, None]], axis=1)
    nan = np.isnan(want)
    assert got.shape == want.shape and np.array_equal(np.isnan(got.view(T)), nan) and np.array_equal(got[~nan], np.ascontiguousarray(want).view(U)[~nan])
    got = np.array([[int(x, 16) for x in g] for g in re.findall(r"^sph ([0-9a-f]+) ([0-9a-f]+) ([0-9a-f]+) ([0-9a-f]+)$", r.stdout, flags=re.M)], dtype=U)
    q, d2 = query.closest_point_sphere(sph[:, 0:3], sph[:, 3], sph[:, 4:7])
    want = np.concatenate([q, d2[:, None]], axis=1)
    assert got.shape == want.shape and np.array_equal(got, np.ascontiguousarray(want).view(U))
    if fi == 0:
        # what the table is for: the seven regions answer what geometry says, and a triangle whose answer is NaN is never picked
        q, d2 = query.closest_point_triangle(e[:, 0:3], e[:, 3:6], e[:, 6:9], e[:, 9:12])
        expect = np.array([[0, 0, 0], [2, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0.5, 0], [1.4, 0.3, 0], [0.5, 0.25, 0]])      # (2, 1.5) on the edge (2, 0) - (0, 1): t = 1.5 / 5
        assert np.abs(q[:7].astype(np.float64) - expect).max() <= 4 * np.finfo(T).eps      # coordinates up to 2: two ulps
        assert np.array_equal(d2[7:14], np.zeros(7, dtype=T)) and np.array_equal(q[7:10], tri[7:10, 9:12])      # exactly on vertices, edges, the face
        scene = dict(spheres5=np.zeros((0, 5)), triangles10=np.concatenate([tri[:, :9], np.ones((len(tri), 1), dtype=T)], axis=1))
        ns = N.NearScan(scene, prec)
        prim, dist, point, _ = ns.query(np.concatenate([tri[:, 9:12], np.full((len(tri), 1), np.inf, dtype=T)], axis=1).astype(np.float64))
        _, d_all = ns.d2_all(tri[:, 9:12])
        assert np.isnan(d_all).any() and (prim >= 0).all() and not np.isnan(dist).any() and not np.isnan(point).any()
        assert not np.isnan(d_all[np.arange(len(prim)), prim]).any()
        sq, sd = query.closest_point_sphere(sph[:, 0:3], sph[:, 3], sph[:, 4:7])
        assert np.array_equal(sq[0], np.array([2.0, -1.0, 2.0], dtype=T)) and np.array_equal(sq[1], sq[0]) and sd[0] == T(2.25)      # the centre: c + (r, 0, 0)


# ------------------------------------------------------------------ properties of the twin, whatever its formulas
SLACK = 64      # multiples of eps * max(|p|, |v|)^2


@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_the_twin_returns_a_closest_point_of_the_triangle(prec):
    """4 096 random point / triangle pairs.  q lies in the triangle: its barycentric coordinates, solved for in extended precision from q itself, are within
    [0, 1] up to SLACK eps; and no point of the triangle is closer: d2 <= |p - x|^2 + SLACK eps M^2 for 64 random points x of the triangle and its three
    vertices, M = max(|p|, |v|) the largest coordinate magnitude of the pair.  Why that unit: q and r = p - q are each a few roundings of values of
    magnitude M, so d2 = |r|^2 is off by a few eps M |r| <= a few eps M^2; 64 covers the dozen operations of the longest region with room."""
    T = S.dtype_of(prec)
    eps = float(np.finfo(T).eps)
    rng = np.random.default_rng(41)
    n = 4096
    v = (rng.normal(size=(n, 3, 3)) * rng.choice([0.1, 1.0, 30.0], size=(n, 1, 1)) + rng.normal(size=(n, 1, 3)) * 3).astype(T)
    p = (v.astype(np.float64).mean(axis=1) + rng.normal(size=(n, 3)) * rng.choice([0.01, 1.0, 50.0], size=(n, 1))).astype(T)
    e1, e2 = v[:, 1] - v[:, 0], v[:, 2] - v[:, 0]
    q, d2 = query.closest_point_triangle(v[:, 0], e1, e2, p)
    assert q.dtype == T and d2.dtype == T and not np.isnan(d2).any()
    W = np.longdouble                                                # the check itself in extended precision: in Float64 it would round as much as what it checks
    V, P, Q = v.astype(W), p.astype(W), q.astype(W)
    M = np.maximum(np.abs(P).max(axis=1), np.abs(V).reshape(n, 9).max(axis=1))
    E1, E2 = V[:, 1] - V[:, 0], V[:, 2] - V[:, 0]
    # barycentric coordinates of q by least squares
    a11, a12, a22 = (E1 * E1).sum(1), (E1 * E2).sum(1), (E2 * E2).sum(1)
    b1, b2 = ((Q - V[:, 0]) * E1).sum(1), ((Q - V[:, 0]) * E2).sum(1)
    det = a11 * a22 - a12 * a12
    bv, bw = (b1 * a22 - b2 * a12) / det, (b2 * a11 - b1 * a12) / det
    off = Q - (V[:, 0] + bv[:, None] * E1 + bw[:, None] * E2)
    edge = np.sqrt(np.minimum(a11, a22))
    tol_b = SLACK * eps * M / edge                                   # a coordinate error of SLACK eps M, in units of the shorter edge
    worst_b = max(float((-bv / tol_b).max()), float((-bw / tol_b).max()), float(((bv + bw - 1) / tol_b).max()))
    worst_plane = float((np.sqrt((off * off).sum(1)) / (SLACK * eps * M)).max())
    a, b = rng.random((n, 64, 1)), rng.random((n, 64, 1))
    flip = (a + b) > 1
    a, b = np.where(flip, 1 - a, a), np.where(flip, 1 - b, b)
    X = np.concatenate([V[:, 0:1] + a * E1[:, None] + b * E2[:, None], V], axis=1)
    dX = ((P[:, None] - X) ** 2).sum(axis=2).min(axis=1)
    worst_d = float(((d2.astype(W) - dX) / (eps * M * M)).max())
    print(prec, "worst barycentric excess %.3f of the slack, off-plane %.3f of the slack, d2 - min over samples %.3f eps M^2 (slack %d)" % (worst_b, worst_plane, worst_d, SLACK))
    assert worst_b <= 1 and worst_plane <= 1 and worst_d <= SLACK


@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_the_exported_triangle_function_equals_the_twin(binding, prec):
    T = S.dtype_of(prec)
    tri = _tri_rows(T)
    rng = np.random.default_rng(42)
    rnd = np.concatenate([rng.normal(size=(256, 9)), rng.normal(size=(256, 3)) * 2], axis=1).astype(T)
    rows = np.concatenate([tri, rnd])
    v0, e1, e2, p = rows[:, 0:3], rows[:, 3:6] - rows[:, 0:3], rows[:, 6:9] - rows[:, 0:3], rows[:, 9:12]
    q, d2 = query.closest_point_triangle(v0, e1, e2, p)
    U = np.uint32 if prec == "f32" else np.uint64
    for i in range(len(rows)):
        gq, gd = binding.closest_point_triangle(v0[i], e1[i], e2[i], p[i], prec)
        if np.isnan(d2[i]):
            assert np.isnan(gd), i
        else:
            assert np.array_equal(gq.view(U), np.ascontiguousarray(q[i]).view(U)) and np.array([gd]).view(U)[0] == np.array([d2[i]]).view(U)[0], i
    fn = getattr(binding.lib(), "spira_closest_point_triangle_" + prec)
    fn.restype = None
    a = [np.ascontiguousarray(x[0]).ctypes.data_as(C.c_void_p) for x in (v0, e1, e2, p)]
    fn(*a, None, None)                                               # both outputs may be NULL


def test_return_codes_without_a_device(binding):
    """Every argument error of the entries is decided before any device is touched: it returns its own code, not SPIRA_E_NO_DEVICE (-2)."""
    lib = binding.lib()
    pts = np.zeros((4, 4), dtype=np.float64)
    pp, out = pts.ctypes.data_as(C.c_void_p), np.zeros(64, dtype=np.float64).ctypes.data_as(C.c_void_p)
    u32 = C.c_uint32
    for name in ENTRIES:
        fn = getattr(lib, name)
        tail = (None,) if "device" in name else ()

        def call(scene, p, n, flags, outs):
            return fn(scene, p, u32(n), u32(flags), *(outs + tail))
        outs = (out, out, out, None)
        assert call(None, None, 4, 0, outs) == -1 and b"point array is NULL" in lib.spira_last_error(), name
        assert call(None, pp, 0, 0, outs) == -1 and b"n_points is 0" in lib.spira_last_error(), name
        assert call(None, pp, 4, 2, outs) == -1 and b"unknown flag bits" in lib.spira_last_error(), name
        assert call(None, pp, 4, 0x80000001, outs) == -1, name
        assert call(None, pp, 4, 0, (None, None, None, out)) == -1 and b"all NULL" in lib.spira_last_error(), name      # trips alone is no output
        assert call(None, pp, (1 << 26) + 1, 0, outs) == -4 and b"SPIRA_MAX_RAYS" in lib.spira_last_error(), name
        assert call(None, pp, 4, 0, outs) == -1 and b"scene handle is NULL or was destroyed" in lib.spira_last_error(), name
        assert call(None, pp, 4, 1, (None, None, out, None)) == -1 and b"scene handle is NULL" in lib.spira_last_error(), name


def test_the_point_sets_reach_what_they_are_for():
    """Asserted from the scan's answers alone (the sets the GPU tests run): hits, misses and invalid points are all there, r_max = the found distance
    mostly keeps the winner and one ulp less always loses it, the far points are valid and their twins are not, exact ties exist in the duplicate scene."""
    for prec in ("f32", "f64"):
        r, ns = N.reference("s4_3", prec), N.scan_of("s4_3", prec)
        prim, parts = r["prim"], r["parts"]
        assert 1900 <= len(prim) <= 2300
        assert (prim[parts["near"]] >= ns.ns).mean() > 0.9 and (prim[parts["box"]] >= 0).all()
        assert (prim[parts["same"]] == prim[r["sel"]]).mean() > 0.5 and ((prim[parts["same"]] == prim[r["sel"]]) | (prim[parts["same"]] == N.MISS)).all()
        assert (prim[parts["below"]] == N.MISS).all() and np.array_equal(r["dist"][parts["below"]], r["points"][parts["below"], 3].astype(ns.T))
        assert (prim[parts["zero"]] >= 0).any() and (prim[parts["zero"]] == N.MISS).any()
        far = prim[parts["far"]]
        assert (far[0::2] >= 0).all() and (far[1::2] == N.INVALID).all()
        assert (prim[r["invalid_at"]] == N.INVALID).all() and (prim[r["invalid_at"][:-1] + 1] >= 0).all()
        assert not r["dist"][prim == N.INVALID].any() and not r["point"][prim < 0].any()
        d = N.reference("dup", prec)
        nd = N.scan_of("dup", prec)
        _, d2 = nd.d2_all(d["points"][d["parts"]["near"]][:64, :3].astype(nd.T))
        m = d2.min(axis=1)
        assert ((d2 == m[:, None]).sum(axis=1) >= 2).all()               # every point has an exact tie at the minimum ...
        first = np.argmax(d2 == m[:, None], axis=1)
        assert (d["prim"][d["parts"]["near"]][:64] > first).all()         # ... and the scan takes the later one
