"""CPU: spira_scene_overlap_tri_* / spira_scene_overlap_tri_any_* without a device — the library exports the entries and the header and the binding name
them; a table of exact cases (small integers); the 20-axis separating-axis test against an independent statement of "two triangles intersect" (an edge of
one pierces the other: six Moeller-Trumbore segment tests) on 200 000 random pairs in Float64; the numpy twins of spira_hip.query against the exported host
arithmetic, byte for byte; the functions the kernels call (spira_trioverlap.h) in tests/native/trioverlap_plan.cpp under ASan + UBSan against the twins; the
lemma the tree walk prunes by (a scene triangle beyond the query's enclosing box by HALF the walk's growth along a world axis is rejected by the leaf test);
the argument errors that need no device; and the query sets of the GPU test reach the states they are for."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import cast_support as S
import trioverlap_support as W
from spira_hip import query

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TRI = ["spira_scene_overlap_tri_f32", "spira_scene_overlap_tri_f64", "spira_scene_overlap_tri_device_f32", "spira_scene_overlap_tri_device_f64"]
ANY = ["spira_scene_overlap_tri_any_f32", "spira_scene_overlap_tri_any_f64", "spira_scene_overlap_tri_any_device_f32", "spira_scene_overlap_tri_any_device_f64"]
HOST = ["spira_overlap_tri_triangle_f32", "spira_overlap_tri_triangle_f64", "spira_overlap_tri_sphere_f32", "spira_overlap_tri_sphere_f64"]


def test_library_header_and_binding_name_the_entries(binding):
    lib = binding.lib()
    hdr = open(os.path.join(ROOT, "include", "spira_hip.h")).read()
    for name in TRI + ANY:
        assert hasattr(lib, name) and name in binding.EXPORTS and re.search(r"^int %s\(const spira_scene \*scene, " % name, hdr, flags=re.M), name
    for name in HOST:
        assert hasattr(lib, name) and name in binding.EXPORTS and re.search(r"^int %s\(const " % name, hdr, flags=re.M), name
    assert "#define SPIRA_ABI_VERSION 3 " in hdr and lib.spira_abi_version() == 3
    for m in ("overlap_tri", "overlap_tri_device", "overlap_tri_any", "overlap_tri_any_device"):
        assert hasattr(binding.Scene, m), m
    for f in ("prepare_triangles", "overlap_tri_triangle", "overlap_tri_sphere", "overlap_triangles", "mesh_pairs", "meshes_intersect"):
        assert hasattr(query, f), f
    mk = open(os.path.join(ROOT, "julia-spira_amd", "csrc", "Makefile")).read()
    assert "spira_trioverlap.h" in mk.split("DEPS", 1)[1].split("\n", 1)[0]      # hashed into spira_build_id


def test_kernels_live_in_the_unit_of_their_precision():
    csrc = os.path.join(ROOT, "julia-spira_amd", "csrc")
    objs = {n: os.path.join(csrc, "spira_tu_%s.o" % n) for n in ("main", "f32", "f64mesh")}
    if not all(os.path.exists(o) for o in objs.values()):
        pytest.skip("objects not present (library built elsewhere)")
    syms = {n: subprocess.run(["nm", o], capture_output=True, text=True, check=True).stdout for n, o in objs.items()}
    for kern in ("12k_trioverlap", "20k_trioverlap_session"):
        assert len(re.findall(kern + "If", syms["f32"])) > 0 and len(re.findall(kern + "Id", syms["f32"])) == 0, kern
        assert len(re.findall(kern + "Id", syms["main"])) > 0 and len(re.findall(kern + "If", syms["main"])) == 0, kern
        assert len(re.findall(kern + "I[fd]", syms["f64mesh"])) == 0, kern


# ------------------------------------------------------------------ the exact table (small integers: every operation is exact in both precisions)
QUERY = [(0, 0, 0), (4, 0, 0), (0, 4, 0)]
NAN = float("nan")
# (name, the scene triangle's three vertices, candidate?)
TABLE = [
    ("a shared vertex", [(0, 0, 0), (-2, 0, 3), (0, -2, 3)], True),
    ("a shared edge", [(0, 0, 0), (4, 0, 0), (2, 0, 3)], True),
    ("coplanar, overlapping", [(1, 1, 0), (6, 1, 0), (1, 6, 0)], True),
    ("coplanar, the scene triangle inside the query", [(1, 1, 0), (2, 1, 0), (1, 2, 0)], True),
    ("coplanar, the query inside the scene triangle", [(-4, -4, 0), (12, -4, 0), (-4, 12, 0)], True),
    ("coplanar, touching along the hypotenuse", [(4, 0, 0), (0, 4, 0), (4, 4, 0)], True),
    ("an edge pierces the query's face", [(1, 1, -1), (1, 1, 1), (5, 5, 1)], True),
    ("cuts the query's interior, neither holds a vertex of the other", [(1, -4, -4), (1, 8, -4), (1, 2, 8)], True),
    ("coplanar, disjoint, apart only along the hypotenuse's normal", [(3, 3, 0), (5, 3, 0), (3, 5, 0)], False),
    ("coplanar, disjoint, beside a leg", [(1, -3, 0), (3, -3, 0), (2, -1, 0)], False),
    ("parallel planes one unit apart", [(1, 1, 1), (2, 1, 1), (1, 2, 1)], False),
    ("tilted, beside the hypotenuse", [(5, 0, -1), (5, 0, 1), (0, 5, 1)], False),
    ("zero area inside the query (a segment)", [(1, 1, 0), (2, 2, 0), (3, 3, 0)], False),
    ("zero area (a point) on the query", [(1, 1, 0), (1, 1, 0), (1, 1, 0)], False),
    ("a NaN vertex", [(1, 1, -1), (1, NAN, 1), (5, 5, 1)], False),
]
# (name, centre, R, candidate?): a shell
BALLS = [
    ("cuts the face", (1, 1, 1), 2.0, True),
    ("the whole triangle inside", (1, 1, 0), 10.0, False),
    ("the whole triangle outside", (1, 1, 5), 2.0, False),
    ("through one vertex from outside", (4, 0, 3), 3.0, True),
    ("through two vertices, the rest inside", (0, 0, 0), 4.0, True),
    ("tangent to the face from above", (1, 1, 2), 2.0, True),
    ("a NaN centre", (1, NAN, 1), 2.0, False),
]
DEGENERATE = [[(0, 0, 0), (1, 1, 1), (2, 2, 2)], [(3, 1, 2), (3, 1, 2), (0, 4, 0)], [(3, 1, 2), (3, 1, 2), (3, 1, 2)]]


def _rows(table):
    q = np.array(QUERY, dtype=np.float64).reshape(9)
    return np.array([np.concatenate([np.array(v[0]), np.array(v[1]) - np.array(v[0]), np.array(v[2]) - np.array(v[0]), q, [NAN]]) for _, v, _ in table])


def _twin_tri(rows, T):
    """The twin on rows [v0 e1 e2 query10]: 1, 0, or -3 where the query is invalid without a frame."""
    rows = np.asarray(rows, dtype=T)
    q0, g1, g2, m, _, _, valid = query.prepare_triangles(rows[:, 9:19], T)
    return np.where(valid, query.overlap_tri_triangle(rows[:, 0:3], rows[:, 3:6], rows[:, 6:9], q0, g1, g2, m).astype(np.int64), -3)


def _twin_sph(rows, T):
    rows = np.asarray(rows, dtype=T)
    q0, g1, g2, _, q1, q2, valid = query.prepare_triangles(rows[:, 4:14], T)
    return np.where(valid, query.overlap_tri_sphere(rows[:, 0:3], rows[:, 3], q0, g1, g2, q1, q2).astype(np.int64), -3)


def _ball_rows():
    q = np.array(QUERY, dtype=np.float64).reshape(9)
    return np.array([np.concatenate([np.array(c, dtype=np.float64), [r], q, [NAN]]) for _, c, r, _ in BALLS])


@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_the_exact_table(binding, prec):
    T = S.dtype_of(prec)
    rows, balls = _rows(TABLE), _ball_rows()
    got = _twin_tri(rows, T)
    for (name, _, want), g, r in zip(TABLE, got, rows.astype(T)):
        assert g == int(want), name
        assert binding.overlap_tri_triangle(r[0:3], r[3:6], r[6:9], r[9:19], prec) == int(want), name
    # the verdict does not depend on which vertex of either triangle comes first
    for rot in range(1, 3):
        for name, v, want in TABLE:
            vs = [v[(k + rot) % 3] for k in range(3)]
            qs = [QUERY[(k + rot) % 3] for k in range(3)]
            for vv, qq in ((vs, QUERY), (v, qs), (vs, qs)):
                row = np.concatenate([np.array(vv[0]), np.array(vv[1]) - np.array(vv[0]), np.array(vv[2]) - np.array(vv[0]), np.array(qq, dtype=np.float64).reshape(9), [0.0]])
                assert _twin_tri(row[None], T)[0] == int(want), (name, rot)
    got = _twin_sph(balls, T)
    for (name, _, _, want), g, r in zip(BALLS, got, balls.astype(T)):
        assert g == int(want), name
        assert binding.overlap_tri_sphere(r[0:3], r[3], r[4:14], prec) == int(want), name
    for d in DEGENERATE:                                              # a zero-area query is invalid, whatever it is asked about
        q10 = np.concatenate([np.array(d, dtype=np.float64).reshape(9), [1.0]])
        assert not query.prepare_triangles(q10[None], T)[6][0]
        assert binding.overlap_tri_triangle([0, 0, 0], [1, 0, 0], [0, 1, 0], q10, prec) == -3 and binding.overlap_tri_sphere([0, 0, 0], 1.0, q10, prec) == -3


# ------------------------------------------------------------------ the SAT against an independent statement
def _pierces(p, d, a, e1, e2):
    """Moeller-Trumbore: does the segment p .. p + d meet the triangle (a, a + e1, a + e2)?  Float64, arrays [n, 3].  Returns (verdict, how close to a
    boundary the decision came: the smallest distance of u, v, 1 - u - v, t, 1 - t from 0, in their own units)."""
    with np.errstate(all="ignore"):
        h = S._cross(d, e2)
        det = S._dot(e1, h)
        s = p - a
        u = S._dot(s, h) / det
        q = S._cross(s, e1)
        v = S._dot(d, q) / det
        t = S._dot(e2, q) / det
        hit = (u >= 0) & (v >= 0) & (u + v <= 1) & (t >= 0) & (t <= 1)
        edge = np.minimum.reduce([np.abs(u), np.abs(v), np.abs(1 - u - v), np.abs(t), np.abs(1 - t)])
    return hit, edge


def test_the_sat_equals_the_piercing_test_on_random_pairs():
    """Gaussian vertices; scene triangles scaled by 0.3 / 1 / 2 and offset by 0.7 sigma.  In general position two triangles intersect exactly when an edge of
    one pierces the other; the 20 axes must say the same on every pair, none left out."""
    rng = np.random.default_rng(2024)
    n = 200_000
    qv = rng.normal(size=(n, 3, 3))
    sv = rng.normal(size=(n, 3, 3)) * np.array([0.3, 1.0, 2.0])[np.arange(n) % 3, None, None] + 0.7 * rng.normal(size=(n, 1, 3))
    q10 = np.concatenate([qv.reshape(n, 9), np.zeros((n, 1))], axis=1)
    q0, g1, g2, m, _, _, valid = query.prepare_triangles(q10, np.float64)
    assert valid.all()
    v0, e1, e2 = sv[:, 0], sv[:, 1] - sv[:, 0], sv[:, 2] - sv[:, 0]
    sat = query.overlap_tri_triangle(v0, e1, e2, q0, g1, g2, m)
    pierce = np.zeros(n, dtype=bool)
    for k in range(3):
        pierce |= _pierces(sv[:, k], sv[:, (k + 1) % 3] - sv[:, k], q0, g1, g2)[0]
        pierce |= _pierces(qv[:, k], qv[:, (k + 1) % 3] - qv[:, k], v0, e1, e2)[0]
    share = pierce.mean()
    assert 0.08 < share < 0.2, share                                 # about 13 % intersect
    bad = np.flatnonzero(sat != pierce)
    assert len(bad) == 0, (len(bad), bad[:8])                        # zero disagreements, no pair excluded


# ------------------------------------------------------------------ the twins against the library's host arithmetic
def _leaf_rows(T, rng, n):
    """(v0, e1, e2, query10) and (centre, R, query10) rows in T: random pairs near each other, the table, zero-area scene triangles and queries, NaN and
    infinite values, products that overflow, and a poisoned tenth value."""
    fi = np.finfo(T)
    qv = rng.normal(size=(n, 3, 3)) * rng.choice([0.05, 1.0, 30.0], size=(n, 1, 1))
    sv = qv.mean(axis=1)[:, None, :] + rng.normal(size=(n, 3, 3)) * rng.choice([0.3, 1.0, 2.0], size=(n, 1, 1)) * np.abs(qv).max(axis=(1, 2))[:, None, None] * 0.5
    sv[3::40, 1] = sv[3::40, 0]                                       # zero-area scene triangles
    qv[5::40, 2] = qv[5::40, 0] + 2 * (qv[5::40, 1] - qv[5::40, 0])   # (nearly) collinear queries
    qv[6::400, 1] = qv[6::400, 0]                                     # segments: invalid
    tri = np.concatenate([sv[:, 0], sv[:, 1] - sv[:, 0], sv[:, 2] - sv[:, 0], qv.reshape(n, 9), rng.normal(size=(n, 1))], axis=1)
    tri[::3, 18] = np.nan                                             # the tenth value is never read
    big = float(np.sqrt(np.float64(fi.max))) * 4
    tri[7, 3:9] = [big, 0, 0, 0, big, 0]                             # the scene triangle's products overflow
    tri[11, 9] = np.nan; tri[12, 14] = np.inf; tri[13, 17] = -np.inf
    tri[14, 12] = big; tri[14, 16] = big                             # m overflows
    tri[15, 2] = np.nan
    c = qv.mean(axis=1) + rng.normal(size=(n, 3)) * np.abs(qv).max(axis=(1, 2))[:, None] * 0.5
    sph = np.concatenate([c, np.abs(qv).max(axis=(1, 2))[:, None] * rng.uniform(0.0, 1.5, (n, 1)), qv.reshape(n, 9), np.full((n, 1), np.nan)], axis=1)
    sph[11, 4] = np.nan; sph[12, 9] = np.inf
    sph[13, 3] = big * big if T is np.float64 else big
    sph[15, 1] = np.nan
    with np.errstate(over="ignore", invalid="ignore"):
        return np.concatenate([tri, _rows(TABLE)]).astype(T), np.concatenate([sph, _ball_rows()]).astype(T)


@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_the_exported_host_functions_equal_the_twins(binding, prec):
    """10^5 random pairs of each kind plus the table, the invalid kinds included: the same verdict from the library's own arithmetic and from the twin."""
    T, ct = S.dtype_of(prec), (C.c_float if prec == "f32" else C.c_double)
    tri, sph = _leaf_rows(T, np.random.default_rng(7), 100_000)
    w_tri, w_sph = _twin_tri(tri, T), _twin_sph(sph, T)
    lib = binding.lib()
    f_tri, f_sph = getattr(lib, "spira_overlap_tri_triangle_" + prec), getattr(lib, "spira_overlap_tri_sphere_" + prec)
    f_tri.restype = f_sph.restype = C.c_int
    f_tri.argtypes = [C.c_void_p] * 4
    f_sph.argtypes = [C.c_void_p, ct, C.c_void_p]
    tri, sph = np.ascontiguousarray(tri), np.ascontiguousarray(sph)
    sz = tri.itemsize
    base, step = tri.ctypes.data, tri.strides[0]
    g_tri = np.array([f_tri(a, a + 3 * sz, a + 6 * sz, a + 9 * sz) for a in range(base, base + step * len(tri), step)])
    base, step = sph.ctypes.data, sph.strides[0]
    radii = sph[:, 3].tolist()
    g_sph = np.array([f_sph(a, r, a + 4 * sz) for a, r in zip(range(base, base + step * len(sph), step), radii)])
    assert np.array_equal(g_tri, w_tri), np.flatnonzero(g_tri != w_tri)[:8]
    assert np.array_equal(g_sph, w_sph), np.flatnonzero(g_sph != w_sph)[:8]
    assert set(w_tri) == {-3, 0, 1} and set(w_sph) == {-3, 0, 1} and binding.RAY_INVALID == -3
    assert (w_tri == 1).sum() > 5000 and (w_tri == 0).sum() > 5000 and (w_sph == 1).sum() > 5000 and (w_sph == 0).sum() > 5000
    assert w_tri[7] == 0 and w_tri[15] == 0 and (w_tri[11:15] == -3).all() and (w_tri[6:100_000:400] == -3).all() and (w_tri[3:100_000:40][w_tri[3:100_000:40] >= 0] == 0).all()
    assert (w_sph[11:13] == -3).all() and w_sph[13] == 0 and w_sph[15] == 0
    for k in W.invalid_kinds(T, None):                                # invalid without a frame: the host functions say so
        assert binding.overlap_tri_triangle([0, 0, 0], [1, 0, 0], [0, 1, 0], k, prec) == -3 and binding.overlap_tri_sphere([0, 0, 0], 1.0, k, prec) == -3


# ------------------------------------------------------------------ the native program
@pytest.fixture(scope="module")
def trioverlap_exe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("trioverlap") / "trioverlap_plan")
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g", "-O1"]
    subprocess.run(["g++", "-std=c++17", "-ffp-contract=off", os.path.join(ROOT, "tests", "native", "trioverlap_plan.cpp"), "-o", exe] + san, check=True)
    return exe


def _frames(prec):
    return [None, ((0.5, -2.0, 8.0), 0.25)] + [S.mesh_frame(S.blob_scene(2, *f)["triangles10"], prec) for f in S.FRAMES[1:3]]


def _query_rows(T, frame, rng, n=120):
    """Queries for the validity rule: every invalid kind, random triangles of every size, and vertices about the origin rule of a frame."""
    u = 1.0 if frame is None else 1.0 / float(frame[1])
    c0 = np.zeros(3) if frame is None else np.asarray(frame[0], dtype=np.float64)
    q = c0 + (rng.normal(size=(n, 3, 3)) * 10.0 ** rng.uniform(-3, 1.3, (n, 1, 1)) + rng.normal(size=(n, 1, 3)) * 20) * u
    q[1::7, 0] = c0 + rng.uniform(63.0, 65.0, (len(q[1::7]), 3)) * u
    q[2::7, 2, 1] = c0[1] - rng.uniform(63.0, 65.0, len(q[2::7])) * u
    rows = np.concatenate([q.reshape(n, 9), rng.normal(size=(n, 1))], axis=1)
    rows[::2, 9] = np.nan
    with np.errstate(over="ignore"):
        return np.concatenate([W.invalid_kinds(T, frame), rows]).astype(T)


@pytest.mark.parametrize("prec", ["f32", "f64"])
@pytest.mark.parametrize("fi", range(4))
def test_the_kernels_functions_under_asan_ubsan_equal_the_twins(trioverlap_exe, prec, fi):
    T = S.dtype_of(prec)
    U = np.uint32 if prec == "f32" else np.uint64
    frame = _frames(prec)[fi]
    rng = np.random.default_rng(300 + fi)
    qs = _query_rows(T, frame, rng)
    tri, sph = _leaf_rows(T, rng, 400 if fi == 0 else 16)            # the leaf arithmetic does not depend on the frame: once in full is enough
    head = "%s %d %r %r %r %r\n" % ((prec, 1) + tuple(float(x) for x in frame[0]) + (float(frame[1]),)) if frame else "%s 0 0 0 0 1\n" % prec
    hexrow = lambda row: " ".join("%x" % int(w) for w in np.ascontiguousarray(row).view(U))
    body = "".join("Q " + hexrow(r) + "\n" for r in qs) + "".join("T " + hexrow(r) + "\n" for r in tri) + "".join("S " + hexrow(r) + "\n" for r in sph)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([trioverlap_exe], input=head + body, capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0 and "all checks passed" in r.stdout and "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stdout[-2000:] + r.stderr[-4000:]
    assert "%d lines answered" % (len(qs) + len(tri) + len(sph)) in r.stdout
    rows = re.findall(r"^tq (\d) (\d)((?: [0-9a-f]+){9})$", r.stdout, flags=re.M)
    assert len(rows) == len(qs)
    g_with, g_without = np.array([int(g[0]) for g in rows], dtype=bool), np.array([int(g[1]) for g in rows], dtype=bool)
    got = np.array([[int(x, 16) for x in g[2].split()] for g in rows], dtype=U)
    _, g1, g2, m, _, _, v_with = query.prepare_triangles(qs, T, frame)
    v_without = query.prepare_triangles(qs, T)[6]
    assert np.array_equal(g_with, v_with) and np.array_equal(g_without, v_without), (np.flatnonzero(g_with != v_with), np.flatnonzero(g_without != v_without))
    n_inv = len(W.invalid_kinds(T, frame))
    assert not v_with[:n_inv].any() and v_with[n_inv:].sum() > 20 and (~v_with[n_inv:]).sum() > (10 if frame else -1)
    want = np.where(v_without[:, None], np.concatenate([g1, g2, m], axis=1), T(0)).astype(T)
    assert np.array_equal(got, np.ascontiguousarray(want).view(U)), np.flatnonzero((got != np.ascontiguousarray(want).view(U)).any(axis=1))
    g_tri = np.array([int(x) for x in re.findall(r"^tri (-?\d)$", r.stdout, flags=re.M)])
    g_sph = np.array([int(x) for x in re.findall(r"^sph (-?\d)$", r.stdout, flags=re.M)])
    w_tri, w_sph = _twin_tri(tri, T), _twin_sph(sph, T)
    assert np.array_equal(g_tri, w_tri), np.flatnonzero(g_tri != w_tri)
    assert np.array_equal(g_sph, w_sph), np.flatnonzero(g_sph != w_sph)


# ------------------------------------------------------------------ the lemma the walk prunes by
@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_a_triangle_beyond_the_enclosing_box_by_half_the_growth_is_rejected(prec):
    """spira_trioverlap.h, "Why the growth suffices": 10^5 scene triangles per precision whose every vertex — v0 and v0 + e_m, the values the record holds —
    lies beyond the query's enclosing box by half the growth 2^-13 (M + 1) along a world axis, one vertex exactly at that distance and the triangle
    otherwise across the box; queries at the frame's centre and 60 frame units away.  The leaf test in T rejects every one."""
    T = S.dtype_of(prec)
    rng = np.random.default_rng(41)
    n = 100_000
    centre, scale = np.array([0.5, -2.0, 8.0]), 0.25
    off = np.where((np.arange(n) % 2 == 0)[:, None], 0.0, 60.0) * np.where(rng.random((n, 3)) < 0.5, -1.0, 1.0)
    size = 10.0 ** rng.uniform(-2, 0.5, (n, 1, 1))
    q = ((centre + (off[:, None, :] + rng.uniform(-1.0, 1.0, (n, 3, 3)) * size) / scale).astype(T)).astype(np.float64)      # within 63.2 units
    q10 = np.concatenate([q.reshape(n, 9), np.zeros((n, 1))], axis=1)
    q0, g1, g2, m, _, _, valid = query.prepare_triangles(q10, T, (centre, scale))
    assert valid.all()
    lo, hi = q.min(axis=1), q.max(axis=1)                            # exact in T
    cT = centre.astype(T)
    flo = ((lo.astype(T) - cT) * T(scale)).astype(np.float32)         # overlap_enter's arithmetic
    fhi = ((hi.astype(T) - cT) * T(scale)).astype(np.float32)
    M = np.maximum(np.abs(flo), np.abs(fhi)).max(axis=1)
    g = (M + np.float32(1)) * np.float32(2.0 ** -12)
    assert g.dtype == np.float32 and (M[1::2] > 50).all() and (M[0::2] < 20).all()
    gap = g.astype(np.float64) / 2 / scale                           # half the growth, in the caller's units
    k, up = rng.integers(0, 3, n), rng.random(n) < 0.5
    rows = np.arange(n)
    bound = np.where(up, hi[rows, k] + gap, lo[rows, k] - gap)
    sgn = np.where(up, 1.0, -1.0)
    ext = (hi - lo).max(axis=1)
    v = (lo + hi)[:, None, :] / 2 + rng.normal(size=(n, 3, 3)) * ext[:, None, None]
    d = rng.uniform(0.0, 2.0, (n, 3)) * ext[:, None]
    d[rows, rng.integers(0, 3, n)] = 0.0                             # one vertex exactly at half the growth
    v[rows, :, k] = (bound[:, None] + sgn[:, None] * d)
    v = v.astype(T)
    for _ in range(20):                                              # rounding may have pulled a vertex, or v0 + e_m, back inside the bound: outward by the deficit
        e1, e2 = v[:, 1] - v[:, 0], v[:, 2] - v[:, 0]
        held = np.stack([v[:, 0].astype(np.float64), v[:, 0].astype(np.float64) + e1, v[:, 0].astype(np.float64) + e2], axis=1)[rows, :, k]
        short = (bound[:, None] - held) * sgn[:, None]
        inside = short > 0
        if not inside.any():
            break
        vk = v[rows, :, k].astype(np.float64)
        ulp = np.spacing(np.abs(v[rows, :, k]).max(axis=1).astype(T)).astype(np.float64)[:, None]
        v[rows, :, k] = np.where(inside, vk + sgn[:, None] * (short + ulp), vk).astype(T)
    assert not inside.any()
    e1, e2 = v[:, 1] - v[:, 0], v[:, 2] - v[:, 0]
    assert (np.abs(held - bound[:, None]).min(axis=1) <= 8 * np.spacing(np.abs(v[rows, :, k]).max(axis=1).astype(T))).mean() > 0.99      # a vertex AT the distance, not merely beyond
    got = query.overlap_tri_triangle(v[:, 0], e1, e2, q0, g1, g2, m)
    assert not got.any(), (int(got.sum()), np.flatnonzero(got)[:8])
    # the same triangles moved onto the box's side of the bound by the box's extent are mostly candidates' neighbours: the test above is not vacuous
    v2 = v.copy()
    v2[rows, :, k] = (v[rows, :, k].astype(np.float64) - sgn[:, None] * (gap + 0.5 * ext)[:, None]).astype(T)
    assert query.overlap_tri_triangle(v2[:, 0], v2[:, 1] - v2[:, 0], v2[:, 2] - v2[:, 0], q0, g1, g2, m).mean() > 0.05


# ------------------------------------------------------------------ argument errors
def test_return_codes_without_a_device(binding):
    """Every argument error of the entries is decided before any device is touched: it returns its own code, not SPIRA_E_NO_DEVICE (-2)."""
    lib = binding.lib()
    tris = np.zeros((4, 10), dtype=np.float64)
    tp, out = tris.ctypes.data_as(C.c_void_p), np.zeros(256, dtype=np.float64).ctypes.data_as(C.c_void_p)
    u32 = C.c_uint32
    for name in TRI:
        fn = getattr(lib, name)
        tail = (None,) if "device" in name else ()

        def call(scene, b, n, k, flags, outs):
            return fn(scene, b, u32(n), u32(k), u32(flags), *(outs + tail))
        outs, none = (out, out, None), (None, None, out)                              # trips alone is no output
        assert call(None, None, 4, 4, 0, outs) == -1 and b"query triangle array is NULL" in lib.spira_last_error(), name
        assert call(None, tp, 0, 4, 0, outs) == -1 and b"n is 0" in lib.spira_last_error(), name
        assert call(None, tp, 4, 4, 2, outs) == -1 and b"unknown flag bits" in lib.spira_last_error(), name
        assert call(None, tp, 4, 4, 0x80000001, outs) == -1, name
        assert call(None, tp, 4, 17, 0, outs) == -1 and b"SPIRA_MAX_OVERLAP" in lib.spira_last_error(), name
        assert call(None, tp, 4, 4, 0, none) == -1 and b"every output is NULL" in lib.spira_last_error(), name
        assert call(None, tp, 4, 0, 0, (out, None, None)) == -1 and b"out_count is NULL" in lib.spira_last_error(), name      # count only needs the count
        assert call(None, tp, (1 << 26) + 1, 0, 0, outs) == -4 and b"SPIRA_MAX_RAYS" in lib.spira_last_error(), name
        assert call(None, tp, (1 << 22) + 1, 16, 0, outs) == -4 and b"n * max_list" in lib.spira_last_error(), name
        for k in (0, 1, 16):
            assert call(None, tp, 4, k, 0, outs) == -1 and b"scene handle is NULL or was destroyed" in lib.spira_last_error(), (name, k)
        assert call(None, tp, 4, 4, 1, outs) == -1 and b"scene handle is NULL" in lib.spira_last_error(), name
    for name in ANY:
        fn = getattr(lib, name)
        tail = (None,) if "device" in name else ()

        def call(scene, b, n, flags, hit):
            return fn(scene, b, u32(n), u32(flags), hit, *tail)
        assert call(None, None, 4, 0, out) == -1 and b"query triangle array is NULL" in lib.spira_last_error(), name
        assert call(None, tp, 0, 0, out) == -1 and b"n is 0" in lib.spira_last_error(), name
        assert call(None, tp, 4, 2, out) == -1 and b"unknown flag bits" in lib.spira_last_error(), name
        assert call(None, tp, 4, 0, None) == -1 and b"NULL" in lib.spira_last_error(), name
        assert call(None, tp, (1 << 26) + 1, 0, out) == -4 and b"SPIRA_MAX_RAYS" in lib.spira_last_error(), name
        assert call(None, tp, 4, 0, out) == -1 and b"scene handle is NULL or was destroyed" in lib.spira_last_error(), name


# ------------------------------------------------------------------ the query sets
@pytest.mark.parametrize("prec", ["f32", "f64"])
@pytest.mark.parametrize("name", ["ico20", "ico33", "torus"])
def test_the_query_sets_reach_the_states_they_are_for(name, prec):
    ref, ss = W.reference(name, prec), W.scan_of(name, prec)
    W.conditions(ref)
    parts, count, valid = ref["parts"], ref["count"], ref["valid"]
    assert (ss.frame is None) == (name == "ico20") and 1800 <= len(count) <= 2200
    assert (count[parts["slice"]] > 16).all() and (count[parts["share"]] > 0).mean() > 0.95 and (count[parts["needle"]][1::2] == 0).all()
    assert (ref["hit"][ref["invalid_at"]] == 255).all() and valid[ref["invalid_at"][:-1] + 1].all()
    assert len(ref["invalid_at"]) >= len(W.invalid_kinds(ss.T, ss.frame)) and np.isnan(ref["tris"][2::3, 9]).all()
    if ss.frame is not None:
        far = valid[parts["far"]]
        assert far[0::2].all() and not far[1::2].any() and (count[parts["far"]][0::2] > 0).sum() >= 8
    for k in (1, 4, 5, 16):
        lst = W.lists(ref, k)
        assert lst.shape == (len(count), k) and ((lst >= 0).sum(axis=1) == np.minimum(count, k)).all()
