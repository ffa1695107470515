"""CPU: spira_scene_overlap_box_* / spira_scene_overlap_any_* without a device — the library exports the entries and the header and the binding name them;
the functions the kernels call (spira_overlap.h: overlap_prepare, overlap_box_triangle, overlap_box_sphere, overlap_insert) and overlap_check pass
tests/native/overlap_plan.cpp under ASan + UBSan bit for bit against the numpy twins of spira_hip.query; the exported host arithmetic equals the twins; a
table of exact cases (dyadic coordinates, the identity quaternion); the twin is a box-triangle test whatever its formulas (cases built by construction in
Float64: a triangle through a point inside the box is a candidate, a triangle beyond the box's support along any direction is not — nor is one beyond the
ENCLOSING box by half the walk's growth, the lemma the tree walk prunes by); consistency with the point queries; the validity rule; the argument errors
that need no device.

One reading of the issue is settled here: a triangle of exactly zero computed area (a segment) is no candidate, through the box or beside it — the table
lists both under "not candidates", and the containment in the enclosing ball's nearest_k candidates needs it (the point queries never pick such a triangle)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import cast_support as S
import nearest_support as N
import overlap_support as V
from spira_hip import query

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BOX = ["spira_scene_overlap_box_f32", "spira_scene_overlap_box_f64", "spira_scene_overlap_box_device_f32", "spira_scene_overlap_box_device_f64"]
ANY = ["spira_scene_overlap_any_f32", "spira_scene_overlap_any_f64", "spira_scene_overlap_any_device_f32", "spira_scene_overlap_any_device_f64"]
HOST = ["spira_overlap_box_triangle_f32", "spira_overlap_box_triangle_f64", "spira_overlap_box_sphere_f32", "spira_overlap_box_sphere_f64"]


def test_library_header_and_binding_name_the_entries(binding):
    lib = binding.lib()
    hdr = open(os.path.join(ROOT, "include", "spira_hip.h")).read()
    for name in BOX + ANY:
        assert hasattr(lib, name) and name in binding.EXPORTS and re.search(r"^int %s\(const spira_scene \*scene, " % name, hdr, flags=re.M), name
    for name in HOST:
        assert hasattr(lib, name) and name in binding.EXPORTS and re.search(r"^int %s\(const " % name, hdr, flags=re.M), name
    assert "#define SPIRA_ABI_VERSION 3 " in hdr and lib.spira_abi_version() == 3
    assert re.search(r"^#define SPIRA_MAX_OVERLAP\s+16u", hdr, flags=re.M) and binding.MAX_OVERLAP == 16
    for m in ("overlap_box", "overlap_box_device", "overlap_any", "overlap_any_device"):
        assert hasattr(binding.Scene, m), m
    for f in ("prepare_boxes", "box_axes", "overlap_box_triangle", "overlap_box_sphere", "overlap_boxes", "boxes_from_bounds", "voxelize"):
        assert hasattr(query, f), f
    mk = open(os.path.join(ROOT, "julia-spira_amd", "csrc", "Makefile")).read()
    assert "spira_overlap.h" in mk.split("DEPS", 1)[1].split("\n", 1)[0]      # hashed into spira_build_id


def test_kernels_live_in_the_unit_of_their_precision():
    csrc = os.path.join(ROOT, "julia-spira_amd", "csrc")
    objs = {n: os.path.join(csrc, "spira_tu_%s.o" % n) for n in ("main", "f32", "f64mesh")}
    if not all(os.path.exists(o) for o in objs.values()):
        pytest.skip("objects not present (library built elsewhere)")
    syms = {n: subprocess.run(["nm", o], capture_output=True, text=True, check=True).stdout for n, o in objs.items()}
    for kern in ("9k_overlap", "17k_overlap_session"):
        assert len(re.findall(kern + "If", syms["f32"])) > 0 and len(re.findall(kern + "Id", syms["f32"])) == 0, kern
        assert len(re.findall(kern + "Id", syms["main"])) > 0 and len(re.findall(kern + "If", syms["main"])) == 0, kern
        assert len(re.findall(kern + "I[fd]", syms["f64mesh"])) == 0, kern


# ------------------------------------------------------------------ the native program
@pytest.fixture(scope="module")
def overlap_exe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("overlap") / "overlap_plan")
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g", "-O1"]
    subprocess.run(["g++", "-std=c++17", "-ffp-contract=off", os.path.join(ROOT, "tests", "native", "overlap_plan.cpp"), "-o", exe] + san, check=True)
    return exe


def _frames(prec):
    return [None, ((0.0, 0.0, 0.0), 1.0), ((0.5, -2.0, 8.0), 0.25)] + [S.mesh_frame(S.blob_scene(2, *f)["triangles10"], prec) for f in S.FRAMES]


def _box_rows(T, frame, rng):
    """Boxes for the validity rule and the axes: every invalid kind, random quaternions of every size, h = 0, and around the two bounds of a frame."""
    u = 1.0 if frame is None else 1.0 / float(frame[1])
    c0 = np.zeros(3) if frame is None else np.asarray(frame[0], dtype=np.float64)
    n = 96
    q = V.quats(rng, n) * (10.0 ** rng.uniform(-3, 3, (n, 1)))
    b = np.concatenate([c0 + rng.normal(size=(n, 3)) * 20 * u, np.abs(rng.normal(size=(n, 3))) * 20 * u, q], axis=1)
    b[::5, 3:6] = 0.0
    b[1::7, 0:3] = c0 + rng.uniform(63.0, 65.0, (len(b[1::7]), 3)) * u      # about the origin rule
    b[2::7, 3:6] = rng.uniform(30.0, 70.0, (len(b[2::7]), 3)) * u           # about the extent rule
    with np.errstate(over="ignore"):
        return np.concatenate([V.invalid_kinds(T, frame), b]).astype(T)


def _leaf_rows(T, rng, n=400):
    """(v0, e1, e2, box) and (centre, R, box) rows in T: random pairs near each other (about half touch), exact-table cases, a degenerate triangle, h = 0,
    an invalid box, and products that overflow (NaN: never a candidate)."""
    fi = np.finfo(T)
    c = rng.normal(size=(n, 3)) * 3
    box = np.concatenate([c, rng.uniform(0.0, 1.0, (n, 3)), V.quats(rng, n)], axis=1)
    box[::9, 3:6] = 0.0
    v0 = c + rng.normal(size=(n, 3)) * 0.8
    e1, e2 = rng.normal(size=(n, 3)) * rng.uniform(0.01, 3, (n, 1)), rng.normal(size=(n, 3)) * rng.uniform(0.01, 3, (n, 1))
    e2[5::50] = 2 * e1[5::50]                                        # zero area
    tri = np.concatenate([v0, e1, e2, box], axis=1)
    big = float(np.sqrt(np.float64(fi.max))) * 4
    tri[7, 3:9] = [big, 0, 0, 0, big, 0]                             # products overflow
    tri[11, 9 + 3] = -1.0                                            # an invalid box
    sph = np.concatenate([c + rng.normal(size=(n, 3)), rng.uniform(0.0, 2.5, (n, 1)), box], axis=1)
    sph[13, 3] = big * big if T is np.float64 else big
    sph[11, 4 + 6:4 + 10] = 0.0                                      # an invalid box
    with np.errstate(over="ignore"):
        return tri.astype(T), sph.astype(T)


def _twin_leaf(rows, T, sphere):
    """The twins on harness rows: 1, 0, or -3 where the box is invalid without a frame."""
    k = 4 if sphere else 9
    b, A, _, valid = query.prepare_boxes(rows[:, k:], T)
    if sphere:
        hit = query.overlap_box_sphere(rows[:, 0:3], rows[:, 3], b[:, 0:3], b[:, 3:6], A)
    else:
        hit = query.overlap_box_triangle(rows[:, 0:3], rows[:, 3:6], rows[:, 6:9], b[:, 0:3], b[:, 3:6], A)
    return np.where(valid, hit.astype(np.int64), -3)


@pytest.mark.parametrize("prec", ["f32", "f64"])
@pytest.mark.parametrize("fi", range(7))
def test_the_kernels_functions_under_asan_ubsan_equal_the_twins(overlap_exe, prec, fi):
    T = S.dtype_of(prec)
    U = np.uint32 if prec == "f32" else np.uint64
    frame = _frames(prec)[fi]
    rng = np.random.default_rng(100 + fi)
    boxes = _box_rows(T, frame, rng)
    tri, sph = _leaf_rows(T, rng)
    if fi > 0:
        tri, sph = tri[:16], sph[:16]            # the leaf arithmetic does not depend on the frame: once in full is enough
    head = "%s %d %r %r %r %r\n" % ((prec, 1) + tuple(float(x) for x in frame[0]) + (float(frame[1]),)) if frame else "%s 0 0 0 0 1\n" % prec
    hexrow = lambda row: " ".join("%x" % int(w) for w in np.ascontiguousarray(row).view(U))
    body = "".join("P " + hexrow(r) + "\n" for r in boxes) + "".join("T " + hexrow(r) + "\n" for r in tri) + "".join("S " + hexrow(r) + "\n" for r in sph)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([overlap_exe], input=head + body, capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0 and "all checks passed" in r.stdout and "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stdout[-2000:] + r.stderr[-4000:]
    assert "%d lines answered" % (len(boxes) + len(tri) + len(sph)) in r.stdout
    # ---- prepare: the verdict with and without the frame, the axes and the enclosing half extents bit for bit
    rows = re.findall(r"^bx (\d) (\d)((?: [0-9a-f]+){12})$", r.stdout, flags=re.M)
    assert len(rows) == len(boxes)
    g_with, g_without = np.array([int(g[0]) for g in rows], dtype=bool), np.array([int(g[1]) for g in rows], dtype=bool)
    got = np.array([[int(x, 16) for x in g[2].split()] for g in rows], dtype=U)
    _, A, He, v_with = query.prepare_boxes(boxes, T, frame)
    _, _, _, v_without = query.prepare_boxes(boxes, T)
    assert np.array_equal(g_with, v_with) and np.array_equal(g_without, v_without), (np.flatnonzero(g_with != v_with), np.flatnonzero(g_without != v_without))
    n_inv = len(V.invalid_kinds(T, frame))
    assert not v_with[:n_inv].any() and v_with[n_inv:].sum() > 20 and (~v_with[n_inv:]).sum() > (10 if frame else -1)
    want = np.concatenate([A.reshape(-1, 9), He], axis=1).astype(T)
    want = np.where(v_without[:, None], want, T(0))
    assert np.array_equal(got, np.ascontiguousarray(want).view(U)), np.flatnonzero((got != np.ascontiguousarray(want).view(U)).any(axis=1))
    # ---- the two leaf functions
    g_tri = np.array([int(x) for x in re.findall(r"^tri (-?\d)$", r.stdout, flags=re.M)])
    g_sph = np.array([int(x) for x in re.findall(r"^sph (-?\d)$", r.stdout, flags=re.M)])
    w_tri, w_sph = _twin_leaf(tri, T, False), _twin_leaf(sph, T, True)
    assert np.array_equal(g_tri, w_tri), np.flatnonzero(g_tri != w_tri)
    assert np.array_equal(g_sph, w_sph), np.flatnonzero(g_sph != w_sph)
    if fi == 0:
        assert (w_tri == 1).sum() > 60 and (w_tri == 0).sum() > 60 and (w_sph == 1).sum() > 60 and (w_sph == 0).sum() > 60
        assert w_tri[11] == -3 and w_sph[11] == -3 and w_tri[7] == 0 and (w_tri[5::50] == 0).all()


@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_the_exported_host_functions_equal_the_twins(binding, prec):
    T = S.dtype_of(prec)
    tri, sph = _leaf_rows(T, np.random.default_rng(7), n=200)
    w_tri, w_sph = _twin_leaf(tri, T, False), _twin_leaf(sph, T, True)
    g_tri = np.array([binding.overlap_box_triangle(r[0:3], r[3:6], r[6:9], r[9:], prec) for r in tri])
    g_sph = np.array([binding.overlap_box_sphere(r[0:3], r[3], r[4:], prec) for r in sph])
    assert np.array_equal(g_tri, w_tri) and np.array_equal(g_sph, w_sph)
    assert set(w_tri) == {-3, 0, 1} and set(w_sph) == {-3, 0, 1} and binding.RAY_INVALID == -3


def test_the_identity_quaternion_gives_the_unit_axes_exactly():
    for T in (np.float32, np.float64):
        for s in (1.0, 3.0, 0.125, 1e-3, 7e5):
            A, n2 = query.box_axes(np.array([0, 0, 0, s], dtype=T))
            assert np.array_equal(A, np.eye(3, dtype=T)) and n2 == T(s) * T(s)
        A, _ = query.box_axes(np.array([0, 0, 3.0, 3.0], dtype=T))          # a quarter turn about z: a signed permutation up to one rounding
        assert np.abs(A - np.array([[0, 1, 0], [-1, 0, 0], [0, 0, 1]])).max() <= 2 * np.finfo(T).eps


# ------------------------------------------------------------------ the exact table (dyadic coordinates, the identity quaternion: every operation is exact)
BOX_C, BOX_H = np.array([0.5, -1.0, 2.0]), np.array([1.0, 0.5, 0.25])
K_ = np.array([1.0, 0.5, 0.25])                                      # the corner (+, +, +), relative to the centre
# (name, three vertices relative to the box centre, candidate?)
TABLE = [
    ("in the face plane x = +h", [(1, -0.25, -0.125), (1, 0.25, -0.125), (1, 0, 0.125)], True),
    ("in the face plane, larger than the face", [(1, -4, -4), (1, 4, -4), (1, 0, 4)], True),
    ("in the face plane z = -h", [(-0.5, 0, -0.25), (0.5, 0, -0.25), (0, 0.25, -0.25)], True),
    ("one vertex on an edge, the rest outside", [(1, 0.5, 0), (2, 0.5, 0.5), (1, 1.5, -0.5)], True),
    ("an edge of the triangle crosses an edge of the box", [(0.5, 1, 0), (1.5, 0, 0), (2, 2, 0)], True),
    ("one vertex on a corner", [K_, K_ + (1, 0, 0), K_ + (0, 1, 1)], True),
    ("the plane touches a corner inside the triangle", [K_ + (-2, -1, 1), K_ + (4, -4, 1), K_ + (-2, 5, -2)], True),
    ("the box inside the triangle's interior, plane z = 0", [(-10, -10, 0), (10, -10, 0), (0, 10, 0)], True),
    ("encloses the box, no vertex inside, tilted", [(-16, 8, 8), (8, -16, 8), (8, 8, -16)], True),
    ("a vertex inside", [(0, 0, 0), (3, 0, 0), (0, 3, 0)], True),
    ("separated only by the face normal", [K_ + (0.5, 0, 0) + (-2, -1, 1), K_ + (0.5, 0, 0) + (4, -4, 1), K_ + (0.5, 0, 0) + (-2, 5, -2)], False),
    ("separated only by cross axes", [(2.25, -0.5, 0), (0.25, 1.5, 0), (1.375, 1.375, -0.75)], False),
    ("beyond a face by a quarter", [(1.25, -0.25, -0.125), (1.25, 0.25, -0.125), (1.25, 0, 0.125)], False),
    ("a segment through the box (zero area)", [(-2, 0, 0), (2, 0, 0), (0, 0, 0)], False),
    ("a segment beside the box (zero area)", [(-2, 2, 0), (2, 2, 0), (0, 2, 0)], False),
    ("a point inside the box (zero area)", [(0, 0, 0), (0, 0, 0), (0, 0, 0)], False),
]
# (name, centre relative to the box centre, R, candidate?): a shell
BALLS = [
    ("encloses the whole box", (0, 0, 0), 4.0, False),
    ("inside the box", (0, 0, 0), 0.125, True),
    ("tangent to a face from outside", (2, 0, 0), 1.0, True),
    ("just short of a face", (2.5, 0, 0), 1.0, False),
    ("tangent from inside: through the farthest corners", (0, 0, 0), float(np.sqrt(1 + 0.25 + 0.0625)), True),
    ("through the farthest corner of an off-centre ball (3, 4, 12 -> 13)", (2, 3.5, 11.75), 13.0, True),
    ("touches the nearest corner (3, 4, 12 -> 13)", (4, 4.5, 12.25), 13.0, True),
    ("crosses a face", (1.5, 0, 0), 1.0, True),
    ("R = 0 inside the box", (0.5, 0.25, 0), 0.0, True),
    ("R = 0 outside", (1.5, 0.25, 0), 0.0, False),
]


def _axes13(v, h):
    """The 13 axis verdicts (True: overlaps) of the triangle v [3, 3] (relative to the centre) against the axis-aligned box h, Float64, written
    independently of the twin: projections of the three vertices on each axis against the box's radius."""
    e = [v[1] - v[0], v[2] - v[1], v[0] - v[2]]
    axes = [np.eye(3)[k] for k in range(3)] + [np.cross(e[0], e[1])] + [np.cross(np.eye(3)[i], ej) for i in range(3) for ej in e]
    out = []
    for a in axes:
        p, r = v @ a, np.abs(a) @ h
        out.append(bool(p.min() <= r and p.max() >= -r))
    return out


@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_the_exact_table(binding, prec):
    T = S.dtype_of(prec)
    for shift in (np.zeros(3), np.array([8.0, -16.0, 4.0])):
        box = np.concatenate([BOX_C + shift, BOX_H, V.IDENTITY]).astype(T)
        b, A, _, valid = query.prepare_boxes(box[None], T)
        assert valid[0]
        for name, verts, want in TABLE:
            v = (np.array(verts, dtype=np.float64) + BOX_C + shift).astype(T)
            assert np.array_equal(v.astype(np.float64), np.array(verts) + BOX_C + shift), name          # dyadic: exact in T
            for order in ((0, 1, 2), (1, 2, 0), (2, 0, 1), (0, 2, 1)):
                v0, e1, e2 = v[order[0]], v[order[1]] - v[order[0]], v[order[2]] - v[order[0]]
                got = bool(query.overlap_box_triangle(v0, e1, e2, b[0, 0:3], b[0, 3:6], A[0]))
                assert got == want, (name, order)
                assert binding.overlap_box_triangle(v0, e1, e2, box, prec) == int(want), (name, order)
        for name, c, R, want in BALLS:
            cc = (np.array(c) + BOX_C + shift).astype(T)
            assert bool(query.overlap_box_sphere(cc, T(R), b[0, 0:3], b[0, 3:6], A[0])) == want, name
            assert binding.overlap_box_sphere(cc, R, box, prec) == int(want), name
    # the two separations are what their names say, by an independent evaluation of the 13 axes
    by_name = {name: np.array(verts, dtype=np.float64) for name, verts, _ in TABLE}
    ax = _axes13(by_name["separated only by the face normal"], BOX_H)
    assert ax[:3] == [True] * 3 and not ax[3] and all(ax[4:])
    ax = _axes13(by_name["separated only by cross axes"], BOX_H)
    assert all(ax[:4]) and not all(ax[4:])
    assert all(_axes13(by_name["a segment through the box (zero area)"], BOX_H))          # the axes alone would pass it: the zero-area rule decides


# ------------------------------------------------------------------ the algorithm, independent of the formulas
def _rotations(q):
    """Float64 rotation matrices (rows: the box axes) of quaternions, by the textbook formula on the normalised quaternion."""
    q = q / np.linalg.norm(q, axis=1)[:, None]
    x, y, z, w = q.T
    return np.stack([np.stack([1 - 2 * (y * y + z * z), 2 * (x * y + z * w), 2 * (x * z - y * w)], axis=-1),
                     np.stack([2 * (x * y - z * w), 1 - 2 * (x * x + z * z), 2 * (y * z + x * w)], axis=-1),
                     np.stack([2 * (x * z + y * w), 2 * (y * z - x * w), 1 - 2 * (x * x + y * y)], axis=-1)], axis=-2)


def _case_quats(rng, n, aligned):
    q = rng.normal(size=(n, 4))
    q[0::4] = V.IDENTITY
    if aligned:                                                      # the identity and quarter turns alone: edges exactly parallel to box axes stay so
        s = np.sqrt(0.5)
        turns = np.array([[0, 0, 0, 1.0], [s, 0, 0, s], [0, s, 0, s], [0, 0, s, s]])
        q = turns[np.arange(n) % 4]
    return q


def _verdict(T, c, h, q, V0, V1, V2):
    box = np.concatenate([c, h, q], axis=1).astype(T)
    b, A, _, valid = query.prepare_boxes(box, T)
    assert valid.all()
    v0, v1, v2 = V0.astype(T), V1.astype(T), V2.astype(T)
    return query.overlap_box_triangle(v0, v1 - v0, v2 - v0, b[:, 0:3], b[:, 3:6], A)


def _edges(rng, n, R, aligned):
    """Two edge vectors of sizes 0.01 .. 3: random, or (aligned) each exactly along a box axis — a grid-aligned mesh's."""
    s1, s2 = 10.0 ** rng.uniform(-2, np.log10(3.0), (n, 1)), 10.0 ** rng.uniform(-2, np.log10(3.0), (n, 1))
    if not aligned:
        return S._unit(rng, n) * s1, S._unit(rng, n) * s2
    i = rng.integers(0, 3, n)
    j = (i + 1 + rng.integers(0, 2, n)) % 3
    sign = np.where(rng.random((n, 2)) < 0.5, -1.0, 1.0)
    return R[np.arange(n), i] * s1 * sign[:, 0:1], R[np.arange(n), j] * s2 * sign[:, 1:2]


N_CASES = 100_000


@pytest.mark.parametrize("aligned", [False, True])
@pytest.mark.parametrize("off", [0.0, 60.0])
def test_by_construction_inside_is_a_candidate_and_beyond_the_support_is_not(off, aligned):
    """(a) a triangle that contains, with barycentric weights >= 0.05, a point at least `gap` inside the box is a candidate; (b) a triangle wholly beyond
    the box's support along a random unit direction by at least `gap` is not — the completeness of the 13 axes.  gap = 1e-3 (1 + off / 16); centres offset
    by `off` per coordinate, h in [0.01, 1], triangle sizes 0.01 .. 3, every fourth box the identity quaternion.  aligned: the identity and quarter turns
    with edges exactly along box axes.  Both precisions, no case left out, none may fail."""
    rng = np.random.default_rng(int(off) + (1000 if aligned else 0))
    n = N_CASES
    gap = 1e-3 * (1 + off / 16)
    c = off + rng.uniform(-1, 1, (n, 3))
    h = rng.uniform(0.01, 1.0, (n, 3))
    q = _case_quats(rng, n, aligned)
    R = _rotations(q)
    # (a)
    p = rng.uniform(-1, 1, (n, 3)) * (h - gap)
    P = c + np.einsum("nk,nkj->nj", p, R)
    w = 0.05 + 0.85 * rng.dirichlet(np.ones(3), n)
    a, b = _edges(rng, n, R, aligned)
    V0 = P - (w[:, 1:2] * a + w[:, 2:3] * b)
    for T in (np.float32, np.float64):
        ok = _verdict(T, c, h, q, V0, V0 + a, V0 + b)
        assert ok.all(), (T.__name__, "inside", (~ok).sum(), np.flatnonzero(~ok)[:5])
    # (b)
    nrm = S._unit(rng, n)
    if aligned:
        nrm[::3] = R[::3, 0]                                         # along a box axis too
    sup = (np.abs(np.einsum("nkj,nj->nk", R, nrm)) * h).sum(axis=1)
    a, b = _edges(rng, n, R, aligned)
    X = c + nrm * sup[:, None] + np.cross(nrm, S._unit(rng, n)) * rng.uniform(0, 1.5, (n, 1))
    verts = np.stack([X, X + a, X + b], axis=1)
    low = np.einsum("nvj,nj->nv", verts - c[:, None, :], nrm).min(axis=1)
    verts += nrm[:, None, :] * ((sup + gap * rng.choice([1.0, 1.0, 3.0], n)) - low)[:, None, None]
    for T in (np.float32, np.float64):
        ok = _verdict(T, c, h, q, verts[:, 0], verts[:, 1], verts[:, 2])
        assert not ok.any(), (T.__name__, "beyond", ok.sum(), np.flatnonzero(ok)[:5])


@pytest.mark.parametrize("case", ["near", "far", "corner"])
def test_beyond_the_enclosing_box_by_half_the_growth_is_not_a_candidate(case):
    """The lemma the walk prunes by (spira_overlap.h, "Why the growth suffices"): in a frame (centre 0, scale 1) a triangle beyond the box's ENCLOSING
    axis-aligned box c +- He by 2^-13 (M + 1) along a world axis, M = max_k (|c_k| + He_k) — half of what the walk grows the enclosing box by — is
    rejected by the SAT in T.  near: centres within 1, h to 1; far: centres at 60; corner: centres at 62 .. 64 with enclosing extents up to the bound."""
    rng = np.random.default_rng({"near": 5, "far": 6, "corner": 7}[case])
    n = N_CASES
    off, hmax = {"near": (0.0, 1.0), "far": (60.0, 1.0), "corner": (63.0, 36.0)}[case]
    c = (off + rng.uniform(-1, 1, (n, 3))) * np.where(rng.random((n, 3)) < 0.5, -1.0, 1.0)
    h = rng.uniform(0.01, hmax, (n, 3))
    q = _case_quats(rng, n, False)
    q[1::4] = np.array([0, 0, np.sqrt(0.5), np.sqrt(0.5)])
    R = _rotations(q)
    He = np.einsum("nk,nkj->nj", h, np.abs(R))
    assert (np.abs(c) <= 64).all() and (He <= 64).all()
    M = (np.abs(c) + He).max(axis=1)
    gap = 2.0 ** -13 * (M + 1)
    k = rng.integers(0, 3, n)
    side = np.where(rng.random(n) < 0.5, -1.0, 1.0)
    axis = np.eye(3)[k] * side[:, None]
    size = hmax * 3
    a, b = S._unit(rng, n) * 10.0 ** rng.uniform(-2, np.log10(size), (n, 1)), S._unit(rng, n) * 10.0 ** rng.uniform(-2, np.log10(size), (n, 1))
    X = c + rng.uniform(-1.2, 1.2, (n, 3)) * He
    verts = np.stack([X, X + a, X + b], axis=1)
    low = np.einsum("nvj,nj->nv", verts - c[:, None, :], axis).min(axis=1)
    verts += axis[:, None, :] * ((He[np.arange(n), k] + gap) - low)[:, None, None]
    for T in (np.float32, np.float64):
        ok = _verdict(T, c, h, q, verts[:, 0], verts[:, 1], verts[:, 2])
        assert not ok.any(), (T.__name__, ok.sum(), np.flatnonzero(ok)[:5])


# ------------------------------------------------------------------ consistency with the point queries
def test_candidates_lie_between_those_of_the_inscribed_and_the_enclosing_ball():
    """Float64 twins, 500 triangles of the torus and its 3 spheres: the candidates of a box are among the nearest_k candidates (d2 <= r r) of its enclosing
    ball (c, |h| (1 + 1e-9)) and include those of its inscribed ball (c, min_k h_k (1 - 1e-9))."""
    sc = V.scene("torus")
    sc = dict(sc, triangles10=np.array(sc["triangles10"][:500]))
    ss = V.OverlapScan(sc, "f64", frame=None)
    ss.frame = None
    rng = np.random.default_rng(17)
    n = 600
    ext = S.target_box(sc)[3]
    c = np.concatenate([N.near_surface(rng, sc, n // 2, frac=0.05)[:, :3], N.in_box(rng, sc, n - n // 2)[:, :3]])
    h = rng.uniform(0.01, 0.3, (n, 3)) * ext
    boxes = np.concatenate([c, h, V.quats(rng, n)], axis=1)
    cand, valid = ss.candidates(boxes)
    assert valid.all()
    _, d2 = ss.d2_all(c)
    r_out = np.sqrt((h * h).sum(axis=1)) * (1 + 1e-9)
    r_in = h.min(axis=1) * (1 - 1e-9)
    outer, inner = d2 <= (r_out * r_out)[:, None], d2 <= (r_in * r_in)[:, None]
    assert not (cand & ~outer).any() and not (inner & ~cand).any()
    assert cand.sum() > 2000 and (outer & ~cand).sum() > 500 and (cand & ~inner).sum() > 500 and inner[:, :3].any() and cand[:, :3].sum() > 20


# ------------------------------------------------------------------ validity and errors
@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_validity(binding, prec):
    T = S.dtype_of(prec)
    for frame in (None, ((0.5, -2.0, 8.0), 0.25)):
        kinds = V.invalid_kinds(T, frame)
        _, _, _, valid = query.prepare_boxes(kinds, T, frame)
        assert not valid.any(), np.flatnonzero(valid)
        good = kinds[0].copy(); good[0] = kinds[1][0]
        assert query.prepare_boxes(good[None], T, frame)[3][0]
        zero = good.copy(); zero[3:6] = 0.0
        assert query.prepare_boxes(zero[None], T, frame)[3][0]                       # h = 0: a point
        n_plain = len(V.invalid_kinds(T, None))
        for k in kinds[:n_plain]:                                                   # invalid without a frame: the host functions say so
            assert binding.overlap_box_triangle([0, 0, 0], [1, 0, 0], [0, 1, 0], k, prec) == -3
            assert binding.overlap_box_sphere([0, 0, 0], 1.0, k, prec) == -3
    # the extent bound at, just under and just over 64, for the identity and a rotated box
    ss = V.scan_of("ico33", prec)
    scale = T(ss.frame[1])
    for quat in (V.IDENTITY, np.array([0.3, -0.5, 0.2, 0.7])):
        h_in, h_out = V.extent_bound(ss, quat)
        He = lambda hh: query.prepare_boxes(np.concatenate([ss.frame[0], [hh] * 3, quat])[None], T, ss.frame)[2][0]
        assert (He(h_in) * scale <= T(64)).all() and (He(h_out) * scale > T(64)).any() and h_out == np.nextafter(h_in, T(np.inf))
        assert (He(np.nextafter(h_in, T(0))) * scale <= T(64)).all()
    h_at = T(64.0) / scale                                                           # the identity: He = h exactly, 64 itself is valid
    at = np.concatenate([ss.frame[0], [h_at] * 3, V.IDENTITY])[None]
    assert query.prepare_boxes(at, T, ss.frame)[3][0]
    over = at.copy(); over[0, 4] = np.nextafter(h_at, T(np.inf))
    assert not query.prepare_boxes(over, T, ss.frame)[3][0] and query.prepare_boxes(over, T)[3][0]


def test_return_codes_without_a_device(binding):
    """Every argument error of the entries is decided before any device is touched: it returns its own code, not SPIRA_E_NO_DEVICE (-2)."""
    lib = binding.lib()
    boxes = np.zeros((4, 10), dtype=np.float64)
    bp, out = boxes.ctypes.data_as(C.c_void_p), np.zeros(256, dtype=np.float64).ctypes.data_as(C.c_void_p)
    u32 = C.c_uint32
    for name in BOX:
        fn = getattr(lib, name)
        tail = (None,) if "device" in name else ()

        def call(scene, b, n, k, flags, outs):
            return fn(scene, b, u32(n), u32(k), u32(flags), *(outs + tail))
        outs, none = (out, out, None), (None, None, out)                              # trips alone is no output
        assert call(None, None, 4, 4, 0, outs) == -1 and b"box array is NULL" in lib.spira_last_error(), name
        assert call(None, bp, 0, 4, 0, outs) == -1 and b"n is 0" in lib.spira_last_error(), name
        assert call(None, bp, 4, 4, 2, outs) == -1 and b"unknown flag bits" in lib.spira_last_error(), name
        assert call(None, bp, 4, 4, 0x80000001, outs) == -1, name
        assert call(None, bp, 4, 17, 0, outs) == -1 and b"SPIRA_MAX_OVERLAP" in lib.spira_last_error(), name
        assert call(None, bp, 4, 4, 0, none) == -1 and b"every output is NULL" in lib.spira_last_error(), name
        assert call(None, bp, 4, 0, 0, (out, None, None)) == -1 and b"out_count is NULL" in lib.spira_last_error(), name      # count only needs the count
        assert call(None, bp, (1 << 26) + 1, 0, 0, outs) == -4 and b"SPIRA_MAX_RAYS" in lib.spira_last_error(), name
        assert call(None, bp, (1 << 22) + 1, 16, 0, outs) == -4 and b"n * max_list" in lib.spira_last_error(), name
        for k in (0, 1, 16):
            assert call(None, bp, 4, k, 0, outs) == -1 and b"scene handle is NULL or was destroyed" in lib.spira_last_error(), (name, k)
        assert call(None, bp, 4, 4, 1, outs) == -1 and b"scene handle is NULL" in lib.spira_last_error(), name
    for name in ANY:
        fn = getattr(lib, name)
        tail = (None,) if "device" in name else ()

        def call(scene, b, n, flags, hit):
            return fn(scene, b, u32(n), u32(flags), hit, *tail)
        assert call(None, None, 4, 0, out) == -1 and b"box array is NULL" in lib.spira_last_error(), name
        assert call(None, bp, 0, 0, out) == -1 and b"n is 0" in lib.spira_last_error(), name
        assert call(None, bp, 4, 2, out) == -1 and b"unknown flag bits" in lib.spira_last_error(), name
        assert call(None, bp, 4, 0, None) == -1 and b"NULL" in lib.spira_last_error(), name
        assert call(None, bp, (1 << 26) + 1, 0, out) == -4 and b"SPIRA_MAX_RAYS" in lib.spira_last_error(), name
        assert call(None, bp, 4, 0, out) == -1 and b"scene handle is NULL or was destroyed" in lib.spira_last_error(), name


def test_helpers_and_the_box_sets_reach_what_they_are_for():
    lo, hi = np.array([[0.0, 1.0, 2.0], [-1.0, -1.0, -1.0]]), np.array([[1.0, 3.0, 2.5], [1.0, 1.0, 1.0]])
    b = query.boxes_from_bounds(lo, hi)
    assert np.array_equal(b, [[0.5, 2.0, 2.25, 0.5, 1.0, 0.25, 0, 0, 0, 1], [0, 0, 0, 1, 1, 1, 0, 0, 0, 1]])
    vb = query.voxel_boxes([0, 0, 0], [1, 2, 4], (2, 2, 4), np.float32)
    assert vb.shape == (16, 10) and np.array_equal(vb[0], [0.25, 0.5, 0.5, 0.25, 0.5, 0.5, 0, 0, 0, 1]) and np.array_equal(vb[1, :3], [0.25, 0.5, 1.5])
    for name in ("ico20", "ico33"):
        ref, ss = V.reference(name, "f32"), V.scan_of(name, "f32")
        parts, count = ref["parts"], ref["count"]
        assert (ss.frame is None) == (name == "ico20")
        assert (count[parts["whole"]] >= len(ss.tri)).all()                           # every triangle a candidate
        assert (count[parts["surface"]] > 0).mean() > 0.5 and (count[parts["surface"]] == 0).any()
        assert (count[parts["zero"]] > 0).any() and (count[parts["thin"]] > 0).any()
        assert (ref["hit"][ref["invalid_at"]] == 255).all() and ref["valid"][ref["invalid_at"][:-1] + 1].all()
        if ss.frame is not None:
            far = ref["valid"][parts["far"]]
            assert far[0::2].all() and not far[1::2].any() and (count[parts["far"]][0::2] > 16).any()
            small = ref["valid"][parts["small"]]
            assert small[0::2].all() and not small[1::2].any()
        for k in (1, 4, 5, 16):
            lst = V.lists(ref, k)
            assert lst.shape == (len(count), k) and ((lst >= 0).sum(axis=1) == np.minimum(count, k)).all()
            assert ((np.diff(lst, axis=1) > 0) | (lst[:, 1:] < 0)).all()               # ascending, the unused slots behind
