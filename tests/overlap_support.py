"""The yardstick of the box overlap tests (spira_scene_overlap_box_* / spira_scene_overlap_any_*): the brute-force scan of the contract
(csrc/spira_overlap.h) over the numpy twins of spira_hip.query — every object's candidate verdict from overlap_box_sphere / overlap_box_triangle, spheres
[0..) then triangles [0..) in the caller's order; the count of all candidates, the first max_list of them in ascending index — plus the scenes and the box
sets of tests/test_overlap_cpu.py and tests/test_gpu_overlap.py.  Scenes and frames come from nearest_support / cast_support by import, read-only."""
import functools

import numpy as np

import cast_support as S
import nearest_support as N
from spira_hip import query, scenes

MISS, INVALID = S.MISS, S.INVALID
IDENTITY = np.array([0.0, 0.0, 0.0, 1.0])


class OverlapScan(N.NearScan):
    """The scan over one scene in one precision; the fields and the frame are NearScan's."""

    def candidates(self, boxes10, chunk=64):
        """cand bool [n, k] — every box against every object, spheres first; False in the rows of invalid boxes — and valid [n]."""
        b, A, _, valid = query.prepare_boxes(boxes10, self.T, self.frame)
        n, k = len(b), self.ns + len(self.tri)
        cand = np.zeros((n, k), dtype=bool)
        idx = np.flatnonzero(valid)
        for a in range(0, len(idx), chunk):
            ii = idx[a:a + chunk]
            c, h, Ai = b[ii, None, 0:3], b[ii, None, 3:6], A[ii, None]
            if self.ns:
                cand[ii, :self.ns] = query.overlap_box_sphere(self.sp[None, :, 0:3], self.sp[None, :, 3], c, h, Ai)
            if len(self.tri):
                cand[ii, self.ns:] = query.overlap_box_triangle(self.v0[None], self.e1[None], self.e2[None], c, h, Ai)
        return cand, valid

    def overlap(self, boxes10):
        """dict(cand, valid, count uint32 [n], hit uint8 [n]): the contract's count and any form (invalid: 0 and 255)."""
        cand, valid = self.candidates(boxes10)
        count = cand.sum(axis=1).astype(np.uint32)
        return dict(cand=cand, valid=valid, count=count, hit=np.where(valid, count > 0, 255).astype(np.uint8))


def lists(ref, max_list):
    """out_prim [n, max_list] of a scan's answer: the first max_list candidates in ascending index, MISS in unused slots, INVALID for invalid boxes."""
    cand, valid = ref["cand"], ref["valid"]
    n, k = cand.shape
    out = np.full((n, max_list), MISS, dtype=np.int32)
    order = np.where(cand, np.arange(k)[None, :], k)
    order.sort(axis=1)
    head = order[:, :max_list]
    if head.shape[1] < max_list:
        head = np.concatenate([head, np.full((n, max_list - head.shape[1]), k)], axis=1)
    out[head < k] = head[head < k]
    out[~valid] = INVALID
    return out


# ------------------------------------------------------------------ scenes
@functools.lru_cache(maxsize=None)
def torus_scene():
    """A closed mesh of 2 048 triangles — a torus (32 x 32 quads, radii 1 and 0.4, gently bumped) about (0.3, 0.8, -1.2) — and three spheres: one
    through the tube, one inside the tube's hollow, one apart."""
    nu = nv = 32
    u, v = np.meshgrid(np.arange(nu) * (2 * np.pi / nu), np.arange(nv) * (2 * np.pi / nv), indexing="ij")
    r = 0.4 + 0.05 * np.sin(3 * u) * np.cos(2 * v)
    p = np.stack([(1.0 + r * np.cos(v)) * np.cos(u), r * np.sin(v), (1.0 + r * np.cos(v)) * np.sin(u)], axis=-1) + np.array([0.3, 0.8, -1.2])
    vid = lambda i, j: (i % nu) * nv + (j % nv)
    f = []
    for i in range(nu):
        for j in range(nv):
            f.append((vid(i, j), vid(i + 1, j), vid(i + 1, j + 1)))
            f.append((vid(i, j), vid(i + 1, j + 1), vid(i, j + 1)))
    t = scenes.mesh_triangles10(p.reshape(-1, 3), np.array(f), 1)
    sp = np.array([[1.3, 0.8, -1.2, 0.5, 1.0], [-0.7, 0.8, -1.2, 0.2, 2.0], [0.3, 2.2, -1.2, 0.3, 1.0]])
    m = np.array([[0.8, 0.8, 0.8, 0, 0, 0, 0.5, 0.0], [0.7, 0.3, 0.2, 0, 0, 0, 0.2, 0.4], [0.2, 0.3, 0.7, 0, 0, 0, 0.0, 1.0]])      # three: test_gpu_refit.deform deals 1 .. 3
    t.setflags(write=False)
    return dict(spheres5=sp, materials8=m, triangles10=t)


def ico_spheres(n):
    """nearest_support.ico_scene's first n triangles with three (20) or two (33) small spheres in the place of the ground sphere."""
    s = N.ico_scene(n)
    sp = np.array([[0.2, 0.9, -1.1, 0.6, 1.0], [0.9, 0.9, -1.1, 0.25, 1.0], [0.2, 1.9, -1.1, 0.2, 1.0]])
    return dict(s, spheres5=sp[:3 if n <= 32 else 2])


SCENES = {"ico20": lambda: ico_spheres(20), "ico33": lambda: ico_spheres(33), "torus": torus_scene}


@functools.lru_cache(maxsize=None)
def scene(name):
    return SCENES[name]()


# ------------------------------------------------------------------ box sets: [n, 10] Float64
def quats(rng, n):
    """Every fourth the identity, every fourth plus one a quarter turn about an axis, the rest random — none of unit length, so normalisation matters."""
    q = rng.normal(size=(n, 4)) * 2.3
    q[0::4] = IDENTITY
    s = np.sqrt(0.5)
    turn = np.array([[s, 0, 0, s], [0, s, 0, s], [0, 0, s, s]]) * 3.0
    q[1::4] = turn[np.arange(len(q[1::4])) % 3]
    return q


def _boxes(c, h, q):
    return np.concatenate([c, h, q], axis=1)


def at_surface(rng, sc, n, lo=0.005, hi=0.04):
    ext = S.target_box(sc)[3]
    c = N.near_surface(rng, sc, n, frac=0.02)[:, :3]
    return _boxes(c, rng.uniform(lo, hi, (n, 3)) * ext, quats(rng, n))


def containing(rng, sc, n):
    """Boxes that hold the whole target: every object of the mesh is a candidate."""
    _, _, c, ext = S.target_box(sc)
    return _boxes(c + 0.05 * ext * rng.normal(size=(n, 3)), rng.uniform(1.2, 1.6, (n, 3)) * ext, quats(rng, n))


def flat_and_needle(rng, sc, n):
    """Even boxes flat (one half extent of 1e-4 .. 1e-3 of the extent), odd ones needles (two such), the others 0.1 .. 0.6 of it; through the target."""
    lo, hi, c, ext = S.target_box(sc)
    h = rng.uniform(0.1, 0.6, (n, 3)) * ext
    thin = rng.uniform(1e-4, 1e-3, (n, 3)) * ext
    k = rng.integers(0, 3, n)
    flat = np.arange(3)[None, :] == k[:, None]
    mask = np.where((np.arange(n) % 2 == 0)[:, None], flat, ~flat)
    return _boxes(c + (rng.random((n, 3)) - 0.5) * (hi - lo), np.where(mask, thin, h), quats(rng, n))


def zero_extent(rng, sc, T, n):
    """h = 0: points ON the mesh's vertices as T holds them and edge midpoints (a candidate or a rounding away from one), and segments (one axis 0.2 ext)."""
    ext = S.target_box(sc)[3]
    tri = sc.get("triangles10")
    if tri is not None and len(tri):
        c = N.on_vertices_and_edges(rng, sc, T, n)[:, :3]
    else:
        c = N.surface_points(rng, sc, n)
    h = np.zeros((n, 3))
    h[2::3, 0] = 0.2 * ext
    return _boxes(c, h, quats(rng, n))


def extent_bound(ss, quat):
    """The largest uniform half extent h (h, h, h) of T the rule accepts under the quaternion `quat` in the scan's frame, and the next value of T."""
    T = ss.T

    def ok(h):
        b = np.concatenate([np.asarray(ss.frame[0], dtype=np.float64), [h, h, h], quat])[None]
        return bool(query.prepare_boxes(b, T, ss.frame)[3][0])
    h = T(60.0 / float(ss.frame[1]) / np.sqrt(3.0))
    assert ok(h)
    hi = T(65.0 / float(ss.frame[1]))
    assert not ok(hi)
    for _ in range(80):                                              # bisection in T down to neighbouring values
        mid = T((np.float64(h) + np.float64(hi)) / 2)
        if mid == h or mid == hi:
            break
        if ok(mid):
            h = mid
        else:
            hi = mid
    return h, np.nextafter(h, T(np.inf))


def far_boxes(rng, ss, sc, n):
    """Centres at 60 .. 64 frame units (y above), extents just under the bound (even) and just over it (odd: invalid); the valid ones reach the mesh."""
    c0, unit = np.asarray(ss.frame[0], dtype=np.float64), 1.0 / float(ss.frame[1])
    off = rng.uniform(60.0, 64.0, (n, 3)) * np.where(rng.random((n, 3)) < 0.5, -1.0, 1.0)
    off[:, 1] = np.abs(off[:, 1])
    c = (c0 + off * unit).astype(ss.T).astype(np.float64)
    q = quats(rng, n).astype(ss.T).astype(np.float64)
    h = np.zeros((n, 3))
    for i in range(n):
        h_in, h_out = extent_bound(ss, q[i])
        h[i] = float(h_in) if i % 2 == 0 else float(h_out)
    return _boxes(c, h, q)


def far_small(rng, ss, sc, n):
    """Small boxes whose centres are valid at 60 .. 64 units, interleaved with twins whose centre is beyond the origin rule."""
    rays, axis, sign = S.rays_far(rng, ss, sc, n)
    twins = S.rays_far_outside(rays, axis, sign, ss)
    c = np.stack([rays[:, :3], twins[:, :3]], axis=1).reshape(-1, 3)
    ext = S.target_box(sc)[3]
    return _boxes(c, np.full((2 * n, 3), 0.05 * ext), quats(rng, 2 * n))


def invalid_kinds(T, frame):
    """One box per invalidity cause, each otherwise harmless."""
    fi = np.finfo(T)
    c0 = np.zeros(3) if frame is None else np.asarray(frame[0], dtype=np.float64)
    u = 1.0 if frame is None else 1.0 / float(frame[1])
    good = np.concatenate([c0 + np.array([0.1, 0.3, -0.2]) * u, np.array([0.2, 0.1, 0.3]) * u, [0.3, -0.2, 0.1, 0.9]])
    kinds = []
    for k, v in ((0, np.nan), (2, np.nan), (4, np.nan), (7, np.nan), (9, np.nan), (1, np.inf), (3, np.inf), (5, -np.inf), (6, np.inf), (9, -np.inf),
                 (3, -1e-3 * u), (5, -float(fi.tiny))):
        r = good.copy(); r[k] = v; kinds.append(r)
    r = good.copy(); r[6:10] = 0.0; kinds.append(r)                                              # n2 = 0
    r = good.copy(); r[6:10] = [0.0, 0.0, 0.0, float(np.sqrt(np.float64(fi.tiny))) / 4]; kinds.append(r)      # n2 below the smallest normal number
    r = good.copy(); r[6:10] = [0.0, 0.0, 0.0, float(np.sqrt(np.float64(fi.max))) * 2]; kinds.append(r)       # n2 overflows
    if frame is not None:
        r = good.copy(); r[0] = float(c0[0]) + 65.0 * u; kinds.append(r)                         # the origin rule
        r = good.copy(); r[4] = 120.0 * u; kinds.append(r)                                       # the extent rule
    return np.array(kinds)


def interleave_invalid(boxes, T, frame, every=7):
    kinds = invalid_kinds(T, frame)
    out = np.array(boxes, dtype=np.float64)
    at = np.arange(0, len(out), every)
    out[at] = kinds[np.arange(len(at)) % len(kinds)]
    return out, at


def build_set(ss, sc, seed=91, n_surf=1024, n_whole=24, n_thin=384, n_zero=192, n_far=32, n_small=48, n_mixed=140):
    """The box set of one scene with the scan's answers (header of tests/test_gpu_overlap.py).  dict(boxes, cand, valid, count, hit, parts, invalid_at)."""
    T = ss.T
    rng = np.random.default_rng(seed)
    parts, rows = {}, []

    def add(name, b):
        a = sum(len(r) for r in rows)
        rows.append(np.asarray(b, dtype=np.float64)); parts[name] = slice(a, a + len(b))
    add("surface", at_surface(rng, sc, n_surf))
    add("whole", containing(rng, sc, n_whole))
    add("thin", flat_and_needle(rng, sc, n_thin))
    add("zero", zero_extent(rng, sc, T, n_zero))
    if ss.frame is not None:
        add("far", far_boxes(rng, ss, sc, n_far))
        add("small", far_small(rng, ss, sc, n_small))
    mixed, at = interleave_invalid(at_surface(rng, sc, n_mixed, hi=0.2), T, ss.frame)
    add("mixed", mixed)
    with np.errstate(over="ignore"):
        boxes = np.array(np.concatenate(rows), dtype=T).astype(np.float64)          # the values the library sees
    ref = ss.overlap(boxes)
    return N._freeze(dict(ref, boxes=boxes, parts=parts, invalid_at=at + parts["mixed"].start))


# ------------------------------------------------------------------ the sets of the edge tests (test_overlap_edges_cpu.py, test_gpu_overlap_edges.py)
FRAME_SET = dict(n_surf=384, n_whole=8, n_thin=128, n_zero=64, n_far=16, n_small=24, n_mixed=70)


@functools.lru_cache(maxsize=None)
def frame_case(prec, fi, how):
    """nearest_support.frame_mesh — the blob mesh in placement fi of cast_support.FRAMES, as built, after an update, after a rebuild — with a box set of
    718 boxes in the frame that holds.  Returns (A, B, the scan of B, the set)."""
    A, B, frame = N.frame_mesh(prec, fi, how)
    ss = OverlapScan(B, prec, frame=frame)
    return A, B, ss, build_set(ss, B, seed=95 + fi, **FRAME_SET)


def frame_conditions(ref):
    """What a frame case must hold, asserted: the valid / invalid pattern of the far boxes and the small far boxes, boxes with more than 16 candidates,
    valid ones with none, with 1 .. 4 and with 5 .. 16, invalid ones, and a valid far box that touches something.  Returns the counts."""
    v, c = ref["valid"], ref["count"].astype(np.int64)
    far, small = ref["parts"]["far"], ref["parts"]["small"]
    assert v[far][0::2].all() and not v[far][1::2].any() and v[small][0::2].all() and not v[small][1::2].any()
    out = dict(many=int((c > 16).sum()), none=int((v & (c == 0)).sum()), few=int(((c >= 1) & (c <= 4)).sum()), some=int(((c >= 5) & (c <= 16)).sum()),
               invalid=int((~v).sum()), far_touching=int((c[far][0::2] > 0).sum()))
    assert out["many"] >= 32 and out["none"] >= 48 and out["few"] >= 200 and out["some"] >= 100 and out["invalid"] >= 40 and out["far_touching"] >= 1, out
    return out


@functools.lru_cache(maxsize=None)
def deep_set(prec):
    """The blob at level 4 (5 120 triangles, 2 spheres): 8 boxes that contain the whole mesh and 120 boxes at its surface."""
    sc = N.scene("s4_4")
    ss = OverlapScan(sc, prec)
    rng = np.random.default_rng(97)
    boxes = np.array(np.concatenate([containing(rng, sc, 8), at_surface(rng, sc, 120)]), dtype=ss.T).astype(np.float64)
    return ss, N._freeze(dict(ss.overlap(boxes), boxes=boxes, parts=dict(whole=slice(0, 8), surface=slice(8, 128))))


@functools.lru_cache(maxsize=None)
def scan_of(name, prec):
    return OverlapScan(scene(name), prec)


@functools.lru_cache(maxsize=None)
def reference(name, prec):
    return build_set(scan_of(name, prec), scene(name))
