"""The yardstick of the closest-point tests (spira_scene_closest_point_*): the brute-force scan of the contract (include/spira_hip.h, "closest-point
queries") over the numpy twins of spira_hip.query — spheres [0..) then triangles [0..) in the caller's order, best starting at r_max * r_max, object k
taken exactly when d2_k <= best — plus the scenes and the point sets of tests/test_nearest_cpu.py and tests/test_gpu_nearest.py.  Scenes and frames come
from cast_support, read-only."""
import functools

import numpy as np

import cast_support as S
from spira_hip import query, scenes

MISS, INVALID = S.MISS, S.INVALID


class NearScan:
    """The scan over one scene in one precision.  frame: as cast_support.Scan's — the (centre, scale) the validity rule is restated with where it is not
    a fresh build's of this mesh."""

    def __init__(self, scene, prec, frame=None):
        self.prec, self.T = prec, S.dtype_of(prec)
        T = self.T
        self.sp = np.ascontiguousarray(scene["spheres5"], dtype=T).reshape(-1, 5)
        tri = scene.get("triangles10")
        self.tri = np.ascontiguousarray(tri if tri is not None else np.zeros((0, 10)), dtype=T).reshape(-1, 10)
        self.ns = len(self.sp)
        self.frame = frame if frame is not None else S.mesh_frame(tri, prec)
        self.v0 = self.tri[:, 0:3]
        self.e1 = self.tri[:, 3:6] - self.tri[:, 0:3]                # the differences in T: what the LDS records and the tree's records hold
        self.e2 = self.tri[:, 6:9] - self.tri[:, 0:3]

    def d2_all(self, p):
        """q [n, k, 3] and d2 [n, k] of every point against every object, spheres first."""
        qs, ds = [], []
        if self.ns:
            q, d = query.closest_point_sphere(self.sp[None, :, 0:3], self.sp[None, :, 3], p[:, None, :])
            qs.append(q); ds.append(d)
        if len(self.tri):
            q, d = query.closest_point_triangle(self.v0[None], self.e1[None], self.e2[None], p[:, None, :])
            qs.append(q); ds.append(d)
        return np.concatenate(qs, axis=1), np.concatenate(ds, axis=1)

    def query(self, points4, chunk=256):
        """prim int32 [n], dist [n], point [n, 3], valid [n]: the contract (miss: -1, r_max copied, 0; invalid: -3, 0, 0)."""
        T = self.T
        pts, valid = query.prepare_points(points4, T, self.frame)
        n = len(pts)
        prim, dist, point = np.full(n, INVALID, dtype=np.int32), np.zeros(n, dtype=T), np.zeros((n, 3), dtype=T)
        idx = np.flatnonzero(valid)
        with np.errstate(all="ignore"):
            for a in range(0, len(idx), chunk):
                ii = idx[a:a + chunk]
                p, best0 = pts[ii, :3], pts[ii, 3] * pts[ii, 3]
                q, d2 = self.d2_all(p)
                ok = d2 <= best0[:, None]                            # NaN: never
                m = np.where(ok, d2, T(np.inf)).min(axis=1)
                hit = ok.any(axis=1)
                # the last object at the minimal distance: every such object passes d2 <= best when the scan reaches it, and nothing after the last does
                at = ok & (d2 == m[:, None])
                last = d2.shape[1] - 1 - np.argmax(at[:, ::-1], axis=1)
                prim[ii] = np.where(hit, last, MISS)
                dist[ii] = np.where(hit, np.sqrt(m), pts[ii, 3])
                point[ii] = np.where(hit[:, None], q[np.arange(len(ii)), last], T(0))
        return prim, dist, point, valid


# ------------------------------------------------------------------ scenes
@functools.lru_cache(maxsize=None)
def _ico_triangles():
    v, f = scenes.icosphere(1)
    t = scenes.mesh_triangles10(v * 0.7 + np.array([0.2, 0.9, -1.1]), f, 1)
    t.setflags(write=False)
    return t


def ico_scene(n):
    """The first n triangles of the level-1 icosphere (80 triangles, radius 0.7 about (0.2, 0.9, -1.1)) and one sphere: 32 stay in LDS, 33 is the
    smallest tree."""
    return dict(spheres5=np.array([[0.0, -100.5, -1.0, 100.0, 1.0]]), materials8=np.array([[0.8, 0.8, 0.8, 0, 0, 0, 0.5, 0.0]]), triangles10=np.array(_ico_triangles()[:n]))


def _dup():
    d = S.duplicate_scene(S.blob_scene(3), np.random.default_rng(21))[0]
    return dict(d, materials8=np.tile(d["materials8"], (2, 1)))      # duplicate_scene deals materials 1 .. 6


SCENES = {"s1": scenes.scene_s1, "quad": S.quad_scene, "ico32": lambda: ico_scene(32), "ico33": lambda: ico_scene(33), "ico80": lambda: ico_scene(80),
          "s4_3": lambda: S.blob_scene(3), "s4_4": lambda: S.blob_scene(4), "dup": _dup}


@functools.lru_cache(maxsize=None)
def scene(name):
    return SCENES[name]()


# ------------------------------------------------------------------ point sets: [n, 4] Float64, r_max +Inf unless said
def _p4(p, r_max=np.inf):
    p = np.asarray(p, dtype=np.float64).reshape(-1, 3)
    return np.concatenate([p, np.broadcast_to(np.asarray(r_max, dtype=np.float64), (len(p),)).reshape(-1, 1)], axis=1)


def surface_points(rng, sc, n):
    """Points ON the scene's objects in Float64: interior points of triangles drawn at random (a scene without triangles: points on its small spheres)."""
    tri = sc.get("triangles10")
    if tri is not None and len(tri):
        v = np.asarray(tri, dtype=np.float64)[rng.integers(0, len(tri), n), :9].reshape(-1, 3, 3)
        a = rng.uniform(0.05, 0.9, (n, 1)); b = rng.uniform(0.02, 0.95, (n, 1)) * (1 - a)
        return v[:, 0] + a * (v[:, 1] - v[:, 0]) + b * (v[:, 2] - v[:, 0])
    s = np.asarray(sc["spheres5"], dtype=np.float64)
    s = s[s[:, 3] < 10][rng.integers(0, (s[:, 3] < 10).sum(), n)]
    return s[:, :3] + s[:, 3:4] * S._unit(rng, n)


def near_surface(rng, sc, n, frac=0.01):
    """Surface points displaced by up to frac of the extent in a random direction."""
    ext = S.target_box(sc)[3]
    return _p4(surface_points(rng, sc, n) + frac * ext * rng.random((n, 1)) * S._unit(rng, n))


def in_box(rng, sc, n, grow=1.5):
    lo, hi, c, _ = S.target_box(sc)
    return _p4(c + (rng.random((n, 3)) - 0.5) * (hi - lo) * grow)


def centres(sc, T):
    """The box centre of the target and, for a mesh, its vertex mean (the icosphere's centre): everything nearly equidistant.  Rounded to T."""
    lo, hi, c, _ = S.target_box(sc)
    pts = [c]
    tri = sc.get("triangles10")
    if tri is not None and len(tri):
        pts.append(np.asarray(tri, dtype=np.float64)[:, :9].reshape(-1, 3).mean(axis=0))
    return _p4(np.array(pts).astype(T).astype(np.float64))


def on_vertices_and_edges(rng, sc, T, n):
    """Even points: a vertex of the mesh as T holds it; odd points: the midpoint of an edge (of the T-rounded vertices, rounded to T again)."""
    v = S._mesh_vertices(sc, T)
    ti, vi = rng.integers(0, len(v), n), rng.integers(0, 3, n)
    p = np.where((np.arange(n) % 2 == 0)[:, None], v[ti, vi], 0.5 * (v[ti, vi] + v[ti, (vi + 1) % 3]))
    return _p4(p.astype(T).astype(np.float64))


def far_points(rng, ns, sc, n):
    """Valid points at 60 .. 64 frame units (cast_support.rays_far's origins) interleaved with their invalid twins just outside the bound."""
    rays, axis, sign = S.rays_far(rng, ns, sc, n)
    twins = S.rays_far_outside(rays, axis, sign, ns)
    return _p4(np.stack([rays[:, :3], twins[:, :3]], axis=1).reshape(-1, 3))


def invalid_kinds(T, frame):
    """One point per invalidity cause, each otherwise harmless (a frame given: a point near its centre, in its units)."""
    c0 = np.zeros(3) if frame is None else np.asarray(frame[0], dtype=np.float64)
    good = np.concatenate([c0 + np.array([0.1, 1.0, -0.5]) / (1.0 if frame is None else float(frame[1])), [np.inf]])
    kinds = []
    for k, v in ((0, np.nan), (1, np.nan), (2, np.nan), (3, np.nan), (0, np.inf), (1, -np.inf), (2, np.inf), (3, -1e-3), (3, -np.inf)):
        r = good.copy(); r[k] = v; kinds.append(r)
    if frame is not None:
        r = good.copy(); r[0] = float(frame[0][0]) + 65.0 / frame[1]; kinds.append(r)
    return np.array(kinds)


def interleave_invalid(points4, T, frame, every=7):
    """points4 with every `every`-th row replaced by the invalid kinds in turn.  Returns (points, at)."""
    kinds = invalid_kinds(T, frame)
    out = np.array(points4, dtype=np.float64)
    at = np.arange(0, len(out), every)
    out[at] = kinds[np.arange(len(at)) % len(kinds)]
    return out, at


def _freeze(d):
    for a in d.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return d


def build_set(ns, sc, seed=31, n_near=768, n_box=640, n_edge=128, n_far=64, n_r=96):
    """The point set of one scene with the scan's answers, about 2 048 points: near-surface, in the grown box, the centres, vertices and edge
    midpoints, (a tree only) far points with their invalid twins; then for the first n_r triangle-or-sphere winners of the near-surface part the same
    point with r_max = the found distance, r_max = nextafter(that, 0), and r_max = 0 on vertex points; and the invalid kinds interleaved with copies of
    valid points.  dict(points, prim, dist, point, valid, parts) — parts: name -> slice."""
    T = ns.T
    rng = np.random.default_rng(seed)
    parts, rows = {}, []

    def add(name, p):
        a = sum(len(r) for r in rows)
        rows.append(p); parts[name] = slice(a, a + len(p))
    add("near", near_surface(rng, sc, n_near))
    add("box", in_box(rng, sc, n_box))
    add("centres", centres(sc, T))
    has_tri = len(ns.tri) > 0
    if has_tri:
        add("edges", on_vertices_and_edges(rng, sc, T, n_edge))
    if ns.frame is not None:
        add("far", far_points(rng, ns, sc, n_far))
    base = np.array(np.concatenate(rows), dtype=T).astype(np.float64)          # the values the library sees
    prim, dist, _, valid = ns.query(base)
    sel = np.flatnonzero(prim[parts["near"]] >= 0)[:n_r] + parts["near"].start
    same, below = base[sel].copy(), base[sel].copy()
    same[:, 3] = dist[sel]
    below[:, 3] = np.nextafter(dist[sel], T(0))
    rows = [base]
    add("same", same); add("below", below)
    if has_tri:
        zero = base[parts["edges"]].copy(); zero[:, 3] = 0.0
        add("zero", zero)
    mixed, at = interleave_invalid(base[parts["box"]][:140], T, ns.frame)
    add("mixed", mixed)
    points = np.array(np.concatenate(rows), dtype=T).astype(np.float64)
    prim, dist, point, valid = ns.query(points)
    return _freeze(dict(points=points, prim=prim, dist=dist, point=point, valid=valid, parts=parts, sel=sel, invalid_at=at + parts["mixed"].start))


def frame_mesh(prec, fi, how):
    """The blob mesh in placement fi of cast_support.FRAMES; how = create: as built; update: twisted (test_gpu_refit.deform), the validity frame stays the
    creation frame; rebuild: twisted, then scaled by 1.7 and moved, the frame is the fresh build's of that mesh.  Returns (A, B, frame) — frame None: B's own."""
    from test_gpu_refit import deform
    A = S.blob_scene(2, *S.FRAMES[fi])
    if how == "create":
        return A, A, None
    tri = deform(A["triangles10"])
    if how == "rebuild":
        tri = np.array(tri)
        for v in range(3):
            tri[:, 3 * v:3 * v + 3] = tri[:, 3 * v:3 * v + 3] * 1.7 + np.array([0.5, -0.25, 1.0]) * S.FRAMES[fi][0]
    B = dict(A, triangles10=tri)
    return A, B, S.mesh_frame(A["triangles10"], prec) if how == "update" else S.mesh_frame(tri, prec)


@functools.lru_cache(maxsize=None)
def scan_of(name, prec):
    return NearScan(scene(name), prec)


@functools.lru_cache(maxsize=None)
def reference(name, prec):
    return build_set(scan_of(name, prec), scene(name))
