"""The yardstick of the signed distance tests (spira_scene_signed_distance_*), composed from the yardsticks of the entries it is made of, imported and not
edited: nearest_support.NearScan for step 1 (the closest-point scan); hits_support.candidates on a cast_support.Scan built from the scene's TRIANGLES
ALONE for the three rays [p, 0, D_j, +Inf] — the oracle's per-object triangle test on every triangle, no sphere; and the rules of steps 2 to 4 restated
here in numpy.  Plus the scenes and point sets of tests/test_sdf_cpu.py and tests/test_gpu_sdf.py, each reference computed once and left unchanged."""
import functools

import numpy as np

import cast_support as S
import hits_support as H
import nearest_support as N
from spira_hip import _binding as B
from spira_hip import query, scenes

MISS, INVALID = S.MISS, S.INVALID
SKIPPED = B.SDF_SKIPPED      # the binding's constant: the yardstick is of this entry and of nothing before it


def rays_of(points3, j):
    """Ray j of every point as a caller would hand it to cast, in Float64: [p, t_min 0, INSIDE_DIRECTIONS[j], t_max +Inf]."""
    p = np.asarray(points3, dtype=np.float64).reshape(-1, 3)
    n = len(p)
    return np.concatenate([p, np.zeros((n, 1)), np.tile(np.asarray(query.INSIDE_DIRECTIONS[j], dtype=np.float64), (n, 1)), np.full((n, 1), np.inf)], axis=1)


def triangles_only(scene):
    return dict(spheres5=np.zeros((0, 5)), materials8=scene["materials8"], triangles10=scene["triangles10"])


def has_triangles(scene):
    tri = scene.get("triangles10")
    return tri is not None and len(tri) > 0


def triangle_counts(scene, prec, points4, frame=None):
    """c_j [n, 3] of every point, every ray counted (0 for an invalid point): the candidates of ray j among the scene's triangles alone."""
    sc = S.Scan(H._oracle(), triangles_only(scene), prec, frame)
    pts = np.asarray(points4, dtype=np.float64)
    out = np.zeros((len(pts), 3), dtype=np.uint32)
    for j in range(3):
        cands, _, _ = H.candidates(sc, rays_of(pts[:, :3], j))
        out[:, j] = [0 if c is None else len(c) for c in cands]
    return out


def in_spheres(scene, T, points3):
    """Step 2: w = p - c, l = sqrt((w.x w.x + w.y w.y) + w.z w.z) in T, inside when l < r as given."""
    sp = np.asarray(scene["spheres5"], dtype=T).reshape(-1, 5)
    p = np.asarray(points3, dtype=T).reshape(-1, 3)
    out = np.zeros(len(p), dtype=bool)
    with np.errstate(all="ignore"):
        for s in sp:
            w = p - s[None, 0:3]
            l = np.sqrt((w[:, 0] * w[:, 0] + w[:, 1] * w[:, 1]) + w[:, 2] * w[:, 2])
            out |= l < s[3]
    return out


def decide(valid, in_sphere, counts, with_mesh):
    """Steps 3 and 4: (inside uint8 [n], crossings uint32 [n, 3]) from every ray's count."""
    n = len(valid)
    cr = np.full((n, 3), SKIPPED, dtype=np.uint32)
    inside = np.array(in_sphere, dtype=bool)
    if with_mesh:
        for i in range(n):
            c0, c1, c2 = (int(x) for x in counts[i])
            if c0 % 2 == c1 % 2:
                cr[i], odd = (c0, c1, SKIPPED), c0 % 2 == 1
            else:
                cr[i], odd = (c0, c1, c2), c2 % 2 == 1
            inside[i] |= odd
    inside &= valid
    cr[~valid] = 0
    return np.where(valid, inside.astype(np.uint8), np.uint8(255)), cr


def reference(scene, prec, points4, frame=None):
    """dict(points, prim, dist, point, inside, crossings, counts, valid, scan): the contract's outputs for points4 (rounded to T first: the values the
    library sees).  frame: as NearScan's and Scan's."""
    T = S.dtype_of(prec)
    ns = N.NearScan(scene, prec, frame)
    points = np.array(np.asarray(points4, dtype=np.float64), dtype=T).astype(np.float64)
    prim, dist, point, valid = ns.query(points)
    with_mesh = has_triangles(scene)
    counts = triangle_counts(scene, prec, points, ns.frame) if with_mesh else np.zeros((len(points), 3), dtype=np.uint32)
    inside, crossings = decide(valid, in_spheres(scene, T, points[:, :3]), counts, with_mesh)
    dist = np.array(dist)
    neg = inside == 1
    dist[neg] = -np.abs(dist[neg])                                   # the sign bit set where the point is inside
    ref = dict(points=points, prim=prim, dist=dist, point=point, inside=inside, crossings=crossings, counts=counts, valid=valid)
    for a in ref.values():
        a.setflags(write=False)
    return dict(ref, scan=ns)


# ------------------------------------------------------------------ scenes
def mesh_only(scene):
    return dict(scene, spheres5=np.zeros((0, 5)))


@functools.lru_cache(maxsize=None)
def ico3_scene():
    """scenes.icosphere(3): 1 280 triangles, a convex closed mesh with a tree, no spheres."""
    v, f = scenes.icosphere(3)
    t = scenes.mesh_triangles10(v, f, 1)
    t.setflags(write=False)
    return dict(spheres5=np.zeros((0, 5)), materials8=np.array([[0.8, 0.8, 0.8, 0, 0, 0, 0.5, 0.0]]), triangles10=t)


def lds_scene():
    """32 triangles of the nested shells (they stay in LDS: no tree) and blob_scene's two spheres."""
    return H.shells_scene(1, n_shells=10, max_tris=32)


def spheres_scene():
    return scenes.scene_s1()


# ------------------------------------------------------------------ point sets ([n, 4] Float64)
def _p4(p, r_max=np.inf):
    return N._p4(p, r_max)


def blob_points(scene, seed=5, n_near=260, n_box=200, n_light=48, n_ground=24, n_r=48):
    """The set of the blob scenes: near the mesh's surface (both sides), uniform in the grown box (in a scene with the ground sphere the part below it is
    inside that sphere), points inside and just outside the light sphere, points under the ground sphere's top, finite r_max on some (misses: r_max copied,
    signed), and nearest_support's invalid kinds interleaved with valid points."""
    rng = np.random.default_rng(seed)
    rows = [N.near_surface(rng, scene, n_near, frac=0.03), N.in_box(rng, scene, n_box)]
    sp = np.asarray(scene["spheres5"], dtype=np.float64).reshape(-1, 5)
    if len(sp):
        light = sp[np.argmin(sp[:, 3])]
        rows.append(_p4(light[:3] + light[3] * rng.uniform(0.0, 1.3, (n_light, 1)) * S._unit(rng, n_light)))
        ground = sp[np.argmax(sp[:, 3])]                             # its top lies under the mesh: points of the box's footprint from just above it to 2 extents down
        lo, hi, c, e = S.target_box(scene)
        g = c + (rng.random((n_ground, 3)) - 0.5) * (hi - lo)
        g[:, 1] = (ground[1] + ground[3]) - e * rng.uniform(-0.02, 2.0, n_ground)
        rows.append(_p4(g))
    ext = S.target_box(scene)[3]
    short = N.in_box(rng, scene, n_r)
    short[:, 3] = ext * 10.0 ** rng.uniform(-2.5, -0.5, n_r)
    rows.append(short)
    return np.concatenate(rows)


def with_invalid(points4, prec, frame):
    """points4 followed by 70 of its own points with every 7th replaced by an invalid kind in turn.  Returns (points, index of the invalid ones)."""
    T = S.dtype_of(prec)
    mixed, at = N.interleave_invalid(points4[:70], T, frame)
    return np.concatenate([points4, mixed]), at + len(points4)


@functools.lru_cache(maxsize=None)
def blob_ref(prec):
    """blob_scene(2): the 320-triangle mesh plus the ground and light spheres."""
    scene = S.blob_scene(2)
    pts, at = with_invalid(blob_points(scene), prec, S.mesh_frame(scene["triangles10"], prec))
    return dict(reference(scene, prec, pts), scene=scene, invalid_at=at)


@functools.lru_cache(maxsize=None)
def lds_ref(prec):
    scene = lds_scene()
    pts, at = with_invalid(blob_points(scene, seed=6, n_near=160, n_box=120, n_light=24, n_ground=12, n_r=24), prec, None)
    return dict(reference(scene, prec, pts), scene=scene, invalid_at=at)


@functools.lru_cache(maxsize=None)
def spheres_ref(prec):
    scene = spheres_scene()
    rng = np.random.default_rng(7)
    sp = np.asarray(scene["spheres5"], dtype=np.float64)
    small = sp[sp[:, 3] < 10]
    pick = small[rng.integers(0, len(small), 160)]
    inner = _p4(pick[:, :3] + pick[:, 3:4] * rng.uniform(0.0, 1.5, (160, 1)) * S._unit(rng, 160))
    box = N.in_box(rng, scene, 200)
    box[-48:, 3] = 10.0 ** rng.uniform(-3.0, -0.5, 48)               # finite r_max: some miss
    pts, at = with_invalid(np.concatenate([box, inner]), prec, None)
    return dict(reference(scene, prec, pts), scene=scene, invalid_at=at)


# (a) the convex mesh with a ground truth
N_CONVEX = 400


@functools.lru_cache(maxsize=None)
def convex_points():
    """400 points about the icosphere's centre c = 0 in a fixed direction set (default_rng(11)): |p - c| <= 0.95 r_in for the first half, >= 1.05 R for the
    second.  r_in: the smallest distance of a face's plane from c, R: the largest vertex radius, both in Float64.  Returns (points4, truth, r_in, R)."""
    tri = np.asarray(ico3_scene()["triangles10"], dtype=np.float64)
    v = tri[:, :9].reshape(-1, 3, 3)
    nrm = np.cross(v[:, 1] - v[:, 0], v[:, 2] - v[:, 0])
    nrm /= np.linalg.norm(nrm, axis=1)[:, None]
    r_in = float(np.abs((nrm * v[:, 0]).sum(axis=1)).min())
    R = float(np.linalg.norm(v.reshape(-1, 3), axis=1).max())
    rng = np.random.default_rng(11)
    u = S._unit(rng, N_CONVEX)
    half = N_CONVEX // 2
    rad = np.concatenate([r_in * rng.uniform(0.0, 0.95, half), R * rng.uniform(1.05, 3.0, N_CONVEX - half)])
    pts = _p4(u * rad[:, None])
    truth = np.arange(N_CONVEX) < half
    pts.setflags(write=False); truth.setflags(write=False)
    return pts, truth, r_in, R


@functools.lru_cache(maxsize=None)
def convex_ref(prec):
    pts, truth, r_in, R = convex_points()
    return dict(reference(ico3_scene(), prec, pts), scene=ico3_scene(), truth=truth, r_in=r_in, R=R)


# (b) the open mesh whose votes disagree
QUAD_SEED, N_QUAD = 3, 300


@functools.lru_cache(maxsize=None)
def quad_ref(prec):
    """cast_support.quad_scene() — 600 triangles, an open mesh — and 300 points uniform in its box (default_rng(QUAD_SEED), chosen once): at least a
    quarter of them have c_0 and c_1 of different parity (ray 2 is walked) and at least a quarter agree (SKIPPED)."""
    scene = S.quad_scene()
    rng = np.random.default_rng(QUAD_SEED)
    return dict(reference(scene, prec, N.in_box(rng, scene, N_QUAD, grow=1.0)), scene=scene)


def vote_split(ref):
    """(points whose first two parities differ, points where they agree) among the valid ones."""
    c = ref["counts"][ref["valid"]].astype(np.int64)
    differ = (c[:, 0] % 2) != (c[:, 1] % 2)
    return int(differ.sum()), int((~differ).sum())


# (c) the Lipschitz property on a closed mesh
N_PAIRS = 300


@functools.lru_cache(maxsize=None)
def lipschitz_scene():
    return mesh_only(S.blob_scene(2))


@functools.lru_cache(maxsize=None)
def lipschitz_points():
    """300 pairs (a, b), |a - b| = 1 % of the extent, a within 1 % of the surface: most pairs straddle the surface or lie next to it.  Rows 2 i and 2 i + 1."""
    scene = lipschitz_scene()
    rng = np.random.default_rng(13)
    ext = S.target_box(scene)[3]
    a = N.near_surface(rng, scene, N_PAIRS, frac=0.01)[:, :3]
    b = a + 0.01 * ext * S._unit(rng, N_PAIRS)
    pts = _p4(H.interleave(a, b))
    pts.setflags(write=False)
    return pts


def lipschitz_tol(scene, prec):
    """Twice the rounding bound csrc/spira_nearest.h derives for a leaf test's q and r, in world units.  The line (header comment, item (d)):
        "rounding of va, vb, vc; r = p - q adds u (64 + A); so sqrt(d2_scan) >= dist(p, triangle) - 6 u (A + 64)."
    in normalised units, A = amax_n the mesh's largest coordinate there, u = 2^-24 (Float32) or 2^-53 (Float64); divided by the frame's scale."""
    centre, scale = S.mesh_frame(scene["triangles10"], prec)
    u = 2.0 ** -24 if prec == "f32" else 2.0 ** -53
    A = float(np.abs(np.asarray(scene["triangles10"], dtype=np.float64)[:, :9]).max()) * scale
    return 2.0 * 6.0 * u * (A + 64.0) / scale


def lipschitz_failures(points4, dist, tol):
    """The pairs with |sd(a) - sd(b)| > |a - b| + tol, in Float64 on the values given."""
    p = np.asarray(points4, dtype=np.float64)[:, :3]
    sd = np.asarray(dist, dtype=np.float64)
    gap = np.linalg.norm(p[0::2] - p[1::2], axis=1)
    return np.flatnonzero(np.abs(sd[0::2] - sd[1::2]) > gap + tol)


@functools.lru_cache(maxsize=None)
def lipschitz_ref(prec):
    scene = lipschitz_scene()
    return dict(reference(scene, prec, lipschitz_points()), scene=scene, tol=lipschitz_tol(scene, prec))


# ------------------------------------------------------------------ placements, updates and rebuilds
@functools.lru_cache(maxsize=None)
def frame_case(prec, fi, how):
    """nearest_support.frame_mesh(prec, fi, how) — the blob scene in placement fi as built, updated or rebuilt — with 200 points about the mesh that
    holds, far ones (60 .. 64 frame units, with their invalid twins) included.  Returns (A, B, reference of B in the frame that holds)."""
    A, B, frame = N.frame_mesh(prec, fi, how)
    ns = N.NearScan(B, prec, frame=frame)
    rng = np.random.default_rng(40 + fi)
    pts = np.concatenate([N.near_surface(rng, B, 90, frac=0.03), N.in_box(rng, B, 70), N.far_points(rng, ns, B, 20)])
    return A, B, reference(B, prec, pts, frame=frame)
