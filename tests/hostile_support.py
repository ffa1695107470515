"""Hostile meshes for the list queries of a scene handle, with their item sets and the yardsticks' answers (no test lives here): shared by
tests/test_hostile_meshes_cpu.py, which asserts from the yardsticks alone what the sets reach, and tests/test_gpu_hostile_meshes.py, which runs them on
the device.  Every mesh is a legal input (triangles_check accepts any finite triangle) that the nice meshes of the per-query tests never give a walk:
child boxes that quantise to lo == hi, no extent on one axis, leaves that hold a point or a segment, internal boxes that all cover the whole frame, a tree
twice as deep as the blob's, all Morton keys equal.

The meshes are deterministic Float64 triangles10 arrays of 96 .. 200 triangles (above the 32-triangle LDS limit: each has a tree) in the unit box about
(0, 0, -1), materials 1 .. 3, each in a scene with nearest_support.ico_scene's ground sphere so that the scans mix spheres and triangles.  No mesh has zero
extent on every axis.

The sets are the existing builders' (sweep_support, overlap_support, nearest_support, cast_support, hits_support, sdf_support, imported and not edited
beyond sweep_support.grazing's draw) with reduced counts — invalid kinds interleaved, far items at 60 .. 64 frame units with their invalid twins — plus a
targeted part per mesh (targets): items at, near and aimed at the features that make the mesh hostile.  Everything is computed once per
(mesh, precision, frame) and left unchanged; create and rebuild share a set, since both hold the target mesh in its own fresh frame."""
import functools

import numpy as np

import cast_support as S
import hits_support as H
import knearest_support as KS
import nearest_support as N
import overlap_support as V
import sdf_support as D
import sweep_support as W

MISS, INVALID = S.MISS, S.INVALID
CENTRE = np.array([0.0, 0.0, -1.0])
LO = CENTRE - 0.5
MESHES = ("zero_area", "mixed_scales", "needles", "flat", "copies", "geometric")      # create and rebuild
UPDATES = ("zero_area", "mixed_scales", "geometric", "scrambled")                     # update
N_CLUSTERS = 40                                                                        # geometric: clusters of 4 triangles, cluster k at scale 2^-k
CLUSTER_AT = LO + 0.1                                                                  # mixed_scales: the corner the tiny cluster sits at
CLUSTER_SHRINK = 1e-3
SPHERES = np.array([[0.0, -100.5, -1.0, 100.0, 1.0]])
MATERIALS = np.array([[0.8, 0.8, 0.2, 0, 0, 0, 0.0, 1.0], [0.8, 0.8, 0.8, 0, 0, 0, 0.5, 0.0], [0.7, 0.3, 0.2, 0, 0, 0, 0.2, 0.4]])


def _rows(v):
    """triangles10 of vertices [n, 3, 3], materials 1 .. 3 in turn."""
    n = len(v)
    return np.concatenate([np.asarray(v, dtype=np.float64).reshape(n, 9), (1.0 + np.arange(n) % 3)[:, None]], axis=1)


def _soup(rng, n, size=0.08, spread=0.9):
    """n triangles of about `size` with centres uniform in the box shrunk to `spread`: vertices [n, 3, 3]."""
    c = CENTRE + (rng.random((n, 1, 3)) - 0.5) * (spread - size)
    return c + (rng.random((n, 3, 3)) - 0.5) * size


def _zero_area():
    v = _soup(np.random.default_rng(101), 120)
    i = np.arange(120)
    v[i % 5 == 0, 1] = v[i % 5 == 0, 0]                              # a segment
    v[i % 10 == 0, 2] = v[i % 10 == 0, 0]                            # a point
    return _rows(v)


def _mixed_scales():
    rng = np.random.default_rng(102)
    v = _soup(rng, 160, size=0.02)
    even = np.arange(160) % 2 == 0
    # (triangles of 0.6 before the shrink, 6e-4 after it: the ray scan's |a| < 1e-8 would leave out anything much smaller, wherever it is aimed)
    v[even] = CLUSTER_AT + (_soup(rng, 80, size=0.6) - CENTRE) * CLUSTER_SHRINK
    v[0] = LO + np.array([[0.0, 0.0, 0.0], [1.0, 1.0, 0.0], [0.0, 1.0, 1.0]])      # one triangle spans the whole box
    return _rows(v)


def _needles():
    rng = np.random.default_rng(103)
    v = _soup(rng, 96)
    for i in range(0, 96, 3):
        u, w = S._unit(rng, 1)[0], S._unit(rng, 1)[0]
        mid = CENTRE + 0.02 * (rng.random(3) - 0.5)
        v[i, 0], v[i, 1] = mid - 0.45 * u, mid + 0.45 * u
        v[i, 2] = v[i, 0] + 1e-3 * w
    return _rows(v)


def _flat():
    xs = np.linspace(LO[0], LO[0] + 1.0, 9)
    ys = np.linspace(LO[1], LO[1] + 1.0, 9)
    v = []
    for j in range(8):
        for i in range(8):
            t = [[xs[i], ys[j], CENTRE[2]], [xs[i + 1], ys[j], CENTRE[2]], [xs[i + 1], ys[j + 1], CENTRE[2]]]
            v += [t, t]                                              # each cell's triangle twice: repeated centroids, exact ties
    return _rows(np.array(v))


def _copies():
    one = np.concatenate([CENTRE + [-0.4, -0.3, 0.1], CENTRE + [0.45, -0.2, 0.0], CENTRE + [0.0, 0.5, -0.1], [2.0]])
    return np.repeat(one[None, :], 200, axis=0)                      # every Morton key equal


def _geometric():
    rng = np.random.default_rng(106)
    v = np.zeros((4 * N_CLUSTERS, 3, 3))
    for k in range(N_CLUSTERS):
        s = 2.0 ** -k
        c = LO + s * (0.65 + 0.02 * (rng.random((4, 1, 3)) - 0.5))
        v[4 * k:4 * k + 4] = c + (rng.random((4, 3, 3)) - 0.5) * 0.2 * s
    return _rows(v)


def _soup160():
    return _rows(_soup(np.random.default_rng(107), 160))


def _scrambled():
    return _soup160()[np.random.default_rng(108).permutation(160)]


_BUILDERS = dict(zero_area=_zero_area, mixed_scales=_mixed_scales, needles=_needles, flat=_flat, copies=_copies, geometric=_geometric, scrambled=_scrambled,
                 soup160=_soup160)


@functools.lru_cache(maxsize=None)
def mesh(name):
    t = _BUILDERS[name]()
    t.setflags(write=False)
    return t


def scene_of(tri):
    return dict(spheres5=SPHERES, materials8=MATERIALS, triangles10=tri)


def shrunk(tri, factor=0.6):
    """The mesh scaled about the middle of its bounds (test_gpu_rebuild._awkward's first pose, without its shift)."""
    t = np.array(tri, dtype=np.float64)
    v = t[:, :9].reshape(-1, 3)
    c = (v.min(axis=0) + v.max(axis=0)) / 2.0
    t[:, :9] = ((v - c) * factor + c).reshape(-1, 9)
    return t


@functools.lru_cache(maxsize=None)
def poses(name, how):
    """(first, target): the handle is created on `first` and — how = update / rebuild — brought to `target`.  The first pose is the target shrunk by 0.6
    about its centre; for `scrambled` it is the same soup before the permutation: the bounds stay, the topology becomes useless."""
    target = mesh(name)
    if how == "create":
        return target, target
    first = mesh("soup160") if name == "scrambled" else shrunk(target)
    first.setflags(write=False)
    return first, target


def frame_of(name, prec, how):
    """The frame the validity rules hold in: a fresh build's of the target (create, rebuild), or the creation pose's (update)."""
    first, target = poses(name, how)
    return S.mesh_frame(first if how == "update" else target, prec)


def zero_area_mask(tri, T):
    """The triangles without area as T holds them: two vertices equal."""
    v = np.asarray(tri, dtype=T)[:, :9].reshape(-1, 3, 3)
    return (v[:, 0] == v[:, 1]).all(axis=1) | (v[:, 0] == v[:, 2]).all(axis=1) | (v[:, 1] == v[:, 2]).all(axis=1)


def surviving_clusters(prec):
    """geometric: the clusters with a triangle whose three vertices are distinct in T."""
    ok = ~zero_area_mask(mesh("geometric"), S.dtype_of(prec))
    return np.flatnonzero(ok.reshape(N_CLUSTERS, 4).any(axis=1))


# ------------------------------------------------------------------ the targeted part
N_SPOTS = 24


def spots(name, prec):
    """(p [m, 3], s [m], ti [m]): places on the features that make the mesh hostile — an interior point of triangle ti (on a segment or a point where
    it has collapsed) — and the local size there: half the shortest edge with length, 0.01 for a point."""
    tri = np.asarray(mesh(name), dtype=np.float64)
    rng = np.random.default_rng(111)
    n = len(tri)
    if name == "zero_area":
        ti = np.arange(0, n, 5)                                      # the 24 collapsed ones
    elif name == "mixed_scales":
        ti = np.concatenate([2 + 2 * rng.permutation(79)[:14], 1 + 2 * rng.permutation(80)[:6], [0, 0, 0, 0]])      # the cluster, the rest, the big one
    elif name == "needles":
        ti = 3 * rng.permutation(32)[:N_SPOTS]
    elif name == "copies":
        ti = np.zeros(N_SPOTS, dtype=np.int64)
    elif name == "geometric":
        alive = surviving_clusters(prec)
        ks = [alive[0], alive[len(alive) // 2], alive[-1]]           # the first, a middle and the last surviving octave
        ti = np.concatenate([np.repeat(4 * k + np.arange(4), 2) for k in ks])
    else:
        ti = rng.permutation(n)[:N_SPOTS]
    v = tri[ti, :9].reshape(-1, 3, 3)
    a = rng.uniform(0.1, 0.8, (len(ti), 1)); b = rng.uniform(0.1, 0.9, (len(ti), 1)) * (1 - a)
    p = v[:, 0] + a * (v[:, 1] - v[:, 0]) + b * (v[:, 2] - v[:, 0])
    e = np.stack([np.linalg.norm(v[:, 1] - v[:, 0], axis=1), np.linalg.norm(v[:, 2] - v[:, 0], axis=1), np.linalg.norm(v[:, 2] - v[:, 1], axis=1)], axis=1)
    s = 0.5 * np.where(e > 0, e, np.inf).min(axis=1)
    return p, np.where(np.isfinite(s), s, 0.01), ti


def _up(rng, n):
    """Unit vectors of the upper half space: an origin along one is clear of the ground sphere."""
    u = S._unit(rng, n)
    u[:, 1] = np.abs(u[:, 1])
    return u


def _ray_rows(o, d, t_min=0.0, t_max=np.inf):
    n = len(o)
    return np.concatenate([o, np.full((n, 1), t_min), d, np.full((n, 1), t_max)], axis=1)


def target_rays(name, prec):
    """Rays at the spots: from 1.2 across the box, and from 10 local sizes away; plus what only this mesh has — along the needles' long edge, and for
    `flat` rays along its zero-extent axis and in its plane, the other components both signed zeros."""
    p, s, ti = spots(name, prec)
    rng = np.random.default_rng(112)
    m = len(p)
    o1, o2 = p + 1.2 * _up(rng, m), p + 10.0 * s[:, None] * _up(rng, m)
    rows = [_ray_rows(o1, 2.3 * (p - o1)), _ray_rows(o2, p - o2)]
    tri = np.asarray(mesh(name), dtype=np.float64)
    if name == "needles":
        v = tri[ti[:12], :9].reshape(-1, 3, 3)
        d = v[:, 1] - v[:, 0]
        rows.append(_ray_rows(v[:, 0] - 0.2 * d, d))
    if name == "flat":
        q = p[:16].copy()
        z = np.array([0.0, -0.0])
        i = np.arange(16)
        d = np.stack([z[i % 2], z[(i // 2) % 2], np.where((i // 4) % 2 == 0, 1.0, -1.0)], axis=1)
        o = q - 0.7 * d
        o[8:, 2] = q[8:, 2] - 1e-3 * d[8:, 2]                        # the second half starts next to the plane
        rows.append(_ray_rows(o, d))
        d = np.stack([np.where(i % 2 == 0, 1.0, -1.0), z[(i // 2) % 2], z[(i // 4) % 2]], axis=1)
        d[8:] = d[8:, [1, 0, 2]]
        rows.append(_ray_rows(q - 0.8 * d, d))                       # in the plane: the origin has its z exactly
    return np.concatenate(rows)


def target_sweeps(name, prec):
    """The target rays as sweeps with radii of half and twice the local size in turn, and sweeps that start in overlap with the spot."""
    p, s, _ = spots(name, prec)
    rng = np.random.default_rng(113)
    rays = target_rays(name, prec)
    m = len(p)
    k = np.arange(len(rays))
    radii = np.where(k % 2 == 0, 0.5, 2.0) * s[k % m]
    start = _ray_rows(p + 0.5 * s[:, None] * S._unit(rng, m), S._unit(rng, m))
    return np.concatenate([rays, start]), np.concatenate([radii, s])


def target_points(name, prec):
    """The spots themselves, points a local size away, and points three sizes away that look no further than two."""
    p, s, _ = spots(name, prec)
    rng = np.random.default_rng(114)
    m = len(p)
    near = p + s[:, None] * S._unit(rng, m)
    short = np.concatenate([p + 3.0 * s[:, None] * S._unit(rng, m), 2.0 * s[:, None]], axis=1)
    return np.concatenate([N._p4(p), N._p4(near), short])


def target_boxes(name, prec):
    """Boxes of about the local size at the spots, boxes without extent on them, and flat boxes a size away."""
    p, s, _ = spots(name, prec)
    rng = np.random.default_rng(115)
    m = len(p)
    flat = rng.uniform(0.5, 2.0, (m, 3)) * s[:, None]
    flat[np.arange(m), np.arange(m) % 3] = 1e-3 * s
    return np.concatenate([V._boxes(p, rng.uniform(0.2, 2.0, (m, 3)) * s[:, None], V.quats(rng, m)), V._boxes(p, np.zeros((m, 3)), V.quats(rng, m)),
                           V._boxes(p + s[:, None] * S._unit(rng, m), flat, V.quats(rng, m))])


# ------------------------------------------------------------------ the sets with the yardsticks' answers
SWEEP_SET = dict(n_head=64, n_graze=48, n_over=48, n_box=64, n_axis=24, n_far=16, n_big=16, n_bound=16, n_in=16, n_win=24, n_zero=16, n_corner=16)
NEAR_SET = dict(n_near=128, n_box=96, n_edge=40, n_far=20, n_r=40)
BOX_SET = dict(n_surf=192, n_whole=8, n_thin=96, n_zero=48, n_far=16, n_small=16, n_mixed=70)
K_HITS, KS_NEAR, K_BOX = 4, (4, 16), 8


def _round(a, T):
    with np.errstate(over="ignore"):
        return np.array(np.asarray(a, dtype=np.float64), dtype=T).astype(np.float64)      # the values the library sees


def _joined(a, b, keys):
    """The base set a followed by the targeted items b; a's parts and indices still hold, since it comes first."""
    return dict(a, **{k: np.concatenate([a[k], b[k]]) for k in keys})


def _sweep_set(name, prec, sc, frame):
    ss = W.SweepScan(sc, prec, frame=frame)
    base = W.build_set(ss, sc, seed=171, **SWEEP_SET)
    rays, radii = target_sweeps(name, prec)
    rays, radii = _round(rays, ss.T), _round(radii, ss.T)
    prim, t, point, normal, valid = ss.sweep(rays, radii)
    more = dict(rays=rays, radii=radii, prim=prim, t=t, point=point, normal=normal, valid=valid)
    out = _joined(base, more, more.keys())
    out["targets"] = slice(len(base["rays"]), len(out["rays"]))
    return N._freeze(out), ss


def _near_set(name, prec, sc, frame):
    ns = N.NearScan(sc, prec, frame=frame)
    base = N.build_set(ns, sc, seed=131, **NEAR_SET)
    pts = _round(target_points(name, prec), ns.T)
    prim, dist, point, valid = ns.query(pts)
    more = dict(points=pts, prim=prim, dist=dist, point=point, valid=valid)
    out = _joined(base, more, more.keys())
    out["targets"] = slice(len(base["points"]), len(out["points"]))
    return N._freeze(out), ns


def _box_set(name, prec, sc, frame):
    ss = V.OverlapScan(sc, prec, frame=frame)
    base = V.build_set(ss, sc, seed=191, **BOX_SET)
    boxes = _round(target_boxes(name, prec), ss.T)
    more = dict(ss.overlap(boxes), boxes=boxes)
    out = _joined(base, more, more.keys())
    out["targets"] = slice(len(base["boxes"]), len(out["boxes"]))
    return N._freeze(out), ss


def _ray_set(name, prec, sc, frame):
    """One ray list for cast / occluded and cast_hits: cast_support's (a), (b), (c) with every second ray aimed at a triangle, axis rays, far rays with
    their invalid twins, the target rays, the three t windows of the first 32 mesh hits, and the invalid kinds among copies of valid rays."""
    scan = S.Scan(H._oracle(), sc, prec, frame)
    rng = np.random.default_rng(151)
    abc = S.aim_at_triangles(rng, np.concatenate([S.rays_a(rng, sc, 64), S.rays_b(rng, sc, 96), S.rays_c(rng, sc, 32)]), sc)
    far, axis, sign = S.rays_far(rng, scan, sc, 24)
    head = np.concatenate([abc, S.rays_axis(rng, sc, 48, scan.T), H.interleave(far, S.rays_far_outside(far, axis, sign, scan)), target_rays(name, prec)])
    with np.errstate(over="ignore"):
        prim, t, _, _ = scan.cast(head)
    same, below, beyond, _ = S.rays_d(head, prim, t, scan.ns, scan.T, 32)
    mixed = np.array(head[:70])
    kinds = S.invalid_kinds(scan.T, scan.frame)
    at = np.arange(0, 70, 7)
    mixed[at] = kinds[np.arange(len(at)) % len(kinds)]
    rays = np.concatenate([head, same, below, beyond, mixed])
    with np.errstate(over="ignore"):
        cast = S.scanned(scan, rays)
        hits = H.reference(sc, prec, rays, frame)
    n_abc, n_t = len(abc) + 48 + 48, len(target_rays(name, prec))
    return dict(cast, targets=slice(n_abc, n_abc + n_t)), hits


def _sdf_set(name, prec, sc, frame, ns):
    """sdf_support.blob_points's parts for a scene whose only sphere is the ground: near the surface, in the grown box, under the ground sphere's top,
    finite r_max, far points with their invalid twins, the target points, and the invalid kinds among copies of valid points."""
    rng = np.random.default_rng(141)
    lo, hi, c, ext = S.target_box(sc)
    g = c + (rng.random((24, 3)) - 0.5) * (hi - lo)
    g[:, 1] = -0.5 - ext * rng.uniform(-0.02, 2.0, 24)
    short = N.in_box(rng, sc, 64)
    short[:, 3] = ext * 10.0 ** rng.uniform(-2.5, -0.5, 64)
    pts = np.concatenate([N.near_surface(rng, sc, 140, frac=0.03), N.in_box(rng, sc, 100), N._p4(g), short, N.far_points(rng, ns, sc, 16), target_points(name, prec)])
    n_t = len(target_points(name, prec))
    pts, at = D.with_invalid(pts, prec, frame)
    ref = D.reference(sc, prec, pts, frame=frame)
    return dict(ref, invalid_at=at, targets=slice(len(pts) - 70 - n_t, len(pts) - 70))


@functools.lru_cache(maxsize=None)
def _sets(name, prec, kind):
    how = "update" if kind == "update" else "create"
    sc = scene_of(poses(name, how)[1])
    frame = frame_of(name, prec, how)
    sweep, ss = _sweep_set(name, prec, sc, frame)
    near, ns = _near_set(name, prec, sc, frame)
    boxes, bs = _box_set(name, prec, sc, frame)
    cast, hits = _ray_set(name, prec, sc, frame)
    return dict(name=name, prec=prec, scene=sc, frame=frame, ns=len(SPHERES), sweep=sweep, sweep_scan=ss, near=near, near_scan=ns, order=KS.order_of(ns, near["points"]),
                boxes=boxes, box_scan=bs, cast=cast, hits=hits, sdf=_sdf_set(name, prec, sc, frame, ns))


def sets(name, prec, how):
    """Every query's set for the mesh the handle holds after `how`, with the answers in the frame that holds.  create and rebuild share one."""
    return _sets(name, prec, "update" if how == "update" else "fresh")


def cases():
    """The matrix: (mesh, how) — create and rebuild for MESHES, update for UPDATES."""
    return [(n, h) for n in MESHES for h in ("create", "rebuild")] + [(n, "update") for n in UPDATES]


QUERIES = ("cast", "hits", "near", "knear", "sweep", "boxes", "sdf")


def winners(st, query):
    """Per item of a query's set the triangle indices that answer it ([n, k] int, -1 in unused places; mesh indices, the spheres subtracted) and
    (empty [n], invalid [n]): a valid item without any object / an invalid item."""
    ns = st["ns"]
    if query == "cast":
        prim = st["cast"]["prim"][:, None]
    elif query == "hits":
        prim = H.cut(st["hits"]["cands"], st["hits"]["prepared"], st["hits"]["sc"].T, K_HITS)[0]
    elif query == "near":
        prim = st["near"]["prim"][:, None]
    elif query == "knear":
        prim = KS.cut(st["order"], KS_NEAR[0])[0]
    elif query == "sweep":
        prim = st["sweep"]["prim"][:, None]
    elif query == "sdf":
        prim = st["sdf"]["prim"][:, None]
    else:
        prim = V.lists(st["boxes"], K_BOX)
    invalid = (prim == INVALID).all(axis=1)
    empty = (prim == MISS).all(axis=1)
    return np.where(prim >= ns, prim - ns, -1), empty, invalid


# ------------------------------------------------------------------ the render walk: paths through scene_s4's camera, started where the mesh is
RENDER = dict(W=1280, H=720, spp=4, depth=4, n=200, seed=17)
# three 16 x 16 pixel windows per mesh (1-based x0, x1, y0, y1), chosen once where the mesh covers most of the window: the soups cover a twentieth of their
# own bounding window, and 600 paths spread over it would meet too few triangles
RENDER_WINDOWS = {
    "zero_area": [(610, 626, 294, 310), (720, 736, 336, 352), (610, 626, 432, 448)],
    "mixed_scales": [(546, 562, 306, 322), (562, 578, 320, 336), (544, 560, 322, 338)],
    "needles": [(576, 592, 332, 348), (710, 726, 304, 320), (626, 642, 432, 448)],
    "flat": [(544, 560, 412, 428), (706, 722, 412, 428), (652, 668, 440, 456)],
    "copies": [(566, 582, 298, 314), (582, 598, 300, 316), (598, 614, 302, 318)],
    "geometric": [(668, 684, 380, 396), (658, 674, 388, 404), (596, 612, 324, 340)],
    "scrambled": [(602, 618, 326, 342), (682, 698, 380, 396), (698, 714, 346, 362)],
}


def render_scene(name):
    """The mesh's scene with scene_s4's camera."""
    from spira_hip import scenes
    return dict(scene_of(np.array(mesh(name))), camera12=scenes.scene_s4(level=1)["camera12"])


def render_paths(k, window):
    """The (i, j, sample) list test_gpu_bvh._trace_equal draws for window k: the same generator, seed and order."""
    rng = np.random.default_rng(RENDER["seed"] + k)
    x0, x1, y0, y1 = window
    n = RENDER["n"]
    return np.stack([rng.integers(x0, x1, n), rng.integers(y0, y1, n), rng.integers(0, RENDER["spp"], n)], axis=1).astype(np.uint32)
