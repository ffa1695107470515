"""Ray queries on a scene handle: the numpy restatement of the library's ray preparation (include/spira_hip.h, "ray queries") and the torch form of
spira_scene_cast_device_* / spira_scene_occluded_device_*; the multi-hit queries (cast_all, count_hits, inside_mesh); the closest-point queries and the
K-nearest ones (k_nearest, count_within); the sphere sweeps (sweep_spheres, sweep_segments) with the numpy twins of csrc/spira_sweep.h; the box overlap
queries (overlap_boxes, voxelize) with the numpy twins of csrc/spira_overlap.h; the triangle overlap queries (overlap_triangles, mesh_pairs,
meshes_intersect: spira_hip/trioverlap.py, named here) with the numpy twins of csrc/spira_trioverlap.h; the signed distance queries (signed_distance, inside_points,
distance_field) with the numpy restatement of their sign rule.

A ray is eight values [ox oy oz t_min dx dy dz t_max].  The library normalises the direction in the call's precision T, nothing fused:
s = (dx dx + dy dy) + dz dz, d = (dx, dy, dz) / sqrt(s); t, t_min and t_max are distances along that unit direction."""
import numpy as np

from . import _binding as B

ORIGIN_BOUND = 64      # the origin rule of scenes with a tree: |(o_k - centre_k) * scale| <= 64


def normalize_rays(rays8, dtype, frame=None):
    """The preparation of spira_query.h (cast_ray_prepare), bit for bit: returns (rays, valid) — `rays` a copy of rays8 in `dtype` whose direction columns
    are the unit directions the kernels walk with (left as given where the ray is invalid), `valid` the library's verdict per ray.
    frame: None for a scene without a tree, else (centre[3], scale) of the tree's normalised frame — the origin rule is then applied."""
    T = np.dtype(dtype).type
    r = np.array(rays8, dtype=T, copy=True).reshape(-1, 8)
    with np.errstate(all="ignore"):
        valid = ~np.isnan(r).any(axis=1)
        valid &= np.isfinite(r[:, [0, 1, 2, 4, 5, 6]]).all(axis=1)
        s = (r[:, 4] * r[:, 4] + r[:, 5] * r[:, 5]) + r[:, 6] * r[:, 6]
        valid &= np.isfinite(s) & ~(s < np.finfo(T).tiny)
        valid &= ~(r[:, 3] < T(0)) & ~(r[:, 7] < r[:, 3])
        if frame is not None:
            c, scale = np.asarray(frame[0], dtype=T), T(frame[1])
            x = (r[:, :3] - c[None, :]) * scale
            valid &= ((x >= T(-ORIGIN_BOUND)) & (x <= T(ORIGIN_BOUND))).all(axis=1)
        d = r[:, 4:7] / np.sqrt(s)[:, None]
    r[:, 4:7] = np.where(valid[:, None], d, r[:, 4:7])
    return r, valid


def _device_list(who, scene, x, columns, stream):
    """The test every device front end makes of its list `x` (a contiguous tensor [n, columns] on a device, in the scene's precision).  Returns the torch
    dtype, n and the stream to enqueue on (`stream`; None: the current one of the tensor's device)."""
    import torch
    want = torch.float32 if scene.prec == "f32" else torch.float64
    if x.dtype != want or not x.is_cuda or x.dim() != 2 or x.shape[1] != columns or not x.is_contiguous():
        raise ValueError("%s: a contiguous device tensor of n x %d %s values is needed" % (who, columns, scene.prec))
    return want, x.shape[0], stream if stream is not None else torch.cuda.current_stream(x.device)


def _ptr(t):
    return t.data_ptr() if t is not None else 0


def cast_rays(scene, rays, want_normal=False, occlusion=False, inplace=False, stream=None):
    """spira_scene_cast_device_* (occlusion: spira_scene_occluded_device_*) for a torch tensor of rays [n, 8] on the scene's device, in the scene's
    precision.  Enqueues on `stream` (a torch.cuda.Stream; None: the current one) and returns device tensors without synchronising:
    (prim int32 [n], t [n], normal [n, 3] or None), or hit uint8 [n] for occlusion.  `rays` must stay alive until the work has run."""
    import torch
    want, n, st = _device_list("cast_rays", scene, rays, 8, stream)
    with torch.cuda.stream(st):
        if occlusion:
            hit = torch.empty(n, dtype=torch.uint8, device=rays.device)
            scene.occluded_device(rays.data_ptr(), n, hit.data_ptr(), st.cuda_stream, inplace=inplace)
            return hit
        prim = torch.empty(n, dtype=torch.int32, device=rays.device)
        t = torch.empty(n, dtype=want, device=rays.device)
        nrm = torch.empty((n, 3), dtype=want, device=rays.device) if want_normal else None
        scene.cast_device(rays.data_ptr(), n, prim.data_ptr(), t.data_ptr(), _ptr(nrm), st.cuda_stream, inplace=inplace)
    return prim, t, nrm


# ------------------------------------------------------------------ multi-hit ray queries (spira_scene_cast_hits_*; csrc/spira_hits.h)
def cast_all(scene, rays, max_hits, count_all=False, inplace=False, want_prim=True, want_t=True, stream=None):
    """The first max_hits hits of every ray, ordered by t ascending and, among equal t, by object index descending: (prim int32 [n, K], t [n, K],
    count [n]), None where not wanted.  rays: a host array [n, 8] — the host form, numpy arrays back — or a torch tensor on the scene's device in the
    scene's precision — spira_scene_cast_hits_device_*, enqueued on `stream` (a torch.cuda.Stream; None: the current one), device tensors back without
    synchronising (count as int32); `rays` must stay alive until the work has run.  count_all: count every candidate of the ray, not the slots filled."""
    if isinstance(rays, np.ndarray) or not hasattr(rays, "is_cuda"):
        return scene.cast_hits(rays, max_hits, inplace=inplace, count_all=count_all, want_prim=want_prim, want_t=want_t)
    import torch
    want, n, st = _device_list("cast_all", scene, rays, 8, stream)
    k = int(max_hits)
    room = k if 0 < k <= B.MAX_HITS else 1
    with torch.cuda.stream(st):
        prim = torch.empty((n, room), dtype=torch.int32, device=rays.device) if want_prim and k else None
        t = torch.empty((n, room), dtype=want, device=rays.device) if want_t and k else None
        count = torch.empty(n, dtype=torch.int32, device=rays.device)
        scene.cast_hits_device(rays.data_ptr(), n, k, _ptr(prim), _ptr(t), count.data_ptr(), st.cuda_stream, inplace=inplace, count_all=count_all)
    return prim, t, count


def count_hits(scene, rays, inplace=False, stream=None):
    """The number of candidates of every ray within its [t_min, t_max] — max_hits = 0 with HITS_COUNT_ALL, no list is kept; 0 for an invalid ray.
    Host array or device tensor, as cast_all."""
    return cast_all(scene, rays, 0, count_all=True, inplace=inplace, stream=stream)[2]


INSIDE_DIRECTIONS = ((0.5377, 0.7211, 0.4366), (-0.6123, 0.3142, 0.7255), (0.2873, -0.4691, -0.8351))      # fixed, parallel to no axis and no diagonal


def inside_mesh(scene, points, max_hits=B.MAX_HITS):
    """For every point of `points` (host array [n, 3]): is it inside the scene's mesh?  Meant for CLOSED meshes (every edge shared by two triangles, no
    self-intersection): a ray from an inside point crosses the surface an odd number of times.  Three rays per point along INSIDE_DIRECTIONS (t_min 0,
    t_max +Inf), the parity of each ray's TRIANGLE crossings, and the majority of the three votes — a ray exactly through an edge or a vertex may count
    a crossing twice, which is why three directions vote.
    A scene without spheres: the count alone decides (max_hits = 0 with HITS_COUNT_ALL, no list is kept or copied), whatever the number of crossings.
    A scene with spheres: a sphere counts once per ray whichever side the origin is on, so its hits say nothing about parity; they are taken out by
    subtracting the listed hits with prim < n_spheres from the count, which needs the list: max_hits (16 at most) slots per ray.  A ray is only refused
    (ValueError) when that cannot be done — it has more candidates than slots AND fewer sphere hits listed than the scene has spheres, so a sphere hit
    may lie beyond the list; with every sphere already listed the crossings beyond the list are all triangles and the count stands.
    Points the library calls invalid (NaN, infinite, beyond the origin rule) are outside.  Returns bool [n]."""
    p = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    n = len(p)
    ns = scene.counts[0]
    k = int(max_hits) if ns else 0
    if ns and not 0 < k <= B.MAX_HITS:
        raise ValueError("inside_mesh: a scene with spheres needs the list (max_hits in 1 .. %d) to take their hits out" % B.MAX_HITS)
    votes = np.zeros(n, dtype=np.int32)
    for d in INSIDE_DIRECTIONS:
        rays = np.concatenate([p, np.zeros((n, 1)), np.tile(np.asarray(d, dtype=np.float64), (n, 1)), np.full((n, 1), np.inf)], axis=1)
        prim, _, count = scene.cast_hits(rays, k, count_all=True, want_t=False)
        crossings = count.astype(np.int64)
        if ns:
            listed = ((prim >= 0) & (prim < ns)).sum(axis=1)
            if ((count > k) & (listed < ns)).any():
                raise ValueError("inside_mesh: a ray has more than max_hits = %d candidates and a sphere hit may lie beyond the list" % k)
            crossings -= listed
        votes += (crossings % 2 == 1)
    return votes >= 2


# ------------------------------------------------------------------ closest-point queries (spira_scene_closest_point_*; csrc/spira_nearest.h)
def prepare_points(points4, dtype, frame=None):
    """The validity rule of spira_nearest.h (nearest_point_prepare), bit for bit: returns (points, valid) — `points` a copy of points4 ([px py pz r_max])
    in `dtype`, `valid` the library's verdict per point.  frame: None for a scene without a tree, else (centre[3], scale): the origin rule is applied."""
    T = np.dtype(dtype).type
    p = np.array(points4, dtype=T, copy=True).reshape(-1, 4)
    with np.errstate(all="ignore"):
        valid = ~np.isnan(p).any(axis=1)
        valid &= np.isfinite(p[:, :3]).all(axis=1)
        valid &= ~(p[:, 3] < T(0))
        if frame is not None:
            c, scale = np.asarray(frame[0], dtype=T), T(frame[1])
            x = (p[:, :3] - c[None, :]) * scale
            valid &= ((x >= T(-ORIGIN_BOUND)) & (x <= T(ORIGIN_BOUND))).all(axis=1)
    return p, valid


def _dot3(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def closest_point_triangle(v0, e1, e2, p):
    """The numpy twin of spira::closest_point_triangle: v0, e1 = v1 - v0, e2 = v2 - v0 and p are arrays [..., 3] of ONE dtype that broadcast against each
    other (points x objects: p[:, None, :] against v0[None, :, :]).  Every region is evaluated and the first matching test of the library's order picks;
    the same operations in the same order on the same values, nothing fused.  Returns (q [..., 3], d2 [...])."""
    v0, e1, e2, p = (np.asarray(x) for x in (v0, e1, e2, p))
    T = p.dtype.type
    with np.errstate(all="ignore"):
        ap = p - v0
        d1, d2 = _dot3(e1, ap), _dot3(e2, ap)
        bp = ap - e1
        d3, d4 = _dot3(e1, bp), _dot3(e2, bp)
        cp = ap - e2
        d5, d6 = _dot3(e1, cp), _dot3(e2, cp)
        vc = d1 * d4 - d3 * d2
        vb = d5 * d2 - d1 * d6
        va = d3 * d6 - d5 * d4
        g, h = d4 - d3, d5 - d6
        r1 = (d1 <= T(0)) & (d2 <= T(0))
        r2 = (d3 >= T(0)) & (d4 <= d3)
        r3 = (vc <= T(0)) & (d1 >= T(0)) & (d3 <= T(0))
        r4 = (d6 >= T(0)) & (d5 <= d6)
        r5 = (vb <= T(0)) & (d2 >= T(0)) & (d6 <= T(0))
        r6 = (va <= T(0)) & (g >= T(0)) & (h >= T(0))
        v3 = (d1 / (d1 - d3))[..., None]
        w5 = (d2 / (d2 - d6))[..., None]
        w6 = (g / (g + h))[..., None]
        s = T(1) / ((va + vb) + vc)
        v7, w7 = (vb * s)[..., None], (vc * s)[..., None]
        v0b = np.broadcast_to(v0, np.broadcast(v0, p).shape)
        q = (v0 + e1 * v7) + e2 * w7
        q = np.where(r6[..., None], (v0 + e1) + (e2 - e1) * w6, q)
        q = np.where(r5[..., None], v0 + e2 * w5, q)
        q = np.where(r4[..., None], v0 + e2, q)
        q = np.where(r3[..., None], v0 + e1 * v3, q)
        q = np.where(r2[..., None], v0 + e1, q)
        q = np.where(r1[..., None], v0b, q)
        r = p - q
        return q, _dot3(r, r)


def closest_point_sphere(c, radius, p):
    """The numpy twin of spira::closest_point_sphere: c [..., 3], radius [...], p [..., 3] of ONE dtype, broadcasting.  Returns (q [..., 3], d2 [...])."""
    c, radius, p = np.asarray(c), np.asarray(radius), np.asarray(p)
    T = p.dtype.type
    with np.errstate(all="ignore"):
        w = p - c
        l = np.sqrt(_dot3(w, w))
        q_far = c + w * (radius / l)[..., None]
        rb = np.broadcast_to(radius, l.shape)
        q_near = c + np.stack([rb, np.zeros_like(rb), np.zeros_like(rb)], axis=-1)
        q = np.where((l >= np.finfo(T).tiny)[..., None], q_far, q_near)
        r = p - q
        return q, _dot3(r, r)


def closest_points(scene, points, inplace=False, want_point=True, want_trips=False, stream=None):
    """spira_scene_closest_point_device_* for a torch tensor of points [n, 4] ([px py pz r_max]) on the scene's device, in the scene's precision.  Enqueues
    on `stream` (a torch.cuda.Stream; None: the current one) and returns device tensors without synchronising: (prim int32 [n], dist [n], point [n, 3]
    or None, trips int32 [n] or None).  `points` must stay alive until the work has run."""
    import torch
    want, n, st = _device_list("closest_points", scene, points, 4, stream)
    with torch.cuda.stream(st):
        prim = torch.empty(n, dtype=torch.int32, device=points.device)
        dist = torch.empty(n, dtype=want, device=points.device)
        q = torch.empty((n, 3), dtype=want, device=points.device) if want_point else None
        trips = torch.empty(n, dtype=torch.int32, device=points.device) if want_trips else None
        scene.closest_point_device(points.data_ptr(), n, prim.data_ptr(), dist.data_ptr(), _ptr(q), st.cuda_stream, inplace=inplace, d_trips_ptr=_ptr(trips))
    return prim, dist, q, trips


# ------------------------------------------------------------------ K-nearest point queries (spira_scene_nearest_k_*; csrc/spira_knearest.h)
def k_nearest(scene, points, k, count_all=False, inplace=False, want_prim=True, want_dist=True, want_point=True, want_trips=False, stream=None):
    """The k closest objects of every point ([px py pz r_max]), ordered by squared distance ascending and, among equal ones, by object index descending:
    (prim int32 [n, K], dist [n, K], point [n, K, 3], count [n], trips [n]), None where not wanted.  points: a host array [n, 4] — the host form, numpy
    arrays back — or a torch tensor on the scene's device in the scene's precision — spira_scene_nearest_k_device_*, enqueued on `stream` (a
    torch.cuda.Stream; None: the current one), device tensors back without synchronising (count and trips as int32); `points` must stay alive until the
    work has run.  count_all: count every object within r_max, not the slots filled."""
    if isinstance(points, np.ndarray) or not hasattr(points, "is_cuda"):
        return scene.nearest_k(points, k, inplace=inplace, count_all=count_all, want_prim=want_prim, want_dist=want_dist, want_point=want_point, want_trips=want_trips)
    import torch
    want, n, st = _device_list("k_nearest", scene, points, 4, stream)
    k = int(k)
    room = k if 0 < k <= B.MAX_NEAR else 1
    with torch.cuda.stream(st):
        prim = torch.empty((n, room), dtype=torch.int32, device=points.device) if want_prim and k else None
        dist = torch.empty((n, room), dtype=want, device=points.device) if want_dist and k else None
        q = torch.empty((n, room, 3), dtype=want, device=points.device) if want_point and k else None
        count = torch.empty(n, dtype=torch.int32, device=points.device)
        trips = torch.empty(n, dtype=torch.int32, device=points.device) if want_trips else None
        scene.nearest_k_device(points.data_ptr(), n, k, _ptr(prim), _ptr(dist), _ptr(q), count.data_ptr(), st.cuda_stream, inplace=inplace, count_all=count_all,
                               d_trips_ptr=_ptr(trips))
    return prim, dist, q, count, trips


def count_within(scene, points, radius=None, inplace=False, stream=None):
    """The number of objects within the radius of every point — max_near = 0 with NEAR_COUNT_ALL, no list is kept; 0 for an invalid point.  points: [n, 4]
    with r_max in the fourth column, or [n, 3] with `radius` (a number or one per point) to go there.  Host array or device tensor, as k_nearest."""
    if radius is not None:
        if isinstance(points, np.ndarray) or not hasattr(points, "is_cuda"):
            p = np.asarray(points, dtype=np.float64).reshape(-1, 3)
            points = np.concatenate([p, np.broadcast_to(np.asarray(radius, dtype=np.float64), (len(p),)).reshape(-1, 1)], axis=1)
        else:
            import torch
            r = torch.as_tensor(radius, dtype=points.dtype, device=points.device).expand(points.shape[0]).reshape(-1, 1)
            points = torch.cat([points[:, :3], r], dim=1).contiguous()
    return k_nearest(scene, points, 0, count_all=True, inplace=inplace, stream=stream)[3]


# ------------------------------------------------------------------ sphere sweeps (spira_scene_sweep_*; csrc/spira_sweep.h)
SWEEP_RADIUS_BOUND = 64      # scenes with a tree: rs * scale <= 64, rs = r + r * 2^-10


def prepare_sweeps(rays8, radii, dtype, frame=None):
    """The validity rule of spira_sweep.h (sweep_prepare), bit for bit: returns (rays, radii, valid) — `rays` as normalize_rays gives them (unit directions
    where the RAY is valid), `radii` in `dtype`, `valid` the library's verdict per sweep: the ray valid by cast's rule, r not NaN, finite and >= 0, and —
    with a frame (centre[3], scale) — rs * scale <= 64."""
    T = np.dtype(dtype).type
    r, valid = normalize_rays(rays8, T, frame)
    rad = np.array(radii, dtype=T, copy=True).reshape(-1)
    if len(rad) != len(r):
        raise ValueError("prepare_sweeps: one radius per ray is needed")
    with np.errstate(all="ignore"):
        valid = valid & ~np.isnan(rad) & np.isfinite(rad) & ~(rad < T(0))
        if frame is not None:
            rs = rad + rad * T(2.0 ** -10)
            valid &= (rs * T(frame[1])) <= T(SWEEP_RADIUS_BOUND)
    return r, rad, valid


def _sweep_radii(r, T):
    r2 = r * r
    rs = r + r * T(2.0 ** -10)
    return r2, rs * rs


def _sweep_foot(a, o, d):
    t_b = _dot3(d, a - o)
    return t_b, (o + d * t_b[..., None]) - a


def _sweep_root_point(m, d, rr, far_root=False):
    md, mm = _dot3(m, d), _dot3(m, m)
    s = np.sqrt(md * md - (mm - rr))
    return (-md) + s if far_root else (-md) - s


def _sweep_root_edge(m, e, d, r2, T):
    ee, de, me, md, mm = _dot3(e, e), _dot3(d, e), _dot3(m, e), _dot3(m, d), _dot3(m, m)
    qa, qb, qc = ee - de * de, ee * md - de * me, ee * (mm - r2) - me * me
    tau = ((-qb) - np.sqrt(qb * qb - qa * qc)) / qa
    f = (me + de * tau) / ee
    return np.where((f >= T(0)) & (f <= T(1)), tau, T(np.nan))


def _sweep_decide(closest_point, o, d, t_min, t_max, r2, rs2, q0, d20, tp, T):
    """Steps 1, 3 and the candidate rule at closest = t_max for proposals tp [..., P]: every proposal within [t_min, t_max] of an object that does not
    start in overlap is evaluated (closest_point(sel, pc): the object's function for the objects at index tuple sel, at the points pc), the smallest
    verified one is t_k.  A proposal beyond t_max is no candidate verified or not, so leaving it out changes no output."""
    start = d20 <= r2
    ok = (tp >= t_min[..., None]) & ~(tp > t_max[..., None]) & ~start[..., None]      # NaN: never
    at = np.nonzero(ok)
    sel = at[:-1]
    qc, dc = closest_point(sel, o[sel] + d[sel] * tp[at][:, None])
    qv, dv = np.zeros(tp.shape + (3,), dtype=tp.dtype), np.full(tp.shape, np.inf, dtype=tp.dtype)
    qv[at], dv[at] = qc, dc
    ok &= dv <= rs2[..., None]
    key = np.where(ok, tp, T(np.inf))
    j = np.argmin(key, axis=-1)                                      # the first of the smallest: equal proposals evaluate the same point
    tk = np.take_along_axis(key, j[..., None], axis=-1)[..., 0]
    qk = np.take_along_axis(qv, j[..., None, None], axis=-2)[..., 0, :]
    found = start | ok.any(axis=-1)
    tk = np.where(start, t_min, tk)
    qk = np.where(start[..., None], q0, qk)
    hit = found & ~((tk < t_min) | (tk > t_max))
    return np.where(hit, tk, t_max), np.where(hit[..., None], qk, T(0)), hit


def sweep_sphere_triangle(v0, e1, e2, o, d, r, t_min, t_max):
    """The numpy twin of spira::sweep_sphere_triangle with bound = t_max: v0, e1, e2, o, d (unit) are arrays [..., 3] and r, t_min, t_max arrays [...] of ONE
    dtype that broadcast against each other.  Every branch is evaluated — the start overlap, the seven proposals, a verification of each — and np.where
    selects; the same operations in the same order on the same values as the header.  Returns (t [...], q [..., 3], hit [...]): t = t_k and q = q_k where
    the triangle is a candidate at closest = t_max, else t_max and 0."""
    v0, e1, e2, o, d, r, t_min, t_max = np.broadcast_arrays(*[np.asarray(x) for x in (v0, e1, e2, o, d)] + [np.asarray(x)[..., None] for x in (r, t_min, t_max)])
    single = o.ndim == 1                                             # one sweep against one triangle: a leading axis for the gather below
    if single:
        v0, e1, e2, o, d, r, t_min, t_max = (x[None] for x in (v0, e1, e2, o, d, r, t_min, t_max))
    r, t_min, t_max = r[..., 0], t_min[..., 0], t_max[..., 0]
    T = o.dtype.type
    with np.errstate(all="ignore"):
        r2, rs2 = _sweep_radii(r, T)
        p0 = o + d * t_min[..., None]
        q0, d20 = closest_point_triangle(v0, e1, e2, p0)
        t_b, w = _sweep_foot(v0, o, d)
        n = np.stack([e1[..., 1] * e2[..., 2] - e1[..., 2] * e2[..., 1], e1[..., 2] * e2[..., 0] - e1[..., 0] * e2[..., 2],
                      e1[..., 0] * e2[..., 1] - e1[..., 1] * e2[..., 0]], axis=-1)
        nl = np.sqrt(_dot3(n, n))
        s0, nd, nw = _dot3(n, p0 - v0), _dot3(n, d), _dot3(n, w)
        off = r * nl
        off = np.where(s0 < T(0), -off, off)
        tau = (off - nw) / nd
        g = w + d * tau[..., None]
        p1, p2, a11, a12, a22 = _dot3(e1, g), _dot3(e2, g), _dot3(e1, e1), _dot3(e1, e2), _dot3(e2, e2)
        bv, bw, det = a22 * p1 - a12 * p2, a11 * p2 - a12 * p1, a11 * a22 - a12 * a12
        t_face = np.where((nd == nd) & (nd != T(0)) & (bv >= T(0)) & (bw >= T(0)) & (bv + bw <= det), t_b + tau, T(np.nan))
        w1, w2, e3 = w - e1, w - e2, e2 - e1
        tp = np.stack([t_face, t_b + _sweep_root_edge(w, e1, d, r2, T), t_b + _sweep_root_edge(w, e2, d, r2, T), t_b + _sweep_root_edge(w1, e3, d, r2, T),
                       t_b + _sweep_root_point(w, d, r2), t_b + _sweep_root_point(w1, d, r2), t_b + _sweep_root_point(w2, d, r2)], axis=-1)
        cp = lambda sel, pc: closest_point_triangle(v0[sel], e1[sel], e2[sel], pc)
        t, q, hit = _sweep_decide(cp, o, d, t_min, t_max, r2, rs2, q0, d20, tp, T)
    return (t[0], q[0], hit[0]) if single else (t, q, hit)


def sweep_sphere_sphere(c, radius, o, d, r, t_min, t_max):
    """The numpy twin of spira::sweep_sphere_sphere with bound = t_max (the shell of the sphere c [..., 3], radius [...]); arguments and results as
    sweep_sphere_triangle."""
    c, o, d, radius, r, t_min, t_max = np.broadcast_arrays(*[np.asarray(x) for x in (c, o, d)] + [np.asarray(x)[..., None] for x in (radius, r, t_min, t_max)])
    single = o.ndim == 1
    if single:
        c, o, d, radius, r, t_min, t_max = (x[None] for x in (c, o, d, radius, r, t_min, t_max))
    radius, r, t_min, t_max = radius[..., 0], r[..., 0], t_min[..., 0], t_max[..., 0]
    T = o.dtype.type
    with np.errstate(all="ignore"):
        r2, rs2 = _sweep_radii(r, T)
        p0 = o + d * t_min[..., None]
        q0, d20 = closest_point_sphere(c, radius, p0)
        t_b, w = _sweep_foot(c, o, d)
        rp, rm = radius + r, radius - r
        tp = np.stack([t_b + _sweep_root_point(w, d, rp * rp), np.where(radius > r, t_b + _sweep_root_point(w, d, rm * rm, far_root=True), T(np.nan))], axis=-1)
        cp = lambda sel, pc: closest_point_sphere(c[sel], radius[sel], pc)
        t, q, hit = _sweep_decide(cp, o, d, t_min, t_max, r2, rs2, q0, d20, tp, T)
    return (t[0], q[0], hit[0]) if single else (t, q, hit)


def sweep_spheres(scene, rays, radii, blocked=False, inplace=False, want_point=True, want_normal=True, want_trips=False, stream=None):
    """spira_scene_sweep_* (blocked: spira_scene_sweep_blocked_*): the first contact of a ball of radius radii[i] whose centre moves along rays[i]
    ([ox oy oz t_min dx dy dz t_max], as for cast).  Returns (prim int32 [n], t [n], point [n, 3], normal [n, 3], trips [n]), None where not wanted, or for
    blocked the uint8 [n] verdicts (1 blocked, 0 free, 255 invalid).  rays, radii: host arrays — the host form, numpy arrays back — or torch tensors on the
    scene's device in the scene's precision — the device form, enqueued on `stream` (a torch.cuda.Stream; None: the current one), device tensors back
    without synchronising (trips as int32); the inputs must stay alive until the work has run."""
    if isinstance(rays, np.ndarray) or not hasattr(rays, "is_cuda"):
        if blocked:
            return scene.sweep_blocked(rays, radii, inplace=inplace)
        return scene.sweep(rays, radii, inplace=inplace, want_point=want_point, want_normal=want_normal, want_trips=want_trips)
    import torch
    want, n, st = _device_list("sweep_spheres", scene, rays, 8, stream)
    if radii.dtype != want or not radii.is_cuda or radii.dim() != 1 or radii.shape[0] != n or not radii.is_contiguous():
        raise ValueError("sweep_spheres: radii must be a contiguous device tensor of n %s values" % scene.prec)
    with torch.cuda.stream(st):
        if blocked:
            hit = torch.empty(n, dtype=torch.uint8, device=rays.device)
            scene.sweep_blocked_device(rays.data_ptr(), radii.data_ptr(), n, hit.data_ptr(), st.cuda_stream, inplace=inplace)
            return hit
        prim = torch.empty(n, dtype=torch.int32, device=rays.device)
        t = torch.empty(n, dtype=want, device=rays.device)
        point = torch.empty((n, 3), dtype=want, device=rays.device) if want_point else None
        nrm = torch.empty((n, 3), dtype=want, device=rays.device) if want_normal else None
        trips = torch.empty(n, dtype=torch.int32, device=rays.device) if want_trips else None
        scene.sweep_device(rays.data_ptr(), radii.data_ptr(), n, prim.data_ptr(), t.data_ptr(), _ptr(point), _ptr(nrm), st.cuda_stream, inplace=inplace,
                           d_trips_ptr=_ptr(trips))
    return prim, t, point, nrm, trips


def sweep_segments(scene, a, b, radius):
    """A ball of `radius` (a number or one per segment) moved from a[i] to b[i] (host arrays [n, 3]): rays with t_min 0 and t_max = |b - a|.  Returns
    (prim int32 [n], the fraction of the segment travelled at the first contact — 1 for a free segment, 0 for one the library calls invalid, such as
    a == b — and the contact point [n, 3])."""
    a, b = np.asarray(a, dtype=np.float64).reshape(-1, 3), np.asarray(b, dtype=np.float64).reshape(-1, 3)
    T = np.float32 if scene.prec == "f32" else np.float64
    d = b - a
    length = np.sqrt((d * d).sum(axis=1))
    rays = np.concatenate([a, np.zeros((len(a), 1)), d, length[:, None]], axis=1).astype(T)
    rad = np.broadcast_to(np.asarray(radius, dtype=np.float64), (len(a),)).astype(T)
    prim, t, point, _, _ = scene.sweep(rays, rad, want_normal=False)
    with np.errstate(all="ignore"):
        frac = np.where(prim == B.RAY_INVALID, T(0), t / rays[:, 7])
    return prim, frac, point


# ------------------------------------------------------------------ box overlap queries (spira_scene_overlap_box_* / _any_*; csrc/spira_overlap.h)
OVERLAP_EXTENT_BOUND = 64      # scenes with a tree: He_k * scale <= 64, He the enclosing axis-aligned half extent


def box_axes(quat):
    """The numpy twin of spira::overlap_axes: quat [..., 4] = (qx, qy, qz, qw) of one dtype.  Returns (A [..., 3, 3], n2 [...]) — row i of A is the box
    axis A_i in world coordinates; the library normalises the quaternion."""
    q = np.asarray(quat)
    T = q.dtype.type
    with np.errstate(all="ignore"):
        n2 = (q[..., 0] * q[..., 0] + q[..., 1] * q[..., 1]) + (q[..., 2] * q[..., 2] + q[..., 3] * q[..., 3])
        l = np.sqrt(n2)
        x, y, z, w = q[..., 0] / l, q[..., 1] / l, q[..., 2] / l, q[..., 3] / l
        xx, yy, zz, xy, xz, yz, xw, yw, zw = x * x, y * y, z * z, x * y, x * z, y * z, x * w, y * w, z * w
        one, two = T(1), T(2)
        a0 = np.stack([one - two * (yy + zz), two * (xy + zw), two * (xz - yw)], axis=-1)
        a1 = np.stack([two * (xy - zw), one - two * (xx + zz), two * (yz + xw)], axis=-1)
        a2 = np.stack([two * (xz + yw), two * (yz - xw), one - two * (xx + yy)], axis=-1)
    return np.stack([a0, a1, a2], axis=-2), n2


def prepare_boxes(boxes10, dtype, frame=None):
    """The validity rule of spira_overlap.h (overlap_prepare), bit for bit: returns (boxes, A, He, valid) — `boxes` a copy of boxes10
    ([cx cy cz hx hy hz qx qy qz qw]) in `dtype`, A [n, 3, 3] the box axes, He [n, 3] the enclosing axis-aligned half extents, `valid` the library's
    verdict per box: no NaN, nothing infinite, h >= 0, n2 finite and normal, and — with a frame (centre[3], scale) — the origin rule for the centre and
    He_k * scale <= 64."""
    T = np.dtype(dtype).type
    b = np.array(boxes10, dtype=T, copy=True).reshape(-1, 10)
    with np.errstate(all="ignore"):
        valid = ~np.isnan(b).any(axis=1) & np.isfinite(b).all(axis=1)
        valid &= ~(b[:, 3:6] < T(0)).any(axis=1)
        A, n2 = box_axes(b[:, 6:10])
        valid &= np.isfinite(n2) & ~(n2 < np.finfo(T).tiny)
        h = b[:, 3:6]
        He = (np.abs(A[:, 0, :]) * h[:, 0:1] + np.abs(A[:, 1, :]) * h[:, 1:2]) + np.abs(A[:, 2, :]) * h[:, 2:3]
        if frame is not None:
            c, scale = np.asarray(frame[0], dtype=T), T(frame[1])
            x = (b[:, :3] - c[None, :]) * scale
            valid &= ((x >= T(-ORIGIN_BOUND)) & (x <= T(ORIGIN_BOUND))).all(axis=1)
            valid &= ((He * scale) <= T(OVERLAP_EXTENT_BOUND)).all(axis=1)
    return b, A, He, valid


def _box_frame(A, a):
    return np.stack([_dot3(A[..., 0, :], a), _dot3(A[..., 1, :], a), _dot3(A[..., 2, :], a)], axis=-1)


def _overlap_axis(p0, p1, p2, rad):
    ok = ~(np.isnan(p0) | np.isnan(p1) | np.isnan(p2) | np.isnan(rad))
    return ok & (np.minimum(np.minimum(p0, p1), p2) <= rad) & (np.maximum(np.maximum(p0, p1), p2) >= -rad)


def overlap_box_triangle(v0, e1, e2, c, h, A):
    """The numpy twin of spira::overlap_box_triangle: v0, e1 = v1 - v0, e2 = v2 - v0, the box centre c and half extents h are arrays [..., 3] and A
    [..., 3, 3] (box_axes) of ONE dtype that broadcast against each other (boxes x objects: c[:, None, :] against v0[None, :, :]).  All 13 axes are
    evaluated; the same operations in the same order on the same values as the header.  Returns the candidate verdict, bool [...]."""
    v0, e1, e2, c, h, A = (np.asarray(x) for x in (v0, e1, e2, c, h, A))
    with np.errstate(all="ignore"):
        u0, f1, f2 = _box_frame(A, v0 - c), _box_frame(A, e1), _box_frame(A, e2)
        u1, u2, f3 = u0 + f1, u0 + f2, f2 - f1
        ok = np.ones(np.broadcast(u0[..., 0], h[..., 0]).shape, dtype=bool)
        for k in range(3):
            ok &= _overlap_axis(u0[..., k], u1[..., k], u2[..., k], h[..., k])
        n = np.stack([f1[..., 1] * f2[..., 2] - f1[..., 2] * f2[..., 1], f1[..., 2] * f2[..., 0] - f1[..., 0] * f2[..., 2],
                      f1[..., 0] * f2[..., 1] - f1[..., 1] * f2[..., 0]], axis=-1)
        pn = _dot3(n, u0)
        ok &= _overlap_axis(pn, pn, pn, (np.abs(n[..., 0]) * h[..., 0] + np.abs(n[..., 1]) * h[..., 1]) + np.abs(n[..., 2]) * h[..., 2])
        ok &= (n != 0).any(axis=-1)                                   # zero area: never a candidate
        for f in (f1, f2, f3):
            for i in range(3):
                a, b = (i + 1) % 3, (i + 2) % 3
                fa, fb = f[..., a], f[..., b]
                ok &= _overlap_axis(u0[..., b] * fa - u0[..., a] * fb, u1[..., b] * fa - u1[..., a] * fb, u2[..., b] * fa - u2[..., a] * fb,
                                    np.abs(fb) * h[..., a] + np.abs(fa) * h[..., b])
    return ok


def overlap_box_sphere(centre, radius, c, h, A):
    """The numpy twin of spira::overlap_box_sphere (the sphere is a shell): centre [..., 3], radius [...], and the box c, h, A as overlap_box_triangle."""
    centre, radius, c, h, A = (np.asarray(x) for x in (centre, radius, c, h, A))
    T = c.dtype.type
    with np.errstate(all="ignore"):
        p = _box_frame(A, centre - c)
        a = np.abs(p)
        e = a - h
        e = np.where(e > T(0), e, T(0))
        g = a + h
        dmin2, dmax2, r2 = _dot3(e, e), _dot3(g, g), radius * radius
        return (dmin2 <= r2) & (dmax2 >= r2)


def overlap_boxes(scene, boxes, max_list, any=False, inplace=False, want_trips=False, stream=None):
    """spira_scene_overlap_box_* (any: spira_scene_overlap_any_*): the objects that touch each oriented box ([cx cy cz hx hy hz qx qy qz qw]).  Returns
    (prim int32 [n, K] — the first max_list candidates in ascending object index, None with max_list = 0 —, count [n] of ALL candidates, trips [n] or
    None), or for `any` the uint8 [n] verdicts (1 touched, 0 not, 255 invalid).  boxes: a host array [n, 10] — the host form, numpy arrays back — or a torch
    tensor on the scene's device in the scene's precision — the device form, enqueued on `stream` (a torch.cuda.Stream; None: the current one), device
    tensors back without synchronising (count and trips as int32); `boxes` must stay alive until the work has run."""
    if isinstance(boxes, np.ndarray) or not hasattr(boxes, "is_cuda"):
        if any:
            return scene.overlap_any(boxes, inplace=inplace)
        return scene.overlap_box(boxes, max_list, inplace=inplace, want_trips=want_trips)
    import torch
    _, n, st = _device_list("overlap_boxes", scene, boxes, 10, stream)
    k = int(max_list)
    room = k if 0 < k <= B.MAX_OVERLAP else 1
    with torch.cuda.stream(st):
        if any:
            hit = torch.empty(n, dtype=torch.uint8, device=boxes.device)
            scene.overlap_any_device(boxes.data_ptr(), n, hit.data_ptr(), st.cuda_stream, inplace=inplace)
            return hit
        prim = torch.empty((n, room), dtype=torch.int32, device=boxes.device) if k else None
        count = torch.empty(n, dtype=torch.int32, device=boxes.device)
        trips = torch.empty(n, dtype=torch.int32, device=boxes.device) if want_trips else None
        scene.overlap_box_device(boxes.data_ptr(), n, k, _ptr(prim), count.data_ptr(), st.cuda_stream, inplace=inplace, d_trips_ptr=_ptr(trips))
    return prim, count, trips


def boxes_from_bounds(lo, hi):
    """Axis-aligned boxes [n, 10] with the identity quaternion from their corners lo, hi [n, 3] (numpy arrays, or torch tensors — then on their device):
    c = (lo + hi) / 2, h = (hi - lo) / 2."""
    if hasattr(lo, "is_cuda"):
        import torch
        q = torch.zeros((lo.shape[0], 4), dtype=lo.dtype, device=lo.device)
        q[:, 3] = 1
        return torch.cat([(lo + hi) / 2, (hi - lo) / 2, q], dim=1).contiguous()
    lo, hi = np.asarray(lo), np.asarray(hi)
    lo, hi = lo.reshape(-1, 3), hi.reshape(-1, 3)
    q = np.zeros((len(lo), 4), dtype=np.result_type(lo, hi))
    q[:, 3] = 1
    return np.concatenate([(lo + hi) / 2, (hi - lo) / 2, q], axis=1)


def voxel_boxes(lo, hi, dims, dtype):
    """The cells of voxelize as host boxes [nx ny nz, 10] in `dtype`, x slowest: with half_k = fl((hi_k - lo_k) / (2 dims_k)) (Float64, then rounded to
    dtype), cell i of axis k has the centre lo_k + (2 i + 1) half_k (in dtype: one product, one sum) and the half extent half_k."""
    T = np.dtype(dtype).type
    lo64, hi64 = np.asarray(lo, dtype=np.float64).reshape(3), np.asarray(hi, dtype=np.float64).reshape(3)
    dims = [int(d) for d in dims]
    half = ((hi64 - lo64) / (2.0 * np.asarray(dims, dtype=np.float64))).astype(T)
    lo_t = lo64.astype(T)
    cs = [lo_t[k] + (2 * np.arange(dims[k]) + 1).astype(T) * half[k] for k in range(3)]
    g = np.stack(np.meshgrid(*cs, indexing="ij"), axis=-1).reshape(-1, 3)
    out = np.zeros((len(g), 10), dtype=T)
    out[:, 0:3], out[:, 3:6], out[:, 9] = g, half[None, :], T(1)
    return out


def voxelize(scene, lo, hi, dims, stream=None):
    """A surface voxelisation: the grid of dims = (nx, ny, nz) cells over the box [lo, hi]; a cell is True where its closed box touches a surface of the
    scene (a triangle, or a sphere's shell).  The cells (voxel_boxes' arithmetic, identity quaternions) are made on the scene's device with torch and
    answered by spira_scene_overlap_any_device_* on `stream` (a torch.cuda.Stream; None: the current one).  Returns a bool device tensor [nx, ny, nz]
    without synchronising; cells the library calls invalid (beyond the origin or the extent rule) are False."""
    import torch
    want = torch.float32 if scene.prec == "f32" else torch.float64
    T = np.float32 if scene.prec == "f32" else np.float64
    dims = [int(d) for d in dims]
    lo64, hi64 = np.asarray(lo, dtype=np.float64).reshape(3), np.asarray(hi, dtype=np.float64).reshape(3)
    half = ((hi64 - lo64) / (2.0 * np.asarray(dims, dtype=np.float64))).astype(T)
    lo_t = lo64.astype(T)
    dev = torch.device("cuda", torch.cuda.current_device())      # (a handle is resident on the current device)
    st = stream if stream is not None else torch.cuda.current_stream(dev)
    n = dims[0] * dims[1] * dims[2]
    with torch.cuda.stream(st):
        cs = []
        for k in range(3):
            odd = (2 * torch.arange(dims[k], device=dev) + 1).to(want)
            cs.append(torch.tensor(lo_t[k], dtype=want, device=dev) + odd * torch.tensor(half[k], dtype=want, device=dev))
        boxes = torch.zeros((dims[0], dims[1], dims[2], 10), dtype=want, device=dev)
        boxes[..., 0] = cs[0][:, None, None]
        boxes[..., 1] = cs[1][None, :, None]
        boxes[..., 2] = cs[2][None, None, :]
        for k in range(3):
            boxes[..., 3 + k] = float(half[k])
        boxes[..., 9] = 1
        boxes = boxes.reshape(n, 10)
        hit = overlap_boxes(scene, boxes, 0, any=True, stream=st)
        boxes.record_stream(st)
        return (hit == 1).reshape(dims[0], dims[1], dims[2])


# ------------------------------------------------------------------ signed distance queries (spira_scene_signed_distance_*; csrc/spira_sdf.h)
def inside_spheres(spheres5, points, dtype):
    """Step 2 of the contract in numpy: w = p - c, l = sqrt(w.w) (closest_point_sphere's values), inside when l < r as given.  spheres5 [ns, 5] and
    points [n, 3] are taken in `dtype`.  Returns bool [n]."""
    T = np.dtype(dtype).type
    sp = np.asarray(spheres5, dtype=T).reshape(-1, 5)
    p = np.asarray(points, dtype=T).reshape(-1, 3)
    if not len(sp):
        return np.zeros(len(p), dtype=bool)
    with np.errstate(all="ignore"):
        w = p[:, None, :] - sp[None, :, 0:3]
        l = np.sqrt(_dot3(w, w))
        return (l < sp[None, :, 3]).any(axis=1)


def signed_distance_rules(valid, prim, dist, point, in_sphere, counts, has_triangles):
    """Steps 2 to 4 of the contract in numpy, given the closest-point scan's outputs (prim, dist, point: miss and invalid rows as that entry writes them),
    the sphere verdict of step 2 (bool [n]) and the triangle candidates of the three rays (counts [n, 3], every ray counted).  Returns (prim, dist, point,
    inside uint8 [n], crossings uint32 [n, 3]) as spira_scene_signed_distance_* writes them: ray 2's slot is SDF_SKIPPED where the first two parities
    agree, all three where the scene has no triangle; an invalid point has inside 255 and crossings 0."""
    valid = np.asarray(valid, dtype=bool)
    n = len(valid)
    cr = np.full((n, 3), B.SDF_SKIPPED, dtype=np.uint32)
    mesh = np.zeros(n, dtype=bool)
    if has_triangles:
        c = np.asarray(counts).reshape(n, 3).astype(np.uint32)
        agree = ((c[:, 0] ^ c[:, 1]) & 1) == 0
        cr[:, 0], cr[:, 1] = c[:, 0], c[:, 1]
        cr[:, 2] = np.where(agree, np.uint32(B.SDF_SKIPPED), c[:, 2])
        mesh = (np.where(agree, c[:, 0], c[:, 2]) & 1) == 1
    inside = valid & (np.asarray(in_sphere, dtype=bool) | mesh)
    cr[~valid] = 0
    d = np.array(dist, copy=True)
    d[inside] = -np.abs(d[inside])                                   # the sign bit set: -0.0 can occur
    return np.array(prim, copy=True), d, np.array(point, copy=True), np.where(valid, inside.astype(np.uint8), np.uint8(255)), cr


def signed_distance(scene, points, inplace=False, want_point=True, want_crossings=False, want_trips=False, stream=None):
    """The nearest surface of every point ([px py pz r_max]) and which side of it the point is on: (prim int32 [n], dist [n] — negative inside —,
    point [n, 3], inside uint8 [n] (1, 0, 255 for an invalid point), crossings [n, 3], trips [n]), None where not wanted.  The sign is meaningful for
    closed meshes and defined for every mesh, as inside_mesh's; a point inside a sphere of the scene is inside.  points: a host array [n, 4] — the host
    form, numpy arrays back — or a torch tensor on the scene's device in the scene's precision — spira_scene_signed_distance_device_*, enqueued on
    `stream` (a torch.cuda.Stream; None: the current one), device tensors back without synchronising (crossings and trips as int32: SDF_SKIPPED reads -1);
    `points` must stay alive until the work has run."""
    if isinstance(points, np.ndarray) or not hasattr(points, "is_cuda"):
        return scene.signed_distance(points, inplace=inplace, want_point=want_point, want_crossings=want_crossings, want_trips=want_trips)
    import torch
    want, n, st = _device_list("signed_distance", scene, points, 4, stream)
    with torch.cuda.stream(st):
        prim = torch.empty(n, dtype=torch.int32, device=points.device)
        dist = torch.empty(n, dtype=want, device=points.device)
        q = torch.empty((n, 3), dtype=want, device=points.device) if want_point else None
        inside = torch.empty(n, dtype=torch.uint8, device=points.device)
        cr = torch.empty((n, 3), dtype=torch.int32, device=points.device) if want_crossings else None
        trips = torch.empty(n, dtype=torch.int32, device=points.device) if want_trips else None
        scene.signed_distance_device(points.data_ptr(), n, prim.data_ptr(), dist.data_ptr(), _ptr(q), inside.data_ptr(), st.cuda_stream, inplace=inplace,
                                     d_crossings_ptr=_ptr(cr), d_trips_ptr=_ptr(trips))
    return prim, dist, q, inside, cr, trips


def inside_points(scene, points, stream=None):
    """The sign-only form: is every point ([n, 3], or [n, 4] whose fourth column is ignored) inside the scene — inside a sphere, or inside the mesh by the
    vote of signed_distance?  No nearest walk is run.  Host array: bool numpy array back; device tensor: a bool device tensor, enqueued on `stream` without
    synchronising.  Points the library calls invalid are outside."""
    if isinstance(points, np.ndarray) or not hasattr(points, "is_cuda"):
        p = np.asarray(points, dtype=np.float64)
        p = p.reshape(-1, p.shape[-1])[:, :3]
        p4 = np.concatenate([p, np.zeros((len(p), 1))], axis=1)
        inside = scene.signed_distance(p4, want_prim=False, want_dist=False, want_point=False)[3]
        return inside == 1
    import torch
    want = torch.float32 if scene.prec == "f32" else torch.float64
    if points.dtype != want or not points.is_cuda or points.dim() != 2 or points.shape[1] not in (3, 4):
        raise ValueError("inside_points: a device tensor of n x 3 or n x 4 %s values is needed" % scene.prec)
    n = points.shape[0]
    st = stream if stream is not None else torch.cuda.current_stream(points.device)
    with torch.cuda.stream(st):
        p4 = torch.zeros((n, 4), dtype=want, device=points.device)
        p4[:, :3] = points[:, :3]
        inside = torch.empty(n, dtype=torch.uint8, device=points.device)
        scene.signed_distance_device(p4.data_ptr(), n, 0, 0, 0, inside.data_ptr(), st.cuda_stream)
        p4.record_stream(st)
        return inside == 1


def distance_field(scene, lo, hi, dims, band=None, stream=None):
    """A signed distance field: the grid of dims = (nx, ny, nz) cells over the box [lo, hi], each cell's CENTRE (voxel_boxes' arithmetic, made on the
    scene's device with torch) answered by one spira_scene_signed_distance_device_* call on `stream` (a torch.cuda.Stream; None: the current one) with
    r_max = band, or +Inf when band is None: negative inside, band (signed) where nothing lies within it.  Returns a device tensor [nx, ny, nz] in the
    scene's precision without synchronising; cells the library calls invalid (beyond the origin rule) are NaN."""
    import torch
    want = torch.float32 if scene.prec == "f32" else torch.float64
    T = np.float32 if scene.prec == "f32" else np.float64
    dims = [int(d) for d in dims]
    lo64, hi64 = np.asarray(lo, dtype=np.float64).reshape(3), np.asarray(hi, dtype=np.float64).reshape(3)
    half = ((hi64 - lo64) / (2.0 * np.asarray(dims, dtype=np.float64))).astype(T)
    lo_t = lo64.astype(T)
    dev = torch.device("cuda", torch.cuda.current_device())      # (a handle is resident on the current device)
    st = stream if stream is not None else torch.cuda.current_stream(dev)
    n = dims[0] * dims[1] * dims[2]
    with torch.cuda.stream(st):
        cs = []
        for k in range(3):
            odd = (2 * torch.arange(dims[k], device=dev) + 1).to(want)
            cs.append(torch.tensor(lo_t[k], dtype=want, device=dev) + odd * torch.tensor(half[k], dtype=want, device=dev))
        pts = torch.empty((dims[0], dims[1], dims[2], 4), dtype=want, device=dev)
        pts[..., 0] = cs[0][:, None, None]
        pts[..., 1] = cs[1][None, :, None]
        pts[..., 2] = cs[2][None, None, :]
        pts[..., 3] = float("inf") if band is None else float(T(band))
        pts = pts.reshape(n, 4)
        dist = torch.empty(n, dtype=want, device=dev)
        inside = torch.empty(n, dtype=torch.uint8, device=dev)
        scene.signed_distance_device(pts.data_ptr(), n, 0, dist.data_ptr(), 0, inside.data_ptr(), st.cuda_stream)
        pts.record_stream(st)
        field = torch.where(inside == 255, torch.full_like(dist, float("nan")), dist)
        return field.reshape(dims[0], dims[1], dims[2])


# ------------------------------------------------------------------ triangle overlap queries (spira_scene_overlap_tri_* / _tri_any_*; csrc/spira_trioverlap.h)
from .trioverlap import (meshes_intersect, mesh_pairs, overlap_tri_sphere, overlap_tri_triangle, overlap_triangles,      # noqa: E402,F401
                         prepare_triangles)
