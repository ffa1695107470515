"""Triangle overlap queries on a scene handle (spira_scene_overlap_tri_* / spira_scene_overlap_tri_any_*): the numpy twins of csrc/spira_trioverlap.h,
operation for operation (prepare_triangles, overlap_tri_triangle, overlap_tri_sphere), the host / torch front end (overlap_triangles) and what a caller
with a second mesh asks (mesh_pairs, meshes_intersect).  spira_hip.query names all of them: query.overlap_triangles is this module's."""
import numpy as np

from . import _binding as B

ORIGIN_BOUND = 64      # the origin rule of scenes with a tree: |(q_k - centre_k) * scale| <= 64, for each of the three vertices


def _dot3(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def _cross3(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], axis=-1)


def prepare_triangles(triangles10, dtype, frame=None):
    """The validity rule of spira_trioverlap.h (trioverlap_prepare), bit for bit: returns (q0, g1, g2, m, q1, q2, valid) — the query vertices of
    triangles10 ([q0 q1 q2 mat]; the tenth value is never looked at) in `dtype`, g1 = q1 - q0, g2 = q2 - q0, m = cross(g1, g2), and the library's verdict
    per query: no NaN and nothing infinite among the nine coordinates, m finite and not exactly (0, 0, 0), and — with a frame (centre[3], scale) — the
    origin rule for each of the three vertices."""
    T = np.dtype(dtype).type
    with np.errstate(all="ignore"):
        t = np.array(np.asarray(triangles10).reshape(-1, 10)[:, :9], dtype=T, copy=True)
        valid = ~np.isnan(t).any(axis=1) & np.isfinite(t).all(axis=1)
        q0, q1, q2 = t[:, 0:3], t[:, 3:6], t[:, 6:9]
        g1, g2 = q1 - q0, q2 - q0
        m = _cross3(g1, g2)
        valid &= np.isfinite(m).all(axis=1) & (m != 0).any(axis=1)
        if frame is not None:
            c, scale = np.asarray(frame[0], dtype=T), T(frame[1])
            for q in (q0, q1, q2):
                x = (q - c[None, :]) * scale
                valid &= ((x >= T(-ORIGIN_BOUND)) & (x <= T(ORIGIN_BOUND))).all(axis=1)
    return q0, g1, g2, m, q1, q2, valid


def _tri_axis(s0, s1, s2, p1, p2):
    ok = ~(np.isnan(s0) | np.isnan(s1) | np.isnan(s2) | np.isnan(p1) | np.isnan(p2))
    zero = np.zeros_like(p1)
    lo_s, hi_s = np.minimum(np.minimum(s0, s1), s2), np.maximum(np.maximum(s0, s1), s2)
    lo_q, hi_q = np.minimum(np.minimum(zero, p1), p2), np.maximum(np.maximum(zero, p1), p2)
    return ok & (lo_s <= hi_q) & (lo_q <= hi_s)


def overlap_tri_triangle(v0, e1, e2, q0, g1, g2, m):
    """The numpy twin of spira::overlap_tri_triangle: the scene triangle's v0, e1 = v1 - v0, e2 = v2 - v0 and the query's q0, g1, g2, m (prepare_triangles)
    are arrays [..., 3] of ONE dtype that broadcast against each other (queries x objects: q0[:, None, :] against v0[None, :, :]).  All 20 axes are
    evaluated; the same operations in the same order on the same values as the header.  Returns the candidate verdict, bool [...]."""
    v0, e1, e2, q0, g1, g2, m = (np.asarray(x) for x in (v0, e1, e2, q0, g1, g2, m))
    with np.errstate(all="ignore"):
        u0 = v0 - q0
        u1, u2, e3, g3 = u0 + e1, u0 + e2, e2 - e1, g2 - g1
        n = _cross3(e1, e2)
        shape = np.broadcast(u0[..., 0], e1[..., 0], g1[..., 0]).shape
        ok = np.ones(shape, dtype=bool)
        for k in range(3):
            ok &= _tri_axis(u0[..., k], u1[..., k], u2[..., k], g1[..., k], g2[..., k])
        pn = _dot3(n, u0)
        ok &= _tri_axis(pn, pn, pn, _dot3(n, g1), _dot3(n, g2))
        ok &= (n != 0).any(axis=-1)                                   # zero area: never a candidate
        zero = np.zeros(shape, dtype=u0.dtype)
        ok &= _tri_axis(_dot3(m, u0), _dot3(m, u1), _dot3(m, u2), zero, zero)
        pairs = [(g, e) for g in (g1, g2, g3) for e in (e1, e2, e3)] + [(n, e) for e in (e1, e2, e3)] + [(m, g) for g in (g1, g2, g3)]
        for a, b in pairs:
            L = _cross3(*np.broadcast_arrays(a, b))
            ok &= _tri_axis(_dot3(L, u0), _dot3(L, u1), _dot3(L, u2), _dot3(L, g1), _dot3(L, g2))
    return ok


def overlap_tri_sphere(centre, radius, q0, g1, g2, q1, q2):
    """The numpy twin of spira::overlap_tri_sphere (the sphere is a shell): centre [..., 3], radius [...], and the query's q0, g1, g2 and its own
    vertices q1, q2 (prepare_triangles), broadcasting as overlap_tri_triangle."""
    centre, radius, q0, g1, g2, q1, q2 = (np.asarray(x) for x in (centre, radius, q0, g1, g2, q1, q2))
    with np.errstate(all="ignore"):
        from .query import closest_point_triangle
        _, dmin2 = closest_point_triangle(q0, g1, g2, centre)
        d = []
        for q in (q0, q1, q2):
            r = centre - q
            d.append(_dot3(r, r))
        dmax2 = np.fmax(np.fmax(d[0], d[1]), d[2])
        r2 = radius * radius
        return (dmin2 <= r2) & (dmax2 >= r2)


def overlap_triangles(scene, tris, max_list, any=False, inplace=False, want_trips=False, stream=None):
    """spira_scene_overlap_tri_* (any: spira_scene_overlap_tri_any_*): the objects each triangle of `tris` ([q0 q1 q2 mat], the layout of a scene's
    triangles10; the tenth value is ignored) cuts.  Returns (prim int32 [n, K] — the first max_list candidates in ascending object index, None with
    max_list = 0 —, count [n] of ALL candidates, trips [n] or None), or for `any` the uint8 [n] verdicts (1 cut, 0 not, 255 invalid).  tris: a host array
    [n, 10] — the host form, numpy arrays back — or a torch tensor on the scene's device in the scene's precision — the device form, enqueued on `stream`
    (a torch.cuda.Stream; None: the current one), device tensors back without synchronising (count and trips as int32); `tris` must stay alive until the
    work has run."""
    if isinstance(tris, np.ndarray) or not hasattr(tris, "is_cuda"):
        if any:
            return scene.overlap_tri_any(tris, inplace=inplace)
        return scene.overlap_tri(tris, max_list, inplace=inplace, want_trips=want_trips)
    import torch
    from .query import _device_list, _ptr
    _, n, st = _device_list("overlap_triangles", scene, tris, 10, stream)
    k = int(max_list)
    room = k if 0 < k <= B.MAX_OVERLAP else 1
    with torch.cuda.stream(st):
        if any:
            hit = torch.empty(n, dtype=torch.uint8, device=tris.device)
            scene.overlap_tri_any_device(tris.data_ptr(), n, hit.data_ptr(), st.cuda_stream, inplace=inplace)
            return hit
        prim = torch.empty((n, room), dtype=torch.int32, device=tris.device) if k else None
        count = torch.empty(n, dtype=torch.int32, device=tris.device)
        trips = torch.empty(n, dtype=torch.int32, device=tris.device) if want_trips else None
        scene.overlap_tri_device(tris.data_ptr(), n, k, _ptr(prim), count.data_ptr(), st.cuda_stream, inplace=inplace, d_trips_ptr=_ptr(trips))
    return prim, count, trips


def mesh_pairs(scene, triangles10, max_list=16):
    """The pair list of a second mesh against a scene handle (host arrays): every (query, object) pair — query the row of triangles10, object the scene's
    index, spheres first — that the first max_list candidates of each query hold, as an int64 array [p, 2] in ascending (query, object) order, and a bool
    mask [n] of the queries whose count exceeded the list (their pairs are incomplete: ask again with a finer mesh or take them to the host)."""
    prim, count, _ = overlap_triangles(scene, triangles10, max_list)
    keep = prim >= 0
    qi, slot = np.nonzero(keep)
    return np.stack([qi.astype(np.int64), prim[qi, slot].astype(np.int64)], axis=1), count > np.uint32(max_list)


def meshes_intersect(scene, triangles10):
    """Does any triangle of triangles10 (host array) cut any object of the scene?  The any form; invalid queries cut nothing."""
    return bool((overlap_triangles(scene, triangles10, 0, any=True) == 1).any())
