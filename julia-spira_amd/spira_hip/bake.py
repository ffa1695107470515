"""Baking at surface points: irradiance and ambient occlusion through the hemisphere gather (spira_scene_gather_*, spira_scene_gather_visible_*).

A point is [px py pz nx ny nz]; the library draws the cosine-weighted directions of its hemisphere itself (csrc/spira_gather.h), so a bake of n points
at spp samples is one call on n x 6 values.  `hemisphere_rays` restates the library's generator in numpy bit for bit (the same operations in the same
order and precision: tests compare the two by array_equal), with the counter RNG of spira_hip.cameras.
"""
import numpy as np

from . import _binding as B
from . import cameras as _cam

GATHER_BOUNCE = 255      # the bounce index of a gather direction's RNG key: the lens's slot, which no path reaches (max_depth <= 255)


def hemisphere_rays(points6, sample=0, seed=0, key0=0, prec="f32"):
    """The numpy restatement of spira_gather_rays_*: [n, 6] = [p, v], v not normalised; six zeros for an invalid point."""
    npdt = B._dt(prec)[0]
    pts = np.ascontiguousarray(points6, dtype=npdt).reshape(-1, 6)
    n = len(pts)
    tiny = np.finfo(npdt).tiny
    valid, nh = _cam.ray_prepare(pts, prec)
    key = _cam.rng_key(seed, np.uint32(key0) + np.arange(n, dtype=np.uint32), sample, GATHER_BOUNCE)
    q = np.zeros((n, 3), dtype=npdt)
    todo = np.ones(n, dtype=bool)
    with np.errstate(all="ignore"):
        for t in range(1, _cam.K_MAX_TRIES + 1):
            if not todo.any():
                break
            u0, u1, u2 = _cam._rng3_key(key, t, prec, 1.0 / 1048576.0)
            a0, a1, a2 = u0 - npdt(1), u1 - npdt(1), u2 - npdt(1)
            ok = todo & ((a0 * a0 + a1 * a1) + a2 * a2 < npdt(1))
            q[ok, 0], q[ok, 1], q[ok, 2] = a0[ok], a1[ok], a2[ok]
            todo &= ~ok
        qq = (q[:, 0] * q[:, 0] + q[:, 1] * q[:, 1]) + q[:, 2] * q[:, 2]
        small = qq < tiny
        qh = q / np.sqrt(np.where(small, npdt(1), qq))[:, None]
        qh[small] = 0
        out = np.empty((n, 6), dtype=npdt)
        out[:, 0:3] = pts[:, 0:3]
        out[:, 3:6] = nh + qh
        ok_ray, _ = _cam.ray_prepare(out, prec)
    fallback = valid & ~ok_ray
    out[fallback, 3:6] = nh[fallback]
    out[~valid] = 0
    return out


def triangle_points(triangles10, prec="f64"):
    """One point per triangle of triangles10 (n x [v0 v1 v2 material]): the centroid with the unit geometric normal normalize(cross(e1, e2)),
    e1 = v1 - v0, e2 = v2 - v0 — the normal spira_render_features_* defines.  [n, 6] in `prec`; a degenerate triangle gives a zero normal (an invalid point)."""
    npdt = B._dt(prec)[0]
    t = np.ascontiguousarray(triangles10, dtype=np.float64).reshape(-1, 10)
    v0, v1, v2 = t[:, 0:3], t[:, 3:6], t[:, 6:9]
    c = (v0 + v1 + v2) / 3.0
    nrm = np.cross(v1 - v0, v2 - v0)
    length = np.sqrt((nrm * nrm).sum(axis=1))
    with np.errstate(all="ignore"):
        nrm = np.where(length[:, None] > 0, nrm / length[:, None], 0.0)
    return np.ascontiguousarray(np.concatenate([c, nrm], axis=1), dtype=npdt)


def irradiance(scene, points6, spp, max_depth, seed=0, sample0=0, key0=0, flags=0):
    """pi * sum / spp of Scene.gather, [n, 3] in the scene's precision: the cosine-weighted estimate of the irradiance arriving at every point
    (rows of invalid points stay 0)."""
    npdt = B._dt(scene.prec)[0]
    sums = scene.gather(points6, spp, max_depth, seed=seed, sample0=sample0, key0=key0, flags=flags)
    return (sums * npdt(np.pi)) / npdt(spp)


def ambient_occlusion(scene, points6, spp, t_max, t_min=1e-3, seed=0, sample0=0, key0=0, inplace=False):
    """visible / spp of Scene.gather_visible, float64 [n]: the cosine-weighted share of every point's hemisphere that is open within t_max (1: nothing
    near; rows of invalid points stay 0)."""
    counts = scene.gather_visible(points6, spp, t_min=t_min, t_max=t_max, seed=seed, sample0=sample0, key0=key0, inplace=inplace)
    return counts.astype(np.float64) / float(spp)


def snap_to_surface(scene, points6, triangles10, r_max=float("inf"), inplace=False):
    """Snaps points6 (n x [px py pz nx ny nz]) to the scene's surface with Scene.closest_point: the position becomes the nearest surface point within r_max,
    and where that point lies on a triangle the normal becomes that triangle's, triangle_points' normalize(cross(e1, e2)) (triangles10: the mesh the
    handle holds, in the caller's order).  A point whose nearest object is a sphere keeps its normal; a point with nothing within r_max, or an invalid
    one, is left as it is.  Returns (points6 snapped, in the scene's precision; prim int32 [n])."""
    npdt = B._dt(scene.prec)[0]
    out = np.array(points6, dtype=npdt, copy=True).reshape(-1, 6)
    p4 = np.concatenate([out[:, :3], np.full((len(out), 1), r_max, dtype=npdt)], axis=1)
    prim, _, q, _ = scene.closest_point(p4, inplace=inplace, want_dist=False)
    hit = prim >= 0
    out[hit, :3] = q[hit]
    ns = scene.counts[0]
    on_tri = hit & (prim >= ns)
    if on_tri.any():
        nrm = triangle_points(triangles10, scene.prec)[:, 3:6]
        out[on_tri, 3:6] = nrm[prim[on_tri] - ns]
    return out, prim
