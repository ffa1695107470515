"""Baking at surface points: irradiance and ambient occlusion through the hemisphere gather (spira_scene_gather_*, spira_scene_gather_visible_*); and
light probes at free points: nine spherical-harmonic coefficients of the incoming radiance through spira_scene_probe_sh_* (csrc/spira_probe.h), with
`sphere_rays` and `sh9` the numpy twins of its generator and its basis.

A point is [px py pz nx ny nz]; the library draws the cosine-weighted directions of its hemisphere itself (csrc/spira_gather.h), so a bake of n points
at spp samples is one call on n x 6 values.  `hemisphere_rays` restates the library's generator in numpy bit for bit (the same operations in the same
order and precision: tests compare the two by array_equal), with the counter RNG of spira_hip.cameras.
"""
import numpy as np

from . import _binding as B
from . import cameras as _cam

GATHER_BOUNCE = 255      # the bounce index of a gather direction's RNG key: the lens's slot, which no path reaches (max_depth <= 255)


def _ball_draw(n, sample, seed, key0, prec):
    """q of points 0 .. n - 1 (keys key0 + k) and `sample`: the first of tries 1 .. 64 under bounce 255 that lies in the unit ball, else 0.  [n, 3]."""
    npdt = B._dt(prec)[0]
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
    return q


def hemisphere_rays(points6, sample=0, seed=0, key0=0, prec="f32"):
    """The numpy restatement of spira_gather_rays_*: [n, 6] = [p, v], v not normalised; six zeros for an invalid point."""
    npdt = B._dt(prec)[0]
    pts = np.ascontiguousarray(points6, dtype=npdt).reshape(-1, 6)
    n = len(pts)
    tiny = np.finfo(npdt).tiny
    valid, nh = _cam.ray_prepare(pts, prec)
    q = _ball_draw(n, sample, seed, key0, prec)
    with np.errstate(all="ignore"):
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


# ---------------------------------------------------------------- light probes (csrc/spira_probe.h)
SH9_C = (0.28209479177387814, 0.4886025119029199, 1.0925484305920792, 0.31539156525252005, 0.5462742152960396)      # c0 .. c4, each rounded to T once
SH9_BAND = (0, 1, 1, 1, 2, 2, 2, 2, 2)                                         # the band of Y_j
SH9_COSINE = (np.pi, 2.0 * np.pi / 3.0, np.pi / 4.0)                           # the cosine lobe's factor per band


def sphere_rays(points3, sample=0, seed=0, key0=0, prec="f32"):
    """The numpy restatement of spira_probe_rays_*: [n, 6] = [p, qh], qh uniform on the unit sphere; six zeros for an invalid point."""
    npdt = B._dt(prec)[0]
    pts = np.ascontiguousarray(points3, dtype=npdt).reshape(-1, 3)
    n = len(pts)
    q = _ball_draw(n, sample, seed, key0, prec)
    with np.errstate(all="ignore"):
        valid = np.all((pts - pts) == 0, axis=1)
        qq = (q[:, 0] * q[:, 0] + q[:, 1] * q[:, 1]) + q[:, 2] * q[:, 2]
        small = qq < np.finfo(npdt).tiny
        qh = q / np.sqrt(np.where(small, npdt(1), qq))[:, None]
    qh[small] = (0, 0, 1)
    out = np.concatenate([pts, qh], axis=1)
    out[~valid] = 0
    return out


def sh9(d):
    """The numpy restatement of spira_sh9_basis_*: Y_0 .. Y_8 at the unit directions d ([..., 3]) as [..., 9], the same operations in the same order in
    d's dtype (float32 or float64)."""
    d = np.asarray(d)
    T = d.dtype.type
    c0, c1, c2, c3, c4 = (T(c) for c in SH9_C)
    x, y, z = d[..., 0], d[..., 1], d[..., 2]
    Y = np.empty(d.shape[:-1] + (9,), dtype=d.dtype)
    Y[..., 0] = c0
    Y[..., 1] = c1 * y
    Y[..., 2] = c1 * z
    Y[..., 3] = c1 * x
    Y[..., 4] = c2 * (x * y)
    Y[..., 5] = c2 * (y * z)
    Y[..., 6] = c3 * (T(3) * (z * z) - T(1))
    Y[..., 7] = c2 * (x * z)
    Y[..., 8] = c4 * (x * x - y * y)
    return Y


def light_probes(scene, points3, spp, max_depth, seed=0, sample0=0, key0=0, flags=0):
    """(4 pi / spp) * sums of Scene.probe_sh, [n, 9, 3] in the scene's precision: the coefficients of the radiance arriving at every point on the nine
    real spherical harmonics of bands 0 .. 2 (rows of invalid points stay 0).  sh9_radiance and sh9_irradiance read them."""
    npdt = B._dt(scene.prec)[0]
    sums = scene.probe_sh(points3, spp, max_depth, seed=seed, sample0=sample0, key0=key0, flags=flags)
    return (sums * npdt(4.0 * np.pi)) / npdt(spp)


def probe_grid(lo, hi, dims, prec="f32"):
    """The centres of the dims = (nx, ny, nz) cells of the box [lo, hi], [n, 3] in `prec`, x slowest: query.voxel_boxes' arithmetic."""
    from . import query as _query
    return np.ascontiguousarray(_query.voxel_boxes(lo, hi, dims, B._dt(prec)[0])[:, 0:3])


def probes_outside(scene, points3):
    """bool [n]: True where a probe lies in free space — not inside a sphere or the closed mesh (query.inside_points).  Drop the others before baking."""
    from . import query as _query
    return ~_query.inside_points(scene, np.asarray(points3))


def _sh9_sum(coeffs, dirs, weights):
    c = np.asarray(coeffs)
    Y = sh9(np.asarray(dirs, dtype=c.dtype)) * np.asarray(weights, dtype=c.dtype)
    return (c * Y[..., :, None]).sum(axis=-2)


def sh9_radiance(coeffs, dirs):
    """sum_j coeffs_j Y_j(dirs): the radiance the coefficients ([n, 9, 3] or [9, 3]) stand for, along the unit directions dirs ([n, 3] or [3])."""
    return _sh9_sum(coeffs, dirs, np.ones(9))


def sh9_irradiance(coeffs, normals):
    """The irradiance at a surface of unit normal `normals` ([n, 3] or [3]) under the radiance of coeffs ([n, 9, 3] or [9, 3]): the convolution with the
    clamped cosine lobe, sum_j A_band(j) coeffs_j Y_j(n) with A = pi, 2 pi / 3, pi / 4."""
    return _sh9_sum(coeffs, normals, [SH9_COSINE[b] for b in SH9_BAND])
