"""The yardstick of the sphere-sweep tests (spira_scene_sweep_* / spira_scene_sweep_blocked_*): the brute-force scan of the contract (csrc/spira_sweep.h)
over the numpy twins of spira_hip.query — every object's t_k and q_k from sweep_sphere_sphere / sweep_sphere_triangle, spheres [0..) then triangles [0..) in
the caller's order, the candidates within [t_min, t_max], the minimal t, ties to the LATER object — with the outputs of the contract (point, normal), plus
the sweep sets of tests/test_sweep_cpu.py and tests/test_gpu_sweep.py.  Scenes and frames come from nearest_support / cast_support by import, read-only.

Why the minimum with ties to the last index is the scan: the sequential scan takes object k when !(t_k < t_min || t_k > closest) and then closest = t_k; it
ends at the smallest t_k within [t_min, t_max], and every object AT that t passes when the scan reaches it while nothing after the last of them does."""
import functools

import numpy as np

import cast_support as S
import nearest_support as N
from spira_hip import query

MISS, INVALID = S.MISS, S.INVALID


class SweepScan(N.NearScan):
    """The scan over one scene in one precision; the fields and the frame are NearScan's."""

    def contacts(self, o, d, r, t_min, t_max):
        """t [n, k], q [n, k, 3], hit [n, k] of every sweep against every object, spheres first."""
        ts, qs, hs = [], [], []
        a = (o[:, None, :], d[:, None, :], r[:, None], t_min[:, None], t_max[:, None])
        if self.ns:
            t, q, h = query.sweep_sphere_sphere(self.sp[None, :, 0:3], self.sp[None, :, 3], *a)
            ts.append(t); qs.append(q); hs.append(h)
        if len(self.tri):
            t, q, h = query.sweep_sphere_triangle(self.v0[None], self.e1[None], self.e2[None], *a)
            ts.append(t); qs.append(q); hs.append(h)
        return np.concatenate(ts, axis=1), np.concatenate(qs, axis=1), np.concatenate(hs, axis=1)

    def sweep(self, rays8, radii, chunk=128):
        """prim int32 [n], t [n], point [n, 3], normal [n, 3], valid [n]: the contract (miss: -1, t_max copied, 0, 0; invalid: -3, 0, 0, 0)."""
        T = self.T
        rays, rad, valid = query.prepare_sweeps(rays8, radii, T, self.frame)
        n = len(rays)
        prim, t, point, normal = np.full(n, INVALID, dtype=np.int32), np.zeros(n, dtype=T), np.zeros((n, 3), dtype=T), np.zeros((n, 3), dtype=T)
        idx = np.flatnonzero(valid)
        with np.errstate(all="ignore"):
            for a in range(0, len(idx), chunk):
                ii = idx[a:a + chunk]
                o, d, t_min, t_max, r = rays[ii, 0:3], rays[ii, 4:7], rays[ii, 3], rays[ii, 7], rad[ii]
                tk, qk, hit = self.contacts(o, d, r, t_min, t_max)
                key = np.where(hit, tk, T(np.inf))
                m = key.min(axis=1)
                any_ = hit.any(axis=1)
                at = hit & (tk == m[:, None])
                last = tk.shape[1] - 1 - np.argmax(at[:, ::-1], axis=1)
                q = qk[np.arange(len(ii)), last]
                tw = np.where(any_, m, t_max)
                rv = (o + d * tw[:, None]) - q
                l = np.sqrt(query._dot3(rv, rv))
                nrm = np.where((l >= np.finfo(T).tiny)[:, None], rv / l[:, None], -d)
                prim[ii] = np.where(any_, last, MISS)
                t[ii] = tw
                point[ii] = np.where(any_[:, None], q, T(0))
                normal[ii] = np.where(any_[:, None], nrm, T(0))
        return prim, t, point, normal, valid


# ------------------------------------------------------------------ sweep sets: rays [n, 8] and radii [n], Float64
def _rays(o, d, t_min=0.0, t_max=np.inf):
    n = len(o)
    return np.concatenate([o, np.full((n, 1), t_min), d, np.full((n, 1), t_max)], axis=1)


def head_on(rng, sc, n, lo=0.01, hi=0.10, dist=1.5):
    """From c + dist ext u toward random surface points, the direction scaled so that normalisation matters; r uniform in [lo, hi] ext."""
    _, _, c, ext = S.target_box(sc)
    o = c + dist * ext * S._unit(rng, n)
    return _rays(o, 2.3 * (N.surface_points(rng, sc, n) - o)), rng.uniform(lo, hi, n) * ext


def grazing(rng, sc, n):
    """Paths tangent to the surface: through p + s r nrm along a direction perpendicular to nrm, for a surface point p with its normal nrm (a triangle's,
    a small sphere's), s = +-(0.9 .. 1.1) — the ball passes p at about its radius (or, on the inner side of a closed mesh, runs inside it).  The path
    starts 1.5 extents before p and is 3 extents long.  Only triangles with area are drawn: a segment or a point has no normal, and a NaN sweep would
    quietly join the invalid ones (a mesh whose triangles all have area draws exactly what it drew before)."""
    ext = S.target_box(sc)[3]
    tri = sc.get("triangles10")
    if tri is not None and len(tri):
        v = np.asarray(tri, dtype=np.float64)[:, :9].reshape(-1, 3, 3)
        with_area = np.flatnonzero(np.cross(v[:, 1] - v[:, 0], v[:, 2] - v[:, 0]).any(axis=1))
        v = v[with_area[rng.integers(0, len(with_area), n)]]
        a = rng.uniform(0.05, 0.9, (n, 1)); b = rng.uniform(0.02, 0.95, (n, 1)) * (1 - a)
        p = v[:, 0] + a * (v[:, 1] - v[:, 0]) + b * (v[:, 2] - v[:, 0])
        nrm = np.cross(v[:, 1] - v[:, 0], v[:, 2] - v[:, 0])
    else:
        sp = np.asarray(sc["spheres5"], dtype=np.float64)
        sp = sp[sp[:, 3] < 10][rng.integers(0, (sp[:, 3] < 10).sum(), n)]
        nrm = S._unit(rng, n)
        p = sp[:, :3] + sp[:, 3:4] * nrm
    nrm = nrm / np.linalg.norm(nrm, axis=1)[:, None]
    tau = np.cross(nrm, S._unit(rng, n))
    tau /= np.linalg.norm(tau, axis=1)[:, None]
    r = rng.uniform(0.01, 0.10, n) * ext
    off = r * rng.uniform(0.9, 1.1, n) * np.where(rng.random(n) < 0.5, -1.0, 1.0)
    return _rays(p + off[:, None] * nrm - 1.5 * ext * tau, 2.3 * tau, t_max=3.0 * ext), r


def overlapping(rng, sc, n, frac=0.05):
    """Origins within half a radius of the surface, r = frac ext (several triangles of the finer meshes), random directions."""
    ext = S.target_box(sc)[3]
    o = N.near_surface(rng, sc, n, frac=0.5 * frac)[:, :3]
    return _rays(o, S._unit(rng, n)), np.full(n, frac * ext)


def in_box(rng, sc, n):
    ext = S.target_box(sc)[3]
    return _rays(N.in_box(rng, sc, n)[:, :3], S._unit(rng, n)), rng.uniform(0.01, 0.10, n) * ext


def inside_spheres(rng, sc, n):
    """Origins inside the scene's spheres, near the shell on its upper side (the ground sphere's centre is far below the origin rule), r below the
    sphere's radius: the R - r root."""
    sp = np.asarray(sc["spheres5"], dtype=np.float64)
    ext = S.target_box(sc)[3]
    s = sp[np.arange(n) % len(sp)]
    u = S._unit(rng, n) * 0.2 + np.array([0.0, 1.0, 0.0])
    u /= np.linalg.norm(u, axis=1)[:, None]
    u = np.where((s[:, 3] >= 10)[:, None], u, S._unit(rng, n))
    o = s[:, :3] + s[:, 3:4] * rng.uniform(0.5, 0.9, (n, 1)) * u
    return _rays(o, S._unit(rng, n)), np.minimum(0.08 * s[:, 3], 0.05 * ext)


def radius_bound(ss):
    """The largest radius of T the rule accepts in the scan's frame, and the next value of T above it."""
    T = ss.T
    scale = T(ss.frame[1])
    ok = lambda r: bool((r + r * T(2.0 ** -10)) * scale <= T(query.SWEEP_RADIUS_BOUND))
    r = T(T(query.SWEEP_RADIUS_BOUND) / scale / T(1 + 2.0 ** -10))
    while not ok(r):
        r = np.nextafter(r, T(0))
    while ok(np.nextafter(r, T(np.inf))):
        r = np.nextafter(r, T(np.inf))
    return r, np.nextafter(r, T(np.inf))


def at_radius_bound(rng, ss, sc, n):
    """Balls as large as the rule allows (even sweeps: the last valid radius; odd: the first invalid one) from diagonal directions, so that every origin
    coordinate stays within the origin rule, aimed at the mesh."""
    r_in, r_out = radius_bound(ss)
    c, ext = np.asarray(ss.frame[0], dtype=np.float64), 1.0 / float(ss.frame[1])
    u = np.where(rng.random((n, 3)) < 0.5, -1.0, 1.0) * rng.uniform(0.5, 0.62, (n, 3))
    u[:, 1] = np.abs(u[:, 1])
    u /= np.linalg.norm(u, axis=1)[:, None]
    o = c + (float(r_in) + 1.5 * ext) * u
    r = np.where(np.arange(n) % 2 == 0, float(r_in), float(r_out))
    return _rays(o, N.surface_points(rng, sc, n) - o), r


def corner_sweeps(rng, ss, sc, n):
    """The corner of both rules at once: every origin coordinate at 60 .. 64 frame units (y above), the radius the last valid one, aimed at the mesh —
    the longest paths through the largest grown boxes the walk can meet."""
    r_in, _ = radius_bound(ss)
    c, unit = np.asarray(ss.frame[0], dtype=np.float64), 1.0 / float(ss.frame[1])
    off = rng.uniform(60.0, 64.0, (n, 3)) * np.where(rng.random((n, 3)) < 0.5, -1.0, 1.0)
    off[:, 1] = np.abs(off[:, 1])
    o = (c + off * unit).astype(ss.T).astype(np.float64)
    return _rays(o, N.surface_points(rng, sc, n) - o), np.full(n, float(r_in))


def big_balls(rng, ss, sc, n):
    """r of 1 .. 4 frame units from above (clear of the ground sphere), aimed at the mesh."""
    c, unit = np.asarray(ss.frame[0], dtype=np.float64), 1.0 / float(ss.frame[1])
    r = rng.uniform(1.0, 4.0, n) * unit
    u = S._unit(rng, n) * 0.5 + np.array([0.0, 1.0, 0.0])
    u /= np.linalg.norm(u, axis=1)[:, None]
    o = c + (r + 2.0 * unit)[:, None] * u
    return _rays(o, N.surface_points(rng, sc, n) - o), r


def far_sweeps(rng, ss, sc, n):
    """Valid sweeps from 60 .. 64 frame units (cast_support.rays_far) interleaved with their invalid twins just outside the bound; r = 2 % of the extent."""
    rays, axis, sign = S.rays_far(rng, ss, sc, n)
    twins = S.rays_far_outside(rays, axis, sign, ss)
    ext = S.target_box(sc)[3]
    return np.stack([rays, twins], axis=1).reshape(-1, 8), np.full(2 * n, 0.02 * ext)


def invalid_kinds(T, frame):
    """One sweep per invalidity cause: cast's invalid rays with a good radius, then a good ray with each bad radius."""
    rays = S.invalid_kinds(T, frame)
    c0 = np.zeros(3) if frame is None else np.asarray(frame[0], dtype=np.float64)
    u = 1.0 if frame is None else 1.0 / float(frame[1])
    good = np.concatenate([c0 + np.array([0.1, 1.0, 0.5]) * u, [0.0], [0.2, -0.5, -1.0], [np.inf]])
    bad_r = [np.nan, np.inf, -np.inf, -1e-3 * u] + ([66.0 * u] if frame is not None else [])
    return np.concatenate([rays, np.tile(good, (len(bad_r), 1))]), np.concatenate([np.full(len(rays), 0.05 * u), bad_r])


def interleave_invalid(rays, radii, T, frame, every=7):
    k_rays, k_rad = invalid_kinds(T, frame)
    rays, radii = np.array(rays, dtype=np.float64), np.array(radii, dtype=np.float64)
    at = np.arange(0, len(rays), every)
    rays[at], radii[at] = k_rays[np.arange(len(at)) % len(k_rays)], k_rad[np.arange(len(at)) % len(k_rad)]
    return rays, radii, at


def build_set(ss, sc, seed=71, n_head=448, n_graze=256, n_over=256, n_box=256, n_axis=96, n_far=64, n_big=96, n_bound=64, n_in=64, n_win=96, n_zero=64, n_corner=48):
    """The sweep set of one scene with the scan's answers, about 2 000 sweeps (header of tests/test_gpu_sweep.py).  dict(rays, radii, prim, t, point, normal,
    valid, parts, sel, invalid_at) — parts: name -> slice."""
    T = ss.T
    rng = np.random.default_rng(seed)
    parts, rows, rads = {}, [], []

    def add(name, rr):
        a = sum(len(x) for x in rows)
        rows.append(np.asarray(rr[0], dtype=np.float64)); rads.append(np.asarray(rr[1], dtype=np.float64)); parts[name] = slice(a, a + len(rr[0]))
    ext = S.target_box(sc)[3]
    has_tri = len(ss.tri) > 0
    add("head", head_on(rng, sc, n_head))
    add("graze", grazing(rng, sc, n_graze))
    add("over", overlapping(rng, sc, n_over))
    add("box", in_box(rng, sc, n_box))
    z = head_on(rng, sc, n_zero)
    add("zero", (z[0], np.zeros(n_zero)))
    if has_tri:
        v = N.on_vertices_and_edges(rng, sc, T, n_zero)[:, :3]          # r = 0 on a vertex or an edge midpoint: d2_0 = 0 or a rounding above it
        add("zero_on", (_rays(v, S._unit(rng, n_zero)), np.zeros(n_zero)))
        add("axis", (S.rays_axis(rng, sc, n_axis, T), np.full(n_axis, 0.02 * ext)))
    if ss.ns:
        add("inside", inside_spheres(rng, sc, n_in))
    if ss.frame is not None:
        add("far", far_sweeps(rng, ss, sc, n_far))
        add("big", big_balls(rng, ss, sc, n_big))
        add("bound", at_radius_bound(rng, ss, sc, n_bound))
        add("corner", corner_sweeps(rng, ss, sc, n_corner))
    base, brad = np.array(np.concatenate(rows), dtype=T).astype(np.float64), np.array(np.concatenate(rads), dtype=T).astype(np.float64)      # what the library sees
    prim, t, _, _, _ = ss.sweep(base, brad)
    head = parts["head"]
    sel = np.flatnonzero((prim[head] >= 0) & (t[head] > 0))[:n_win] + head.start
    same, below, beyond = base[sel].copy(), base[sel].copy(), base[sel].copy()
    same[:, 7] = t[sel]
    below[:, 7] = np.nextafter(t[sel], T(0))
    beyond[:, 3] = np.nextafter(t[sel], T(np.inf))
    rows, rads = [base], [brad]
    add("same", (same, brad[sel])); add("below", (below, brad[sel])); add("beyond", (beyond, brad[sel]))
    mixed = interleave_invalid(base[parts["box"]][:140], brad[parts["box"]][:140], T, ss.frame)
    add("mixed", mixed[:2])
    rays, radii = np.array(np.concatenate(rows), dtype=T).astype(np.float64), np.array(np.concatenate(rads), dtype=T).astype(np.float64)
    prim, t, point, normal, valid = ss.sweep(rays, radii)
    return N._freeze(dict(rays=rays, radii=radii, prim=prim, t=t, point=point, normal=normal, valid=valid, parts=parts, sel=sel,
                          invalid_at=mixed[2] + parts["mixed"].start))


scene = N.scene


@functools.lru_cache(maxsize=None)
def scan_of(name, prec):
    return SweepScan(N.scene(name), prec)


@functools.lru_cache(maxsize=None)
def reference(name, prec):
    return build_set(scan_of(name, prec), N.scene(name))
