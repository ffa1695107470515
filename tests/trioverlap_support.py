"""The yardstick of the triangle overlap tests (spira_scene_overlap_tri_* / spira_scene_overlap_tri_any_*): the brute-force scan of the contract
(csrc/spira_trioverlap.h) over the numpy twins of spira_hip.query — every object's candidate verdict from overlap_tri_sphere / overlap_tri_triangle, spheres
[0..) then triangles [0..) in the caller's order; the count of all candidates, the first max_list of them in ascending index (overlap_support.lists) — plus
the query sets of tests/test_trioverlap_cpu.py and tests/test_gpu_trioverlap.py.  Scenes and frames come from overlap_support / nearest_support /
cast_support by import, read-only."""
import functools

import numpy as np

import cast_support as S
import nearest_support as N
import overlap_support as V
from spira_hip import query

MISS, INVALID = S.MISS, S.INVALID
lists = V.lists
scene = V.scene


class TriScan(N.NearScan):
    """The scan over one scene in one precision; the fields and the frame are NearScan's."""

    def candidates(self, tris10, chunk=64):
        """cand bool [n, k] — every query against every object, spheres first; False in the rows of invalid queries — and valid [n]."""
        q0, g1, g2, m, q1, q2, valid = query.prepare_triangles(tris10, self.T, self.frame)
        n, k = len(q0), self.ns + len(self.tri)
        cand = np.zeros((n, k), dtype=bool)
        idx = np.flatnonzero(valid)
        for a in range(0, len(idx), chunk):
            ii = idx[a:a + chunk]
            Q0, G1, G2, M, Q1, Q2 = (x[ii, None] for x in (q0, g1, g2, m, q1, q2))
            if self.ns:
                cand[ii, :self.ns] = query.overlap_tri_sphere(self.sp[None, :, 0:3], self.sp[None, :, 3], Q0, G1, G2, Q1, Q2)
            if len(self.tri):
                cand[ii, self.ns:] = query.overlap_tri_triangle(self.v0[None], self.e1[None], self.e2[None], Q0, G1, G2, M)
        return cand, valid

    def overlap(self, tris10):
        """dict(cand, valid, count uint32 [n], hit uint8 [n]): the contract's count and any form (invalid: 0 and 255)."""
        cand, valid = self.candidates(tris10)
        count = cand.sum(axis=1).astype(np.uint32)
        return dict(cand=cand, valid=valid, count=count, hit=np.where(valid, count > 0, 255).astype(np.uint8))


# ------------------------------------------------------------------ query sets: [n, 10] Float64 (the tenth value is filled in by build_set)
def _tris(q0, q1, q2):
    return np.concatenate([q0, q1, q2, np.ones((len(q0), 1))], axis=1)


def straddling(rng, sc, n, lo=0.01, hi=0.08):
    """Small triangles about points within 2 % of the extent of the surface."""
    ext = S.target_box(sc)[3]
    c = N.near_surface(rng, sc, n, frac=0.02)[:, :3]
    size = rng.uniform(lo, hi, (n, 1)) * ext
    return _tris(c + size * S._unit(rng, n), c + size * S._unit(rng, n), c + size * S._unit(rng, n))


def shifted_in_plane(rng, sc, T, n):
    """The scene's own triangles (as T holds them) moved within their plane by up to 0.6 of their edges."""
    v = S._mesh_vertices(sc, T)[rng.integers(0, len(sc["triangles10"]), n)]
    e1, e2 = v[:, 1] - v[:, 0], v[:, 2] - v[:, 0]
    d = rng.uniform(-0.6, 0.6, (n, 1)) * e1 + rng.uniform(-0.6, 0.6, (n, 1)) * e2
    return _tris(v[:, 0] + d, v[:, 1] + d, v[:, 2] + d)


def sharing(rng, sc, T, n):
    """Copies of the scene's triangles that keep exactly one vertex (even) or one edge (odd) — the values T holds — with the rest moved off the plane."""
    ext = S.target_box(sc)[3]
    v = S._mesh_vertices(sc, T)[rng.integers(0, len(sc["triangles10"]), n)]
    first = rng.integers(0, 3, n)
    v = np.stack([v[np.arange(n), (first + k) % 3] for k in range(3)], axis=1)
    out = v + 0.08 * ext * rng.normal(size=(n, 3, 3))
    out[:, 0] = v[:, 0]
    out[1::2, 1] = v[1::2, 1]
    return _tris(out[:, 0], out[:, 1], out[:, 2])


def slicing(rng, sc, n, proposals=8_000_000):
    """Large triangles (circumradius three extents, about the mesh's middle) in the planes that cut the most objects: of `proposals` / objects random
    planes through the mesh's box, the n that a plane test in Float64 says cross the most triangles and spheres."""
    lo, hi, c, ext = S.target_box(sc)
    v = np.asarray(sc["triangles10"], dtype=np.float64)[:, :9].reshape(-1, 3, 3)
    sp = np.asarray(sc["spheres5"], dtype=np.float64).reshape(-1, 5)
    p = int(min(400_000, max(4 * n, proposals // (len(v) + len(sp)))))
    nrm = S._unit(rng, p)
    off = (nrm * (c + (rng.random((p, 3)) - 0.5) * (hi - lo))).sum(axis=1)
    cut = np.zeros(p, dtype=np.int64)
    for a in range(0, p, 20_000):
        d = np.einsum("nk,tvk->ntv", nrm[a:a + 20_000], v) - off[a:a + 20_000, None, None]
        cut[a:a + 20_000] = ((d.min(axis=2) < 0) & (d.max(axis=2) > 0)).sum(axis=1)
        cut[a:a + 20_000] += (np.abs(nrm[a:a + 20_000] @ sp[:, :3].T - off[a:a + 20_000, None]) < sp[:, 3]).sum(axis=1)
    best = np.argsort(-cut, kind="stable")[:n]
    nrm, off = nrm[best], off[best]
    mid = c - ((nrm * c).sum(axis=1) - off)[:, None] * nrm                               # the middle of the box, dropped onto the plane
    a = S._normalize(S._cross(nrm, S._unit(rng, n)))
    b = S._cross(nrm, a)
    ang = rng.uniform(0, 2 * np.pi, n)[:, None] + np.array([0.0, 2.1, 4.2])[None, :]
    q = mid[:, None, :] + 3.0 * ext * (np.cos(ang)[..., None] * a[:, None, :] + np.sin(ang)[..., None] * b[:, None, :])
    return _tris(q[:, 0], q[:, 1], q[:, 2])


def needles_and_far(rng, sc, n):
    """Even: needles through the mesh's box (two vertices 1e-4 .. 1e-3 of the extent apart, the third across the box); odd: tiny triangles (1e-3 of the
    extent) two to three extents away from the mesh."""
    lo, hi, c, ext = S.target_box(sc)
    a = c + (rng.random((n, 3)) - 0.5) * (hi - lo)
    needle = _tris(a, a + rng.uniform(1e-4, 1e-3, (n, 1)) * ext * S._unit(rng, n), c + (rng.random((n, 3)) - 0.5) * (hi - lo) * 1.4)
    f = c + rng.uniform(2.0, 3.0, (n, 1)) * ext * S._unit(rng, n)
    tiny = _tris(f, f + 1e-3 * ext * S._unit(rng, n), f + 1e-3 * ext * S._unit(rng, n))
    return np.where((np.arange(n) % 2 == 0)[:, None], needle, tiny)


def far_vertices(rng, ss, sc, n):
    """Scenes with a tree: triangles with one vertex (q0, q1, q2 in turn) at 60 .. 64 frame units and the other two at the mesh, each followed by its twin
    whose far vertex is just beyond the origin rule (invalid)."""
    ext = S.target_box(sc)[3]
    rays, axis, sign = S.rays_far(rng, ss, sc, n)
    twins = S.rays_far_outside(rays, axis, sign, ss)
    target = rays[:, :3] + rays[:, 4:7]
    near = np.stack([target + 0.03 * ext * S._unit(rng, n), target + 0.03 * ext * S._unit(rng, n)], axis=1)
    out = np.zeros((2 * n, 10))
    for j, far in enumerate((rays[:, :3], twins[:, :3])):
        v = np.stack([far, near[:, 0], near[:, 1]], axis=1)
        v = np.stack([v[np.arange(n), (k - np.arange(n)) % 3] for k in range(3)], axis=1)      # the far vertex is vertex i mod 3
        out[j::2] = _tris(v[:, 0], v[:, 1], v[:, 2])
    return out


def _grid(frame):
    """(origin, step): points origin + integers * step are exact in both precisions and lie about the frame's centre (no frame: the integers themselves)."""
    if frame is None:
        return np.zeros(3), 1.0
    step = 2.0 ** (np.floor(np.log2(1.0 / float(frame[1]))) - 4)
    return np.round(np.asarray(frame[0], dtype=np.float64) / step) * step, step


def invalid_kinds(T, frame):
    """One query per invalidity cause, each otherwise harmless."""
    fi = np.finfo(T)
    o, s = _grid(frame)
    good = np.concatenate([o + s * np.array([1, 2, -1]), o + s * np.array([4, 1, 0]), o + s * np.array([0, 5, 3]), [1.0]])
    kinds = []
    for k, v in ((0, np.nan), (4, np.nan), (8, np.nan), (1, np.inf), (5, -np.inf), (6, np.inf)):
        r = good.copy(); r[k] = v; kinds.append(r)
    r = good.copy(); r[3:6] = r[0:3]; kinds.append(r)                                            # q1 = q0: a segment
    r = good.copy(); r[3:6] = r[0:3]; r[6:9] = r[0:3]; kinds.append(r)                           # a point
    r = good.copy(); r[6:9] = r[0:3] + 2 * (r[3:6] - r[0:3]); kinds.append(r)                    # collinear, exactly: m = (0, 0, 0)
    big = float(np.sqrt(np.float64(fi.max))) * 4
    r = good.copy(); r[3] = big; r[7] = big; kinds.append(r)                                     # m overflows
    r = good.copy(); r[3] = float(fi.max); r[0] = -float(fi.max); kinds.append(r)                # g1 overflows
    if frame is not None:
        for k in (0, 4, 8):                                                                      # the origin rule, each vertex
            r = good.copy(); r[k] = float(frame[0][k % 3]) + (65.0 if k != 4 else -65.0) / float(frame[1]); kinds.append(r)
    return np.array(kinds)


def interleave_invalid(tris, T, frame, every=7):
    kinds = invalid_kinds(T, frame)
    out = np.array(tris, dtype=np.float64)
    at = np.arange(0, len(out), every)
    out[at] = kinds[np.arange(len(at)) % len(kinds)]
    return out, at


def build_set(ss, sc, seed=191, n_straddle=900, n_shift=200, n_share=240, n_slice=32, n_needle=256, n_far=48, n_mixed=210):
    """The query set of one scene with the scan's answers (header of tests/test_gpu_trioverlap.py).  dict(tris, cand, valid, count, hit, parts,
    invalid_at).  The tenth value of every third query is NaN: it is never read."""
    T = ss.T
    rng = np.random.default_rng(seed)
    parts, rows = {}, []

    def add(name, t):
        a = sum(len(r) for r in rows)
        rows.append(np.asarray(t, dtype=np.float64)); parts[name] = slice(a, a + len(t))
    add("straddle", straddling(rng, sc, n_straddle))
    add("shift", shifted_in_plane(rng, sc, T, n_shift))
    add("share", sharing(rng, sc, T, n_share))
    add("slice", slicing(rng, sc, n_slice))
    add("needle", needles_and_far(rng, sc, n_needle))
    if ss.frame is not None:
        add("far", far_vertices(rng, ss, sc, n_far))
    mixed, at = interleave_invalid(straddling(rng, sc, n_mixed, hi=0.3), T, ss.frame)
    add("mixed", mixed)
    with np.errstate(over="ignore"):
        tris = np.array(np.concatenate(rows), dtype=T).astype(np.float64)             # the values the library sees
    tris[2::3, 9] = np.nan
    ref = ss.overlap(tris)
    return N._freeze(dict(ref, tris=tris, parts=parts, invalid_at=at + parts["mixed"].start))


def conditions(ref):
    """What a query set must reach, asserted (the issue's condition): at least 20 queries with more than 16 candidates, more than 100 valid ones with none,
    more than 100 with 1 .. 4, at least 20 invalid.  Returns the counts."""
    v, c = ref["valid"], ref["count"].astype(np.int64)
    out = dict(many=int((c > 16).sum()), none=int((v & (c == 0)).sum()), few=int(((c >= 1) & (c <= 4)).sum()), invalid=int((~v).sum()))
    assert out["many"] >= 20 and out["none"] > 100 and out["few"] > 100 and out["invalid"] >= 20, out
    return out


@functools.lru_cache(maxsize=None)
def scan_of(name, prec):
    return TriScan(scene(name), prec)


@functools.lru_cache(maxsize=None)
def reference(name, prec):
    return build_set(scan_of(name, prec), scene(name))
