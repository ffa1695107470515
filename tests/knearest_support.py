"""The yardstick of the K-nearest tests (spira_scene_nearest_k_*): the contract's order by brute force.  For every valid point, every object's d2 and q
(nearest_support.NearScan.d2_all: the numpy twins of the two closest-point functions), those with d2 <= r_max * r_max kept (a NaN never), sorted by
(d2 ascending, object index descending); the first TOP places are kept, which is one more than any K a call may ask for, so every K is a cut of the one
order.  Scenes and point sets are nearest_support's (about 2 100 points per scene: the sessions refill), read-only.

The sets are held to what they are for, here, wherever a test asks for them (conditions): points with more than K candidates, with fewer (some, and
none), and on the duplicate scene candidates tied exactly across the K-th / (K + 1)-th place.  The second half holds the sets of the edge tests
(tests/test_gpu_knearest_edges.py; tests/test_knearest_edges_cpu.py asserts their premises): the placements of cast_support.FRAMES, r_max at the K-th
distance from far points, the pile of 17-fold coincident triangles, r_max whose square leaves the normal range, and points about the 5 120-triangle tree."""
import functools

import numpy as np

import nearest_support as N
from spira_hip import query

MISS, INVALID = N.MISS, N.INVALID
MAX_NEAR = 16
TOP = MAX_NEAR + 1


def order_of(ns, points4, chunk=128):
    """dict(points, valid, r_max [n] in T, total [n] candidates, prim [n, TOP] (MISS beyond total), d2 [n, TOP], q [n, TOP, 3]) — the order of every point."""
    T = ns.T
    pts, valid = query.prepare_points(points4, T, ns.frame)
    n = len(pts)
    m = ns.ns + len(ns.tri)
    top = min(TOP, m)
    prim, d2, q = np.full((n, TOP), MISS, dtype=np.int32), np.zeros((n, TOP), dtype=T), np.zeros((n, TOP, 3), dtype=T)
    total = np.zeros(n, dtype=np.uint32)
    idx = np.flatnonzero(valid)
    with np.errstate(all="ignore"):
        for a in range(0, len(idx), chunk):
            ii = idx[a:a + chunk]
            p, best0 = pts[ii, :3], pts[ii, 3] * pts[ii, 3]
            qq, dd = ns.d2_all(p)
            ok = dd <= best0[:, None]                                # NaN: never
            assert not np.isinf(dd[ok]).any()                        # (the key below stands for "no candidate")
            total[ii] = ok.sum(axis=1)
            key = np.where(ok, dd, T(np.inf))
            # (d2 ascending, index descending): a stable sort of the objects taken from the last to the first
            o = (m - 1) - np.argsort(key[:, ::-1], axis=1, kind="stable")[:, :top]
            rows = np.arange(len(ii))[:, None]
            used = np.arange(top)[None, :] < total[ii][:, None]
            prim[ii, :top] = np.where(used, o, MISS)
            d2[ii, :top] = np.where(used, dd[rows, o], T(0))
            q[ii, :top] = np.where(used[:, :, None], qq[rows, o], T(0))
    out = dict(points=np.array(points4, dtype=np.float64), valid=valid, r_max=pts[:, 3].copy(), total=total, prim=prim, d2=d2, q=q)
    for a in out.values():
        a.setflags(write=False)
    return out


def cut(ref, K):
    """The contract's outputs at max_near = K: prim int32 [n, K], dist [n, K], point [n, K, 3], count uint32 [n] (the slots filled)."""
    T = ref["d2"].dtype.type
    valid, total = ref["valid"], ref["total"]
    count = np.minimum(total, K).astype(np.uint32)
    used = np.arange(K)[None, :] < count[:, None]
    prim = np.where(used, ref["prim"][:, :K], np.where(valid, MISS, INVALID)[:, None]).astype(np.int32)
    with np.errstate(all="ignore"):
        dist = np.where(used, np.sqrt(ref["d2"][:, :K]), np.where(valid, ref["r_max"], T(0))[:, None]).astype(T)
    point = np.where(used[:, :, None], ref["q"][:, :K], T(0)).astype(T)
    return prim, dist, point, count


@functools.lru_cache(maxsize=None)
def reference(name, prec):
    """The order of nearest_support's point set of the scene."""
    return order_of(N.scan_of(name, prec), N.reference(name, prec)["points"])


def conditions(ref, K, ties=False):
    """What a set must hold for K, asserted: points with more than K candidates, with fewer than K but some (K > 1), with none; ties: candidates tied
    exactly across the K-th / (K + 1)-th place — there the index alone decides who is kept.  Returns the four counts."""
    total, valid = ref["total"].astype(np.int64), ref["valid"]
    more, fewer, none = int((total > K).sum()), int(((total < K) & (total > 0)).sum()), int((valid & (total == 0)).sum())
    assert more >= 64 and none >= 8 and (K == 1 or ties or fewer >= 8), (K, more, fewer, none)      # (ties: the duplicate scene's candidates come in pairs)
    tied = int(((total > K) & (ref["d2"][:, K - 1] == ref["d2"][:, K])).sum())
    assert not ties or tied >= 4, (K, tied)
    return more, fewer, none, tied


@functools.lru_cache(maxsize=None)
def edge_set(name, prec, K, n=64):
    """r_max at the K-th distance: for the first n near-surface points with more than K candidates, the same point with r_max = sqrt(the K-th d2) —
    r_max * r_max rounds, so the K-th object mostly stays and sometimes goes, as the scan says — with r_max one ulp below — the K-th object and everything
    tied with it goes: fewer than K slots are filled — and the vertex and edge points with r_max = 0.  The order of the set, and parts: name -> slice."""
    ns, base, sup = N.scan_of(name, prec), reference(name, prec), N.reference(name, prec)
    T = ns.T
    near = sup["parts"]["near"]
    sel = np.flatnonzero(base["total"][near] > K)[:n] + near.start
    assert len(sel) == n
    with np.errstate(all="ignore"):
        r = np.sqrt(base["d2"][sel, K - 1])
    same, below = base["points"][sel].copy(), base["points"][sel].copy()
    same[:, 3] = r
    below[:, 3] = np.nextafter(r, T(0))
    zero = base["points"][sup["parts"]["edges"]][:n].copy()
    zero[:, 3] = 0.0
    out = dict(order_of(ns, np.concatenate([same, below, zero])))
    out["parts"] = dict(same=slice(0, n), below=slice(n, 2 * n), zero=slice(2 * n, 2 * n + len(zero)))
    t = out["total"].astype(np.int64)
    assert (t[out["parts"]["same"]] >= K).mean() > 0.5
    assert (t[out["parts"]["below"]] < K).all()
    if name != "dup":                                                # (there the K-th object's twin goes with it)
        assert (t[out["parts"]["below"]] == K - 1).mean() > 0.5
    assert (t[out["parts"]["zero"]] > 0).any() and (t[out["parts"]["zero"]] == 0).any()
    return out


# ------------------------------------------------------------------ the sets of the edge tests (test_knearest_edges_cpu.py, test_gpu_knearest_edges.py)
FRAME_SET = dict(n_near=256, n_box=192, n_edge=64, n_far=48, n_r=32)


@functools.lru_cache(maxsize=None)
def frame_case(prec, fi, how):
    """nearest_support.frame_mesh — the blob mesh in placement fi of cast_support.FRAMES, as built, after an update, after a rebuild — with the point set
    test_gpu_nearest._frame_case gives it and the order of those points in the frame that holds.  Returns (A, B, the scan of B, the set, the order)."""
    A, B, frame = N.frame_mesh(prec, fi, how)
    ns = N.NearScan(B, prec, frame=frame)
    pts = N.build_set(ns, B, seed=33 + fi, **FRAME_SET)
    return A, B, ns, pts, order_of(ns, pts["points"])


def far_valid(pts):
    """The indices of a set's valid far points (the even ones) and of their invalid twins."""
    far = np.arange(pts["parts"]["far"].start, pts["parts"]["far"].stop)
    return far[0::2], far[1::2]


@functools.lru_cache(maxsize=None)
def far_edge_set(prec, fi, K):
    """edge_set's construction at 60 .. 64 frame units: the valid far points of frame_case(prec, fi, "create") with r_max = sqrt(the K-th d2) (same) and one
    ulp below (below).  There d2 is in the thousands of normalised units and the bound STARTS at a candidate's distance: near_bestn's rounding decides."""
    _, _, ns, pts, base = frame_case(prec, fi, "create")
    T = ns.T
    sel, _ = far_valid(pts)
    assert len(sel) == FRAME_SET["n_far"] and (base["total"][sel] > K).all()
    with np.errstate(all="ignore"):
        r = np.sqrt(base["d2"][sel, K - 1])
    same, below = base["points"][sel].copy(), base["points"][sel].copy()
    same[:, 3] = r
    below[:, 3] = np.nextafter(r, T(0))
    n = len(sel)
    out = dict(order_of(ns, np.concatenate([same, below])))
    out["parts"] = dict(same=slice(0, n), below=slice(n, 2 * n))
    t = out["total"].astype(np.int64)
    assert out["valid"].all()
    assert (t[out["parts"]["same"]] >= K).mean() > 0.5
    assert (t[out["parts"]["below"]] < K).all()
    return out


PILE_COPIES = 17
PILE_SET = dict(seed=52, n_near=256, n_box=192, n_edge=64, n_far=48, n_r=32)


@functools.lru_cache(maxsize=None)
def pile_scene(copies=PILE_COPIES):
    """nearest_support.ico_scene(33)'s 33 triangles `copies` times, interleaved by one permutation of default_rng(51), with its ground sphere: a tree, and
    every triangle candidate is tied `copies`-fold — more often than the longest list is long."""
    s = N.ico_scene(33)
    t = np.tile(s["triangles10"], (copies, 1))[np.random.default_rng(51).permutation(33 * copies)]
    t.setflags(write=False)
    return dict(s, triangles10=t)


@functools.lru_cache(maxsize=None)
def pile_scan(prec):
    return N.NearScan(pile_scene(), prec)


@functools.lru_cache(maxsize=None)
def pile_set(prec):
    return N.build_set(pile_scan(prec), pile_scene(), **PILE_SET)


@functools.lru_cache(maxsize=None)
def pile_ref(prec):
    return order_of(pile_scan(prec), pile_set(prec)["points"])


def pile_conditions(ref, K):
    """What the pile is for, asserted for K: points with more than K candidates; for K >= 2 every one of them tied across the K-th / (K + 1)-th place; on
    most the whole list one run of equal d2 (d2[0] == d2[K]: every later arrival with that d2 is decided by index alone); valid points with no candidate.
    Returns the four counts."""
    total, valid, d2 = ref["total"].astype(np.int64), ref["valid"], ref["d2"]
    more = total > K
    tied = more & (d2[:, K - 1] == d2[:, K])
    run = more & (d2[:, 0] == d2[:, K])
    none = valid & (total == 0)
    assert more.sum() >= 700 and (K == 1 or tied.sum() == more.sum()) and run.sum() >= 600 and none.sum() >= 32, (K, more.sum(), tied.sum(), run.sum(), none.sum())
    return int(more.sum()), int(tied.sum()), int(run.sum()), int(none.sum())


def extreme_radii(T):
    """Four r_max of T: (a) the largest whose square is finite, (b) the first whose square is +Inf, (c) one whose square underflows to 0, (d) one whose
    square is subnormal."""
    fi = np.finfo(T)
    with np.errstate(all="ignore"):
        a = T(np.sqrt(np.float64(fi.max)))
        while np.isinf(a * a):
            a = np.nextafter(a, T(0))
        while np.isfinite(np.nextafter(a, T(np.inf)) * np.nextafter(a, T(np.inf))):
            a = np.nextafter(a, T(np.inf))
        b = np.nextafter(a, T(np.inf))
        c = T(np.ldexp(1.0, (fi.minexp - fi.nmant) // 2 - 4))        # the square is 2^-8 of the smallest subnormal number
        d = T(np.ldexp(1.0, (fi.minexp - 8) // 2))                   # the square is about 2^-8 of the smallest normal number
        assert np.isfinite(a * a) and np.isinf(b * b) and np.isfinite(b) and c > 0 and c * c == 0 and 0 < d * d < fi.tiny
    return dict(a=a, b=b, c=c, d=d)


@functools.lru_cache(maxsize=None)
def extreme_radius_set(name, prec, n=32):
    """n vertex and edge-midpoint points (nearest_support.on_vertices_and_edges, default_rng(53)) of the scene — "pile" or a name of nearest_support — each
    with the four r_max of extreme_radii: near_load squares r_max in T.  (a), (b): every object is a candidate; (c), (d): only the objects at d2 = 0.  The
    order of the 4 n points and parts: "a" .. "d" -> slice."""
    sc, ns = (pile_scene(), pile_scan(prec)) if name == "pile" else (N.scene(name), N.scan_of(name, prec))
    T = ns.T
    p = N.on_vertices_and_edges(np.random.default_rng(53), sc, T, n)
    rows, parts = [], {}
    for k, (key, r) in enumerate(extreme_radii(T).items()):
        q = p.copy()
        q[:, 3] = float(r)
        rows.append(q); parts[key] = slice(k * n, (k + 1) * n)
    out = dict(order_of(ns, np.concatenate(rows)))
    out["parts"] = parts
    t, m = out["total"].astype(np.int64), ns.ns + len(ns.tri)
    assert out["valid"].all() and np.array_equal(out["r_max"], np.concatenate(rows)[:, 3].astype(T))
    for key in "ab":
        assert (t[parts[key]] == m).all(), (key, t[parts[key]])
    for key in "cd":
        assert (t[parts[key]] > 0).any() and (t[parts[key]] == 0).any() and t[parts[key]].max() < m, (key, t[parts[key]])
    return out


@functools.lru_cache(maxsize=None)
def deep_set(prec):
    """256 points of nearest_support's s4_4 (5 120 triangles, one level deeper than s4_3): 128 near-surface, 96 in the grown box, 32 far (16 valid, their 16
    twins invalid), r_max +Inf.  The order and parts."""
    sc, ns = N.scene("s4_4"), N.scan_of("s4_4", prec)
    rng = np.random.default_rng(57)
    rows = [N.near_surface(rng, sc, 128), N.in_box(rng, sc, 96), N.far_points(rng, ns, sc, 16)]
    out = dict(order_of(ns, np.array(np.concatenate(rows), dtype=ns.T).astype(np.float64)))
    out["parts"] = dict(near=slice(0, 128), box=slice(128, 224), far=slice(224, 256))
    return out
