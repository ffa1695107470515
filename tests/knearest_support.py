"""The yardstick of the K-nearest tests (spira_scene_nearest_k_*): the contract's order by brute force.  For every valid point, every object's d2 and q
(nearest_support.NearScan.d2_all: the numpy twins of the two closest-point functions), those with d2 <= r_max * r_max kept (a NaN never), sorted by
(d2 ascending, object index descending); the first TOP places are kept, which is one more than any K a call may ask for, so every K is a cut of the one
order.  Scenes and point sets are nearest_support's (about 2 100 points per scene: the sessions refill), read-only.

The sets are held to what they are for, here, wherever a test asks for them (conditions): points with more than K candidates, with fewer (some, and
none), and on the duplicate scene candidates tied exactly across the K-th / (K + 1)-th place."""
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
