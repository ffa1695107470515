"""GPU: every tree walk of a scene handle held to its brute-force scan on the hostile meshes of tests/hostile_support.py — collapsed triangles, scales a
thousand times apart, needles through the whole box, a mesh without extent on one axis, 200 copies of one triangle (all Morton keys equal), clusters that
halve forty times (a tree 8 levels deep, its late clusters points in Float32), and a soup updated to a permutation of itself (a refit on a useless
topology).  tests/test_hostile_meshes_cpu.py asserts from the yardsticks alone what the sets reach.

One handle per (mesh, precision, how) — created, created on the shrunk pose and updated, or rebuilt — and all seven queries on it, each compared bit for
bit with its yardstick through the per-query modules' own _check helpers (sessions and in place, the staging poisoned with an all-NaN call before every
compared call): cast and occluded, cast_hits at K = 4 with and without count_all, closest_point, nearest_k at K = 4 and 16 and count_within, sweep and
sweep_blocked, overlap_box at K = 8 and overlap_any, signed_distance and its sign-only form; then the identities between the queries on the same handle.
A second test holds the render walk to the oracle on the same meshes.  The trips are printed for docs/experiments.md; only their equality between the two
organisations is asserted, where the query's own module asserts it."""
import contextlib

import numpy as np
import pytest

import cast_support as S
import hostile_support as X
import knearest_support as KS
import test_gpu_cast as GC
import test_gpu_cast_edges as GCE
import test_gpu_hits as GH
import test_gpu_knearest as GK
import test_gpu_nearest as GN
import test_gpu_overlap as GO
import test_gpu_sdf as GD
import test_gpu_sweep as GW
from spira_hip import query

pytestmark = pytest.mark.gpu

PRECS = ["f32", "f64"]
_bits = GN._bits


@contextlib.contextmanager
def _handle(gpu, name, prec, how):
    first, target = X.poses(name, how)
    with gpu.Scene(X.SPHERES, X.MATERIALS, np.array(first), prec) as h:
        if how == "update":
            h.update(triangles10=np.array(target))
        elif how == "rebuild":
            h.rebuild(np.array(target))
        yield h


def _report(name, prec, how, what, trips):
    for org, t in zip(("sessions", "in place"), trips):
        print("TRIPS %s %s %s %s %s: mean %.2f max %d" % (name, prec, how, what, org, t.mean(), t.max()))


def _same_walk(trips):
    assert np.array_equal(trips[0], trips[1])                        # the same walk, whatever the organisation


def _cast(h, st):
    ref = st["cast"]
    for ip in (False, True):
        GCE._poison(h, len(ref["rays"]))
        GC._check_against(h, ref["sc"], ref, inplace=(ip,))


def _hits(h, st):
    GH._check(h, st["hits"], ks=(X.K_HITS,), flags=GH.FLAGS)


def _near(h, st):
    return GN._check_ref(h, st["near"])


def _knear(h, st):
    order = st["order"]
    out = [GK._check(h, order, K) for K in X.KS_NEAR]
    GK._check(h, order, X.KS_NEAR[0], count_all=True)
    want = np.where(order["valid"], order["total"], 0).astype(np.uint32)
    for ip in (False, True):
        GK._poison(h, len(want), 0, count_all=True)
        got = query.count_within(h, order["points"], inplace=ip)
        assert got.dtype == np.uint32 and np.array_equal(got, want), (ip, np.flatnonzero(got != want)[:8])
    return out


def _sweep(h, st):
    return GW._check_ref(h, st["sweep"])


def _boxes(h, st):
    return GO._check(h, st["boxes"], ks=(X.K_BOX,))


def _sdf(h, st):
    ref = st["sdf"]
    trips = GD._check(h, ref, st["prec"])
    for ip in (False, True):                                         # the sign-only form: no nearest walk, the same verdict and crossings
        GD._poison(h, len(ref["points"]))
        prim, dist, point, inside, cr, _ = h.signed_distance(ref["points"], inplace=ip, want_prim=False, want_dist=False, want_point=False, want_crossings=True)
        assert prim is None and dist is None and point is None
        assert np.array_equal(inside, ref["inside"]) and np.array_equal(cr.astype(np.uint32), ref["crossings"]), ip
    return trips


def _identities(h, st):
    T = S.dtype_of(st["prec"])
    near, order = st["near"], st["order"]
    pts = near["points"]
    # nearest_k at K = 1 is closest_point, byte for byte, with the same trips
    for ip in (False, True):
        GN._poison(h, len(pts))
        c_prim, c_dist, c_point, c_trips = h.closest_point(pts, inplace=ip, want_trips=True)
        GK._poison(h, len(pts), 1)
        prim, dist, point, count, trips = h.nearest_k(pts, 1, inplace=ip, want_trips=True)
        assert np.array_equal(prim[:, 0], c_prim) and np.array_equal(_bits(dist[:, 0]), _bits(c_dist)) and np.array_equal(_bits(point[:, 0]), _bits(c_point))
        assert np.array_equal(count, (c_prim >= 0).astype(np.uint32)) and np.array_equal(trips, c_trips)
    # a sweep with t_min = t_max = 0 is blocked exactly where an object lies within r of its origin
    v = near["valid"]
    p = pts[v, :3]
    rng = np.random.default_rng(181)
    n = len(p)
    r = np.array(rng.uniform(0.0, 0.1, n) * rng.choice([1.0, 1e-3], n), dtype=T).astype(np.float64)
    rays = np.concatenate([p, np.zeros((n, 1)), S._unit(rng, n), np.zeros((n, 1))], axis=1)
    count = query.count_within(h, p, r)
    assert 0.1 < (count > 0).mean() < 0.9
    for ip in (False, True):
        GW._poison(h, n)
        assert np.array_equal(h.sweep_blocked(rays, r, inplace=ip), (count > 0).astype(np.uint8)), ip
    # |signed_distance| is closest_point's distance; prim and point are its own
    sd = st["sdf"]["points"]
    for ip in (False, True):
        GN._poison(h, len(sd))
        c_prim, c_dist, c_point, _ = h.closest_point(sd, inplace=ip)
        GD._poison(h, len(sd))
        prim, dist, point, inside, _, _ = h.signed_distance(sd, inplace=ip)
        assert np.array_equal(prim, c_prim) and np.array_equal(_bits(point), _bits(c_point)) and np.array_equal(_bits(np.abs(dist)), _bits(np.abs(c_dist)))
        assert np.array_equal(np.signbit(dist), inside == 1)


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("name,how", X.cases())
def test_every_walk_against_its_scan(gpu, name, how, prec):
    st = X.sets(name, prec, how)
    ns = st["ns"]
    with _handle(gpu, name, prec, how) as h:
        centre, scale = GC._device_frame(gpu, h)
        assert np.array_equal(centre, st["frame"][0]) and scale == st["frame"][1]      # the frame the validity rules are restated with is the tree's
        _cast(h, st)
        _hits(h, st)
        trips = dict(near=_near(h, st), sweep=_sweep(h, st), boxes=_boxes(h, st), sdf=_sdf(h, st))
        k4, k16 = _knear(h, st)
        trips.update(knear4=k4, knear16=k16)
        _identities(h, st)
    for what, t in trips.items():
        _report(name, prec, how, what, t)
        _same_walk(t)
    # a triangle winner was reached through the tree: at least the root and its leaf test; an invalid item takes no trip
    for what, prim in (("near", st["near"]["prim"]), ("sweep", st["sweep"]["prim"]), ("sdf", st["sdf"]["prim"]), ("knear4", st["order"]["prim"][:, 0])):
        for t in trips[what]:
            assert t[prim >= ns].min() >= 2, what
    for what, valid in (("near", st["near"]["valid"]), ("sweep", st["sweep"]["valid"]), ("boxes", st["boxes"]["valid"]), ("sdf", st["sdf"]["valid"]), ("knear4", st["order"]["valid"])):
        for t in trips[what]:
            assert not t[~valid].any(), what
    for t in trips["boxes"]:
        assert t[st["boxes"]["cand"][:, ns:].any(axis=1)].min() >= 2


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("name", X.MESHES + ("scrambled",))
def test_render_walk_against_the_oracle(gpu, oracle, name, prec):
    """The closest-hit walk of the renderer on the same meshes, through scene_s4's camera: 600 paths of depth 4 started in three windows on the mesh, every
    segment's prim, t and direction bit for bit the oracle's, which scans every triangle; then the image in place and with the deferred mesh pass, the
    same pixels and segments, within the renderer's tolerance of the oracle's."""
    from test_gpu_bvh import _trace_equal, _with_env
    from test_gpu_parity import _args, _close, _counts
    s, r = X.render_scene(name), X.RENDER
    hits = 0
    for k, window in enumerate(X.RENDER_WINDOWS[name]):
        hits += _trace_equal(gpu, oracle, s, prec, W=r["W"], H=r["H"], spp=r["spp"], depth=r["depth"], n=r["n"], seed=r["seed"] + k, window=window)
    assert hits >= 100
    ns, nm, nt = _counts(s)
    res = {}
    for d in ("1", "0"):
        def run():
            hdr, _ = gpu.render(*_args(s), gpu.make_params(160, 90, 4, 4, ns, nm, nt, flags=gpu.KERNEL_WAVEFRONT, seed=12), prec)
            return hdr, gpu.counters()["segments"]
        res[d] = _with_env(gpu, {"SPIRA_DEFER_MESH": d}, run)
    assert np.array_equal(res["1"][0], res["0"][0]) and res["1"][1] == res["0"][1]
    ohdr, _, oseg = oracle.render(*_args(s), oracle.make_params(160, 90, 4, 4, ns, nm, nt, seed=12), prec)
    nbad, worst = _close(res["1"][0], ohdr)
    assert nbad == 0 and res["1"][1] == oseg, (nbad, worst, res["1"][1], oseg)
