"""GPU: the arrays of the seven one-launch list queries (cast, closest point, multi-hit, K-nearest, sweep, box overlap, signed distance), wanted one at a
time.  The host form stages a call's arrays in one buffer, each block bound to the field of the kernel's arguments it is read through, NULL arrays taking
no room: an output wanted alone lies elsewhere than in the call that wants them all, and must come back the same, bit for bit — a block bound to the wrong
field or laid over another shows here.  On a scene with a tree (the refilled sessions) and on one with spheres and LDS triangles (one lane per item), in
both precisions, for 130 items — more than two waves and no multiple of 64, so the sessions' ranges split unevenly — a few of them invalid, and K = 3, so
that the index lists are no multiple of 8 bytes long.  And the device form through spira_hip.query against the host form on the same inputs, bit for bit.
What the values must BE is the business of the per-query tests; here only that every organisation of a call's arrays gives the same ones."""
import functools

import numpy as np
import pytest

import cast_support as S
import nearest_support as N
import overlap_support as O
import sdf_support as D
import sweep_support as W
from spira_hip import query

pytestmark = pytest.mark.gpu

PRECS = ["f32", "f64"]
SCENES = {"tree": lambda: N.ico_scene(33), "lds": D.lds_scene}
N_ITEMS, K = 130, 3
INVALID_AT = (5, 64, 129)

# query: (the Scene method, the input sets, the arguments after them, the outputs in the order returned).  trips is a diagnostic and no output of its own
# (alone it is an argument error), so it is wanted together with prim.
QUERIES = {
    "cast": ("cast", ("rays",), (), ("prim", "t", "normal")),
    "closest_point": ("closest_point", ("points",), (), ("prim", "dist", "point", "trips")),
    "cast_hits": ("cast_hits", ("rays",), (K,), ("prim", "t", "count")),
    "nearest_k": ("nearest_k", ("points",), (K,), ("prim", "dist", "point", "count", "trips")),
    "sweep": ("sweep", ("sweeps", "radii"), (), ("prim", "t", "point", "normal", "trips")),
    "overlap_box": ("overlap_box", ("boxes",), (K,), ("prim", "count", "trips")),
    "signed_distance": ("signed_distance", ("points",), (), ("prim", "dist", "point", "inside", "crossings", "trips")),
}


@functools.lru_cache(maxsize=None)
def _inputs(scene_name):
    """The lists of one scene, Float64, read-only: 130 items each, the rows INVALID_AT made invalid by a NaN."""
    sc = SCENES[scene_name]()
    rng = np.random.default_rng(1303)
    sweeps, radii = W.head_on(rng, sc, N_ITEMS)
    x = dict(rays=S.rays_b(rng, sc, N_ITEMS), points=np.concatenate([N.near_surface(rng, sc, 65, frac=0.05), N.in_box(rng, sc, N_ITEMS - 65)]), sweeps=sweeps,
             radii=radii, boxes=np.concatenate([O.at_surface(rng, sc, 100, hi=0.2), O.containing(rng, sc, N_ITEMS - 100)]))
    for name, a in x.items():
        assert len(a) == N_ITEMS, name
        if a.ndim == 2:
            a[list(INVALID_AT), 0] = np.nan
        a.setflags(write=False)
    return sc, x


def _open(gpu, scene, prec):
    return gpu.Scene(scene["spheres5"] if len(scene["spheres5"]) else None, scene["materials8"], scene.get("triangles10"), prec)


def _same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype.itemsize == b.dtype.itemsize and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def _call(h, name, x, wanted):
    method, ins, more, outs = QUERIES[name]
    args = [x[k] for k in ins] + list(more)
    return dict(zip(outs, getattr(h, method)(*args, **{"want_" + o: o in wanted for o in outs})))


def _poison(h, name, x, wanted):
    """The staging buffer outlives a call: the same call over NaN items first leaves the invalid pattern in every element the next one must write, so
    that an element it fails to write cannot pass for the right answer of the call before."""
    _call(h, name, {k: np.full_like(v, np.nan) for k, v in x.items()}, wanted)


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("scene_name", sorted(SCENES))
@pytest.mark.parametrize("name", sorted(QUERIES))
def test_an_output_wanted_alone_equals_the_full_call(gpu, name, scene_name, prec):
    sc, x = _inputs(scene_name)
    outs = QUERIES[name][3]
    with _open(gpu, sc, prec) as h:
        _poison(h, name, x, outs)
        full = _call(h, name, x, outs)
        assert all(full[o] is not None and len(full[o]) == N_ITEMS for o in outs)
        prim = full["prim"].reshape(N_ITEMS, -1)
        assert np.array_equal(np.flatnonzero((prim == S.INVALID).all(axis=1)), INVALID_AT) and (prim[:, 0] >= 0).sum() >= 16      # (not all misses)
        for o in outs:
            wanted = (o, "prim") if o == "trips" else (o,)
            _poison(h, name, x, wanted)
            got = _call(h, name, x, wanted)
            assert all((got[p] is None) == (p not in wanted) for p in outs), (o, [p for p in outs if got[p] is not None])
            for p in wanted:
                assert _same(got[p], full[p]), (name, scene_name, prec, "wanted " + o, "differs in " + p)


def _device(prec, *arrays):
    import torch
    tdt = torch.float32 if prec == "f32" else torch.float64
    return [torch.tensor(a, dtype=tdt, device="cuda:0").contiguous() for a in arrays]


def _host(outs):
    import torch
    torch.cuda.synchronize()
    return [o.cpu().numpy() for o in (outs if isinstance(outs, tuple) else (outs,))]


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("scene_name", sorted(SCENES))
def test_the_device_forms_equal_the_host_forms(gpu, scene_name, prec):
    sc, x = _inputs(scene_name)
    with _open(gpu, sc, prec) as h:
        rays, points, sweeps, radii, boxes = _device(prec, x["rays"], x["points"], x["sweeps"], x["radii"], x["boxes"])
        pairs = {
            "cast": (h.cast(x["rays"], want_normal=True), query.cast_rays(h, rays, want_normal=True)),
            "occluded": (h.occluded(x["rays"]), query.cast_rays(h, rays, occlusion=True)),
            "closest_point": (h.closest_point(x["points"], want_trips=True), query.closest_points(h, points, want_trips=True)),
            "cast_hits": (h.cast_hits(x["rays"], K), query.cast_all(h, rays, K)),
            "nearest_k": (h.nearest_k(x["points"], K, want_trips=True), query.k_nearest(h, points, K, want_trips=True)),
            "sweep": (h.sweep(x["sweeps"], x["radii"], want_trips=True), query.sweep_spheres(h, sweeps, radii, want_trips=True)),
            "sweep_blocked": (h.sweep_blocked(x["sweeps"], x["radii"]), query.sweep_spheres(h, sweeps, radii, blocked=True)),
            "overlap_box": (h.overlap_box(x["boxes"], K, want_trips=True), query.overlap_boxes(h, boxes, K, want_trips=True)),
            "overlap_any": (h.overlap_any(x["boxes"]), query.overlap_boxes(h, boxes, 0, any=True)),
            "signed_distance": (h.signed_distance(x["points"], want_crossings=True, want_trips=True),
                                query.signed_distance(h, points, want_crossings=True, want_trips=True)),
        }
        for name, (host, dev) in pairs.items():
            host = list(host) if isinstance(host, tuple) else [host]
            dev = _host(dev)
            assert len(host) == len(dev), name
            for k, (a, b) in enumerate(zip(host, dev)):
                assert a is not None and len(a) == N_ITEMS and _same(a, b), (name, scene_name, prec, "output %d" % k)
