"""GPU: spira_scene_cast_hits_* (spira_hits.h: k_hits, k_hits_session) against the yardstick of tests/hits_support.py — the oracle's per-object tests on
every object, sorted by (t ascending, index descending), cut to K — in both precisions, compared with numpy.array_equal on bytes: prim, t and count,
for K in {1, 2, 3, 16} x flags {0, INPLACE, COUNT_ALL, both}, each call on a staging poisoned first.  Every ray set first proves, on the yardstick's output alone, that it reaches what it is
for: rays with more candidates than K, with fewer, with none, and on the ties set two candidates of equal t straddling slots K - 1 / K."""
import functools
import os

import numpy as np
import pytest

import cast_support as S
import hits_support as H
import nearest_support as N
from spira_hip import query

pytestmark = pytest.mark.gpu

KS = (1, 2, 3, 16)
FLAGS = ((False, False), (True, False), (False, True), (True, True))      # (inplace, count_all)


def _line_scene():
    """Five spheres strung along the x axis, the second and third overlapping."""
    sp = np.array([[-4.0, 0, 0, 0.8, 1], [-2.0, 0, 0, 0.9, 1], [-1.0, 0, 0, 0.7, 1], [1.5, 0, 0, 0.5, 1], [4.0, 0, 0, 1.0, 1]])
    return dict(spheres5=sp, materials8=np.array([[0.8, 0.8, 0.8, 0, 0, 0, 0.5, 0.0]]), triangles10=None)


def _line_rays(rng, n):
    o = np.concatenate([[-8.0], [0.0], [0.0]]) + 0.3 * (rng.random((n, 3)) - 0.5)
    tgt = np.array([8.0, 0, 0]) + 1.6 * (rng.random((n, 3)) - 0.5) * np.array([0, 1, 1])
    r = np.concatenate([o, np.full((n, 1), 0.001), 2.0 * (tgt - o), np.full((n, 1), np.inf)], axis=1)
    r[1::4, :3] = np.array([-1.5, 0.0, 0.0]) + 0.2 * (rng.random((len(r[1::4]), 3)) - 0.5)      # origins inside the overlap: far roots
    r[2::8, 7] = 4.5                                                                              # a t_max that cuts the string
    r[3::16, 4:7] = [0.0, 1.0, 0.2]                                                               # away from everything
    return r


SCENES = {
    "line": _line_scene,
    "shells_lds": lambda: H.shells_scene(1, n_shells=10, max_tris=32),
    "ico33": lambda: N.scene("ico33"),
    "shells": lambda: H.shells_scene(1, n_shells=10),
}


@functools.lru_cache(maxsize=None)
def _scene(name):
    return SCENES[name]()


@functools.lru_cache(maxsize=None)
def _ref(name, prec):
    rng = np.random.default_rng(17)
    scene = _scene(name)
    if name == "line":
        rays = _line_rays(rng, 96)
    elif name == "shells":
        rays = H.rays_through(rng, scene, 512)
    elif name == "ico33":
        rays = S.aim_at_triangles(rng, np.concatenate([S.rays_b(rng, scene, 64), S.rays_c(rng, scene, 32)]), scene)
    else:
        rays = H.rays_through(rng, scene, 96)
    return H.reference(scene, prec, rays)


@functools.lru_cache(maxsize=None)
def _ties_ref(prec):
    s = S.ties_set(prec)
    return H.reference(s["scene"], prec, s["rays"]["rays"])


def _open(gpu, scene, prec):
    sp = scene["spheres5"]
    return gpu.Scene(sp if len(sp) else None, scene["materials8"], scene["triangles10"], prec)


def _totals(ref):
    return np.array([-1 if c is None else len(c) for c in ref["cands"]])


def _check(h, ref, ks=KS, flags=FLAGS, also=None):
    """Every call on a staging poisoned first (hits_support.poison): a slot the kernel never stores cannot hold the call before's right answer.
    also(K, inplace, count_all, g_prim, g_t, g_count): further assertions on the same answers."""
    T = ref["sc"].T
    for K in ks:
        prim, t, count, total = H.cut(ref["cands"], ref["prepared"], T, K)
        for inplace, count_all in flags:
            H.poison(h, len(ref["rays"]), K, inplace)
            g_prim, g_t, g_count = h.cast_hits(ref["rays"], K, inplace=inplace, count_all=count_all)
            want_count = total if count_all else count
            bad = np.flatnonzero((g_prim != prim).any(axis=1) | (g_count != want_count))
            print(ref["sc"].prec, "K", K, "inplace", inplace, "count_all", count_all, "rays", len(prim), "mismatching", len(bad))
            assert np.array_equal(g_prim, prim) and np.array_equal(g_t.view(np.uint8), t.view(np.uint8)) and np.array_equal(g_count, want_count), \
                (K, inplace, count_all, bad[:8], g_prim[bad[:4]], prim[bad[:4]], g_count[bad[:8]], want_count[bad[:8]])
            if also is not None:
                also(K, inplace, count_all, g_prim, g_t, g_count)


@pytest.mark.parametrize("prec", ["f32", "f64"])
@pytest.mark.parametrize("name", ["line", "shells_lds", "ico33", "shells"])
def test_knob_sweep_against_the_scan(gpu, name, prec):
    ref = _ref(name, prec)
    tot = _totals(ref)
    assert ref["valid"].all()
    # the set reaches what it is for: no candidate at all, fewer than K and more than K for the K of the sweep this scene can exceed
    top = {"line": 3, "ico33": 2, "shells_lds": 2, "shells": 16}[name]
    print(name, prec, "candidates per ray: max", tot.max(), "zero", (tot == 0).sum(), "histogram", np.bincount(tot)[:24])
    assert (tot == 0).sum() >= 4 and (tot > top).sum() >= 8 and ((tot > 0) & (tot < top)).sum() >= 4
    if name == "shells":
        assert len(ref["sc"].tri) > 32 and 300 <= len(ref["sc"].tri) <= 1000 and (tot >= 17).sum() >= 32
    if name == "shells_lds":
        assert len(ref["sc"].tri) == 32
    if name == "line":
        first = np.array([c[0][1] if c else -1 for c in ref["cands"]])
        assert len(set(first.tolist())) >= 3                      # origins inside a sphere: its far root leads the list
    with _open(gpu, _scene(name), prec) as h:
        _check(h, ref)
        # K = 1 is Scene.cast, byte for byte
        c_prim, c_t, _ = h.cast(ref["rays"])
        for ip in (False, True):
            g_prim, g_t, _ = h.cast_hits(ref["rays"], 1, inplace=ip)
            assert np.array_equal(g_prim[:, 0], c_prim) and np.array_equal(g_t[:, 0].view(np.uint8), c_t.view(np.uint8))


@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_equal_t_straddling_the_last_slot(gpu, prec):
    ref = _ties_ref(prec)
    pair = S.ties_set(prec)["pair"]
    straddle = {K: 0 for K in (1, 3)}
    for c in ref["cands"]:
        for K in straddle:
            if c is not None and len(c) > K and c[K - 1][0] == c[K][0]:
                assert c[K - 1][1] > c[K][1] and pair[c[K - 1][1]] == c[K][1]
                straddle[K] += 1
    print(prec, "rays with equal t at slots K-1 / K:", straddle)
    assert straddle[1] >= 40 and straddle[3] >= 4
    with _open(gpu, S.ties_set(prec)["scene"], prec) as h:
        _check(h, ref)


@pytest.mark.parametrize("prec", ["f32", "f64"])
@pytest.mark.parametrize("n", [1000, 999, 5])
def test_sessions_against_in_place(gpu, prec, n):
    """The 33-triangle tree with SPIRA_CAST_REFILL 1 and 64 (a refill after every finished lane / only when the whole wave is free), one wave per CU:
    1 000 rays split evenly over the plan's waves or not (rem), and fewer rays than a wave has lanes."""
    scene = _scene("ico33")
    rng = np.random.default_rng(23)
    rays = S.aim_at_triangles(rng, S.rays_b(rng, scene, n), scene)
    ref = H.reference(scene, prec, rays[:64])
    tot = _totals(ref)
    assert n == 5 or ((tot >= 2).sum() >= 8 and (tot == 0).sum() >= 4)
    with _open(gpu, scene, prec) as h:
        want = {(K, ca): h.cast_hits(rays, K, inplace=True, count_all=ca) for K in (2, 16) for ca in (False, True)}
        prim, t, count, total = H.cut(ref["cands"], ref["prepared"], ref["sc"].T, 2)
        m = len(prim)
        assert np.array_equal(want[(2, False)][0][:m], prim) and np.array_equal(want[(2, True)][2][:m], total) and np.array_equal(want[(2, False)][1][:m], t)
        old = {k: os.environ.get(k) for k in ("SPIRA_CAST_REFILL", "SPIRA_CAST_WAVES_PER_CU")}
        try:
            for refill in ("1", "64"):
                os.environ["SPIRA_CAST_REFILL"], os.environ["SPIRA_CAST_WAVES_PER_CU"] = refill, "1"
                plan = gpu.cast_plan(n, 256)
                assert plan["refill_free"] == int(refill) and (n == 5 or (plan["rem"] == 0) == (n == 1000))
                for (K, ca), w in want.items():
                    H.poison(h, n, K, False)                     # between `want` and the session call: same n, same K, the same layout
                    got = h.cast_hits(rays, K, count_all=ca)
                    for a, b in zip(got, w):
                        assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), (refill, K, ca)
        finally:
            for k, v in old.items():
                if v is None:
                    os.environ.pop(k, None)
                else:
                    os.environ[k] = v


@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_edges(gpu, prec):
    ref = _ref("shells", prec)
    T = ref["sc"].T
    rays = np.array(ref["rays"][:128])
    sub = dict(ref, rays=rays, cands=ref["cands"][:128], prepared=ref["prepared"][:128])
    tot = _totals(sub)
    with _open(gpu, _scene("shells"), prec) as h:
        # max_hits = 0, count only, NULL lists; t_max = +Inf with COUNT_ALL
        assert np.isinf(rays[:, 7]).sum() >= 64
        for ip in (False, True):
            p0, t0, c0 = h.cast_hits(rays, 0, inplace=ip, count_all=True)
            assert p0 is None and t0 is None and np.array_equal(c0, tot.astype(np.uint32))
            assert np.array_equal(query.count_hits(h, rays, inplace=ip), tot.astype(np.uint32))
        # one NULL output at a time
        full = h.cast_hits(rays, 3)
        for k, kw in enumerate(({"want_prim": False}, {"want_t": False}, {"want_count": False})):
            got = h.cast_hits(rays, 3, **kw)
            assert got[k] is None and all(np.array_equal(a, b) for j, (a, b) in enumerate(zip(got, full)) if j != k)
        # t_min == t_max: the hit itself and nothing else
        prim, t, count, total = H.cut(sub["cands"], sub["prepared"], T, 1)
        sel = np.flatnonzero(prim[:, 0] >= 0)[:48]
        at = np.array(rays[sel]); at[:, 3] = t[sel, 0]; at[:, 7] = t[sel, 0]
        r_at = H.reference(_scene("shells"), prec, at)
        assert (_totals(r_at) >= 1).all()
        _check(h, r_at, ks=(1, 3), flags=((False, False), (True, True)))
        # the invalid kinds interleaved with valid rays: neighbours undisturbed
        kinds = S.invalid_kinds(T, ref["sc"].frame)
        mixed = np.array(rays)
        where = np.arange(0, len(mixed), 5)[:2 * len(kinds)]
        mixed[where] = kinds[np.arange(len(where)) % len(kinds)]
        r_mixed = H.reference(_scene("shells"), prec, mixed)
        assert not r_mixed["valid"][where].any() and r_mixed["valid"].sum() == len(mixed) - len(where)
        _check(h, r_mixed, ks=(1, 16))
        g_prim, g_t, g_count = h.cast_hits(mixed, 4, count_all=True)
        assert (g_prim[where] == -3).all() and not g_t[where].any() and not g_count[where].any()
    # K larger than the number of objects
    line = _ref("line", prec)
    assert _totals(line).max() <= 5
    with _open(gpu, _scene("line"), prec) as h:
        g_prim, g_t, g_count = h.cast_hits(line["rays"], 16)
        assert (g_prim[:, 5:] == -1).all() and np.array_equal(g_t[:, 5:], np.broadcast_to(line["prepared"][:, 7:8], g_t[:, 5:].shape)) and g_count.max() <= 5


@pytest.mark.parametrize("how", ["update", "rebuild"])
@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_device_form_and_new_trees(gpu, prec, how):
    """Torch tensors on a non-default stream equal the host form; after update_device / rebuild_device on another stream, a scan of the new arrays."""
    import torch
    A = _scene("shells")
    ref_a = _ref("shells", prec)
    rays = np.array(ref_a["rays"][:192])
    Bs = dict(A, triangles10=H.warp(A["triangles10"]))
    ref_b = H.reference(Bs, prec, rays, frame=ref_a["sc"].frame if how == "update" else None)
    tdt = torch.float32 if prec == "f32" else torch.float64
    d_tri = torch.tensor(Bs["triangles10"], dtype=tdt, device="cuda:0").contiguous()
    d_rays = torch.tensor(rays, dtype=tdt, device="cuda:0").contiguous()
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()
    with _open(gpu, A, prec) as h:
        host = h.cast_hits(rays, 16, count_all=True)
        dev = query.cast_all(h, d_rays, 16, count_all=True, stream=s2)
        s2.synchronize()
        for a, b in zip(dev, host):
            assert np.array_equal(a.cpu().numpy().view(np.uint8), b.view(np.uint8))
        (h.update_device if how == "update" else h.rebuild_device)(d_tri, s1)
        dev = query.cast_all(h, d_rays, 3, stream=s2)
        cnt = query.count_hits(h, d_rays, stream=s2)
        s2.synchronize()
        if how == "rebuild":
            centre, scale = H.device_frame(gpu, h)
            ref_b = H.reference(Bs, prec, rays, frame=(centre, scale))
        assert ref_b["valid"].all()
        prim, t, count, total = H.cut(ref_b["cands"], ref_b["prepared"], ref_b["sc"].T, 3)
        assert not np.array_equal(prim, H.cut(ref_a["cands"][:192], ref_a["prepared"][:192], ref_b["sc"].T, 3)[0])
        assert np.array_equal(dev[0].cpu().numpy(), prim) and np.array_equal(dev[1].cpu().numpy().view(np.uint8), t.view(np.uint8))
        assert np.array_equal(dev[2].cpu().numpy().astype(np.uint32), count) and np.array_equal(cnt.cpu().numpy().astype(np.uint32), total)


@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_inside_mesh_on_a_closed_blob(gpu, prec):
    """Points well inside the blob (towards its centre from surface points) and outside it (beyond surface points, and far away) are told apart."""
    scene = S.blob_scene(2)
    rng = np.random.default_rng(41)
    lo, hi, c, ext = S.target_box(scene)
    surf = N.surface_points(rng, scene, 64)
    inside = c + 0.5 * (surf - c)
    outside = np.concatenate([c + 1.3 * (surf - c), c + 2.0 * ext * S._unit(rng, 32)])
    outside = outside[outside[:, 1] > -0.45]                      # (above the ground sphere's surface; spheres are taken out of the parity anyway)
    with _open(gpu, scene, prec) as h:
        got_in, got_out = query.inside_mesh(h, inside), query.inside_mesh(h, outside)
    print(prec, "inside:", got_in.sum(), "of", len(inside), "outside:", (~got_out).sum(), "of", len(outside))
    assert got_in.all() and not got_out.any()
