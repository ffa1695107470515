"""GPU: the claims spira_query.h rests on that tests/test_gpu_cast.py never reaches, each against the reference's linear scan (tests/cast_support.py) or
against the library's own default organisation, always bit for bit — no tolerance, no measurement:
  * the origin rule: valid rays from 60 .. 64 normalised units away, in four placements of the mesh, after an update and after a rebuild, with their
    invalid twins just beyond the bound interleaved and with t windows that end before, on and behind the hit;
  * axis-parallel directions with signed zeros, origins on the mesh's bounding planes, rays inside the planes of axis-aligned squares (leaf boxes of
    zero extent), corners and shared edges hit head-on;
  * ties between duplicate triangles and the 32 / 33-triangle tree threshold through cast;
  * SPIRA_CAST_REFILL and SPIRA_CAST_WAVES_PER_CU, with the plan shown to change;
  * lists long enough that k_cast's grid-stride loop takes a second trip and make_cast_plan stops adding waves — in the device form: the host form
    at that size is an open finding, described above _upload;
  * every subset of the outputs, host and device form.
The ray sets and the scan's answers come from tests/cast_support.py; tests/test_cast_edges_cpu.py asserts without a device that they reach what they are for."""
import functools
import itertools

import numpy as np
import pytest

import cast_support as S
from spira_hip import scenes
from test_gpu_bvh import _with_env
from test_gpu_cast import N_REFILL, _check_against, _device_frame, _handle, _reference, _refill_rays, _scan, _scene

pytestmark = pytest.mark.gpu

P_LONG = 4099


def _open(gpu, scene, prec):
    return gpu.Scene(scene["spheres5"] if len(scene["spheres5"]) else None, scene["materials8"], scene["triangles10"], prec)


def _check(h, sc, j):
    _check_against(h, sc, None, j["rays"], j["prim"], j["t"], j["prepared"])


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({1: np.uint8, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def _same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(_bits(a), _bits(b))


@functools.lru_cache(maxsize=None)
def _nan_rays(n, prec):
    return np.full((n, 8), np.nan, dtype=S.dtype_of(prec))


def _poison(h, n):
    """The host form stages its outputs in a workspace that outlives the call: after a call on the same list it holds the right answers already, and
    an output the next call failed to write would go unnoticed.  n invalid rays (NaN) leave -3 / 0 / 0 / 255 in every staged element first — through
    both organisations, so that an element one of them skips is written by the other."""
    bad = _nan_rays(n, h.prec)
    for ip in (False, True):
        prim = h.cast(bad, want_normal=True, inplace=ip)[0]
        occ = h.occluded(bad, inplace=ip)
        assert prim[0] == -3 and prim[-1] == -3 and occ[0] == 255 and occ[-1] == 255


def _num_cus():
    import torch
    return int(torch.cuda.get_device_properties(0).multi_processor_count)


def test_blob_scene_is_scene_s4_without_the_camera(gpu):
    for level in (2, 3):
        a, b = S.blob_scene(level), scenes.scene_s4(level=level)
        for k in ("triangles10", "spheres5", "materials8"):
            assert _same(a[k], b[k]), (level, k)


def _twins_answer_invalid(h, j, at):
    g_prim, g_t, g_n = h.cast(j["rays"], want_normal=True)
    assert (g_prim[at] == -3).all() and not g_t[at].any() and not g_n[at].any() and (h.occluded(j["rays"])[at] == 255).all()
    assert (g_prim[at - 1] != -3).all()


# ------------------------------------------------------------------------------------------------ 1, 2: the origin rule
@pytest.mark.parametrize("fi", range(len(S.FRAMES)))
@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_far_origins(gpu, prec, fi):
    """"Why 64" of spira_query.h: a valid origin at 60 .. 64 normalised units leaves the Float32 entry point within the builder's pad, whatever the mesh's
    size and place.  Vertices and edge midpoints are the targets; the twins one step beyond the bound answer -3 / 0 / 0 / 255."""
    fs = S.far_set(prec, fi)
    sc, j = fs["sc"], S.far_joined(fs)
    with _open(gpu, fs["scene"], prec) as h:
        centre, scale = _device_frame(gpu, h)
        assert np.array_equal(centre, sc.frame[0]) and scale == sc.frame[1]
        _check(h, sc, j)
        _twins_answer_invalid(h, j, np.arange(1, 2 * S.N_FAR, 2))


@functools.lru_cache(maxsize=None)
def _moved():
    from test_gpu_refit import deform
    A = S.blob_scene(3)
    return A, dict(A, triangles10=deform(A["triangles10"]))


@pytest.mark.parametrize("how", ["update", "rebuild"])
@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_far_origins_after_an_update_and_after_a_rebuild(gpu, prec, how):
    """After an update the tree keeps the frame it was built in and pads with refit_pad's bound (spira_refit.h: never the smaller pad); after a rebuild
    it has a new frame, which must be the fresh build's of the deformed mesh (mesh_frame).  The far rays are built in the frame that holds and scanned
    against the deformed triangles.  Host form."""
    import oracle_py
    A, B = _moved()
    n = 96
    with _open(gpu, A, prec) as h:
        before = _device_frame(gpu, h)
        fa = S.mesh_frame(A["triangles10"], prec)
        assert np.array_equal(before[0], fa[0]) and before[1] == fa[1]
        (h.update if how == "update" else h.rebuild)(triangles10=B["triangles10"])
        got = _device_frame(gpu, h)
        want = fa if how == "update" else S.mesh_frame(B["triangles10"], prec)
        assert np.array_equal(got[0], want[0]) and got[1] == want[1], (how, got, want)
        if how == "rebuild":
            assert not (np.array_equal(got[0], fa[0]) and got[1] == fa[1])       # the two cases test two frames
        sc = S.Scan(oracle_py, B, prec, frame=want)
        fs = S.far_rays_in(sc, B, seed=17, n=n, n_win=24)
        assert fs["far"]["valid"].all() and 4 * (fs["far"]["prim"] >= sc.ns).sum() >= 3 * n and not fs["twins"]["valid"].any() and len(fs["sel"]) == 24
        j = S.far_joined(fs)
        _check(h, sc, j)
        _twins_answer_invalid(h, j, np.arange(1, 2 * n, 2))


# ------------------------------------------------------------------------------------------------ 3: axis rays, planes, squares
@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_axis_rays_and_bounding_planes(gpu, prec):
    """rcp_fast(0) is +-Inf in Float32 and NaN in Float64, bvh8_rcp clamps to 2^40: a zero or -0.0 direction component, an origin exactly on a plane of
    the root box (a slab distance of 0, or 0 x Inf) must prune nothing the scan hits — from outside the box and from inside it."""
    a = S.axis_set(prec, 3)
    sc = a["sc"]
    assert len(sc.tri) == 1280 and a["axis"]["valid"].all() and a["planes"]["valid"].all()
    assert 3 * (a["axis"]["prim"] >= sc.ns).sum() >= S.N_AXIS and 10 * (a["axis"]["prim"] < 0).sum() >= S.N_AXIS
    # the plane rays at this level, from the scan: all 12 inward rays hit the mesh, no in-plane and no outward ray does (as at level 2)
    on_mesh = a["planes"]["prim"] >= sc.ns
    assert [int(on_mesh[a["kind"] == k].sum()) for k in (S.PLANE_IN, S.PLANE_INWARD, S.PLANE_OUTWARD)] == [0, 12, 0]
    with _open(gpu, a["scene"], prec) as h:
        _check(h, sc, S.join([a["axis"], a["planes"]]))


@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_axis_aligned_squares(gpu, prec):
    """Leaf boxes of zero extent: rays along a square's normal at an interior point, at the midpoint of the edge its two triangles share and at a corner;
    rays lying in a square's plane; and axis rays that start 60 normalised units away along their axis."""
    q = S.quad_set(prec)
    sc, j = q["sc"], S.join([q["quads"], q["axis_far"]])
    with _open(gpu, q["scene"], prec) as h:
        _check_against(h, sc, None, j["rays"], j["prim"], j["t"], j["prepared"], normals=False)
        # the normals' criterion of _check_against without its premise that the Float32 restatement differs from the Float64 one: the normal of an
        # axis-aligned triangle is +-e_k in any precision, the floor is 0 and the library's normal has to be exact
        e_n, n64 = sc.normals(j["prepared"], j["prim"], j["t"], sc.T), sc.normals(j["prepared"], j["prim"], j["t"], np.float64)
        floor = float(np.abs(e_n.astype(np.float64) - n64).max())
        for ip in (False, True):
            g_n = h.cast(j["rays"], want_normal=True, inplace=ip)[2]
            assert float(np.abs(g_n.astype(np.float64) - n64).max()) <= 4 * floor and not g_n[j["prim"] < 0].any(), (ip, floor)
            assert (np.abs(g_n[j["prim"] >= 0]).sum(axis=1) == 1).all()


# ------------------------------------------------------------------------------------------------ 4: ties, the tree threshold
@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_ties_go_to_the_later_triangle(gpu, prec):
    s = S.ties_set(prec)
    r = s["rays"]
    with _open(gpu, s["scene"], prec) as h:
        _check(h, s["sc"], r)
        for ip in (False, True):
            g_prim = h.cast(r["rays"], inplace=ip)[0]
            hit = g_prim >= 0
            assert hit.sum() >= 50 and (g_prim[hit] > s["pair"][g_prim[hit]]).all()


@pytest.mark.parametrize("nt", [32, 33, 34])
def test_tree_threshold(gpu, nt):
    """32 triangles are scanned in LDS by k_cast (no tree, no origin rule), 33 get a tree and the session kernel."""
    import oracle_py
    from test_gpu_parity import random_scene
    rng = np.random.default_rng(2)
    scene = random_scene(rng, 3, nt)
    sc = S.Scan(oracle_py, scene, "f32")
    assert (sc.frame is None) == (nt <= 32)
    # (rays_a + rays_b alone hit these few triangles with 4 .. 7 rays of 96: every second ray is aimed at a triangle)
    j = S.scanned(sc, S.aim_at_triangles(rng, np.concatenate([S.rays_a(rng, scene, 48), S.rays_b(rng, scene, 48)]), scene))
    assert j["valid"].all() and (j["prim"] >= sc.ns).sum() >= 32 and (j["prim"] < 0).sum() >= 24
    with _open(gpu, scene, "f32") as h:
        _check(h, sc, j)


# ------------------------------------------------------------------------------------------------ 5: the session knobs
# AN OPEN FINDING, and why the lists below live on the device.  A first version of tests 5 and 6 ran the tiled and the long lists through the HOST form:
# numpy arrays of 40 .. 270 MB went into Scene.cast / Scene.occluded, outputs of up to 100 MB came back into fresh arrays, and all of them were freed
# when the test ended.  This module passed, and so did every run of it alone.  In the whole suite the next module then met a GPU fault in a test this
# change does not touch (test_gpu_denoise.py::test_features_against_bounce_zero_of_the_traces[s4-160-90-4-f64]): "an illegal memory access" reported by
# trace_impl's hipMemcpyAsync of `dirs` — 1.38 MB, device to a pageable numpy array — after its copies of `prims` (230 KB) and `ts` (460 KB), behind
# the same kernel on the same stream, had succeeded; so k_trace itself had not faulted.  With the lists on the device, as below, the same sequence of
# modules passes.  The cause is NOT established.  What is known: the library's host forms hand the caller's pageable pointers straight to
# hipMemcpyAsync (cast_impl, trace_impl); cast_impl synchronises its stream before it returns; its staging arithmetic is in size_t and in bounds at
# this size (ray_b + 4 t_b + prim_b + n); the failing copy was the first one of 1 MB or more into pageable memory after the large arrays had been freed.
# A suspicion, not more: the runtime copies pageable memory of that size by pinning the caller's pages in place and keeps such pinnings, and one was
# used again for an address that had been unmapped and mapped anew.  Until that is settled the host form of a list of hundreds of megabytes has NO test, and
# nothing in this module gives the library a host array of 1 MB or more that is freed afterwards: the 20 011-ray arrays are cached for the life of
# the process, and _upload sends its rays in pieces of 256 KB.
def _upload(arr, prec):
    """A host array of rays as a device tensor of the handle's precision, in pieces of 4 096 rays (256 KB in Float64): see the open finding above."""
    import torch
    a = np.ascontiguousarray(arr, dtype=S.dtype_of(prec))
    return torch.cat([torch.tensor(a[i:i + 4096], device="cuda:0") for i in range(0, len(a), 4096)]).contiguous()


def _cast_on_device(h, d_rays, inplace=False):
    """Cast and occlusion in device form into buffers pre-filled with a sentinel no answer can be: device tensors (prim, t, normal [n, 3], hit)."""
    import torch
    n, tdt = d_rays.shape[0], d_rays.dtype
    prim = torch.full((n,), -77, dtype=torch.int32, device="cuda:0")
    t = torch.full((n,), -12345.0, dtype=tdt, device="cuda:0")
    nrm = torch.full((n, 3), -12345.0, dtype=tdt, device="cuda:0")
    hit = torch.full((n,), 77, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    st = torch.cuda.current_stream()
    h.cast_device(d_rays.data_ptr(), n, prim.data_ptr(), t.data_ptr(), nrm.data_ptr(), st.cuda_stream, inplace=inplace)
    h.occluded_device(d_rays.data_ptr(), n, hit.data_ptr(), st.cuda_stream, inplace=inplace)
    st.synchronize()
    return prim, t, nrm, hit


def _first_period(outs, k, what):
    """The answers of a list tiled k times: every period must be the first, bit for bit — compared on the device; the first period comes back as host arrays."""
    import torch
    heads = []
    for o in outs:
        b = o.contiguous().view(k, -1)
        bi = b.view({1: torch.uint8, 4: torch.int32, 8: torch.int64}[b.element_size()])
        bad = torch.nonzero((bi != bi[0]).any(dim=1)).flatten()
        assert bad.numel() == 0, (what, o.dtype, bad[:8].cpu().numpy())
        heads.append(b[0].cpu().numpy())
    heads[2] = heads[2].reshape(-1, 3)
    assert (heads[0] != -77).all() and (heads[1] != -12345.0).all() and (heads[2] != -12345.0).all() and (heads[3] != 77).all(), what
    return tuple(heads)


@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_session_knobs_agree_bitwise(gpu, prec):
    """SPIRA_CAST_REFILL and SPIRA_CAST_WAVES_PER_CU are read per call: any setting gives the default's bytes (the default's answers are pinned to the scan by
    test_gpu_cast.py::test_refills).  At 20 011 rays the plan's wave count is bound by 128 rays per wave (39 workgroups) and no waves-per-CU setting
    moves it on a device of 156 CUs or more, so the wave settings are also run on that list tiled until the device's capacity binds as well, where
    `waves` does change; every period of the tiled answers must be the first, and the first the default's.  The tiled list is made and compared on
    the device (device form) because of the open finding above; the host form runs on the 20 011 rays."""
    num_cus = _num_cus()
    rays = _refill_rays()
    k = 1
    while (N_REFILL * k) // 512 <= 5 * num_cus:
        k += 1
    n_tiled = N_REFILL * k
    d_tiled = _upload(rays, prec).repeat(k, 1).contiguous()

    def run():
        _poison(h, N_REFILL)
        return h.cast(rays, want_normal=True) + (h.occluded(rays),)

    def run_tiled(what):
        return _first_period(_cast_on_device(h, d_tiled), k, what)

    with _handle(gpu, "s4_4", prec) as h:
        want = run()
        plan, plan_t = gpu.cast_plan(N_REFILL, num_cus), gpu.cast_plan(n_tiled, num_cus)
        print(prec, "num_cus", num_cus, "rays", N_REFILL, "plan", plan, "tiled x", k, "plan", plan_t)
        assert plan["refill_free"] == 16 and plan_t["waves"] == num_cus * 20
        assert (want[0] >= 2).sum() > N_REFILL // 4 and (want[0] < 0).sum() > N_REFILL // 10
        for a, b in zip(run_tiled("default"), want):
            assert _same(a, b)
        for env in ({"SPIRA_CAST_REFILL": "1"}, {"SPIRA_CAST_REFILL": "64"}, {"SPIRA_CAST_WAVES_PER_CU": "1"}, {"SPIRA_CAST_WAVES_PER_CU": "64"},
                    {"SPIRA_CAST_REFILL": "1", "SPIRA_CAST_WAVES_PER_CU": "1"}):
            def go():
                long = run_tiled(env) if "SPIRA_CAST_WAVES_PER_CU" in env else None
                return run(), long, gpu.cast_plan(N_REFILL, num_cus), gpu.cast_plan(n_tiled, num_cus)
            got, long, p, pt = _with_env(gpu, env, go)
            for a, b in zip(got, want):
                assert _same(a, b), env
            if "SPIRA_CAST_REFILL" in env:
                assert p["refill_free"] == int(env["SPIRA_CAST_REFILL"]) != plan["refill_free"] and pt["refill_free"] == p["refill_free"], (env, p)
            if "SPIRA_CAST_WAVES_PER_CU" in env:
                w = int(env["SPIRA_CAST_WAVES_PER_CU"])
                assert pt["waves"] != plan_t["waves"] and (pt["waves"] == max(1, num_cus // 4) * 4 if w == 1 else pt["waves"] > plan_t["waves"]), (env, pt, plan_t)
                assert pt["base"] * pt["waves"] + pt["rem"] == n_tiled
                for a, b in zip(long, want):
                    assert _same(a, b), env
        assert gpu.cast_plan(N_REFILL, num_cus) == plan                     # the environment is as it was


# ------------------------------------------------------------------------------------------------ 6: long lists
@functools.lru_cache(maxsize=None)
def _long_base(name, prec):
    """4 099 rays: the module's reference set, then rays_b.  The scan's answers: all of them on s1 (five spheres), on s4_3 the reference set (scanned
    already) and every 28th ray of the rest."""
    ref, sc, scene = _reference(name, prec), _scan(name, prec), _scene(name)
    more = S.rays_b(np.random.default_rng(13), scene, P_LONG - len(ref["rays"]))
    rays = np.concatenate([ref["rays"], more])
    sub = np.arange(P_LONG) if name == "s1" else np.concatenate([np.arange(len(ref["rays"])), np.arange(len(ref["rays"]), P_LONG, 28)])
    rest = sub[len(ref["rays"]):]
    prim, t, valid, _ = sc.cast(rays[rest])
    assert valid.all()
    return rays, sub, np.concatenate([ref["prim"], prim]), np.concatenate([ref["t"], t])


def _long_n(num_cus):
    return (64 * 256 * num_cus + 1000) // P_LONG * P_LONG + P_LONG


def _check_long(gpu, name, prec, organisations):
    """Device form, NOT the host form the long lists were meant to use: see the open finding above.  The list is tiled on the device and its answers are
    compared there.  The kernels, the plan and the grid are the host form's, so the second trip of the grid-stride loop and the capped plan are
    pinned; the host form's staging and copies at this size are not (test_output_subsets and the 20 011-ray lists cover them at small sizes only)."""
    num_cus = _num_cus()
    n = _long_n(num_cus)
    plan = gpu.cast_plan(n, num_cus)
    print(name, prec, "num_cus", num_cus, "rays", n, "plan", plan)
    assert n % P_LONG == 0 and n - P_LONG <= 64 * 256 * num_cus + 1000 < n
    assert plan["grid_flat"] * 256 < n and plan["waves"] == num_cus * 20, plan      # the flat grid strides; the session plan is at the device's capacity
    rays, sub, prim, t = _long_base(name, prec)
    k = n // P_LONG
    d_tiled = _upload(rays, prec).repeat(k, 1).contiguous()
    assert d_tiled.shape == (n, 8)
    first = None
    with _handle(gpu, name, prec) as h:
        for ip in organisations:
            head = _first_period(_cast_on_device(h, d_tiled, inplace=ip), k, ip)      # output i is output i mod P, everywhere
            assert np.array_equal(head[0][sub], prim) and _same(head[1][sub], t), ip
            assert np.array_equal(head[3], (head[0] >= 0).astype(np.uint8)), ip
            if first is None:
                first = head
            for a, b in zip(head, first):
                assert _same(a, b), ip
    assert (first[0] >= 0).sum() > P_LONG // 8 and (first[0] < 0).sum() > P_LONG // 8


def test_long_list_f32_mesh(gpu):
    """More rays than 64 x 256 x num_cus: k_cast (SPIRA_CAST_INPLACE) takes a second trip of its grid-stride loop, and the session plan has stopped
    adding waves, so each wave's range grows instead."""
    _check_long(gpu, "s4_3", "f32", (False, True))


def test_long_list_f64_spheres(gpu):
    """The same length without a tree: k_cast<double, false, false>, the only kernel a sphere scene has."""
    _check_long(gpu, "s1", "f64", (False,))


# ------------------------------------------------------------------------------------------------ 7: output subsets
SUBSETS = [c for c in itertools.product((False, True), repeat=3) if any(c) and not all(c)]


@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_output_subsets(gpu, prec):
    """out_prim, out_t and out_normal one at a time and in pairs give the bytes of the full call: the host form lays its staging blocks out by hand, the
    device form writes the caller's buffers, which are 64 elements longer than the list here and must keep their sentinel beyond it."""
    import torch
    ref = _reference("s4_3", prec)
    rays, n = ref["rays"], len(ref["rays"])
    tdt = torch.float32 if prec == "f32" else torch.float64
    d_rays = torch.tensor(np.array(rays), dtype=tdt, device="cuda:0").contiguous()
    with _handle(gpu, "s4_3", prec) as h:
        for ip in (False, True):
            full = h.cast(rays, want_normal=True, inplace=ip)
            assert np.array_equal(full[0], ref["prim"]) and np.array_equal(full[1], ref["t"])
            for wp, wt, wn in SUBSETS:
                _poison(h, n)
                got = h.cast(rays, want_prim=wp, want_t=wt, want_normal=wn, inplace=ip)
                for g, f, w in zip(got, full, (wp, wt, wn)):
                    assert (g is None) if not w else _same(g, f), (ip, wp, wt, wn)
            for wp, wt, wn in SUBSETS + [(True, True, True)]:
                d_prim = torch.full((n + 64,), -77, dtype=torch.int32, device="cuda:0")
                d_t = torch.full((n + 64,), 12345.0, dtype=tdt, device="cuda:0")
                d_n = torch.full((3 * (n + 64),), 12345.0, dtype=tdt, device="cuda:0")
                torch.cuda.synchronize()
                st = torch.cuda.current_stream()
                h.cast_device(d_rays.data_ptr(), n, d_prim.data_ptr() if wp else 0, d_t.data_ptr() if wt else 0, d_n.data_ptr() if wn else 0, st.cuda_stream, inplace=ip)
                st.synchronize()
                g_prim, g_t, g_n = d_prim.cpu().numpy(), d_t.cpu().numpy(), d_n.cpu().numpy()
                for g, f, w, m, sentinel in ((g_prim, full[0], wp, n, -77), (g_t, full[1], wt, n, 12345.0), (g_n, full[2].reshape(-1), wn, 3 * n, 12345.0)):
                    assert (g[m:] == sentinel).all(), (ip, wp, wt, wn)
                    assert _same(g[:m], f) if w else (g[:m] == sentinel).all(), (ip, wp, wt, wn)
