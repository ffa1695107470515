"""GPU: the claims of spira_hits.h that tests/test_gpu_hits.py never reaches, each against the yardstick of tests/hits_support.py (hits_support.reference,
hits_support.cut) and always with numpy.array_equal on the bytes of prim, t and count (the total under count_all) — no tolerance, no measurement:
  * pruning at the bound (argument (d)): far origins in four placements of the mesh, where lists of K are cut between candidates of bit-equal t, with the
    invalid twins interleaved and the t windows; the same after an update and after a rebuild;
  * the list capacities: K = 4 (a full register list), 5 (the smallest scratch list), 8, 15 (scratch lists shorter than their capacity) and 16, on far
    rays through ten nested shells with up to 25 candidates;
  * axis-parallel and in-plane rays, signed zeros, origins on the root box's planes, zero-extent leaf boxes, where COUNT_ALL keeps best at +Inf;
  * ties at every slot between duplicated triangles, an odd K cutting a pair in half;
  * the device form into sentinel-filled buffers with a guard row, and every subset of its outputs;
  * the session knobs on lists that split evenly over the plan's waves and that do not;
  * a list long enough for a second trip of k_hits' grid-stride loop — the lane's list is used again — and for the capped session plan.
Before every compared host-form call the staging is poisoned (hits_support.poison): an output slot a kernel never stores cannot hold an earlier call's
right answer.  The sets come from hits_support.py; tests/test_hits_edges_cpu.py asserts without a device that they reach what they are for."""
import functools
import itertools

import numpy as np
import pytest

import cast_support as S
import hits_support as H
import nearest_support as N
from spira_hip import query
from test_gpu_bvh import _with_env
from test_gpu_cast import _device_frame
from test_gpu_cast_edges import P_LONG, _long_n, _moved, _num_cus, _same, _upload
from test_gpu_hits import FLAGS, _check, _open

pytestmark = pytest.mark.gpu

KS = (1, 2, 3, 4, 5, 8, 15, 16)
SENT_PRIM, SENT_T, SENT_COUNT = -77, -12345.0, 77


def _twins(at):
    """For _check: every slot of a twin holds -3 / 0 with count 0, and the ray before it does not answer -3."""
    def also(K, inplace, count_all, g_prim, g_t, g_count):
        assert (g_prim[at] == -3).all() and not g_t[at].any() and not g_count[at].any(), (K, inplace, count_all)
        assert (g_prim[at - 1] != -3).all(), (K, inplace, count_all)
    return also


# ------------------------------------------------------------------------------------------------ 1: far origins, four placements
@pytest.mark.parametrize("fi", range(len(S.FRAMES)))
@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_far_origins(gpu, prec, fi):
    """Argument (d): a candidate AT the bound is still tested, though the tree prunes with the bound rounded up from (bound - t0) x scale — 60 .. 64
    normalised units from the mesh, where t0 is large and a Float32 t has a large ulp.  These sets never hold more than 8 candidates."""
    ref = H.far_ref(prec, fi)
    sc = ref["sc"]
    with _open(gpu, S.far_set(prec, fi)["scene"], prec) as h:
        centre, scale = _device_frame(gpu, h)
        assert np.array_equal(centre, sc.frame[0]) and scale == sc.frame[1]
        _check(h, ref, ks=(1, 2, 3, 4, 5, 8), also=_twins(np.arange(1, 2 * S.N_FAR, 2)))


# ------------------------------------------------------------------------------------------------ 2: long lists at far origins
@pytest.mark.parametrize("fi", range(len(S.FRAMES)))
@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_long_lists_at_far_origins(gpu, prec, fi):
    """Lists of 4, 5, 8, 15 and 16 that fill: far rays through the centre of ten nested shells, 17 .. 25 candidates on most of them."""
    ref = H.shells_far_ref(prec, fi)
    with _open(gpu, ref["scene"], prec) as h:
        centre, scale = _device_frame(gpu, h)
        assert np.array_equal(centre, ref["sc"].frame[0]) and scale == ref["sc"].frame[1]
        _check(h, ref, ks=KS, also=_twins(np.arange(1, 2 * H.N_SHELLS_FAR, 2)))


# ------------------------------------------------------------------------------------------------ 3: far origins after an update and after a rebuild
@pytest.mark.parametrize("how", ["update", "rebuild"])
@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_far_origins_after_an_update_and_after_a_rebuild(gpu, prec, how):
    """After an update the boxes carry refit_pad and the tree keeps its frame; after a rebuild the frame is the fresh build's of the deformed mesh.  The
    far rays are built in the frame that holds and scanned against the deformed triangles.  Host form."""
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
        sc = S.Scan(H._oracle(), B, prec, frame=want)
        fs = S.far_rays_in(sc, B, seed=17, n=n, n_win=24)
        assert fs["far"]["valid"].all() and 4 * (fs["far"]["prim"] >= sc.ns).sum() >= 3 * n and not fs["twins"]["valid"].any() and len(fs["sel"]) == 24
        ref = H.reference(B, prec, S.far_joined(fs)["rays"], frame=want)
        tot = H.totals(ref)
        print(prec, how, "rays", len(tot), "valid", int((tot >= 0).sum()), "most candidates", int(tot.max()), "bit-equal t at slots K-1 / K:",
              {K: H.straddles(ref["cands"], K) for K in (1, 2, 4, 5)})
        assert (tot >= 0).sum() == n + 6 * 24 and tot.max() >= 2
        _check(h, ref, ks=(1, 2, 4, 5), also=_twins(np.arange(1, 2 * n, 2)))


# ------------------------------------------------------------------------------------------------ 4: axis rays, bounding planes, squares
@pytest.mark.parametrize("which", ["axis", "quads"])
@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_axis_rays_planes_and_squares(gpu, prec, which):
    """rcp_fast(0) is +-Inf in Float32 and NaN in Float64, a slab distance may be 0 or 0 x Inf, leaf boxes have zero extent: nothing the scan accepts may
    be pruned, and under COUNT_ALL — best stays what bvh8_enter made of t_max = +Inf — every candidate is counted once."""
    ref = H.axis_ref(prec) if which == "axis" else H.quad_ref(prec)
    total = H.totals(ref).astype(np.uint32)
    n = len(ref["rays"])
    with _open(gpu, ref["scene"], prec) as h:
        _check(h, ref, ks=(1, 2, 3, 4, 5, 16))
        for ip in (False, True):
            H.poison(h, n, 0, ip)
            assert np.array_equal(query.count_hits(h, ref["rays"], inplace=ip), total), ip


# ------------------------------------------------------------------------------------------------ 5: ties at every slot
@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_ties_at_every_slot(gpu, prec):
    """Duplicated triangles: the candidates come in pairs of bit-equal t, the later index first.  An odd K cuts a pair in half and keeps the later index."""
    ref = H.dup_ref(prec)
    pair = ref["pair"]
    assert H.pairs_hold(ref) and all(H.straddles(ref["cands"], K) >= 8 for K in (1, 3, 5))
    tot = H.totals(ref)

    def also(K, inplace, count_all, g_prim, g_t, g_count):
        for m in range(0, K - 1, 2):
            both = g_prim[:, m + 1] >= 0
            assert _same(g_t[both, m], g_t[both, m + 1]) and (g_prim[both, m] > g_prim[both, m + 1]).all(), (K, inplace, count_all, m)
            assert np.array_equal(pair[g_prim[both, m]], g_prim[both, m + 1]), (K, inplace, count_all, m)
        if K % 2:
            cut = tot > K
            assert cut.sum() >= 8 and (g_prim[cut, K - 1] > pair[g_prim[cut, K - 1]]).all(), (K, inplace, count_all)

    with _open(gpu, ref["scene"], prec) as h:
        _check(h, ref, ks=(1, 2, 3, 4, 5, 16), also=also)


# ------------------------------------------------------------------------------------------------ 6: device form, sentinels, output subsets
def _hits_on_device(h, d_rays, K, stream, inplace=False, count_all=False, want=(True, True, True)):
    """The device form on `stream` into buffers pre-filled with sentinels no answer can be, one guard row behind the list: tensors (prim [n + 1, K],
    t [n + 1, K], count [n + 1]), all of them returned whether they were passed or not."""
    import torch
    n = d_rays.shape[0]
    prim = torch.full((n + 1, K), SENT_PRIM, dtype=torch.int32, device="cuda:0")
    t = torch.full((n + 1, K), SENT_T, dtype=d_rays.dtype, device="cuda:0")
    count = torch.full((n + 1,), SENT_COUNT, dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()
    h.cast_hits_device(d_rays.data_ptr(), n, K, prim.data_ptr() if want[0] else 0, t.data_ptr() if want[1] else 0, count.data_ptr() if want[2] else 0,
                       stream.cuda_stream, inplace=inplace, count_all=count_all)
    stream.synchronize()
    return prim, t, count


SUBSETS = [c for c in itertools.product((False, True), repeat=3) if any(c) and not all(c)]      # (want_prim, want_t, want_count)


@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_device_form_sentinels_and_output_subsets(gpu, prec):
    import torch
    ref = H.shells_far_ref(prec, 3)
    rays, n = ref["rays"], len(ref["rays"])
    T = ref["sc"].T
    d_rays = torch.tensor(np.asarray(rays, dtype=T), device="cuda:0").contiguous()
    st = torch.cuda.Stream()
    sent = (SENT_PRIM, SENT_T, SENT_COUNT)
    with _open(gpu, ref["scene"], prec) as h:
        for K in KS:
            prim, t, count, total = H.cut(ref["cands"], ref["prepared"], T, K)
            for ip, ca in FLAGS:
                H.poison(h, n, K, ip)
                host = h.cast_hits(rays, K, inplace=ip, count_all=ca)
                assert np.array_equal(host[0], prim) and _same(host[1], t) and np.array_equal(host[2], total if ca else count), (K, ip, ca)
                dev = [o.cpu().numpy() for o in _hits_on_device(h, d_rays, K, st, inplace=ip, count_all=ca)]
                for g, f, s in zip(dev, host, sent):
                    assert (g[n:] == s).all(), (K, ip, ca)                             # the guard row is untouched
                    assert (g[:n] != s).all(), (K, ip, ca)                             # no sentinel is left inside the list
                    assert _same(g[:n].view(f.dtype), f), (K, ip, ca)                  # the host form's bytes
        for K in (4, 5):
            for ip in (False, True):
                full = [o.cpu().numpy() for o in _hits_on_device(h, d_rays, K, st, inplace=ip)]
                for want in SUBSETS:
                    got = [o.cpu().numpy() for o in _hits_on_device(h, d_rays, K, st, inplace=ip, want=want)]
                    for g, f, w, s in zip(got, full, want, sent):
                        assert _same(g, f) if w else (g == s).all(), (K, ip, want)


# ------------------------------------------------------------------------------------------------ 7: session knobs
@pytest.mark.parametrize("n", [1000, 999])
@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_session_knobs(gpu, prec, n):
    """SPIRA_CAST_REFILL 1 and 64 (a refill after every finished lane / only when the whole wave is free, where a lane's deferred store waits longest) with
    one wave per CU, on 1 000 rays that split evenly over the plan's waves and on 999 that do not: the session's bytes are the in-place bytes, and both
    the scan's on the list's first period."""
    ref = H.shells_far_ref(prec, 0)
    T = ref["sc"].T
    m = len(ref["rays"])
    rays = np.ascontiguousarray(ref["rays"][np.arange(n) % m])
    with _open(gpu, ref["scene"], prec) as h:
        want = {}
        for K in (4, 5, 15):
            prim, t, count, total = H.cut(ref["cands"], ref["prepared"], T, K)
            for ca in (False, True):
                H.poison(h, n, K, True)
                w = want[(K, ca)] = h.cast_hits(rays, K, inplace=True, count_all=ca)
                assert np.array_equal(w[0][:m], prim) and _same(w[1][:m], t) and np.array_equal(w[2][:m], total if ca else count), (K, ca)
        for refill in ("1", "64"):
            def go():
                plan = gpu.cast_plan(n, 256)
                assert plan["refill_free"] == int(refill) and (plan["rem"] == 0) == (n == 1000), plan
                for (K, ca), w in want.items():
                    H.poison(h, n, K, False)
                    got = h.cast_hits(rays, K, count_all=ca)
                    for a, b in zip(got, w):
                        assert _same(a, b), (refill, K, ca)
            _with_env(gpu, {"SPIRA_CAST_REFILL": refill, "SPIRA_CAST_WAVES_PER_CU": "1"}, go)


# ------------------------------------------------------------------------------------------------ 8: a long list
@functools.lru_cache(maxsize=None)
def _long_ref():
    scene = N.scene("ico33")
    rng = np.random.default_rng(13)
    return dict(H.reference(scene, "f32", S.aim_at_triangles(rng, S.rays_b(rng, scene, P_LONG), scene)), scene=scene)


def test_long_list_f32(gpu):
    """More rays than 64 x 256 x num_cus: k_hits takes a second trip of its grid-stride loop — a lane's HitsLane, at capacity 16 a scratch list, is used
    again — and the session plan has stopped adding waves.  Device form only (the host form at this size: the open finding of test_gpu_cast_edges.py);
    the list is tiled on the device and every period of prim, t and count is compared there with the first, the first with the scan."""
    import torch
    num_cus = _num_cus()
    n = _long_n(num_cus)
    plan = gpu.cast_plan(n, num_cus)
    print("num_cus", num_cus, "rays", n, "plan", plan)
    assert n % P_LONG == 0 and n - P_LONG <= 64 * 256 * num_cus + 1000 < n
    assert plan["grid_flat"] * 256 < n and plan["waves"] == num_cus * 20, plan      # the flat grid strides; the session plan is at the device's capacity
    assert n * 5 < 1 << 26                                                          # hits_check's limit on n_rays x max_hits
    ref = _long_ref()
    tot = H.totals(ref)
    assert ref["valid"].all() and (tot >= 2).sum() > P_LONG // 8 and (tot == 0).sum() > P_LONG // 8
    k = n // P_LONG
    d_tiled = _upload(ref["rays"], "f32").repeat(k, 1).contiguous()
    assert d_tiled.shape == (n, 8)
    st = torch.cuda.Stream()
    with _open(gpu, ref["scene"], "f32") as h:
        for K in (2, 5):
            prim, t, count, total = H.cut(ref["cands"], ref["prepared"], np.float32, K)
            for ip in (False, True):
                outs = _hits_on_device(h, d_tiled, K, st, inplace=ip)
                heads = []
                for o, s in zip(outs, (SENT_PRIM, SENT_T, SENT_COUNT)):
                    assert bool((o[n:] == s).all()), (K, ip)
                    b = o[:n].contiguous().view(k, -1).view(torch.int32)
                    bad = torch.nonzero((b != b[0]).any(dim=1)).flatten()
                    assert bad.numel() == 0, (K, ip, o.dtype, bad[:8].cpu().numpy())      # output i is output i mod P, everywhere
                    heads.append(o[:P_LONG].cpu().numpy())
                del outs
                assert np.array_equal(heads[0], prim) and _same(heads[1], t) and np.array_equal(heads[2].view(np.uint32), count), (K, ip)
