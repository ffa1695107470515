"""GPU (MI355X): k_path_own (csrc/spira_device.h; its statements: csrc/spira_path_body.h, FIXED; the dispatch: csrc/spira_plan.h, own_kernel_ok;
DESIGN.md §4) — the full pixel-owning pass of 64 slots of a Float64 sphere scene in a kernel of its own, in which what k_path decides per sub-chunk
from its arguments is a compile-time constant.  Only which kernel runs the pass changes: against SPIRA_OWN_KERNEL=0 (k_path, same library) the images
are the same bits and the counters the same numbers, and spira_get_own_passes says which passes the new kernel rendered — what the plan says
(tests/native/own_dispatch.cpp has the same table on the host): the planner makes a call's passes equal, so at 64 slots per pass spp 128 is 64 + 64
(both own), spp 127 is 64 + 63 (own, then k_path's tail) and spp 130 is 44 + 43 + 43 (all k_path's)."""
import numpy as np
import pytest

from spira_hip import distributed as D
from spira_hip import scenes
from test_gpu_parity import _args, _close, _counts
from test_gpu_pixel_table import CAMERAS, _small_spheres, _with_camera
from test_gpu_specdiv import _Env

pytestmark = pytest.mark.gpu

COUNTERS = ("segments", "radiance_stores", "radiance_rmw", "rays_enqueued", "sky_pixels", "launches", "passes", "redone_waves")
W, H = 97, 55                 # 5 335 pixels, 84 waves: runs straddle row ends, the last wave has pixels past the tile
SMALL = (9, 5)                # 45 pixels: one wave, 19 of its pixels past the tile


def _pair(gpu, s, params, own, what, **env):
    """The render with the kernel of its own and with SPIRA_OWN_KERNEL=0: same bits, same counters; `own` passes in k_path_own (None: every pass), none with the knob off."""
    with _Env(**env):
        hdr, _ = gpu.render(*_args(s), params, "f64")
        c, n = gpu.counters(), gpu.own_passes()
    with _Env(**dict(env, SPIRA_OWN_KERNEL=0)):
        hdr0, _ = gpu.render(*_args(s), params, "f64")
        c0, n0 = gpu.counters(), gpu.own_passes()
    assert n == (c["passes"] if own is None else own) and n0 == 0, (what, n, own, c["passes"], n0)
    assert np.array_equal(hdr, hdr0), (what, float(np.abs(hdr - hdr0).max()))
    for k in COUNTERS:
        assert c[k] == c0[k], (what, k, c[k], c0[k])
    return hdr, c


def _params(gpu, s, w, h, spp, depth, seed, **kw):
    ns, nm, nt = _counts(s)
    return gpu.make_params(w, h, spp, depth, ns, nm, nt, flags=gpu.POST_NONE, seed=seed, batch_rays=64 * w * h, **kw)


@pytest.mark.parametrize("size", [(W, H), SMALL], ids=["97x55", "9x5"])
@pytest.mark.parametrize("spp,passes,own", [(64, 1, 1), (128, 2, 2), (130, 3, 0), (127, 2, 1), (6, 1, 0)])
def test_same_bits_over_spp_and_tiles(gpu, size, spp, passes, own):
    w, h = size
    s = scenes.scene_s1()
    _, c = _pair(gpu, s, _params(gpu, s, w, h, spp, 8, 31), own, (size, spp))
    assert c["passes"] == passes


@pytest.mark.parametrize("depth", [1, 8])
def test_same_bits_over_depth(gpu, depth):
    s = scenes.scene_s1()
    _pair(gpu, s, _params(gpu, s, W, H, 64, depth, 17), 1, depth)


def test_same_bits_progressive(gpu):
    """Two calls of 64 samples: the second starts at sample 64 and adds to the sums of the first (accum_first off)."""
    s = scenes.scene_s1()
    sums = {}
    for knob in (1, 0):
        acc = np.zeros((3, H, W), dtype=np.float64)
        with _Env(SPIRA_OWN_KERNEL=knob):
            for call in range(2):
                gpu.accumulate(*_args(s), _params(gpu, s, W, H, 64, 6, 8), 64 * call, acc, None, "f64")
                assert gpu.own_passes() == knob
        sums[knob] = acc
    assert np.array_equal(sums[1], sums[0])


def test_same_bits_dealt_rows(gpu):
    """Rows dealt round-robin in stripes of 4 over three ranks."""
    s = scenes.scene_s1()
    for rank in range(3):
        tp = D.tile_params(H, 3, rank, 4)
        ns, nm, nt = _counts(s)
        _pair(gpu, s, gpu.make_params(W, H, 64, 8, ns, nm, nt, flags=gpu.POST_NONE, seed=9, **tp), 1, ("rank", rank))


@pytest.mark.parametrize("spec", [2, 0])
def test_same_bits_speculative_division(gpu, spec):
    """SPIRA_SPEC_DIV=2: the whole pass rendered again by k_path_own<double, false>; 0: that kernel alone."""
    s = scenes.scene_s1()
    p = _params(gpu, s, W, H, 64, 8, 12)
    hdr, c = _pair(gpu, s, p, 1, ("spec", spec), SPIRA_SPEC_DIV=spec)
    assert (c["redone_waves"] > 0) == (spec == 2)
    hdr1, _ = gpu.render(*_args(s), p, "f64")           # and the same bits as the default speculation
    assert np.array_equal(hdr, hdr1)


@pytest.mark.parametrize("knob", ["SPIRA_SKY_RUNS", "SPIRA_PIXEL_TABLE", "SPIRA_REACH_MASKS", "SPIRA_PRIVATE_L", "SPIRA_FUSED_RESOLVE", "SPIRA_CAM_CONSTS"])
def test_a_knob_off_is_k_path(gpu, knob):
    """A pass without one of the facts the kernel holds as constants is k_path's — and the same image."""
    s = scenes.scene_s1()
    p = _params(gpu, s, W, H, 64, 8, 5)
    hdr, _ = gpu.render(*_args(s), p, "f64")
    assert gpu.own_passes() == 1
    with _Env(**{knob: 0}):
        hdr0, _ = gpu.render(*_args(s), p, "f64")
        assert gpu.own_passes() == 0
    assert np.array_equal(hdr, hdr0)


@pytest.mark.parametrize("cam", sorted(CAMERAS))
def test_same_bits_cameras(gpu, cam):
    s = scenes.scene_s1()
    if CAMERAS[cam] is not None:
        s = _with_camera(gpu, s, *CAMERAS[cam])
    _, c = _pair(gpu, s, _params(gpu, s, W, H, 64, 8, 2), 1, cam)
    if cam == "sky_alone":
        assert c["sky_pixels"] == W * H // 4 * 4 and c["rays_enqueued"] == 0
    if cam == "inside_ground":
        assert c["sky_pixels"] == 0


@pytest.mark.parametrize("n,own", [(32, 1), (33, 0)])
def test_same_bits_many_spheres(gpu, n, own):
    """32 spheres: every bit of the reach mask is used; 33: the mask has no bit for the last one, the pass is k_path's."""
    s = _small_spheres(scenes.scene_s1(), n)
    assert _counts(s)[0] == n
    _, c = _pair(gpu, s, _params(gpu, s, W, H, 64, 4, 4), own, n)
    assert c["sky_pixels"] > 0


def test_oracle(gpu, oracle):
    """97 x 55, spp 64, depth 8 against the CPU oracle, at the suite's tolerance, segments exact."""
    s = scenes.scene_s1()
    ns, nm, nt = _counts(s)
    hdr, _ = gpu.render(*_args(s), _params(gpu, s, W, H, 64, 8, 6), "f64")
    segments, own = gpu.counters()["segments"], gpu.own_passes()
    ohdr, _, oseg = oracle.render(*_args(s), oracle.make_params(W, H, 64, 8, ns, nm, nt, seed=6), "f64")
    nbad, worst = _close(hdr, ohdr)
    assert own == 1 and nbad == 0 and segments == oseg, (own, nbad, worst, segments, oseg)


def test_full_size(gpu):
    """The benchmark's shape: 1080p, 64 slots per pass (a frame handed to the host is rendered as row slabs, a pass each: all of them k_path_own's)."""
    s = scenes.scene_s1()
    ns, nm, nt = _counts(s)
    _, c = _pair(gpu, s, gpu.make_params(1920, 1080, 64, 8, ns, nm, nt, flags=gpu.POST_NONE, seed=1), None, "1080p")
    assert c["sky_pixels"] == 560856
