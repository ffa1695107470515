"""GPU (MI355X): all-sky runs (csrc/spira_device.h, PathArgs::sky_runs; csrc/spira_sky.h) — in a pixel-owning pass of a Float64
sphere scene a run of 4 adjacent pixels none of whose camera rays can reach a sphere never enters k_path's loop: the wave sums the run's sky terms
ahead of it, in sample order, and the sums reach the accumulator with the wave's other pixels.  Only where the terms are added changes: with
SPIRA_SKY_RUNS=0 (every path through the loop: the same dealing of all the others) the images are the same bits and every counter the same number,
and with SPIRA_FUSED_RESOLVE=0 (round-robin dealing + k_resolve) the images and the pinned counters are."""
import numpy as np
import pytest

from spira_hip import distributed as D
from spira_hip import scenes
from test_gpu_parity import _args, _counts
from test_gpu_specdiv import _Env

pytestmark = pytest.mark.gpu

PINNED = ("samples", "segments", "radiance_rmw", "radiance_stores", "passes", "bounce_launches")
W, H = 97, 55                 # 5 335 pixels: runs straddle row ends, the tile ends with an incomplete run, the last wave's pixels lie past the tile
SMALL = (9, 5)                # 45 pixels: less than one wave's 64
MODES = (("sky", {}), ("loop", dict(SPIRA_SKY_RUNS=0)), ("resolve", dict(SPIRA_FUSED_RESOLVE=0)))


def _three(gpu, s, params, **env):
    """default (all-sky runs summed ahead of the loop) / every path through the loop / round-robin dealing + k_resolve"""
    out = {}
    for name, kv in MODES:
        with _Env(**dict(env, **kv)):
            hdr, _ = gpu.render(*_args(s), params, "f64")
            out[name] = (hdr, gpu.counters())
    return out


def _same(out, what):
    h, c = out["sky"]
    for other in ("loop", "resolve"):
        h0, c0 = out[other]
        assert np.array_equal(h, h0), (what, other, float(np.abs(h - h0).max()))
        for k in PINNED:
            assert c[k] == c0[k], (what, other, k, c[k], c0[k])
        assert c0["sky_pixels"] == 0, (what, other, c0["sky_pixels"])
    c0 = out["loop"][1]
    assert c["rays_enqueued"] == c0["rays_enqueued"] and c["launches"] == c0["launches"], (what, c, c0)      # the others are dealt as before
    return c["sky_pixels"]


def _host_sky_pixels(gpu, s, w, h):
    """What the exported classifier gives on the host: pixels of complete runs of 4 inside the (whole-frame) tile whose four pixels are all sky."""
    sph = np.asarray(s["spheres5"], dtype=np.float64)
    sky = np.array([gpu.sky_pixel(s["camera12"], w, h, p % w + 1, h - p // w, sph) for p in range(w * h)], dtype=bool)      # row 0 is the top: j = H
    runs = sky[: (w * h) // 4 * 4].reshape(-1, 4).all(axis=1)
    return 4 * int(runs.sum())


def _with_camera(gpu, s, position, look_at, up, fov):
    return dict(s, camera12=gpu.camera_lookat(position, look_at, up, fov, np.float32(16.0 / 9.0), prec="f32").astype(np.float64))


@pytest.mark.parametrize("size", [(W, H), SMALL], ids=["97x55", "9x5"])
@pytest.mark.parametrize("spp,passes", [(1, 1), (3, 1), (64, 1), (65, 2), (130, 3)])
def test_same_bits_over_spp_and_tiles(gpu, size, spp, passes):
    """One slot, partial rows of slots, a full wave of slots, two passes (33 + 32 slots) and three (44 + 43 + 43): later passes start from accum."""
    w, h = size
    s = scenes.scene_s1()
    ns, nm, nt = _counts(s)
    out = _three(gpu, s, gpu.make_params(w, h, spp, 8, ns, nm, nt, flags=gpu.POST_NONE, seed=31, batch_rays=64 * w * h))
    assert out["sky"][1]["passes"] == passes
    n = _same(out, (size, spp))
    assert n == passes * _host_sky_pixels(gpu, s, w, h), (size, spp, n)      # (every pass of the call sums them)


@pytest.mark.parametrize("depth", [1, 8])
def test_same_bits_over_depth(gpu, depth):
    s = scenes.scene_s1()
    ns, nm, nt = _counts(s)
    assert _same(_three(gpu, s, gpu.make_params(W, H, 6, depth, ns, nm, nt, flags=gpu.POST_NONE, seed=17)), depth) > 0


def test_counter_is_the_host_count(gpu):
    """S1 at 97x55: the kernel sums exactly the runs the exported function calls sky, and there are some."""
    s = scenes.scene_s1()
    ns, nm, nt = _counts(s)
    n = _same(_three(gpu, s, gpu.make_params(W, H, 4, 8, ns, nm, nt, flags=gpu.POST_NONE, seed=3)), "count")
    want = _host_sky_pixels(gpu, s, W, H)
    assert n == want and want > 0, (n, want)


def test_same_bits_progressive(gpu):
    s = scenes.scene_s1()
    ns, nm, nt = _counts(s)
    sums = {}
    for name, kv in MODES:
        acc = np.zeros((3, H, W), dtype=np.float64)
        s0 = 0
        with _Env(**kv):
            for n in (5, 64):             # two calls: the second starts from the first's sums
                gpu.accumulate(*_args(s), gpu.make_params(W, H, n, 6, ns, nm, nt, seed=8), s0, acc, None, "f64")
                s0 += n
        sums[name] = acc
    assert np.array_equal(sums["sky"], sums["resolve"]) and np.array_equal(sums["sky"], sums["loop"])


def test_same_bits_dealt_rows(gpu):
    s = scenes.scene_s1()
    ns, nm, nt = _counts(s)
    total = 0
    for rank in range(3):                 # rows dealt round-robin in stripes of 4 over three ranks: a tile's neighbouring rows are 8 frame rows apart
        tp = D.tile_params(H, 3, rank, 4)
        total += _same(_three(gpu, s, gpu.make_params(W, H, 12, 8, ns, nm, nt, flags=gpu.POST_NONE, seed=9, **tp)), ("rank", rank))
    assert total > 0


@pytest.mark.parametrize("spec", [2, 0])
def test_same_bits_speculative_division(gpu, spec):
    """SPIRA_SPEC_DIV=2: every wave is rendered again by the exact launch — it classifies the same runs, sums them again and adds them once; 0: one
    exact launch."""
    s = scenes.scene_s1()
    ns, nm, nt = _counts(s)
    p = gpu.make_params(W, H, 16, 8, ns, nm, nt, flags=gpu.POST_NONE, seed=12)
    out = _three(gpu, s, p, SPIRA_SPEC_DIV=spec)
    assert (out["sky"][1]["redone_waves"] > 0) == (spec == 2)
    assert _same(out, ("spec", spec)) == _host_sky_pixels(gpu, s, W, H)      # counted once, too
    hdr, _ = gpu.render(*_args(s), p, "f64")        # and the same bits as the default speculation
    assert np.array_equal(hdr, out["sky"][0])


def test_same_bits_two_passes_rendered_again(gpu):
    """Every wave of both passes rendered again: the second pass's sums start from what the first left in accum, which no reported wave has touched."""
    s = scenes.scene_s1()
    ns, nm, nt = _counts(s)
    out = _three(gpu, s, gpu.make_params(W, H, 40, 8, ns, nm, nt, flags=gpu.POST_NONE, seed=5, batch_rays=20 * W * H), SPIRA_SPEC_DIV=2)
    assert out["sky"][1]["passes"] == 2
    _same(out, "spec2 x 2 passes")


def test_same_bits_slot_major(gpu):
    """SPIRA_PRIVATE_L=0: the sums wait in the slot-0 plane of the slot-major L."""
    s = scenes.scene_s1()
    ns, nm, nt = _counts(s)
    out = _three(gpu, s, gpu.make_params(W, H, 20, 8, ns, nm, nt, flags=gpu.POST_NONE, seed=23), SPIRA_PRIVATE_L=0)
    assert _same(out, "slot-major") > 0


def test_every_run_is_sky(gpu):
    """A narrow camera looking level, past the scene: no line of sight meets a sphere (the scan's disc knows no direction: the spheres behind count).
    98 x 54 = 4 x 1 323 pixels: no incomplete run."""
    w, h = 98, 54
    s = _with_camera(gpu, scenes.scene_s1(), [0, 1, 3], [10, 1, 3], [0, 1, 0], 8.0)
    ns, nm, nt = _counts(s)
    out = _three(gpu, s, gpu.make_params(w, h, 20, 8, ns, nm, nt, flags=gpu.POST_NONE, seed=2))
    assert _same(out, "all sky") == w * h
    assert out["sky"][1]["rays_enqueued"] == 0 and out["sky"][1]["segments"] == w * h * 20


def test_no_run_is_sky(gpu):
    """Straight down at the ground."""
    s = _with_camera(gpu, scenes.scene_s1(), [0, 1, 3], [0, 0, 3], [0, 0, -1], 40.0)
    ns, nm, nt = _counts(s)
    assert _same(_three(gpu, s, gpu.make_params(W, H, 8, 8, ns, nm, nt, flags=gpu.POST_NONE, seed=2)), "no sky") == 0


def test_full_size(gpu):
    """The benchmark's shape: 1080p, 64 slots in one pass."""
    s = scenes.scene_s1()
    ns, nm, nt = _counts(s)
    n = _same(_three(gpu, s, gpu.make_params(1920, 1080, 64, 8, ns, nm, nt, flags=gpu.POST_NONE, seed=1)), "1080p")
    assert 0.24 * 1920 * 1080 <= n <= 0.272 * 1920 * 1080, n
