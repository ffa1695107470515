"""GPU (MI355X): the per-wave pixel table and the reach masks of the pixel-owning passes (csrc/spira_device.h, PathArgs::pixel_table / reach_masks;
csrc/spira_sky.h, pixel_reach) — a camera row of k_path's loop reads its pixel's facts from LDS instead of dividing and hashing per
path, and its scan visits only the spheres its run of 4 pixels can reach.  Only where the words come from and which spheres are asked changes: with both
knobs off, with either off alone and with SPIRA_FUSED_RESOLVE=0 (round-robin dealing + k_resolve) the images are the same bits and the counters the
same numbers (against SPIRA_FUSED_RESOLVE=0: those that do not count its resolve launch or the dealing — the pinned set of test_gpu_sky_runs.py)."""
import numpy as np
import pytest

from spira_hip import distributed as D
from spira_hip import scenes
from test_gpu_parity import _args, _close, _counts
from test_gpu_specdiv import _Env

pytestmark = pytest.mark.gpu

COUNTERS = ("segments", "radiance_stores", "radiance_rmw", "rays_enqueued", "sky_pixels", "launches", "passes")
PINNED = ("segments", "radiance_stores", "radiance_rmw", "passes")      # what round-robin dealing + k_resolve keeps
W, H = 97, 55                 # 5 335 pixels: runs straddle row ends, the tile ends with an incomplete run, the last wave's pixels lie past the tile
SMALL = (9, 5)                # 45 pixels: less than one wave's 64
MODES = (("new", {}), ("neither", dict(SPIRA_PIXEL_TABLE=0, SPIRA_REACH_MASKS=0)), ("no_table", dict(SPIRA_PIXEL_TABLE=0)),
         ("no_masks", dict(SPIRA_REACH_MASKS=0)), ("resolve", dict(SPIRA_FUSED_RESOLVE=0)))


def _all(gpu, s, params, **env):
    out = {}
    for name, kv in MODES:
        with _Env(**dict(env, **kv)):
            hdr, _ = gpu.render(*_args(s), params, "f64")
            out[name] = (hdr, gpu.counters())
    return out


def _same(out, what):
    h, c = out["new"]
    for other in ("neither", "no_table", "no_masks", "resolve"):
        h0, c0 = out[other]
        assert np.array_equal(h, h0), (what, other, float(np.abs(h - h0).max()))
        for k in (PINNED if other == "resolve" else COUNTERS):
            assert c[k] == c0[k], (what, other, k, c[k], c0[k])
    return c


def _with_camera(gpu, s, position, look_at, up, fov):
    return dict(s, camera12=gpu.camera_lookat(position, look_at, up, fov, np.float32(16.0 / 9.0), prec="f32").astype(np.float64))


def _small_spheres(s, n):
    """n small spheres on a grid in front of S1's camera, S1's materials in turn: with n > 32 the last rows have no bit in a reach mask."""
    k = np.arange(n)
    sph = np.stack([-1.4 + 0.4 * (k % 8), -0.6 + 0.35 * (k // 8), np.zeros(n), np.full(n, 0.12), 1 + k % 5], axis=1)
    return dict(s, spheres5=np.asarray(sph, dtype=np.float32).astype(np.float64))


@pytest.mark.parametrize("size", [(W, H), SMALL], ids=["97x55", "9x5"])
@pytest.mark.parametrize("spp,passes", [(1, 1), (3, 1), (64, 1), (65, 2), (130, 3)])
def test_same_bits_over_spp_and_tiles(gpu, size, spp, passes):
    """k_eff 1 and 3 (a row of 16 slots spans runs: the mask is all ones, the table is still read), 64 (rows inside one run), two passes (33 + 32 slots)
    and three (44 + 43 + 43)."""
    w, h = size
    s = scenes.scene_s1()
    ns, nm, nt = _counts(s)
    out = _all(gpu, s, gpu.make_params(w, h, spp, 8, ns, nm, nt, flags=gpu.POST_NONE, seed=31, batch_rays=64 * w * h))
    assert _same(out, (size, spp))["passes"] == passes


@pytest.mark.parametrize("depth", [1, 8])
def test_same_bits_over_depth(gpu, depth):
    s = scenes.scene_s1()
    ns, nm, nt = _counts(s)
    _same(_all(gpu, s, gpu.make_params(W, H, 16, depth, ns, nm, nt, flags=gpu.POST_NONE, seed=17)), depth)


def test_same_bits_progressive(gpu):
    s = scenes.scene_s1()
    ns, nm, nt = _counts(s)
    sums = {}
    for name, kv in MODES:
        acc = np.zeros((3, H, W), dtype=np.float64)
        s0 = 0
        with _Env(**kv):
            for n in (5, 64):             # two calls: the second's samples start at 5 (PixelEntry holds no sample: the slot and sample0 give it)
                gpu.accumulate(*_args(s), gpu.make_params(W, H, n, 6, ns, nm, nt, seed=8), s0, acc, None, "f64")
                s0 += n
        sums[name] = acc
    for name, _ in MODES[1:]:
        assert np.array_equal(sums["new"], sums[name]), name


def test_same_bits_dealt_rows(gpu):
    """Rows dealt round-robin in stripes of 4 over three ranks: j comes from ref_row_j, through the table."""
    s = scenes.scene_s1()
    ns, nm, nt = _counts(s)
    for rank in range(3):
        tp = D.tile_params(H, 3, rank, 4)
        _same(_all(gpu, s, gpu.make_params(W, H, 16, 8, ns, nm, nt, flags=gpu.POST_NONE, seed=9, **tp)), ("rank", rank))


@pytest.mark.parametrize("spec", [2, 0])
def test_same_bits_speculative_division(gpu, spec):
    """SPIRA_SPEC_DIV=2: every wave is rendered again by the exact launch, which fills its own table and masks; 0: one exact launch."""
    s = scenes.scene_s1()
    ns, nm, nt = _counts(s)
    p = gpu.make_params(W, H, 16, 8, ns, nm, nt, flags=gpu.POST_NONE, seed=12)
    out = _all(gpu, s, p, SPIRA_SPEC_DIV=spec)
    assert (out["new"][1]["redone_waves"] > 0) == (spec == 2)
    _same(out, ("spec", spec))
    hdr, _ = gpu.render(*_args(s), p, "f64")        # and the same bits as the default speculation
    assert np.array_equal(hdr, out["new"][0])


def test_same_bits_slot_major(gpu):
    s = scenes.scene_s1()
    ns, nm, nt = _counts(s)
    _same(_all(gpu, s, gpu.make_params(W, H, 32, 8, ns, nm, nt, flags=gpu.POST_NONE, seed=23), SPIRA_PRIVATE_L=0), "slot-major")


CAMERAS = {
    "s1": None,
    "sky_alone": ([0, 1, 3], [10, 1, 3], [0, 1, 0], 8.0),                # level, past the scene: no line of sight meets a sphere
    "inside_ground": ([0, -50, 0], [0, -50, -1], [0, 1, 0], 40.0),       # inside the radius-100 ground sphere: its bit is set in every mask
    "small_behind": ([0, 0.2, -3], [0, 0.2, -6], [0, 1, 0], 40.0),       # the three small spheres behind the camera: the folded angle keeps their bits
}


@pytest.mark.parametrize("cam", sorted(CAMERAS))
def test_same_bits_cameras(gpu, cam):
    s = scenes.scene_s1()
    if CAMERAS[cam] is not None:
        s = _with_camera(gpu, s, *CAMERAS[cam])
    ns, nm, nt = _counts(s)
    c = _same(_all(gpu, s, gpu.make_params(W, H, 16, 8, ns, nm, nt, flags=gpu.POST_NONE, seed=2)), cam)
    if cam == "sky_alone":
        assert c["sky_pixels"] == W * H // 4 * 4 and c["rays_enqueued"] == 0
    if cam == "inside_ground":
        assert c["sky_pixels"] == 0


@pytest.mark.parametrize("n", [32, 40])
def test_same_bits_many_spheres(gpu, n):
    """32 spheres: every bit of the mask is used; 40: beyond the 32-bit mask the rows scan everything, and a pixel that sees sphere 32 + alone is no sky."""
    s = _small_spheres(scenes.scene_s1(), n)
    ns, nm, nt = _counts(s)
    assert ns == n
    c = _same(_all(gpu, s, gpu.make_params(W, H, 16, 4, ns, nm, nt, flags=gpu.POST_NONE, seed=4)), n)
    sph = np.asarray(s["spheres5"], dtype=np.float64)
    sky = np.array([gpu.sky_pixel(s["camera12"], W, H, p % W + 1, H - p // W, sph) for p in range(W * H)], dtype=bool)
    assert c["sky_pixels"] == 4 * int(sky[: W * H // 4 * 4].reshape(-1, 4).all(axis=1).sum()) > 0


def test_oracle(gpu, oracle):
    """97 x 55, spp 3 (rows span runs) and spp 16 (rows inside runs: the masked scan) against the CPU oracle, at the suite's tolerance."""
    s = scenes.scene_s1()
    ns, nm, nt = _counts(s)
    for spp in (3, 16):
        hdr, _ = gpu.render(*_args(s), gpu.make_params(W, H, spp, 8, ns, nm, nt, flags=gpu.POST_NONE, seed=6), "f64")
        segments = gpu.counters()["segments"]
        ohdr, _, oseg = oracle.render(*_args(s), oracle.make_params(W, H, spp, 8, ns, nm, nt, seed=6), "f64")
        nbad, worst = _close(hdr, ohdr)
        assert nbad == 0 and segments == oseg, (spp, nbad, worst, segments, oseg)


def test_full_size(gpu):
    """The benchmark's shape: 1080p, 64 slots in one pass."""
    s = scenes.scene_s1()
    ns, nm, nt = _counts(s)
    c = _same(_all(gpu, s, gpu.make_params(1920, 1080, 64, 8, ns, nm, nt, flags=gpu.POST_NONE, seed=1)), "1080p")
    assert c["sky_pixels"] == 560856
