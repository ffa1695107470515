"""GPU (MI355X): pixel-owning passes (csrc/spira_device.h, PathArgs::accum) — in Float64 scenes of spheres alone each k_path wave
renders every slot of its own pixels and sums them into the image at its end, instead of k_resolve streaming the pass's radiance after the launch.
With SPIRA_FUSED_RESOLVE=1 (the default) and 0 (sub-chunks dealt round-robin, then k_resolve) the images are the same bits and the counters the
same numbers (but the queue traffic, rays_enqueued, which follows the dealing).  Everything else keeps the round-robin dealing either way: the
launch count tells which organisation ran."""
import numpy as np
import pytest

from spira_hip import distributed as D
from spira_hip import scenes
from test_gpu_parity import _args, _counts
from test_gpu_specdiv import _Env

pytestmark = pytest.mark.gpu

PINNED = ("samples", "segments", "radiance_rmw", "radiance_stores", "passes", "bounce_launches")
SCENES = {"s1": scenes.scene_s1, "s2": scenes.scene_s2, "s3": scenes.scene_s3, "glass": scenes.scene_s2_glass}
W, H = 97, 55                 # neither a multiple of the run length nor of 64 pixels: waves with pixels past the tile's end


def _flags(gpu, name):
    return gpu.POST_NONE | ((gpu.EXT_DIELECTRIC | gpu.EXT_SPECTRAL) if name == "glass" else 0)


def _both(gpu, s, params, prec, **env):
    out = {}
    for fused in (1, 0):
        with _Env(SPIRA_FUSED_RESOLVE=fused, **env):
            hdr, _ = gpu.render(*_args(s), params, prec)
            out[fused] = (hdr, gpu.counters())
    return out


def _owning(name, prec):
    return name == "s1" and prec == "f64"      # (S2, S3 hold LDS triangles; the glass scene runs the extensions)


def _same(out, engaged, what):
    (h1, c1), (h0, c0) = out[1], out[0]
    assert np.array_equal(h1, h0), (what, float(np.abs(h1.astype(np.float64) - h0).max()))
    for k in PINNED:
        assert c1[k] == c0[k], (what, k, c1[k], c0[k])
    # the pixel-owning build launches no k_resolve: one launch less per pass exactly where it applies
    assert c1["launches"] == c0["launches"] - (c0["passes"] if engaged else 0), (what, c1["launches"], c0["launches"])


@pytest.mark.parametrize("prec", ["f64", "f32"])
@pytest.mark.parametrize("name", sorted(SCENES))
def test_same_bits_over_spp(gpu, name, prec):
    s = SCENES[name]()
    ns, nm, nt = _counts(s)
    for spp in (1, 3, 64, 65):            # 65 slots in one pass: more than a wave's 64 lanes, the round-robin dealing + k_resolve in both
        _same(_both(gpu, s, gpu.make_params(W, H, spp, 8, ns, nm, nt, flags=_flags(gpu, name), seed=31), prec), spp <= 64 and _owning(name, prec), (name, spp, prec))


@pytest.mark.parametrize("prec", ["f64", "f32"])
def test_same_bits_multi_pass(gpu, prec):
    for name in ("s1", "glass"):
        s = SCENES[name]()
        ns, nm, nt = _counts(s)
        # 10 samples in passes of 3, 3, 3, 1 slots; 128 samples in two passes of 64 (the sums carry from pass to pass through the image)
        for spp, batch in ((10, 3 * W * H), (128, 64 * W * H)):
            p = gpu.make_params(W, H, spp, 6, ns, nm, nt, flags=_flags(gpu, name), seed=5, batch_rays=batch)
            out = _both(gpu, s, p, prec)
            assert out[1][1]["passes"] > 1
            _same(out, _owning(name, prec), (name, spp, prec))


@pytest.mark.parametrize("prec", ["f64", "f32"])
def test_same_bits_progressive(gpu, prec):
    s = scenes.scene_s1()
    ns, nm, nt = _counts(s)
    npdt = np.float32 if prec == "f32" else np.float64
    sums = {}
    for fused in (1, 0):
        acc = np.zeros((3, H, W), dtype=npdt)
        s0 = 0
        with _Env(SPIRA_FUSED_RESOLVE=fused):
            for n in (5, 64, 2):
                gpu.accumulate(*_args(s), gpu.make_params(W, H, n, 6, ns, nm, nt, seed=8), s0, acc, None, prec)
                s0 += n
        sums[fused] = acc
    assert np.array_equal(sums[1], sums[0])


@pytest.mark.parametrize("prec", ["f64", "f32"])
def test_same_bits_dealt_rows(gpu, prec):
    s = scenes.scene_s1()
    ns, nm, nt = _counts(s)
    for rank in range(3):                 # rows dealt round-robin in stripes of 4 over three ranks
        tp = D.tile_params(H, 3, rank, 4)
        _same(_both(gpu, s, gpu.make_params(W, H, 12, 8, ns, nm, nt, flags=gpu.POST_NONE, seed=9, **tp), prec), _owning("s1", prec), (rank, prec))


@pytest.mark.parametrize("prec", ["f64", "f32"])
def test_same_bits_every_wave_rendered_again(gpu, prec):
    """SPIRA_SPEC_DIV=2: the speculative launch reports every wave, so its waves must leave the image alone and the exact launch resolve them."""
    for name in ("s1", "glass"):
        s = SCENES[name]()
        ns, nm, nt = _counts(s)
        p = gpu.make_params(W, H, 16, 8, ns, nm, nt, flags=_flags(gpu, name), seed=12)
        out = _both(gpu, s, p, prec, SPIRA_SPEC_DIV=2)
        assert out[1][1]["redone_waves"] > 0
        _same(out, _owning(name, prec), (name, prec))
        with _Env(SPIRA_FUSED_RESOLVE=1):        # and the same bits as the default speculation
            hdr, _ = gpu.render(*_args(s), p, prec)
        assert np.array_equal(hdr, out[1][0]), name


def test_one_ray_per_lane_subchunks_keep_the_resolve_launch(gpu):
    s = scenes.scene_s1()
    ns, nm, nt = _counts(s)
    _same(_both(gpu, s, gpu.make_params(W, H, 24, 8, ns, nm, nt, flags=gpu.POST_NONE, seed=3), "f64", SPIRA_R=1), False, ("R=1", "f64"))


@pytest.mark.parametrize("prec", ["f64", "f32"])
def test_same_bits_full_size(gpu, prec):
    """The benchmark's shape: 1080p, 64 slots in one pass, 32 400 pixel-owning waves."""
    s = scenes.scene_s1()
    ns, nm, nt = _counts(s)
    _same(_both(gpu, s, gpu.make_params(1920, 1080, 64, 8, ns, nm, nt, flags=gpu.POST_NONE, seed=1), prec), _owning("s1", prec), ("1080p", prec))
