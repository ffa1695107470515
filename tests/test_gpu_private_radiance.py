"""GPU (MI355X): wave-private radiance blocks (csrc/spira_device.h, PathArgs::l_private) — in a pixel-owning pass of a Float64
sphere scene wave w keeps the radiance of its path e at L[w * 64 k_eff + e] instead of the slot-major L[slot * tile_pixels + pixel], and the queue
word carries e instead of the path index (the RNG key is carried beside it: max_depth <= 128; deeper renders keep the slot-major layout).
Only where the bytes live changes: with SPIRA_FUSED_RESOLVE=0 (round-robin dealing + k_resolve on the slot-major layout) the images are the same
bits and the counters the same numbers (but rays_enqueued, which follows the dealing), and with SPIRA_PRIVATE_L=0 (pixel-owning passes on the
slot-major layout: the same dealing) every counter is the same number."""
import numpy as np
import pytest

from spira_hip import distributed as D
from spira_hip import scenes
from test_gpu_parity import ATOL, RTOL, _args, _close, _counts
from test_gpu_specdiv import _Env

pytestmark = pytest.mark.gpu

PINNED = ("samples", "segments", "radiance_rmw", "radiance_stores", "passes", "bounce_launches")
W, H = 97, 55                 # 5 335 pixels: 21 workgroups of 256 pixels, the last wave's block lies past n_first = k_eff * tile_pixels
SMALL = (9, 5)                # 45 pixels: less than one wave's 64


def _three(gpu, s, params, **env):
    """default (wave-private blocks) / pixel-owning on the slot-major layout / round-robin dealing + k_resolve"""
    out = {}
    for name, kv in (("private", {}), ("slot_major", dict(SPIRA_PRIVATE_L=0)), ("resolve", dict(SPIRA_FUSED_RESOLVE=0))):
        with _Env(**dict(env, **kv)):
            hdr, _ = gpu.render(*_args(s), params, "f64")
            out[name] = (hdr, gpu.counters())
    return out


def _same(out, what, owning=True):
    h, c = out["private"]
    for other in ("slot_major", "resolve"):
        h0, c0 = out[other]
        assert np.array_equal(h, h0), (what, other, float(np.abs(h - h0).max()))
        for k in PINNED:
            assert c[k] == c0[k], (what, other, k, c[k], c0[k])
    c0 = out["slot_major"][1]
    assert c["rays_enqueued"] == c0["rays_enqueued"] and c["launches"] == c0["launches"], (what, c, c0)      # the same dealing: the same queue traffic
    # a pixel-owning pass launches no k_resolve
    cr = out["resolve"][1]
    assert c["launches"] == cr["launches"] - (cr["passes"] if owning else 0), (what, c["launches"], cr["launches"])


@pytest.mark.parametrize("size", [(W, H), SMALL], ids=["97x55", "9x5"])
@pytest.mark.parametrize("spp,passes", [(1, 1), (3, 1), (64, 1), (65, 2), (130, 3)])
def test_same_bits_over_spp_and_tiles(gpu, size, spp, passes):
    """One slot, partial slots, a full wave of slots, two passes (33 + 32 slots) and three (44 + 43 + 43): the sums carry through the image."""
    w, h = size
    s = scenes.scene_s1()
    ns, nm, nt = _counts(s)
    out = _three(gpu, s, gpu.make_params(w, h, spp, 8, ns, nm, nt, flags=gpu.POST_NONE, seed=31, batch_rays=64 * w * h))
    assert out["private"][1]["passes"] == passes
    _same(out, (size, spp))


@pytest.mark.parametrize("depth", [1, 8, 128, 129])
def test_same_bits_both_sides_of_the_carried_key(gpu, depth):
    """max_depth <= 128: the RNG key rides in the queue and the queue word addresses the wave's block; 129: the key is derived from the path index,
    so the word stays the path index and L slot-major.  (Depth 1: no queue at all.)"""
    s = scenes.scene_s1()
    ns, nm, nt = _counts(s)
    _same(_three(gpu, s, gpu.make_params(W, H, 6, depth, ns, nm, nt, flags=gpu.POST_NONE, seed=17)), depth)


def test_same_bits_deep_paths(gpu):
    """More samples at the deepest render that still carries its key: the long paths' terms (stores and read-modify-writes) all land in the wave's block."""
    s = scenes.scene_s1()
    ns, nm, nt = _counts(s)
    out = _three(gpu, s, gpu.make_params(W, H, 20, 128, ns, nm, nt, flags=gpu.POST_NONE, seed=23))
    _same(out, "deep")


def test_same_bits_progressive(gpu):
    s = scenes.scene_s1()
    ns, nm, nt = _counts(s)
    sums = {}
    for name, kv in (("private", {}), ("slot_major", dict(SPIRA_PRIVATE_L=0)), ("resolve", dict(SPIRA_FUSED_RESOLVE=0))):
        acc = np.zeros((3, H, W), dtype=np.float64)
        s0 = 0
        with _Env(**kv):
            for n in (5, 64):             # two calls: the second starts from the first's sums
                gpu.accumulate(*_args(s), gpu.make_params(W, H, n, 6, ns, nm, nt, seed=8), s0, acc, None, "f64")
                s0 += n
        sums[name] = acc
    assert np.array_equal(sums["private"], sums["resolve"]) and np.array_equal(sums["private"], sums["slot_major"])


def test_same_bits_dealt_rows(gpu):
    s = scenes.scene_s1()
    ns, nm, nt = _counts(s)
    for rank in range(3):                 # rows dealt round-robin in stripes of 4 over three ranks
        tp = D.tile_params(H, 3, rank, 4)
        _same(_three(gpu, s, gpu.make_params(W, H, 12, 8, ns, nm, nt, flags=gpu.POST_NONE, seed=9, **tp)), ("rank", rank))


@pytest.mark.parametrize("spec", [2, 0])
def test_same_bits_speculative_division(gpu, spec):
    """SPIRA_SPEC_DIV=2: every wave is rendered again by the exact launch, on the same grid — it finds (and overwrites) the same block; 0: one exact launch."""
    s = scenes.scene_s1()
    ns, nm, nt = _counts(s)
    p = gpu.make_params(W, H, 16, 8, ns, nm, nt, flags=gpu.POST_NONE, seed=12)
    out = _three(gpu, s, p, SPIRA_SPEC_DIV=spec)
    assert (out["private"][1]["redone_waves"] > 0) == (spec == 2)
    _same(out, ("spec", spec))
    hdr, _ = gpu.render(*_args(s), p, "f64")        # and the same bits as the default speculation
    assert np.array_equal(hdr, out["private"][0])


def test_against_the_oracle(gpu, oracle):
    s = scenes.scene_s1()
    ns, nm, nt = _counts(s)
    hdr, _ = gpu.render(*_args(s), gpu.make_params(W, H, 16, 8, ns, nm, nt, flags=gpu.POST_NONE, seed=scenes.seed_for(3)), "f64")
    c = gpu.counters()
    ohdr, _, oseg = oracle.render(*_args(s), oracle.make_params(W, H, 16, 8, ns, nm, nt, seed=scenes.seed_for(3)), "f64")
    nbad, worst = _close(hdr, ohdr, RTOL, ATOL)
    assert nbad == 0, "%d pixel-channels off, worst rel %.3g" % (nbad, worst)
    assert c["samples"] == W * H * 16 and c["segments"] == oseg


def test_full_size(gpu):
    """The benchmark's shape: 1080p, 64 slots in one pass, 32 400 waves with a 96 KB block each."""
    s = scenes.scene_s1()
    ns, nm, nt = _counts(s)
    _same(_three(gpu, s, gpu.make_params(1920, 1080, 64, 8, ns, nm, nt, flags=gpu.POST_NONE, seed=1)), "1080p")
