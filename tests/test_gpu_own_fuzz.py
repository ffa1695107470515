"""GPU (MI355X): the pixel-owning passes on random sphere scenes and cameras (tests/own_fuzz_support.py: a seeded draw — 1 .. 40 spheres, sub-pixel ones,
one that contains the camera, a camera turned away, no sphere at all; any position, roll and field of view; frames 2 x 2 .. 96 x 60 at 1 .. 130 samples,
whole or as dealt rows — and a hand-made list of edges; tests/test_own_fuzz_cpu.py shows which states they reach).  Everything between the planner and
the accumulator that is a shortcut of geometry or bookkeeping — pixel-owning waves, wave-private radiance, all-sky run sums, the pixel table, the reach
masks, the camera's packets, k_path_own (csrc/spira_path_body.h, csrc/spira_sky.h, csrc/spira_plan.h) — is held, case by case in Float64, to
  (a) the CPU oracle: the suite's tolerance, segments exact;
  (b) the megakernel, which has none of the shortcuts: the same bits, the same segments;
  (c) the same library with the shortcuts switched off — SPIRA_FUSED_RESOLVE=0; sky runs, table, masks and packets off together; SPIRA_OWN_KERNEL=0; one
      knob of the case's own off alone — the same bits and the counters the files of each knob pin;
  (d) the host's classifier: spira_get_sky_pixels is, pass for pass, the pixels of the tile's complete runs of 4 that spira_sky_pixel_f64 calls sky;
  (e) the planner: spira_get_own_passes is what own_kernel_ok says of the call (the support module's rule), and 0 with SPIRA_OWN_KERNEL=0;
  (f) the other entries: a resident scene gives the arrays' bits; two progressive calls give sums within tolerance of the oracle, with its segments, the
      same bits with SPIRA_FUSED_RESOLVE=0, and (d) and (e) call by call.
Every fourth drawn case is rendered in Float32 too (nothing is pixel-owning there, but no other test renders a random sphere-only scene): (a) and (b).
Ahead of every compared render a frame of another size goes through the same staging, so that a stale buffer cannot pass for an answer."""
import numpy as np
import pytest

import own_fuzz_support as S
from test_gpu_own_kernel import COUNTERS as OWN_COUNTERS
from test_gpu_parity import _args, _close
from test_gpu_pixel_table import COUNTERS, PINNED
from test_gpu_private_radiance import PINNED as PRIVATE_PINNED
from test_gpu_specdiv import _Env

pytestmark = pytest.mark.gpu

CHUNK = 8
NO_SKY = tuple(k for k in COUNTERS if k != "sky_pixels")              # SPIRA_SKY_RUNS=0 sums no run ahead of the loop (tests/test_gpu_sky_runs.py)
ALL_OFF = dict(SPIRA_SKY_RUNS=0, SPIRA_PIXEL_TABLE=0, SPIRA_REACH_MASKS=0, SPIRA_CAM_CONSTS=0)
KNOB_COUNTERS = {"SPIRA_SKY_RUNS": NO_SKY, "SPIRA_PIXEL_TABLE": COUNTERS, "SPIRA_REACH_MASKS": COUNTERS, "SPIRA_CAM_CONSTS": COUNTERS, "SPIRA_PRIVATE_L": PRIVATE_PINNED}


def _params(mk, c, spp, flags=0):
    return mk.make_params(c["W"], c["H"], spp, c["depth"], len(c["spheres5"]), len(c["materials8"]), 0, flags=flags, seed=c["seed"], **c["tile"])


def _gpu_params(gpu, c, spp, flags=0):
    p = _params(gpu, c, spp, flags | gpu.POST_NONE)
    p.batch_rays = c["batch_rays"]
    return p


def _poison(gpu, c, prec):
    """A frame of another size and another seed through the staging the next call's outputs use."""
    other = dict(c, W=c["W"] + 3, H=c["H"] + 2, tile={}, seed=c["seed"] ^ 0x5A5A, depth=1, batch_rays=0)
    gpu.render(*_args(S.scene_of(c)), _gpu_params(gpu, other, 1), prec)


def _render(gpu, c, prec="f64", flags=0, **env):
    with _Env(**env):
        _poison(gpu, c, prec)
        hdr, _ = gpu.render(*_args(S.scene_of(c)), _gpu_params(gpu, c, c["spp"], flags), prec)
        return hdr, gpu.counters(), gpu.own_passes()


def _accumulate(gpu, c, sky, checked, **env):
    """The case's two progressive calls into one sum; with `checked`, (d) and (e) after each.  Returns (sums, segments of both calls)."""
    rows = len(S.tile_rows(c))
    sums = np.zeros((3, rows, c["W"]), dtype=np.float64)
    seg = 0
    with _Env(**env):
        for s0, n in S.calls(c):
            _poison(gpu, c, "f64")
            gpu.accumulate(*_args(S.scene_of(c)), _gpu_params(gpu, c, n), s0, sums, None, "f64")
            k = gpu.counters()
            seg += k["segments"]
            if checked:
                assert gpu.own_passes() == S.predicted_own_passes(c, n), (c["name"], "accumulate", s0, n, gpu.own_passes())
                assert k["sky_pixels"] == S.predicted_sky_pixels(c, sky, n), (c["name"], "accumulate", s0, n, k["sky_pixels"])
    return sums, seg


def _same(what, a, b, keys):
    (h, k, _), (h0, k0, _) = a, b
    assert np.array_equal(h, h0), (what, int((h != h0).sum()), float(np.abs(h - h0).max()))
    for key in keys:
        assert k[key] == k0[key], (what, key, k[key], k0[key])


def _check(gpu, oracle, it, c, f32=False):
    what = (it, c["name"], len(c["spheres5"]), c["W"], c["H"], c["spp"], c["depth"], c["batch_rays"], c["tile"], c["how"], c["split"], c["seed"])
    S.log_line(it, c)
    _, sky = S.reach_table(gpu, c)
    own, sky_pixels = S.predicted_own_passes(c), S.predicted_sky_pixels(c, sky)
    ohdr, _, oseg = oracle.render(*_args(S.scene_of(c)), _params(oracle, c, c["spp"]), "f64")

    new = _render(gpu, c)
    nbad, worst = _close(new[0], ohdr)                                                                     # (a)
    assert nbad == 0 and new[1]["segments"] == oseg, (what, "oracle", nbad, worst, new[1]["segments"], oseg)
    assert new[1]["sky_pixels"] == sky_pixels, (what, "sky_pixels", new[1]["sky_pixels"], sky_pixels)      # (d)
    assert new[2] == own, (what, "own_passes", new[2], own, S.pass_slots(c))                               # (e)
    _same((what, "mega"), new, _render(gpu, c, flags=gpu.KERNEL_MEGA), ("segments",))                      # (b)
    _same((what, "resolve"), new, _render(gpu, c, SPIRA_FUSED_RESOLVE=0), PINNED)                          # (c)
    _same((what, "all off"), new, _render(gpu, c, **ALL_OFF), NO_SKY)
    other = _render(gpu, c, SPIRA_OWN_KERNEL=0)
    _same((what, "k_path"), new, other, OWN_COUNTERS)
    assert other[2] == 0, (what, "own_passes with SPIRA_OWN_KERNEL=0", other[2])
    _same((what, c["knob"]), new, _render(gpu, c, **{c["knob"]: 0}), KNOB_COUNTERS[c["knob"]])

    if c["how"] == "handle":                                                                               # (f)
        with gpu.Scene(c["spheres5"], c["materials8"], None, "f64") as h:
            _poison(gpu, c, "f64")
            hdr, _ = h.render(c["camera12"], _gpu_params(gpu, c, c["spp"]))
            _same((what, "handle"), new, (hdr, gpu.counters(), None), COUNTERS)
            assert gpu.own_passes() == own, (what, "handle", gpu.own_passes(), own)
    elif c["how"] == "accumulate":
        sums, seg = _accumulate(gpu, c, sky, True)
        nbad, worst = _close(sums / np.float64(c["spp"]), ohdr)
        assert nbad == 0 and seg == oseg, (what, "accumulate", nbad, worst, seg, oseg)
        sums0, seg0 = _accumulate(gpu, c, sky, False, SPIRA_FUSED_RESOLVE=0)
        assert np.array_equal(sums, sums0) and seg == seg0, (what, "accumulate, resolve", float(np.abs(sums - sums0).max()), seg, seg0)

    if f32:
        S.log_line(it, c, "f32")
        ohdr, _, oseg = oracle.render(*_args(S.scene_of(c)), _params(oracle, c, c["spp"]), "f32")
        new = _render(gpu, c, "f32")
        nbad, worst = _close(new[0], ohdr)
        assert nbad == 0 and new[1]["segments"] == oseg, (what, "f32 oracle", nbad, worst, new[1]["segments"], oseg)
        assert new[2] == 0 and new[1]["sky_pixels"] == 0, (what, "f32 is never pixel-owning", new[2], new[1]["sky_pixels"])
        _same((what, "f32 mega"), new, _render(gpu, c, "f32", flags=gpu.KERNEL_MEGA), ("segments",))


@pytest.fixture(scope="module")
def drawn(gpu):
    return S.default_cases(gpu)


@pytest.mark.parametrize("chunk", range(-(-S.iters() // CHUNK)))
def test_drawn_cases(gpu, oracle, drawn, chunk):
    """SPIRA_FUZZ_OWN_SEED / SPIRA_FUZZ_OWN_ITERS: longer one-off campaigns (the defaults are what the suite runs, and what tests/test_own_fuzz_cpu.py counts)."""
    for it in range(chunk * CHUNK, min((chunk + 1) * CHUNK, len(drawn))):
        _check(gpu, oracle, it, drawn[it], f32=it % 4 == 0)


@pytest.mark.parametrize("case", S.FIXED, ids=[c["name"] for c in S.FIXED])
def test_fixed_cases(gpu, oracle, case):
    _check(gpu, oracle, "fixed", S.realise(case, gpu))
