"""GPU (MI355X): the wave-cooperative drain of the random-vector list (csrc/spira_device.h, drain_unit_sphere_list; DESIGN.md §4, docs/experiments.md §21).

Phase 2 of a k_path / k_bounce trip turns the RNG keys on the wave's LDS list into random_in_unit_sphere() of each key: lanes try one entry each
while unclaimed entries remain, then groups of lanes evaluate several tries of each pending entry at once (the lowest accepted try wins); Float64
accepts by an exact integer test and keeps the draw's two hash words.  The vector is a pure function of the key, so none of this may change a bit.
Here: (1) the routine alone, one wave per list, against a plain per-lane loop — list lengths around every threshold, both precisions, the try bound
at 64 and at small values where entries run out of tries (tests/native/rnd_list.hip, built with hipcc at test time); (2) the shapes that reach the
tail inside real launches — lists of a few entries, full lists trip after trip in a closed scene, the short sub-chunks of a 65-sample render — against the
megakernel (one lane per path, serial draws) bit for bit and the oracle's segment count."""
import os
import subprocess

import numpy as np
import pytest

from spira_hip import scenes
from test_gpu_parity import _args, _counts

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

LINES = 12        # 2 precisions x the try bounds 64, 1, 2, 3, 5, 7


def test_every_entry_is_random_in_unit_sphere_of_its_key(tmp_path):
    exe = str(tmp_path / "rnd_list")
    subprocess.run(["/opt/rocm/bin/hipcc", "-O3", "-std=c++17", "-ffp-contract=off", "--offload-arch=gfx950", "-I" + os.path.join(ROOT, "include"),
                    "-o", exe, os.path.join(ROOT, "tests", "native", "rnd_list.hip")], check=True, timeout=600)
    out = subprocess.run([exe, "64", "20261017"], capture_output=True, text=True, timeout=120)
    print(out.stdout)
    assert out.returncode == 0, out.stdout + out.stderr
    lines = [l for l in out.stdout.strip().splitlines() if "MAXT" in l]
    assert len(lines) == LINES and out.stdout.strip().endswith("ok")
    for line in lines:
        assert " 0 mismatching" in line and " 0 slots behind a list touched" in line, line
        f = line.replace(",", "").split()
        bound, exhausted, accepted, last = int(f[2].rstrip(":")), int(f[f.index("exhausted") - 1]), int(f[f.index("accepted") - 1]), int(f[f.index("on") - 1])
        assert accepted > 0, line
        if bound < 64:                   # both outcomes, and an accept on the last allowed try (MAXT = 2: 23 % of the entries run out)
            assert exhausted > 0 and last > 0, line


# scene, width, height, spp, depth, extra parameters, passes
SHAPES = {
    "tile45_spp1": (scenes.scene_s1, 9, 5, 1, 8, {}, 1),             # 45 paths: lists of a few entries, the tail from the first iteration
    "tile45_spp3": (scenes.scene_s1, 9, 5, 3, 8, {}, 1),
    "closed_box": (scenes.scene_s3, 61, 35, 2, 24, {}, 1),           # every ray hits again: full lists, dense continuation trip after trip
    # 65 samples: one more than a pixel-owning pass takes.  As planned by default (one pass of 65 slots, paths dealt round-robin, k_resolve) and with
    # passes capped at 64 slots (the planner evens them out: 33 + 32, both pixel-owning) — late rounds of either leave short sub-chunks
    "spp65_one_pass": (scenes.scene_s1, 96, 54, 65, 8, {}, 1),
    "spp65_two_passes": (scenes.scene_s1, 96, 54, 65, 8, dict(batch_rays=64 * 96 * 54), 2),
}
_memo = {}


def _reference(gpu, oracle, shape, prec):
    """the megakernel's image and the oracle's segment count: made once per (shape, precision)"""
    if (shape, prec) not in _memo:
        make, W, H, spp, depth, extra, _ = SHAPES[shape]
        s = make()
        ns, nm, nt = _counts(s)
        hdr, _ = gpu.render(*_args(s), gpu.make_params(W, H, spp, depth, ns, nm, nt, flags=gpu.KERNEL_MEGA | gpu.POST_NONE, seed=21, **extra), prec)
        mseg = gpu.counters()["segments"]
        _, _, oseg = oracle.render(*_args(s), oracle.make_params(W, H, spp, depth, ns, nm, nt, seed=21), prec)
        hdr.setflags(write=False)
        _memo[(shape, prec)] = (hdr, mseg, oseg)
    return _memo[(shape, prec)]


@pytest.mark.parametrize("org", ["wavefront", "bounce"])
@pytest.mark.parametrize("prec", ["f64", "f32"])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_tail_shapes_in_real_launches(gpu, oracle, shape, prec, org):
    make, W, H, spp, depth, extra, passes = SHAPES[shape]
    m_hdr, mseg, oseg = _reference(gpu, oracle, shape, prec)
    s = make()
    ns, nm, nt = _counts(s)
    kernel = gpu.KERNEL_WAVEFRONT if org == "wavefront" else gpu.KERNEL_BOUNCE
    hdr, _ = gpu.render(*_args(s), gpu.make_params(W, H, spp, depth, ns, nm, nt, flags=kernel | gpu.POST_NONE, seed=21, **extra), prec)
    c = gpu.counters()
    print("%s %s %s: %d segments (oracle %d, megakernel %d), %d passes" % (shape, prec, org, c["segments"], oseg, mseg, c["passes"]))
    assert c["passes"] == passes
    assert c["segments"] == oseg == mseg, (shape, prec, org, c["segments"], oseg, mseg)
    assert np.array_equal(hdr, m_hdr), (shape, prec, org, float(np.abs(hdr.astype(np.float64) - m_hdr).max()))
