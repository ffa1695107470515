"""CPU: the case list of tests/test_gpu_own_fuzz.py (tests/own_fuzz_support.py: the default seed's 64 drawn cases and FIXED) reaches the states it is
for.  From host arithmetic alone — the library's exports spira_pixel_reach_f64 / spira_sky_pixel_f64, the planner's rule restated in the support module
and the oracle — these count how many cases sit in each of the states where the pixel-owning stack (csrc/spira_path_body.h) can go wrong:
kinds, sample counts, entries, tiles, passes k_path_own renders and passes of 64 slots it must not, tiles whose runs are partly / never / all sky,
masks that are neither empty nor full, a sphere in bit 31 alone, a sphere beyond the mask alone, a camera inside a sphere, frames below one wave, rows
that are no multiple of a run, tiles that end inside a run, and paths that go on after their camera ray.  The numbers are conditions: where the draw
misses one, the draw changes."""
import numpy as np
import pytest

import own_fuzz_support as S
from spira_hip import scenes


@pytest.fixture(scope="module")
def cases(binding):
    """Every case with what the host says of it: masks and sky of the tile's pixels, its passes and the k_path_own count per call."""
    assert S.seed() == S.DEFAULT_SEED and S.iters() == S.DEFAULT_ITERS, "the conditions below are those of the default campaign: unset SPIRA_FUZZ_OWN_*"
    out = []
    for c in S.default_cases(binding) + [S.realise(c, binding) for c in S.FIXED]:
        masks, sky = S.reach_table(binding, c)
        c = dict(c, masks=masks, sky=sky, own=[S.predicted_own_passes(c, n) for _, n in S.calls(c)], slots=[S.pass_slots(c, n) for _, n in S.calls(c)])
        out.append(c)
    return out


def _count(cases, pred):
    return sum(1 for c in cases if pred(c))


def test_s1_is_s1():
    s = scenes.scene_s1()
    assert np.array_equal(S._f32(S.S1_SPHERES), s["spheres5"]) and np.array_equal(S._f32(S.S1_MATERIALS), s["materials8"])


def test_cases_are_float32_exact_and_within_the_shapes(cases):
    for c in cases:
        for k in ("spheres5", "materials8", "camera12"):
            assert np.array_equal(c[k], c[k].astype(np.float32).astype(np.float64)), (c["name"], k)
        assert 2 <= c["W"] <= 96 and 2 <= c["H"] <= 60 and c["spp"] in S.SPPS and c["W"] * c["H"] * c["spp"] <= S.MAX_PATHS, c["name"]
        assert c["how"] in S.HOWS and c["knob"] in S.KNOBS and 1 <= c["depth"] <= 255
        assert c["batch_rays"] in (0, 64 * c["W"] * c["H"], 3 * c["W"] * c["H"])
        assert sum(n for _, n in S.calls(c)) == c["spp"] and all(n >= 1 for _, n in S.calls(c))
        assert len(c["masks"]) == len(S.tile_rows(c)) * c["W"] > 0
    assert len({c["name"] for c in S.FIXED}) == len(S.FIXED)             # (the names are the GPU tests' ids)


def test_draw(cases):
    for kind in S.KINDS:
        assert _count(cases, lambda c: c["kind"] == kind) >= 3, kind
    for spp in S.SPPS:
        assert _count(cases, lambda c: c["spp"] == spp) >= 2, spp
    for how in S.HOWS:
        assert _count(cases, lambda c: c["how"] == how) >= 8, how
    assert _count(cases, lambda c: c["tile"]) >= 12
    share = {k: p for k, p in zip(S.KINDS, S.SHARES)}
    assert min(share.values()) >= 0.08 and abs(sum(share.values()) - 1) < 1e-12


def test_dispatch_states(cases):
    assert _count(cases, lambda c: sum(c["own"]) >= 1) >= 12
    # passes of 64 slots that are k_path's: 33 + spheres, depth 129, no sphere
    not_own = [c for c in cases if any(64 in s for s in c["slots"]) and sum(c["own"]) == 0]
    assert len(not_own) >= 6, len(not_own)
    assert any(len(c["spheres5"]) > 32 for c in not_own) and any(c["depth"] > 128 for c in not_own) and any(len(c["spheres5"]) == 0 for c in not_own)
    # the table of tests/test_gpu_own_kernel.py at batch_rays = 64 W H
    by_name = {c["name"]: c for c in cases}
    for label in ("s1", "sides32"):
        got = [(by_name["%s_spp%d" % (label, spp)]["slots"], sum(by_name["%s_spp%d" % (label, spp)]["own"])) for spp in (64, 127, 128, 130)]
        if label == "sides32":
            assert got == [([[64]], 1), ([[64, 63]], 1), ([[64, 64]], 2), ([[44, 44, 42]], 0)], got
        else:           # (127 and 128 as two calls of 64 + 63 and 64 + 64 samples)
            assert got == [([[64]], 1), ([[64], [63]], 1), ([[64], [64]], 2), ([[44, 44, 42]], 0)], got
    assert sum(by_name["sides33_spp64"]["own"]) == 0 and by_name["sides33_spp64"]["slots"] == [[64]]


def test_sky_run_states(cases):
    some = none = every = 0
    for c in cases:
        runs = S.sky_runs(c["sky"])
        if len(runs) == 0:
            continue
        some += 0 < runs.sum() < len(runs)
        none += runs.sum() == 0
        every += runs.sum() == len(runs)
    assert some >= 20 and none >= 3 and every >= 3, (some, none, every)


def test_mask_states(cases):
    def full(c):
        return np.uint32((1 << min(len(c["spheres5"]), 32)) - 1)
    mixed = _count(cases, lambda c: len(c["spheres5"]) and np.mean((c["masks"] != 0) & (c["masks"] != full(c))) >= 0.05)
    assert mixed >= 15, mixed
    assert _count(cases, lambda c: (c["masks"] == np.uint32(1 << 31)).any()) >= 2
    assert _count(cases, lambda c: len(c["spheres5"]) > 32 and ((c["masks"] == 0) & ~c["sky"]).any()) >= 2
    inside = 0
    for c in cases:
        for s in range(min(len(c["spheres5"]), 32)):
            d = np.linalg.norm(c["spheres5"][s, 0:3] - c["camera12"][0:3])
            if d < c["spheres5"][s, 3]:
                assert ((c["masks"] >> np.uint32(s)) & 1).all(), (c["name"], s)        # a camera inside a sphere: every mask has its bit
                inside += 1
                break
    assert inside >= 2, inside
    # what pixel_reach says of a radius that is not positive: "may hit"
    c = next(c for c in cases if c["name"] == "radius_zero_and_negative")
    assert ((c["masks"] >> np.uint32(5)) & 1).all() and ((c["masks"] >> np.uint32(6)) & 1).all()
    # sky_pixel is pixel_reach == 0 where the mask has a bit for every sphere
    for c in cases:
        if len(c["spheres5"]) <= 32:
            assert np.array_equal(c["sky"], c["masks"] == 0), c["name"]


def test_sizes(cases):
    assert _count(cases, lambda c: len(c["masks"]) < 64) >= 2
    assert _count(cases, lambda c: c["W"] % 4 != 0) >= 10
    assert _count(cases, lambda c: len(c["masks"]) % S.RUN != 0) >= 5


def test_paths_go_on(cases, oracle):
    """The oracle's segments exceed W H spp — some path went on after its camera ray — in at least 75 % of the cases that have a sphere."""
    on = total = 0
    for c in cases:
        ns = len(c["spheres5"])
        if ns == 0:
            continue
        rows = len(S.tile_rows(c))
        p = oracle.make_params(c["W"], c["H"], c["spp"], c["depth"], ns, len(c["materials8"]), 0, seed=c["seed"], **c["tile"])
        _, _, seg = oracle.render(c["spheres5"], c["materials8"], None, c["camera12"], p, "f64")
        assert seg >= rows * c["W"] * c["spp"]
        on += seg > rows * c["W"] * c["spp"]
        total += 1
    assert on >= 0.75 * total, (on, total)


def test_frames_of_one_column_or_row_are_refused(binding):
    """W = 1 and H = 1 never reach a kernel (u = (i - 1 + rand) / (W - 1)): SPIRA_E_INVALID from the validation, ahead of any device call."""
    c = S.realise(S.FIXED[0], binding)
    for W, H in ((1, 8), (8, 1)):
        with pytest.raises(binding.SpiraError) as e:
            binding.render(c["spheres5"], c["materials8"], None, c["camera12"], binding.make_params(W, H, 64, 4, len(c["spheres5"]), len(c["materials8"])), "f64")
        assert "error -1" in str(e.value) and "width and height must be >= 2" in str(e.value)
