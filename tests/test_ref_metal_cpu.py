"""CPU: SPIRA_SEM_METAL of the oracle against the reference's own kernel, compiled for the CPU.

`oracle/_ref/` (make -C oracle _ref; oracle/Makefile, oracle/ref_metal/) holds src/spira_path_trace_kernel.metal of the reference un-escaped and
compiled as it stands with the ROCm clang++, in Float32 (`f32`), with `float` read as `double` (`f64`), and as `f64` with sin / cos undoing the
Float32 rounding of the file's PI literal (`f64pi`).  The arithmetic of the stand-in header is the oracle's convention (IEEE, written order, libm
sin / cos): what is pinned is control flow, RNG draw order, constants and statement order, not Apple's rounding.  The libraries exist only where
a reference checkout was present at build time; without them this module skips (and test_ref_libraries_built_where_the_checkout_is fails when the
checkout is there and the libraries are not).

Per pixel, oracle against reference, both seeded with metal_state0 and rendered bottom-up (oracle row = gid.y):
  * the LCG state after the pixel's last sample: equal state = equal number of draws = the same way through lobe choice, rejection loop,
    roulette and cut-off.  Float64: every pixel of every input.  Float32: all but `cap` pixels, cap = (pixels whose state differs between the
    Float32 and the Float64 REFERENCE builds) + 1, at most 1 % of the input: the reference's own sensitivity to rounding, measured per input at
    test time, not a setting.
  * radiance of the state-equal pixels, relative to |x| + 1e-3, against 4 x the reference's own floor (below).

The oracle departs from the file in Float64 in one known way: the file's PI is a Float32 literal (`2.0f * PI * r1` is off by
2.8e-8 relative), the oracle's sincos_turn takes exact quarter turns.  (Two more literals, 0.7f of the sky and 0.1f of the tangent-frame switch,
are read as Float64 0.7 and 0.1 by oracle and kernels: 1.7e-8 on the sky's green channel, and a switch window 1.5e-9 wide that no test can hit.)
The Float64 floor therefore is the reference against itself across exactly that PI difference: `f64` against `f64pi`.

Measured (this module's 48 inputs; ROCm clang++ 22, glibc libm):
  states, reference f64 against f64pi: 0 differing pixels on every input (required by test_reference_f64_states_do_not_depend_on_the_pi_literal)
  states, reference f32 against f64:   0 differing pixels on 46 inputs, 1 on two (0.02 %, 0.03 %): the Float32 cap is 1 or 2 pixels
  states, oracle against reference:    f64 0 on every input; f32 0 on 47 inputs, 1 on one
  radiance, reference against itself:  f32 worst pixel 1.33e-3, largest per-input 99th percentile 4.96e-6; f64 1.15e-5 and 6.72e-8
  radiance, oracle against reference:  f32 worst pixel 1.4e-3, 99th percentile 1.98e-7 (most pixels bit-equal); f64 1.15e-5 and 6.72e-8 (the PI
                                       departure and nothing else: the same figures as the reference across it)
"""
import os

import numpy as np
import pytest

from ref_metal_support import (FLAGS, CASES, ROOT, case, hold_to_reference, lcg, need_ref, oracle_render, reference, reference_floor, u24)


# ---------------------------------------------------------------------------------------------------------------------------------- tests
def _scene_needs(request, name):
    """S1 and S2 come from spira_hip.scenes, whose builders take their camera from the product library's host-side spira_camera_lookat_*: only
    these cases need the library built (no GPU); the emitter and closed scenes, and every one-pixel scene, need the oracle alone."""
    if name in ("s1", "s2"):
        request.getfixturevalue("binding")


def test_ref_libraries_built_where_the_checkout_is(oracle):
    """A reference checkout that can be found and no oracle/_ref: the recipe is broken, not skipped.  The search here is this test's own and wider
    than build()'s record (oracle/_ref/SEARCHED.txt) so that the two do not share a blind spot: REFERENCE, every directory named `reference` beside
    the repository or beside one of its parent directories, one in the home directory, and every place build() says it looked."""
    home = os.path.expanduser("~")
    places = [os.environ.get("REFERENCE"), os.path.join(home, "reference"), "/root/reference"]
    d = ROOT
    while os.path.dirname(d) != d:
        d = os.path.dirname(d)
        places.append(os.path.join(d, "reference"))
    places += oracle.reference_candidates()
    record = oracle.reference_search_record()
    found = [p for p in places if p and os.path.exists(os.path.join(p, "src", "spira_path_trace_kernel.metal"))]
    if found:
        assert oracle.ref_metal_available(), "reference checkout at %s, but oracle/_ref holds no libraries (build() %s)" % (found[0], record)


@pytest.mark.parametrize("build", ["f32", "f64", "f64pi"])
def test_argument_evaluation_order_guard(oracle, build):
    """The file's random_unit_vector draws three uniforms inside ONE constructor's argument list; C++ leaves their order open.  Metal's compiler
    (clang) goes left to right: x, y, z = draws 1, 2, 3.  A recipe that compiles with gcc (right to left) fails here."""
    need_ref(oracle)
    tried = 0
    for state in range(1, 400):
        s1 = lcg(state); s2 = lcg(s1); s3 = lcg(s2)
        p = np.array([u24(s1), u24(s2), u24(s3)]) * 2.0 - 1.0
        if not (p @ p < 0.98) or abs(abs(p[0]) - abs(p[2])) < 0.05:       # first triple accepted, clearly; x and z tell each other apart
            continue
        xyz, after = oracle.ref_metal_unit_vector(state, build)
        assert after == s3, (state, after, s3)
        assert np.allclose(xyz, p / np.sqrt(p @ p), rtol=0, atol=1e-6 if build == "f32" else 1e-14), (state, xyz, p / np.sqrt(p @ p))
        tried += 1
    assert tried > 100


def test_metal_state0_twin(oracle):
    """oracle_py.metal_state0 (numpy) == the oracle's: with max_depth 0 no draw but the two of the jitter happens."""
    sp, ma = np.array([[0, 0, -1, 0.5, 1.0]]), np.array([[0.5, 0.5, 0.5, 0, 0, 0, 0, 1.0]])
    cam = oracle.camera([0.0, 0.0, 3.0], [0.0, 0.0, 0.0], [0.0, 1.0, 0.0], 45.0, 1.5, 1.0, "f64")
    for seed in (0, 1, 77, 2 ** 40 + 12345, 2 ** 64 - 1):
        p = oracle.make_params(9, 6, 1, 0, 1, 1, 0, flags=FLAGS, seed=seed)
        _, _, _, st = oracle.render_variant(sp, ma, cam, p, "f32", want_states=True)
        want = [lcg(int(s), 2) for s in oracle.metal_state0(seed, np.arange(54))]
        assert np.array_equal(st, np.array(want, dtype=np.uint32)), seed


@pytest.mark.parametrize("name,depth,spp", CASES)
def test_reference_f64_states_do_not_depend_on_the_pi_literal(oracle, request, name, depth, spp):
    """The inputs (seeds, sizes) are ones on which no pixel's control flow is decided within the 2.8e-8 of the file's Float32 PI: only then is
    'zero differing states in Float64' a fair demand on the oracle, whose sincos_turn takes exact quarter turns."""
    need_ref(oracle)
    _scene_needs(request, name)
    n, _ = reference_floor(oracle, case(oracle, name, depth, spp), "f64")
    assert n == 0


@pytest.mark.parametrize("prec", ["f32", "f64"])
@pytest.mark.parametrize("name,depth,spp", CASES)
def test_oracle_metal_equals_reference(oracle, request, name, depth, spp, prec):
    need_ref(oracle)
    _scene_needs(request, name)
    c = case(oracle, name, depth, spp)
    hdr, states = oracle_render(oracle, c, prec)
    hold_to_reference(oracle, c, prec, hdr, states, "oracle %s" % name)


# ---- the file's constants, one at a time, through one-pixel scenes: the camera's horizontal and vertical are zero, so every camera ray is
# (0, 0, 0) -> (0, 0, -1) whatever the jitter draws
def _one_pixel(spheres5, materials8, spp, depth, seed=5):
    cam = np.array([0, 0, 0, 0, 0, -1, 0, 0, 0, 0, 0, 0], dtype=np.float64)
    return dict(spheres5=np.array(spheres5, dtype=np.float64), materials8=np.array(materials8, dtype=np.float64), camera12=cam,
                W=1, H=1, spp=spp, depth=depth, seed=seed)


def _both(oracle, c, prec, what):
    """Oracle and reference on a one-pixel scene: (oracle sum [3], oracle state, reference sum, reference state), held to each other first."""
    hdr, states = oracle_render(oracle, c, prec)
    assert hold_to_reference(oracle, c, prec, hdr, states, what) == 0
    ref_mean, ref_states = reference(oracle, c, prec)
    return hdr.reshape(3).astype(np.float64) * c["spp"], int(states[0]), ref_mean.reshape(3) * c["spp"], int(ref_states[0])


MIRROR = [0.8, 0.8, 0.8, 0, 0, 0, 1.0, 0.0]
SKY_AT_HORIZON = 0.5 * np.array([1.0, 1.0, 1.0]) + 0.5 * np.array([0.5, 0.7, 1.0])


@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_constant_epsilon(oracle, prec):
    """A mirror sphere whose near root is t0.  t0 > EPSILON = 1e-4: hit from outside, reflected straight back into the sky: 2 + 1 draws a sample.
    t0 < EPSILON: the near root is refused, the far root hits from inside and the path bounces between the poles: 2 + max_depth draws (depth 3:
    no roulette yet).  Then a sweep through the edge itself, where oracle and reference (the same IEEE operations) must still decide alike."""
    need_ref(oracle)
    s0 = int(oracle.metal_state0(5, [0])[0])
    for t0, draws in ((1.02e-4, 3), (0.98e-4, 5), (5e-4, 3), (2e-5, 5)):
        c = _one_pixel([[0, 0, -(0.5 + t0), 0.5, 1]], [MIRROR], 4, 3)
        osum, ost, rsum, rst = _both(oracle, c, prec, "epsilon t0=%g" % t0)
        assert ost == rst == lcg(s0, 4 * draws), (t0, draws)
        if draws == 3:
            assert np.allclose(rsum, 4 * 0.8 * SKY_AT_HORIZON, rtol=1e-6) and np.allclose(osum, 4 * 0.8 * SKY_AT_HORIZON, rtol=1e-6)
    seen = set()
    for t0 in np.linspace(0.999e-4, 1.001e-4, 41):
        c = _one_pixel([[0, 0, -(0.5 + t0), 0.5, 1]], [MIRROR], 2, 3)
        _, ost, _, rst = _both(oracle, c, prec, "epsilon sweep")
        assert ost in (lcg(s0, 6), lcg(s0, 10))
        seen.add(ost)
    assert len(seen) == 2          # the sweep crosses the edge


@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_constants_inside_tie_cutoff_and_lobe_draw(oracle, prec):
    need_ref(oracle)
    s0 = int(oracle.metal_state0(5, [0])[0])
    dim_light = [0.005, 0.005, 0.005, 2, 3, 4, 0.0, 1.0]
    # a ray that starts at the centre of a sphere takes the SECOND root; albedo 0.005 < 0.01 ends the path after its first bounce; metallic = 0
    # still draws the lobe choice: 2 (jitter) + 1 (lobe) + 2 (hemisphere) draws a sample, radiance = the emission
    c = _one_pixel([[0, 0, 0, 1.0, 1]], [dim_light], 8, 8)
    osum, ost, rsum, rst = _both(oracle, c, prec, "inside")
    assert ost == rst == lcg(s0, 8 * 5)
    assert np.array_equal(rsum, [16, 24, 32]) and np.array_equal(osum, [16, 24, 32])
    # metallic = 1: the draw is made as well, and with roughness 0 no rejection draws follow: 2 + 1
    c = _one_pixel([[0, 0, -2, 0.5, 1]], [[0.005, 0.005, 0.005, 2, 3, 4, 1.0, 0.0]], 8, 8)
    osum, ost, rsum, rst = _both(oracle, c, prec, "mirror")
    assert ost == rst == lcg(s0, 8 * 3) and np.array_equal(rsum, [16, 24, 32]) and np.array_equal(osum, [16, 24, 32])
    # two coincident spheres: `t < closest_t` is strict, the EARLIER one keeps the tie
    red, green = [0.005, 0.005, 0.005, 1, 0, 0, 0.0, 1.0], [0.005, 0.005, 0.005, 0, 1, 0, 0.0, 1.0]
    c = _one_pixel([[0, 0, -2, 0.5, 1], [0, 0, -2, 0.5, 2]], [red, green], 8, 8)
    osum, ost, rsum, rst = _both(oracle, c, prec, "tie")
    assert np.array_equal(rsum, [8, 0, 0]) and np.array_equal(osum, [8, 0, 0]) and ost == rst == lcg(s0, 8 * 5)
    # a rough metal and a half-metallic rough material: rejection loop and lobe choice, no closed form: oracle == reference, state for state
    for mat in ([0.9, 0.9, 0.9, 0, 0, 0, 1.0, 0.7], [0.9, 0.9, 0.9, 0, 0, 0, 0.5, 0.7]):
        for seed in range(20):
            c = _one_pixel([[0, 0, -2, 0.5, 1], [0, 0, 0, 30.0, 2]], [mat, [0.9, 0.9, 0.9, 0.1, 0.1, 0.1, 0.0, 1.0]], 8, 24, seed=seed)
            _both(oracle, c, prec, "rough")


@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_constant_roulette_compares_strictly(oracle, prec):
    """`random_uniform > p_continue` ends a path: a draw EQUAL to p_continue lets it live.  The camera sits in the middle of a mirror shell of
    albedo 0.5, so the path runs from pole to pole, one lobe draw a bounce, and at depth index 4 p_continue = 0.5^5 = 2^-5 exactly.  The two seeds
    are ones (found by search: one in 2^24) whose 8th draw, the first roulette draw, is exactly 2^-5.  Strict: the path lives, throughput becomes
    1, bounce 5 draws twice more and max_depth 6 ends it: 10 draws.  `>=` would stop at 8."""
    need_ref(oracle)
    for seed in (346115, 49098030):
        s0 = int(oracle.metal_state0(seed, [0])[0])
        assert u24(lcg(s0, 8)) == 2.0 ** -5
        c = _one_pixel([[0, 0, 0, 1.0, 1]], [[0.5, 0.5, 0.5, 1, 1, 1, 1.0, 0.0]], 1, 6, seed=seed)
        osum, ost, rsum, rst = _both(oracle, c, prec, "roulette tie")
        assert ost == rst == lcg(s0, 10)
        # emission 1 at every bounce: 1 + 1/2 + 1/4 + 1/8 + 1/16 (bounces 0-4), then throughput 1 at bounce 5
        assert np.array_equal(rsum, [2.9375] * 3) and np.array_equal(osum, [2.9375] * 3)
