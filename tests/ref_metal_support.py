"""Shared by tests/test_ref_metal_cpu.py and tests/test_gpu_variants.py (not a test module): the inputs, the reference's own floors and the
assertions that hold SPIRA_SEM_METAL of the oracle, or of a kernel, to the reference's .metal kernel compiled for the CPU (oracle/_ref).
What is compared, the cap and the tolerances are explained in tests/test_ref_metal_cpu.py."""
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SEM_METAL, POST_NONE, ROWS_BOTTOM_UP = 0x2, 0x300, 0x1000
FLAGS = SEM_METAL | POST_NONE | ROWS_BOTTOM_UP

# The reference against itself, state-equal pixels, relative to |x| + 1e-3.  `python tests/ref_metal_support.py` reproduces them (it runs
# measure_floors() below over CASES, the 48 inputs of tests/test_ref_metal_cpu.py) and prints the input each figure comes from.
# f32: Float32 build against Float64 build.  f64: Float64 build against the Float64 build whose sin / cos undo the Float32 PI.
# Where they lie: f32 worst pixel = emitter scene, depth 24, spp 1, 33x47, pixel 611 (one path beside a branch: the 99th percentile is 270 times
# smaller, and that line is the one that binds); f32 99th percentile, f64 worst pixel (pixel 1942) and f64 99th percentile = S1, depth 8, spp 1, 96x54.
FLOOR_WORST = {"f32": 1.33e-3, "f64": 1.15e-5}      # worst pixel over all inputs
FLOOR_P99 = {"f32": 4.96e-6, "f64": 6.72e-8}        # largest per-input 99th percentile
HEADROOM = 4.0                                    # other seeds, other libm: tolerance = 4 x floor


def need_ref(oracle):
    """Skips when oracle/_ref holds no libraries, and says where build() looked for a reference checkout."""
    if not oracle.ref_metal_available():
        pytest.skip("oracle/_ref is not built: no reference checkout was found at build time (%s); "
                    "set REFERENCE=<checkout> and run __graft_entry__.build(), or make -C oracle _ref REFERENCE=<checkout>" % oracle.reference_search_record())


# ------------------------------------------------------------------------------------------------------------------------------- inputs
def scene_emitter(oracle):
    """An emitter, a partly-metallic rough sphere (0 < metallic < 1: both lobes of one material), a mirror, a rough metal, a diffuse ground."""
    materials8 = np.array([
        [0.6, 0.6, 0.5, 0, 0, 0, 0.0, 1.0],     # ground
        [1.0, 1.0, 1.0, 6, 5, 4, 0.0, 0.0],     # emitter
        [0.8, 0.6, 0.3, 0, 0, 0, 0.5, 0.4],     # partly metallic, rough
        [0.9, 0.9, 0.9, 0, 0, 0, 1.0, 0.0],     # mirror
        [0.7, 0.8, 0.9, 0, 0, 0, 1.0, 0.3],     # rough metal
    ])
    spheres5 = np.array([
        [0, -100.5, -1, 100, 1],
        [0, 0, -1, 0.5, 3],
        [1, 0, -1, 0.5, 4],
        [-1, 0, -1, 0.5, 5],
        [0, 2.2, -0.5, 0.6, 2],
    ], dtype=np.float64)
    cam = oracle.camera([0.0, 1.0, 3.0], [0.0, 0.0, -1.0], [0.0, 1.0, 0.0], 45.0, 16.0 / 9.0, 1.0, "f64")
    return dict(spheres5=spheres5, materials8=materials8, camera12=cam)


def scene_closed(oracle):
    """The camera inside one large diffuse sphere: no path ends in the sky, so roulette, the 0.01 throughput cut and max_depth end every path."""
    materials8 = np.array([
        [0.75, 0.75, 0.75, 0.05, 0.04, 0.03, 0.0, 1.0],  # the enclosing sphere, seen from inside; glows faintly, so every bounce on it shows in the radiance
        [1.0, 1.0, 1.0, 8, 8, 8, 0.0, 0.0],     # emitter
        [0.8, 0.5, 0.4, 0, 0, 0, 0.6, 0.25],    # partly metallic, rough
        [0.9, 0.9, 0.9, 0, 0, 0, 1.0, 0.0],     # mirror
    ])
    spheres5 = np.array([
        [0, 2, 0, 12, 1],
        [0, 4, 0, 1, 2],
        [-1.2, 0, 0, 0.8, 3],
        [1.2, 0, 0, 0.8, 4],
    ], dtype=np.float64)
    cam = oracle.camera([0.0, 1.0, 5.0], [0.0, 0.5, 0.0], [0.0, 1.0, 0.0], 50.0, 4.0 / 3.0, 1.0, "f64")
    return dict(spheres5=spheres5, materials8=materials8, camera12=cam)


def _spheres_only(s):
    return dict(spheres5=s["spheres5"], materials8=s["materials8"], camera12=s["camera12"])


SCENES = ("s1", "s2", "emitter", "closed")
DEPTHS = (1, 2, 4, 5, 8, 24)                     # 5: the first roulette draw (depth index 4 > 3)
SPPS = (1, 8)                                    # 8: the state runs from sample to sample
SIZES = ((96, 54), (61, 35), (33, 47), (75, 41))  # non-square, odd, portrait
CASES = [(sc, d, spp) for sc in SCENES for d in DEPTHS for spp in SPPS]


def scene(oracle, name):
    if name == "emitter":
        return scene_emitter(oracle)
    if name == "closed":
        return scene_closed(oracle)
    from spira_hip import scenes
    return _spheres_only(scenes.scene_s1() if name == "s1" else scenes.scene_s2())


def case(oracle, name, depth, spp):
    k = CASES.index((name, depth, spp))
    W, H = SIZES[k % len(SIZES)]
    return dict(scene(oracle, name), W=W, H=H, spp=spp, depth=depth, seed=1000 + k)


# --------------------------------------------------------------------------------------------------------------------------- comparisons
def rel_err(a, b):
    """Per pixel: the largest channel's |a - b| / (|b| + 1e-3); a, b [3, H, W] MEANS."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return (np.abs(a - b) / (np.abs(b) + 1e-3)).max(axis=0).reshape(-1)


def reference(oracle, c, build):
    sums, states = oracle.ref_metal(c["spheres5"], c["materials8"], c["camera12"], c["W"], c["H"], c["spp"], c["depth"], seed=c["seed"], build=build)
    return sums.astype(np.float64) / c["spp"], states


def reference_floor(oracle, c, prec):
    """The reference against itself: (number of pixels whose state differs, rel_err of the others).  f32: the Float32 build against the Float64
    one; f64: the Float64 build against the one whose sin / cos undo the Float32 PI."""
    a, sa = reference(oracle, c, "f32" if prec == "f32" else "f64pi")
    b, sb = reference(oracle, c, "f64")
    eq = sa == sb
    return int((~eq).sum()), rel_err(a, b)[eq]


def state_cap(oracle, c, prec):
    """How many pixels' states may differ from the reference's: none in Float64; in Float32 the reference's own Float32-against-Float64 count on
    this input plus one pixel, never above 1 % of the input."""
    if prec == "f64":
        return 0
    n, _ = reference_floor(oracle, c, "f32")
    return min(n + 1, (c["W"] * c["H"]) // 100)


def hold_to_reference(oracle, c, prec, mean, states, what):
    """The assertions shared with tests/test_gpu_variants.py: `mean` [3, H, W] (row = gid.y) and `states` [H * W] of the oracle or of a kernel
    against the reference build of the same precision."""
    ref_mean, ref_states = reference(oracle, c, prec)
    eq = np.asarray(states).reshape(-1) == ref_states
    n_diff, cap = int((~eq).sum()), state_cap(oracle, c, prec)
    r = rel_err(mean, ref_mean)[eq]
    worst, p99 = (float(r.max()), float(np.percentile(r, 99))) if r.size else (0.0, 0.0)
    print("%s %s %dx%d spp %d depth %d: states differ on %d pixels (cap %d); radiance worst %.3g, 99th percentile %.3g"
          % (what, prec, c["W"], c["H"], c["spp"], c["depth"], n_diff, cap, worst, p99))
    assert n_diff <= cap, (what, prec, n_diff, cap, np.flatnonzero(~eq)[:8])
    assert worst <= HEADROOM * FLOOR_WORST[prec], (what, prec, worst)          # floors measured: f32 1.33e-3, f64 1.15e-5
    assert p99 <= HEADROOM * FLOOR_P99[prec], (what, prec, p99)               # floors measured: f32 4.96e-6, f64 6.72e-8
    return n_diff


def oracle_render(oracle, c, prec):
    ns, nm = len(c["spheres5"]), len(c["materials8"])
    p = oracle.make_params(c["W"], c["H"], c["spp"], c["depth"], ns, nm, 0, flags=FLAGS, seed=c["seed"])
    hdr, _, _, states = oracle.render_variant(c["spheres5"], c["materials8"], c["camera12"], p, prec, want_states=True)
    return hdr, states


def lcg(st, n=1):
    for _ in range(n):
        st = (st * 1664525 + 1013904223) & 0xFFFFFFFF
    return st


def u24(st):
    return (st & 0x00FFFFFF) / float(0x01000000)


def measure_floors(oracle):
    """Prints what the module's docstring and FLOOR_* quote: the reference against itself on every input."""
    for prec in ("f32", "f64"):
        worst, p99, counts = (0.0, None), (0.0, None), []
        for name, depth, spp in CASES:
            c = case(oracle, name, depth, spp)
            n, r = reference_floor(oracle, c, prec)
            counts.append((n, round(100.0 * n / (c["W"] * c["H"]), 2)))
            where = (name, "depth", depth, "spp", spp, "%dx%d" % (c["W"], c["H"]))
            worst = max(worst, (float(r.max()), where + ("pixel", int(np.argmax(r)))), key=lambda t: t[0])
            p99 = max(p99, (float(np.percentile(r, 99)), where), key=lambda t: t[0])
        print(prec, "floor: worst %.3g at %s, largest 99th percentile %.3g at %s; state counts (pixels, %%) per input:" % (worst + p99), counts)


if __name__ == "__main__":
    import sys
    for p in (os.path.join(ROOT, "julia-spira_amd"), os.path.join(ROOT, "oracle")):
        sys.path.insert(0, p)
    import oracle_py
    measure_floors(oracle_py)
