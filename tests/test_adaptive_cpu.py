"""CPU: adaptive sampling (spira_render_adaptive_*) without a device — the library exports the new symbols, the stopping rule as the library's
host arithmetic (spira_adaptive_converged_*, the inline function the kernels call) equals its numpy restatement spira_hip/adaptive.py bit for
bit, hand-made cases sit on the side of the threshold they were made for, the schedule and workspace arithmetic of spira_plan.h survives a
sweep under ASan + UBSan, and the argument checks that run before device initialisation return their documented codes."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from spira_hip import adaptive, scenes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["spira_render_adaptive_f32", "spira_render_adaptive_f64", "spira_render_adaptive_scene_f32", "spira_render_adaptive_scene_f64",
       "spira_render_adaptive_scene_device_f32", "spira_render_adaptive_scene_device_f64", "spira_adaptive_converged_f32", "spira_adaptive_converged_f64"]


def test_library_exports_the_adaptive_symbols(binding):
    lib = binding.lib()
    for name in NEW:
        assert hasattr(lib, name), name
        assert name in binding.EXPORTS, name
    assert C.sizeof(binding.Adaptive) == 24
    assert [n for n, _ in binding.Adaptive._fields_] == ["min_spp", "batch_spp", "tolerance", "floor"]
    hdr = open(os.path.join(ROOT, "include", "spira_hip.h")).read()
    assert "typedef struct spira_adaptive {" in hdr and "uint32_t min_spp, batch_spp;" in hdr and "double   tolerance, floor;" in hdr


def test_adaptive_kernels_live_in_the_unit_of_their_precision_and_beside_k_path():
    """The feature's kernels have names of their own (no k_path instantiation was added: tests/test_abi_cpu.py counts those), Float32 ones in the
    Float32 translation unit, Float64 ones in the main unit, none in the mesh unit."""
    import re
    csrc = os.path.join(ROOT, "julia-spira_amd", "csrc")
    objs = {n: os.path.join(csrc, "spira_tu_%s.o" % n) for n in ("main", "f32", "f64mesh")}
    if not all(os.path.exists(o) for o in objs.values()):
        pytest.skip("objects not present (library built elsewhere)")
    syms = {n: subprocess.run(["nm", o], capture_output=True, text=True, check=True).stdout for n, o in objs.items()}
    for kern in ("18k_resolve_adaptive", "8k_refine", "19k_finalize_adaptive"):
        assert len(re.findall(kern + "If", syms["f32"])) > 0 and len(re.findall(kern + "Id", syms["f32"])) == 0, kern
        assert len(re.findall(kern + "Id", syms["main"])) > 0 and len(re.findall(kern + "If", syms["main"])) == 0, kern
        assert len(re.findall(kern + "I[fd]", syms["f64mesh"])) == 0, kern
        for text in syms.values():
            for line in text.splitlines():
                if kern in line:
                    assert "6k_pathI" not in line
    assert re.search(r" W _ZN8spira_tu4ImplIfE15render_adaptiveE", syms["f32"]) and re.search(r" U _ZN8spira_tu4ImplIfE15render_adaptiveE", syms["main"])
    mk = open(os.path.join(csrc, "Makefile")).read()
    assert "spira_adaptive.h" in mk.split("DEPS", 1)[1].split("\n", 1)[0]      # hashed into spira_build_id


def _random_inputs(rng, T, n):
    """Rule inputs that reach every branch: ordinary pixels (Q close to Y*Y/n, so that V rounds to either side of 0 and of rhs), n = 2, huge, tiny,
    infinite and NaN values."""
    cnt = rng.integers(2, 1 << 12, size=n).astype(np.uint32)
    cnt[rng.random(n) < 0.1] = 2
    cnt[rng.random(n) < 0.02] = 1 << 24
    mean = rng.random((3, n)) * 2.0
    s3 = (mean * cnt).astype(T)
    Y = adaptive.luma(s3[0], s3[1], s3[2], "f32" if T is np.float32 else "f64").astype(np.float64)
    # Q = Y^2 / n * (1 + spread): spread 0 puts V at the rounding level (either sign), small spreads put V near rhs for the tolerances below
    spread = np.choose(rng.integers(0, 4, size=n), [np.zeros(n), rng.normal(size=n) * 1e-7, rng.random(n) * 1e-2, rng.random(n) * 3.0])
    q = (Y * Y / cnt * (1.0 + spread)).astype(T)
    special = rng.random(n)
    big = np.finfo(T).max
    tiny = np.finfo(T).tiny
    for lo, hi, val in ((0.00, 0.01, np.nan), (0.01, 0.02, np.inf), (0.02, 0.03, big), (0.03, 0.04, tiny), (0.04, 0.05, tiny * np.finfo(T).eps)):
        sel = (special >= lo) & (special < hi)
        which = rng.integers(0, 4, size=n)
        for ch in range(3):
            s3[ch, sel & (which == ch)] = val
        q[sel & (which == 3)] = val
    return s3, q, cnt


@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_rule_matches_numpy_bitwise(binding, prec):
    T = np.float32 if prec == "f32" else np.float64
    cdt = C.c_float if prec == "f32" else C.c_double
    rng = np.random.default_rng(7 if prec == "f32" else 8)
    n = 120000
    s3, q, cnt = _random_inputs(rng, T, n)
    fn = binding.lib().spira_adaptive_converged_f32 if prec == "f32" else binding.lib().spira_adaptive_converged_f64
    fn.argtypes = [C.c_void_p, cdt, C.c_uint32, C.c_double, C.c_double]
    fn.restype = C.c_int
    seen = {0: 0, 1: 0}
    for tol, floor in ((0.0, 0.0), (1e-3, 0.0), (0.02, 0.0), (0.05, 0.01), (0.3, 1.0), (1e-30, 0.0), (1e30, 1e30), (5e-324, 0.0)):
        want = adaptive.converged(s3, q, cnt, tol, floor, prec)
        rows = np.ascontiguousarray(s3.T)
        got = np.empty(n, dtype=bool)
        base = rows.ctypes.data
        step = rows.strides[0]
        for k in range(n):
            rc = fn(base + k * step, cdt(q[k]), int(cnt[k]), tol, floor)
            assert rc in (0, 1), (k, rc)
            got[k] = rc == 1
        bad = np.nonzero(got != want)[0]
        assert bad.size == 0, (prec, tol, floor, bad[:5], s3[:, bad[:5]], q[bad[:5]], cnt[bad[:5]])
        if tol == 0.0:
            assert not got.any()                      # tolerance 0 never converges
        nan = np.isnan(s3).any(axis=0) | np.isnan(q)
        assert not got[nan].any()                     # a NaN anywhere: not converged
        seen[0] += int((~got).sum()); seen[1] += int(got.sum())
    assert seen[0] > n and seen[1] > n                # both answers well represented
    # V rounding negative really occurs in the inputs (n Q < Y Y by rounding) and is clamped, not rejected
    with np.errstate(all="ignore"):
        Y = adaptive.luma(s3[0], s3[1], s3[2], prec)
        d = cnt.astype(T) * q - Y * Y
    neg = (d < 0) & np.isfinite(d)
    assert neg.sum() > 1000
    assert adaptive.converged(s3, q, cnt, 0.05, 0.01, prec)[neg].all()


@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_rule_hand_made_cases(binding, prec):
    T = np.float32 if prec == "f32" else np.float64

    def sums(samples):            # samples: [n, 3] -> (sum3, Q) in sample order, in T
        s = np.zeros(3, dtype=T)
        q = T(0)
        for r in np.asarray(samples, dtype=T):
            s = s + r
            y = adaptive.luma(r[0], r[1], r[2], prec)
            q = q + y * y
        return s, q

    def both(samples, tol, floor=0.0):
        s, q = sums(samples)
        a = bool(adaptive.converged(s, q, len(samples), tol, floor, prec))
        b = binding.adaptive_converged(s, q, len(samples), tol, floor, prec)
        assert a == bool(b)
        return a

    # constant samples: zero variance, converged at min_spp = 2 for any tolerance > 0 — and never for tolerance 0
    const = [[0.5, 0.25, 0.125]] * 2
    assert both(const, 1e-3) and both(const * 8, 1e-3) and not both(const, 0.0)
    assert both([[0.0, 0.0, 0.0]] * 4, 0.05, 0.01)                   # a black pixel converges through the floor ...
    assert both([[0.0, 0.0, 0.0]] * 4, 0.05, 0.0)                    # ... and without one too (V = 0 <= rhs = 0)
    # two-valued grey samples: n/2 of luminance a and n/2 of b.  mean m = (a + b) / 2, sample variance s^2 = n (a - b)^2 / (4 (n - 1)),
    # standard error = |a - b| / (2 sqrt(n - 1)); relative to the mean: e = |a - b| / ((a + b) sqrt(n - 1))
    n, a, b = 16, 1.0, 0.5
    e = abs(a - b) / ((a + b) * np.sqrt(n - 1.0))
    grey = [[a, a, a]] * (n // 2) + [[b, b, b]] * (n // 2)           # (luminance of a grey sample = its value up to rounding of the weights' sum)
    assert not both(grey, e * 0.99) and both(grey, e * 1.01)
    assert not both(grey, e * 0.5) and both(grey, e * 2)
    # the floor loosens the threshold for dark pixels only: tolerance * (mean + floor)
    dark = [[0.02, 0.02, 0.02]] * 8 + [[0.0, 0.0, 0.0]] * 8
    assert not both(dark, 0.05, 0.0) and both(dark, 0.05, 1.0)
    # error codes of the host entry
    with pytest.raises(binding.SpiraError) as ex:
        binding.adaptive_converged(np.zeros(3), 0.0, 2, -1.0, 0.0, prec)
    assert "error -1" in str(ex.value)
    with pytest.raises(binding.SpiraError) as ex:
        binding.adaptive_converged(np.zeros(3), 0.0, 0, 0.1, 0.0, prec)
    assert "error -1" in str(ex.value)
    with pytest.raises(binding.SpiraError):
        binding.adaptive_converged(np.zeros(3), 0.0, 2, 0.1, float("nan"), prec)


def test_levels_and_counts_from_samples():
    assert adaptive.levels(8, 8, 40) == [8, 16, 24, 32, 40]
    assert adaptive.levels(8, 8, 41) == [8, 16, 24, 32, 40, 41]
    assert adaptive.levels(2, 1, 2) == [2] and adaptive.levels(4, 100, 64) == [4, 64]
    for bad in ((1, 1, 8), (2, 0, 8), (9, 1, 8)):
        with pytest.raises(ValueError):
            adaptive.levels(*bad)
    # three pixels: constant (stops at min), noisy (runs to the cap), constant-then-noisy (the rule never looks ahead: stops at min)
    rng = np.random.default_rng(3)
    rad = np.zeros((24, 3, 3))
    rad[:, :, 0] = 0.5
    rad[:, :, 1] = rng.random((24, 1)) * 5
    rad[:, :, 2] = 0.25
    rad[8:, :, 2] = rng.random((16, 1)) * 5
    n, s, q = adaptive.counts_from_samples(rad, 8, 8, 0.01, 0.0, "f64")
    assert list(n) == [8, 24, 8]
    assert np.array_equal(s[:, 0], [4.0, 4.0, 4.0]) and np.array_equal(s[:, 2], [2.0, 2.0, 2.0])      # the sums at the count the pixel stopped with
    seq = np.zeros(3)
    for k in range(24):
        seq = seq + rad[k, :, 1]
    assert np.array_equal(s[:, 1], seq)
    n0, _, _ = adaptive.counts_from_samples(rad, 8, 8, 0.0, 0.0, "f64")
    assert list(n0) == [24, 24, 24]                   # tolerance 0: everybody to the cap


def test_adaptive_plan_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "adaptive_plan")
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g", "-O1"]
    subprocess.run(["g++", "-std=c++17", "-ffp-contract=off", os.path.join(ROOT, "tests", "native", "adaptive_plan.cpp"), "-o", exe] + san, check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-6000:]
    assert "all checks passed" in r.stdout and "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr


def test_argument_validation_runs_before_the_device(binding):
    """Every documented argument error of the adaptive entries is reported before a device is looked for, so the codes can be checked here:
    bad schedules SPIRA_E_INVALID (-1), estimators / organisations / extensions outside the scope SPIRA_E_UNSUPPORTED (-5)."""
    s = scenes.scene_s1()
    sp, ma, cam = s["spheres5"], s["materials8"], s["camera12"]

    def err(params, ad, prec="f32", **kw):
        with pytest.raises(binding.SpiraError) as e:
            binding.render_adaptive(sp, ma, None, cam, params, ad, prec, **kw)
        return str(e.value)
    P = lambda **kw: binding.make_params(16, 9, kw.pop("spp", 16), kw.pop("depth", 4), 5, 5, **kw)
    good = binding.make_adaptive(4, 4, 0.05, 0.01)
    for prec in ("f32", "f64"):
        assert "error -1" in err(P(), binding.make_adaptive(1, 4, 0.05), prec)            # min_spp < 2
        assert "error -1" in err(P(), binding.make_adaptive(4, 0, 0.05), prec)            # batch_spp < 1
        assert "error -1" in err(P(spp=3), good, prec)                                    # min_spp > cap
        assert "error -1" in err(P(), binding.make_adaptive(4, 4, -0.05), prec)           # negative tolerance
        assert "error -1" in err(P(), binding.make_adaptive(4, 4, 0.05, -1.0), prec)      # negative floor
        assert "error -1" in err(P(), binding.make_adaptive(4, 4, float("nan")), prec)
        assert "error -1" in err(P(depth=0), good, prec)                                  # nothing to sample
        assert "error -1" in err(P(), good, prec, want_hdr=False, want_spp=False, want_q=False)      # no output at all
        for flags in (binding.SEM_CPU, binding.SEM_METAL, binding.SEM_HYBRID, binding.KERNEL_MEGA, binding.KERNEL_BOUNCE, binding.KERNEL_WAVEFRONT,
                      binding.EXT_DIELECTRIC, binding.EXT_SPECTRAL):
            assert "error -5" in err(P(flags=flags), good, prec), hex(flags)
        assert "error -4" in err(P(spp=(1 << 24) + 1), good, prec)                        # the cap obeys the limits of every entry
    rc = binding.lib().spira_render_adaptive_f32(None, None, None, None, None, None, None, None, None, None)
    assert rc == -1
    if binding.device_count() == 0:                   # and a valid call fails loudly without a device: no CPU fallback here either
        assert "error -2" in err(P(), good)
