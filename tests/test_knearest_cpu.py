"""CPU: spira_scene_nearest_k_* without a device — header, library and binding name the four entries and the two constants (ABI still 3); near_offer and
near_insert (spira_knearest.h), the functions the kernels keep a lane's list with, and nearest_k_check (spira_plan.h) pass tests/native/knearest_plan.cpp
under ASan + UBSan, the lists and bounds bit for bit against a sort; every argument error comes back with its own code and no device; the kernels sit in
the translation unit of their precision; and the yardstick (tests/knearest_support.py) has the points its tests are for and agrees with
nearest_support.NearScan at K = 1."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import cast_support as S
import knearest_support as KS
import nearest_support as N

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["spira_scene_nearest_k_f32", "spira_scene_nearest_k_f64", "spira_scene_nearest_k_device_f32", "spira_scene_nearest_k_device_f64"]


def test_library_header_and_binding_name_the_entries(binding):
    lib = binding.lib()
    hdr = open(os.path.join(ROOT, "include", "spira_hip.h")).read()
    for name in NEW:
        assert hasattr(lib, name) and name in binding.EXPORTS and re.search(r"^int %s\(const spira_scene \*scene, " % name, hdr, flags=re.M), name
    assert "#define SPIRA_ABI_VERSION 3 " in hdr and lib.spira_abi_version() == 3
    for const, val in (("SPIRA_MAX_NEAR", "16u"), ("SPIRA_NEAR_COUNT_ALL", "0x2u"), ("SPIRA_CAST_INPLACE", "0x1u")):
        assert re.search(r"^#define %s\s+%s" % (const, re.escape(val)), hdr, flags=re.M), const
    assert (binding.MAX_NEAR, binding.NEAR_COUNT_ALL) == (16, 2) and KS.MAX_NEAR == binding.MAX_NEAR
    for m in ("nearest_k", "nearest_k_device"):
        assert hasattr(binding.Scene, m), m
    from spira_hip import query
    for f in ("k_nearest", "count_within"):
        assert callable(getattr(query, f)), f
    mk = open(os.path.join(ROOT, "julia-spira_amd", "csrc", "Makefile")).read()
    assert "spira_knearest.h" in mk.split("DEPS", 1)[1].split("\n", 1)[0]      # hashed into spira_build_id


def test_knear_kernels_live_in_the_unit_of_their_precision():
    csrc = os.path.join(ROOT, "julia-spira_amd", "csrc")
    objs = {n: os.path.join(csrc, "spira_tu_%s.o" % n) for n in ("main", "f32", "f64mesh")}
    if not all(os.path.exists(o) for o in objs.values()):
        pytest.skip("objects not present (library built elsewhere)")
    syms = {n: subprocess.run(["nm", o], capture_output=True, text=True, check=True).stdout for n, o in objs.items()}
    for kern in ("7k_knear", "15k_knear_session"):
        assert len(re.findall(kern + "If", syms["f32"])) > 0 and len(re.findall(kern + "Id", syms["f32"])) == 0, kern
        assert len(re.findall(kern + "Id", syms["main"])) > 0 and len(re.findall(kern + "If", syms["main"])) == 0, kern
        assert len(re.findall(kern + "I[fd]", syms["f64mesh"])) == 0, kern
    assert re.search(r" W _ZN8spira_tu4ImplIfE9nearest_kE", syms["f32"]) and re.search(r" U _ZN8spira_tu4ImplIfE9nearest_kE", syms["main"])


@pytest.fixture(scope="module")
def knearest_plan_exe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("knearest") / "knearest_plan")
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g", "-O1"]
    subprocess.run(["g++", "-std=c++17", "-ffp-contract=off", os.path.join(ROOT, "tests", "native", "knearest_plan.cpp"), "-o", exe] + san, check=True)
    return exe


def _streams(T, seed):
    """Candidate streams heavy with ties, for every K in 0 .. 16 (so every K in 0 .. CAP of every capacity): d2 from a handful of values — best0 itself
    (a candidate exactly at the bound), the value one ulp beyond it (never one), a NaN (never one) and values met many times — and indices drawn from a
    small range without repeats, so equal d2 meets neighbouring indices.  Lengths from none to far more than K.  Each with K, best0 and count_all."""
    rng = np.random.default_rng(seed)
    out = []
    for K in range(0, 17):
        for n in (0, 1, 3, 17, 40):
            best0 = T(rng.choice([2.5, 7.0, np.inf]))
            beyond = np.nextafter(best0, T(np.inf)) if np.isfinite(best0) else T(np.nan)
            vals = np.array([0.0, 0.5, 1.25, np.nextafter(T(1.25), T(2)), 2.5, float(best0) if np.isfinite(best0) else 1e30, beyond, np.nan], dtype=T)
            d2 = vals[rng.integers(0, len(vals), n)]
            prim = rng.permutation(max(n + 4, 8))[:n].astype(np.int64)
            for count_all in ((0, 1) if K in (0, 1, 4, 16) or n == 40 else (0,)):
                if K == 0 and not count_all:
                    continue                                          # (refused by the entries)
                out.append((K, best0, count_all, d2, prim))
    return out


def _feed(prec, K, best0, count_all, d2, prim):
    U = np.uint32 if prec == "f32" else np.uint64
    head = "%s %d %x %d %d\n" % (prec, K, int(np.array([best0]).view(U)[0]), count_all, len(d2))
    return head + "".join("%x %d\n" % (int(b), int(p)) for b, p in zip(d2.view(U), prim))


@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_near_offer_and_nearest_k_check_under_asan_ubsan(knearest_plan_exe, prec):
    T = S.dtype_of(prec)
    U = np.uint32 if prec == "f32" else np.uint64
    bits = lambda x: int(np.array([x], dtype=T).view(U)[0])
    streams = _streams(T, 5 if prec == "f32" else 6)
    rng = np.random.default_rng(78)
    text, want = "", []
    seen = dict(nan=0, at_bound=0, beyond=0, more=0, ties=0)
    for K, best0, count_all, d2, prim in streams:
        cands = [(float(d), int(p)) for d, p in zip(d2.tolist(), prim.tolist()) if d <= float(best0)]       # a NaN is never one
        order = sorted(cands, key=lambda e: (e[0], -e[1]))[:K]
        bound = T(order[-1][0]) if (len(order) == K and K > 0 and not count_all) else best0
        exp = (len(order), bits(bound), [(bits(e[0]), e[1]) for e in order])
        seen["nan"] += int(np.isnan(d2).any()); seen["at_bound"] += int((d2 == best0).any()); seen["beyond"] += int((d2 > best0).any())
        seen["more"] += len(cands) > K; seen["ties"] += len({e[0] for e in order}) < len(order)
        for _ in range(2):                                           # the stream as drawn, then shuffled: the same list
            text += _feed(prec, K, best0, count_all, d2, prim)
            want.append((K, count_all, len(cands), exp))
            sh = rng.permutation(len(d2))
            d2, prim = d2[sh], prim[sh]
    assert min(seen.values()) >= 8, seen
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([knearest_plan_exe], input=text, capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-6000:]
    assert "rules checked" in r.stdout and "all checks passed" in r.stdout and "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr
    cases = r.stdout.split("case ")[1:]
    assert len(cases) == len(want)
    for block, (K, count_all, n_cands, exp) in zip(cases, want):
        lists = re.findall(r"^list ([qr]) (\d+) (\d+) ([0-9a-f]+) (\d+)(.*)$", block, flags=re.M)
        caps = [c for c in (1, 4, 16) if K <= c]
        assert [(l[0], int(l[1])) for l in lists] == [(kind, c) for c in caps for kind in "qr"], (K, lists)      # every capacity that holds K, both kinds of entry
        for kind, cap, n, bound, total, rest in lists:
            got = [(int(a, 16), int(b)) for a, b in re.findall(r"([0-9a-f]+):(-?\d+)", rest)]
            assert (int(n), int(bound, 16), got) == exp, (K, count_all, kind, cap, got, exp)
            if count_all:
                assert int(total) == n_cands, (K, kind, cap, total, n_cands)      # every candidate is counted when the bound stays best0
            else:
                assert len(exp[2]) <= int(total) <= n_cands


def test_return_codes_without_a_device(binding):
    """Every argument error is decided before any device is touched: it returns its own code, never SPIRA_E_NO_DEVICE (-2)."""
    lib = binding.lib()
    pts = np.zeros((4, 4), dtype=np.float64)
    pp, out = pts.ctypes.data_as(C.c_void_p), np.zeros(1024, dtype=np.float64).ctypes.data_as(C.c_void_p)
    u32 = C.c_uint32
    for name in NEW:
        fn = getattr(lib, name)
        tail = (None,) if "device" in name else ()

        def call(p, n, k, flags, outs):
            return fn(None, p, u32(n), u32(k), u32(flags), *(outs + tail))
        outs = (out, out, out, out, None)                            # prim, dist, point, count, trips
        assert call(None, 4, 1, 0, outs) == -1 and b"point array is NULL" in lib.spira_last_error(), name
        assert call(pp, 0, 1, 0, outs) == -1 and b"n_points is 0" in lib.spira_last_error(), name
        assert call(pp, 4, 1, 4, outs) == -1 and b"unknown flag bits" in lib.spira_last_error(), name
        assert call(pp, 4, 1, 0x80000001, outs) == -1 and b"unknown flag bits" in lib.spira_last_error(), name
        assert call(pp, 4, 17, 0, outs) == -1 and b"SPIRA_MAX_NEAR" in lib.spira_last_error(), name
        assert call(pp, 4, 0, 0, outs) == -1 and b"without SPIRA_NEAR_COUNT_ALL" in lib.spira_last_error(), name
        assert call(pp, 4, 0, 1, outs) == -1, name
        assert call(pp, 4, 2, 0, (None, None, None, None, out)) == -1 and b"all NULL" in lib.spira_last_error(), name      # trips alone is no output
        assert call(pp, 4, 0, 2, (out, out, out, None, None)) == -1 and b"out_count is NULL" in lib.spira_last_error(), name   # the lists are ignored at max_near 0
        assert call(pp, (1 << 26) + 1, 1, 0, outs) == -4 and b"SPIRA_MAX_RAYS" in lib.spira_last_error(), name
        assert call(pp, (1 << 22) + 1, 16, 0, outs) == -4 and b"n_points * max_near" in lib.spira_last_error(), name
        assert call(pp, 1 << 28, 16, 0, outs) == -4, name                                                                  # 2^32: the product is formed in 64 bits
        assert call(pp, 1 << 31, 2, 0, outs) == -4, name
        for flags, k, o in ((0, 1, outs), (1, 16, outs), (2, 0, (None, None, None, out, None)), (3, 4, (out, None, None, None, None)),
                            (0, 3, (None, out, None, None, None)), (0, 5, (None, None, out, None, None)), (2, 2, (None, None, None, out, out))):
            assert call(pp, 4, k, flags, o) == -1 and b"scene handle is NULL or was destroyed" in lib.spira_last_error(), (name, flags, k)


def test_the_point_sets_reach_what_they_are_for():
    """The conditions of knearest_support for every scene and K the GPU tests use, from the yardstick alone."""
    for prec in ("f32", "f64"):
        for name in ("s1", "ico32", "ico80", "s4_3"):
            KS.conditions(KS.reference(name, prec), 4)
        for K in (1, 2, 3, 4, 5, 15, 16):
            KS.conditions(KS.reference("ico33", prec), K)
            more, fewer, none, tied = KS.conditions(KS.reference("dup", prec), K, ties=True)
            assert tied >= 64, (prec, K, tied)
        for name, K in (("s4_3", 4), ("dup", 3), ("dup", 16)):
            KS.edge_set(name, prec, K)


@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_the_yardstick_at_one_is_the_closest_point_scan(prec):
    """knearest_support's order cut to K = 1 is nearest_support.NearScan.query, on the tree scene and on the duplicate scene's ties; and every K is a
    prefix of the next."""
    for name in ("s4_3", "dup"):
        ref, scan = KS.reference(name, prec), N.reference(name, prec)
        prim, dist, point, count = KS.cut(ref, 1)
        assert np.array_equal(prim[:, 0], scan["prim"]) and np.array_equal(dist[:, 0], scan["dist"]) and np.array_equal(point[:, 0], scan["point"])
        assert np.array_equal(count, (scan["prim"] >= 0).astype(np.uint32))
        p4, d4, q4, c4 = KS.cut(ref, 4)
        p16, d16, q16, c16 = KS.cut(ref, 16)
        full = c16 == 16
        assert full.sum() > 64 and np.array_equal(p4[full], p16[full, :4]) and np.array_equal(q4[full], q16[full, :4])
        d2 = ref["d2"][full, :16]
        assert (np.diff(d2, axis=1) >= 0).all()
        tie = np.diff(d2, axis=1) == 0
        assert (np.diff(p16[full], axis=1)[tie] < 0).all()           # among equal d2: the later object first
