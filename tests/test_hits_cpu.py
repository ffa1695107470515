"""CPU: spira_scene_cast_hits_* without a device — header, library and binding name the four entries and the two constants (ABI still 3); hits_insert
(spira_hits.h), the one function the kernels keep a lane's list with, and hits_check (spira_plan.h) pass tests/native/hits_plan.cpp under ASan + UBSan,
the lists and bounds bit for bit against sorted(...)[:K]; every argument error comes back with its own code and no device; the kernels sit in the
translation unit of their precision; and the yardstick (tests/hits_support.py) agrees with cast_support.Scan at K = 1."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import cast_support as S
import hits_support as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["spira_scene_cast_hits_f32", "spira_scene_cast_hits_f64", "spira_scene_cast_hits_device_f32", "spira_scene_cast_hits_device_f64"]


def test_library_header_and_binding_name_the_entries(binding):
    lib = binding.lib()
    hdr = open(os.path.join(ROOT, "include", "spira_hip.h")).read()
    for name in NEW:
        assert hasattr(lib, name) and name in binding.EXPORTS and re.search(r"^int %s\(const spira_scene \*scene, " % name, hdr, flags=re.M), name
    assert "#define SPIRA_ABI_VERSION 3 " in hdr and lib.spira_abi_version() == 3
    for const, val in (("SPIRA_MAX_HITS", "16u"), ("SPIRA_HITS_COUNT_ALL", "0x2u"), ("SPIRA_CAST_INPLACE", "0x1u")):
        assert re.search(r"^#define %s\s+%s" % (const, re.escape(val)), hdr, flags=re.M), const
    assert (binding.MAX_HITS, binding.HITS_COUNT_ALL) == (16, 2)
    for m in ("cast_hits", "cast_hits_device"):
        assert hasattr(binding.Scene, m), m
    from spira_hip import query
    for f in ("cast_all", "count_hits", "inside_mesh"):
        assert callable(getattr(query, f)), f
    mk = open(os.path.join(ROOT, "julia-spira_amd", "csrc", "Makefile")).read()
    assert "spira_hits.h" in mk.split("DEPS", 1)[1].split("\n", 1)[0]      # hashed into spira_build_id


@pytest.fixture(scope="module")
def hits_plan_exe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("hits") / "hits_plan")
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g", "-O1"]
    subprocess.run(["g++", "-std=c++17", "-ffp-contract=off", os.path.join(ROOT, "tests", "native", "hits_plan.cpp"), "-o", exe] + san, check=True)
    return exe


def _sequences(T, seed):
    """Candidate sequences heavy with ties: t from a handful of values (t_max itself among them), indices drawn from a small range without repeats, so
    equal t meets neighbouring indices.  Each with K and t_max."""
    rng = np.random.default_rng(seed)
    out = []
    for K in (1, 2, 3, 4, 5, 15, 16):
        for n in (0, 1, 3, 17, 40):
            t_max = T(rng.choice([2.5, 7.0, np.inf]))
            vals = np.array([0.0, 0.5, 1.25, np.nextafter(T(1.25), T(2)), 2.5, float(t_max) if np.isfinite(t_max) else 1e30], dtype=T)
            vals = vals[vals <= t_max]
            t = vals[rng.integers(0, len(vals), n)]
            prim = rng.permutation(max(n + 4, 8))[:n].astype(np.int64)
            out.append((K, t_max, t, prim))
    return out


def _feed(prec, K, t_max, t, prim):
    U = np.uint32 if prec == "f32" else np.uint64
    head = "%s %d %x %d\n" % (prec, K, int(np.array([t_max]).view(U)[0]), len(t))
    return head + "".join("%x %d\n" % (int(b), int(p)) for b, p in zip(t.view(U), prim))


@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_hits_insert_and_hits_check_under_asan_ubsan(hits_plan_exe, prec):
    T = S.dtype_of(prec)
    U = np.uint32 if prec == "f32" else np.uint64
    seqs = _sequences(T, 3 if prec == "f32" else 4)
    rng = np.random.default_rng(77)
    text, want = "", []
    for K, t_max, t, prim in seqs:
        order = sorted(zip(t.tolist(), prim.tolist()), key=lambda e: (e[0], -e[1]))[:K]
        bound = T(order[-1][0]) if len(order) == K else t_max
        exp = (len(order), int(np.array([bound], dtype=T).view(U)[0]), [(int(np.array([e[0]], dtype=T).view(U)[0]), e[1]) for e in order])
        for _ in range(2):                                       # the sequence as drawn, then shuffled: the same list
            text += _feed(prec, K, t_max, t, prim)
            want.append((K, exp))
            sh = rng.permutation(len(t))
            t, prim = t[sh], prim[sh]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([hits_plan_exe], input=text, capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-6000:]
    assert "rules checked" in r.stdout and "all checks passed" in r.stdout and "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr
    cases = r.stdout.split("case ")[1:]
    assert len(cases) == len(want)
    ties = 0
    for block, (K, exp) in zip(cases, want):
        lists = re.findall(r"^list (\d+) (\d+) ([0-9a-f]+)(.*)$", block, flags=re.M)
        assert [int(l[0]) for l in lists] == [c for c in (1, 4, 16) if K <= c or c == 16], (K, lists)
        for cap, n, bound, rest in lists:
            got = [(int(a, 16), int(b)) for a, b in re.findall(r"([0-9a-f]+):(-?\d+)", rest)]
            assert (int(n), int(bound, 16), got) == exp, (K, cap, got, exp)
        ties += len({e[0] for e in exp[2]}) < len(exp[2])
    assert ties >= 8                                             # equal t inside the kept lists, resolved by index


def test_return_codes_without_a_device(binding):
    """Every argument error is decided before any device is touched: it returns its own code, never SPIRA_E_NO_DEVICE (-2)."""
    lib = binding.lib()
    rays = np.zeros((4, 8), dtype=np.float64)
    rp, out = rays.ctypes.data_as(C.c_void_p), np.zeros(256, dtype=np.float64).ctypes.data_as(C.c_void_p)
    u32 = C.c_uint32
    for name in NEW:
        fn = getattr(lib, name)
        tail = (None,) if "device" in name else ()

        def call(r, n, k, flags, outs):
            return fn(None, r, u32(n), u32(k), u32(flags), *(outs + tail))
        outs = (out, out, out)
        assert call(None, 4, 1, 0, outs) == -1 and b"ray array is NULL" in lib.spira_last_error(), name
        assert call(rp, 0, 1, 0, outs) == -1 and b"n_rays is 0" in lib.spira_last_error(), name
        assert call(rp, 4, 1, 4, outs) == -1 and b"unknown flag bits" in lib.spira_last_error(), name
        assert call(rp, 4, 17, 0, outs) == -1 and b"SPIRA_MAX_HITS" in lib.spira_last_error(), name
        assert call(rp, 4, 0, 0, outs) == -1 and b"without SPIRA_HITS_COUNT_ALL" in lib.spira_last_error(), name
        assert call(rp, 4, 0, 1, outs) == -1, name
        assert call(rp, 4, 2, 0, (None, None, None)) == -1 and b"all NULL" in lib.spira_last_error(), name
        assert call(rp, 4, 0, 2, (out, out, None)) == -1 and b"out_count is NULL" in lib.spira_last_error(), name
        assert call(rp, (1 << 26) + 1, 1, 0, outs) == -4 and b"SPIRA_MAX_RAYS" in lib.spira_last_error(), name
        assert call(rp, (1 << 22) + 1, 16, 0, outs) == -4 and b"n_rays * max_hits" in lib.spira_last_error(), name
        assert call(rp, 1 << 28, 16, 0, outs) == -4, name
        for flags, k, o in ((0, 1, outs), (1, 16, outs), (2, 0, (None, None, out)), (3, 4, (out, None, None)), (0, 3, (None, out, None))):
            assert call(rp, 4, k, flags, o) == -1 and b"scene handle is NULL or was destroyed" in lib.spira_last_error(), (name, flags, k)


def test_hits_kernels_live_in_the_unit_of_their_precision():
    csrc = os.path.join(ROOT, "julia-spira_amd", "csrc")
    objs = {n: os.path.join(csrc, "spira_tu_%s.o" % n) for n in ("main", "f32", "f64mesh")}
    if not all(os.path.exists(o) for o in objs.values()):
        pytest.skip("objects not present (library built elsewhere)")
    syms = {n: subprocess.run(["nm", o], capture_output=True, text=True, check=True).stdout for n, o in objs.items()}
    for kern in ("6k_hits", "14k_hits_session"):
        assert len(re.findall(kern + "If", syms["f32"])) > 0 and len(re.findall(kern + "Id", syms["f32"])) == 0, kern
        assert len(re.findall(kern + "Id", syms["main"])) > 0 and len(re.findall(kern + "If", syms["main"])) == 0, kern
        assert len(re.findall(kern + "I[fd]", syms["f64mesh"])) == 0, kern
    assert re.search(r" W _ZN8spira_tu4ImplIfE4hitsE", syms["f32"]) and re.search(r" U _ZN8spira_tu4ImplIfE4hitsE", syms["main"])


@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_the_yardstick_at_one_hit_is_the_closest_hit_scan(oracle, prec):
    """hits_support's sort cut to K = 1 is cast_support.Scan.cast on a shells scene (spheres, many triangles per ray) and on the ties set's duplicates."""
    scene = H.shells_scene(1, n_shells=4)
    rays = H.rays_through(np.random.default_rng(1), scene, 48)
    for sc_scene, rr in ((scene, rays), (S.ties_set(prec)["scene"], S.ties_set(prec)["rays"]["rays"][:48])):
        ref = H.reference(sc_scene, prec, rr)
        prim, t, count, total = H.cut(ref["cands"], ref["prepared"], ref["sc"].T, 1)
        c_prim, c_t, valid, _ = ref["sc"].cast(rr)
        assert np.array_equal(prim[:, 0], c_prim) and np.array_equal(t[:, 0], c_t) and np.array_equal(count, (c_prim >= 0).astype(np.uint32))
        assert (total >= 2).sum() >= 8 and (total == 0).sum() >= 1
