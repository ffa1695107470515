"""CPU: spira_scene_signed_distance_* without a device — header, library, binding and query name the four entries and the constant (ABI still 3);
spira_sdf.h is hashed into the build id; the kernels sit in the translation unit of their precision; signed_distance_check (spira_plan.h) and the
HIP-free part of spira_sdf.h pass tests/native/sdf_plan.cpp under ASan + UBSan; every argument error comes back with its own code and no device; and
the yardstick (tests/sdf_support.py) holds its premises, so that the GPU tests test the kernel and not the luck of the inputs: (a) on a convex mesh its
sign is the ground truth for every point, (b) on an open mesh both vote outcomes occur often, (c) on a closed mesh the signed distance is Lipschitz."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import cast_support as S
import sdf_support as D
from spira_hip import query

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["spira_scene_signed_distance_f32", "spira_scene_signed_distance_f64", "spira_scene_signed_distance_device_f32", "spira_scene_signed_distance_device_f64"]


def test_library_header_and_binding_name_the_entries(binding):
    lib = binding.lib()
    hdr = open(os.path.join(ROOT, "include", "spira_hip.h")).read()
    for name in NEW:
        assert hasattr(lib, name) and name in binding.EXPORTS and re.search(r"^int %s\(const spira_scene \*scene, " % name, hdr, flags=re.M), name
    assert "#define SPIRA_ABI_VERSION 3 " in hdr and lib.spira_abi_version() == 3
    assert re.search(r"^#define SPIRA_SDF_SKIPPED\s+0xFFFFFFFFu", hdr, flags=re.M)
    assert binding.SDF_SKIPPED == 0xFFFFFFFF and D.SKIPPED == 0xFFFFFFFF
    assert "meaningful for closed meshes" in " ".join(hdr.lower().split()) and "defined" in hdr.lower()
    for m in ("signed_distance", "signed_distance_device"):
        assert hasattr(binding.Scene, m), m
    for f in ("signed_distance", "inside_points", "distance_field", "signed_distance_rules", "inside_spheres"):
        assert callable(getattr(query, f)), f
    mk = open(os.path.join(ROOT, "julia-spira_amd", "csrc", "Makefile")).read()
    assert "spira_sdf.h" in mk.split("DEPS", 1)[1].split("\n", 1)[0]      # hashed into spira_build_id


def test_sdf_kernels_live_in_the_unit_of_their_precision():
    csrc = os.path.join(ROOT, "julia-spira_amd", "csrc")
    objs = {n: os.path.join(csrc, "spira_tu_%s.o" % n) for n in ("main", "f32", "f64mesh")}
    if not all(os.path.exists(o) for o in objs.values()):
        pytest.skip("objects not present (library built elsewhere)")
    syms = {n: subprocess.run(["nm", o], capture_output=True, text=True, check=True).stdout for n, o in objs.items()}
    for kern in ("5k_sdf", "13k_sdf_session"):
        assert len(re.findall(kern + "If", syms["f32"])) > 0 and len(re.findall(kern + "Id", syms["f32"])) == 0, kern
        assert len(re.findall(kern + "Id", syms["main"])) > 0 and len(re.findall(kern + "If", syms["main"])) == 0, kern
        assert len(re.findall(kern + "I[fd]", syms["f64mesh"])) == 0, kern
    assert re.search(r" W _ZN8spira_tu4ImplIfE15signed_distanceE", syms["f32"]) and re.search(r" U _ZN8spira_tu4ImplIfE15signed_distanceE", syms["main"])


@pytest.fixture(scope="module")
def sdf_plan_exe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("sdf") / "sdf_plan")
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g", "-O1"]
    subprocess.run(["g++", "-std=c++17", "-ffp-contract=off", os.path.join(ROOT, "tests", "native", "sdf_plan.cpp"), "-o", exe] + san, check=True)
    return exe


def test_signed_distance_check_and_the_rays_under_asan_ubsan(sdf_plan_exe):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([sdf_plan_exe], capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-6000:]
    for line in ("rules checked", "vote checked", "all checks passed"):
        assert line in r.stdout
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr
    # the rays the kernels make are query.INSIDE_DIRECTIONS rounded to T under normalize_rays, bit for bit
    rows = re.findall(r"^ray (f32|f64) (\d) ([0-9a-f ]+) \| ([0-9a-f ]+)$", r.stdout, flags=re.M)
    assert len(rows) == 6
    p = np.array([[0.25, -1.5, 3.0]])
    for prec, j, ray, unit in rows:
        T, U = S.dtype_of(prec), (np.uint32 if prec == "f32" else np.uint64)
        rays, valid = query.normalize_rays(D.rays_of(p, int(j)), T)
        assert valid.all()
        want_ray = np.array(D.rays_of(p, int(j)), dtype=T)[0].view(U)
        assert [int(x, 16) for x in ray.split()] == [int(x) for x in want_ray], (prec, j)
        assert [int(x, 16) for x in unit.split()] == [int(x) for x in rays[0, 4:7].view(U)], (prec, j)


def test_return_codes_without_a_device(binding):
    """Every argument error is decided before any device is touched: it returns its own code, never SPIRA_E_NO_DEVICE (-2)."""
    lib = binding.lib()
    pts = np.zeros((4, 4), dtype=np.float64)
    pp, out = pts.ctypes.data_as(C.c_void_p), np.zeros(1024, dtype=np.float64).ctypes.data_as(C.c_void_p)
    u32 = C.c_uint32
    for name in NEW:
        fn = getattr(lib, name)
        tail = (None,) if "device" in name else ()

        def call(p, n, flags, outs):
            return fn(None, p, u32(n), u32(flags), *(outs + tail))
        outs = (out, out, out, out, out, None)                       # prim, dist, point, inside, crossings, trips
        assert call(None, 4, 0, outs) == -1 and b"point array is NULL" in lib.spira_last_error(), name
        assert call(pp, 0, 0, outs) == -1 and b"n_points is 0" in lib.spira_last_error(), name
        for flags in (2, 4, 3, 0x80000001):
            assert call(pp, 4, flags, outs) == -1 and b"unknown flag bits" in lib.spira_last_error(), (name, flags)
        assert call(pp, 4, 0, (None, None, None, None, None, out)) == -1 and b"all NULL" in lib.spira_last_error(), name      # trips alone is no output
        assert call(pp, (1 << 26) + 1, 0, outs) == -4 and b"SPIRA_MAX_RAYS" in lib.spira_last_error(), name
        assert call(pp, 1 << 31, 1, outs) == -4, name
        for m in range(1, 32):                                       # every other NULL combination reaches the handle check
            o = tuple(out if (m >> k) & 1 else None for k in range(5)) + (None,)
            for flags in (0, 1):
                assert call(pp, 4, flags, o) == -1 and b"scene handle is NULL or was destroyed" in lib.spira_last_error(), (name, m, flags)


def test_the_rules_of_query_are_the_yardsticks():
    """query.signed_distance_rules and query.inside_spheres (numpy, vectorised) against sdf_support's own restatement, on every kind of row."""
    rng = np.random.default_rng(2)
    n = 512
    valid = rng.random(n) > 0.1
    counts = rng.integers(0, 7, (n, 3)).astype(np.uint32)
    in_sphere = rng.random(n) > 0.8
    prim = np.where(valid, rng.integers(-1, 5, n), S.INVALID).astype(np.int32)
    dist = np.where(valid, rng.random(n), 0.0)
    dist[::17] = 0.0
    point = rng.random((n, 3))
    for with_mesh in (True, False):
        inside, cr = D.decide(valid, in_sphere, counts, with_mesh)
        g_prim, g_dist, g_point, g_inside, g_cr = query.signed_distance_rules(valid, prim, dist, point, in_sphere, counts, with_mesh)
        assert np.array_equal(g_inside, inside) and np.array_equal(g_cr, cr) and np.array_equal(g_prim, prim) and np.array_equal(g_point, point)
        neg = inside == 1
        assert np.array_equal(np.signbit(g_dist), neg | np.signbit(dist)) and np.array_equal(np.abs(g_dist), np.abs(dist))
        assert (np.signbit(g_dist) & (g_dist == 0)).any() == bool((neg & (dist == 0)).any())      # -0.0 occurs where an inside point has distance 0
    for prec in ("f32", "f64"):
        T = S.dtype_of(prec)
        for ref in (D.blob_ref(prec), D.spheres_ref(prec)):
            v = ref["valid"]
            a = query.inside_spheres(ref["scene"]["spheres5"], ref["points"][:, :3], T)
            b = D.in_spheres(ref["scene"], T, ref["points"][:, :3])
            assert np.array_equal(a[v], b[v]) and 8 < b[v].sum() < v.sum() - 8


@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_the_sets_reach_what_they_are_for(prec):
    """What the GPU cases rely on, from the yardstick alone: every scene has points on both sides, misses, invalid points; the blob scene has points
    inside the light sphere and outside the mesh; the spheres-only scene's slots are all SKIPPED; the LDS scene has no tree."""
    blob, lds, sph = D.blob_ref(prec), D.lds_ref(prec), D.spheres_ref(prec)
    for ref in (blob, lds, sph):
        v = ref["valid"]
        assert (ref["inside"][v] == 1).sum() >= 32 and (ref["inside"][v] == 0).sum() >= 32, (prec, np.bincount(ref["inside"]))
        assert (ref["inside"][~v] == 255).all() and len(ref["invalid_at"]) >= 9 and not ref["crossings"][~v].any() and not ref["dist"][~v].any()
        assert np.array_equal(np.flatnonzero(~v), ref["invalid_at"])
        assert ((ref["prim"] == D.MISS) & v).sum() >= 4                                  # finite r_max: misses, r_max copied and signed
        assert np.array_equal(np.signbit(ref["dist"][v]), ref["inside"][v] == 1)
    assert blob["scan"].frame is not None and lds["scan"].frame is None and len(lds["scene"]["triangles10"]) == 32
    light = blob["scene"]["spheres5"][1]
    in_light = np.linalg.norm(blob["points"][:, :3] - light[:3], axis=1) < 0.99 * light[3]
    odd = D.decide(blob["valid"], np.zeros(len(in_light), dtype=bool), blob["counts"], True)[0] == 1
    assert (in_light & blob["valid"] & ~odd).sum() >= 8 and (blob["inside"][in_light & blob["valid"]] == 1).all()      # inside by step 2 alone
    assert (odd & ~D.in_spheres(blob["scene"], S.dtype_of(prec), blob["points"][:, :3])).sum() >= 32                 # inside by step 3 alone
    assert (sph["crossings"][sph["valid"]] == D.SKIPPED).all()
    assert (blob["crossings"][blob["valid"]][:, 2] == D.SKIPPED).sum() >= 64


@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_convex_mesh_ground_truth(prec):
    """(a) scenes.icosphere(3), 1 280 triangles: for ALL 400 points — |p - c| <= 0.95 r_in or >= 1.05 R — the yardstick's inside is |p - c| < r_in."""
    ref = D.convex_ref(prec)
    assert len(ref["scene"]["triangles10"]) == 1280 and ref["scan"].frame is not None and ref["valid"].all()
    radius = np.linalg.norm(ref["points"][:, :3], axis=1)
    assert ((radius <= 0.95 * ref["r_in"]) | (radius >= 1.05 * ref["R"])).all() and 0.9 < ref["r_in"] < ref["R"] <= 1.0 + 1e-12
    truth = radius < ref["r_in"]
    assert np.array_equal(truth, ref["truth"]) and truth.sum() == 200
    assert np.array_equal(ref["inside"] == 1, truth), np.flatnonzero((ref["inside"] == 1) != truth)
    assert np.array_equal(np.signbit(ref["dist"]), truth)


@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_open_mesh_votes_disagree_and_agree(prec):
    """(b) cast_support.quad_scene(): of 300 points at least a quarter have c_0 and c_1 of different parity (ray 2 decides) and a quarter agree."""
    ref = D.quad_ref(prec)
    assert ref["valid"].all() and len(ref["points"]) == 300
    differ, agree = D.vote_split(ref)
    assert differ >= 75 and agree >= 75, (differ, agree)
    sk = ref["crossings"][:, 2] == D.SKIPPED
    assert sk.sum() == agree and (~sk).sum() == differ


@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_lipschitz_on_a_closed_mesh(prec):
    """(c) blob_scene(2)'s mesh, 300 pairs 1 % of the extent apart at the surface: |sd(a) - sd(b)| <= |a - b| + tol for every pair, tol twice the bound
    of csrc/spira_nearest.h (sdf_support.lipschitz_tol quotes the line).  A wrong sign breaks the property by about 2 |sd|."""
    ref = D.lipschitz_ref(prec)
    assert ref["valid"].all() and len(ref["points"]) == 2 * D.N_PAIRS
    ext = S.target_box(ref["scene"])[3]
    assert 0 < ref["tol"] < (1e-4 if prec == "f32" else 1e-12) * ext
    inside = ref["inside"] == 1
    straddle = inside[0::2] != inside[1::2]
    assert straddle.sum() >= 30 and inside.sum() >= 100 and (~inside).sum() >= 100
    bad = D.lipschitz_failures(ref["points"], ref["dist"], ref["tol"])
    assert len(bad) == 0, (bad[:8], ref["dist"][2 * bad[:8]], ref["dist"][2 * bad[:8] + 1])
    # the property has teeth: one wrong sign on a pair that lies on one side, more than half its gap from the surface, is a failure
    sd = np.abs(ref["dist"])
    gap = np.linalg.norm(ref["points"][0::2, :3] - ref["points"][1::2, :3], axis=1)
    deep = np.flatnonzero(~straddle & (2 * np.minimum(sd[0::2], sd[1::2]) > gap + ref["tol"]))
    assert len(deep) >= 10
    flipped = np.array(ref["dist"])
    flipped[2 * deep[0]] = -flipped[2 * deep[0]]
    assert list(D.lipschitz_failures(ref["points"], flipped, ref["tol"])) == [deep[0]]
