"""CPU: spira_scene_rebuild_* without a device — the library exports the four symbols and the header, the Python binding and the Julia shim name them, the
build arithmetic of spira_lbvh.h (the functions the kernels call) passes tests/native/lbvh_plan.cpp under ASan + UBSan against trees bvh_build made, the
kernels sit in the translation unit of their precision, and the argument errors that need no device come back as documented."""
import math
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["spira_scene_rebuild_f32", "spira_scene_rebuild_f64", "spira_scene_rebuild_device_f32", "spira_scene_rebuild_device_f64"]

# Surface-area cost of the rebuilt (Morton order) tree over bvh_build's (SAH) tree, per mesh: the value lbvh_plan.cpp measured (docs/experiments.md §24,
# the larger of the two precisions) plus 10 %.  The cap's job is to catch a broken collapse (a chain instead of a tree costs several times as much).
COST_MEASURED = {"icosphere": 1.0456, "soup": 1.1094, "tiny33": 1.2709, "copies200": 0.9805, "flatgrid": 1.0086}


def test_library_header_binding_and_julia_name_the_rebuild_entries(binding):
    lib = binding.lib()
    hdr = open(os.path.join(ROOT, "include", "spira_hip.h")).read()
    for name in NEW:
        assert hasattr(lib, name) and name in binding.EXPORTS and re.search(r"^int %s\(spira_scene \*scene, " % name, hdr, flags=re.M), name
    assert "#define SPIRA_ABI_VERSION 3 " in hdr and lib.spira_abi_version() == 3
    assert "ONCE PER LEVEL" in hdr and "bit for bit the render of a fresh handle" in hdr and "NO frame rule" in hdr
    assert hasattr(binding.Scene, "rebuild") and hasattr(binding.Scene, "rebuild_device")
    jl = open(os.path.join(ROOT, "julia-spira_amd", "julia", "SPIRA.jl")).read()
    assert "rebuild!" in re.search(r"^export (.*?)\n\n", jl, flags=re.S | re.M).group(1)
    for name in NEW:
        assert "ccall((:%s, libspira)" % name in jl, name


def test_rebuild_arithmetic_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "lbvh_plan")
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g", "-O1"]
    subprocess.run(["g++", "-std=c++17", "-ffp-contract=off", "-pthread", os.path.join(ROOT, "tests", "native", "lbvh_plan.cpp"), "-o", exe] + san, check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-6000:]
    assert "all checks passed" in r.stdout and "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr
    rows = re.findall(r"^(\w+) (f32|f64): (\d+) triangles, .* cost ratio ([-+.\w]+)$", r.stdout, flags=re.M)
    assert sorted((m, p) for m, p, _, _ in rows) == sorted((m, p) for m in COST_MEASURED for p in ("f32", "f64")), r.stdout
    for mesh, prec, _, ratio in rows:
        print(mesh, prec, ratio)
        assert math.isfinite(float(ratio)) and 0.0 < float(ratio) <= 1.10 * COST_MEASURED[mesh], (mesh, prec, ratio)


def test_rebuild_kernels_live_in_the_unit_of_their_precision():
    csrc = os.path.join(ROOT, "julia-spira_amd", "csrc")
    mk = open(os.path.join(csrc, "Makefile")).read()
    assert "spira_lbvh.h" in mk.split("DEPS", 1)[1].split("\n", 1)[0]      # hashed into spira_build_id
    objs = {n: os.path.join(csrc, "spira_tu_%s.o" % n) for n in ("main", "f32", "f64mesh")}
    if not all(os.path.exists(o) for o in objs.values()):
        pytest.skip("objects not present (library built elsewhere)")
    syms = {n: subprocess.run(["nm", o], capture_output=True, text=True, check=True).stdout for n, o in objs.items()}
    for kern in ("12k_lbvh_check", "11k_lbvh_keys", "13k_lbvh_commit"):
        assert len(re.findall(kern + "If", syms["f32"])) > 0 and len(re.findall(kern + "Id", syms["f32"])) == 0, kern
        assert len(re.findall(kern + "Id", syms["main"])) > 0 and len(re.findall(kern + "If", syms["main"])) == 0, kern
        assert len(re.findall(kern + "I[fd]", syms["f64mesh"])) == 0, kern
    for kern in ("k_lbvh_radix", "k_lbvh_boxes", "k_lbvh_make", "k_lbvh_scan", "k_lbvh_write"):      # nothing of these reads T: compiled once
        assert kern in syms["main"] and kern not in syms["f32"] and kern not in syms["f64mesh"], kern
    assert re.search(r" W _ZN8spira_tu4ImplIfE13scene_rebuildE", syms["f32"]) and re.search(r" U _ZN8spira_tu4ImplIfE13scene_rebuildE", syms["main"])
    assert re.search(r" T .*lbvh_topology", syms["main"]) and re.search(r" U .*lbvh_topology", syms["f32"]) and "lbvh_topology" not in syms["f64mesh"]


def test_rebuild_of_no_handle_is_refused_before_the_device(binding):
    lib = binding.lib()
    for name in NEW:
        fn = getattr(lib, name)
        assert (fn(None, None, None) if "device" in name else fn(None, None)) == -1
        assert b"scene handle is NULL or was destroyed" in lib.spira_last_error()
