"""CPU: spira_scene_update_* without a device — the library exports the four symbols and the header, the Python binding and the Julia shim name them, the
refit arithmetic of spira_refit.h (the functions the kernels call) passes tests/native/refit_plan.cpp under ASan + UBSan on trees bvh_build made, the
kernels sit in the translation unit of their precision, and the argument errors that need no device come back as documented."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["spira_scene_update_f32", "spira_scene_update_f64", "spira_scene_update_device_f32", "spira_scene_update_device_f64"]


def test_library_header_binding_and_julia_name_the_update_entries(binding):
    lib = binding.lib()
    hdr = open(os.path.join(ROOT, "include", "spira_hip.h")).read()
    for name in NEW:
        assert hasattr(lib, name) and name in binding.EXPORTS and re.search(r"^int %s\(spira_scene \*scene, " % name, hdr, flags=re.M), name
    assert "#define SPIRA_ABI_VERSION 3 " in hdr and lib.spira_abi_version() == 3
    assert "SYNCHRONISES `stream` ONCE" in hdr and "spira_scene_create_multi_* (whatever its n_devices): SPIRA_E_UNSUPPORTED" in hdr
    assert hasattr(binding.Scene, "update") and hasattr(binding.Scene, "update_device")
    jl = open(os.path.join(ROOT, "julia-spira_amd", "julia", "SPIRA.jl")).read()
    assert "update!" in re.search(r"^export (.*?)\n\n", jl, flags=re.S | re.M).group(1)
    assert "ccall((:spira_scene_update_f32, libspira)" in jl and "ccall((:spira_scene_update_device_f32, libspira)" in jl


def test_refit_arithmetic_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "refit_plan")
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g", "-O1"]
    subprocess.run(["g++", "-std=c++17", "-ffp-contract=off", "-pthread", os.path.join(ROOT, "tests", "native", "refit_plan.cpp"), "-o", exe] + san, check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-6000:]
    assert "all checks passed" in r.stdout and "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr
    # the vacuity guard's figures: every mesh and precision reported, and more than half of the triangles left their old leaf box
    rows = re.findall(r"(\d+) of (\d+) deformed triangles outside their old leaf box", r.stdout)
    assert len(rows) == 4 and all(2 * int(a) > int(b) for a, b in rows), r.stdout


def test_refit_kernels_live_in_the_unit_of_their_precision():
    csrc = os.path.join(ROOT, "julia-spira_amd", "csrc")
    objs = {n: os.path.join(csrc, "spira_tu_%s.o" % n) for n in ("main", "f32", "f64mesh")}
    if not all(os.path.exists(o) for o in objs.values()):
        pytest.skip("objects not present (library built elsewhere)")
    syms = {n: subprocess.run(["nm", o], capture_output=True, text=True, check=True).stdout for n, o in objs.items()}
    for kern in ("13k_refit_check", "12k_refit_tris", "13k_refit_level"):
        assert len(re.findall(kern + "If", syms["f32"])) > 0 and len(re.findall(kern + "Id", syms["f32"])) == 0, kern
        assert len(re.findall(kern + "Id", syms["main"])) > 0 and len(re.findall(kern + "If", syms["main"])) == 0, kern
        assert len(re.findall(kern + "I[fd]", syms["f64mesh"])) == 0, kern
    assert re.search(r" W _ZN8spira_tu4ImplIfE12scene_updateE", syms["f32"]) and re.search(r" U _ZN8spira_tu4ImplIfE12scene_updateE", syms["main"])
    mk = open(os.path.join(csrc, "Makefile")).read()
    assert "spira_refit.h" in mk.split("DEPS", 1)[1].split("\n", 1)[0]      # hashed into spira_build_id


def test_update_of_no_handle_is_refused_before_the_device(binding):
    lib = binding.lib()
    for name in NEW:
        fn = getattr(lib, name)
        assert (fn(None, None, None) if "device" in name else fn(None, None, None, None)) == -1
        assert b"scene handle is NULL or was destroyed" in lib.spira_last_error()
