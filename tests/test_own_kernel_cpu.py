"""CPU: which kernel renders a k_path pass (csrc/spira_plan.h, own_kernel_ok) without a device.  k_path_own holds a full pixel-owning
pass's facts as compile-time constants (csrc/spira_path_body.h, FIXED), so it is only right where the host launches it under exactly those facts:
tests/native/own_dispatch.cpp checks the predicate under ASan + UBSan — the headline pass, every condition switched off alone, the edges of k_eff,
n_spheres, max_depth and the LDS grant, and whole plans pass by pass (spp 64, 127, 128, 130) — and the library declares, exports and binds the count of
such passes beside spira_get_sky_pixels."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_predicate_and_plans_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "own_dispatch")
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g", "-O1"]
    subprocess.run(["g++", "-std=c++17", os.path.join(ROOT, "tests", "native", "own_dispatch.cpp"), "-o", exe] + san, check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-6000:]
    assert "all checks passed" in r.stdout and "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr


def test_export_is_declared_and_bound(binding):
    header = open(os.path.join(ROOT, "include", "spira_hip.h")).read()
    assert re.search(r"^int\s+spira_get_own_passes\(uint64_t \*out\);", header, re.M)
    assert "spira_get_own_passes" in binding.EXPORTS and callable(binding.own_passes)
    assert hasattr(binding.lib(), "spira_get_own_passes")
    assert binding.lib().spira_get_own_passes(None) < 0          # NULL is refused, with a message
    assert binding.lib().spira_last_error()
    assert binding.lib().spira_abi_version() == binding.ABI_VERSION == 3      # spira_counters keeps its layout: the count has an export of its own
    import ctypes
    assert ctypes.sizeof(binding.Counters) == 120


def test_the_library_holds_the_two_kernels_and_no_others(binding):
    """k_path_own<double, SPEC> for both SPEC and no Float32 or other instantiation, read from the built library as tests/test_abi_cpu.py reads k_path's
    (which unit a kernel is compiled in is that module's test: it sorts every host stub by its first template argument, and this one's is the precision)."""
    blob = open(binding.LIB_PATH, "rb").read()
    names = set(re.findall(rb"_ZN5spira10k_path_ownI[A-Za-z0-9_]*?EEvNS_8PathArgs", blob))
    assert names == {b"_ZN5spira10k_path_ownIdLb0EEEvNS_8PathArgs", b"_ZN5spira10k_path_ownIdLb1EEEvNS_8PathArgs"}, sorted(names)
