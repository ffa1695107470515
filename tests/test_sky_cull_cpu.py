"""CPU: the all-sky classifier of the pixel-owning passes (csrc/spira_sky.h) without a device — the library exports it, the header
includes nothing of HIP, and tests/native/sky_cull.cpp holds the function against the sphere scan's own discriminant under ASan + UBSan: on the S1
camera at 1080p (where it must still classify at least 24 % of the pixels) and at 97x55, on 200 random cameras and sphere sets, and on the edge cases
(camera inside and on a sphere, a sphere behind the camera, radius 0, a radius-100 sphere grazing the frame, NaN and Inf)."""
import os
import subprocess

import numpy as np

from spira_hip import scenes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_library_exports_the_classifier(binding):
    lib = binding.lib()
    for name in ("spira_sky_pixel_f64", "spira_get_sky_pixels"):
        assert hasattr(lib, name) and name in binding.EXPORTS, name
    src = open(os.path.join(ROOT, "julia-spira_amd", "csrc", "spira_sky.h")).read()
    assert "#include <hip" not in src and "hip_runtime" not in src
    mk = open(os.path.join(ROOT, "julia-spira_amd", "csrc", "Makefile")).read()
    assert "spira_sky.h" in mk.split("DEPS", 1)[1].split("\n", 1)[0]      # hashed into spira_build_id


def test_exported_function_on_s1(binding):
    """The centre of the frame looks at the red sphere, the top row at the sky; a NULL pointer is an error code, not a crash."""
    s = scenes.scene_s1()
    cam, sph = s["camera12"], np.asarray(s["spheres5"], dtype=np.float64)
    assert binding.sky_pixel(cam, 1920, 1080, 960, 540, sph) == 0
    assert binding.sky_pixel(cam, 1920, 1080, 1, 1, sph) == 0            # the bottom row (j = 1) sees the ground
    assert binding.sky_pixel(cam, 1920, 1080, 3, 1080, sph) == 1          # the top row: sky
    assert binding.sky_pixel(cam, 1920, 1080, 3, 1080, sph[:0]) == 1      # no sphere at all
    assert binding.lib().spira_sky_pixel_f64(None, 4, 4, 1, 1, None, 0) < 0


def test_classifier_against_the_scan_under_asan_ubsan(binding, tmp_path):
    s = scenes.scene_s1()
    vals = list(np.asarray(s["camera12"], dtype=np.float64)) + list(np.asarray(s["spheres5"], dtype=np.float64).ravel())
    scene = tmp_path / "s1.txt"
    scene.write_text("\n".join(float(v).hex() for v in vals) + "\n")
    exe = str(tmp_path / "sky_cull")
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g", "-O1"]
    subprocess.run(["g++", "-std=c++17", "-ffp-contract=off", os.path.join(ROOT, "tests", "native", "sky_cull.cpp"), "-o", exe] + san, check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe, str(scene)], capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-6000:]
    assert "all checks passed" in r.stdout and "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr
