"""CPU: the reach mask of the pixel-owning passes (csrc/spira_sky.h, pixel_reach) without a device — the library exports it, and
tests/native/reach_mask.cpp holds every clear bit against the sphere scan's own discriminant under ASan + UBSan: on the S1 camera at 1080p (where at
least 75 % of the (pixel, sphere) pairs must come out unreachable), at 97x55 and 9x5, on 200 random cameras and sphere sets, on the edge cases (camera
inside and on a sphere, a sphere behind the camera, radius <= 0, W or H below 2, 0 / 1 / 32 / 33 / 40 spheres), sky_pixel against the function it replaced
on all of them, and the two fields of the launch plan."""
import os
import subprocess

import numpy as np

from spira_hip import scenes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_exported_function_on_s1(binding):
    """Bit s = sphere s of S1 (red, ground, metal, glass-like, light).  The centre looks at the red sphere; the top row sees nothing; the bottom row the
    ground alone; the mask and spira_sky_pixel_f64 agree."""
    s = scenes.scene_s1()
    cam, sph = s["camera12"], np.asarray(s["spheres5"], dtype=np.float64)
    assert "spira_pixel_reach_f64" in binding.EXPORTS
    assert binding.pixel_reach(cam, 1920, 1080, 960, 540, sph) & 1
    assert binding.pixel_reach(cam, 1920, 1080, 3, 1080, sph) == 0 and binding.sky_pixel(cam, 1920, 1080, 3, 1080, sph) == 1
    assert binding.pixel_reach(cam, 1920, 1080, 1, 1, sph) == 2 and binding.sky_pixel(cam, 1920, 1080, 1, 1, sph) == 0
    assert binding.pixel_reach(cam, 1920, 1080, 3, 1080, sph[:0]) == 0
    assert binding.pixel_reach(cam, 1, 1080, 1, 7, sph) == 0xFFFFFFFF          # W below 2: every bit
    assert binding.lib().spira_pixel_reach_f64(None, 4, 4, 1, 1, None, 0, None) < 0
    for i, j in ((1, 1), (700, 500), (960, 540), (1300, 420), (1919, 1079), (960, 1000)):
        assert (binding.pixel_reach(cam, 1920, 1080, i, j, sph) == 0) == (binding.sky_pixel(cam, 1920, 1080, i, j, sph) == 1)


def test_mask_against_the_scan_under_asan_ubsan(binding, tmp_path):
    s = scenes.scene_s1()
    vals = list(np.asarray(s["camera12"], dtype=np.float64)) + list(np.asarray(s["spheres5"], dtype=np.float64).ravel())
    scene = tmp_path / "s1.txt"
    scene.write_text("\n".join(float(v).hex() for v in vals) + "\n")
    exe = str(tmp_path / "reach_mask")
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g", "-O1"]
    subprocess.run(["g++", "-std=c++17", "-ffp-contract=off", os.path.join(ROOT, "tests", "native", "reach_mask.cpp"), "-o", exe] + san, check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe, str(scene)], capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-6000:]
    assert "all checks passed" in r.stdout and "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr
