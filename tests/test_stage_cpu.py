"""CPU: the staging of a host-form list call without a device — stage_layout (spira_plan.h), the one place that decides where a call's arrays lie in the
context's staging buffer, passes tests/native/stage_plan.cpp under ASan + UBSan: every present/NULL combination of up to 8 blocks, sizes around the
alignment and at the entries' limits; a present block starts at a multiple of 16 bytes, order is kept, a NULL block has no room, nothing wraps.
stage_in (spira_hip.hip) calls it."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def stage_plan_exe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("stage") / "stage_plan")
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g", "-O1"]
    subprocess.run(["g++", "-std=c++17", os.path.join(ROOT, "tests", "native", "stage_plan.cpp"), "-o", exe] + san, check=True)
    return exe


def test_stage_layout_under_asan_ubsan(stage_plan_exe):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([stage_plan_exe], capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-6000:]
    for line in ("small tables checked", "large tables checked", "limits checked", "all checks passed"):
        assert line in r.stdout
    assert int(re.search(r"^(\d+) cases$", r.stdout, flags=re.M).group(1)) > 100000
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr


def test_stage_in_follows_the_layout():
    src = open(os.path.join(ROOT, "julia-spira_amd", "csrc", "spira_hip.hip")).read()
    assert "spira::stage_layout(" in src.split("int stage_in(", 1)[1].split("\n}\n", 1)[0]
