"""CPU: the host twins of a handle's tree as a program that emits bytes (tests/native/tree_twin.h, tree_twin_dump.cpp) — what tests/test_gpu_tree_bytes.py
compares the device's trees with.  Here the program itself is put to the test, stand-alone under ASan + UBSan (host code only, nothing of it is loaded
into Python): one chain create -> update -> rebuild -> update on the 1 280-triangle icosphere, in both precisions (Float64 with screening records):
  (a) a clean sanitizer run, every step taken;
  (b) an update with the very array the tree was created from changes only what spira_refit.h lets a refit change: the program's own identity check
      (check_identity_bounds, the one of refit_plan.cpp: a grid step + the pad difference + one Float32 ulp) passes, and everything a refit keeps is
      byte-identical — summary, triangle records, screening records, imask / child_base / tri_base / rank / word 7, the holes;
  (c) the same job twice gives the same file, and so does the program built without the sanitizers (the build the GPU tests use)."""
import filecmp

import numpy as np
import pytest

import test_gpu_rebuild as RB          # deform(): the module's tests are marked gpu, its helpers are plain numpy
import tree_twin_support as TW


@pytest.fixture(scope="module")
def programs(tmp_path_factory):
    d = tmp_path_factory.mktemp("tree_twin")
    return d, TW.build_dump(d, sanitize=True), TW.build_dump(d)


def _nodes(step):
    return step.blobs["nodes"].view(np.uint32).reshape(-1, TW.NODE_DWORDS)


@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_twin_program_under_asan_ubsan(programs, prec):
    d, san, plain = programs
    A = TW.icosphere3()
    B = RB.deform(A)
    assert len(A) == 1280
    chain = [("create", A), ("update", A), ("rebuild", B), ("update", A)]
    screen = prec == "f64"
    steps, r, out = TW.run_dump(san, d, "chain_" + prec, prec, 3, screen, chain, env=TW.SAN_ENV)
    # (a)
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr and "CHECK failed" not in r.stderr, r.stderr[-4000:]
    assert [s.status for s in steps] == [0, 0, 0, 0]
    packet = 16 if prec == "f32" else 32
    for s in steps:
        sm = TW.summary(s.blobs["summary"])
        assert (sm.prec, sm.n) == (packet // 4, 1280) and sm.level_first[0] == 0 and sm.level_first[1] == 1 and sm.level_first[-1] == sm.n_slots
        assert len(s.blobs["nodes"]) == sm.n_slots * 80 and len(s.blobs["records"]) == (3 + 3 * 1280) * packet
        assert len(s.blobs["screen"]) == (3 * 1280 * 16 if screen else 0)
    # (b)
    assert "step 1: identity refit moves a child bound by at most" in r.stdout, r.stdout
    built, ident = steps[0], steps[1]
    assert np.array_equal(built.blobs["summary"], ident.blobs["summary"])
    assert np.array_equal(built.blobs["records"][2 * packet:], ident.blobs["records"][2 * packet:])          # all but the root box (frame packets 0 and 1)
    assert np.array_equal(built.blobs["screen"], ident.blobs["screen"])
    a, b = _nodes(built), _nodes(ident)
    assert np.array_equal(a[:, 3] >> 24, b[:, 3] >> 24) and np.array_equal(a[:, 4:8], b[:, 4:8])
    lo_x, hi_x = a[:, 8:10].copy().view(np.uint8).reshape(-1, 8), a[:, 14:16].copy().view(np.uint8).reshape(-1, 8)
    holes = np.all((lo_x == 255) & (hi_x == 0), axis=1)
    assert holes.any() and not holes.all() and np.array_equal(a[holes], b[holes])
    # a rebuild is a new tree, and the update after it keeps that tree's topology
    rebuilt, last = steps[2], steps[3]
    assert not np.array_equal(rebuilt.blobs["nodes"], built.blobs["nodes"])
    assert np.array_equal(rebuilt.blobs["summary"], last.blobs["summary"]) and np.array_equal(_nodes(rebuilt)[:, 4:8], _nodes(last)[:, 4:8])
    # (c)
    _, r2, out2 = TW.run_dump(san, d, "again_" + prec, prec, 3, screen, chain, env=TW.SAN_ENV)
    _, _, out3 = TW.run_dump(plain, d, "plain_" + prec, prec, 3, screen, chain)
    assert filecmp.cmp(out, out2, shallow=False) and filecmp.cmp(out, out3, shallow=False)
