"""GPU: what tests/test_gpu_overlap.py leaves open in spira_overlap.h, each against the scan of tests/overlap_support.py and always on the bytes of the
lists, the counts and the any form:
  * the four placements of cast_support.FRAMES, as built, after an update and after a rebuild — the walk prunes in Float32 in the tree's frame, the
    box's corners and axes come from the caller's units — with far boxes at 60 .. 64 frame units and their invalid twins;
  * the session at both ends of the refill threshold (SPIRA_CAST_REFILL 1 and 64) on box lists that split evenly over the plan's waves and that do not;
  * the 5 120-triangle tree under boxes that contain the whole mesh: every triangle is met, the list keeps the first 16.
Before every compared host-form call the staging is poisoned (test_gpu_overlap._poison).  tests/test_overlap_edges_cpu.py asserts without a device
that the sets reach what they are for."""
import numpy as np
import pytest

import cast_support as S
import nearest_support as N
import overlap_support as V
from test_gpu_overlap import _check, _open

pytestmark = pytest.mark.gpu

PRECS = ["f32", "f64"]


@pytest.mark.parametrize("how", ["create", "update", "rebuild"])
@pytest.mark.parametrize("fi", range(len(S.FRAMES)))
@pytest.mark.parametrize("prec", PRECS)
def test_frames_updates_and_rebuilds(gpu, prec, fi, how):
    A, B, ss, ref = V.frame_case(prec, fi, how)
    V.frame_conditions(ref)
    with _open(gpu, A, prec) as h:
        if how != "create":
            (h.update if how == "update" else h.rebuild)(triangles10=B["triangles10"])
        trips = _check(h, ref, ks=(0, 4, 5, 16))
    assert np.array_equal(trips[0], trips[1])                        # the same walk, whatever the organisation
    assert trips[0][ref["valid"]].min() >= 1 and not trips[0][~ref["valid"]].any()


@pytest.mark.parametrize("refill", [1, 64])
@pytest.mark.parametrize("n", [1000, 999])
@pytest.mark.parametrize("prec", PRECS)
def test_session_refills_at_both_ends_of_the_threshold(gpu, prec, n, refill):
    """k_overlap_session against its in-place twin and the scan on the smallest tree at the two ends of the walk loop's exit condition (SPIRA_CAST_REFILL 64:
    a refill only when the whole wave is free; 1: after every finished lane), with SPIRA_CAST_WAVES_PER_CU 1: 4 waves of about 250 boxes, every wave
    refills; 1 000 divides among them evenly (rem = 0), 999 leaves rem = 3."""
    from test_gpu_bvh import _with_env
    ref = V.reference("ico33", prec)
    pick = np.arange(n) * 37 % len(ref["boxes"])                     # boxes of every kind
    boxes = ref["boxes"][pick]

    def go():
        plan = gpu.cast_plan(n, 256)
        assert plan["refill_free"] == refill and plan["base"] > 64 and plan["base"] * plan["waves"] + plan["rem"] == n and (plan["rem"] != 0) == (n == 999), plan
        with _open(gpu, V.scene("ico33"), prec) as h:
            t_session, t_inplace = _check(h, ref, pick=pick, ks=(0, 4, 16))
            out = [(h.overlap_box(boxes, k), h.overlap_box(boxes, k, inplace=True)) for k in (4, 16)]
            return t_session, t_inplace, out, (h.overlap_any(boxes), h.overlap_any(boxes, inplace=True))
    t_session, t_inplace, out, (a_session, a_inplace) = _with_env(gpu, {"SPIRA_CAST_REFILL": str(refill), "SPIRA_CAST_WAVES_PER_CU": "1"}, go)
    for session, inplace in out:
        for a, b in zip(session[:2], inplace[:2]):                   # prim, count
            assert a.dtype == b.dtype and np.array_equal(a, b)
    assert np.array_equal(a_session, a_inplace)
    assert np.array_equal(t_session, t_inplace) and (t_session >= 2).sum() > n // 4          # lanes that walked


@pytest.mark.parametrize("prec", PRECS)
def test_whole_mesh_boxes_on_the_deep_tree(gpu, prec):
    """scene_s4(level=4)'s 5 120 triangles, one level deeper than the torus: a containing box prunes nothing — every triangle is met and counted, the list
    stops taking at 16 and holds the first 16 indices whatever the order of the visits — beside boxes at the surface that meet a few."""
    ss, ref = V.deep_set(prec)
    whole = ref["parts"]["whole"]
    assert ref["cand"][whole][:, ss.ns:].all() and (ref["count"][whole] >= 5120).all()
    first = np.flatnonzero(ref["cand"][0])[:16]
    assert np.array_equal(V.lists(ref, 16)[whole], np.tile(first, (8, 1)))
    with _open(gpu, N.scene("s4_4"), prec) as h:
        trips = _check(h, ref, ks=(1, 16))
    assert np.array_equal(trips[0], trips[1])
    assert (trips[0][whole] > len(ss.tri)).all()                     # a trip per triangle and the nodes above them
    assert trips[0][ref["parts"]["surface"]].max() < trips[0][whole].min()      # a box at the surface prunes
