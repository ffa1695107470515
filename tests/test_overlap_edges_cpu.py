"""CPU: the box sets of tests/test_gpu_overlap_edges.py reach what they are for — asserted from the overlap yardstick alone (tests/overlap_support.py), in
both precisions and with fixed seeds, before any device is involved, so that no device case can pass on an empty premise.  Every assertion is a condition
on the inputs of the device tests, not a measurement; every count is printed.  The sets are built once per process (lru_cache) and left unchanged."""
import numpy as np
import pytest

import cast_support as S
import overlap_support as V

PRECS = ["f32", "f64"]


@pytest.mark.parametrize("how", ["create", "update", "rebuild"])
@pytest.mark.parametrize("fi", range(len(S.FRAMES)))
@pytest.mark.parametrize("prec", PRECS)
def test_frame_cases_hold_every_kind_of_box(prec, fi, how):
    """718 boxes about the blob mesh (320 triangles, 2 spheres) in the four placements, as built, updated and rebuilt: lists that overflow 16, that fill
    partly, that stay empty; invalid boxes; far boxes valid and invalid in turn, and at least one valid far box that touches something."""
    A, B, ss, ref = V.frame_case(prec, fi, how)
    assert len(ref["boxes"]) == 718 and ss.ns + len(ss.tri) == 322 and ss.frame is not None
    if how != "create":
        fa = S.mesh_frame(A["triangles10"], prec)
        assert (np.array_equal(ss.frame[0], fa[0]) and ss.frame[1] == fa[1]) == (how == "update")
    c = V.frame_conditions(ref)
    print(prec, fi, how, c)
    assert c["many"] >= 32 and c["none"] >= 48 and c["few"] >= 200 and c["some"] >= 100 and c["invalid"] >= 40 and c["far_touching"] >= 1
    whole = ref["parts"]["whole"]
    assert ref["cand"][whole][:, ss.ns:].all()                       # a containing box: every triangle
    for k in (4, 5, 16):
        lst = V.lists(ref, k)
        full = ref["count"] >= k
        assert (lst[full] >= 0).all() and (np.diff(lst[full], axis=1) > 0).all() and (lst[~ref["valid"]] == V.INVALID).all()


@pytest.mark.parametrize("prec", PRECS)
def test_deep_set(prec):
    ss, d = V.deep_set(prec)
    assert len(ss.tri) == 5120 and len(d["boxes"]) == 128 and d["valid"].all()
    whole, surf = d["parts"]["whole"], d["parts"]["surface"]
    assert d["cand"][whole][:, ss.ns:].all() and (d["count"][whole] >= 5120).all()
    first = np.flatnonzero(d["cand"][0])[:16]
    assert np.array_equal(V.lists(d, 16)[whole], np.tile(first, (8, 1))) and first[-1] <= 16
    c = d["count"][surf].astype(np.int64)
    print(prec, "surface boxes: none", int((c == 0).sum()), "1 .. 16", int(((c > 0) & (c <= 16)).sum()), "more", int((c > 16).sum()))
    assert ((c > 0) & (c <= 16)).sum() >= 64 and (c > 16).sum() >= 8
