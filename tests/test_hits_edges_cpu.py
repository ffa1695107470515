"""CPU: the ray sets of tests/test_gpu_hits_edges.py reach what they are for — asserted from the multi-hit yardstick alone (tests/hits_support.py), in
both precisions and with fixed seeds, before any device is involved, so that no device case can pass on an empty premise.  Every assertion is a
condition on the inputs of the device tests, not a measurement; every count is printed.  The sets are built once per process in hits_support.py
(lru_cache) and left unchanged; the device module uses the same ones."""
import numpy as np
import pytest

import cast_support as S
import hits_support as H

PRECS = ["f32", "f64"]


def _report(what, ref):
    tot = H.totals(ref)
    ties = {K: H.straddles(ref["cands"], K) for K in (1, 2, 3, 4, 5)}
    print(what, "rays", len(tot), "valid", int((tot >= 0).sum()), "most candidates", int(tot.max()), "rays with more than 4 / 8 / 16:",
          int((tot > 4).sum()), int((tot > 8).sum()), int((tot > 16).sum()), "bit-equal t at slots K-1 / K:", ties)
    return tot, ties


def test_shells_scene_keeps_its_bytes_and_takes_a_placement():
    a = H.shells_scene(1, n_shells=10)
    b = S.blob_scene(1)
    assert a["triangles10"].shape == (800, 10) and np.array_equal(a["triangles10"][:80], b["triangles10"]) and np.array_equal(a["spheres5"], b["spheres5"])
    scale, shift = S.FRAMES[3]
    m = H.shells_scene(1, n_shells=10, scale=scale, shift=shift)
    assert np.array_equal(m["triangles10"][:80], S.blob_scene(1, scale, shift)["triangles10"]) and np.array_equal(m["spheres5"], S.blob_scene(1, scale, shift)["spheres5"])
    assert np.array_equal(m["triangles10"][:, 9], a["triangles10"][:, 9])
    assert np.allclose(m["triangles10"][:, :9], a["triangles10"][:, :9] * scale + np.tile(shift, 3), rtol=0, atol=1e-12)


def test_straddles_counts_a_cut_between_equal_t():
    c = [None, [], [(1.0, 5)], [(1.0, 5), (1.0, 3), (2.0, 9)], [(1.0, 5), (2.0, 9), (2.0, 4)]]
    assert [H.straddles(c, K) for K in (1, 2, 3)] == [1, 1, 0]


@pytest.mark.parametrize("fi", range(len(S.FRAMES)))
@pytest.mark.parametrize("prec", PRECS)
def test_far_sets_hold_candidates_at_the_bound(oracle, prec, fi):
    """A list of K cut between two candidates of bit-equal t: the second is a candidate AT the bound (argument (d) of spira_hits.h), far from the mesh
    where a Float32 t has a large ulp and the walk's t0 is large."""
    ref = H.far_ref(prec, fi)
    tot, ties = _report("far %s frame %d:" % (prec, fi), ref)
    assert len(tot) == 2 * S.N_FAR + 6 * S.N_WIN == 896 and (tot >= 0).sum() == 640
    twins = np.arange(1, 2 * S.N_FAR, 2)
    assert (tot[twins] == -1).all() and (tot[twins - 1] >= 0).all() and (tot[2 * S.N_FAR:] >= 0).all()
    assert tot.max() <= 8 and (tot > 4).sum() >= 24
    assert ties[1] >= 6 and ties[2] >= 8 and ties[3] >= 3
    assert (tot == 0).sum() >= 8                                      # and rays whose whole list is unused slots


@pytest.mark.parametrize("fi", range(len(S.FRAMES)))
@pytest.mark.parametrize("prec", PRECS)
def test_shells_far_sets_fill_the_long_lists(oracle, prec, fi):
    ref = H.shells_far_ref(prec, fi)
    tot, _ = _report("shells-far %s frame %d:" % (prec, fi), ref)
    assert len(ref["sc"].tri) == 800 and len(tot) == 2 * H.N_SHELLS_FAR
    assert (tot[0::2] >= 0).all() and (tot[1::2] == -1).all()        # 96 of 96 valid, every twin invalid
    assert (tot > 16).sum() >= 48 and (tot > 8).sum() >= 72
    assert ((tot >= 0) & (tot < 5)).sum() >= 1                        # a scratch list that stays shorter than K


@pytest.mark.parametrize("prec", PRECS)
def test_axis_and_plane_rays_reach_five_candidates(oracle, prec):
    ref = H.axis_ref(prec)
    tot, _ = _report("axis + planes %s:" % prec, ref)
    assert len(tot) == S.N_AXIS + 48 == 240 and ref["valid"].all() and tot.max() >= 5 and (tot == 0).sum() >= 8


@pytest.mark.parametrize("prec", PRECS)
def test_quad_rays_tie_at_the_first_slots(oracle, prec):
    """A ray along a square's normal through the edge its halves share, or through a corner, meets two or more triangles at one t."""
    ref = H.quad_ref(prec)
    tot, ties = _report("quads + far axis rays %s:" % prec, ref)
    assert len(tot) == 2 * S.N_QUADS + S.N_AXIS == 792 and ref["valid"].all()
    if prec == "f32":
        assert ties[1] >= 30 and ties[2] >= 12


@pytest.mark.parametrize("prec", PRECS)
def test_duplicates_straddle_every_odd_list_length(oracle, prec):
    ref = H.dup_ref(prec)
    tot, ties = _report("dup %s (seed %d, %d rays):" % (prec, H.DUP_SEED, H.N_DUP), ref)
    assert ref["sc"].ns == 0 and len(ref["sc"].tri) == 2560 and ref["valid"].all() and np.array_equal(ref["pair"][ref["pair"]], np.arange(2560))
    assert H.pairs_hold(ref)
    for K in (1, 3, 5):
        assert ties[K] >= 8, (K, ties)                                # more than K candidates and a pair cut by K
    assert ties[2] == 0 and ties[4] == 0                              # (an even K falls between two pairs)
