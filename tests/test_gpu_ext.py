"""GPU (MI355X): the two extensions (SPIRA_EXT_DIELECTRIC, SPIRA_EXT_SPECTRAL) of the HIP path against their restatement in
the oracle — geometry bit for bit, images to the north-star tolerance, segment counts exact, wavefront == megakernel.
PARITY UNPINNED: no reference code exists for these features; excluded from every graded SPIRA_SEM_A run."""
import numpy as np
import pytest

from spira_hip import scenes
from test_gpu_parity import _args, _close, _counts, random_scene

pytestmark = pytest.mark.gpu


glass_scene = scenes.scene_s2_glass      # S2 with two glass spheres and a glass triangle


@pytest.mark.parametrize("prec", ["f32", "f64"])
@pytest.mark.parametrize("ext", ["dielectric", "spectral", "both"])
def test_ext_geometry_and_image_match_oracle(gpu, oracle, ext, prec):
    flags = {"dielectric": gpu.EXT_DIELECTRIC, "spectral": gpu.EXT_SPECTRAL, "both": gpu.EXT_DIELECTRIC | gpu.EXT_SPECTRAL}[ext] | gpu.POST_NONE
    s = glass_scene()
    ns, nm, nt = _counts(s)
    rng = np.random.default_rng(3)
    W, H, spp, depth, n = 200, 112, 6, 8, 2500
    ijs = np.stack([rng.integers(1, W + 1, n), rng.integers(1, H + 1, n), rng.integers(0, spp, n)], axis=1).astype(np.uint32)
    prims, ts, dirs, rad = gpu.trace_paths(*_args(s), gpu.make_params(W, H, spp, depth, ns, nm, nt, flags=flags, seed=4), ijs, prec)
    po = oracle.make_params(W, H, spp, depth, ns, nm, nt, flags=flags, seed=4)
    glass_hits = 0
    for k in range(n):
        cnt, oprims, ots, odirs, orad = oracle.trace_path(*_args(s), po, int(ijs[k, 0]), int(ijs[k, 1]), int(ijs[k, 2]), prec)
        oprims = np.where(np.arange(depth) < cnt, oprims, -2)
        assert np.array_equal(prims[k], oprims), (k, prims[k], oprims)
        assert np.array_equal(ts[k][:cnt].view(np.uint8), ots[:cnt].view(np.uint8)), (k, ts[k], ots)
        assert np.array_equal(dirs[k][:cnt].view(np.uint8), odirs[:cnt].view(np.uint8)), k
        assert np.allclose(rad[k], orad, rtol=1e-5, atol=1e-6), (k, rad[k], orad)
        glass_hits += int(np.isin(oprims[:cnt], [2, 3, 5]).sum())
    assert glass_hits > 300
    for kern in (gpu.KERNEL_WAVEFRONT, gpu.KERNEL_MEGA):
        hdr, _ = gpu.render(*_args(s), gpu.make_params(W, H, spp, depth, ns, nm, nt, flags=flags | kern, seed=4), prec)
        seg = gpu.counters()["segments"]
        if kern == gpu.KERNEL_WAVEFRONT:
            first = hdr
            ohdr, _, oseg = oracle.render(*_args(s), po, prec)
            assert _close(hdr, ohdr)[0] == 0 and seg == oseg
        else:
            assert np.array_equal(hdr, first) and seg == oseg


@pytest.mark.parametrize("prec", ["f64", "f32"])
def test_ext_bvh_mesh_and_tiling(gpu, oracle, prec):
    """A glass blob (1 280 triangles through the BVH) in spectral mode: oracle image, and an interleaved tiling reassembles bit for bit."""
    from spira_hip import distributed as D
    s = scenes.scene_s4(level=3)
    s["materials8"][2] = [0.9, 0.95, 1.0, 0, 0, 0, 0.0, -1.45]
    ns, nm, nt = _counts(s)
    flags = gpu.EXT_DIELECTRIC | gpu.EXT_SPECTRAL | gpu.POST_NONE
    W, H = 128, 72
    hdr, _ = gpu.render(*_args(s), gpu.make_params(W, H, 4, 10, ns, nm, nt, flags=flags, seed=6), prec)
    seg = gpu.counters()["segments"]
    ohdr, _, oseg = oracle.render(*_args(s), oracle.make_params(W, H, 4, 10, ns, nm, nt, flags=flags, seed=6), prec)
    assert _close(hdr, ohdr)[0] == 0 and seg == oseg
    tiles = [gpu.render(*_args(s), gpu.make_params(W, H, 4, 10, ns, nm, nt, flags=flags, seed=6, **D.tile_params(H, 3, r, 4)), prec)[0] for r in range(3)]
    mr = D.max_rows(H, 3, 4)
    padded = [np.concatenate([t, np.zeros((3, mr - t.shape[1], W), dtype=t.dtype)], axis=1) for t in tiles]
    assert np.array_equal(D.assemble(padded, H, 3, 4), hdr)


def test_ext_flags_are_rejected_where_not_built(gpu):
    s = scenes.scene_s1()
    for flags in (gpu.EXT_SPECTRAL | gpu.SEM_METAL, gpu.EXT_DIELECTRIC | gpu.SEM_CPU, gpu.EXT_SPECTRAL | gpu.KERNEL_BOUNCE):
        with pytest.raises(gpu.SpiraError, match="error -5"):
            gpu.render(s["spheres5"], s["materials8"], None, s["camera12"], gpu.make_params(32, 18, 1, 2, 5, 5, 0, flags=flags))


def test_ext_off_is_bit_identical_to_default(gpu):
    """The EXT instantiations with nothing to do (no negative roughness) against the default kernels."""
    s = scenes.scene_s2()
    ns, nm, nt = _counts(s)
    a, _ = gpu.render(*_args(s), gpu.make_params(160, 90, 5, 6, ns, nm, nt, seed=2), "f32")
    b, _ = gpu.render(*_args(s), gpu.make_params(160, 90, 5, 6, ns, nm, nt, flags=gpu.EXT_DIELECTRIC, seed=2), "f32")
    assert np.array_equal(a, b)


def test_ext_golden_fixture_on_gpu(gpu):
    """The committed extension fixture (oracle-generated regression pin) against the HIP path."""
    import json
    import os
    g = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "ext_s2glass_96x54_spp4_d8.json")))
    s = scenes.scene_s2()
    m = np.array(g["materials8"])
    for name in ("dielectric", "spectral", "both"):
        for prec in ("f64", "f32"):
            hdr, _ = gpu.render(s["spheres5"], m, s["triangles10"], s["camera12"],
                                gpu.make_params(96, 54, 4, 8, 5, 6, 1, flags=g[name]["flags"] | gpu.POST_NONE, seed=g["seed"]), prec)
            got = np.array([[hdr[c, y, x] for c in range(3)] for y, x in g["pixels"]], dtype=np.float64)
            want = np.array(g[name][prec]["values"])
            assert np.all(np.abs(got - want) <= 1e-6 + 1e-5 * np.abs(want)) and gpu.counters()["segments"] == g[name][prec]["segments"], (name, prec)
