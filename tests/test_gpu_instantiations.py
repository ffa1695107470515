"""GPU (MI355X): every k_path instantiation the library holds (csrc/spira_device.h, k_path<T, R, BVH, EXT, SPEC, MODE, TRI>) rendered by a case
that reaches it, against the oracle and against the same scene through the default path.

KERNELS lists every instantiation by its template arguments: the case that makes the dispatch (csrc/spira_hip.hip, launch_path_mode /
launch_path_resume) pick it, or why no render can.  tests/test_abi_cpu.py::test_every_k_path_instantiation_has_a_case reads the names out of
libspira_hip.so and fails when the library holds one this table does not know.  Each reachable entry: image within the north-star tolerance
of the oracle, exact segment count, the same bits as the default path's render (and that as the megakernel's), and counters that show the entry's kernel did the rendering
(a default render launches the exact kernel behind every speculative one, and that launch renders nothing): one launch less per pass where
speculation is off, no second mesh launch where the pass is one launch, rays parked on the mesh lists where the traversal is deferred."""
import numpy as np
import pytest

from spira_hip import scenes
from test_gpu_parity import _args, _close, _counts
from test_gpu_specdiv import _Env

pytestmark = pytest.mark.gpu

EXT = 0x20000 | 0x40000      # SPIRA_EXT_DIELECTRIC | SPIRA_EXT_SPECTRAL (include/spira_hip.h)


def _spheres_glass():
    """The glass scene without its triangle: the extension instantiations without the LDS triangle scan."""
    s = scenes.scene_s2_glass()
    return dict(s, triangles10=None)


def _mesh():
    return scenes.scene_s4(level=3)          # 1 280 triangles: through the BVH


def _mesh_glass():
    s = scenes.scene_s4(level=3)
    s["materials8"] = s["materials8"].copy()
    s["materials8"][2] = [0.9, 0.95, 1.0, 0, 0, 0, 0.0, -1.45]
    return s


# scene name -> (scene, flags, (W, H, spp, depth)); the mesh sizes put the blob over a fifth of the frame
SCENES = {
    "s1": (scenes.scene_s1, 0, (160, 90, 6, 8)),
    "s2": (scenes.scene_s2, 0, (160, 90, 6, 8)),
    "glass": (scenes.scene_s2_glass, EXT, (160, 90, 6, 8)),
    "glass_spheres": (_spheres_glass, EXT, (160, 90, 6, 8)),
    "mesh": (_mesh, 0, (128, 72, 4, 8)),
    "mesh_glass": (_mesh_glass, EXT, (128, 72, 4, 10)),
}

# case name -> (scene name, environment knobs)
EXACT = {"SPIRA_SPEC_DIV": "0"}
ONE_LAUNCH = {"SPIRA_MESH_TWO_PASS": "0"}
IN_PLACE = {"SPIRA_DEFER_MESH": "0"}
CASES = {
    "s1": ("s1", {}),
    "s1_exact": ("s1", EXACT),
    "s2": ("s2", {}),
    "s2_exact": ("s2", EXACT),
    "s2_r1": ("s2", {"SPIRA_R": "1"}),
    "glass": ("glass", {}),
    "glass_exact": ("glass", EXACT),
    "glass_spheres": ("glass_spheres", {}),
    "glass_spheres_exact": ("glass_spheres", EXACT),
    "mesh": ("mesh", {}),
    "mesh_exact": ("mesh", EXACT),
    "mesh_one_launch": ("mesh", ONE_LAUNCH),
    "mesh_one_launch_exact": ("mesh", dict(ONE_LAUNCH, **EXACT)),
    "mesh_in_place": ("mesh", IN_PLACE),
    "mesh_in_place_exact": ("mesh", dict(IN_PLACE, **EXACT)),
    "mesh_glass": ("mesh_glass", {}),
    "mesh_glass_exact": ("mesh_glass", EXACT),
    "mesh_glass_one_launch": ("mesh_glass", ONE_LAUNCH),
    "mesh_glass_one_launch_exact": ("mesh_glass", dict(ONE_LAUNCH, **EXACT)),
    "mesh_glass_in_place_exact": ("mesh_glass", dict(IN_PLACE, **EXACT)),
    "mesh_r1": ("mesh", {"SPIRA_R": "1"}),
    "mesh_r1_one_launch": ("mesh", {"SPIRA_R": "1", **ONE_LAUNCH}),
    "mesh_r1_in_place": ("mesh", {"SPIRA_R": "1", **IN_PLACE}),
}

_BVH_TRI = ("unreachable: a scene drawn through the BVH has no LDS triangles (scene_pointers sets n_triangles = 0), and at R = 2 the dispatch "
            "picks TRI by n_triangles")

# (precision, R, BVH, EXT, SPEC, MODE, TRI) -> the cases that reach the instantiation, or why none can.  MODE: 0 one launch (sphere scenes; mesh
# scenes with SPIRA_MESH_TWO_PASS=0 / SPIRA_DEFER_MESH=0), 1 the parking launch of a mesh pass, 2 its second, fat-wave launch (always exact).
KERNELS = {}
for _p in ("f", "d"):
    KERNELS.update({
        (_p, 2, False, False, True, 0, False): ["s1"],
        (_p, 2, False, False, False, 0, False): ["s1_exact"],
        (_p, 2, False, False, True, 0, True): ["s2"],
        (_p, 2, False, False, False, 0, True): ["s2_exact"],
        (_p, 1, False, False, False, 0, True): ["s2_r1"],
        (_p, 2, False, True, True, 0, True): ["glass"],
        (_p, 2, False, True, False, 0, True): ["glass_exact"],
        (_p, 2, False, True, True, 0, False): ["glass_spheres"],
        (_p, 2, False, True, False, 0, False): ["glass_spheres_exact"],
        (_p, 2, True, False, True, 1, False): ["mesh"],
        (_p, 2, True, False, False, 1, False): ["mesh_exact"],
        (_p, 2, True, False, False, 2, False): ["mesh", "mesh_exact"],
        (_p, 2, True, False, True, 0, False): ["mesh_one_launch", "mesh_in_place"],
        (_p, 2, True, False, False, 0, False): ["mesh_one_launch_exact", "mesh_in_place_exact"],
        (_p, 2, True, True, True, 1, False): ["mesh_glass"],
        (_p, 2, True, True, False, 1, False): ["mesh_glass_exact"],
        (_p, 2, True, True, False, 2, False): ["mesh_glass", "mesh_glass_exact"],
        (_p, 2, True, True, True, 0, False): ["mesh_glass_one_launch"],
        (_p, 2, True, True, False, 0, False): ["mesh_glass_one_launch_exact", "mesh_glass_in_place_exact"],
        (_p, 1, True, False, False, 1, True): ["mesh_r1"],
        (_p, 1, True, False, False, 2, True): ["mesh_r1"],
        (_p, 1, True, False, False, 0, True): ["mesh_r1_one_launch", "mesh_r1_in_place"],
    })
    for _ext in (False, True):
        for _spec in (False, True):
            for _mode in (0, 1):
                KERNELS[(_p, 2, True, _ext, _spec, _mode, True)] = _BVH_TRI
        KERNELS[(_p, 2, True, _ext, False, 2, True)] = _BVH_TRI      # (launch_path_resume: the same test of n_triangles)

REACHABLE = sorted(k for k, v in KERNELS.items() if not isinstance(v, str))


def key_id(k):
    return "%s-R%d-%s-%s-%s-M%d-%s" % (k[0], k[1], "bvh" if k[2] else "nobvh", "ext" if k[3] else "noext", "spec" if k[4] else "exact", k[5],
                                      "tri" if k[6] else "notri")


def _plan(scene, env, prec):
    """What the dispatch does with this case, per pass: (speculative launch, two mesh launches, k_resolve launch, traversal deferred)."""
    name = SCENES[scene]
    mesh = scene.startswith("mesh")
    ext = name[1] != 0
    R = 2 if ext else int(env.get("SPIRA_R", "2"))
    spec = env.get("SPIRA_SPEC_DIV", "1") != "0" and R == 2
    defer = mesh and env.get("SPIRA_DEFER_MESH", "1") != "0"
    two_pass = defer and env.get("SPIRA_MESH_TWO_PASS", "1") != "0"
    fused = prec == "f64" and R == 2 and scene == "s1"       # (spira_hip.hip, `fused`: Float64 spheres alone, no extension, <= 64 slots)
    return spec, two_pass, not fused, defer


_memo = {}


def _render(gpu, scene, env, prec, kernel=0):
    key = (scene, tuple(sorted(env.items())), prec, kernel)
    if key not in _memo:
        make, flags, (W, H, spp, depth) = SCENES[scene]
        s = make()
        ns, nm, nt = _counts(s)
        with _Env(**env):
            hdr, _ = gpu.render(*_args(s), gpu.make_params(W, H, spp, depth, ns, nm, nt, flags=flags | kernel | gpu.POST_NONE, seed=29), prec)
            _memo[key] = (hdr, gpu.counters())
    return _memo[key]


def _oracle(oracle, scene, prec):
    key = ("oracle", scene, prec)
    if key not in _memo:
        make, flags, (W, H, spp, depth) = SCENES[scene]
        s = make()
        ns, nm, nt = _counts(s)
        ohdr, _, oseg = oracle.render(*_args(s), oracle.make_params(W, H, spp, depth, ns, nm, nt, flags=flags | 0x300, seed=29), prec)
        _memo[key] = (ohdr, oseg)
    return _memo[key]


def _check_case(gpu, oracle, case, prec):
    scene, env = CASES[case]
    hdr, c = _render(gpu, scene, env, prec)
    ohdr, oseg = _oracle(oracle, scene, prec)
    nbad, worst = _close(hdr, ohdr)
    assert nbad == 0, (case, prec, nbad, worst)
    assert c["segments"] == oseg, (case, prec, c["segments"], oseg)
    d_hdr, d = _render(gpu, scene, {}, prec)          # the default path
    assert np.array_equal(hdr, d_hdr), (case, prec, float(np.abs(hdr.astype(np.float64) - d_hdr).max()))
    # ... which is itself the megakernel's bits (k_mega: one lane per path, no k_path at all), so a change confined to the kernels a default render
    # uses cannot hide behind the comparison above (the oracle's tolerance, 1e-5, leaves room for a last-bit change)
    m_hdr, m = _render(gpu, scene, {}, prec, gpu.KERNEL_MEGA)
    assert np.array_equal(d_hdr, m_hdr) and m["segments"] == d["segments"], (case, prec, float(np.abs(m_hdr.astype(np.float64) - d_hdr).max()))
    assert c["segments"] == d["segments"] and c["passes"] == d["passes"] and c["redone_waves"] == 0, (case, prec)
    # the launches tell which kernels rendered: every difference to the default's count is one of the plan's launches per pass
    got, dflt = _plan(scene, env, prec), _plan(scene, {}, prec)
    per_pass = lambda pl: int(pl[0]) + 1 + int(pl[1]) + int(pl[2])
    assert c["launches"] - d["launches"] == c["passes"] * (per_pass(got) - per_pass(dflt)), (case, prec, c["launches"], d["launches"], got, dflt)
    if scene.startswith("mesh"):
        if got[3]:
            assert 0 < c["rays_parked"] == d["rays_parked"], (case, prec, c["rays_parked"], d["rays_parked"])
        else:
            assert c["rays_parked"] == 0, (case, prec, c["rays_parked"])      # traversal in place: nothing waits on a list
    else:
        assert c["rays_parked"] == 0


@pytest.mark.parametrize("key", REACHABLE, ids=key_id)
def test_instantiation_matches_oracle_and_default_path(gpu, oracle, key):
    prec = "f32" if key[0] == "f" else "f64"
    for case in KERNELS[key]:
        _check_case(gpu, oracle, case, prec)


@pytest.mark.parametrize("prec", ["f32", "f64"])
@pytest.mark.parametrize("scene", ["s2", "mesh"])
def test_waves_work_through_several_sub_chunks(gpu, oracle, scene, prec):
    """SPIRA_BLOCKS_PER_CU=1: 4 waves per CU for a pass of 614 400 rays, so every wave renders several sub-chunks (128 rays at R = 2, 64 at R = 1)
    one after another on the same LDS lists and queue regions.  Speculative, exact and R = 1 kernels: the same bits as the default grid, and the oracle."""
    make = {"s2": scenes.scene_s2, "mesh": _mesh}[scene]
    s = make()
    ns, nm, nt = _counts(s)
    W, H, spp, depth = 320, 240, 8, 8
    p = gpu.make_params(W, H, spp, depth, ns, nm, nt, flags=gpu.POST_NONE, seed=37)
    ref, _ = gpu.render(*_args(s), p, prec)
    c0 = gpu.counters()
    assert c0["passes"] == 1 and c0["samples"] == W * H * spp >= 600_000
    ohdr, _, oseg = oracle.render(*_args(s), oracle.make_params(W, H, spp, depth, ns, nm, nt, seed=37), prec)
    nbad, worst = _close(ref, ohdr)
    assert nbad == 0 and c0["segments"] == oseg, (nbad, worst, c0["segments"], oseg)
    for env in ({}, EXACT, {"SPIRA_R": "1"}, {"SPIRA_SPEC_DIV": "2"}) + ((ONE_LAUNCH, dict(ONE_LAUNCH, **EXACT)) if scene == "mesh" else ()):
        with _Env(SPIRA_BLOCKS_PER_CU=1, **env):
            hdr, _ = gpu.render(*_args(s), p, prec)
            c = gpu.counters()
        assert np.array_equal(hdr, ref) and c["segments"] == c0["segments"] and c["rays_parked"] == c0["rays_parked"], (env, prec)
        assert (c["redone_waves"] > 0) == (env.get("SPIRA_SPEC_DIV") == "2"), (env, c["redone_waves"])
