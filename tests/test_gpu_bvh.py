"""GPU (MI355X): triangle meshes through the device BVH must return exactly what the reference's linear
closest-hit scan returns (examples/julia-raytracer.jl:213-258): bit-exact geometry against the oracle, which
scans every triangle like the reference does; images to the north-star tolerance; ties go to the later triangle."""
import numpy as np
import pytest

from spira_hip import scenes
from test_gpu_parity import RTOL, ATOL, _args, _close, _counts, random_scene

pytestmark = pytest.mark.gpu


def _trace_equal(gpu, oracle, s, prec, W=160, H=90, spp=4, depth=6, n=3000, seed=17, window=None):
    rng = np.random.default_rng(seed)
    ns, nm, nt = _counts(s)
    x0, x1, y0, y1 = window if window else (1, W + 1, 1, H + 1)      # 1-based pixel window the paths start in
    ijs = np.stack([rng.integers(x0, x1, n), rng.integers(y0, y1, n), rng.integers(0, spp, n)], axis=1).astype(np.uint32)
    prims, ts, dirs, rad = gpu.trace_paths(*_args(s), gpu.make_params(W, H, spp, depth, ns, nm, nt, seed=seed), ijs, prec)
    po = oracle.make_params(W, H, spp, depth, ns, nm, nt, seed=seed)
    tri_hits = 0
    for k in range(n):
        cnt, oprims, ots, odirs, orad = oracle.trace_path(*_args(s), po, int(ijs[k, 0]), int(ijs[k, 1]), int(ijs[k, 2]), prec)
        oprims = np.where(np.arange(depth) < cnt, oprims, -2)
        assert np.array_equal(prims[k], oprims), (k, prims[k], oprims)
        assert np.array_equal(ts[k][:cnt].view(np.uint8), ots[:cnt].view(np.uint8)), (k, ts[k], ots)
        assert np.array_equal(dirs[k][:cnt].view(np.uint8), odirs[:cnt].view(np.uint8)), k
        tri_hits += int((oprims >= ns).sum())
    return tri_hits


@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_bvh_geometry_bit_exact_blob(gpu, oracle, prec):
    s = scenes.scene_s4(level=3)          # 1280 triangles: the oracle scans them all per segment
    assert _trace_equal(gpu, oracle, s, prec, window=(68, 94, 34, 58)) > 300      # paths aimed at the mesh


@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_bvh_geometry_bit_exact_random_soup(gpu, oracle, prec):
    rng = np.random.default_rng(5)
    s = random_scene(rng, 12, 900, n_mats=7)     # intersecting, overlapping triangles + spheres
    assert _trace_equal(gpu, oracle, s, prec, n=2500) > 500


def test_bvh_ties_go_to_the_later_triangle(gpu, oracle):
    """Duplicate every triangle (same vertices, different material): t is identical, the scan keeps the LATER one."""
    rng = np.random.default_rng(9)
    s = random_scene(rng, 0, 200, n_mats=6)
    t = s["triangles10"]
    dup = t.copy()
    dup[:, 9] = (t[:, 9] % 6) + 1
    order = rng.permutation(400)
    both = np.concatenate([t, dup])[order]
    s["triangles10"] = both
    s["spheres5"] = np.zeros((0, 5))
    _trace_equal(gpu, oracle, s, "f32", n=2000)
    ns, nm, nt = _counts(s)
    hdr, _ = gpu.render(*_args(s), gpu.make_params(96, 54, 4, 4, ns, nm, nt, seed=3), "f32")
    ohdr, _, oseg = oracle.render(*_args(s), oracle.make_params(96, 54, 4, 4, ns, nm, nt, seed=3), "f32")
    assert _close(hdr, ohdr)[0] == 0 and gpu.counters()["segments"] == oseg


@pytest.mark.parametrize("kernel", ["wavefront", "mega"])
@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_bvh_image_matches_oracle(gpu, oracle, prec, kernel):
    s = scenes.scene_s4(level=4)          # 5120 triangles
    ns, nm, nt = _counts(s)
    kflag = gpu.KERNEL_MEGA if kernel == "mega" else gpu.KERNEL_WAVEFRONT
    hdr, _ = gpu.render(*_args(s), gpu.make_params(128, 72, 4, 5, ns, nm, nt, flags=kflag, seed=11), prec)
    ohdr, _, oseg = oracle.render(*_args(s), oracle.make_params(128, 72, 4, 5, ns, nm, nt, seed=11), prec)
    nbad, worst = _close(hdr, ohdr)
    assert nbad == 0, (nbad, worst)
    assert gpu.counters()["segments"] == oseg


def test_bvh_threshold_boundary_and_cache(gpu, oracle):
    """33 triangles take the BVH path, 32 the LDS scan: both must equal the oracle; changing the mesh between calls
    must rebuild the cached tree."""
    rng = np.random.default_rng(2)
    for nt_ in (32, 33, 34):
        s = random_scene(rng, 3, nt_)
        ns, nm, nt = _counts(s)
        hdr, _ = gpu.render(*_args(s), gpu.make_params(80, 45, 3, 4, ns, nm, nt, seed=1), "f32")
        ohdr, _, _ = oracle.render(*_args(s), oracle.make_params(80, 45, 3, 4, ns, nm, nt, seed=1), "f32")
        assert _close(hdr, ohdr)[0] == 0, nt_


def test_config5_full_size_tiling_and_bunny_sized_mesh(gpu):
    """BASELINE configs[4] shape: 81 920-triangle mesh + spheres, 1920x1080 depth 12 (spp reduced for test time):
    finite image, the 8-way stripe tiling reproduces the untiled checksum, mega == wavefront."""
    import zlib
    from spira_hip import distributed as D
    s = scenes.scene_s4(level=6)
    ns, nm, nt = _counts(s)
    W, H, spp, depth = 1920, 1080, 2, 12
    a, _ = gpu.render(*_args(s), gpu.make_params(W, H, spp, depth, ns, nm, nt, seed=scenes.seed_for(5)), "f32")
    assert np.isfinite(a).all() and a.min() >= 0
    c = gpu.counters()
    assert W * H * spp < c["segments"] <= W * H * spp * depth
    tiles = [gpu.render(*_args(s), gpu.make_params(W, H, spp, depth, ns, nm, nt, seed=scenes.seed_for(5), **D.tile_params(H, 8, r, 8)), "f32")[0]
             for r in range(8)]
    assert zlib.crc32(D.assemble(tiles, H, 8, 8).tobytes()) == zlib.crc32(a.tobytes())
    b, _ = gpu.render(*_args(s), gpu.make_params(W, H, spp, depth, ns, nm, nt, flags=gpu.KERNEL_MEGA, seed=scenes.seed_for(5)), "f32")
    assert np.array_equal(a, b)


def test_deferred_mesh_traversal_equals_in_place(gpu):
    """k_path parks rays that reach the mesh's bounding box and walks them in sessions (a parked ray is shaded a round or more later; packets
    carry their own stage).  SPIRA_DEFER_MESH=0 traverses in place: same pixels, same segments —
    with glass (extension) and without, depth 1 .. 12."""
    import os
    s = scenes.scene_s4(level=4)
    ns, nm, nt = _counts(s)
    glass = dict(s, materials8=s["materials8"].copy())
    glass["materials8"][2] = [0.9, 0.95, 1.0, 0, 0, 0, 0.0, -1.45]
    old = os.environ.get("SPIRA_DEFER_MESH")
    try:
        for scene, flags in ((s, 0), (glass, gpu.EXT_DIELECTRIC | gpu.EXT_SPECTRAL)):
            for depth in (1, 2, 5, 12):
                res = {}
                for d in ("1", "0"):
                    os.environ["SPIRA_DEFER_MESH"] = d
                    hdr, _ = gpu.render(*_args(scene), gpu.make_params(200, 113, 5, depth, ns, nm, nt, flags=flags | gpu.KERNEL_WAVEFRONT, seed=12, batch_rays=40000), "f32")
                    res[d] = (hdr, gpu.counters()["segments"])
                assert np.array_equal(res["1"][0], res["0"][0]) and res["1"][1] == res["0"][1], (flags, depth)
    finally:
        if old is None:
            os.environ.pop("SPIRA_DEFER_MESH", None)
        else:
            os.environ["SPIRA_DEFER_MESH"] = old


def _with_env(gpu, settings, fn):
    import os
    old = {k: os.environ.get(k) for k in settings}
    try:
        for k, v in settings.items():
            os.environ[k] = v
        return fn()
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_mesh_pass_organisations_and_session_knobs_agree_bitwise(gpu, prec):
    """A mesh pass runs as two launches (thin waves park the rays that reach the mesh's box, fat waves traverse them in refilled sessions and
    carry those paths on).  One launch with the sessions inside it, any number of fat waves, any refill threshold,
    sessions that wait for a batch or not: the same pixels and the same segment count, with and without the glass / spectral extension."""
    s = scenes.scene_s4(level=4)
    ns, nm, nt = _counts(s)
    glass = dict(s, materials8=s["materials8"].copy())
    glass["materials8"][2] = [0.9, 0.95, 1.0, 0, 0, 0, 0.0, -1.45]
    variants = [{}, {"SPIRA_MESH_TWO_PASS": "0"}, {"SPIRA_MESH_FAT_WAVES_PER_CU": "1"}, {"SPIRA_MESH_FAT_WAVES_PER_CU": "64"}, {"SPIRA_MESH_REFILL": "1"},
                {"SPIRA_MESH_REFILL": "64"}, {"SPIRA_MESH_MIN_BATCH": "1"}, {"SPIRA_MESH_MIN_BATCH": "100000", "SPIRA_MESH_TWO_PASS": "0"},
                {"SPIRA_BLOCKS_PER_CU": "3"}]
    for scene, flags in ((s, 0), (glass, gpu.EXT_DIELECTRIC | gpu.EXT_SPECTRAL)):
        for depth, batch in ((12, 0), (5, 30000)):
            p = gpu.make_params(240, 135, 6, depth, ns, nm, nt, flags=flags | gpu.KERNEL_WAVEFRONT, seed=21, batch_rays=batch)
            ref = None
            for v in variants:
                def run():
                    # (a leaf-size change needs a new tree: the context's cache is keyed by the triangle bytes only, so perturb nothing and use a handle)
                    with gpu.Scene(scene["spheres5"], scene["materials8"], scene["triangles10"], prec) as h:
                        hdr, _ = h.render(scene["camera12"], p)
                    return hdr, gpu.counters()["segments"], gpu.counters()["rays_parked"]
                got = _with_env(gpu, v, run)
                if ref is None:
                    ref = got
                assert np.array_equal(got[0], ref[0]) and got[1] == ref[1], (v, flags, depth)
                # the rays that reach the mesh's box wait on a list whatever the organisation (the roofline's bytes count them)
                assert 0 < got[2] <= got[1] and got[2] == ref[2], (v, got[2], ref[2])


def test_rays_parked_counter(gpu):
    """spira_counters.rays_parked: 0 where no ray ever waits on a mesh list (no mesh; traversal in place), the same number with and
    without the speculative division (a wave rendered again is counted once)."""
    s1 = scenes.scene_s1()
    gpu.render(*_args(s1), gpu.make_params(96, 54, 2, 4, *_counts(s1), seed=3), "f32")
    assert gpu.counters()["rays_parked"] == 0
    s = scenes.scene_s4(level=3)
    p = gpu.make_params(200, 120, 4, 8, *_counts(s), flags=gpu.KERNEL_WAVEFRONT, seed=4)
    seen = {}
    for env in ({}, {"SPIRA_SPEC_DIV": "0"}, {"SPIRA_SPEC_DIV": "2"}, {"SPIRA_DEFER_MESH": "0"}):
        for prec in ("f32", "f64"):
            def run():
                gpu.render(*_args(s), p, prec)
                return gpu.counters()["rays_parked"]
            seen[(tuple(env.items()), prec)] = _with_env(gpu, env, run)
    for prec in ("f32", "f64"):
        a, b, c, d = (seen[(tuple(e.items()), prec)] for e in ({}, {"SPIRA_SPEC_DIV": "0"}, {"SPIRA_SPEC_DIV": "2"}, {"SPIRA_DEFER_MESH": "0"}))
        assert a > 0 and a == b == c and d == 0, (prec, a, b, c, d)


@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_bvh_normalised_frame_any_scale_and_position(gpu, oracle, prec):
    """The tree's boxes live in the mesh's normalised frame (Float32 in both precisions): a mesh scaled by 1e-3 / 1e3 or moved far from the
    origin — with the camera moved along — must give the linear scan's geometry bit for bit, like the mesh of ordinary size at the origin."""
    base = scenes.scene_s4(level=3)
    for scale, shift in ((1.0, (0.0, 0.0, 0.0)), (1e-3, (0.0, 0.0, 0.0)), (1e3, (0.0, 0.0, 0.0)), (1.0, (300.0, -200.0, 150.0)), (0.05, (-40.0, 7.0, 90.0))):
        if prec == "f32" and (scale != 1.0 and shift != (0.0, 0.0, 0.0)):
            continue
        s = dict(base)
        sh = np.asarray(shift)
        t = base["triangles10"].copy()
        for v in range(3):
            t[:, 3 * v:3 * v + 3] = t[:, 3 * v:3 * v + 3] * scale + sh
        sp = base["spheres5"].copy()
        sp[:, :3] = sp[:, :3] * scale + sh
        sp[:, 3] *= scale
        cam = np.asarray(base["camera12"], dtype=np.float64).copy()
        cam[0:3] = cam[0:3] * scale + sh          # origin
        cam[3:6] = cam[3:6] * scale + sh          # lower-left corner (a point)
        cam[6:12] *= scale                        # horizontal, vertical (vectors)
        s.update(triangles10=t, spheres5=sp, camera12=cam)
        hits = _trace_equal(gpu, oracle, s, prec, n=1200, window=(68, 94, 34, 58))       # (asserts bit-equality path by path)
        # (at scale 1e-3 the reference's own absolute thresholds — |a| < 1e-8 in the triangle test, t_min = 0.001 — leave no triangle hit: oracle and GPU agree on that too)
        assert hits > 100 or scale < 0.01, (scale, shift, hits)


def test_bvh_far_camera_and_axis_parallel_rays(gpu, oracle):
    """Rays that start hundreds of mesh sizes away (the Float32 side of a ray starts where it enters the mesh's box) and rays parallel to an
    axis (1/d clamped) against a mesh of axis-aligned quads: bit-exact against the linear scan."""
    from cast_support import quad_scene
    s = quad_scene()                               # axis-aligned little squares at random places: many boxes of zero extent along one axis
    from spira_hip import _binding as B
    for pos, look in (([0.0, 0.0, 500.0], [0.0, 0.0, 0.0]), ([0.0, 0.0, 3.0], [0.0, 0.0, 0.0]), ([250.0, 0.0, 0.0], [0.0, 0.0, 0.0])):
        s["camera12"] = B.camera_lookat(pos, look, [0.0, 1.0, 0.0], 0.4 if max(map(abs, pos)) > 100 else 40.0, 16.0 / 9.0, 1.0, prec="f64")
        assert _trace_equal(gpu, oracle, s, "f64", W=161, H=91, n=1500) > 100, pos      # odd sizes: the centre pixel's ray is exactly axis-parallel


@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_depth_one_mesh_render_allocates_its_own_queues(gpu, oracle, prec):
    """max_depth = 1 on a mesh scene still sends the parked camera rays' hits through the hit queue.  With the device's workspaces freed first
    (spira_shutdown) the call must size the queues itself — it used to rely on what earlier calls had left (fuzz seed 4041, case 17: a depth-1
    render larger than every earlier one of its precision aborted the process)."""
    s = scenes.scene_s4(level=2)
    ns, nm, nt = _counts(s)
    gpu.lib().spira_shutdown()
    hdr, _ = gpu.render(*_args(s), gpu.make_params(62, 52, 7, 1, ns, nm, nt, flags=gpu.POST_NONE, seed=766849796527), prec)
    ohdr, _, oseg = oracle.render(*_args(s), oracle.make_params(62, 52, 7, 1, ns, nm, nt, flags=gpu.POST_NONE, seed=766849796527), prec)
    assert _close(hdr, ohdr)[0] == 0 and gpu.counters()["segments"] == oseg


def test_float32_triangle_screen_contract(tmp_path):
    """The Float32 screen of a Float64 walk (spira_device.h, tri_screen_f32; an experiment build, measured slower and not the default) must never
    reject a triangle the scan's own Float64 test accepts, and what it calls a certain hit must be one, within its distance bound:
    tests/native/tri_screen.hip over 2^28 adversarial ray / triangle pairs (edges, vertices, grazing rays, slivers, meshes far from the origin)."""
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "tri_screen")
    subprocess.run(["/opt/rocm/bin/hipcc", "-O3", "-std=c++17", "-ffp-contract=off", "--offload-arch=gfx950", "-I" + os.path.join(root, "include"),
                    "-o", exe, os.path.join(root, "tests", "native", "tri_screen.hip")], check=True, timeout=600)
    out = subprocess.run([exe, "1024", "1024", "20261005"], capture_output=True, text=True, timeout=300)
    print(out.stdout)
    assert out.returncode == 0 and "screened out 0;" in out.stdout and "of those wrong 0" in out.stdout, out.stdout + out.stderr


def test_screened_float64_walk_experiment_build():
    """`make screen` (csrc/Makefile): the library with the Float64 walk run on Float32 screens + batched exact tests.  Not the default (2 .. 6 % slower,
    DESIGN.md / docs/experiments.md) — but it must return exactly the linear scan's result like the default walk: the bit-exact mesh tests of this file
    (Float64) run on it in a child process."""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    csrc = os.path.join(root, "julia-spira_amd", "csrc")
    # built by __graft_entry__.build() and travelled with the snapshot; never compiled here (three translation units on a cold GPU box take minutes)
    assert subprocess.run(["make", "-q", "-C", csrc, "screen"]).returncode == 0, "libspira_hip_screen.so is missing or older than its sources: run __graft_entry__.build()"
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-x", "-q", "-m", "gpu", "-k",
                        "(bit_exact or image_matches or organisations_and_session_knobs or normalised_frame or far_camera or depth_one or deferred) and not experiment"], capture_output=True, text=True, timeout=900,
                       env=dict(os.environ, SPIRA_HIP_LIB=os.path.join(csrc, "libspira_hip_screen.so")), cwd=root)
    assert r.returncode == 0 and " passed" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
