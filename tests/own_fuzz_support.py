"""The cases of tests/test_own_fuzz_cpu.py and tests/test_gpu_own_fuzz.py: sphere-only scenes and cameras for the pixel-owning passes (csrc/spira_path_body.h,
`own`; csrc/spira_sky.h; csrc/spira_plan.h, own_kernel_ok) — a seeded draw (draw_case) and a hand-made list (FIXED) — and what the host
can say of a case without a device: the passes the planner cuts it into, which of them k_path_own renders, the reach mask of every pixel of the tile
and the pixels the kernel must sum as all-sky runs.  Importing this needs neither a GPU nor the library; drawing and realising a case needs the binding
(camera_lookat, pixel_reach, sky_pixel: host arithmetic).  Every scene number goes through Float32, so it is exact in both precisions.

A case is a dict: kind, name, spheres5, materials8, cam (position, look_at, up, fov, aspect) and the camera12 made of it, W, H, spp, depth, batch_rays,
tile (the tiling fields of spira_params, {} for the whole frame), how (render: arrays; handle: a resident scene; accumulate: two calls of split[0] +
split[1] = spp samples into one sum), knob (the SPIRA_* knob this case also switches off alone) and seed.

Campaigns: SPIRA_FUZZ_OWN_SEED / SPIRA_FUZZ_OWN_ITERS (the defaults are what the suite runs), SPIRA_FUZZ_LOG (one flushed line per case before it runs)."""
import ctypes as C
import os

import numpy as np

from spira_hip import distributed as D
from test_gpu_parity import random_scene

DEFAULT_SEED, DEFAULT_ITERS = 20261021, 64
KINDS = ("few", "many", "full32", "over32", "tiny", "huge_in", "behind", "empty")
SHARES = (0.15, 0.15, 0.15, 0.13, 0.10, 0.10, 0.12, 0.10)                  # every kind at least 8 %
SPPS = (1, 2, 3, 5, 8, 16, 33, 63, 64, 65, 127, 128, 130)
SPP_SHARES = (0.0525, 0.0525, 0.0525, 0.0525, 0.0525, 0.10, 0.0525, 0.0525, 0.22, 0.0525, 0.10, 0.10, 0.06)      # the 64-slot passes are what the stack is built for
HOWS = ("render", "handle", "accumulate")
KNOBS = ("SPIRA_SKY_RUNS", "SPIRA_PIXEL_TABLE", "SPIRA_REACH_MASKS", "SPIRA_PRIVATE_L", "SPIRA_CAM_CONSTS")
MAX_PATHS = 350000                    # W H spp of the largest case: tests/test_gpu_own_kernel.py::test_oracle's 97 x 55 x 64
RUN = 4                               # SPIRA_RESOLVE_RUN: adjacent pixels of the tile's order that share a reach word and are summed as sky together
DEFAULT_BATCH = 160 << 20             # Knobs::batch_rays (csrc/spira_plan.h)


def _f32(a):
    return np.asarray(a, dtype=np.float32).astype(np.float64)


def seed():
    return int(os.environ.get("SPIRA_FUZZ_OWN_SEED", str(DEFAULT_SEED)))


def iters():
    return int(os.environ.get("SPIRA_FUZZ_OWN_ITERS", str(DEFAULT_ITERS)))


# ---------------------------------------------------------------------------------- cases
def realise(case, binding):
    """camera12 from the case's cam, as tests/test_gpu_pixel_table.py::_with_camera makes it; spheres5 given as a function of that camera is called."""
    c = dict(case)
    pos, look, up, fov, aspect = c["cam"]
    c["camera12"] = binding.camera_lookat(pos, look, up, fov, np.float32(aspect), prec="f32").astype(np.float64)
    if callable(c["spheres5"]):
        c["spheres5"] = c["spheres5"](c)
    c["spheres5"] = _f32(c["spheres5"]).reshape(-1, 5)
    c["materials8"] = _f32(c["materials8"])
    return c


def scene_of(case):
    return dict(spheres5=case["spheres5"], materials8=case["materials8"], triangles10=None, camera12=case["camera12"])


def _draw_spheres(rng, n, n_mats, r_lo=0.1, r_hi=0.7):
    """random_scene's spheres: centres uniform in [-3, 3]^3 + (0, 0, -4), any material."""
    sph = np.zeros((n, 5))
    sph[:, 0:3] = rng.uniform(-3, 3, (n, 3)) + [0, 0, -4]
    sph[:, 3] = rng.uniform(r_lo, r_hi, n)
    sph[:, 4] = rng.integers(1, n_mats + 1, n)
    return sph


def draw_case(rng, binding):
    kind = KINDS[int(rng.choice(len(KINDS), p=SHARES))]
    mats = random_scene(rng, 0, 0)["materials8"]           # its material draw: one emitter, metal and rough ones
    nm = len(mats)
    if kind == "few":
        sph = _draw_spheres(rng, int(rng.integers(1, 8)), nm)
    elif kind in ("many", "behind"):
        sph = _draw_spheres(rng, int(rng.integers(1 if kind == "behind" else 8, 32)), nm)
    elif kind == "full32":
        sph = _draw_spheres(rng, 32, nm)
    elif kind == "over32":
        sph = _draw_spheres(rng, int(rng.integers(33, 41)), nm)
    elif kind == "tiny":
        sph = _draw_spheres(rng, int(rng.integers(1, 32)), nm, 0.002, 0.03)      # sub-pixel at these frame sizes
    elif kind == "huge_in":
        sph = _draw_spheres(rng, int(rng.integers(2, 12)), nm)
        sph[int(rng.integers(0, len(sph))), 3] = 30.0      # contains the camera wherever both are drawn (they are at most 11 apart)
    else:
        sph = np.zeros((0, 5))
    pos = np.array([0, 0, 1.0]) + rng.uniform(-1, 1, 3)
    look = np.array([0, 0, -4.0]) + rng.uniform(-2, 2, 3)
    if kind == "behind":
        look = 2 * pos - look                              # turned away: every sphere lies behind the image plane
    up = np.array([rng.uniform(-0.5, 0.5), 1.0, rng.uniform(-0.5, 0.5)])
    fov = float(rng.uniform(8, 100))
    spp = int(SPPS[int(rng.choice(len(SPPS), p=SPP_SHARES))])
    while True:                                            # the size is drawn again, not the spp
        W, H = int(rng.integers(2, 97)), int(rng.integers(2, 61))
        if W * H * spp <= MAX_PATHS:
            break
    aspect = W / H if rng.random() < 0.8 else float(rng.uniform(0.5, 2.5))
    depth = int(rng.integers(1, 11))
    batch = int((0, 64 * W * H, 3 * W * H)[int(rng.choice(3, p=(0.3, 0.5, 0.2)))])
    tile = {}
    if rng.random() < 0.3:
        world = int(rng.integers(2, 5))
        tile = D.tile_params(H, world, int(rng.integers(0, world)), int(rng.integers(1, 9)))
        if tile["rows"] == 0:
            tile = {}
    how = HOWS[int(rng.choice(3, p=(0.4, 0.3, 0.3)))]
    split = None
    if how == "accumulate":
        if spp == 1:
            how = "render"
        else:
            n1 = 64 if spp > 64 and rng.random() < 0.5 else int(rng.integers(1, spp))
            split = (n1, spp - n1)
    knob = KNOBS[int(rng.integers(0, len(KNOBS)))]
    return realise(dict(kind=kind, name=kind, spheres5=sph, materials8=mats, cam=(_f32(pos), _f32(look), _f32(up), fov, aspect), W=W, H=H, spp=spp, depth=depth,
                        batch_rays=batch, tile=tile, how=how, split=split, knob=knob, seed=int(rng.integers(0, 2 ** 40))), binding)


def default_cases(binding, n=None, seed_=None):
    rng = np.random.default_rng(seed() if seed_ is None else seed_)
    return [draw_case(rng, binding) for _ in range(iters() if n is None else n)]


# ---- the hand-made list.  S1's spheres and materials (spira_hip/scenes.py, scene_s1; restated so that importing this needs no library —
# tests/test_own_fuzz_cpu.py holds them to it) and its camera.
S1_MATERIALS = [[0.7, 0.3, 0.3, 0, 0, 0, 0.0, 0.5], [0.5, 0.5, 0.5, 0, 0, 0, 0.0, 0.9], [0.8, 0.8, 0.8, 0, 0, 0, 1.0, 0.0], [0.8, 0.8, 1.0, 0, 0, 0, 0.9, 0.0],
                [1.0, 1.0, 1.0, 5, 5, 5, 0.0, 0.0]]
S1_SPHERES = [[0.0, 0.0, 0.0, 0.5, 1], [0.0, -100.5, 0.0, 100.0, 2], [1.0, 0.0, 0.0, 0.5, 3], [-1.0, 0.0, 0.0, 0.5, 4], [0.0, 5.0, 0.0, 1.0, 5]]
S1_CAM = ([0, 1, 3], [0, 0, 0], [0, 1, 0], 40.0)


def _sides(n, centre=None):
    """n - 1 small spheres in two columns at the left and right edges of a 16:9 frame seen from (0, 0, 3) at fov 40, S1's materials in turn, and the last
    sphere (index n - 1) alone in the middle of the frame, where the sky would be: with n = 32 its pixels' masks are exactly 1 << 31, with n > 32 it has no bit."""
    k = np.arange(n - 1)
    side = np.where(k % 2 == 0, -1.0, 1.0)
    sph = np.stack([side * (1.45 + 0.2 * ((k // 2) % 2)), -0.9 + 0.1 * (k // 2), np.zeros(n - 1), np.full(n - 1, 0.09), 1 + k % 5], axis=1)
    return np.concatenate([sph, [[0.0, 0.3, 0.0, 0.25, 1] if centre is None else centre]])


SIDES_CAM = ([0, 0, 3], [0, 0, 0], [0, 1, 0], 40.0)


def tile_rows(case):
    """Frame rows (0 is the top) of the tile, in its own order."""
    t = case["tile"]
    return D.rows_of_rank(case["H"], t["stripe_count"], t["stripe_rank"], t["stripe_h"]) if t else list(range(case["H"]))


def _corner_spheres(case):
    """Sub-pixel spheres (a 20th of a pixel across) on the lines of sight through pixel corners: where a run of the tile's order ends inside a row
    (pixel 4k + 3 | 4k + 4), at the last column's two edges (u = 1 and u = W / (W - 1)) and at the first column's."""
    cam, W, H = case["camera12"], case["W"], case["H"]
    org, llc, hor, ver = cam[0:3], cam[3:6], cam[6:9], cam[9:12]
    uv = []
    for p in range(RUN - 1, W * H - 1, RUN):
        y, x = divmod(p, W)
        if x + 1 < W and len(uv) < 20 and (p // RUN) % 3 == 0:
            uv.append(((x + 1) / (W - 1), (H - y) / (H - 1)))
    for y in (0, H // 2, H - 1):
        uv += [(1.0, (H - y) / (H - 1)), (W / (W - 1), (H - y - 1) / (H - 1)), (0.0, (H - y) / (H - 1))]
    sph = []
    for n, (u, v) in enumerate(uv):
        d = llc + hor * u + ver * v - org
        sph.append(list(org + d * (2.0 / np.linalg.norm(d))) + [0.004, 1 + n % 5])
    return np.array(sph)


def _fixed():
    out = []

    def add(name, spheres, cam, W, H, spp=64, depth=6, aspect=None, batch=0, tile=None, how="render", split=None, materials=S1_MATERIALS, kind="fixed"):
        n = len(out)
        out.append(dict(kind=kind, name=name, spheres5=spheres, materials8=materials, cam=tuple(cam) + (W / H if aspect is None else aspect,), W=W, H=H, spp=spp,
                        depth=depth, batch_rays=batch, tile=tile or {}, how=how, split=split, knob=KNOBS[n % len(KNOBS)], seed=1000 + n))

    s1 = S1_SPHERES
    # the camera exactly on a sphere's surface (|C| == r: at the origin, the sphere of radius 2 around (0, 0, -2)), looking along the tangent plane, and exactly at a centre
    add("camera_on_surface", [[0, 0, -2, 2, 3], [3, 0, 0.5, 0.5, 1], [3, 1, -0.5, 0.4, 5], [3, -0.5, 1.5, 0.3, 4]], ([0, 0, 0], [1, 0, 0], [0, 1, 0], 60.0), 45, 27)
    add("camera_at_centre", s1 + [[0, 1, 3, 1.5, 3]], S1_CAM, 31, 17, depth=4)
    add("coincident_spheres", s1 + [[0.0, 0.0, 0.0, 0.5, 3], [1.0, 0.0, 0.0, 0.5, 5]], S1_CAM, 45, 25, how="handle")
    add("radius_zero_and_negative", s1 + [[0.5, 0.6, 0.5, 0.0, 1], [-0.5, 0.6, 0.5, -0.25, 3]], S1_CAM, 45, 25)
    add("sphere31_alone", _sides(32), SIDES_CAM, 61, 34, depth=4, aspect=16 / 9)
    add("sphere31_alone_16spp", _sides(32), SIDES_CAM, 45, 26, spp=16, depth=4, aspect=16 / 9, how="handle")
    add("sphere35_alone", _sides(36), SIDES_CAM, 61, 34, depth=4, aspect=16 / 9)
    add("sphere35_alone_16spp", _sides(36, [0.3, -0.2, 0.0, 0.2, 5]), SIDES_CAM, 45, 26, spp=16, depth=4, aspect=16 / 9, how="accumulate", split=(5, 11))
    add("subpixel_at_corners", _corner_spheres, S1_CAM, 13, 7)
    add("subpixel_at_corners_tile", _corner_spheres, S1_CAM, 27, 15, spp=16, tile=D.tile_params(15, 2, 1, 2))
    # a radius-10 000 ground 100 (then 25) below the camera, 1 - r / |C| = 0.0099 (0.0025), the camera level and rolled by 4 degrees: only the lines of sight within
    # 8 (4) degrees of the horizon pass the ground by, so the band of sky runs crosses every row at another column
    add("ground_10000_rolled", [[0, -10000, 0, 10000, 2], [0, 130, -300, 40, 1], [150, 90, -400, 60, 3], [100, 400, -500, 150, 5]], ([0, 100, 0], [0, 100, -1], [0.07, 1, 0], 50.0),
        61, 33)
    add("ground_10000_rolled_tile", [[0, -10000, 0, 10000, 2], [0, 40, -120, 12, 1], [100, 200, -500, 150, 5]], ([0, 25, 0], [0, 25, -1], [-0.07, 1, 0], 30.0), 63, 36,
        tile=D.tile_params(36, 3, 2, 4))
    # S1 far from the origin and at other scales (powers of two: still exact in Float32)
    far = 2.0 ** 17
    add("s1_translated_2p17", [[x + far, y + far, z + far, r, m] for x, y, z, r, m in s1], ([far, 1 + far, 3 + far], [far, far, far], [0, 1, 0], 40.0), 45, 25)
    for e in (-12, 12):
        k = 2.0 ** e
        add("s1_scaled_2%s%d" % ("p" if e > 0 else "m", abs(e)), [[x * k, y * k, z * k, r * k, m] for x, y, z, r, m in s1], ([0, k, 3 * k], [0, 0, 0], [0, 1, 0], 40.0), 45, 25)
    for W, H in ((2, 2), (2, 60), (96, 2), (9, 5), (64, 16)):
        add("s1_%dx%d" % (W, H), s1, S1_CAM, W, H, how="handle" if W == 64 else "render")
    add("s1_fov_0.5", s1, ([0, 1, 3], [1, 0.5, 0], [0, 1, 0], 0.5), 33, 19)          # the upper edge of the metal sphere's outline
    add("s1_fov_170", s1, ([0, 1, 3], [0, 0, 0], [0, 1, 0], 170.0), 33, 19)
    add("s1_mismatched_aspect", s1, S1_CAM, 50, 50, spp=16, aspect=16 / 9)
    add("s1_depth_1", s1, S1_CAM, 41, 23, depth=1)
    add("s1_depth_129", s1, S1_CAM, 41, 23, depth=129)          # no carried key: slot-major L, k_path
    add("s1_depth_255", s1, S1_CAM, 16, 9, depth=255)
    add("s1_tile_stripes", s1, S1_CAM, 53, 30, tile=D.tile_params(30, 3, 1, 4), how="handle")
    add("s1_tile_single_rows", s1, S1_CAM, 53, 30, tile=D.tile_params(30, 4, 3, 1), how="accumulate", split=(40, 24))
    # passes of 64 slots and their neighbours on a scene of few spheres, on one of 32 and on one of 33: k_path_own renders 1, 1, 2, 0 / 0 passes
    for label, sph in (("s1", s1), ("sides32", _sides(32))):
        for spp in (64, 127, 128, 130):
            how, split = ("accumulate", (64, spp - 64)) if spp in (127, 128) and label == "s1" else ("render", None)
            add("%s_spp%d" % (label, spp), sph, S1_CAM if label == "s1" else SIDES_CAM, 37, 21, spp=spp, depth=5, batch=64 * 37 * 21, how=how, split=split)
    add("sides33_spp64", _sides(33), SIDES_CAM, 37, 21, depth=5, batch=64 * 37 * 21)
    add("empty_spp64", np.zeros((0, 5)), S1_CAM, 37, 21, depth=5, batch=64 * 37 * 21, kind="empty")
    return out


FIXED = _fixed()


# ---------------------------------------------------------------------------------- what the host says of a case
def pass_slots(case, spp=None):
    """Slots of every pass of a call of `spp` samples (make_plan, csrc/spira_plan.h): as many slots as the batch admits, then passes made equal."""
    spp = case["spp"] if spp is None else spp
    tp = len(tile_rows(case)) * case["W"]
    slots = min(max(1, (case["batch_rays"] or DEFAULT_BATCH) // tp), spp)
    n_pass = -(-spp // slots)
    slots = -(-spp // n_pass)
    return [min(slots, spp - p * slots) for p in range(-(-spp // slots))]


def pixel_owning(case, spp=None, prec="f64"):
    """Plan::fused with the default organisation and knobs: a Float64 scene of spheres alone at no more than 64 slots per pass."""
    return prec == "f64" and max(pass_slots(case, spp)) <= 64


def predicted_own_passes(case, spp=None, prec="f64"):
    """THE rule of which passes k_path_own renders (own_kernel_ok, csrc/spira_plan.h), with default knobs: a pixel-owning pass of exactly 64 slots (after the
    planner made the passes equal) of a Float64 scene of 1 .. 32 spheres, max_depth <= 128.  Everything else the predicate asks for follows from these in
    the cases drawn here (R = 2, the LDS for table, masks and camera packets granted, wave-private radiance blocks)."""
    if not pixel_owning(case, spp, prec) or not 1 <= len(case["spheres5"]) <= 32 or case["depth"] > 128:
        return 0
    return sum(1 for k in pass_slots(case, spp) if k == 64)


def calls(case):
    """(sample0, samples) of every call of the case: one, or the two of an accumulate case."""
    if case["how"] != "accumulate":
        return [(0, case["spp"])]
    n1, n2 = case["split"]
    return [(0, n1), (n1, n2)]


def reach_table(binding, case):
    """pixel_reach and sky_pixel (the library's host exports) of every pixel of the tile, in the tile's order: (masks uint32 [rows W], sky bool [rows W])."""
    lib = binding.lib()
    reach, sky = lib.spira_pixel_reach_f64, lib.spira_sky_pixel_f64
    reach.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p]
    sky.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint32]
    cam = np.ascontiguousarray(case["camera12"], dtype=np.float64)
    sph = np.ascontiguousarray(case["spheres5"], dtype=np.float64).reshape(-1, 5)
    cp, sp, n = cam.ctypes.data_as(C.c_void_p), sph.ctypes.data_as(C.c_void_p), len(sph)
    W, H = case["W"], case["H"]
    masks, skies = [], []
    word = C.c_uint32(0)
    for y in tile_rows(case):
        for x in range(W):
            rc = reach(cp, W, H, x + 1, H - y, sp, n, C.byref(word))
            s = sky(cp, W, H, x + 1, H - y, sp, n)
            assert rc == 0 and s in (0, 1), (rc, s)
            masks.append(word.value)
            skies.append(s == 1)
    return np.array(masks, dtype=np.uint32), np.array(skies, dtype=bool)


def sky_runs(sky):
    """Of the complete runs of 4 of the tile's pixel order: which are all sky."""
    return sky[: len(sky) // RUN * RUN].reshape(-1, RUN).all(axis=1)


def predicted_sky_pixels(case, sky, spp=None, prec="f64"):
    """What spira_get_sky_pixels reports after a call with default knobs: every pixel-owning pass sums the all-sky runs again (DESIGN.md §3,
    tests/test_gpu_sky_runs.py: passes x the host's count), other passes none."""
    return RUN * int(sky_runs(sky).sum()) * len(pass_slots(case, spp)) if pixel_owning(case, spp, prec) else 0


def log_line(it, case, prec="f64"):
    path = os.environ.get("SPIRA_FUZZ_LOG")
    if path:
        with open(path, "a") as fh:
            fh.write("own %s %s ns=%d %dx%d spp=%d depth=%d batch=%d tile=%s how=%s split=%s knob=%s seed=%d %s\n" % (
                it, case["name"], len(case["spheres5"]), case["W"], case["H"], case["spp"], case["depth"], case["batch_rays"], case["tile"], case["how"], case["split"],
                case["knob"], case["seed"], prec))
