"""ctypes binding of libspira_hip.so (C ABI: include/spira_hip.h).

This is the same boundary the Julia shim (julia-spira_amd/julia/SPIRA.jl) binds with `ccall`.
There is no CPU fallback: if the HIP library is missing or no MI355X is visible, every render
call raises SpiraError.
"""
import ctypes as C
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.normpath(os.path.join(_HERE, "..", "csrc"))
LIB_PATH = os.environ.get("SPIRA_HIP_LIB", os.path.join(CSRC, "libspira_hip.so"))   # same override as julia/SPIRA.jl

ABI_VERSION = 3      # SPIRA_ABI_VERSION of the include/spira_hip.h this binding was written against (struct layouts, flag values)

# ---- flags (include/spira_hip.h) ----
SEM_A, SEM_CPU, SEM_METAL, SEM_HYBRID = 0x0, 0x1, 0x2, 0x3
KERNEL_DEFAULT, KERNEL_MEGA, KERNEL_BOUNCE, KERNEL_WAVEFRONT = 0x00, 0x10, 0x20, 0x30
POST_ACES, POST_ACES_GAMMA, POST_CLAMP_GAMMA, POST_NONE = 0x000, 0x100, 0x200, 0x300
ROWS_BOTTOM_UP = 0x1000
FLAG_PROFILE = 0x10000
EXT_DIELECTRIC, EXT_SPECTRAL = 0x20000, 0x40000
# ---- ray queries (spira_scene_cast_* / spira_scene_occluded_*) ----
MAX_RAYS = 1 << 26
RAY_MISS, RAY_INVALID = -1, -3
CAST_INPLACE = 0x1
# ---- multi-hit ray queries (spira_scene_cast_hits_*) ----
MAX_HITS = 16
HITS_COUNT_ALL = 0x2
# ---- K-nearest point queries (spira_scene_nearest_k_*) ----
MAX_NEAR = 16
NEAR_COUNT_ALL = 0x2
# ---- box overlap queries (spira_scene_overlap_box_* / spira_scene_overlap_any_*) ----
MAX_OVERLAP = 16
# ---- signed distance queries (spira_scene_signed_distance_*) ----
SDF_SKIPPED = 0xFFFFFFFF
# ---- camera models of the ray generator (spira_camera_rays_*) ----
CAM_PINHOLE, CAM_THIN_LENS, CAM_ORTHO = 0, 1, 2
MAX_DEPTH, MAX_SPP = 255, 1 << 24

EXPORTS = [
    "spira_abi_version", "spira_build_id", "spira_last_error", "spira_device_count", "spira_set_device", "spira_get_counters",
    "spira_get_sky_pixels", "spira_get_own_passes", "spira_sky_pixel_f64", "spira_pixel_reach_f64",
    "spira_shutdown", "spira_camera_lookat_f32", "spira_camera_lookat_f64", "spira_render_f32", "spira_render_f64",
    "spira_render_device_f32", "spira_render_device_f64", "spira_trace_paths_f32", "spira_trace_paths_f64",
    "spira_tonemap_f32", "spira_stripe_rows", "spira_accumulate_f32", "spira_accumulate_f64", "spira_accumulate_device_f32",
    "spira_accumulate_device_f64", "spira_scene_create_f32", "spira_scene_create_f64", "spira_scene_destroy",
    "spira_render_scene_f32", "spira_render_scene_f64", "spira_render_scene_device_f32", "spira_render_scene_device_f64",
    "spira_render_multi_f32", "spira_render_multi_f64", "spira_scene_create_multi_f32", "spira_scene_create_multi_f64",
    "spira_render_multi_scene_f32", "spira_render_multi_scene_f64",
    "spira_render_adaptive_f32", "spira_render_adaptive_f64", "spira_render_adaptive_scene_f32", "spira_render_adaptive_scene_f64",
    "spira_render_adaptive_scene_device_f32", "spira_render_adaptive_scene_device_f64", "spira_adaptive_converged_f32", "spira_adaptive_converged_f64",
    "spira_render_features_f32", "spira_render_features_f64", "spira_render_features_scene_f32", "spira_render_features_scene_f64",
    "spira_render_features_scene_device_f32", "spira_render_features_scene_device_f64",
    "spira_denoise_f32", "spira_denoise_f64", "spira_denoise_device_f32", "spira_denoise_device_f64",
    "spira_scene_update_f32", "spira_scene_update_f64", "spira_scene_update_device_f32", "spira_scene_update_device_f64",
    "spira_scene_rebuild_f32", "spira_scene_rebuild_f64", "spira_scene_rebuild_device_f32", "spira_scene_rebuild_device_f64",
    "spira_scene_cast_f32", "spira_scene_cast_f64", "spira_scene_cast_device_f32", "spira_scene_cast_device_f64",
    "spira_scene_occluded_f32", "spira_scene_occluded_f64", "spira_scene_occluded_device_f32", "spira_scene_occluded_device_f64",
    "spira_scene_radiance_f32", "spira_scene_radiance_f64", "spira_scene_radiance_device_f32", "spira_scene_radiance_device_f64",
    "spira_camera_rays_f32", "spira_camera_rays_f64", "spira_camera_rays_device_f32", "spira_camera_rays_device_f64",
    "spira_gather_rays_f32", "spira_gather_rays_f64", "spira_gather_rays_device_f32", "spira_gather_rays_device_f64",
    "spira_scene_gather_f32", "spira_scene_gather_f64", "spira_scene_gather_device_f32", "spira_scene_gather_device_f64",
    "spira_scene_gather_visible_f32", "spira_scene_gather_visible_f64", "spira_scene_gather_visible_device_f32", "spira_scene_gather_visible_device_f64",
    "spira_sh9_basis_f32", "spira_sh9_basis_f64", "spira_probe_rays_f32", "spira_probe_rays_f64", "spira_probe_rays_device_f32", "spira_probe_rays_device_f64",
    "spira_scene_probe_sh_f32", "spira_scene_probe_sh_f64", "spira_scene_probe_sh_device_f32", "spira_scene_probe_sh_device_f64",
    "spira_scene_closest_point_f32", "spira_scene_closest_point_f64", "spira_scene_closest_point_device_f32", "spira_scene_closest_point_device_f64",
    "spira_closest_point_triangle_f32", "spira_closest_point_triangle_f64",
    "spira_scene_cast_hits_f32", "spira_scene_cast_hits_f64", "spira_scene_cast_hits_device_f32", "spira_scene_cast_hits_device_f64",
    "spira_scene_nearest_k_f32", "spira_scene_nearest_k_f64", "spira_scene_nearest_k_device_f32", "spira_scene_nearest_k_device_f64",
    "spira_scene_sweep_f32", "spira_scene_sweep_f64", "spira_scene_sweep_device_f32", "spira_scene_sweep_device_f64",
    "spira_scene_sweep_blocked_f32", "spira_scene_sweep_blocked_f64", "spira_scene_sweep_blocked_device_f32", "spira_scene_sweep_blocked_device_f64",
    "spira_sweep_sphere_triangle_f32", "spira_sweep_sphere_triangle_f64",
    "spira_scene_overlap_box_f32", "spira_scene_overlap_box_f64", "spira_scene_overlap_box_device_f32", "spira_scene_overlap_box_device_f64",
    "spira_scene_overlap_any_f32", "spira_scene_overlap_any_f64", "spira_scene_overlap_any_device_f32", "spira_scene_overlap_any_device_f64",
    "spira_overlap_box_triangle_f32", "spira_overlap_box_triangle_f64", "spira_overlap_box_sphere_f32", "spira_overlap_box_sphere_f64",
    "spira_scene_overlap_tri_f32", "spira_scene_overlap_tri_f64", "spira_scene_overlap_tri_device_f32", "spira_scene_overlap_tri_device_f64",
    "spira_scene_overlap_tri_any_f32", "spira_scene_overlap_tri_any_f64", "spira_scene_overlap_tri_any_device_f32", "spira_scene_overlap_tri_any_device_f64",
    "spira_overlap_tri_triangle_f32", "spira_overlap_tri_triangle_f64", "spira_overlap_tri_sphere_f32", "spira_overlap_tri_sphere_f64",
    "spira_scene_signed_distance_f32", "spira_scene_signed_distance_f64", "spira_scene_signed_distance_device_f32", "spira_scene_signed_distance_device_f64",
]


class SpiraError(RuntimeError):
    pass


class Params(C.Structure):
    _fields_ = [("width", C.c_uint32), ("height", C.c_uint32), ("spp", C.c_uint32), ("max_depth", C.c_uint32),
                ("n_spheres", C.c_uint32), ("n_materials", C.c_uint32), ("n_triangles", C.c_uint32),
                ("flags", C.c_uint32), ("seed", C.c_uint64), ("row0", C.c_uint32), ("rows", C.c_uint32),
                ("stripe_h", C.c_uint32), ("stripe_count", C.c_uint32), ("stripe_rank", C.c_uint32),
                ("batch_rays", C.c_uint32)]


class Counters(C.Structure):
    _fields_ = [("samples", C.c_uint64), ("segments", C.c_uint64), ("rays_enqueued", C.c_uint64),
                ("radiance_rmw", C.c_uint64), ("radiance_stores", C.c_uint64), ("passes", C.c_uint64), ("launches", C.c_uint64),
                ("kernel_ms", C.c_double), ("bounce_kernel_ms", C.c_double), ("bounce_launches", C.c_uint64), ("redone_waves", C.c_uint64), ("rays_parked", C.c_uint64),
                ("mesh_wave_trips", C.c_uint64), ("mesh_lane_trips", C.c_uint64), ("walk_kernel_ms", C.c_double)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class Adaptive(C.Structure):
    """spira_adaptive: the schedule of an adaptive render (params.spp is the cap)."""
    _fields_ = [("min_spp", C.c_uint32), ("batch_spp", C.c_uint32), ("tolerance", C.c_double), ("floor", C.c_double)]


class Denoise(C.Structure):
    """spira_denoise: the frame size and the settings of a denoise call."""
    _fields_ = [("width", C.c_uint32), ("height", C.c_uint32), ("iterations", C.c_uint32), ("post", C.c_uint32),
                ("sigma_l", C.c_double), ("sigma_z", C.c_double)]


class Radiance(C.Structure):
    """spira_radiance: the samples, depth, seed and pixel keys of a radiance call on a ray list."""
    _fields_ = [("spp", C.c_uint32), ("max_depth", C.c_uint32), ("flags", C.c_uint32), ("sample0", C.c_uint32),
                ("seed", C.c_uint64), ("key0", C.c_uint32), ("reserved", C.c_uint32)]


class Lens(C.Structure):
    """spira_lens: camera model, image size, sample, seed and row range of a generated ray list."""
    _fields_ = [("model", C.c_uint32), ("width", C.c_uint32), ("height", C.c_uint32), ("sample", C.c_uint32),
                ("seed", C.c_uint64), ("row0", C.c_uint32), ("rows", C.c_uint32), ("lens_radius", C.c_double)]


class GatherVisible(C.Structure):
    """spira_gather_visible: the samples, seed, pixel keys and distance range of a visibility gather on a point list."""
    _fields_ = [("spp", C.c_uint32), ("sample0", C.c_uint32), ("seed", C.c_uint64), ("key0", C.c_uint32), ("flags", C.c_uint32),
                ("t_min", C.c_double), ("t_max", C.c_double)]


_lib = None


def build_library():
    """hipcc --offload-arch=gfx950 build of csrc/ (cross-compiles without a GPU)."""
    subprocess.run(["make", "-C", CSRC, "-s"], check=True)


def lib():
    """Load libspira_hip.so; raises SpiraError when it has not been built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise SpiraError("libspira_hip.so is not built (%s); run __graft_entry__.build() / make -C %s" % (LIB_PATH, CSRC))
        try:
            import torch  # noqa: F401  (load torch's HIP runtime first so both share one libamdhip64.so.7)
        except Exception:
            pass
        _lib = C.CDLL(LIB_PATH)
        _lib.spira_last_error.restype = C.c_char_p
        _lib.spira_build_id.restype = C.c_char_p
        _lib.spira_stripe_rows.restype = C.c_uint32
        _lib.spira_stripe_rows.argtypes = [C.c_uint32] * 4
        for name in EXPORTS:
            getattr(_lib, name)  # AttributeError if an ABI symbol is missing
        have = _lib.spira_abi_version()
        if have != ABI_VERSION:      # a stale library (SPIRA_HIP_LIB, an old build directory): other struct sizes and flag values
            _lib = None
            raise SpiraError("%s has ABI version %d, this binding was written for %d" % (LIB_PATH, have, ABI_VERSION))
    return _lib


def build_id():
    """Hash of the kernel sources the loaded library was built from (csrc/Makefile); bench.py attaches PMC figures of exactly these sources."""
    return lib().spira_build_id().decode()


def _check(rc):
    if rc != 0:
        raise SpiraError("libspira_hip error %d: %s" % (rc, lib().spira_last_error().decode()))


def _dt(prec):
    if prec == "f32":
        return np.float32, C.c_float
    if prec == "f64":
        return np.float64, C.c_double
    raise ValueError("prec must be 'f32' or 'f64'")


def _arr(a, dtype):
    if a is None:
        return None, None
    a = np.ascontiguousarray(a, dtype=dtype)
    return a, a.ctypes.data_as(C.c_void_p)


def make_params(width, height, spp, max_depth, n_spheres, n_materials, n_triangles=0, flags=0, seed=0, row0=0, rows=0,
                stripe_h=0, stripe_count=0, stripe_rank=0, batch_rays=0):
    return Params(width, height, spp, max_depth, n_spheres, n_materials, n_triangles, flags, seed, row0, rows,
                  stripe_h, stripe_count, stripe_rank, batch_rays)


def device_count():
    return lib().spira_device_count()


def set_device(d):
    _check(lib().spira_set_device(C.c_int(d)))


def counters():
    c = Counters()
    _check(lib().spira_get_counters(C.byref(c)))
    d = c.as_dict()
    sky = C.c_uint64(0)
    _check(lib().spira_get_sky_pixels(C.byref(sky)))
    d["sky_pixels"] = sky.value
    return d


def own_passes():
    """spira_get_own_passes: passes of the last render that k_path_own rendered (0 with SPIRA_OWN_KERNEL=0 and wherever every pass ran k_path)."""
    n = C.c_uint64(0)
    _check(lib().spira_get_own_passes(C.byref(n)))
    return n.value


def sky_pixel(camera12, width, height, i, j, spheres5):
    """spira_sky_pixel_f64: 1 when no camera ray of pixel (i, j) (1-based reference indices) can meet a sphere, else 0 — the library's host arithmetic."""
    cam = np.ascontiguousarray(camera12, dtype=np.float64)
    sp = np.ascontiguousarray(spheres5, dtype=np.float64).reshape(-1, 5)
    assert cam.shape == (12,)
    fn = lib().spira_sky_pixel_f64
    fn.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint32]
    rc = fn(cam.ctypes.data_as(C.c_void_p), width, height, i, j, sp.ctypes.data_as(C.c_void_p), len(sp))
    if rc < 0:
        _check(rc)
    return rc


def pixel_reach(camera12, width, height, i, j, spheres5):
    """spira_pixel_reach_f64: bit s clear = no camera ray of pixel (i, j) can meet sphere s (s < 32) — the library's host arithmetic."""
    cam = np.ascontiguousarray(camera12, dtype=np.float64)
    sp = np.ascontiguousarray(spheres5, dtype=np.float64).reshape(-1, 5)
    assert cam.shape == (12,)
    fn = lib().spira_pixel_reach_f64
    fn.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p]
    mask = C.c_uint32(0)
    _check(fn(cam.ctypes.data_as(C.c_void_p), width, height, i, j, sp.ctypes.data_as(C.c_void_p), len(sp), C.byref(mask)))
    return mask.value


def stripe_rows(height, stripe_h, stripe_count, stripe_rank):
    return lib().spira_stripe_rows(height, stripe_h, stripe_count, stripe_rank)


def camera_lookat(position, look_at, up, fov_deg, aspect_ratio, focus_dist=1.0, prec="f32"):
    npdt, cdt = _dt(prec)
    p, pp = _arr(position, npdt)
    l, lp = _arr(look_at, npdt)
    u, up_ = _arr(up, npdt)
    out = np.zeros(12, dtype=npdt)
    if prec == "f32":
        _check(lib().spira_camera_lookat_f32(pp, lp, up_, cdt(fov_deg), cdt(aspect_ratio), out.ctypes.data_as(C.c_void_p)))
    else:
        _check(lib().spira_camera_lookat_f64(pp, lp, up_, cdt(fov_deg), cdt(aspect_ratio), cdt(focus_dist),
                                             out.ctypes.data_as(C.c_void_p)))
    return out


def render(spheres5, materials8, triangles10, camera12, params, prec="f32", want_hdr=True, want_img=False):
    """Host-pointer render.  Returns (hdr, img): arrays [3, rows, width] or None."""
    npdt, _ = _dt(prec)
    s, sp = _arr(spheres5, npdt)
    m, mp = _arr(materials8, npdt)
    t, tp = _arr(triangles10, npdt)
    c, cp = _arr(camera12, npdt)
    rows = params.rows if params.rows else params.height
    hdr = np.empty((3, rows, params.width), dtype=npdt) if want_hdr else None
    img = np.empty((3, rows, params.width), dtype=npdt) if want_img else None
    fn = lib().spira_render_f32 if prec == "f32" else lib().spira_render_f64
    _check(fn(sp, mp, tp, cp, C.byref(params), hdr.ctypes.data_as(C.c_void_p) if want_hdr else None,
              img.ctypes.data_as(C.c_void_p) if want_img else None))
    return hdr, img


def render_device(spheres5, materials8, triangles10, camera12, params, d_hdr_ptr, d_img_ptr, stream_ptr, prec="f32"):
    """Asynchronous render into DEVICE buffers (integer addresses, e.g. torch.Tensor.data_ptr())."""
    npdt, _ = _dt(prec)
    s, sp = _arr(spheres5, npdt)
    m, mp = _arr(materials8, npdt)
    t, tp = _arr(triangles10, npdt)
    c, cp = _arr(camera12, npdt)
    fn = lib().spira_render_device_f32 if prec == "f32" else lib().spira_render_device_f64
    _check(fn(sp, mp, tp, cp, C.byref(params), C.c_void_p(d_hdr_ptr or None), C.c_void_p(d_img_ptr or None),
              C.c_void_p(stream_ptr or None)))


def render_multi(spheres5, materials8, triangles10, camera12, params, n_devices, prec="f32", want_hdr=True, want_img=False):
    """spira_render_multi_*: the frame on n_devices GPUs of this node (stripes + one RCCL gather to device 0), host outputs."""
    npdt, _ = _dt(prec)
    s, sp = _arr(spheres5, npdt)
    m, mp = _arr(materials8, npdt)
    t, tp = _arr(triangles10, npdt)
    c, cp = _arr(camera12, npdt)
    hdr = np.empty((3, params.height, params.width), dtype=npdt) if want_hdr else None
    img = np.empty((3, params.height, params.width), dtype=npdt) if want_img else None
    fn = lib().spira_render_multi_f32 if prec == "f32" else lib().spira_render_multi_f64
    _check(fn(sp, mp, tp, cp, C.byref(params), C.c_int(n_devices), hdr.ctypes.data_as(C.c_void_p) if want_hdr else None,
              img.ctypes.data_as(C.c_void_p) if want_img else None))
    return hdr, img


class _SceneProbes:
    """The light-probe entries of a scene handle (csrc/spira_probe.h): Scene inherits them.  They use the handle's `prec`, `_list` and `_query`."""

    def probe_sh(self, points3, spp, max_depth, seed=0, sample0=0, key0=0, flags=0, sums=None, want_valid=False):
        """spira_scene_probe_sh_*: path-traced radiance over the whole sphere of every point of points3 (n x [px py pz], host array; the library draws the
        uniform directions itself, point k under pixel key key0 + k), projected onto the nine real spherical harmonics of bands 0 .. 2.  ADDS samples
        sample0 .. sample0 + spp - 1, in order, to sums ([n, 9, 3], in place; None: a fresh zero array); the SH coefficients of the radiance are
        4 pi * sums / spp.  Returns sums, or (sums, valid uint8 [n]) with want_valid."""
        npdt, _ = _dt(self.prec)
        p = self._list(points3, 3, "points3: n_points x [px py pz]")
        n = len(p)
        if sums is None:
            sums = np.zeros((n, 9, 3), dtype=npdt)
        if sums.dtype != npdt or not sums.flags["C_CONTIGUOUS"] or sums.shape != (n, 9, 3):
            raise ValueError("sums: a contiguous [n_points, 9, 3] array of the handle's precision")
        valid = np.empty(n, dtype=np.uint8) if want_valid else None
        rp = Radiance(spp, max_depth, flags, sample0, seed, key0, 0)
        self._query("probe_sh", False, (p,), (n,), C.byref(rp), (sums, valid))
        return (sums, valid) if want_valid else sums

    def probe_sh_device(self, d_points_ptr, n_points, spp, max_depth, d_sums_ptr, seed=0, sample0=0, key0=0, flags=0, d_valid_ptr=0, stream_ptr=0):
        """spira_scene_probe_sh_device_*: DEVICE addresses (d_valid_ptr 0 / None: not wanted), asynchronous on the stream; the sums are added to in place."""
        rp = Radiance(spp, max_depth, flags, sample0, seed, key0, 0)
        self._query("probe_sh", True, (d_points_ptr,), (n_points,), C.byref(rp), (d_sums_ptr, d_valid_ptr, stream_ptr))


class _SceneTriOverlap:
    """The triangle overlap entries of a scene handle (csrc/spira_trioverlap.h): Scene inherits them.  They use the handle's `_list`, `_flags` and `_query`."""

    def _query_tris(self, triangles10):
        return self._list(triangles10, 10, "triangles10: n x [q0 q1 q2 mat] (the tenth value is ignored)")

    def overlap_tri(self, triangles10, max_list, inplace=False, want_prim=True, want_count=True, want_trips=False):
        """spira_scene_overlap_tri_*: the objects that each triangle of triangles10 cuts (host array, n x [q0 q1 q2 mat], the layout of a scene's own
        triangles10; the tenth value is ignored).  Returns (prim int32 [n, K], count uint32 [n], trips uint32 [n]) exactly as overlap_box does."""
        t = self._query_tris(triangles10)
        n, k = len(t), int(max_list)
        room = k if 0 < k <= MAX_OVERLAP else 1      # (a refused max_list: the entry says so)
        prim = np.empty((n, room), dtype=np.int32) if want_prim and k else None
        count = np.empty(n, dtype=np.uint32) if want_count else None
        trips = np.empty(n, dtype=np.uint32) if want_trips else None
        self._query("overlap_tri", False, (t,), (n, k), self._flags(inplace), (prim, count, trips))
        return prim, count, trips

    def overlap_tri_any(self, triangles10, inplace=False):
        """spira_scene_overlap_tri_any_*: uint8 [n] — 1 where the triangle cuts anything, 0 where nothing, 255 for an invalid query."""
        t = self._query_tris(triangles10)
        hit = np.empty(len(t), dtype=np.uint8)
        self._query("overlap_tri_any", False, (t,), (len(t),), self._flags(inplace), (hit,))
        return hit

    def overlap_tri_device(self, d_triangles_ptr, n, max_list, d_prim_ptr, d_count_ptr, stream_ptr, inplace=False, d_trips_ptr=0):
        """spira_scene_overlap_tri_device_*: DEVICE addresses (0 / None: output not wanted), asynchronous on the stream; nothing is synchronised or
        allocated."""
        self._query("overlap_tri", True, (d_triangles_ptr,), (n, max_list), self._flags(inplace), (d_prim_ptr, d_count_ptr, d_trips_ptr, stream_ptr))

    def overlap_tri_any_device(self, d_triangles_ptr, n, d_hit_ptr, stream_ptr, inplace=False):
        """spira_scene_overlap_tri_any_device_*: DEVICE addresses, asynchronous on the stream."""
        self._query("overlap_tri_any", True, (d_triangles_ptr,), (n,), self._flags(inplace), (d_hit_ptr, stream_ptr))


class Scene(_SceneProbes, _SceneTriOverlap):
    """A scene resident on the current device (spira_scene_create_* / spira_scene_destroy): validated, its BVH built
    and everything uploaded once.  Use as a context manager or call destroy()."""

    def __init__(self, spheres5, materials8, triangles10=None, prec="f32", n_devices=0):
        """n_devices >= 1: spira_scene_create_multi_* — validated and built once, resident on devices 0 .. n_devices-1 (render_multi)."""
        npdt, _ = _dt(prec)
        s, sp = _arr(spheres5, npdt)
        m, mp = _arr(materials8, npdt)
        t, tp = _arr(triangles10, npdt)
        self.prec = prec
        self.n_devices = n_devices
        self.counts = (0 if s is None else len(s), len(m), 0 if t is None else len(t))
        self._h = C.c_void_p()
        if n_devices:
            fn = lib().spira_scene_create_multi_f32 if prec == "f32" else lib().spira_scene_create_multi_f64
            _check(fn(sp, mp, tp, C.c_uint32(self.counts[0]), C.c_uint32(self.counts[1]), C.c_uint32(self.counts[2]), C.c_int(n_devices), C.byref(self._h)))
        else:
            fn = lib().spira_scene_create_f32 if prec == "f32" else lib().spira_scene_create_f64
            _check(fn(sp, mp, tp, C.c_uint32(self.counts[0]), C.c_uint32(self.counts[1]), C.c_uint32(self.counts[2]), C.byref(self._h)))

    def render_multi(self, camera12, params, n_devices=None, want_hdr=True, want_img=False):
        """spira_render_multi_scene_*: the frame on n_devices GPUs from the resident copies of this scene, host outputs."""
        npdt, _ = _dt(self.prec)
        c, cp = _arr(camera12, npdt)
        hdr = np.empty((3, params.height, params.width), dtype=npdt) if want_hdr else None
        img = np.empty((3, params.height, params.width), dtype=npdt) if want_img else None
        fn = lib().spira_render_multi_scene_f32 if self.prec == "f32" else lib().spira_render_multi_scene_f64
        _check(fn(self._h, cp, C.byref(params), C.c_int(n_devices or self.n_devices), hdr.ctypes.data_as(C.c_void_p) if want_hdr else None,
                  img.ctypes.data_as(C.c_void_p) if want_img else None))
        return hdr, img

    def update(self, spheres5=None, materials8=None, triangles10=None):
        """spira_scene_update_*: new contents for this handle from host arrays (None = unchanged; the counts are those of creation).  A mesh with a
        tree is refitted on the device, not rebuilt: its vertices must stay inside the frame the tree was built in (|(x - centre) * scale| <= 1, about the
        mesh's own size of room), else SpiraError (-4) and the handle renders what it rendered before.  Returns when the scene is ready."""
        npdt, _ = _dt(self.prec)
        arrs = [_arr(spheres5, npdt), _arr(materials8, npdt), _arr(triangles10, npdt)]
        for (a, _), n, w in zip(arrs, self.counts, (5, 8, 10)):
            if a is not None and a.size != n * w:
                raise ValueError("update: an array of %d values where the handle holds %d x %d" % (a.size, n, w))
        fn = lib().spira_scene_update_f32 if self.prec == "f32" else lib().spira_scene_update_f64
        _check(fn(self._h, arrs[0][1], arrs[1][1], arrs[2][1]))

    def update_device(self, triangles, stream=None):
        """spira_scene_update_device_*: the mesh's new triangles10 from DEVICE memory — a contiguous torch tensor of the handle's precision and n_triangles x 10
        values, or an integer device address — read on `stream` (a torch stream, an integer hipStream_t, None = the null stream).  Synchronises the stream once
        (the check kernel's status), then enqueues the refit and returns; the array must stay alive until that work has run."""
        npdt, _ = _dt(self.prec)
        if hasattr(triangles, "data_ptr"):
            import torch
            want = torch.float32 if self.prec == "f32" else torch.float64
            if triangles.dtype != want or not triangles.is_contiguous() or not triangles.is_cuda or triangles.numel() != self.counts[2] * 10:
                raise ValueError("update_device: a contiguous device tensor of %d x 10 %s values is needed" % (self.counts[2], self.prec))
            ptr = triangles.data_ptr()
        else:
            ptr = int(triangles or 0)
        sp = getattr(stream, "cuda_stream", stream)
        fn = lib().spira_scene_update_device_f32 if self.prec == "f32" else lib().spira_scene_update_device_f64
        _check(fn(self._h, C.c_void_p(ptr or None), C.c_void_p(sp or None)))

    def rebuild(self, triangles10):
        """spira_scene_rebuild_*: a new triangle array (host, n_triangles x 10 as at creation) and the mesh's tree built anew on the device — a new frame and a
        new topology, so the mesh may be anywhere and of any size (no frame rule).  A refused rebuild leaves the handle as it was.  Returns when the scene is ready."""
        npdt, _ = _dt(self.prec)
        a, ap = _arr(triangles10, npdt)
        if a is not None and a.size != self.counts[2] * 10:
            raise ValueError("rebuild: an array of %d values where the handle holds %d x 10" % (a.size, self.counts[2]))
        fn = lib().spira_scene_rebuild_f32 if self.prec == "f32" else lib().spira_scene_rebuild_f64
        _check(fn(self._h, ap))

    def rebuild_device(self, triangles, stream=None):
        """spira_scene_rebuild_device_*: the same from DEVICE memory — a contiguous torch tensor of the handle's precision and n_triangles x 10 values, or an
        integer device address — read on `stream` (a torch stream, an integer hipStream_t, None = the null stream).  Synchronises the stream once for the check
        kernel's status and bounds and once per level of the new tree, then enqueues the rest and returns; the array must stay alive until that work has run."""
        if hasattr(triangles, "data_ptr"):
            import torch
            want = torch.float32 if self.prec == "f32" else torch.float64
            if triangles.dtype != want or not triangles.is_contiguous() or not triangles.is_cuda or triangles.numel() != self.counts[2] * 10:
                raise ValueError("rebuild_device: a contiguous device tensor of %d x 10 %s values is needed" % (self.counts[2], self.prec))
            ptr = triangles.data_ptr()
        else:
            ptr = int(triangles or 0)
        sp = getattr(stream, "cuda_stream", stream)
        fn = lib().spira_scene_rebuild_device_f32 if self.prec == "f32" else lib().spira_scene_rebuild_device_f64
        _check(fn(self._h, C.c_void_p(ptr or None), C.c_void_p(sp or None)))

    def destroy(self):
        if self._h:
            _check(lib().spira_scene_destroy(self._h))
            self._h = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.destroy()

    def params(self, width, height, spp, max_depth, **kw):
        return make_params(width, height, spp, max_depth, *self.counts, **kw)

    def render(self, camera12, params, want_hdr=True, want_img=False):
        npdt, _ = _dt(self.prec)
        c, cp = _arr(camera12, npdt)
        rows = params.rows if params.rows else params.height
        hdr = np.empty((3, rows, params.width), dtype=npdt) if want_hdr else None
        img = np.empty((3, rows, params.width), dtype=npdt) if want_img else None
        fn = lib().spira_render_scene_f32 if self.prec == "f32" else lib().spira_render_scene_f64
        _check(fn(self._h, cp, C.byref(params), hdr.ctypes.data_as(C.c_void_p) if want_hdr else None,
                  img.ctypes.data_as(C.c_void_p) if want_img else None))
        return hdr, img

    def render_device(self, camera12, params, d_hdr_ptr, d_img_ptr, stream_ptr):
        npdt, _ = _dt(self.prec)
        c, cp = _arr(camera12, npdt)
        fn = lib().spira_render_scene_device_f32 if self.prec == "f32" else lib().spira_render_scene_device_f64
        _check(fn(self._h, cp, C.byref(params), C.c_void_p(d_hdr_ptr or None), C.c_void_p(d_img_ptr or None), C.c_void_p(stream_ptr or None)))

    def render_adaptive(self, camera12, params, adaptive, want_hdr=True, want_img=False, want_spp=True, want_q=True):
        """spira_render_adaptive_scene_*: returns (hdr, img, spp, q) — [3, rows, W], [3, rows, W], uint32 [rows, W], [rows, W] or None."""
        npdt, _ = _dt(self.prec)
        c, cp = _arr(camera12, npdt)
        outs, ptrs = _adaptive_outputs(params, npdt, want_hdr, want_img, want_spp, want_q)
        fn = lib().spira_render_adaptive_scene_f32 if self.prec == "f32" else lib().spira_render_adaptive_scene_f64
        _check(fn(self._h, cp, C.byref(params), C.byref(adaptive), *ptrs))
        return outs

    def render_adaptive_device(self, camera12, params, adaptive, d_hdr_ptr, d_img_ptr, d_spp_ptr, d_q_ptr, stream_ptr):
        """spira_render_adaptive_scene_device_*: DEVICE output addresses (0 / None: not wanted); synchronises the stream once per round."""
        npdt, _ = _dt(self.prec)
        c, cp = _arr(camera12, npdt)
        fn = lib().spira_render_adaptive_scene_device_f32 if self.prec == "f32" else lib().spira_render_adaptive_scene_device_f64
        _check(fn(self._h, cp, C.byref(params), C.byref(adaptive), C.c_void_p(d_hdr_ptr or None), C.c_void_p(d_img_ptr or None),
                  C.c_void_p(d_spp_ptr or None), C.c_void_p(d_q_ptr or None), C.c_void_p(stream_ptr or None)))


    def render_features(self, camera12, params, want_albedo=True, want_normal=True, want_depth=True):
        """spira_render_features_scene_*: returns (albedo [3, rows, W], normal [3, rows, W], depth [rows, W]); None where not wanted."""
        npdt, _ = _dt(self.prec)
        c, cp = _arr(camera12, npdt)
        outs, ptrs = _feature_outputs(params, npdt, want_albedo, want_normal, want_depth)
        fn = lib().spira_render_features_scene_f32 if self.prec == "f32" else lib().spira_render_features_scene_f64
        _check(fn(self._h, cp, C.byref(params), *ptrs))
        return outs

    def render_features_device(self, camera12, params, d_albedo_ptr, d_normal_ptr, d_depth_ptr, stream_ptr):
        """spira_render_features_scene_device_*: DEVICE output addresses (0 / None: not wanted), asynchronous on the stream."""
        npdt, _ = _dt(self.prec)
        c, cp = _arr(camera12, npdt)
        fn = lib().spira_render_features_scene_device_f32 if self.prec == "f32" else lib().spira_render_features_scene_device_f64
        _check(fn(self._h, cp, C.byref(params), C.c_void_p(d_albedo_ptr or None), C.c_void_p(d_normal_ptr or None), C.c_void_p(d_depth_ptr or None),
                  C.c_void_p(stream_ptr or None)))

    def _fn(self, stem, device=False):
        """The entry spira_scene_<stem>[_device]_<prec> of this handle's precision."""
        return getattr(lib(), "spira_scene_" + stem + ("_device_" if device else "_") + self.prec)

    @staticmethod
    def _ptrs(device, arrays):
        """The void * arguments of a call: integer device addresses (0 / None: NULL), or host arrays (numpy; None: NULL)."""
        if device:
            return map(C.c_void_p, arrays)
        return [None if a is None else a.ctypes.data_as(C.c_void_p) for a in arrays]

    @staticmethod
    def _flags(inplace, count_all=0):
        """The flag word of a query: CAST_INPLACE, and the count-all bit of the entries that have one."""
        return C.c_uint32((CAST_INPLACE if inplace else 0) | count_all)

    def _query(self, stem, device, ins, counts, word, outs):
        """One list call: (handle, input arrays, the uint32 counts, the flag word or the parameter struct by reference, output arrays [, stream]); the
        device form takes addresses."""
        _check(self._fn(stem, device)(self._h, *self._ptrs(device, ins), *map(C.c_uint32, counts), word, *self._ptrs(device, outs)))

    def _list(self, a, width, what):
        a = np.ascontiguousarray(a, dtype=_dt(self.prec)[0])
        if a.ndim != 2 or a.shape[1] != width:
            raise ValueError(what)
        return a

    def _rays(self, rays8):
        return self._list(rays8, 8, "rays8: n_rays x [ox oy oz t_min dx dy dz t_max]")

    def _points4(self, points4):
        return self._list(points4, 4, "points4: n_points x [px py pz r_max]")

    def cast(self, rays8, want_normal=False, inplace=False, want_prim=True, want_t=True):
        """spira_scene_cast_*: the closest hit of every ray of rays8 (n x [ox oy oz t_min dx dy dz t_max], host array; directions are normalised by the
        library, t / t_min / t_max are distances along the unit direction).  Returns (prim int32 [n], t [n], normal [n, 3]), None where not wanted:
        prim is the object index (spheres first), RAY_MISS (t = the ray's t_max) or RAY_INVALID (t = 0).  inplace: the comparison organisation."""
        npdt, _ = _dt(self.prec)
        r = self._rays(rays8)
        n = len(r)
        prim = np.empty(n, dtype=np.int32) if want_prim else None
        t = np.empty(n, dtype=npdt) if want_t else None
        nrm = np.empty((n, 3), dtype=npdt) if want_normal else None
        self._query("cast", False, (r,), (n,), self._flags(inplace), (prim, t, nrm))
        return prim, t, nrm

    def occluded(self, rays8, inplace=False):
        """spira_scene_occluded_*: uint8 [n] — 1 where the ray hits anything within [t_min, t_max], 0 where not, 255 for an invalid ray."""
        r = self._rays(rays8)
        hit = np.empty(len(r), dtype=np.uint8)
        self._query("occluded", False, (r,), (len(r),), self._flags(inplace), (hit,))
        return hit

    def cast_device(self, d_rays_ptr, n_rays, d_prim_ptr, d_t_ptr, d_normal_ptr, stream_ptr, inplace=False):
        """spira_scene_cast_device_*: DEVICE addresses (0 / None: output not wanted), asynchronous on the stream; nothing is synchronised or allocated."""
        self._query("cast", True, (d_rays_ptr,), (n_rays,), self._flags(inplace), (d_prim_ptr, d_t_ptr, d_normal_ptr, stream_ptr))

    def occluded_device(self, d_rays_ptr, n_rays, d_hit_ptr, stream_ptr, inplace=False):
        """spira_scene_occluded_device_*: DEVICE addresses, asynchronous on the stream."""
        self._query("occluded", True, (d_rays_ptr,), (n_rays,), self._flags(inplace), (d_hit_ptr, stream_ptr))

    def cast_hits(self, rays8, max_hits, inplace=False, count_all=False, want_prim=True, want_t=True, want_count=True):
        """spira_scene_cast_hits_*: the first max_hits hits of every ray of rays8 (host array, as for cast), ordered by t ascending and, among equal t, by
        object index descending.  Returns (prim int32 [n, K], t [n, K], count uint32 [n]), None where not wanted (with max_hits = 0 the lists are None):
        unused slots hold RAY_MISS and the ray's t_max, every slot of an invalid ray RAY_INVALID and 0.  count: the slots filled, or with count_all every
        candidate of the ray (the walk then prunes with t_max only; max_hits may be 0).  inplace: the comparison organisation."""
        npdt, _ = _dt(self.prec)
        r = self._rays(rays8)
        n, k = len(r), int(max_hits)
        room = k if 0 < k <= MAX_HITS else 1      # (a refused max_hits: the entry says so)
        prim = np.empty((n, room), dtype=np.int32) if want_prim and k else None
        t = np.empty((n, room), dtype=npdt) if want_t and k else None
        count = np.empty(n, dtype=np.uint32) if want_count else None
        self._query("cast_hits", False, (r,), (n, k), self._flags(inplace, HITS_COUNT_ALL if count_all else 0), (prim, t, count))
        return prim, t, count

    def cast_hits_device(self, d_rays_ptr, n_rays, max_hits, d_prim_ptr, d_t_ptr, d_count_ptr, stream_ptr, inplace=False, count_all=False):
        """spira_scene_cast_hits_device_*: DEVICE addresses (0 / None: output not wanted), asynchronous on the stream; nothing is synchronised or
        allocated."""
        self._query("cast_hits", True, (d_rays_ptr,), (n_rays, max_hits), self._flags(inplace, HITS_COUNT_ALL if count_all else 0),
                    (d_prim_ptr, d_t_ptr, d_count_ptr, stream_ptr))

    def closest_point(self, points4, inplace=False, want_prim=True, want_dist=True, want_point=True, want_trips=False):
        """spira_scene_closest_point_*: for every point of points4 (n x [px py pz r_max], host array) the nearest point of the scene's surface within r_max.
        Returns (prim int32 [n], dist [n], point [n, 3], trips uint32 [n]), None where not wanted: prim is the object index (spheres first), RAY_MISS
        (dist = the point's r_max, point 0) or RAY_INVALID (dist 0, point 0).  inplace: the comparison organisation."""
        npdt, _ = _dt(self.prec)
        p = self._points4(points4)
        n = len(p)
        prim = np.empty(n, dtype=np.int32) if want_prim else None
        dist = np.empty(n, dtype=npdt) if want_dist else None
        point = np.empty((n, 3), dtype=npdt) if want_point else None
        trips = np.empty(n, dtype=np.uint32) if want_trips else None
        self._query("closest_point", False, (p,), (n,), self._flags(inplace), (prim, dist, point, trips))
        return prim, dist, point, trips

    def closest_point_device(self, d_points_ptr, n_points, d_prim_ptr, d_dist_ptr, d_point_ptr, stream_ptr, inplace=False, d_trips_ptr=0):
        """spira_scene_closest_point_device_*: DEVICE addresses (0 / None: output not wanted), asynchronous on the stream; nothing is synchronised or
        allocated."""
        self._query("closest_point", True, (d_points_ptr,), (n_points,), self._flags(inplace), (d_prim_ptr, d_dist_ptr, d_point_ptr, d_trips_ptr, stream_ptr))

    def nearest_k(self, points4, max_near, inplace=False, count_all=False, want_prim=True, want_dist=True, want_point=True, want_count=True, want_trips=False):
        """spira_scene_nearest_k_*: the max_near closest objects of every point of points4 (host array, as for closest_point), ordered by squared distance
        ascending and, among equal ones, by object index descending.  Returns (prim int32 [n, K], dist [n, K], point [n, K, 3], count uint32 [n],
        trips uint32 [n]), None where not wanted (with max_near = 0 the lists are None): unused slots hold RAY_MISS, the point's r_max and point 0, every
        slot of an invalid point RAY_INVALID, 0 and 0.  count: the slots filled, or with count_all every object within r_max (the walk then prunes with
        r_max only; max_near may be 0).  inplace: the comparison organisation."""
        npdt, _ = _dt(self.prec)
        p = self._points4(points4)
        n, k = len(p), int(max_near)
        room = k if 0 < k <= MAX_NEAR else 1      # (a refused max_near: the entry says so)
        prim = np.empty((n, room), dtype=np.int32) if want_prim and k else None
        dist = np.empty((n, room), dtype=npdt) if want_dist and k else None
        point = np.empty((n, room, 3), dtype=npdt) if want_point and k else None
        count = np.empty(n, dtype=np.uint32) if want_count else None
        trips = np.empty(n, dtype=np.uint32) if want_trips else None
        self._query("nearest_k", False, (p,), (n, k), self._flags(inplace, NEAR_COUNT_ALL if count_all else 0), (prim, dist, point, count, trips))
        return prim, dist, point, count, trips

    def nearest_k_device(self, d_points_ptr, n_points, max_near, d_prim_ptr, d_dist_ptr, d_point_ptr, d_count_ptr, stream_ptr, inplace=False, count_all=False,
                         d_trips_ptr=0):
        """spira_scene_nearest_k_device_*: DEVICE addresses (0 / None: output not wanted), asynchronous on the stream; nothing is synchronised or
        allocated."""
        self._query("nearest_k", True, (d_points_ptr,), (n_points, max_near), self._flags(inplace, NEAR_COUNT_ALL if count_all else 0),
                    (d_prim_ptr, d_dist_ptr, d_point_ptr, d_count_ptr, d_trips_ptr, stream_ptr))

    def _sweeps(self, rays8, radii):
        npdt, _ = _dt(self.prec)
        r = self._rays(rays8)
        rad = np.ascontiguousarray(radii, dtype=npdt)
        if rad.ndim != 1 or len(rad) != len(r):
            raise ValueError("radii: one radius per ray")
        return r, rad

    def sweep(self, rays8, radii, inplace=False, want_prim=True, want_t=True, want_point=True, want_normal=True, want_trips=False):
        """spira_scene_sweep_*: the first contact of a ball of radius radii[i] whose centre moves along rays8[i] (host arrays; the rays as for cast).
        Returns (prim int32 [n], t [n], point [n, 3], normal [n, 3], trips uint32 [n]), None where not wanted: prim is the object index (spheres first),
        RAY_MISS (t = the ray's t_max, point 0, normal 0) or RAY_INVALID (all 0); t is the distance of the ball's centre along the unit direction, point the
        contact on the surface, normal the unit vector from it to the centre.  inplace: the comparison organisation."""
        npdt, _ = _dt(self.prec)
        r, rad = self._sweeps(rays8, radii)
        n = len(r)
        prim = np.empty(n, dtype=np.int32) if want_prim else None
        t = np.empty(n, dtype=npdt) if want_t else None
        point = np.empty((n, 3), dtype=npdt) if want_point else None
        nrm = np.empty((n, 3), dtype=npdt) if want_normal else None
        trips = np.empty(n, dtype=np.uint32) if want_trips else None
        self._query("sweep", False, (r, rad), (n,), self._flags(inplace), (prim, t, point, nrm, trips))
        return prim, t, point, nrm, trips

    def sweep_blocked(self, rays8, radii, inplace=False):
        """spira_scene_sweep_blocked_*: uint8 [n] — 1 where the ball touches anything within [t_min, t_max], 0 where not, 255 for an invalid sweep."""
        r, rad = self._sweeps(rays8, radii)
        hit = np.empty(len(r), dtype=np.uint8)
        self._query("sweep_blocked", False, (r, rad), (len(r),), self._flags(inplace), (hit,))
        return hit

    def sweep_device(self, d_rays_ptr, d_radii_ptr, n, d_prim_ptr, d_t_ptr, d_point_ptr, d_normal_ptr, stream_ptr, inplace=False, d_trips_ptr=0):
        """spira_scene_sweep_device_*: DEVICE addresses (0 / None: output not wanted), asynchronous on the stream; nothing is synchronised or allocated."""
        self._query("sweep", True, (d_rays_ptr, d_radii_ptr), (n,), self._flags(inplace), (d_prim_ptr, d_t_ptr, d_point_ptr, d_normal_ptr, d_trips_ptr, stream_ptr))

    def sweep_blocked_device(self, d_rays_ptr, d_radii_ptr, n, d_hit_ptr, stream_ptr, inplace=False):
        """spira_scene_sweep_blocked_device_*: DEVICE addresses, asynchronous on the stream."""
        self._query("sweep_blocked", True, (d_rays_ptr, d_radii_ptr), (n,), self._flags(inplace), (d_hit_ptr, stream_ptr))

    def _boxes(self, boxes10):
        return self._list(boxes10, 10, "boxes10: n x [cx cy cz hx hy hz qx qy qz qw]")

    def overlap_box(self, boxes10, max_list, inplace=False, want_prim=True, want_count=True, want_trips=False):
        """spira_scene_overlap_box_*: the objects that touch each oriented box of boxes10 (host array, n x [cx cy cz hx hy hz qx qy qz qw]; the library
        normalises the quaternion).  Returns (prim int32 [n, K], count uint32 [n], trips uint32 [n]), None where not wanted (with max_list = 0 the list is
        None): prim holds the first max_list candidates in ascending object index, unused slots RAY_MISS, every slot of an invalid box RAY_INVALID; count
        is the number of ALL candidates (0 for an invalid box).  inplace: the comparison organisation."""
        b = self._boxes(boxes10)
        n, k = len(b), int(max_list)
        room = k if 0 < k <= MAX_OVERLAP else 1      # (a refused max_list: the entry says so)
        prim = np.empty((n, room), dtype=np.int32) if want_prim and k else None
        count = np.empty(n, dtype=np.uint32) if want_count else None
        trips = np.empty(n, dtype=np.uint32) if want_trips else None
        self._query("overlap_box", False, (b,), (n, k), self._flags(inplace), (prim, count, trips))
        return prim, count, trips

    def overlap_any(self, boxes10, inplace=False):
        """spira_scene_overlap_any_*: uint8 [n] — 1 where anything touches the box, 0 where nothing does, 255 for an invalid box."""
        b = self._boxes(boxes10)
        hit = np.empty(len(b), dtype=np.uint8)
        self._query("overlap_any", False, (b,), (len(b),), self._flags(inplace), (hit,))
        return hit

    def overlap_box_device(self, d_boxes_ptr, n, max_list, d_prim_ptr, d_count_ptr, stream_ptr, inplace=False, d_trips_ptr=0):
        """spira_scene_overlap_box_device_*: DEVICE addresses (0 / None: output not wanted), asynchronous on the stream; nothing is synchronised or
        allocated."""
        self._query("overlap_box", True, (d_boxes_ptr,), (n, max_list), self._flags(inplace), (d_prim_ptr, d_count_ptr, d_trips_ptr, stream_ptr))

    def overlap_any_device(self, d_boxes_ptr, n, d_hit_ptr, stream_ptr, inplace=False):
        """spira_scene_overlap_any_device_*: DEVICE addresses, asynchronous on the stream."""
        self._query("overlap_any", True, (d_boxes_ptr,), (n,), self._flags(inplace), (d_hit_ptr, stream_ptr))

    def signed_distance(self, points4, inplace=False, want_point=True, want_crossings=False, want_trips=False, want_prim=True, want_dist=True, want_inside=True):
        """spira_scene_signed_distance_*: for every point of points4 (host array, as for closest_point) the nearest surface and which side of it the point is
        on.  Returns (prim int32 [n], dist [n], point [n, 3], inside uint8 [n], crossings uint32 [n, 3], trips uint32 [n]), None where not wanted: prim and
        point are closest_point's, dist is closest_point's with the sign bit set where the point is inside; inside is 1, 0 or 255 (an invalid point);
        crossings the triangle candidates of the three rays (SDF_SKIPPED: ray not walked).  With prim, dist and point all unwanted the nearest walk is not
        run (the sign-only query).  inplace: the comparison organisation."""
        npdt, _ = _dt(self.prec)
        p = self._points4(points4)
        n = len(p)
        prim = np.empty(n, dtype=np.int32) if want_prim else None
        dist = np.empty(n, dtype=npdt) if want_dist else None
        point = np.empty((n, 3), dtype=npdt) if want_point else None
        inside = np.empty(n, dtype=np.uint8) if want_inside else None
        crossings = np.empty((n, 3), dtype=np.uint32) if want_crossings else None
        trips = np.empty(n, dtype=np.uint32) if want_trips else None
        self._query("signed_distance", False, (p,), (n,), self._flags(inplace), (prim, dist, point, inside, crossings, trips))
        return prim, dist, point, inside, crossings, trips

    def signed_distance_device(self, d_points_ptr, n_points, d_prim_ptr, d_dist_ptr, d_point_ptr, d_inside_ptr, stream_ptr, inplace=False, d_crossings_ptr=0,
                               d_trips_ptr=0):
        """spira_scene_signed_distance_device_*: DEVICE addresses (0 / None: output not wanted), asynchronous on the stream; nothing is synchronised or
        allocated."""
        self._query("signed_distance", True, (d_points_ptr,), (n_points,), self._flags(inplace),
                    (d_prim_ptr, d_dist_ptr, d_point_ptr, d_inside_ptr, d_crossings_ptr, d_trips_ptr, stream_ptr))

    def radiance(self, rays6, spp, max_depth, seed=0, sample0=0, key0=0, flags=0, sums=None, want_valid=False):
        """spira_scene_radiance_*: path-traced radiance along rays6 (n x [ox oy oz dx dy dz], host array; directions are normalised by the library).
        Ray k, sample s is the renderer's path at pixel key key0 + k.  ADDS samples sample0 .. sample0 + spp - 1, in order, to sums ([n, 3], in place; None: a
        fresh zero array).  Returns sums, or (sums, valid uint8 [n]) with want_valid."""
        npdt, _ = _dt(self.prec)
        r = self._list(rays6, 6, "rays6: n_rays x [ox oy oz dx dy dz]")
        n = len(r)
        if sums is None:
            sums = np.zeros((n, 3), dtype=npdt)
        if sums.dtype != npdt or not sums.flags["C_CONTIGUOUS"] or sums.shape != (n, 3):
            raise ValueError("sums: a contiguous [n_rays, 3] array of the handle's precision")
        valid = np.empty(n, dtype=np.uint8) if want_valid else None
        rp = Radiance(spp, max_depth, flags, sample0, seed, key0, 0)
        self._query("radiance", False, (r,), (n,), C.byref(rp), (sums, valid))
        return (sums, valid) if want_valid else sums

    def radiance_device(self, d_rays_ptr, n_rays, spp, max_depth, d_sums_ptr, seed=0, sample0=0, key0=0, flags=0, d_valid_ptr=0, stream_ptr=0):
        """spira_scene_radiance_device_*: DEVICE addresses (d_valid_ptr 0 / None: not wanted), asynchronous on the stream; the sums are added to in place."""
        rp = Radiance(spp, max_depth, flags, sample0, seed, key0, 0)
        self._query("radiance", True, (d_rays_ptr,), (n_rays,), C.byref(rp), (d_sums_ptr, d_valid_ptr, stream_ptr))


    def _points(self, points6):
        return self._list(points6, 6, "points6: n_points x [px py pz nx ny nz]")

    def gather(self, points6, spp, max_depth, seed=0, sample0=0, key0=0, flags=0, sums=None, want_valid=False):
        """spira_scene_gather_*: path-traced radiance over the hemisphere of every point of points6 (n x [px py pz nx ny nz], host array; the library
        draws the cosine-weighted directions itself, point k under pixel key key0 + k).  ADDS samples sample0 .. sample0 + spp - 1, in order, to sums
        ([n, 3], in place; None: a fresh zero array); irradiance is pi * sums / spp.  Returns sums, or (sums, valid uint8 [n]) with want_valid."""
        npdt, _ = _dt(self.prec)
        p = self._points(points6)
        n = len(p)
        if sums is None:
            sums = np.zeros((n, 3), dtype=npdt)
        if sums.dtype != npdt or not sums.flags["C_CONTIGUOUS"] or sums.shape != (n, 3):
            raise ValueError("sums: a contiguous [n_points, 3] array of the handle's precision")
        valid = np.empty(n, dtype=np.uint8) if want_valid else None
        rp = Radiance(spp, max_depth, flags, sample0, seed, key0, 0)
        self._query("gather", False, (p,), (n,), C.byref(rp), (sums, valid))
        return (sums, valid) if want_valid else sums

    def gather_device(self, d_points_ptr, n_points, spp, max_depth, d_sums_ptr, seed=0, sample0=0, key0=0, flags=0, d_valid_ptr=0, stream_ptr=0):
        """spira_scene_gather_device_*: DEVICE addresses (d_valid_ptr 0 / None: not wanted), asynchronous on the stream; the sums are added to in place."""
        rp = Radiance(spp, max_depth, flags, sample0, seed, key0, 0)
        self._query("gather", True, (d_points_ptr,), (n_points,), C.byref(rp), (d_sums_ptr, d_valid_ptr, stream_ptr))

    def gather_visible(self, points6, spp, t_min=1e-3, t_max=float("inf"), seed=0, sample0=0, key0=0, counts=None, want_valid=False, inplace=False):
        """spira_scene_gather_visible_*: ADDS to counts (uint32 [n], in place; None: a fresh zero array) the number of samples sample0 .. sample0 + spp - 1
        whose hemisphere direction is unoccluded within [t_min, t_max] — what Scene.occluded answers 0 for.  Returns counts, or (counts, valid uint8 [n])
        with want_valid (0: an invalid point, or one beyond the origin bound of a scene with a tree).  inplace: the comparison organisation."""
        p = self._points(points6)
        n = len(p)
        if counts is None:
            counts = np.zeros(n, dtype=np.uint32)
        if counts.dtype != np.uint32 or not counts.flags["C_CONTIGUOUS"] or counts.shape != (n,):
            raise ValueError("counts: a contiguous uint32 [n_points] array")
        valid = np.empty(n, dtype=np.uint8) if want_valid else None
        gv = GatherVisible(spp, sample0, seed, key0, CAST_INPLACE if inplace else 0, t_min, t_max)
        self._query("gather_visible", False, (p,), (n,), C.byref(gv), (counts, valid))
        return (counts, valid) if want_valid else counts

    def gather_visible_device(self, d_points_ptr, n_points, spp, d_counts_ptr, t_min=1e-3, t_max=float("inf"), seed=0, sample0=0, key0=0, d_valid_ptr=0,
                              stream_ptr=0, inplace=False):
        """spira_scene_gather_visible_device_*: DEVICE addresses, asynchronous on the stream; nothing is synchronised or allocated."""
        gv = GatherVisible(spp, sample0, seed, key0, CAST_INPLACE if inplace else 0, t_min, t_max)
        self._query("gather_visible", True, (d_points_ptr,), (n_points,), C.byref(gv), (d_counts_ptr, d_valid_ptr, stream_ptr))


def gather_rays(points6, sample=0, seed=0, key0=0, prec="f32"):
    """spira_gather_rays_*: the hemisphere rays of one sample of every point of points6 (n x [px py pz nx ny nz]) as a host array [n, 6] = [p, v], v not
    normalised; six zeros for an invalid point.  Point k draws under pixel key key0 + k.  Host arithmetic; no device needed."""
    npdt, _ = _dt(prec)
    p = np.ascontiguousarray(points6, dtype=npdt)
    if p.ndim != 2 or p.shape[1] != 6:
        raise ValueError("points6: n_points x [px py pz nx ny nz]")
    out = np.empty((len(p), 6), dtype=npdt)
    fn = lib().spira_gather_rays_f32 if prec == "f32" else lib().spira_gather_rays_f64
    _check(fn(p.ctypes.data_as(C.c_void_p), C.c_uint32(len(p)), C.c_uint32(sample), C.c_uint64(seed), C.c_uint32(key0), out.ctypes.data_as(C.c_void_p)))
    return out


def gather_rays_device(d_points_ptr, n_points, d_rays_ptr, sample=0, seed=0, key0=0, stream_ptr=0, prec="f32"):
    """spira_gather_rays_device_*: the same from and into DEVICE arrays of n_points * 6 values, asynchronous on the stream."""
    _dt(prec)
    fn = lib().spira_gather_rays_device_f32 if prec == "f32" else lib().spira_gather_rays_device_f64
    _check(fn(C.c_void_p(d_points_ptr or None), C.c_uint32(n_points), C.c_uint32(sample), C.c_uint64(seed), C.c_uint32(key0), C.c_void_p(d_rays_ptr or None),
              C.c_void_p(stream_ptr or None)))


def probe_rays(points3, sample=0, seed=0, key0=0, prec="f32"):
    """spira_probe_rays_*: the sphere rays of one sample of every point of points3 (n x [px py pz]) as a host array [n, 6] = [p, qh], qh a uniform
    direction on the unit sphere; six zeros for an invalid point.  Point k draws under pixel key key0 + k.  Host arithmetic; no device needed."""
    npdt, _ = _dt(prec)
    p = np.ascontiguousarray(points3, dtype=npdt)
    if p.ndim != 2 or p.shape[1] != 3:
        raise ValueError("points3: n_points x [px py pz]")
    out = np.empty((len(p), 6), dtype=npdt)
    fn = lib().spira_probe_rays_f32 if prec == "f32" else lib().spira_probe_rays_f64
    _check(fn(p.ctypes.data_as(C.c_void_p), C.c_uint32(len(p)), C.c_uint32(sample), C.c_uint64(seed), C.c_uint32(key0), out.ctypes.data_as(C.c_void_p)))
    return out


def probe_rays_device(d_points_ptr, n_points, d_rays_ptr, sample=0, seed=0, key0=0, stream_ptr=0, prec="f32"):
    """spira_probe_rays_device_*: the same from a DEVICE array of n_points * 3 values into one of n_points * 6, asynchronous on the stream."""
    _dt(prec)
    fn = lib().spira_probe_rays_device_f32 if prec == "f32" else lib().spira_probe_rays_device_f64
    _check(fn(C.c_void_p(d_points_ptr or None), C.c_uint32(n_points), C.c_uint32(sample), C.c_uint64(seed), C.c_uint32(key0), C.c_void_p(d_rays_ptr or None),
              C.c_void_p(stream_ptr or None)))


def sh9_basis(d, prec="f32"):
    """spira_sh9_basis_*: the nine real spherical harmonics of bands 0 .. 2 at the unit directions d ([n, 3] or [3]), [n, 9] or [9] in `prec`."""
    npdt, _ = _dt(prec)
    dd = np.ascontiguousarray(d, dtype=npdt)
    if dd.ndim not in (1, 2) or dd.shape[-1] != 3:
        raise ValueError("d: [n, 3] or [3] unit directions")
    rows = dd.reshape(-1, 3)
    out = np.empty((len(rows), 9), dtype=npdt)
    fn = lib().spira_sh9_basis_f32 if prec == "f32" else lib().spira_sh9_basis_f64
    fn.restype = None
    for k in range(len(rows)):
        fn(rows[k].ctypes.data_as(C.c_void_p), out[k].ctypes.data_as(C.c_void_p))
    return out.reshape(dd.shape[:-1] + (9,))


def gather_plan(n_points, spp, num_cus):
    """The launch plan a gather of n_points x spp gets on a device of num_cus compute units (test support; no device needed): the dict of radiance_plan —
    pass p covers the samples [p * spp_pass, min((p + 1) * spp_pass, spp)) of every point."""
    out = (C.c_uint32 * 8)()
    _check(lib().spira_debug_gather_plan(C.c_uint32(n_points), C.c_uint32(spp), C.c_uint32(num_cus), out))
    v = [int(x) for x in out]
    return {"grid": v[0], "wpb": v[1], "spp_pass": v[2], "n_pass": v[3], "direct": bool(v[4]), "ws_entries": v[5] | (v[6] << 32), "max_items": v[7]}


def make_lens(model, width, height, sample=0, seed=0, row0=0, rows=0, lens_radius=0.0):
    return Lens(model, width, height, sample, seed, row0, rows, lens_radius)


def camera_rays(camera12, model, width, height, sample=0, seed=0, row0=0, rows=0, lens_radius=0.0, prec="f32"):
    """spira_camera_rays_*: the rays of one sample of every pixel of `rows` rows (0: all) as a host array [rows * width, 6] = [o, d], d not normalised,
    ordered by reference pixel (row j - 1 = row0 first: the BOTTOM of the image, v = 0).  Host arithmetic; no device needed."""
    npdt, _ = _dt(prec)
    c, cp = _arr(camera12, npdt)
    assert c.shape == (12,)
    lens = make_lens(model, width, height, sample, seed, row0, rows, lens_radius)
    n = (rows or height) * width
    out = np.empty((n if 0 < n <= MAX_RAYS else 1, 6), dtype=npdt)      # (a refused size: the entry says so)
    fn = lib().spira_camera_rays_f32 if prec == "f32" else lib().spira_camera_rays_f64
    _check(fn(cp, C.byref(lens), out.ctypes.data_as(C.c_void_p)))
    return out


def camera_rays_device(camera12, model, width, height, d_rays_ptr, sample=0, seed=0, row0=0, rows=0, lens_radius=0.0, stream_ptr=0, prec="f32"):
    """spira_camera_rays_device_*: the same into a DEVICE array of (rows or height) * width * 6 values, asynchronous on the stream."""
    npdt, _ = _dt(prec)
    c, cp = _arr(camera12, npdt)
    assert c.shape == (12,)
    lens = make_lens(model, width, height, sample, seed, row0, rows, lens_radius)
    fn = lib().spira_camera_rays_device_f32 if prec == "f32" else lib().spira_camera_rays_device_f64
    _check(fn(cp, C.byref(lens), C.c_void_p(d_rays_ptr or None), C.c_void_p(stream_ptr or None)))


def radiance_plan(n_rays, spp, num_cus):
    """The launch plan a radiance call of n_rays x spp gets on a device of num_cus compute units (test support; no device needed): a dict of grid, wpb,
    spp_pass, n_pass, direct, ws_entries, max_items — pass p covers the samples [p * spp_pass, min((p + 1) * spp_pass, spp))."""
    out = (C.c_uint32 * 8)()
    _check(lib().spira_debug_radiance_plan(C.c_uint32(n_rays), C.c_uint32(spp), C.c_uint32(num_cus), out))
    v = [int(x) for x in out]
    return {"grid": v[0], "wpb": v[1], "spp_pass": v[2], "n_pass": v[3], "direct": bool(v[4]), "ws_entries": v[5] | (v[6] << 32), "max_items": v[7]}


def cast_plan(n_rays, num_cus):
    """The launch plan a cast of n_rays gets on a device of num_cus compute units (test support; no device needed): a dict of grid, wpb, waves, base,
    rem, refill_free, grid_flat, min_rays_per_wave — wave w of the session kernel owns base + (w < rem) rays from w * base + min(w, rem)."""
    out = (C.c_uint32 * 8)()
    _check(lib().spira_debug_cast_plan(C.c_uint32(n_rays), C.c_uint32(num_cus), out))
    return dict(zip(("grid", "wpb", "waves", "base", "rem", "refill_free", "grid_flat", "min_rays_per_wave"), [int(v) for v in out]))


def _feature_outputs(params, npdt, want_albedo, want_normal, want_depth):
    rows = params.rows if params.rows else params.height
    outs = (np.empty((3, rows, params.width), dtype=npdt) if want_albedo else None, np.empty((3, rows, params.width), dtype=npdt) if want_normal else None,
            np.empty((rows, params.width), dtype=npdt) if want_depth else None)
    return outs, [o.ctypes.data_as(C.c_void_p) if o is not None else None for o in outs]


def render_features(spheres5, materials8, triangles10, camera12, params, prec="f32", want_albedo=True, want_normal=True, want_depth=True):
    """spira_render_features_*: host arrays, host outputs.  Returns (albedo, normal, depth): the first-hit features averaged over params.spp camera
    rays per pixel ([3, rows, W], [3, rows, W], [rows, W]); None where not wanted."""
    npdt, _ = _dt(prec)
    s, sp = _arr(spheres5, npdt)
    m, mp = _arr(materials8, npdt)
    t, tp = _arr(triangles10, npdt)
    c, cp = _arr(camera12, npdt)
    outs, ptrs = _feature_outputs(params, npdt, want_albedo, want_normal, want_depth)
    fn = lib().spira_render_features_f32 if prec == "f32" else lib().spira_render_features_f64
    _check(fn(sp, mp, tp, cp, C.byref(params), *ptrs))
    return outs


def make_denoise(width, height, iterations=5, post=POST_ACES, sigma_l=4.0, sigma_z=0.1):
    return Denoise(width, height, iterations, post, sigma_l, sigma_z)


def denoise(color, dn, variance=None, albedo=None, normal=None, depth=None, prec="f32", want_hdr=True, want_img=False, in_place=False):
    """spira_denoise_*: host planes in, host planes out.  color [3, H, W]; variance / depth [H, W] and albedo / normal [3, H, W] or None.
    Returns (hdr, img); in_place: out_hdr is `color` itself (it must then be a contiguous array of the call's precision, and is overwritten)."""
    npdt, _ = _dt(prec)
    if in_place:
        assert want_hdr and color.dtype == npdt and color.flags["C_CONTIGUOUS"]
    c, cp = _arr(color, npdt)
    arrs = [_arr(x, npdt) for x in (variance, albedo, normal, depth)]
    shape = (3, dn.height, dn.width)
    assert c.shape == shape
    for (x, _), want in zip(arrs, (shape[1:], shape, shape, shape[1:])):
        assert x is None or x.shape == want
    hdr = c if in_place else (np.empty(shape, dtype=npdt) if want_hdr else None)
    img = np.empty(shape, dtype=npdt) if want_img else None
    fn = lib().spira_denoise_f32 if prec == "f32" else lib().spira_denoise_f64
    _check(fn(cp, arrs[0][1], arrs[1][1], arrs[2][1], arrs[3][1], C.byref(dn), hdr.ctypes.data_as(C.c_void_p) if hdr is not None else None,
              img.ctypes.data_as(C.c_void_p) if img is not None else None))
    return hdr, img


def denoise_device(d_color_ptr, dn, d_out_hdr_ptr, d_out_img_ptr, stream_ptr, d_variance_ptr=0, d_albedo_ptr=0, d_normal_ptr=0, d_depth_ptr=0, prec="f32"):
    """spira_denoise_device_*: DEVICE plane addresses (0 / None: not given / not wanted); enqueues on the stream and returns."""
    fn = lib().spira_denoise_device_f32 if prec == "f32" else lib().spira_denoise_device_f64
    _check(fn(C.c_void_p(d_color_ptr or None), C.c_void_p(d_variance_ptr or None), C.c_void_p(d_albedo_ptr or None), C.c_void_p(d_normal_ptr or None),
              C.c_void_p(d_depth_ptr or None), C.byref(dn), C.c_void_p(d_out_hdr_ptr or None), C.c_void_p(d_out_img_ptr or None), C.c_void_p(stream_ptr or None)))


def make_adaptive(min_spp, batch_spp, tolerance, floor=0.0):
    return Adaptive(min_spp, batch_spp, tolerance, floor)


def _adaptive_outputs(params, npdt, want_hdr, want_img, want_spp, want_q):
    rows = params.rows if params.rows else params.height
    outs = (np.empty((3, rows, params.width), dtype=npdt) if want_hdr else None, np.empty((3, rows, params.width), dtype=npdt) if want_img else None,
            np.empty((rows, params.width), dtype=np.uint32) if want_spp else None, np.empty((rows, params.width), dtype=npdt) if want_q else None)
    return outs, [o.ctypes.data_as(C.c_void_p) if o is not None else None for o in outs]


def render_adaptive(spheres5, materials8, triangles10, camera12, params, adaptive, prec="f32", want_hdr=True, want_img=False, want_spp=True, want_q=True):
    """spira_render_adaptive_*: host arrays, host outputs.  params.spp is the cap.  Returns (hdr, img, spp, q): the mean over each pixel's own
    sample count [3, rows, W], its display transform, the samples taken (uint32 [rows, W]) and the final Q [rows, W]; None where not wanted."""
    npdt, _ = _dt(prec)
    s, sp = _arr(spheres5, npdt)
    m, mp = _arr(materials8, npdt)
    t, tp = _arr(triangles10, npdt)
    c, cp = _arr(camera12, npdt)
    outs, ptrs = _adaptive_outputs(params, npdt, want_hdr, want_img, want_spp, want_q)
    fn = lib().spira_render_adaptive_f32 if prec == "f32" else lib().spira_render_adaptive_f64
    _check(fn(sp, mp, tp, cp, C.byref(params), C.byref(adaptive), *ptrs))
    return outs


def adaptive_converged(sum3, q, n, tolerance, floor, prec="f32"):
    """spira_adaptive_converged_*: the stopping rule as the library's host arithmetic, for ONE pixel (1, 0; raises on an error code)."""
    npdt, cdt = _dt(prec)
    s = np.ascontiguousarray(sum3, dtype=npdt)
    assert s.shape == (3,)
    fn = lib().spira_adaptive_converged_f32 if prec == "f32" else lib().spira_adaptive_converged_f64
    fn.argtypes = [C.c_void_p, cdt, C.c_uint32, C.c_double, C.c_double]
    rc = fn(s.ctypes.data_as(C.c_void_p), cdt(q), C.c_uint32(n), C.c_double(tolerance), C.c_double(floor))
    if rc < 0:
        _check(rc)
    return rc


def accumulate(spheres5, materials8, triangles10, camera12, params, sample0, sum_rgb, rng_states=None, prec="f32"):
    """Progressive accumulation: adds samples [sample0, sample0 + params.spp) to sum_rgb ([3, rows, W], in place)."""
    npdt, _ = _dt(prec)
    s, sp = _arr(spheres5, npdt)
    m, mp = _arr(materials8, npdt)
    t, tp = _arr(triangles10, npdt)
    c, cp = _arr(camera12, npdt)
    assert sum_rgb.dtype == npdt and sum_rgb.flags["C_CONTIGUOUS"]
    rp = None
    if rng_states is not None:
        assert rng_states.dtype == np.uint32 and rng_states.flags["C_CONTIGUOUS"]
        rp = rng_states.ctypes.data_as(C.c_void_p)
    fn = lib().spira_accumulate_f32 if prec == "f32" else lib().spira_accumulate_f64
    _check(fn(sp, mp, tp, cp, C.byref(params), C.c_uint32(sample0), sum_rgb.ctypes.data_as(C.c_void_p), rp))
    return sum_rgb


def trace_paths(spheres5, materials8, triangles10, camera12, params, ijs, prec="f32"):
    """Diagnostic: per-segment (prims, ts, dirs) and radiance of the paths ijs = [[i, j, sample], ...]."""
    npdt, _ = _dt(prec)
    s, sp = _arr(spheres5, npdt)
    m, mp = _arr(materials8, npdt)
    t, tp = _arr(triangles10, npdt)
    c, cp = _arr(camera12, npdt)
    ij = np.ascontiguousarray(ijs, dtype=np.uint32).reshape(-1, 3)
    n, d = ij.shape[0], params.max_depth
    prims = np.zeros((n, d), dtype=np.int32)
    ts = np.zeros((n, d), dtype=npdt)
    dirs = np.zeros((n, d, 3), dtype=npdt)
    rad = np.zeros((n, 3), dtype=npdt)
    fn = lib().spira_trace_paths_f32 if prec == "f32" else lib().spira_trace_paths_f64
    _check(fn(sp, mp, tp, cp, C.byref(params), C.c_uint32(n), ij.ctypes.data_as(C.c_void_p),
              prims.ctypes.data_as(C.c_void_p), ts.ctypes.data_as(C.c_void_p), dirs.ctypes.data_as(C.c_void_p),
              rad.ctypes.data_as(C.c_void_p)))
    return prims, ts, dirs, rad


def tonemap(values, post):
    v = np.ascontiguousarray(values, dtype=np.float32).copy()
    _check(lib().spira_tonemap_f32(v.ctypes.data_as(C.c_void_p), C.c_uint64(v.size), C.c_uint32(post)))
    return v


def closest_point_triangle(v0, e1, e2, p, prec):
    """spira_closest_point_triangle_*: the library's triangle function on one triangle (v0, e1 = v1 - v0, e2 = v2 - v0) and one point, as host arithmetic
    (no device needed).  Returns (q [3], d2) in the precision's dtype."""
    npdt, _ = _dt(prec)
    a = [np.ascontiguousarray(x, dtype=npdt).reshape(3) for x in (v0, e1, e2, p)]
    q, d2 = np.empty(3, dtype=npdt), np.empty(1, dtype=npdt)
    fn = lib().spira_closest_point_triangle_f32 if prec == "f32" else lib().spira_closest_point_triangle_f64
    fn.restype = None
    fn(*[x.ctypes.data_as(C.c_void_p) for x in a], q.ctypes.data_as(C.c_void_p), d2.ctypes.data_as(C.c_void_p))
    return q, d2[0]


def sweep_sphere_triangle(v0, e1, e2, o, d_unit, r, t_min, t_max, prec):
    """spira_sweep_sphere_triangle_*: the library's leaf function of the sphere sweeps on one triangle (v0, e1 = v1 - v0, e2 = v2 - v0) and one sweep
    (origin o, UNIT direction, radius r, t_min, t_max), as host arithmetic (no device needed).  Returns (t, q [3], hit) in the precision's dtype."""
    npdt, ct = _dt(prec)
    a = [np.ascontiguousarray(x, dtype=npdt).reshape(3) for x in (v0, e1, e2, o, d_unit)]
    t, q, hit = np.empty(1, dtype=npdt), np.empty(3, dtype=npdt), C.c_int(0)
    fn = lib().spira_sweep_sphere_triangle_f32 if prec == "f32" else lib().spira_sweep_sphere_triangle_f64
    fn.restype = None
    fn.argtypes = [C.c_void_p] * 5 + [ct] * 3 + [C.c_void_p, C.c_void_p, C.c_void_p]
    fn(*[x.ctypes.data_as(C.c_void_p) for x in a], ct(npdt(r)), ct(npdt(t_min)), ct(npdt(t_max)), t.ctypes.data_as(C.c_void_p), q.ctypes.data_as(C.c_void_p),
       C.cast(C.byref(hit), C.c_void_p))
    return t[0], q, bool(hit.value)


def overlap_box_triangle(v0, e1, e2, box10, prec):
    """spira_overlap_box_triangle_*: the library's leaf function of the box overlap queries on one triangle (v0, e1 = v1 - v0, e2 = v2 - v0) and one box
    [cx cy cz hx hy hz qx qy qz qw], as host arithmetic (no device needed).  Returns 1, 0, or RAY_INVALID for a box that is invalid without a frame."""
    npdt, _ = _dt(prec)
    a = [np.ascontiguousarray(x, dtype=npdt).reshape(3) for x in (v0, e1, e2)] + [np.ascontiguousarray(box10, dtype=npdt).reshape(10)]
    fn = lib().spira_overlap_box_triangle_f32 if prec == "f32" else lib().spira_overlap_box_triangle_f64
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p] * 4
    return int(fn(*[x.ctypes.data_as(C.c_void_p) for x in a]))


def overlap_box_sphere(centre, radius, box10, prec):
    """spira_overlap_box_sphere_*: the leaf function on one sphere (a shell) and one box, as host arithmetic.  Returns 1, 0 or RAY_INVALID."""
    npdt, ct = _dt(prec)
    c, b = np.ascontiguousarray(centre, dtype=npdt).reshape(3), np.ascontiguousarray(box10, dtype=npdt).reshape(10)
    fn = lib().spira_overlap_box_sphere_f32 if prec == "f32" else lib().spira_overlap_box_sphere_f64
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p, ct, C.c_void_p]
    return int(fn(c.ctypes.data_as(C.c_void_p), ct(npdt(radius)), b.ctypes.data_as(C.c_void_p)))


def overlap_tri_triangle(v0, e1, e2, query10, prec):
    """spira_overlap_tri_triangle_*: the library's leaf function of the triangle overlap queries on one scene triangle (v0, e1 = v1 - v0, e2 = v2 - v0) and
    one query [q0 q1 q2 mat], as host arithmetic (no device needed).  Returns 1, 0, or RAY_INVALID for a query that is invalid without a frame."""
    npdt, _ = _dt(prec)
    a = [np.ascontiguousarray(x, dtype=npdt).reshape(3) for x in (v0, e1, e2)] + [np.ascontiguousarray(query10, dtype=npdt).reshape(10)]
    fn = lib().spira_overlap_tri_triangle_f32 if prec == "f32" else lib().spira_overlap_tri_triangle_f64
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p] * 4
    return int(fn(*[x.ctypes.data_as(C.c_void_p) for x in a]))


def overlap_tri_sphere(centre, radius, query10, prec):
    """spira_overlap_tri_sphere_*: the leaf function on one sphere (a shell) and one query, as host arithmetic.  Returns 1, 0 or RAY_INVALID."""
    npdt, ct = _dt(prec)
    c, q = np.ascontiguousarray(centre, dtype=npdt).reshape(3), np.ascontiguousarray(query10, dtype=npdt).reshape(10)
    fn = lib().spira_overlap_tri_sphere_f32 if prec == "f32" else lib().spira_overlap_tri_sphere_f64
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p, ct, C.c_void_p]
    return int(fn(c.ctypes.data_as(C.c_void_p), ct(npdt(radius)), q.ctypes.data_as(C.c_void_p)))
