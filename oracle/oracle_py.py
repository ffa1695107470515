"""ctypes loader for oracle/libspira_oracle.so — TEST INFRASTRUCTURE ONLY.

Only tests/, __graft_entry__.smoke() and bench.py's cpu_baseline leg import this module.
The product package (julia-spira_amd/) never does.
"""
import ctypes as C
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = None


class SpiraParams(C.Structure):
    """Mirror of spira_params (include/spira_hip.h); the product binding has its own copy."""
    _fields_ = [("width", C.c_uint32), ("height", C.c_uint32), ("spp", C.c_uint32), ("max_depth", C.c_uint32),
                ("n_spheres", C.c_uint32), ("n_materials", C.c_uint32), ("n_triangles", C.c_uint32),
                ("flags", C.c_uint32), ("seed", C.c_uint64), ("row0", C.c_uint32), ("rows", C.c_uint32),
                ("stripe_h", C.c_uint32), ("stripe_count", C.c_uint32), ("stripe_rank", C.c_uint32),
                ("batch_rays", C.c_uint32)]


def build():
    subprocess.run(["make", "-C", _HERE, "-s"], check=True)


def lib():
    global _LIB
    if _LIB is None:
        path = os.path.join(_HERE, "libspira_oracle.so")
        if not os.path.exists(path):
            build()
        _LIB = C.CDLL(path)
        _LIB.oracle_lcg_next.restype = C.c_uint32
        _LIB.oracle_lcg_next.argtypes = [C.c_uint32]
        _LIB.oracle_lcg_uniform.restype = C.c_float
        _LIB.oracle_lcg_uniform.argtypes = [C.c_uint32]
        _LIB.oracle_xorshift32.restype = C.c_uint32
        _LIB.oracle_xorshift32.argtypes = [C.c_uint32]
        _LIB.oracle_xorshift_uniform.restype = C.c_float
        _LIB.oracle_xorshift_uniform.argtypes = [C.c_uint32]
        _LIB.oracle_mix32_export.restype = C.c_uint32
        _LIB.oracle_mix32_export.argtypes = [C.c_uint32]
        _LIB.oracle_post_f32.restype = C.c_float
        _LIB.oracle_post_f32.argtypes = [C.c_float, C.c_uint32]
        _LIB.oracle_post_f64.restype = C.c_double
        _LIB.oracle_post_f64.argtypes = [C.c_double, C.c_uint32]
    return _LIB


def _dt(prec):
    return (np.float64, C.c_double, "_f64") if prec == "f64" else (np.float32, C.c_float, "_f32")


def _arr(a, dtype):
    if a is None:
        return None, None
    a = np.ascontiguousarray(a, dtype=dtype)
    return a, a.ctypes.data_as(C.c_void_p)


def make_params(width, height, spp, max_depth, n_spheres, n_materials, n_triangles=0, flags=0, seed=0,
                row0=0, rows=0, stripe_h=0, stripe_count=0, stripe_rank=0):
    return SpiraParams(width, height, spp, max_depth, n_spheres, n_materials, n_triangles, flags, seed,
                       row0, rows, stripe_h, stripe_count, stripe_rank, 0)


def render(spheres5, materials8, triangles10, camera12, params, prec="f64", n_threads=0, want_img=False):
    """Returns (hdr[3,rows,W], img or None, segments)."""
    npdt, cdt, suf = _dt(prec)
    s, sp = _arr(spheres5, npdt)
    m, mp = _arr(materials8, npdt)
    t, tp = _arr(triangles10, npdt)
    c, cp = _arr(camera12, npdt)
    rows = params.rows if params.rows else params.height
    hdr = np.empty((3, rows, params.width), dtype=npdt)
    img = np.empty((3, rows, params.width), dtype=npdt) if want_img else None
    seg = C.c_uint64(0)
    fn = getattr(lib(), "oracle_render" + suf)
    fn.restype = C.c_int
    rc = fn(sp, mp, tp, cp, C.byref(params), hdr.ctypes.data_as(C.c_void_p),
            img.ctypes.data_as(C.c_void_p) if want_img else None, C.c_int(n_threads), C.byref(seg))
    if rc != 0:
        raise RuntimeError("oracle_render%s failed: %d" % (suf, rc))
    return hdr, img, seg.value


def trace_path(spheres5, materials8, triangles10, camera12, params, i, j, sample, prec="f32"):
    """One path: (n_segments, prims[max_depth], ts, dirs[max_depth,3], radiance[3]); i, j 1-based."""
    npdt, cdt, suf = _dt(prec)
    s, sp = _arr(spheres5, npdt)
    m, mp = _arr(materials8, npdt)
    t, tp = _arr(triangles10, npdt)
    c, cp = _arr(camera12, npdt)
    d = params.max_depth
    prims = np.zeros(d, dtype=np.int32)
    ts = np.zeros(d, dtype=npdt)
    dirs = np.zeros((d, 3), dtype=npdt)
    rad = np.zeros(3, dtype=npdt)
    fn = getattr(lib(), "oracle_trace_path" + suf)
    fn.restype = C.c_int
    n = fn(sp, mp, tp, cp, C.byref(params), C.c_uint32(i), C.c_uint32(j), C.c_uint32(sample),
           prims.ctypes.data_as(C.c_void_p), ts.ctypes.data_as(C.c_void_p), dirs.ctypes.data_as(C.c_void_p),
           rad.ctypes.data_as(C.c_void_p))
    return n, prims, ts, dirs, rad


def render_variant(spheres5, materials8, camera12, params, prec="f32", n_threads=0, want_img=False, want_states=False):
    """SPIRA_SEM_CPU / SPIRA_SEM_METAL restatements (params.flags selects).  Returns (hdr, img or None, segments), and with want_states
    (SPIRA_SEM_METAL) a fourth item: the per-pixel LCG states after the last sample, uint32 [rows * W] in output order."""
    npdt, cdt, suf = _dt(prec)
    s, sp = _arr(spheres5, npdt)
    m, mp = _arr(materials8, npdt)
    c, cp = _arr(camera12, npdt)
    rows = params.rows if params.rows else params.height
    hdr = np.empty((3, rows, params.width), dtype=npdt)
    img = np.empty((3, rows, params.width), dtype=npdt) if want_img else None
    seg = C.c_uint64(0)
    states = np.zeros(rows * params.width, dtype=np.uint32) if want_states else None
    args = (sp, mp, cp, C.byref(params), hdr.ctypes.data_as(C.c_void_p), img.ctypes.data_as(C.c_void_p) if want_img else None,
            C.c_int(n_threads), C.byref(seg))
    if want_states:                                   # the nine-argument entry; the eight-argument one is unchanged
        fn = getattr(lib(), "oracle_render_variant_states" + suf)
        args += (states.ctypes.data_as(C.c_void_p),)
    else:
        fn = getattr(lib(), "oracle_render_variant" + suf)
    fn.restype = C.c_int
    rc = fn(*args)
    if rc != 0:
        raise RuntimeError("oracle_render_variant%s failed: %d" % (suf, rc))
    if want_states:
        return hdr, img, seg.value, states
    return hdr, img, seg.value


def render_hybrid(spheres5, materials8, camera12, params, prec="f32", n_threads=0):
    """SPIRA_SEM_HYBRID: render_hybrid_gpu of src/spira-metal-optimized.jl:1228-1343 as written (whole images only).  Returns (image, segments);
    the image is the reference's: the mean of per-sample tone-mapped colours, rows in the order the flags ask for."""
    npdt, cdt, suf = _dt(prec)
    s, sp = _arr(spheres5, npdt)
    m, mp = _arr(materials8, npdt)
    c, cp = _arr(camera12, npdt)
    hdr = np.empty((3, params.height, params.width), dtype=npdt)
    seg = C.c_uint64(0)
    fn = getattr(lib(), "oracle_render_hybrid" + suf)
    fn.restype = C.c_int
    rc = fn(sp, mp, cp, C.byref(params), hdr.ctypes.data_as(C.c_void_p), None, C.c_int(n_threads), C.byref(seg))
    if rc != 0:
        raise RuntimeError("oracle_render_hybrid%s failed: %d" % (suf, rc))
    return hdr, seg.value


def trace_path_variant(spheres5, materials8, camera12, params, i, j, sample, prec="f32"):
    npdt, cdt, suf = _dt(prec)
    s, sp = _arr(spheres5, npdt)
    m, mp = _arr(materials8, npdt)
    c, cp = _arr(camera12, npdt)
    d = params.max_depth
    prims = np.zeros(d, dtype=np.int32)
    ts = np.zeros(d, dtype=npdt)
    dirs = np.zeros((d, 3), dtype=npdt)
    rad = np.zeros(3, dtype=npdt)
    fn = getattr(lib(), "oracle_trace_path_variant" + suf)
    fn.restype = C.c_int
    n = fn(sp, mp, cp, C.byref(params), C.c_uint32(i), C.c_uint32(j), C.c_uint32(sample), prims.ctypes.data_as(C.c_void_p),
           ts.ctypes.data_as(C.c_void_p), dirs.ctypes.data_as(C.c_void_p), rad.ctypes.data_as(C.c_void_p))
    return n, prims, ts, dirs, rad


def sincos_turn(r, prec="f64"):
    npdt, cdt, suf = _dt(prec)
    out = np.zeros(2, dtype=npdt)
    fn = getattr(lib(), "oracle_sincos_turn" + suf)
    fn.restype = None
    fn(cdt(r), out.ctypes.data_as(C.c_void_p))
    return out


def camera(position, look_at, up, fov_deg, aspect_ratio, focus_dist=1.0, prec="f64"):
    npdt, cdt, suf = _dt(prec)
    p, pp = _arr(position, npdt)
    l, lp = _arr(look_at, npdt)
    u, up_ = _arr(up, npdt)
    out = np.zeros(12, dtype=npdt)
    fn = getattr(lib(), "oracle_camera" + suf)
    fn.restype = None
    fn(pp, lp, up_, cdt(fov_deg), cdt(aspect_ratio), cdt(focus_dist), out.ctypes.data_as(C.c_void_p))
    return out


def hit_sphere(s5, o, d, t_min, t_max, prec="f64"):
    npdt, cdt, suf = _dt(prec)
    s, sp = _arr(s5, npdt)
    o_, op = _arr(o, npdt)
    d_, dp = _arr(d, npdt)
    t = cdt(0)
    n = np.zeros(3, dtype=npdt)
    fn = getattr(lib(), "oracle_hit_sphere" + suf)
    fn.restype = C.c_int
    hit = fn(sp, op, dp, cdt(t_min), cdt(t_max), C.byref(t), n.ctypes.data_as(C.c_void_p))
    return bool(hit), t.value, n


def hit_triangle(t10, o, d, t_min, t_max, prec="f64"):
    npdt, cdt, suf = _dt(prec)
    s, sp = _arr(t10, npdt)
    o_, op = _arr(o, npdt)
    d_, dp = _arr(d, npdt)
    t = cdt(0)
    n = np.zeros(3, dtype=npdt)
    fn = getattr(lib(), "oracle_hit_triangle" + suf)
    fn.restype = C.c_int
    hit = fn(sp, op, dp, cdt(t_min), cdt(t_max), C.byref(t), n.ctypes.data_as(C.c_void_p))
    return bool(hit), t.value, n


def sky(d, prec="f64"):
    npdt, cdt, suf = _dt(prec)
    d_, dp = _arr(d, npdt)
    out = np.zeros(3, dtype=npdt)
    fn = getattr(lib(), "oracle_sky" + suf)
    fn.restype = None
    fn(dp, out.ctypes.data_as(C.c_void_p))
    return out


def post(x, post_flag, prec="f64"):
    return getattr(lib(), "oracle_post_" + prec)(x, post_flag)


def rng_try(seed, pixel, sample, bounce, t, prec="f64"):
    npdt, cdt, suf = _dt(prec)
    out = np.zeros(3, dtype=npdt)
    fn = getattr(lib(), "oracle_rng_try" + suf)
    fn.restype = None
    fn(C.c_uint64(seed), C.c_uint32(pixel), C.c_uint32(sample), C.c_uint32(bounce), C.c_uint32(t),
       out.ctypes.data_as(C.c_void_p))
    return out


def max_threads():
    fn = lib().oracle_max_threads
    fn.restype = C.c_int
    return fn()


# ---------------------------------------------------------------------------------------------------------------------------------------
# oracle/_ref: the reference's own src/spira_path_trace_kernel.metal compiled for the CPU (`make -C oracle _ref`; oracle/Makefile says how,
# oracle/ref_metal/ holds the stand-in header and the driver).  Built only where a reference checkout exists; the libraries travel, the
# checkout need not.  What SPIRA_SEM_METAL of the oracle and of the kernels is pinned to.
_REF_DIR = os.path.join(_HERE, "_ref")
_REF_LIBS = {}
REF_METAL_BUILDS = {"f32": "f32", "f64": "f64", "f64pi": "f64"}     # build name -> precision of its arrays


def reference_candidates():
    """Where a reference checkout is looked for, in order: $REFERENCE; a directory `reference` beside the repository or beside one of its parent
    directories; ~/reference; /root/reference (the place this project's line citations name)."""
    out = [os.environ["REFERENCE"]] if os.environ.get("REFERENCE") else []
    d = os.path.dirname(_HERE)
    while os.path.dirname(d) != d:
        d = os.path.dirname(d)
        out.append(os.path.join(d, "reference"))
    out += [os.path.join(os.path.expanduser("~"), "reference"), "/root/reference"]
    return [p for i, p in enumerate(out) if p not in out[:i]]


def find_reference():
    """The first candidate that holds src/spira_path_trace_kernel.metal, or None."""
    for p in reference_candidates():
        if os.path.isfile(os.path.join(p, "src", "spira_path_trace_kernel.metal")):
            return p
    return None


def build_ref():
    """`make -C oracle _ref` on the checkout find_reference() finds (a $REFERENCE that holds no checkout is an error, not a reason to build
    nothing); leaves oracle/_ref/SEARCHED.txt: where it looked and what it found.  Returns the checkout or None."""
    ref = find_reference()
    if os.environ.get("REFERENCE") and ref != os.environ["REFERENCE"]:
        raise RuntimeError("REFERENCE=%s holds no src/spira_path_trace_kernel.metal" % os.environ["REFERENCE"])
    os.makedirs(_REF_DIR, exist_ok=True)
    with open(os.path.join(_REF_DIR, "SEARCHED.txt"), "w") as f:
        f.write("found: %s\nlooked in: %s\n" % (ref, ", ".join(reference_candidates())))
    subprocess.run(["make", "-C", _HERE, "_ref"] + (["REFERENCE=" + ref] if ref else []), check=True)
    if ref and not ref_metal_available():
        raise RuntimeError("reference checkout at %s, but make -C oracle _ref left no libraries in oracle/_ref" % ref)
    return ref


def reference_search_record():
    """What build_ref() wrote, in one line (for skip reasons and failure messages)."""
    try:
        with open(os.path.join(_REF_DIR, "SEARCHED.txt")) as f:
            return "; ".join(l.strip() for l in f if l.strip())
    except OSError:
        return "build_ref() has not run: no oracle/_ref/SEARCHED.txt"


def ref_metal_path(build):
    return os.path.join(_REF_DIR, "libspira_ref_metal_%s.so" % build)


def ref_metal_available():
    """True when every reference library is there.  Never builds (callers skip when False)."""
    return all(os.path.exists(ref_metal_path(b)) for b in REF_METAL_BUILDS)


def _ref_lib(build):
    if build not in _REF_LIBS:
        if build not in REF_METAL_BUILDS:
            raise ValueError("unknown reference build %r" % (build,))
        l = C.CDLL(ref_metal_path(build))
        l.ref_metal_real_bytes.restype = C.c_int
        assert l.ref_metal_real_bytes() == (4 if REF_METAL_BUILDS[build] == "f32" else 8)
        l.ref_metal_accumulate.restype = C.c_int
        l.ref_metal_unit_vector.restype = C.c_uint32
        _REF_LIBS[build] = l
    return _REF_LIBS[build]


def _mix32(x):
    x = np.asarray(x, dtype=np.uint32).copy()
    x ^= x >> np.uint32(16); x *= np.uint32(0x7feb352d)
    x ^= x >> np.uint32(15); x *= np.uint32(0x846ca68b)
    x ^= x >> np.uint32(16)
    return x


def metal_state0(seed, pixels):
    """Python twin of metal_state0 (oracle/spira_oracle_impl.h; the kernels' is the same): the initial LCG state of each pixel id
    (pixel = gid.y * W + gid.x), derived from the 64-bit seed."""
    with np.errstate(over="ignore"):
        lo, hi = np.uint32(seed & 0xFFFFFFFF), np.uint32((seed >> 32) & 0xFFFFFFFF)
        sA = _mix32(_mix32(lo + np.uint32(0x9E3779B9)) ^ hi)
        sB = _mix32(_mix32(hi + np.uint32(0x85EBCA6B)) ^ lo)
        return _mix32(_mix32(sA + np.asarray(pixels, dtype=np.uint32)) ^ sB)


def ref_metal(spheres5, materials8, camera12, width, height, spp, max_depth, seed=0, build="f32", sample0=0, sums=None, states=None):
    """`path_trace` of the reference, once per pixel and sample.  Returns (sums [3, H, W], states [H * W]): the ACCUMULATED radiance
    (the kernel's `output += L`; divide by the sample count for a mean) and the LCG states after the last sample, row = gid.y (row 0 is
    v = 0: what SPIRA_ROWS_BOTTOM_UP delivers).  states None: seeded like the oracle (metal_state0); pass both back in to continue."""
    npdt, cdt, _ = _dt(REF_METAL_BUILDS[build])
    s, sp = _arr(spheres5, npdt)
    m, mp = _arr(materials8, npdt)
    c, cp = _arr(camera12, npdt)
    n = width * height
    states = metal_state0(seed, np.arange(n)) if states is None else np.ascontiguousarray(states, dtype=np.uint32).copy()
    inter = np.zeros((n, 3), dtype=npdt) if sums is None else np.ascontiguousarray(np.moveaxis(np.asarray(sums, dtype=npdt), 0, -1).reshape(n, 3)).copy()
    rc = _ref_lib(build).ref_metal_accumulate(sp, C.c_uint32(len(s)), mp, C.c_uint32(len(m)), cp, C.c_uint32(width), C.c_uint32(height),
                                              C.c_uint32(spp), C.c_uint32(max_depth), C.c_uint32(sample0),
                                              states.ctypes.data_as(C.c_void_p), inter.ctypes.data_as(C.c_void_p))
    if rc != 0:
        raise RuntimeError("ref_metal_accumulate failed: %d" % rc)
    return np.ascontiguousarray(np.moveaxis(inter.reshape(height, width, 3), -1, 0)), states


def ref_metal_unit_vector(state, build="f32"):
    """The order guard's probe: one call of the file's random_unit_vector from `state`.  Returns (xyz, state afterwards)."""
    npdt, cdt, _ = _dt(REF_METAL_BUILDS[build])
    out = np.zeros(3, dtype=npdt)
    st = _ref_lib(build).ref_metal_unit_vector(C.c_uint32(state), out.ctypes.data_as(C.c_void_p))
    return out, int(st)
