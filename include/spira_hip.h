/*
 * spira_hip.h — C ABI of libspira_hip.so, the MI355X (gfx950) path-trace backend for SPIRA.
 *
 * This is the drop-in boundary for ONE hot path of jenkinsm13/julia-spira: the per-pixel
 * Monte-Carlo path-trace integrator.  The reference has no FFI of its own (it is pure Julia);
 * the boundary is the Julia function surface, so every entry point below names the reference
 * function(s) it replaces (paths relative to the reference repo root):
 *
 *   spira_render_f32 / spira_render_device_f32
 *       replaces  render_hybrid_gpu(width,height,scene,camera; samples_per_pixel,max_depth)
 *                 src/spira-metal-optimized.jl:1228-1343   (the whole per-sample / per-depth
 *                 host loop with its K3..K10 kernels), reached from
 *                 render(scene,camera,W,H; ...)  src/spira-metal-optimized.jl:1453-1490
 *                 at the backend branch :1460-1479 (where `has_amdgpu` falls back to the CPU today),
 *       and       render(world,camera,W,H; samples_per_pixel,max_depth)
 *                 examples/julia-raytracer.jl:387-421 (the parity oracle's pixel loop).
 *   inputs        spheres5 / materials8 are exactly the flat arrays of
 *                 prepare_scene_data(scene)  src/spira-metal-optimized.jl:515-542;
 *                 camera12 is Camera_jl (origin, lower_left_corner, horizontal, vertical)
 *                 src/spira-metal-optimized.jl:360-365 == Camera fields :325-348 and
 *                 examples/julia-raytracer.jl:261-295;
 *                 triangles10 is [v0 v1 v2 material] per triangle, the flattened form of
 *                 Triangle(vertices, material) examples/julia-raytracer.jl:85-94.
 *   spira_render_f64 / spira_render_device_f64
 *       the same path computed in Float64, the precision of examples/julia-raytracer.jl.
 *   spira_camera_lookat_f32/_f64
 *       replaces  Camera(lookfrom,lookat,vup,vfov,aspect_ratio) src/spira-metal-optimized.jl:331-347
 *       and       Camera(; position, look_at, up, fov, aspect_ratio, focus_dist)
 *                 examples/julia-raytracer.jl:271-294.
 *   spira_tonemap_f32
 *       replaces  to_acescg examples/julia-raytracer.jl:370-384, gpu_tone_map_kernel!
 *                 src/spira-metal-optimized.jl:1128-1144 and the clamp+sqrt of
 *                 render_with_cpu :1441-1442.
 *   spira_accumulate_f32/_f64 (+ _device_)
 *       the progressive contract of src/spira_path_trace_kernel.metal:143-145,:252-268
 *       (current_sample_index, persisted rng_states, output += L), which no reference host code drives.
 *   flags & SPIRA_SEM_MASK selects which of the reference's FOUR estimators runs:
 *       ray_color (examples/julia-raytracer.jl:328-367, default), trace_ray of render_with_cpu
 *       (src/spira-metal-optimized.jl:1351-1412), path_trace (src/spira_path_trace_kernel.metal:140-269), render_hybrid_gpu's own
 *       (src/spira-metal-optimized.jl:1228-1343).
 *
 * Conventions: plain pointers and sizes only; every function returns 0 on success and a
 * negative SPIRA_E_* code otherwise; nothing throws, aborts or calls back across the ABI;
 * spira_last_error() returns a thread-local message.  Host-pointer entry points copy in/out;
 * *_device_* entry points take DEVICE pointers for the outputs (e.g. a torch tensor's
 * data_ptr()) plus the hipStream_t to run on (as void*; NULL = the null stream) and do not
 * synchronise.  Streams: all calls on one device share that device's workspaces (ray queues, radiance
 * buffers, the scene of host-array calls), so the library orders them itself — every call makes its
 * stream wait (hipStreamWaitEvent) for the end of the previous call on that device, whatever stream that
 * one ran on.  Calls on different streams are therefore safe without host synchronisation, and run one
 * after the other on the device.  There is NO CPU fallback: every render entry point fails with
 * SPIRA_E_NO_DEVICE when no HIP device is usable.
 */
#ifndef SPIRA_HIP_H
#define SPIRA_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SPIRA_ABI_VERSION 3      /* 3: spira_counters grew (rays_parked in round 3, the traversal counters and walk_kernel_ms in round 4) */

/* ---- error codes ---- */
#define SPIRA_OK            0
#define SPIRA_E_INVALID    -1   /* bad argument (null pointer, zero size, out-of-range index) */
#define SPIRA_E_NO_DEVICE  -2   /* no usable HIP device / runtime error at init */
#define SPIRA_E_HIP        -3   /* a HIP runtime call failed (see spira_last_error) */
#define SPIRA_E_LIMIT      -4   /* scene / parameters exceed a documented limit */
#define SPIRA_E_UNSUPPORTED -5  /* flag combination not implemented */

/* ---- flags (spira_params.flags) ---- */
/* integrator semantics (which of the reference's variants) */
#define SPIRA_SEM_MASK          0x0000000Fu
#define SPIRA_SEM_A             0x00000000u  /* examples/julia-raytracer.jl ray_color :328-367 (graded oracle) */
#define SPIRA_SEM_CPU           0x00000001u  /* render_with_cpu trace_ray src/spira-metal-optimized.jl:1351-1412 */
#define SPIRA_SEM_METAL         0x00000002u  /* path_trace src/spira_path_trace_kernel.metal:140-269 */
#define SPIRA_SEM_HYBRID        0x00000003u  /* render_hybrid_gpu src/spira-metal-optimized.jl:1228-1343 AS WRITTEN — what render() runs on a Metal / CUDA machine:
                                                the whole image in lock step (K3 raygen with per-pixel xorshift32 :610-697, K4 :700-799, the image-wide
                                                "nothing hit: end the sample" :1303, K5 scatter :862-989, contribution halved per depth :1328, K6 shade of
                                                the LAST bounce only :1071-1105, K7 ACES + sqrt per sample :1128-1144, K8 :1055-1068).  Restated, not
                                                repaired.  Spheres only, whole images only (rows == 0), no accumulate entry; out_hdr = out_img = the
                                                reference's (already tone-mapped) image; SPIRA_POST_* and SPIRA_KERNEL_* are ignored. */
/* kernel organisation */
#define SPIRA_KERNEL_MASK       0x000000F0u
#define SPIRA_KERNEL_DEFAULT    0x00000000u  /* the library's choice = the fastest organisation measured for the estimator:
                                                SPIRA_SEM_A: WAVEFRONT; SPIRA_SEM_METAL, SPIRA_SEM_CPU: one lane per pixel / path */
#define SPIRA_KERNEL_MEGA       0x00000010u  /* one lane walks whole paths in registers (with path regeneration) */
#define SPIRA_KERNEL_BOUNCE     0x00000020u  /* wavefront as in round 1: SoA RAY queues, one launch per bounce (comparison point) */
#define SPIRA_KERNEL_WAVEFRONT  0x00000030u  /* wavefront: SoA hit queues, ballot/popcount compaction, ONE persistent launch per pass in
                                                which every wave walks all bounces on its own queue region */
/* The organisation applies to SPIRA_SEM_A and, for WAVEFRONT vs the rest, to SPIRA_SEM_METAL (WAVEFRONT: every wave owns a block of
 * pixels and walks sample after sample on it, the LCG state travelling in the hit packet; otherwise one lane per pixel walks all its
 * samples — the faster form for that estimator).  SPIRA_SEM_CPU always runs one lane per path. */
/* display transform applied to out_img (out_hdr is always the linear mean) */
#define SPIRA_POST_MASK         0x00000F00u
#define SPIRA_POST_ACES         0x00000000u  /* clamp(aces(x),0,1)        examples/julia-raytracer.jl:370-384 */
#define SPIRA_POST_ACES_GAMMA   0x00000100u  /* sqrt(clamp(aces(x),0,1))  src/spira-metal-optimized.jl:1128-1144 */
#define SPIRA_POST_CLAMP_GAMMA  0x00000200u  /* sqrt(clamp(x,0,1))        src/spira-metal-optimized.jl:1441-1442 */
#define SPIRA_POST_NONE         0x00000300u  /* out_img = out_hdr */
/* row order of the outputs: default row 0 = image top, like hdr_data[height-j+1, i]
 * (examples/julia-raytracer.jl:408) and img[height-j+1, i] (src/spira-metal-optimized.jl:1445) */
#define SPIRA_ROWS_BOTTOM_UP    0x00001000u  /* row 0 = v=0 (bottom), the device-buffer order of :1177-1188 */

/* extensions.  The reference only NAMES these features (README.md:10, a comment at
 * src/spira_path_trace_kernel.metal:225): there is no reference code and so no parity to pin — the semantics below are the build's
 * own, restated in oracle/ and compared GPU vs oracle like everything else, and never part of the graded SPIRA_SEM_A runs.
 * SPIRA_SEM_A only; default (wavefront) and MEGA organisations. */
#define SPIRA_EXT_DIELECTRIC    0x00020000u  /* a material whose roughness is NEGATIVE is a smooth dielectric of refractive index
                                                -roughness, tinted by albedo: Snell refraction, Schlick reflectance, total internal
                                                reflection; one uniform draw per interaction picks reflection or refraction */
#define SPIRA_EXT_SPECTRAL      0x00040000u  /* hero-wavelength spectral transport: one wavelength per path (380..730 nm), RGB
                                                reflectance / emission / sky uplifted with the SPD tables of include/spira_spd.h
                                                (staged into LDS), radiance accumulated as linear sRGB through the wavelength's
                                                colour-matching response */

/* diagnostics */
#define SPIRA_FLAG_PROFILE      0x00010000u  /* SPIRA_KERNEL_BOUNCE: bracket every bounce launch with HIP events (slows the
                                                render).  The default organisation always brackets its one launch per pass, so
                                                spira_counters.bounce_kernel_ms is filled by every wavefront render. */

/* ---- limits ---- */
#define SPIRA_MAX_DEPTH        255u        /* bounce index is packed into 8 bits of the RNG key */
#define SPIRA_MAX_SPP          (1u << 24)  /* sample index is packed into 24 bits of the RNG key */
#define SPIRA_MAX_LDS_SPHERES  1024u        /* spheres are always an LDS-resident linear scan */
#define SPIRA_LDS_TRIANGLES    32u          /* up to this many triangles: LDS linear scan; more: device BVH */
#define SPIRA_MAX_TRIANGLES    (1u << 24)

/*
 * Render parameters: a superset of RenderParams_jl (src/spira-metal-optimized.jl:390-400).
 *
 * Tiling (multi-GPU): the image is width x height; this call renders `rows` output rows.
 * Output row r (0-based, in the row order chosen by the flags) of this call is global output
 * row  y = row0 + r                                   when stripe_count <= 1, and
 *      y = ((r / stripe_h) * stripe_count + stripe_rank) * stripe_h + (r % stripe_h)
 * when stripe_count > 1 (interleaved stripes of stripe_h rows, for load balance).  The RNG is
 * keyed by the GLOBAL pixel, so any tiling reproduces the untiled image bit for bit.
 * rows == 0 means "the whole image" (row0, stripe_* ignored).
 */
typedef struct spira_params {
    uint32_t width, height;
    uint32_t spp;            /* samples_per_pixel */
    uint32_t max_depth;      /* max_depth: maximum number of path segments */
    uint32_t n_spheres, n_materials, n_triangles;
    uint32_t flags;
    uint64_t seed;           /* absent in the reference (it never seeds its RNG) */
    uint32_t row0, rows;
    uint32_t stripe_h, stripe_count, stripe_rank;
    uint32_t batch_rays;     /* wavefront: target rays in flight per pass (0 = library default) */
} spira_params;              /* 64 bytes */

/* Counters of the last render on this thread's device context (for roofline arithmetic). */
typedef struct spira_counters {
    uint64_t samples;        /* camera paths started                                   */
    uint64_t segments;       /* path segments traced (ray/scene intersections)         */
    uint64_t rays_enqueued;  /* rays written to a queue (wavefront)                    */
    uint64_t radiance_rmw;   /* read-modify-writes of the per-path radiance (wavefront)*/
    uint64_t radiance_stores;/* plain 16/32-byte stores of the per-path radiance          */
    uint64_t passes;         /* wavefront passes                                       */
    uint64_t launches;       /* kernel launches                                        */
    double   kernel_ms;      /* device time of the render, HIP events on the render stream */
    double   bounce_kernel_ms;   /* device time spent in the dominant (bounce) kernel      */
    uint64_t bounce_launches;    /* launches of that kernel                                 */
    uint64_t redone_waves;       /* waves whose pass was rendered a second time with the compiler's division (speculative division) */
    uint64_t rays_parked;        /* mesh scenes: rays written to (and read back from) a wave's mesh list: 3 x 16/32 bytes each way */
    uint64_t mesh_wave_trips;    /* mesh scenes: trips of the traversal sessions' walk loop, summed over waves (one trip = one memory round trip of every walking lane) */
    uint64_t mesh_lane_trips;    /* ... and the lanes that took part in them: node visits + triangle tests; / (64 * mesh_wave_trips) = lane utilisation of the walk */
    double   walk_kernel_ms;     /* mesh scenes rendered as two launches: device time of the second (fat-wave, traversal) launches; part of bounce_kernel_ms */
} spira_counters;                /* 120 bytes */

/* ---- library / device ---- */
int         spira_abi_version(void);
const char *spira_build_id(void);             /* first 16 hex digits of the SHA-256 of the kernel sources + Makefile this library was built from (bench.py: which profile belongs to it) */
const char *spira_last_error(void);
int         spira_device_count(void);
int         spira_set_device(int device);      /* device used by subsequent calls on this thread */
int         spira_get_counters(spira_counters *out);
int         spira_get_sky_pixels(uint64_t *out);   /* of the same render: pixels of all-sky runs that k_path summed ahead of its loop (SPIRA_SKY_RUNS; 0 wherever no pixel-owning pass ran).  Beside spira_counters, whose layout stays */
int         spira_get_own_passes(uint64_t *out);   /* of the same render: passes that k_path_own rendered — full pixel-owning passes of 64 slots of a Float64 sphere scene (SPIRA_OWN_KERNEL; 0 wherever every pass ran k_path) */
void        spira_shutdown(void);              /* frees cached device workspaces */

/* ---- camera (host arithmetic only; no device needed) ---- */
/* out12 = origin, lower_left_corner, horizontal, vertical.  focus_dist = 1 reproduces the
 * five-argument constructor of src/spira-metal-optimized.jl:331. */
int spira_camera_lookat_f32(const float lookfrom[3], const float lookat[3], const float vup[3],
                            float vfov_deg, float aspect_ratio, float out12[12]);
int spira_camera_lookat_f64(const double position[3], const double look_at[3], const double up[3],
                            double fov_deg, double aspect_ratio, double focus_dist, double out12[12]);

/* ---- render: host pointers ---- */
/* spheres5:   n_spheres   x [cx cy cz r material_index(1-based, stored as a float)]
 * materials8: n_materials x [albedo r g b, emission r g b, metallic|specular, roughness]
 * triangles10:n_triangles x [v0 xyz, v1 xyz, v2 xyz, material_index(1-based)] or NULL
 * out_hdr, out_img: planar, 3 planes of rows*width values (R plane, G plane, B plane);
 *                   either may be NULL.  Scene objects are intersected in the order
 *                   spheres[0..], then triangles[0..] (ties: the later object wins, as in the
 *                   closest-hit scan of examples/julia-raytracer.jl:242-258). */
int spira_render_f32(const float *spheres5, const float *materials8, const float *triangles10,
                     const float camera12[12], const spira_params *params,
                     float *out_hdr, float *out_img);
int spira_render_f64(const double *spheres5, const double *materials8, const double *triangles10,
                     const double camera12[12], const spira_params *params,
                     double *out_hdr, double *out_img);

/* ---- render: device output pointers, asynchronous on `stream` ---- */
int spira_render_device_f32(const float *spheres5, const float *materials8, const float *triangles10,
                            const float camera12[12], const spira_params *params,
                            float *d_out_hdr, float *d_out_img, void *stream);
int spira_render_device_f64(const double *spheres5, const double *materials8, const double *triangles10,
                            const double camera12[12], const spira_params *params,
                            double *d_out_hdr, double *d_out_img, void *stream);

/* ---- multi-device render on ONE node ----
 * Replaces the backend branch of render (src/spira-metal-optimized.jl:1460-1479) for a host that owns several GPUs: the
 * frame is dealt to devices 0..n_devices-1 as interleaved single rows (spira_params "Tiling"; the RNG is keyed by the
 * global pixel, so the result is bit-identical to a one-device render), each device renders its tile on its own stream
 * driven by its own host thread inside the library, no collective runs while rendering, and ONE RCCL exchange (grouped
 * ncclSend / ncclRecv = a gather; n-1 point-to-point transfers over xGMI that arrive at device 0 at once) brings the tiles
 * to device 0, which permutes the rows back to image order and copies the frame to the caller's HOST buffers.
 * params->rows / stripe_* must be 0.  librccl.so.1 is opened at run time (the copy the process already carries, if any);
 * SPIRA_E_UNSUPPORTED when none can be found; the communicators of a device count are made once (ncclCommInitAll) and kept
 * until spira_shutdown.  Afterwards spira_get_counters reports the tile of the calling thread's current device
 * (spira_set_device(d) first for device d's).  A failed exchange aborts the communicators and returns SPIRA_E_HIP: it never hangs.
 * Status: one device through RCCL and n = 2, 3, 8 rehearsed on one device are tested; n > 1 on separate GPUs has not run yet
 * (no multi-GPU box in the build pipeline). */
int spira_render_multi_f32(const float *spheres5, const float *materials8, const float *triangles10,
                           const float camera12[12], const spira_params *params, int n_devices,
                           float *out_hdr, float *out_img);
int spira_render_multi_f64(const double *spheres5, const double *materials8, const double *triangles10,
                           const double camera12[12], const spira_params *params, int n_devices,
                           double *out_hdr, double *out_img);

/* ---- scene handles: validate, build (BVH) and upload a scene ONCE, render it many times ----
 * Replaces the per-render uploads `sphere_data_gpu = MtlArray(sphere_data)` / `material_data_gpu = ...` of
 * render_hybrid_gpu (src/spira-metal-optimized.jl:1247-1254) after prepare_scene_data (:515-542): the host-array
 * entry points above re-validate every material index and hash the whole triangle array on every call (to find
 * the cached BVH), which for an 82 k-triangle mesh is host milliseconds per frame; a handle pays that once.
 * A handle belongs to the device current at creation (spira_set_device) and to one precision.  With a handle,
 * params->n_spheres / n_materials / n_triangles are ignored. */
typedef struct spira_scene spira_scene;
int spira_scene_create_f32(const float *spheres5, const float *materials8, const float *triangles10,
                           uint32_t n_spheres, uint32_t n_materials, uint32_t n_triangles, spira_scene **out);
int spira_scene_create_f64(const double *spheres5, const double *materials8, const double *triangles10,
                           uint32_t n_spheres, uint32_t n_materials, uint32_t n_triangles, spira_scene **out);
int spira_scene_destroy(spira_scene *scene);       /* NULL is a no-op; waits for renders still using it */
/* The same for spira_render_multi_*: ONE validation, ONE BVH build on the host, the scene resident on devices 0 .. n_devices-1
 * (the host-array entry points re-validate, re-hash and, on first use, rebuild the tree per device per call).  The handle is
 * device 0's; spira_scene_destroy frees all copies.  It also works with the single-device entry points on device 0. */
int spira_scene_create_multi_f32(const float *spheres5, const float *materials8, const float *triangles10,
                                 uint32_t n_spheres, uint32_t n_materials, uint32_t n_triangles, int n_devices, spira_scene **out);
int spira_scene_create_multi_f64(const double *spheres5, const double *materials8, const double *triangles10,
                                 uint32_t n_spheres, uint32_t n_materials, uint32_t n_triangles, int n_devices, spira_scene **out);
int spira_render_multi_scene_f32(const spira_scene *scene, const float camera12[12], const spira_params *params, int n_devices,
                                 float *out_hdr, float *out_img);
int spira_render_multi_scene_f64(const spira_scene *scene, const double camera12[12], const spira_params *params, int n_devices,
                                 double *out_hdr, double *out_img);
/* New contents for a LIVE handle (an animated or deforming mesh): the arrays are replaced and the mesh's tree is REFITTED on the device — topology, slot
 * order and frame kept, every box recomputed bottom-up from the new vertices — instead of rebuilt on the host.  The tree only prunes, so a render after an
 * update is bit for bit the render of a fresh handle on the same arrays; what a refit costs is traversal time as the mesh leaves its build pose.
 * The counts (n_spheres, n_materials, n_triangles) and the precision are those of creation.
 * Host form: a NULL array means "unchanged" (all three NULL, or an array the scene was created without: SPIRA_E_INVALID); every array given is validated
 * exactly as spira_scene_create_* validates it, and triangles10 against the frame rule below, BEFORE anything on the device is touched.  Ordered like every
 * entry (renders still traversing the old tree finish first); returns when the scene is ready.
 * Device form: d_triangles10 is a DEVICE array in the triangles10 layout (e.g. a tensor a simulation wrote), read on `stream`.  A check kernel runs first
 * (finite vertices, material index in 1..n_materials, the frame rule); the entry SYNCHRONISES `stream` ONCE to read its status word — as the adaptive entries
 * do once per round — then enqueues the refit and returns without a second synchronisation; d_triangles10 must stay valid until that work has run.
 * A refused update (either form) leaves the handle rendering what it rendered before.
 * Frame rule: the normalised frame of a tree (centre, power-of-two scale) is fixed when the handle is created, with the mesh within about +-0.5 of it; an
 * update whose vertices leave |(x - centre) * scale| <= 1 on any axis is SPIRA_E_LIMIT — create a new handle for such a mesh.  That leaves room to move or
 * grow by about the mesh's own size.  A mesh of at most SPIRA_LDS_TRIANGLES triangles has no tree and no frame: its update is the new array.
 * Errors: the handle's other precision: SPIRA_E_INVALID; a handle made by spira_scene_create_multi_* (whatever its n_devices): SPIRA_E_UNSUPPORTED.
 * The host-array render entry points and their hash-keyed tree cache are not involved. */
int spira_scene_update_f32(spira_scene *scene, const float *spheres5, const float *materials8, const float *triangles10);
int spira_scene_update_f64(spira_scene *scene, const double *spheres5, const double *materials8, const double *triangles10);
int spira_scene_update_device_f32(spira_scene *scene, const float *d_triangles10, void *stream);
int spira_scene_update_device_f64(spira_scene *scene, const double *d_triangles10, void *stream);
/* A new triangle array for a LIVE handle, the mesh's tree built ANEW on the device (spira_lbvh.h): a new frame and a new topology, so there is NO frame rule
 * — the mesh may have walked across the scene or grown to any size — and no refit decay to carry along.  n_triangles and the precision are those of creation;
 * spheres and materials are untouched (spira_scene_update_* still changes them).  The build: exact vertex bounds -> the frame a fresh host build of the same
 * array would get, bit for bit -> 63-bit Morton keys of the centroids, sorted stably -> a binary radix tree (Karras 2012) -> its boxes, bottom-up ->
 * collapsed to the 8-wide slots by the host builder's rules -> the refit passes of spira_scene_update_* write every record and every box.  The tree only
 * prunes: a render after a rebuild is bit for bit the render of a fresh handle on the same arrays.  What differs is the topology (Morton order, not SAH) and
 * with it traversal time (README, docs/experiments.md section 24).  There is no automatic choice between refit and rebuild: the caller decides.
 * Validation is that of the update entries minus the frame rule: every vertex finite, every material index an integer in 1..n_materials, else SPIRA_E_INVALID.
 * Host form: validates on the host BEFORE the device is touched, stages the array, runs the same pipeline; returns when the scene is ready.
 * Device form: d_triangles10 is a DEVICE array in the triangles10 layout, read on `stream`.  A check kernel validates it and reduces the vertex bounds in the
 * same pass.  The entry SYNCHRONISES `stream` ONCE for that status and the bounds, and ONCE PER LEVEL of the new tree for the level's counts (4 levels of
 * 8-wide nodes for a sphere of 1 280 triangles; never more than 61); after the last of these it enqueues the remaining work and returns; d_triangles10 must
 * stay valid until that work has run.  Ordered like every entry: renders still walking the old tree finish first, a render enqueued after the call on any stream sees the new tree.
 * A REFUSED rebuild (either form) leaves the handle rendering what it rendered before: validation, a tree of 62 levels or more, more than 2^24 node slots, a
 * mesh so far from the origin for its size that its boxes cannot be padded in Float32 (SPIRA_E_LIMIT, as for an update) and a failed allocation all refuse
 * while only scratch memory of the device context has been written (kept until spira_shutdown, like the other workspaces).
 * A mesh of at most SPIRA_LDS_TRIANGLES triangles has no tree: its rebuild is the array copy, exactly as for the update.
 * Errors: a NULL or destroyed handle, the handle's other precision, a NULL array, a handle created without triangles: SPIRA_E_INVALID; a handle made by
 * spira_scene_create_multi_* (whatever its n_devices): SPIRA_E_UNSUPPORTED.
 * Afterwards the handle is an ordinary handle: spira_scene_update_* refits the NEW tree and applies the frame rule against the NEW frame, and every render,
 * feature and adaptive entry works on it. */
int spira_scene_rebuild_f32(spira_scene *scene, const float *triangles10);
int spira_scene_rebuild_f64(spira_scene *scene, const double *triangles10);
int spira_scene_rebuild_device_f32(spira_scene *scene, const float *d_triangles10, void *stream);
int spira_scene_rebuild_device_f64(spira_scene *scene, const double *d_triangles10, void *stream);
int spira_render_scene_f32(const spira_scene *scene, const float camera12[12], const spira_params *params,
                           float *out_hdr, float *out_img);
int spira_render_scene_f64(const spira_scene *scene, const double camera12[12], const spira_params *params,
                           double *out_hdr, double *out_img);
int spira_render_scene_device_f32(const spira_scene *scene, const float camera12[12], const spira_params *params,
                                  float *d_out_hdr, float *d_out_img, void *stream);
int spira_render_scene_device_f64(const spira_scene *scene, const double camera12[12], const spira_params *params,
                                  double *d_out_hdr, double *d_out_img, void *stream);

/* ---- ray queries on a scene handle: closest hit and occlusion for the CALLER'S rays (line of sight, range finding, visibility, picking) ----
 * Replaces hit(world, ray, t_min, t_max) of examples/julia-raytracer.jl:242-258 called once per ray: the same scan — spheres [0..) then triangles [0..)
 * in the caller's order, accepted when !(t < t_min || t > closest) with closest starting at t_max — answered for a whole ray list in one launch, a mesh of
 * more than SPIRA_LDS_TRIANGLES triangles through the handle's tree, which only prunes: prim and t are bit for bit the scan's.
 * rays8: n_rays x [ox oy oz t_min dx dy dz t_max].  Preparation per ray, in the call's precision T, nothing fused: s = (dx dx + dy dy) + dz dz,
 * d = (dx, dy, dz) / sqrt(s) — the library normalises (the walk assumes unit directions) and does not trust the caller; t, t_min and t_max are distances
 * along the UNIT direction.
 * Closest hit: the minimal t wins, ties go to the later object, a hit at exactly t_max counts.  out_prim: the object index, spheres first; out_t: that t;
 * out_normal (n_rays x 3, interleaved): the geometric normal of spira_render_features_* (outward normalize(pos - centre) for a sphere, the unflipped unit
 * normalize(cross(e1, e2)) for a triangle) at pos = o + d t.  A miss gives prim SPIRA_RAY_MISS, t = the ray's t_max copied, normal 0.
 * Invalid rays are ordinary input that the entry classifies — prim SPIRA_RAY_INVALID, t 0, normal 0; occlusion output 255 — they never fault and never
 * disturb their neighbours.  A ray is invalid when any of its eight values is NaN; an origin or direction component is infinite; s is not finite or is
 * below the smallest normal number of T; t_min < 0; t_max < t_min; or the origin rule is broken.
 * Origin rule (scenes WITH a tree only): |(o_k - centre_k) * scale| <= 64 on every axis, in T, with the tree's normalised frame (centre, power-of-two
 * scale; the mesh lies within about +-0.5 of it) — i.e. an origin within about 64 mesh sizes of the mesh.  Why: the walk starts from the point where the
 * ray enters the mesh's box, o + d te, computed in T, whose error is a few ulps of max(|o_k|, te); in normalised units that is in Float32 about
 * 3 (amax_n + 64) 2^-24 = 1.2e-5 + 1.8e-7 amax_n (amax_n: the largest coordinate of the mesh) against the builder's box padding of 1e-4 max(1, amax_n),
 * a margin of 8 or more.  A refitted tree (spira_scene_update_*) pads with max_k |centre_k| + 1 / scale in place of amax, which is never smaller for a mesh
 * inside its frame: the fresh build's margin is the smaller one and 64 covers both.  In Float64 (3 (amax_n + 64) 2^-53 against 1e-4 + 1e-9 amax_n) the bound
 * is far from binding and is kept for one contract.  A ray from further away: move its origin along the ray.  Scenes without a tree have no such rule.
 * Occlusion: out_hit[i] is 1 exactly where the closest-hit answer for the same ray would be prim >= 0, 0 otherwise, 255 for an invalid ray; the kernel
 * stops at the first accepted hit.
 * flags: 0, the library's organisation for scenes with a tree: persistent waves that each own a contiguous range of the ray list and refill their free
 * lanes from it while the others keep walking (a traversal session, as the renderer's); or SPIRA_CAST_INPLACE, one lane per ray walking to the end — the
 * comparison point, as SPIRA_KERNEL_BOUNCE is for the renderer.  Both give identical bytes.  Scenes without a tree run one lane per ray either way.
 * Errors, all decided before any device is touched: a NULL ray array, n_rays == 0, unknown flag bits, every output NULL (out_prim, out_t and out_normal may
 * each be NULL, not all three), a NULL or destroyed handle, one of the other precision or of another device: SPIRA_E_INVALID; n_rays > SPIRA_MAX_RAYS:
 * SPIRA_E_LIMIT.  A handle made by spira_scene_create_multi_* is served by device 0's copy, as the single-device render entries serve it.
 * The host form copies in and out and returns when the outputs are written.  The *_device_* form takes DEVICE pointers, is asynchronous on `stream`,
 * synchronises nothing, allocates nothing, and is ordered like every entry: a cast enqueued after a device-form update or rebuild on another stream sees
 * the new tree.  spira_get_counters is not affected by these entries. */
#define SPIRA_MAX_RAYS      (1u << 26)
#define SPIRA_RAY_MISS      -1
#define SPIRA_RAY_INVALID   -3          /* -2 is taken by spira_trace_paths */
#define SPIRA_CAST_INPLACE  0x1u
int spira_scene_cast_f32(const spira_scene *scene, const float *rays8, uint32_t n_rays, uint32_t flags,
                         int *out_prim, float *out_t, float *out_normal);
int spira_scene_cast_f64(const spira_scene *scene, const double *rays8, uint32_t n_rays, uint32_t flags,
                         int *out_prim, double *out_t, double *out_normal);
int spira_scene_cast_device_f32(const spira_scene *scene, const float *d_rays8, uint32_t n_rays, uint32_t flags,
                                int *d_out_prim, float *d_out_t, float *d_out_normal, void *stream);
int spira_scene_cast_device_f64(const spira_scene *scene, const double *d_rays8, uint32_t n_rays, uint32_t flags,
                                int *d_out_prim, double *d_out_t, double *d_out_normal, void *stream);
int spira_scene_occluded_f32(const spira_scene *scene, const float *rays8, uint32_t n_rays, uint32_t flags, uint8_t *out_hit);
int spira_scene_occluded_f64(const spira_scene *scene, const double *rays8, uint32_t n_rays, uint32_t flags, uint8_t *out_hit);
int spira_scene_occluded_device_f32(const spira_scene *scene, const float *d_rays8, uint32_t n_rays, uint32_t flags,
                                    uint8_t *d_out_hit, void *stream);
int spira_scene_occluded_device_f64(const spira_scene *scene, const double *d_rays8, uint32_t n_rays, uint32_t flags,
                                    uint8_t *d_out_hit, void *stream);

/* ---- multi-hit ray queries on a scene handle: the first max_hits hits of every ray, in order (thickness, x-ray sums, layered picking, crossing counts) ----
 * rays8, the preparation, the invalid-ray rule and the origin rule are exactly those of spira_scene_cast_*.
 * Candidates: object k — spheres [0..) then triangles [0..) in the caller's order — is a candidate of a valid ray when the reference's per-object test
 * (hit_sphere, hit_triangle: examples/julia-raytracer.jl:113-187) accepts it with the ray's own t_min and t_max, and t_k is the t that test returns.  A
 * sphere contributes at most one candidate: the near root, or the far root when the near one is below t_min.
 * Order: t ascending and, among equal t, object index DESCENDING — the later object first, the closest-hit tie rule.  The answer is the first max_hits
 * candidates of that order; with max_hits == 1, out_prim and out_t are byte for byte those of spira_scene_cast_*.
 * Outputs, caller-owned: out_prim and out_t are n_rays x max_hits, ray-major; slot j of ray i holds the j-th hit; unused slots hold SPIRA_RAY_MISS and
 * the ray's t_max copied; every slot of an invalid ray holds SPIRA_RAY_INVALID and 0.  out_count[i] (n_rays): without SPIRA_HITS_COUNT_ALL the number of
 * slots filled (<= max_hits); with the flag the number of ALL candidates of the ray — the walk then prunes with t_max only; 0 for an invalid ray.  With the
 * flag max_hits may be 0 and out_prim / out_t may be NULL (count only: out_count is then required); otherwise max_hits is in 1 .. SPIRA_MAX_HITS.  Each
 * output may be NULL, but not all three.
 * Pruning: once K = max_hits hits are known, an object is tested against the K-th t instead of the ray's t_max (not under SPIRA_HITS_COUNT_ALL).  That
 * is exact: the bits of an object's t do not depend on the bound passed (both tests compute t, then compare); a candidate beyond the K-th t of the hits
 * known so far is not among the first K of all; a sphere whose near root lies beyond the bound has its far root beyond it too; and a candidate AT the
 * K-th t is still accepted and placed by its index.  csrc/spira_hits.h has the argument in full.
 * flags: 0, SPIRA_CAST_INPLACE (one lane per ray walking to the end, the comparison point), SPIRA_HITS_COUNT_ALL, or both.  The order is total, so the
 * order in which a walk meets the candidates cannot matter: both organisations give identical bytes.
 * Errors, all decided before any device is touched: a NULL ray array, n_rays == 0, unknown flag bits, max_hits > SPIRA_MAX_HITS, max_hits == 0 without
 * SPIRA_HITS_COUNT_ALL, every output NULL (with max_hits == 0: out_count NULL), a NULL or destroyed handle, one of the other precision or of another
 * device: SPIRA_E_INVALID; n_rays > SPIRA_MAX_RAYS, or n_rays * max_hits > SPIRA_MAX_RAYS (the product formed in 64 bits): SPIRA_E_LIMIT.  A handle made
 * by spira_scene_create_multi_* is served by device 0's copy.  The host form copies in and out and returns when the outputs are written.  The *_device_*
 * form takes DEVICE pointers, is asynchronous on `stream`, synchronises nothing, allocates nothing, and is ordered like every entry: a query enqueued
 * after a device-form update or rebuild on another stream sees the new tree.  spira_get_counters is not affected by these entries. */
#define SPIRA_MAX_HITS        16u
#define SPIRA_HITS_COUNT_ALL  0x2u      /* beside SPIRA_CAST_INPLACE 0x1u */
int spira_scene_cast_hits_f32(const spira_scene *scene, const float *rays8, uint32_t n_rays, uint32_t max_hits, uint32_t flags,
                              int *out_prim, float *out_t, uint32_t *out_count);
int spira_scene_cast_hits_f64(const spira_scene *scene, const double *rays8, uint32_t n_rays, uint32_t max_hits, uint32_t flags,
                              int *out_prim, double *out_t, uint32_t *out_count);
int spira_scene_cast_hits_device_f32(const spira_scene *scene, const float *d_rays8, uint32_t n_rays, uint32_t max_hits, uint32_t flags,
                                     int *d_out_prim, float *d_out_t, uint32_t *d_out_count, void *stream);
int spira_scene_cast_hits_device_f64(const spira_scene *scene, const double *d_rays8, uint32_t n_rays, uint32_t max_hits, uint32_t flags,
                                     int *d_out_prim, double *d_out_t, uint32_t *d_out_count, void *stream);

/* ---- closest-point queries on a scene handle: for the CALLER'S points, the nearest point of the scene's surface (distance fields, proximity, snapping) ----
 * What Embree calls a point query, on the tree that create, update and rebuild maintain, which only prunes: prim, dist and point are bit for bit a scan's.
 * points4: n_points x [px py pz r_max], in the call's precision T.  The scan runs over spheres [0..) then triangles [0..) in the caller's order with
 * best = r_max * r_max (in T): object k replaces the winner exactly when d2_k <= best, then best = d2_k — the minimal squared distance wins, ties go to the
 * later object, an object at exactly r_max counts, a NaN d2 never wins.  All arithmetic in T, in the written order, nothing fused; every dot product is
 * (x x + y y) + z z.
 * Triangle, on v0, e1 = v1 - v0, e2 = v2 - v0 (differences in T), with ap = p - v0, bp = ap - e1, cp = ap - e2 — Ericson's region walk, tests in this order:
 *   1. d1 = e1.ap, d2 = e2.ap:                       d1 <= 0 && d2 <= 0               q = v0
 *   2. d3 = e1.bp, d4 = e2.bp:                       d3 >= 0 && d4 <= d3              q = v0 + e1
 *   3. vc = d1 d4 - d3 d2:                           vc <= 0 && d1 >= 0 && d3 <= 0    v = d1 / (d1 - d3),  q = v0 + e1 v
 *   4. d5 = e1.cp, d6 = e2.cp:                       d6 >= 0 && d5 <= d6              q = v0 + e2
 *   5. vb = d5 d2 - d1 d6:                           vb <= 0 && d2 >= 0 && d6 <= 0    w = d2 / (d2 - d6),  q = v0 + e2 w
 *   6. va = d3 d6 - d5 d4, g = d4 - d3, h = d5 - d6: va <= 0 && g >= 0 && h >= 0      w = g / (g + h),     q = (v0 + e1) + (e2 - e1) w
 *   7. otherwise:                                    s = 1 / ((va + vb) + vc), v = vb s, w = vc s,         q = (v0 + e1 v) + e2 w
 * (the three quotients and the one reciprocal are the only divisions), then r = p - q, d2 = (r.x r.x + r.y r.y) + r.z r.z.  A triangle of zero area may
 * give NaN and is then never picked.  Sphere (centre c, radius r as given): w = p - c, l = sqrt(w.w); l >= the smallest normal number of T: q = c + w (r / l),
 * else q = c + (r, 0, 0); then r' = p - q and d2 by the same formula.  spira_closest_point_triangle_* is the triangle function as host arithmetic (no
 * device is touched): out_q and out_d2 may each be NULL.
 * Outputs, caller-owned, each may be NULL but not all of out_prim, out_dist and out_point: out_prim the object index, spheres first, as for cast; out_dist
 * sqrt(d2) of the winner (IEEE); out_point (n_points x 3, interleaved) the winner's q; out_trips (optional, diagnostic, outside the bit-for-bit contract)
 * the walk trips — node visits plus leaf tests — the point's lane took, 0 for scenes without a tree.
 * A miss (no object within r_max): prim SPIRA_RAY_MISS, dist = the point's r_max copied, point 0.  An INVALID point — prim SPIRA_RAY_INVALID, dist 0,
 * point 0 — never faults and never disturbs its neighbours: any of its four values NaN, a coordinate infinite, r_max < 0, or (scenes WITH a tree only) the
 * origin rule of the ray queries broken for p: |(p_k - centre_k) * scale| <= 64 on every axis, in T.  r_max = +Inf is valid.
 * Why 64 serves here too: the walk skips a child box only when a Float32 lower bound of the squared distance to it, shrunk by (1 - 2^-18), exceeds
 * best scale^2 rounded up; the roundings of the normalised point (at most about 1.2e-5 + 1.2e-7 amax_n), of the dequantised box (6e-8 (1 + amax_n)) and of
 * the leaf test's own q and r (2.3e-5 + 3.6e-7 amax_n) total about 3.6e-5 + 5.4e-7 amax_n against the builder's pad of 1e-4 max(1, amax_n) (the refit pad
 * is never smaller): a margin of 2.7 or more (csrc/spira_nearest.h has the derivation).  The test is strict: equal distances still reach the later triangle.
 * flags: 0, the library's organisation for scenes with a tree — persistent waves owning contiguous ranges of the point list and refilling their free lanes
 * while the others keep walking — or SPIRA_CAST_INPLACE, one lane per point walking to the end, the comparison point.  prim, dist and point are identical
 * bytes under both.  Scenes without a tree run one lane per point either way.
 * Errors, all decided before any device is touched: a NULL point array, n_points == 0, unknown flag bits, out_prim, out_dist and out_point all NULL, a NULL
 * or destroyed handle, one of the other precision or of another device: SPIRA_E_INVALID; n_points > SPIRA_MAX_RAYS: SPIRA_E_LIMIT.  A handle made by
 * spira_scene_create_multi_* is served by device 0's copy.  The host form copies in and out and returns when the outputs are written.  The *_device_* form
 * takes DEVICE pointers, is asynchronous on `stream`, synchronises nothing, allocates nothing, and is ordered like every entry: a query enqueued after a
 * device-form update or rebuild on another stream sees the new tree.  spira_get_counters is not affected by these entries. */
int spira_scene_closest_point_f32(const spira_scene *scene, const float *points4, uint32_t n_points, uint32_t flags,
                                  int *out_prim, float *out_dist, float *out_point, uint32_t *out_trips);
int spira_scene_closest_point_f64(const spira_scene *scene, const double *points4, uint32_t n_points, uint32_t flags,
                                  int *out_prim, double *out_dist, double *out_point, uint32_t *out_trips);
int spira_scene_closest_point_device_f32(const spira_scene *scene, const float *d_points4, uint32_t n_points, uint32_t flags,
                                         int *d_out_prim, float *d_out_dist, float *d_out_point, uint32_t *d_out_trips, void *stream);
int spira_scene_closest_point_device_f64(const spira_scene *scene, const double *d_points4, uint32_t n_points, uint32_t flags,
                                         int *d_out_prim, double *d_out_dist, double *d_out_point, uint32_t *d_out_trips, void *stream);
void spira_closest_point_triangle_f32(const float v0[3], const float e1[3], const float e2[3], const float p[3], float out_q[3], float *out_d2);
void spira_closest_point_triangle_f64(const double v0[3], const double e1[3], const double e2[3], const double p[3], double out_q[3], double *out_d2);

/* ---- K-nearest point queries on a scene handle: the max_near closest objects of every point, in order (contacts within a radius, picking among a few
 *      candidates, smooth-min distance fields, counts within r) ----
 * points4, the validity rule and the origin rule are exactly those of spira_scene_closest_point_*.
 * Candidates: object k — spheres [0..) then triangles [0..) in the caller's order — is a candidate of a valid point when d2_k <= best0, with
 * best0 = r_max * r_max in T; d2_k and q_k are those of the closest-point scan above (the same two functions on the same values, a sphere's radius as
 * given); a NaN d2 is never a candidate.
 * Order: d2 ascending and, among equal d2, object index DESCENDING — the later object first, the tie rule of the closest-point scan and of the multi-hit
 * order.  The answer is the first max_near candidates of that order; with max_near == 1, out_prim, out_dist and out_point are byte for byte those of
 * spira_scene_closest_point_*.
 * Outputs, caller-owned, point-major: out_prim and out_dist are n_points x max_near, out_point is n_points x max_near x 3, interleaved; slot j of point i
 * holds the j-th nearest; out_dist is sqrt(d2) (IEEE).  Unused slots hold SPIRA_RAY_MISS, the point's r_max copied, and point 0; every slot of an invalid
 * point holds SPIRA_RAY_INVALID, 0 and 0.  out_count[i] (n_points): without SPIRA_NEAR_COUNT_ALL the number of slots filled (<= max_near); with the flag
 * the number of ALL candidates of the point — the walk then prunes with best0 only; 0 for an invalid point.  With the flag max_near may be 0: the lists are
 * then ignored and out_count is required; otherwise max_near is in 1 .. SPIRA_MAX_NEAR.  out_trips (n_points; optional, diagnostic, outside the bit-for-bit
 * contract) as for closest point.  Each output may be NULL, but not all of out_prim, out_dist, out_point and out_count.
 * Pruning: once K = max_near objects are known, the walk prunes with the K-th d2 instead of best0 (not under SPIRA_NEAR_COUNT_ALL).  That is exact: the
 * safety argument of the closest-point walk holds for any bound in the place of the best distance; a candidate beyond the K-th d2 of the candidates known
 * so far is not among the first K of all; the bound only shrinks, and a candidate AT the K-th d2 is still met and placed by its index.
 * csrc/spira_knearest.h has the argument in full.
 * flags: 0, SPIRA_CAST_INPLACE (one lane per point walking to the end, the comparison point), SPIRA_NEAR_COUNT_ALL, or both.  The order is total, so
 * both organisations give identical bytes.
 * Errors, all decided before any device is touched: a NULL point array, n_points == 0, unknown flag bits, max_near > SPIRA_MAX_NEAR, max_near == 0 without
 * SPIRA_NEAR_COUNT_ALL, every output NULL (with max_near == 0: out_count NULL), a NULL or destroyed handle, one of the other precision or of another
 * device: SPIRA_E_INVALID; n_points > SPIRA_MAX_RAYS, or n_points * max_near > SPIRA_MAX_RAYS (the product formed in 64 bits): SPIRA_E_LIMIT.  A handle
 * made by spira_scene_create_multi_* is served by device 0's copy.  The host form copies in and out and returns when the outputs are written.  The
 * *_device_* form takes DEVICE pointers, is asynchronous on `stream`, synchronises nothing, allocates nothing, and is ordered like every entry: a query
 * enqueued after a device-form update or rebuild on another stream sees the new tree.  spira_get_counters is not affected by these entries. */
#define SPIRA_MAX_NEAR        16u
#define SPIRA_NEAR_COUNT_ALL  0x2u      /* beside SPIRA_CAST_INPLACE 0x1u */
int spira_scene_nearest_k_f32(const spira_scene *scene, const float *points4, uint32_t n_points, uint32_t max_near, uint32_t flags,
                              int *out_prim, float *out_dist, float *out_point, uint32_t *out_count, uint32_t *out_trips);
int spira_scene_nearest_k_f64(const spira_scene *scene, const double *points4, uint32_t n_points, uint32_t max_near, uint32_t flags,
                              int *out_prim, double *out_dist, double *out_point, uint32_t *out_count, uint32_t *out_trips);
int spira_scene_nearest_k_device_f32(const spira_scene *scene, const float *d_points4, uint32_t n_points, uint32_t max_near, uint32_t flags,
                                     int *d_out_prim, float *d_out_dist, float *d_out_point, uint32_t *d_out_count, uint32_t *d_out_trips, void *stream);
int spira_scene_nearest_k_device_f64(const spira_scene *scene, const double *d_points4, uint32_t n_points, uint32_t max_near, uint32_t flags,
                                     int *d_out_prim, double *d_out_dist, double *d_out_point, uint32_t *d_out_count, uint32_t *d_out_trips, void *stream);

/* ---- signed distance queries on a scene handle: the nearest surface of every point AND which side of it the point is on (signed distance fields,
 *      containment, "am I inside?") ----
 * points4 (n_points x [px py pz r_max]), the validity rule and the origin rule are exactly those of spira_scene_closest_point_*.  Every step below is in the
 * call's precision T, in the written order, nothing fused.  Per valid point p:
 *   1. Nearest surface: the closest-point scan of spira_scene_closest_point_* unchanged.  out_prim and out_point are byte for byte that entry's; out_dist is
 *      that entry's value (sqrt(d2), or r_max copied on a miss) with the sign bit set where the point is inside — -0.0 can occur.
 *   2. Inside a sphere: for sphere s, w = p - c and l = sqrt(w.w) are the values the closest-point sphere function forms, the radius is as given
 *      (spheres5[5 s + 3]); the point is inside the sphere when l < r.
 *   3. Inside the mesh (scenes with at least one triangle): ray j = [p, t_min 0, D_j, t_max +Inf] with D_0 = (0.5377, 0.7211, 0.4366),
 *      D_1 = (-0.6123, 0.3142, 0.7255), D_2 = (0.2873, -0.4691, -0.8351) rounded to T, prepared as any caller's ray is (the unit direction is the one cast
 *      would walk).  c_j is the number of TRIANGLE candidates of that ray under the multi-hit candidate rule: the per-object triangle test with the ray's own
 *      t_min and t_max; spheres are not tested at all.  Rays 0 and 1 are always walked.  If c_0 and c_1 have the same parity, that parity decides (odd:
 *      inside) and c_2 = SPIRA_SDF_SKIPPED; otherwise ray 2 is walked and its parity decides — the majority of three votes.  A scene without triangles: all
 *      three slots are SPIRA_SDF_SKIPPED and the point is not inside a mesh.
 *   4. out_inside is 1 where step 2 or step 3 says inside, else 0.  out_crossings is n_points x 3, the c_j.  out_trips (optional, diagnostic, outside the
 *      contract): node visits plus leaf tests of all the walks the point's lane took.
 * The sign is MEANINGFUL for closed meshes (every edge shared by two triangles, no self-intersection): a ray from an inside point crosses the surface an odd
 * number of times; a ray exactly through an edge or a vertex may count a crossing twice, which is why three directions vote.  It is DEFINED — the rule above,
 * bit for bit — for every mesh, open ones included.
 * An INVALID point gives prim SPIRA_RAY_INVALID, dist 0, point 0, inside 255, crossings 0 0 0; it never faults and never disturbs its neighbours.
 * Each output may be NULL, but not all of out_prim, out_dist, out_point, out_inside and out_crossings.  When out_prim, out_dist and out_point are all NULL the
 * nearest walk is skipped altogether: the sign-only query, whose out_inside and out_crossings equal the full form's.
 * flags: 0, the library's organisation for scenes with a tree — refilled sessions: a lane carries its point through the nearest walk and then the ray walks
 * before it takes the next point — or SPIRA_CAST_INPLACE, one lane per point walking everything to the end.  Both give identical bytes.  Scenes without a tree
 * run one lane per point either way.
 * Errors, all decided before any device is touched: a NULL point array, n_points == 0, unknown flag bits, all five outputs NULL (out_trips alone is no
 * output), a NULL or destroyed handle, one of the other precision or of another device: SPIRA_E_INVALID; n_points > SPIRA_MAX_RAYS: SPIRA_E_LIMIT.  A handle
 * made by spira_scene_create_multi_* is served by device 0's copy.  The host form copies in and out and returns when the outputs are written.  The *_device_*
 * form takes DEVICE pointers, is asynchronous on `stream`, synchronises nothing, allocates nothing, and is ordered like every entry: a query enqueued after a
 * device-form update or rebuild on another stream sees the new tree.  spira_get_counters is not affected by these entries. */
#define SPIRA_SDF_SKIPPED 0xFFFFFFFFu
int spira_scene_signed_distance_f32(const spira_scene *scene, const float *points4, uint32_t n_points, uint32_t flags,
                                    int *out_prim, float *out_dist, float *out_point, uint8_t *out_inside, uint32_t *out_crossings, uint32_t *out_trips);
int spira_scene_signed_distance_f64(const spira_scene *scene, const double *points4, uint32_t n_points, uint32_t flags,
                                    int *out_prim, double *out_dist, double *out_point, uint8_t *out_inside, uint32_t *out_crossings, uint32_t *out_trips);
int spira_scene_signed_distance_device_f32(const spira_scene *scene, const float *d_points4, uint32_t n_points, uint32_t flags,
                                           int *d_out_prim, float *d_out_dist, float *d_out_point, uint8_t *d_out_inside, uint32_t *d_out_crossings,
                                           uint32_t *d_out_trips, void *stream);
int spira_scene_signed_distance_device_f64(const spira_scene *scene, const double *d_points4, uint32_t n_points, uint32_t flags,
                                           int *d_out_prim, double *d_out_dist, double *d_out_point, uint8_t *d_out_inside, uint32_t *d_out_crossings,
                                           uint32_t *d_out_trips, void *stream);

/* ---- sphere sweeps on a scene handle: the first contact of a moving ball (character motion, projectile CCD, camera collision, clearance checks) ----
 * "A ball of radius r moves from o along d: when and where does it first touch the scene?"  rays8 is exactly cast's list, n x [ox oy oz t_min dx dy dz
 * t_max]; the library normalises d; t, t_min and t_max are distances of the ball's CENTRE along the unit direction, c(t) = o + d t.  radii holds n values,
 * one per sweep.  The surface is the object: a sphere is a shell, as for the closest-point queries.
 * Contract (csrc/spira_sweep.h states every formula in its written order and is the authority; all arithmetic in T, nothing fused): with r2 = r r,
 * rs = r + r 2^-10, rs2 = rs rs, object k — spheres [0..) then triangles [0..) in the caller's order — yields at most one t_k.  If the squared distance from
 * c(t_min) to the object (the closest-point function of the entries above) is <= r2, the sweep starts in overlap: t_k = t_min — a sweep with t_min = 0 is
 * blocked at its start exactly where the K-nearest count within r of o is above 0.  Otherwise closed-form roots of "distance = r" (a triangle: its face
 * plane offset toward the start, the three edge cylinders, the three vertex spheres; a sphere: radius R + r from outside, R - r from inside) are PROPOSALS,
 * and the smallest proposal t >= t_min whose closest-point evaluation at c(t) gives d2 <= rs2 is t_k; q_k is that evaluation's point.  Object k is a
 * candidate when !(t_k < t_min || t_k > closest), closest starting at t_max; the minimal t wins and ties go to the LATER object.
 * Outputs, caller-owned: out_prim (the object index), out_t = t_k, out_point = q_k (n x 3: the contact point on the surface), out_normal (n x 3) =
 * (c(t_k) - q_k) / sqrt(d2), or -d where that length is below the smallest normal number; out_trips (optional, diagnostic, outside the bit-for-bit
 * contract) as for closest point.  A miss: prim SPIRA_RAY_MISS, t = the ray's t_max copied, point 0, normal 0.  An INVALID sweep — prim
 * SPIRA_RAY_INVALID, t 0, point 0, normal 0; blocked 255 — never faults and never disturbs its neighbours: the ray is invalid by cast's rule (the origin
 * rule included), or r is NaN, infinite or negative, or — scenes with a tree only — rs * scale > 64 in T (scale: the tree's frame, as in the origin rule).
 * spira_scene_sweep_blocked_*: out_hit[i] is 1 exactly where the sweep gives prim >= 0, else 0; its kernels stop at the first candidate.
 * spira_sweep_sphere_triangle_* is the leaf function as host arithmetic (no device): d_unit must be of unit length; out_hit = the triangle is a candidate
 * at closest = t_max, out_t = t_k (else t_max copied), out_q = q_k (else 0); each output may be NULL.
 * flags: 0, or SPIRA_CAST_INPLACE (one lane per sweep walking to the end, the comparison point); both organisations give identical bytes.
 * Errors, all decided before any device is touched: a NULL ray or radius array, n == 0, unknown flag bits, every output NULL (out_trips alone is no
 * output), a NULL or destroyed handle, one of the other precision or of another device: SPIRA_E_INVALID; n > SPIRA_MAX_RAYS: SPIRA_E_LIMIT.  A handle made
 * by spira_scene_create_multi_* is served by device 0's copy.  The host form copies in and out and returns when the outputs are written.  The *_device_*
 * form takes DEVICE pointers, is asynchronous on `stream`, synchronises nothing, allocates nothing, and is ordered like every entry: a sweep enqueued
 * after a device-form update or rebuild on another stream sees the new tree.  spira_get_counters is not affected by these entries. */
int spira_scene_sweep_f32(const spira_scene *scene, const float *rays8, const float *radii, uint32_t n, uint32_t flags,
                          int *out_prim, float *out_t, float *out_point, float *out_normal, uint32_t *out_trips);
int spira_scene_sweep_f64(const spira_scene *scene, const double *rays8, const double *radii, uint32_t n, uint32_t flags,
                          int *out_prim, double *out_t, double *out_point, double *out_normal, uint32_t *out_trips);
int spira_scene_sweep_device_f32(const spira_scene *scene, const float *d_rays8, const float *d_radii, uint32_t n, uint32_t flags,
                                 int *d_out_prim, float *d_out_t, float *d_out_point, float *d_out_normal, uint32_t *d_out_trips, void *stream);
int spira_scene_sweep_device_f64(const spira_scene *scene, const double *d_rays8, const double *d_radii, uint32_t n, uint32_t flags,
                                 int *d_out_prim, double *d_out_t, double *d_out_point, double *d_out_normal, uint32_t *d_out_trips, void *stream);
int spira_scene_sweep_blocked_f32(const spira_scene *scene, const float *rays8, const float *radii, uint32_t n, uint32_t flags, uint8_t *out_hit);
int spira_scene_sweep_blocked_f64(const spira_scene *scene, const double *rays8, const double *radii, uint32_t n, uint32_t flags, uint8_t *out_hit);
int spira_scene_sweep_blocked_device_f32(const spira_scene *scene, const float *d_rays8, const float *d_radii, uint32_t n, uint32_t flags, uint8_t *d_out_hit, void *stream);
int spira_scene_sweep_blocked_device_f64(const spira_scene *scene, const double *d_rays8, const double *d_radii, uint32_t n, uint32_t flags, uint8_t *d_out_hit, void *stream);
void spira_sweep_sphere_triangle_f32(const float v0[3], const float e1[3], const float e2[3], const float o[3], const float d_unit[3], float r, float t_min, float t_max,
                                     float *out_t, float out_q[3], int *out_hit);
void spira_sweep_sphere_triangle_f64(const double v0[3], const double e1[3], const double e2[3], const double o[3], const double d_unit[3], double r, double t_min, double t_max,
                                     double *out_t, double out_q[3], int *out_hit);

/* ---- box overlap queries on a scene handle: which objects touch an oriented box (voxelisation, region selection and trigger volumes, contact
 *      broadphase, culling a mesh against a cell) ----
 * boxes10 is n x [cx cy cz hx hy hz qx qy qz qw]: centre, half extents, and a rotation quaternion the library normalises as it normalises ray directions.
 * Contract (csrc/spira_overlap.h states every formula in its written order and is the authority; all arithmetic in T, nothing fused): with
 * n2 = (qx qx + qy qy) + (qz qz + qw qw) and (x, y, z, w) = q / sqrt(n2) the box axes are A0 = (1 - 2 (yy + zz), 2 (xy + zw), 2 (xz - yw)),
 * A1 = (2 (xy - zw), 1 - 2 (xx + zz), 2 (yz + xw)), A2 = (2 (xz + yw), 2 (yz - xw), 1 - 2 (xx + yy)); a world vector a has the box-frame coordinates
 * (dot(A0, a), dot(A1, a), dot(A2, a)); the identity quaternion gives the unit axes exactly.  A TRIANGLE is a candidate when all 13 axes of the
 * separating-axis test overlap (the three box axes, the face normal, the nine cross(unit_i, edge_j)), evaluated on the record's own v0, e1, e2 taken to
 * the box frame; an axis with projections p0, p1, p2 and radius rad overlaps when min(p) <= rad && max(p) >= -rad — closed, touching counts; a NaN in
 * any projection makes the object no candidate, and so does a computed face normal of exactly (0, 0, 0) (a triangle of zero area, which the point
 * queries never pick either).  A SPHERE is a shell, as for the point queries: with p the box-frame coordinates of its centre less the
 * box's, dmin2 = sum max(|p_k| - h_k, 0)^2 and dmax2 = sum (|p_k| + h_k)^2, it is a candidate when dmin2 <= R R && dmax2 >= R R.
 * Outputs, caller-owned: out_count[i] (n) is the number of ALL candidates of box i — spheres [0..) then triangles [0..) in the caller's order; out_prim
 * (n x max_list) holds the first max_list candidates in ASCENDING object index, unused slots SPIRA_RAY_MISS; every slot of an INVALID box holds
 * SPIRA_RAY_INVALID and its count is 0.  max_list is in 0 .. SPIRA_MAX_OVERLAP; 0 counts only, and out_count is then required.  Index order carries no
 * spatial bound, so the walk never prunes with the list and the count is always complete (there is no count flag).  out_trips (n; optional, diagnostic,
 * outside the bit-for-bit contract) as for closest point.  Each of out_prim and out_count may be NULL, not both.
 * spira_scene_overlap_any_*: out_hit[i] is 1 exactly where the count is above 0, else 0, 255 for an invalid box; its kernels leave at the first candidate.
 * A box is INVALID — it never faults and never disturbs its neighbours — when any of its ten values is NaN or infinite, some h_k < 0, n2 is not finite or
 * below the smallest normal number of T, or — scenes with a tree only — the origin rule of the ray queries fails for its centre, or He_k * scale > 64 on
 * some axis, He_k = (|A0_k| h0 + |A1_k| h1) + |A2_k| h2 being the enclosing axis-aligned half extent.  h = 0 is valid: a point, a segment, a rectangle.
 * spira_overlap_box_triangle_* / spira_overlap_box_sphere_* are the leaf functions as host arithmetic (no device): 1, 0, or SPIRA_RAY_INVALID for a box
 * that is invalid without a frame.
 * flags: 0, or SPIRA_CAST_INPLACE (one lane per box walking to the end, the comparison point); both organisations give identical bytes.
 * Errors, all decided before any device is touched: a NULL box array, n == 0, unknown flag bits, max_list > SPIRA_MAX_OVERLAP, every output NULL (with
 * max_list == 0: out_count NULL; out_trips alone is no output), a NULL or destroyed handle, one of the other precision or of another device:
 * SPIRA_E_INVALID; n > SPIRA_MAX_RAYS, or n * max_list > SPIRA_MAX_RAYS (the product formed in 64 bits): SPIRA_E_LIMIT.  A handle made by
 * spira_scene_create_multi_* is served by device 0's copy.  The host form copies in and out and returns when the outputs are written.  The *_device_*
 * form takes DEVICE pointers, is asynchronous on `stream`, synchronises nothing, allocates nothing, and is ordered like every entry: a query enqueued
 * after a device-form update or rebuild on another stream sees the new tree.  spira_get_counters is not affected by these entries. */
#define SPIRA_MAX_OVERLAP     16u
int spira_scene_overlap_box_f32(const spira_scene *scene, const float *boxes10, uint32_t n, uint32_t max_list, uint32_t flags,
                                int *out_prim, uint32_t *out_count, uint32_t *out_trips);
int spira_scene_overlap_box_f64(const spira_scene *scene, const double *boxes10, uint32_t n, uint32_t max_list, uint32_t flags,
                                int *out_prim, uint32_t *out_count, uint32_t *out_trips);
int spira_scene_overlap_box_device_f32(const spira_scene *scene, const float *d_boxes10, uint32_t n, uint32_t max_list, uint32_t flags,
                                       int *d_out_prim, uint32_t *d_out_count, uint32_t *d_out_trips, void *stream);
int spira_scene_overlap_box_device_f64(const spira_scene *scene, const double *d_boxes10, uint32_t n, uint32_t max_list, uint32_t flags,
                                       int *d_out_prim, uint32_t *d_out_count, uint32_t *d_out_trips, void *stream);
int spira_scene_overlap_any_f32(const spira_scene *scene, const float *boxes10, uint32_t n, uint32_t flags, uint8_t *out_hit);
int spira_scene_overlap_any_f64(const spira_scene *scene, const double *boxes10, uint32_t n, uint32_t flags, uint8_t *out_hit);
int spira_scene_overlap_any_device_f32(const spira_scene *scene, const float *d_boxes10, uint32_t n, uint32_t flags, uint8_t *d_out_hit, void *stream);
int spira_scene_overlap_any_device_f64(const spira_scene *scene, const double *d_boxes10, uint32_t n, uint32_t flags, uint8_t *d_out_hit, void *stream);
int spira_overlap_box_triangle_f32(const float v0[3], const float e1[3], const float e2[3], const float box10[10]);
int spira_overlap_box_triangle_f64(const double v0[3], const double e1[3], const double e2[3], const double box10[10]);
int spira_overlap_box_sphere_f32(const float centre[3], float radius, const float box10[10]);
int spira_overlap_box_sphere_f64(const double centre[3], double radius, const double box10[10]);

/* ---- triangle overlap queries on a scene handle: which objects does a triangle cut (mesh against mesh narrowphase, cloth or a skinned mesh against
 *      the environment, selection by a cutting polygon, the pair list an intersection curve starts from) ----
 * triangles10 is n x [q0 q1 q2 mat], the layout of a scene's triangles10: the array another handle was created from or updated with is a query list as it
 * is, host or device.  The tenth value is never read (it may be NaN).
 * Contract (csrc/spira_trioverlap.h states every formula in its written order and is the authority; all arithmetic in T, nothing fused): with
 * g1 = q1 - q0, g2 = q2 - q0, g3 = g2 - g1, m = cross(g1, g2) and, for a scene triangle's record v0, e1, e2: u0 = v0 - q0, u1 = u0 + e1, u2 = u0 + e2,
 * e3 = e2 - e1, n = cross(e1, e2), an axis L overlaps when min(dot(L, u_m)) <= max(0, dot(L, g1), dot(L, g2)) and min(0, dot(L, g1), dot(L, g2)) <=
 * max(dot(L, u_m)) with no NaN among the six values — closed, touching counts.  A TRIANGLE is a candidate when all 20 axes overlap: the three world unit
 * axes (the components themselves), n, m, the nine cross(g_i, e_j), the three cross(n, e_j) and the three cross(m, g_i) (which separate coplanar pairs),
 * and n is not exactly (0, 0, 0).  A SPHERE is a shell: with dmin2 the squared distance of closest_point_triangle(q0, g1, g2, C) and dmax2 the largest
 * squared distance from C to q0, q1, q2, it is a candidate when dmin2 <= R R && dmax2 >= R R.
 * A query is INVALID — it never faults and never disturbs its neighbours — when any of its nine coordinates is NaN or infinite, m is not finite or is
 * exactly (0, 0, 0) (a segment or a point is no triangle query), or — scenes with a tree only — the origin rule of the ray queries fails for one of its
 * three vertices.  There is no extent rule.
 * Outputs, max_list, flags, out_trips, the errors, the host and the device form and their ordering are spira_scene_overlap_box_*'s above, word for word,
 * with "query triangle" for "box".  spira_overlap_tri_triangle_* / spira_overlap_tri_sphere_* are the leaf functions as host arithmetic (no device): 1, 0,
 * or SPIRA_RAY_INVALID for a query that is invalid without a frame. */
int spira_scene_overlap_tri_f32(const spira_scene *scene, const float *triangles10, uint32_t n, uint32_t max_list, uint32_t flags,
                                int *out_prim, uint32_t *out_count, uint32_t *out_trips);
int spira_scene_overlap_tri_f64(const spira_scene *scene, const double *triangles10, uint32_t n, uint32_t max_list, uint32_t flags,
                                int *out_prim, uint32_t *out_count, uint32_t *out_trips);
int spira_scene_overlap_tri_device_f32(const spira_scene *scene, const float *d_triangles10, uint32_t n, uint32_t max_list, uint32_t flags,
                                       int *d_out_prim, uint32_t *d_out_count, uint32_t *d_out_trips, void *stream);
int spira_scene_overlap_tri_device_f64(const spira_scene *scene, const double *d_triangles10, uint32_t n, uint32_t max_list, uint32_t flags,
                                       int *d_out_prim, uint32_t *d_out_count, uint32_t *d_out_trips, void *stream);
int spira_scene_overlap_tri_any_f32(const spira_scene *scene, const float *triangles10, uint32_t n, uint32_t flags, uint8_t *out_hit);
int spira_scene_overlap_tri_any_f64(const spira_scene *scene, const double *triangles10, uint32_t n, uint32_t flags, uint8_t *out_hit);
int spira_scene_overlap_tri_any_device_f32(const spira_scene *scene, const float *d_triangles10, uint32_t n, uint32_t flags, uint8_t *d_out_hit, void *stream);
int spira_scene_overlap_tri_any_device_f64(const spira_scene *scene, const double *d_triangles10, uint32_t n, uint32_t flags, uint8_t *d_out_hit, void *stream);
int spira_overlap_tri_triangle_f32(const float v0[3], const float e1[3], const float e2[3], const float query10[10]);
int spira_overlap_tri_triangle_f64(const double v0[3], const double e1[3], const double e2[3], const double query10[10]);
int spira_overlap_tri_sphere_f32(const float centre[3], float radius, const float query10[10]);
int spira_overlap_tri_sphere_f64(const double centre[3], double radius, const double query10[10]);

/* ---- radiance along the CALLER'S rays on a scene handle: the integrator for any camera, light probe, irradiance point or lightmap texel ----
 * Replaces ray_color(ray, world, depth) of examples/julia-raytracer.jl:328-367 called once per ray and sample — the function the reference's render loop
 * calls with get_ray's ray (:398-402), here for a ray list the caller owns, with the estimator, RNG and sample order of every render entry.
 * rays6: n_rays x [ox oy oz dx dy dz].  Preparation per ray, in the call's precision T, nothing fused: s = (dx dx + dy dy) + dz dz,
 * d = (dx, dy, dz) / sqrt(s) — exactly what the renderer's normalize() and the ray queries' preparation do.  A ray is INVALID when any of its six values is
 * NaN or infinite, or s is not finite or is below the smallest normal number of T: out_valid[k] = 0 (valid rays: 1), nothing is added to its sums, and its
 * neighbours are not disturbed.  There is no origin rule: every segment is the renderer's own.
 * Paths: ray k, sample s in sample0 .. sample0 + spp - 1, is the path the renderer would trace for a camera ray of that origin and unit direction at PIXEL
 * KEY key0 + k: SPIRA_SEM_A, every random number from rng_key(sA, sB, key0 + k, s, bounce) with sA, sB derived from `seed` as every entry derives them;
 * every segment with t_min 0.001, the first included; scatter while bounce + 1 < max_depth; sky, emission, the extensions and the tree walk as in a render.
 * So a ray list made from a pinhole camera (spira_camera_rays_* below) with key0 = row0 * width reproduces spira_accumulate_* and spira_render_scene_*
 * bit for bit.
 * Sums: sum_rgb is n_rays x 3, INTERLEAVED, caller-owned.  The entry ADDS, per channel in T, one addition per sample in ascending sample order,
 * sum = sum + L_s — the contract of spira_accumulate_*: k calls of n samples leave bit for bit the sums of one call of k*n samples, and a ray list traced
 * in chunks (key0 advanced by the rays before the chunk) leaves bit for bit the sums of the whole list.  out_valid may be NULL; sum_rgb may not.
 * flags: 0, SPIRA_EXT_DIELECTRIC, SPIRA_EXT_SPECTRAL; any other bit is SPIRA_E_UNSUPPORTED.
 * Errors, all decided before any device is touched: a NULL ray array, struct or sum_rgb, n_rays == 0, spp == 0, max_depth outside 1 .. SPIRA_MAX_DEPTH,
 * reserved != 0, a NULL or destroyed handle, one of the other precision or of another device: SPIRA_E_INVALID; n_rays > SPIRA_MAX_RAYS, key0 + n_rays > 2^32,
 * sample0 + spp > SPIRA_MAX_SPP: SPIRA_E_LIMIT.  A scene whose LDS the device refuses: SPIRA_E_LIMIT, as for a render.  A handle made by
 * spira_scene_create_multi_* is served by device 0's copy.
 * The host form copies rays in, sum_rgb in AND out, out_valid out, and returns when they are written.  The *_device_* form takes DEVICE pointers, is
 * asynchronous on `stream`, synchronises nothing, allocates only on its first call at a size (the workspace stays in the device context until
 * spira_shutdown; a call of one sample per ray needs none) and is ordered like every entry: a call enqueued after a device-form update or rebuild on
 * another stream sees the new tree.  spira_get_counters is not affected by these entries. */
typedef struct spira_radiance {
    uint32_t spp, max_depth, flags, sample0;
    uint64_t seed;
    uint32_t key0, reserved;         /* reserved must be 0 */
} spira_radiance;                    /* 32 bytes */
int spira_scene_radiance_f32(const spira_scene *scene, const float *rays6, uint32_t n_rays, const spira_radiance *rp,
                             float *sum_rgb, uint8_t *out_valid);
int spira_scene_radiance_f64(const spira_scene *scene, const double *rays6, uint32_t n_rays, const spira_radiance *rp,
                             double *sum_rgb, uint8_t *out_valid);
int spira_scene_radiance_device_f32(const spira_scene *scene, const float *d_rays6, uint32_t n_rays, const spira_radiance *rp,
                                    float *d_sum_rgb, uint8_t *d_out_valid, void *stream);
int spira_scene_radiance_device_f64(const spira_scene *scene, const double *d_rays6, uint32_t n_rays, const spira_radiance *rp,
                                    double *d_sum_rgb, uint8_t *d_out_valid, void *stream);

/* ---- camera ray generator: the ray list of one sample of every pixel of `rows` rows, for the radiance entries above ----
 * Replaces get_ray(camera, u, v) of examples/julia-raytracer.jl:298-306 with the pixel jitter of :398-399 — and gives the reference's stored-but-unused
 * lens_radius (:261-295, "No defocus blur" :298) its thin lens.  camera12 as everywhere (origin, lower_left_corner, horizontal, vertical; focus_dist is
 * already in it).  rays6: rows * width x [ox oy oz dx dy dz], directions NOT normalised (the radiance entry normalises), ordered by reference pixel:
 * ray k = (j - 1 - row0) * width + (i - 1) for i in 1 .. width, j - 1 in row0 .. row0 + rows - 1, j = 1 the BOTTOM row (v = 0).  The ray's key is its global
 * pixel (j - 1) * width + (i - 1): pass key0 = row0 * width to the radiance entry.
 * All models, in T, in the written order, nothing fused: (xu, xv) = the pixel jitter of every render entry, rng3(rng_key(pixel, sample, 0), 0);
 * u = ((i - 1) + xu) / (W - 1), v = ((j - 1) + xv) / (H - 1); P = (llc + hor u) + ver v.
 *   SPIRA_CAM_PINHOLE    o = origin, d = P - origin: bit for bit the renderer's camera ray before normalisation.
 *   SPIRA_CAM_THIN_LENS  lens_radius == 0 is PINHOLE by definition.  Else eu = normalize(hor), ev = normalize(ver); a lens point p from the reference's
 *                        rejection idiom under key (pixel, sample, bounce 255 — no path's, max_depth <= 255): tries t = 1 .. 64, p = (2 u0 - 1, 2 u1 - 1),
 *                        accepted when p.p < 1, else p = 0; off = eu (R p.x) + ev (R p.y), o = origin + off, d = (P - origin) - off, R = lens_radius
 *                        rounded to T once: every ray of a pixel sample meets the focus plane at P.
 *   SPIRA_CAM_ORTHO      o = P, d = ((llc + hor / 2) + ver / 2) - origin: every ray runs along the camera axis.
 * Limits: width, height >= 2, a known model, lens_radius finite and >= 0, row0 + rows <= height (rows == 0: the whole image, row0 ignored), NULL pointers:
 * else SPIRA_E_INVALID; width * height >= 2^31, sample >= SPIRA_MAX_SPP, rows * width > SPIRA_MAX_RAYS: SPIRA_E_LIMIT.
 * The host form is host arithmetic (the same inline function the kernel calls; no device needed).  The *_device_* form writes a DEVICE array, is
 * asynchronous on `stream`, synchronises and allocates nothing, and is ordered like every device entry. */
#define SPIRA_CAM_PINHOLE 0u
#define SPIRA_CAM_THIN_LENS 1u
#define SPIRA_CAM_ORTHO 2u
typedef struct spira_lens {
    uint32_t model, width, height, sample;
    uint64_t seed;
    uint32_t row0, rows;             /* reference rows j-1, from the bottom; rows == 0: all */
    double   lens_radius;
} spira_lens;                        /* 40 bytes */
int spira_camera_rays_f32(const float camera12[12], const spira_lens *lens, float *rays6);
int spira_camera_rays_f64(const double camera12[12], const spira_lens *lens, double *rays6);
int spira_camera_rays_device_f32(const float camera12[12], const spira_lens *lens, float *d_rays6, void *stream);
int spira_camera_rays_device_f64(const double camera12[12], const spira_lens *lens, double *d_rays6, void *stream);

/* ---- hemisphere gather at surface points: irradiance sums and visibility counts for irradiance points and lightmap texels (light probes: below) ----
 * The reference has no baker; what these entries integrate is ray_color (examples/julia-raytracer.jl:328-367) and the hit scan (:242-258), over directions
 * drawn by the reference's own rejection idiom (random_in_unit_sphere, :309-316).  The caller gives POINTS; the library draws the hemisphere directions with
 * its own RNG inside the kernel, so a lightmap of n points at spp samples is one call on n x 6 values, not n * spp rays.
 * points6: n_points x [px py pz nx ny nz] in the call's precision T.  The sampling rule, in T, in the written order, nothing fused:
 *   validity   a point is INVALID when any of its six values is NaN or infinite, or (nx nx + ny ny) + nz nz is not finite or is below the smallest normal
 *              number of T — the radiance entry's rule for a ray, applied to the six values.  Otherwise nh = n / sqrt(n.n).
 *   q          for point k and sample s, the rejection idiom under the key rng_key(sA, sB, key0 + k, s, 255): tries t = 1 .. 64, scale 2^-20,
 *              q = (2 u0 - 1, 2 u1 - 1, 2 u2 - 1), accepted when (q.x q.x + q.y q.y) + q.z q.z < 1, else q = 0.  Bounce 255 is the lens's slot of
 *              spira_camera_rays_*: no path reaches it (bounces 0 .. 254) and a gather has no lens; the path's own keys are left alone.
 *   direction  qh = q / sqrt(q.q), or 0 when q.q is below the smallest normal number of T; v = nh + qh — a unit normal plus a uniform point on the unit
 *              sphere is exactly cosine-weighted.  Where [p, v] is no valid ray for the radiance entry (v cancelled to nothing), v = nh.
 *   ray        [p, v], v NOT normalised: the radiance entry and the ray queries normalise it with the one formula the gather kernels use.
 *   invalid    the generator writes six zeros, which the radiance entry and the ray queries classify as invalid themselves.
 * So every number below is, by construction, what the existing entries give for the ray lists of spira_gather_rays_*.
 *
 * spira_gather_rays_*: rays6 = the ray list (n_points x 6) of ONE sample of every point.  The host form is host arithmetic (the same inline function the
 * kernels call; no device needed).  The *_device_* form takes DEVICE pointers, is asynchronous on `stream`, synchronises and allocates nothing.
 * Limits: NULL pointers, n_points == 0: SPIRA_E_INVALID; n_points > SPIRA_MAX_RAYS, key0 + n_points > 2^32, sample >= SPIRA_MAX_SPP: SPIRA_E_LIMIT.
 *
 * spira_scene_gather_*: for every valid point k and every sample s in sample0 .. sample0 + spp - 1, the path spira_scene_radiance_* traces along the ray
 * [p, v(k, s)] at pixel key key0 + k, sample s; sum_rgb (n_points x 3, INTERLEAVED, caller-owned) takes sum = sum + L_s per channel in T, one addition
 * per sample in ascending sample order.  So k calls of n samples leave bit for bit the sums of one call of k*n samples, and a point list gathered in chunks
 * (key0 advanced by the points before the chunk) leaves bit for bit the sums of the whole list.  Irradiance is pi * sum / spp (the directions are
 * cosine-weighted): that scaling is the caller's — the entry returns sums, like every accumulate entry.  out_valid[k] = 0 and nothing added for an
 * invalid point, 1 otherwise; out_valid may be NULL, sum_rgb may not.  The struct is spira_radiance, unchanged; flags: 0, SPIRA_EXT_DIELECTRIC,
 * SPIRA_EXT_SPECTRAL, any other bit SPIRA_E_UNSUPPORTED.  Errors, limits (n_points for n_rays), stream ordering, multi-device handles and the workspace
 * are spira_scene_radiance_*'s: every check before any device is touched; a call enqueued after a device-form update or rebuild on another stream sees
 * the new tree; the device form allocates only on its first call at a size (a call of one sample per point needs no workspace), and the workspace stays
 * in the device context until spira_shutdown.  n_points * spp may exceed 2^32: the call is split into passes by samples.
 *
 * spira_scene_gather_visible_*: adds to visible_u32[k] the number of samples s in sample0 .. sample0 + spp - 1 for which spira_scene_occluded_* answers 0
 * for the ray [p, t_min, v(k, s), t_max] (t_min, t_max rounded to T once; distances along the unit direction).  out_valid[k] = 0 and nothing added where
 * the point is invalid or breaks the ray queries' origin rule (scenes with a tree; the rule reads the origin only, so it holds for all samples of a point
 * or for none), 1 otherwise.  Ambient occlusion is 1 - visible / spp.  flags: 0, the refilled traversal sessions of the ray queries over generated rays,
 * or SPIRA_CAST_INPLACE, one lane per (point, sample) — identical bytes; scenes without a tree run one lane per item either way.
 * Errors, all decided before any device is touched: NULL points, struct or visible_u32, n_points == 0, spp == 0, a NaN in t_min / t_max, t_min < 0,
 * t_max < t_min (t_max = +Inf is allowed), unknown flag bits, a NULL or destroyed handle, one of the other precision or of another device:
 * SPIRA_E_INVALID; n_points > SPIRA_MAX_RAYS, key0 + n_points > 2^32, sample0 + spp > SPIRA_MAX_SPP: SPIRA_E_LIMIT.  The host form copies points in,
 * visible_u32 in AND out, out_valid out.  The *_device_* form is asynchronous on `stream`, synchronises and allocates nothing, and is ordered like every
 * entry.  spira_get_counters is not affected by any of these entries. */
typedef struct spira_gather_visible {
    uint32_t spp, sample0;
    uint64_t seed;
    uint32_t key0, flags;            /* 0 or SPIRA_CAST_INPLACE */
    double   t_min, t_max;
} spira_gather_visible;              /* 40 bytes */
int spira_gather_rays_f32(const float *points6, uint32_t n_points, uint32_t sample, uint64_t seed, uint32_t key0, float *rays6);
int spira_gather_rays_f64(const double *points6, uint32_t n_points, uint32_t sample, uint64_t seed, uint32_t key0, double *rays6);
int spira_gather_rays_device_f32(const float *d_points6, uint32_t n_points, uint32_t sample, uint64_t seed, uint32_t key0, float *d_rays6, void *stream);
int spira_gather_rays_device_f64(const double *d_points6, uint32_t n_points, uint32_t sample, uint64_t seed, uint32_t key0, double *d_rays6, void *stream);
int spira_scene_gather_f32(const spira_scene *scene, const float *points6, uint32_t n_points, const spira_radiance *rp,
                           float *sum_rgb, uint8_t *out_valid);
int spira_scene_gather_f64(const spira_scene *scene, const double *points6, uint32_t n_points, const spira_radiance *rp,
                           double *sum_rgb, uint8_t *out_valid);
int spira_scene_gather_device_f32(const spira_scene *scene, const float *d_points6, uint32_t n_points, const spira_radiance *rp,
                                  float *d_sum_rgb, uint8_t *d_out_valid, void *stream);
int spira_scene_gather_device_f64(const spira_scene *scene, const double *d_points6, uint32_t n_points, const spira_radiance *rp,
                                  double *d_sum_rgb, uint8_t *d_out_valid, void *stream);
int spira_scene_gather_visible_f32(const spira_scene *scene, const float *points6, uint32_t n_points, const spira_gather_visible *gv,
                                   uint32_t *visible_u32, uint8_t *out_valid);
int spira_scene_gather_visible_f64(const spira_scene *scene, const double *points6, uint32_t n_points, const spira_gather_visible *gv,
                                   uint32_t *visible_u32, uint8_t *out_valid);
int spira_scene_gather_visible_device_f32(const spira_scene *scene, const float *d_points6, uint32_t n_points, const spira_gather_visible *gv,
                                          uint32_t *d_visible_u32, uint8_t *d_out_valid, void *stream);
int spira_scene_gather_visible_device_f64(const spira_scene *scene, const double *d_points6, uint32_t n_points, const spira_gather_visible *gv,
                                          uint32_t *d_visible_u32, uint8_t *d_out_valid, void *stream);

/* ---- light probes: the radiance arriving at free points from the whole sphere, projected onto the nine real spherical harmonics of bands 0 .. 2 ----
 * A probe is a point in free space with no normal; its answer must serve every normal a moving object later shows it.  That answer is 9 x 3 numbers:
 * the projection of the incoming radiance onto Y_0 .. Y_8.  csrc/spira_probe.h is the authority for what follows.  All arithmetic in the call's
 * precision T, in the written order, nothing fused.
 * points3: n_points x [px py pz].  A point is INVALID when any of the three values is NaN or infinite.  There is no origin rule, as in the radiance entry.
 *   q          for point k and sample s, the gather's draw, exactly: the rejection idiom under the key rng_key(sA, sB, key0 + k, s, 255), tries
 *              t = 1 .. 64, scale 2^-20, a = (u0 - 1, u1 - 1, u2 - 1), accepted when (a.x a.x + a.y a.y) + a.z a.z < 1.
 *   direction  qq = q.q, qh = q / sqrt(qq); where qq is below the smallest normal number of T (no try accepted), qh = (0, 0, 1).  A uniform point in the
 *              ball, normalised, is uniform on the sphere: every valid point has a valid ray for every sample.
 *   ray        [p, qh], qh NOT normalised again by the generator; the path's unit direction d is what the radiance entry's preparation gives for those six
 *              values (s = (dx dx + dy dy) + dz dz, d = (dx, dy, dz) / sqrt(s)).
 *   invalid    the generator writes six zeros.
 *   basis      x y z = d; c0 = 0.28209479177387814, c1 = 0.4886025119029199, c2 = 1.0925484305920792, c3 = 0.31539156525252005, c4 = 0.5462742152960396,
 *              double literals each rounded to T once:
 *              Y0 = c0, Y1 = c1 y, Y2 = c1 z, Y3 = c1 x, Y4 = c2 (x y), Y5 = c2 (y z), Y6 = c3 (3 (z z) - 1), Y7 = c2 (x z), Y8 = c4 (x x - y y).
 *              No Condon-Shortley sign: the ordering most graphics code uses.
 *
 * spira_sh9_basis_*: out9 = Y_0 .. Y_8 at the unit direction d_unit.  Host arithmetic.
 *
 * spira_probe_rays_*: rays6 = the ray list (n_points x 6) of ONE sample of every point.  The host form is host arithmetic (the same inline function the
 * kernels call; no device needed).  The *_device_* form takes DEVICE pointers, is asynchronous on `stream`, synchronises and allocates nothing.
 * Limits: NULL pointers, n_points == 0: SPIRA_E_INVALID; n_points > SPIRA_MAX_RAYS, key0 + n_points > 2^32, sample >= SPIRA_MAX_SPP: SPIRA_E_LIMIT.
 *
 * spira_scene_probe_sh_*: sum_sh is n_points x 9 x 3, INTERLEAVED ([k][j][channel]), caller-owned.  The entry ADDS: for every valid point k, for
 * s = sample0 .. sample0 + spp - 1 ascending, L_s is the radiance spira_scene_radiance_* gives for the ray [p, qh(k, s)] at pixel key key0 + k, sample s,
 * and sum[k][j][c] = sum[k][j][c] + Y_j(d_s) * L_s[c]: one product, then one addition.  So k calls of n samples leave bit for bit the sums of one call of
 * k*n samples, a point list in chunks (key0 advanced by the points before the chunk) leaves bit for bit the sums of the whole list, and any pass split
 * leaves the same bytes.  The SH coefficients of the radiance are (4 pi / spp) * sum: that scaling is the caller's, as pi / spp is for the gather.
 * out_valid[k] = 0 and nothing added for an invalid point, 1 otherwise; out_valid may be NULL, sum_sh may not.  The struct is spira_radiance, unchanged;
 * flags: 0, SPIRA_EXT_DIELECTRIC, SPIRA_EXT_SPECTRAL, any other bit SPIRA_E_UNSUPPORTED.  Errors, limits (n_points <= SPIRA_MAX_RAYS, key0 + n_points <= 2^32,
 * sample0 + spp <= SPIRA_MAX_SPP), stream ordering, multi-device handles and the workspace are spira_scene_gather_*'s: every check before any device is
 * touched; a call enqueued after a device-form update or rebuild on another stream sees the new tree; a handle made by spira_scene_create_multi_* is
 * served by device 0's copy; the device form allocates only on its first call at a size (a call of one sample per point needs no workspace), and the
 * workspace — the gather's, under the gather's knobs — stays in the device context until spira_shutdown.  n_points * spp may exceed 2^32: the call is
 * split into passes by samples.  spira_get_counters is not affected by any of these entries. */
void spira_sh9_basis_f32(const float d_unit[3], float out9[9]);
void spira_sh9_basis_f64(const double d_unit[3], double out9[9]);
int spira_probe_rays_f32(const float *points3, uint32_t n_points, uint32_t sample, uint64_t seed, uint32_t key0, float *rays6);
int spira_probe_rays_f64(const double *points3, uint32_t n_points, uint32_t sample, uint64_t seed, uint32_t key0, double *rays6);
int spira_probe_rays_device_f32(const float *d_points3, uint32_t n_points, uint32_t sample, uint64_t seed, uint32_t key0, float *d_rays6, void *stream);
int spira_probe_rays_device_f64(const double *d_points3, uint32_t n_points, uint32_t sample, uint64_t seed, uint32_t key0, double *d_rays6, void *stream);
int spira_scene_probe_sh_f32(const spira_scene *scene, const float *points3, uint32_t n_points, const spira_radiance *rp,
                             float *sum_sh, uint8_t *out_valid);
int spira_scene_probe_sh_f64(const spira_scene *scene, const double *points3, uint32_t n_points, const spira_radiance *rp,
                             double *sum_sh, uint8_t *out_valid);
int spira_scene_probe_sh_device_f32(const spira_scene *scene, const float *d_points3, uint32_t n_points, const spira_radiance *rp,
                                    float *d_sum_sh, uint8_t *d_out_valid, void *stream);
int spira_scene_probe_sh_device_f64(const spira_scene *scene, const double *d_points3, uint32_t n_points, const spira_radiance *rp,
                                    double *d_sum_sh, uint8_t *d_out_valid, void *stream);

/* ---- progressive accumulation (checkpoint / resume / adaptive sampling) ----
 * The contract the reference's kernel was designed for and no host code uses: `current_sample_index`,
 * persisted `rng_states`, `output_hdr_image[p] += L` (src/spira_path_trace_kernel.metal:143-145, :252-268).
 * Renders samples [sample0, sample0 + params->spp) of every pixel of the tile and ADDS their radiance, in
 * sample order, to sum_rgb (planar 3 x rows x width running sums, caller-owned; zero them before the first
 * call).  image = sum_rgb / total samples; k calls of n samples leave bit for bit the sums of one call of k*n.
 * rng_states (rows*width words, or NULL) is used by SPIRA_SEM_METAL only, whose LCG state runs from sample to
 * sample: written by every call, read when sample0 > 0 — SPIRA_SEM_METAL with sample0 > 0 and rng_states == NULL
 * is SPIRA_E_INVALID (it would replay the first call's samples).  Host pointers, or device pointers + stream. */
int spira_accumulate_f32(const float *spheres5, const float *materials8, const float *triangles10,
                         const float camera12[12], const spira_params *params, uint32_t sample0,
                         float *sum_rgb, uint32_t *rng_states);
int spira_accumulate_f64(const double *spheres5, const double *materials8, const double *triangles10,
                         const double camera12[12], const spira_params *params, uint32_t sample0,
                         double *sum_rgb, uint32_t *rng_states);
int spira_accumulate_device_f32(const float *spheres5, const float *materials8, const float *triangles10,
                                const float camera12[12], const spira_params *params, uint32_t sample0,
                                float *d_sum_rgb, uint32_t *d_rng_states, void *stream);
int spira_accumulate_device_f64(const double *spheres5, const double *materials8, const double *triangles10,
                                const double camera12[12], const spira_params *params, uint32_t sample0,
                                double *d_sum_rgb, uint32_t *d_rng_states, void *stream);

/* ---- adaptive sampling: render to a noise target, per-pixel sample counts ----
 * params->spp is the CAP.  Round 0 gives every pixel of the tile min_spp samples; every later round gives each pixel still active
 * min(batch_spp, spp - n) more; a pixel leaves the active set the first time the rule below holds at the end of a round, or at the cap,
 * so a pixel ends with one of the counts min_spp, min_spp + batch_spp, ..., spp; the render ends when the set is empty.  Every adaptive
 * render starts at sample 0 (there is no sample0), and "pixel p received its first n samples" means what it means everywhere else in
 * this library: the RNG is keyed by (global pixel, sample) and sums run in sample order, so out_hdr at a pixel with out_spp == n is, bit
 * for bit, the plain render of spp = n there, whatever the tiling (rows / row0 / stripe_* as in every entry), list order or scheduling.
 * The rule, per pixel, evaluated in the render precision T in exactly this order, nothing fused: with sum = the RGB sums and
 * Q = the sum over the samples, in order, of y*y, y = (0.2126 r + 0.7152 g) + 0.0722 b the luminance of ONE sample, after n samples
 *     Y = (0.2126 sum.r + 0.7152 sum.g) + 0.0722 sum.b,   V = max(n Q - Y Y, 0),   rhs = ((tol (Y + n floor)) (tol (Y + n floor))) (n - 1)
 *     converged  <=>  tolerance > 0  and  V <= rhs            (any NaN in V or rhs: not converged; tolerance == 0: never)
 * i.e. "standard error of the mean luminance <= tolerance * (mean + floor)" multiplied through by n^2 (n - 1).  tolerance and floor are
 * rounded to T once.  The cancellation in n Q - Y Y costs about 1e-7 Y^2 in Float32 against a threshold of about tolerance^2 Y^2 n:
 * harmless for tolerance >= 1e-3.  A per-pixel stopping rule biases the estimate slightly downward in noisy pixels (a pixel whose
 * first samples happen to agree stops before it meets its rare bright ones); min_spp exists to bound that.
 * Limits: min_spp >= 2, batch_spp >= 1, min_spp <= params->spp, tolerance >= 0, floor >= 0, max_depth >= 1, else SPIRA_E_INVALID.
 * Scope: SPIRA_SEM_A with SPIRA_KERNEL_DEFAULT, both precisions, spheres, LDS triangles and BVH meshes; any other estimator or
 * organisation and the SPIRA_EXT_* flags are SPIRA_E_UNSUPPORTED.
 * Outputs (any may be NULL, not all): out_hdr / out_img as in every entry (the mean over the pixel's OWN count, then the display
 * transform); out_spp rows*width samples taken; out_q rows*width the final Q.  Afterwards spira_counters.samples is the sum of out_spp,
 * and launches, passes (round 0's passes + the refinement rounds) and kernel_ms cover the whole call.
 * The host reads the length of the active list once per round to size the next launch: these entries SYNCHRONISE their stream once per
 * round — the *_device_* form too, which is otherwise asynchronous like the other device entries. */
typedef struct spira_adaptive {
    uint32_t min_spp, batch_spp;
    double   tolerance, floor;
} spira_adaptive;            /* 24 bytes */
int spira_render_adaptive_f32(const float *spheres5, const float *materials8, const float *triangles10,
                              const float camera12[12], const spira_params *params, const spira_adaptive *adaptive,
                              float *out_hdr, float *out_img, uint32_t *out_spp, float *out_q);
int spira_render_adaptive_f64(const double *spheres5, const double *materials8, const double *triangles10,
                              const double camera12[12], const spira_params *params, const spira_adaptive *adaptive,
                              double *out_hdr, double *out_img, uint32_t *out_spp, double *out_q);
int spira_render_adaptive_scene_f32(const spira_scene *scene, const float camera12[12], const spira_params *params, const spira_adaptive *adaptive,
                                    float *out_hdr, float *out_img, uint32_t *out_spp, float *out_q);
int spira_render_adaptive_scene_f64(const spira_scene *scene, const double camera12[12], const spira_params *params, const spira_adaptive *adaptive,
                                    double *out_hdr, double *out_img, uint32_t *out_spp, double *out_q);
int spira_render_adaptive_scene_device_f32(const spira_scene *scene, const float camera12[12], const spira_params *params, const spira_adaptive *adaptive,
                                           float *d_out_hdr, float *d_out_img, uint32_t *d_out_spp, float *d_out_q, void *stream);
int spira_render_adaptive_scene_device_f64(const spira_scene *scene, const double camera12[12], const spira_params *params, const spira_adaptive *adaptive,
                                           double *d_out_hdr, double *d_out_img, uint32_t *d_out_spp, double *d_out_q, void *stream);
/* The rule as host arithmetic (the same inline function the kernels call; no device needed): 1 converged, 0 not, or a negative
 * SPIRA_E_* code (sum3 NULL, n outside 1 .. 2^24, tolerance or floor negative or NaN). */
int spira_adaptive_converged_f32(const float sum3[3], float q, uint32_t n, double tolerance, double floor);
int spira_adaptive_converged_f64(const double sum3[3], double q, uint32_t n, double tolerance, double floor);

/* ---- all-sky pixels (Float64 pixel-owning passes, SPIRA_SKY_RUNS) ----
 * Can any camera ray of pixel (i, j) (reference indices: 1 .. width, 1 .. height from the bottom row) meet any sphere?  The host arithmetic of the
 * function k_path asks (csrc/spira_sky.h; no device needed): 1 no ray of the pixel can — it sees the sky alone —, 0 one may, or a negative SPIRA_E_*
 * code (a NULL pointer).  It errs towards 0 only. */
int spira_sky_pixel_f64(const double camera12[12], uint32_t width, uint32_t height, uint32_t i, uint32_t j, const double *spheres5, uint32_t n_spheres);
/* Which spheres can they meet?  *out_mask: bit s is clear only if no camera ray of the pixel can meet sphere s (s < 32; spheres beyond have no bit and
 * count as reachable; every bit is set where the pixel's own guards fail).  k_path ORs the masks of a run's pixels and its camera rays test the spheres
 * whose bit is set (SPIRA_REACH_MASKS).  0, or a negative SPIRA_E_* code (a NULL pointer).  A bit errs towards set only. */
int spira_pixel_reach_f64(const double camera12[12], uint32_t width, uint32_t height, uint32_t i, uint32_t j, const double *spheres5, uint32_t n_spheres, uint32_t *out_mask);

/* ---- first-hit feature buffers: per-pixel albedo, normal and depth, the guides of the denoiser below ----
 * For samples 0 .. params->spp - 1 of each pixel: the camera ray every render entry takes (RNG key: global pixel, sample, bounce 0) and its closest
 * hit as the renderer finds it (t_min 0.001, the later object wins ties, the BVH walk for meshes).  A hit on an object at distance t contributes
 * albedo = the material's albedo triple, normal = the shading code's geometric normal (outward normalize(pos - centre) for a sphere, the unflipped
 * unit normalize(cross(e1, e2)) for a triangle) and depth = t; a miss contributes albedo (1, 1, 1), normal 0 and depth 0.  Each output is the sum
 * over the samples in sample order divided once by spp, in the call's precision, nothing fused; so depth > 0 exactly where some sample hit.
 * out_albedo, out_normal: 3 planes, out_depth: 1 plane, all planar rows*width; any may be NULL, not all.  Tiling (rows / row0 / stripe_*) and
 * SPIRA_ROWS_BOTTOM_UP as in every entry; max_depth is not used.  Scope: SPIRA_SEM_A with SPIRA_KERNEL_DEFAULT, both precisions, spheres, LDS
 * triangles and BVH meshes; any other estimator or organisation and the SPIRA_EXT_* flags are SPIRA_E_UNSUPPORTED.  The *_device_* form is
 * asynchronous on `stream` and ordered like every device entry.  spira_get_counters is not affected by these entries. */
int spira_render_features_f32(const float *spheres5, const float *materials8, const float *triangles10,
                              const float camera12[12], const spira_params *params,
                              float *out_albedo, float *out_normal, float *out_depth);
int spira_render_features_f64(const double *spheres5, const double *materials8, const double *triangles10,
                              const double camera12[12], const spira_params *params,
                              double *out_albedo, double *out_normal, double *out_depth);
int spira_render_features_scene_f32(const spira_scene *scene, const float camera12[12], const spira_params *params,
                                    float *out_albedo, float *out_normal, float *out_depth);
int spira_render_features_scene_f64(const spira_scene *scene, const double camera12[12], const spira_params *params,
                                    double *out_albedo, double *out_normal, double *out_depth);
int spira_render_features_scene_device_f32(const spira_scene *scene, const float camera12[12], const spira_params *params,
                                           float *d_out_albedo, float *d_out_normal, float *d_out_depth, void *stream);
int spira_render_features_scene_device_f64(const spira_scene *scene, const double camera12[12], const spira_params *params,
                                           double *d_out_albedo, double *d_out_normal, double *d_out_depth, void *stream);

/* ---- denoiser: a variance-guided, feature-guided a-trous filter on a WHOLE frame ----
 * color: 3 planes height*width (the out_hdr of a whole frame), required.  Optional guides, each independent of the others: variance (1 plane: the
 * variance of the pixel's MEAN luminance), albedo (3 planes), normal (3 planes), depth (1 plane).  out_hdr / out_img: 3 planes each, either may be
 * NULL, not both; out_hdr may alias color.  Limits: iterations 1 .. 6, sigma_l > 0, sigma_z > 0, post one of SPIRA_POST_*, width, height >= 1, else
 * SPIRA_E_INVALID.  Defaults that work: sigma_l = 4, sigma_z = 0.1, iterations = 5.
 * Arithmetic, all in the call's precision T in the written order, nothing fused, constants rounded to T once; luma(r, g, b) = (0.2126 r + 0.7152 g)
 * + 0.0722 b; k = [1/16, 1/4, 3/8, 1/4, 1/16]; max(x, 0) is x > 0 ? x : 0:
 *   prepare  albedo given: a = albedo + 0.001 per channel, c = color / a, ya = luma(a); else a = 1, c = color, ya = 1.
 *            variance given: v = variance / (ya * ya) with albedo, else v = variance.
 *   for it = 0 .. iterations - 1, s = 1 << it, at every pixel p:
 *            y_p = luma(c_p).  variance given: g_p = the 3x3 blur of v around p (taps in row-major order, coordinates clamped to the image, weights
 *            (1/4, 1/2, 1/4) x (1/4, 1/2, 1/4), g = g + w_k * v_k), den = (sigma_l * sigma_l) * g_p + 1e-12.
 *            The 25 taps q = p + s (dx, dy), dy = -2..2 outer, dx = -2..2 inner, taps outside the image skipped: w = k[dy+2] * k[dx+2];
 *            depth given: hit_p = z_p > 0, hit_q = z_q > 0; hit_p != hit_q: w = 0; both hit: the normal factor when normal is given, then
 *            t = max(1 - |z_p - z_q| / (sigma_z * max(z_p, z_q)), 0), w = w * (t * t); both miss: w as it is.
 *            depth NULL and normal given: the normal factor alone, at every tap.
 *            normal factor: e = max((n_p.x n_q.x + n_p.y n_q.y) + n_p.z n_q.z, 0), e squared six times, w = w * e.
 *            variance given: dl = y_p - y_q, t = max(1 - (dl * dl) / den, 0), w = w * (t * t).
 *            sw = sw + w, sc = sc + w * c_q per channel, sv = sv + (w * w) * v_q;  then c'_p = sc / sw, v'_p = sv / (sw * sw).
 *   finish   out_hdr = c * a, out_img = post(out_hdr).
 * The centre tap (dx = dy = 0) takes none of the depth, normal and luminance factors: it always weighs 9/64, so sw >= 9/64 for finite inputs.  (Its
 * depth and luminance factors are 1 in any case; its normal factor would be |n_p|^128, and a normal averaged over samples that partly missed is short
 * enough for that to underflow in Float32 and leave a silhouette pixel with 0 / 0.)  Non-finite inputs give unspecified values at the pixels they
 * reach, never a fault.
 * The host form copies in and out.  The *_device_* form takes DEVICE pointers and a stream, is ordered like every device entry, does not synchronise,
 * and allocates only on its first call at a given size (the workspaces stay in the device context until spira_shutdown). */
typedef struct spira_denoise {
    uint32_t width, height, iterations, post;
    double   sigma_l, sigma_z;
} spira_denoise;             /* 32 bytes */
int spira_denoise_f32(const float *color, const float *variance, const float *albedo, const float *normal, const float *depth,
                      const spira_denoise *dn, float *out_hdr, float *out_img);
int spira_denoise_f64(const double *color, const double *variance, const double *albedo, const double *normal, const double *depth,
                      const spira_denoise *dn, double *out_hdr, double *out_img);
int spira_denoise_device_f32(const float *d_color, const float *d_variance, const float *d_albedo, const float *d_normal, const float *d_depth,
                             const spira_denoise *dn, float *d_out_hdr, float *d_out_img, void *stream);
int spira_denoise_device_f64(const double *d_color, const double *d_variance, const double *d_albedo, const double *d_normal, const double *d_depth,
                             const spira_denoise *dn, double *d_out_hdr, double *d_out_img, void *stream);

/* ---- diagnostics: per-segment trace of chosen paths (parity tests compare geometry bitwise) ----
 * ijs: n_paths x [i, j, sample] with i in 1..width, j in 1..height (the loop indices of
 * examples/julia-raytracer.jl:392-397) and sample in 0..spp-1.  Outputs, per path and bounce b <
 * max_depth: prims = object index hit (spheres first, then triangles), -1 = miss, -2 = path
 * already ended; ts = hit distance; dirs = the segment's ray direction; radiance = the sample's
 * radiance (n_paths x 3). */
int spira_trace_paths_f32(const float *spheres5, const float *materials8, const float *triangles10,
                          const float camera12[12], const spira_params *params, uint32_t n_paths,
                          const uint32_t *ijs, int *prims, float *ts, float *dirs, float *radiance);
int spira_trace_paths_f64(const double *spheres5, const double *materials8, const double *triangles10,
                          const double camera12[12], const spira_params *params, uint32_t n_paths,
                          const uint32_t *ijs, int *prims, double *ts, double *dirs, double *radiance);

/* ---- post ---- */
/* In-place display transform of n host values (post = one of SPIRA_POST_*). Host arithmetic. */
int spira_tonemap_f32(float *values, uint64_t n, uint32_t post);

/* ---- helpers ---- */
/* Number of output rows a given stripe_rank renders (height rows, stripes of stripe_h). */
uint32_t spira_stripe_rows(uint32_t height, uint32_t stripe_h, uint32_t stripe_count, uint32_t stripe_rank);

#ifdef __cplusplus
}
#endif
#endif /* SPIRA_HIP_H */
