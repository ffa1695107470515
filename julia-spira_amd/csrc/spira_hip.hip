// spira_hip.hip — host side of libspira_hip.so: device contexts, workspaces, the wavefront
// pass loop and the C ABI declared in include/spira_hip.h.  gfx950 (MI355X) only.
//
// Replaces the host loops of render_hybrid_gpu (src/spira-metal-optimized.jl:1228-1343): the
// reference launches >= spp*(1 + max_depth*(12*n_spheres + 4)) synchronous kernels with host
// round trips per depth; here one pass = one launch of the persistent path kernel
// (mesh scenes: a parking launch + a fat-wave launch; SPIRA_KERNEL_BOUNCE: max_depth bounce kernels)
// + 1 resolve kernel, fully asynchronous on one HIP stream, the live-ray counts staying on the
// device, and a pass carries `slots` samples of every pixel of the tile at once.
// What a call launches and how large its workspaces are is decided in spira_plan.h (make_plan: pure arithmetic, swept on the CPU under sanitizers);
// here Impl<T>::render validates, plans, sizes the workspaces from the plan and calls the organisation's enqueue_* function, and verify_path_args
// checks every k_path launch against the buffers actually allocated.
// Every entry point that enqueues on a context runs inside a Session: open (context, lock, stream, ordered after the previous call's end) ... close
// (launch errors, the end event, a host caller's wait); render and adaptive render share prepare_path_call, FrameOut and begin/end_counters.  A launch
// that the device refuses its LDS for is a return code (launch_lds) which the launch helpers and enqueue_* functions hand up at the first refusal.
#include <hip/hip_runtime.h>
#include <sys/mman.h>
#include <rccl/rccl.h>      // types and prototypes only: librccl is opened at run time (dlopen), never linked
#include <dlfcn.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <condition_variable>
#include <mutex>
#include <new>
#include <string>
#include <thread>
#include <type_traits>
#include <vector>

#include "../../include/spira_hip.h"
#include "../../include/spira_spd.h"
#include "spira_device.h"
#include "spira_bvh.h"
#include "spira_validate.h"
#include "spira_plan.h"
#include "spira_adaptive.h"
#include "spira_denoise.h"
#include "spira_refit.h"
#include "spira_lbvh.h"
#include "spira_query.h"
#include "spira_radiance.h"
#include "spira_gather.h"
#include "spira_probe.h"
#include "spira_nearest.h"
#include "spira_hits.h"
#include "spira_knearest.h"
#include "spira_sweep.h"
#include "spira_overlap.h"
#include "spira_trioverlap.h"
#include "spira_sdf.h"

// The library is built from this one file as THREE translation units (Makefile), because what the optimiser does to one family of kernels it undoes
// on another (profiles/r03_compiler_flags.md):
//   SPIRA_TU_F32      spira_tu::Impl<float> (every Float32 entry: below) and every kernel its members launch, with -fno-slp-vectorize.  The SLP vectoriser pairs Float32
//                     operations into v_pk_mul/add/fma_f32 and pays for every pair with register moves: without it S1 runs 13 % and the closed box S3
//                     20 % faster in Float32 (Float64 has no packed arithmetic to form: indifferent, the mesh scene 4 % better off WITH the pass).
//   SPIRA_TU_F64MESH  the Float64 path kernels of mesh scenes (k_path<double, ., BVH = true, ...>), with the compiler's defaults.
//   SPIRA_TU_MAIN     the C ABI, the host runtime and every other Float64 kernel, with -mllvm -two-entry-phi-node-folding-threshold=1: SimplifyCFG then
//                     turns far fewer two-sided branches into selects, which is 4 % of k_path on S1 in Float64 (1 % on the closed box) — and 5.5 % the
//                     other way on the mesh kernels, hence their own unit.  (No effect on the Float32 kernels or the secondary Float64 ones.)
// None of the macros defined (make stats, tests): one translation unit, the compiler's defaults, Impl<T> instantiated where it is called.  The state below
// is shared by all units (inline variables of a named namespace: one instance in the library); the functions further down are internal to each unit, but
// for the members of spira_tu::Impl<T>, which is how a Float32 call that enters through the C ABI in the SPIRA_TU_MAIN unit ends up in the SPIRA_TU_F32 one:
// `extern template struct Impl<float>` in the first, `template struct Impl<float>` at the end of the second, and C++ does the rest.  Adding an entry: its declaration in
// Impl, its definition (out of class, NOT inline, outside the unnamed namespace its helpers live in), the C wrappers, the header, _binding.py.
#if (defined(SPIRA_TU_MAIN) + defined(SPIRA_TU_F32) + defined(SPIRA_TU_F64MESH)) > 1
#error "SPIRA_TU_MAIN, SPIRA_TU_F32 and SPIRA_TU_F64MESH are three different translation units"
#endif
struct spira_scene;
// A host-output frame rendered as `count` consecutive row slabs (render_host_slabs): slab `index` > 0 continues the call of slab 0 — same scene (already in
// the context's store), same counters and event brackets (they add up), and the caller holds the context's lock across all of them.
struct SlabCtl { uint32_t index, count; };
namespace spira_tu {
// Every entry that a Float32 call has to reach in the SPIRA_TU_F32 unit: one static member each, defined further down where its helpers are.  The members
// must NOT be inline (none defined in the class, none marked inline): an explicit instantiation declaration does not suppress an inline member, and the
// Float32 kernels it launches would be compiled into the SPIRA_TU_MAIN unit as well, with that unit's flags.  (An explicit instantiation takes the members
// in the order declared here, and the kernels of the SPIRA_TU_F32 unit come out in that order: a new member goes at the end.)
template <class T> struct Impl {
    static int render(const spira_scene *h, const T *spheres5, const T *materials8, const T *triangles10, const T *camera12, const spira_params *p,
                      T *out_hdr, T *out_img, bool out_on_device, void *user_stream,
                      bool progressive = false, uint32_t sample0 = 0, uint32_t *rng_states = nullptr, const SlabCtl *slab = nullptr);
    static int trace(const T *spheres5, const T *materials8, const T *triangles10, const T *camera12, const spira_params *p,
                     uint32_t n_paths, const uint32_t *ijs, int *prims, T *ts, T *dirs, T *radiance);
    static int render_adaptive(const spira_scene *h, const T *spheres5, const T *materials8, const T *triangles10, const T *camera12, const spira_params *p,
                               const spira_adaptive *ad, T *out_hdr, T *out_img, uint32_t *out_spp, T *out_q, bool out_on_device, void *user_stream);
    static int features(const spira_scene *h, const T *spheres5, const T *materials8, const T *triangles10, const T *camera12, const spira_params *p,
                        T *out_albedo, T *out_normal, T *out_depth, bool out_on_device, void *user_stream);
    static int scene_update(spira_scene *h, const T *spheres5, const T *materials8, const T *triangles10, const T *d_triangles10, bool device_form, void *user_stream);
    static int scene_rebuild(spira_scene *h, const T *triangles10, const T *d_triangles10, bool device_form, void *user_stream);
    static int cast(const spira_scene *h, const T *rays8, uint32_t n_rays, uint32_t flags, int *out_prim, T *out_t, T *out_normal, uint8_t *out_hit,
                    bool any, bool on_device, void *user_stream);
    static int nearest(const spira_scene *h, const T *points4, uint32_t n_points, uint32_t flags, int *out_prim, T *out_dist, T *out_point, uint32_t *out_trips,
                       bool on_device, void *user_stream);
    static int hits(const spira_scene *h, const T *rays8, uint32_t n_rays, uint32_t max_hits, uint32_t flags, int *out_prim, T *out_t, uint32_t *out_count,
                    bool on_device, void *user_stream);
    static int nearest_k(const spira_scene *h, const T *points4, uint32_t n_points, uint32_t max_near, uint32_t flags, int *out_prim, T *out_dist, T *out_point,
                         uint32_t *out_count, uint32_t *out_trips, bool on_device, void *user_stream);
    static int sweep(const spira_scene *h, const T *rays8, const T *radii, uint32_t n_sweeps, uint32_t flags, int *out_prim, T *out_t, T *out_point, T *out_normal,
                     uint8_t *out_hit, uint32_t *out_trips, bool any, bool on_device, void *user_stream);
    static int overlap(const spira_scene *h, const T *boxes10, uint32_t n_boxes, uint32_t max_list, uint32_t flags, int *out_prim, uint32_t *out_count, uint8_t *out_hit,
                       uint32_t *out_trips, bool any, bool on_device, void *user_stream);
    static int signed_distance(const spira_scene *h, const T *points4, uint32_t n_points, uint32_t flags, int *out_prim, T *out_dist, T *out_point, uint8_t *out_inside,
                               uint32_t *out_crossings, uint32_t *out_trips, bool on_device, void *user_stream);
    static int radiance(const spira_scene *h, const T *rays6, uint32_t n_rays, const spira_radiance *rp, T *sum_rgb, uint8_t *out_valid, bool on_device, void *user_stream);
    static int camera_rays(const T *camera12, const spira_lens *lens, T *rays6, bool on_device, void *user_stream);
    static int gather(const spira_scene *h, const T *points6, uint32_t n_points, const spira_radiance *rp, T *sum_rgb, uint8_t *out_valid, bool on_device, void *user_stream);
    static int gather_visible(const spira_scene *h, const T *points6, uint32_t n_points, const spira_gather_visible *gv, uint32_t *visible, uint8_t *out_valid,
                              bool on_device, void *user_stream);
    static int gather_rays(const T *points6, uint32_t n_points, uint32_t sample, uint64_t seed, uint32_t key0, T *rays6, bool on_device, void *user_stream);
    static int denoise(const T *color, const T *variance, const T *albedo, const T *normal, const T *depth, const spira_denoise *dn,
                       T *out_hdr, T *out_img, bool on_device, void *user_stream);
    static int probe_sh(const spira_scene *h, const T *points3, uint32_t n_points, const spira_radiance *rp, T *sum_sh, uint8_t *out_valid, bool on_device, void *user_stream);
    static int probe_rays(const T *points3, uint32_t n_points, uint32_t sample, uint64_t seed, uint32_t key0, T *rays6, bool on_device, void *user_stream);
    static int overlap_tri(const spira_scene *h, const T *triangles10, uint32_t n_tris, uint32_t max_list, uint32_t flags, int *out_prim, uint32_t *out_count,
                           uint8_t *out_hit, uint32_t *out_trips, bool any, bool on_device, void *user_stream);
};
// defined in the SPIRA_TU_F64MESH unit: launch_path<double> of a mesh scene (PathArgs::mesh_mode 0 or 1) and launch_path_resume<double> (mode 2)
int launch_path_mesh_f64(int R, dim3 grid, size_t lds, hipStream_t st, const spira::PathArgs<double> &a, int spec);
int launch_path_resume_f64(int R, dim3 grid, size_t lds, hipStream_t st, const spira::PathArgs<double> &a);
}
// The unit split of the Float32 entries, which the compiler enforces: this unit calls Impl<float> and instantiates none of it (the SPIRA_TU_F32 unit does,
// at the end of the file, after every member's definition).  Before every use.
#ifdef SPIRA_TU_MAIN
extern template struct spira_tu::Impl<float>;
#endif

namespace spira_host {

inline thread_local std::string tl_err;
inline thread_local int tl_device = 0;

inline int fail(int code, const std::string &msg) { tl_err = msg; return code; }

#define HIP_TRY(expr)                                                                                   \
    do {                                                                                                \
        hipError_t e_ = (expr);                                                                         \
        if (e_ != hipSuccess)                                                                           \
            return fail(SPIRA_E_HIP, std::string(#expr) + ": " + hipGetErrorString(e_));                \
    } while (0)

struct DevBuf {
    void *p = nullptr;
    size_t cap = 0;
    int ensure(size_t bytes) {
        if (bytes <= cap) return 0;
        if (p) { (void)hipFree(p); p = nullptr; cap = 0; }
        hipError_t e = hipMalloc(&p, bytes);
        if (e != hipSuccess) return fail(SPIRA_E_HIP, std::string("hipMalloc: ") + hipGetErrorString(e));
        cap = bytes;
        return 0;
    }
    void release() { if (p) { (void)hipFree(p); p = nullptr; cap = 0; } }
};

// A scene resident on one device: the flat arrays exactly as the ABI takes them (+ the BVH of a large mesh).
// The context owns one (re-uploaded per call, the BVH cached by a hash of the triangle bytes); every
// spira_scene handle owns one (validated, built and uploaded once by spira_scene_create_*).
struct SceneStore {
    DevBuf arrays, bvh_nodes, bvh_tris, bvh_tris32;      // (bvh_tris32: Float64 scenes only — the Float32 screening records of the walk)
    uint32_t ns = 0, nm = 0, nt = 0;
    uint64_t bvh_hash = 0; uint32_t bvh_n = 0, bvh_slots = 0; int bvh_prec = 0, bvh_depth = 0;
    bool moderate = false;                    // every coordinate / radius of ordinary magnitude (spira::scene_scale_moderate): speculative division pays
    bool moderate_s = true, moderate_t = true;      // ... its two halves, spheres and triangles: spira_scene_update_* replaces them one at a time
    // what a refit of the tree needs (spira_refit.h): the frame the tree was built in, the first slot of every level (+ n_slots at the end), and — allocated by
    // the first update — one Float32 box per triangle and per node slot, and the staged triangle array of a host-form update
    double bvh_centre[3] = {0, 0, 0}, bvh_scale = 1;
    std::vector<uint32_t> bvh_level_first;
    DevBuf refit_tbox, refit_nbox, refit_stage;
    void release() {
        arrays.release(); bvh_nodes.release(); bvh_tris.release(); bvh_tris32.release(); refit_tbox.release(); refit_nbox.release(); refit_stage.release();
        bvh_hash = 0; bvh_n = 0;
    }
};

// spira_scene_rebuild_* (spira_lbvh.h): what the host reads back, and the context's scratch carved for n triangles.  Named types: the kernels that do not
// depend on the precision live in one translation unit and are reached from the others through spira_tu::lbvh_topology.
struct LbvhSmall { unsigned long long nlo[3], hi[3]; uint32_t status, pad; uint32_t totals[4]; };      // bounds as lbvh_enc codes (nlo: of the complement, so 0 is neutral for both)
struct LbvhWs {
    uint64_t *keys; uint32_t *idx;                 // lbvh_sort_size(n) of each: sorted in place
    spira::RefitBox *leafbox, *bbox;              // per triangle (original order); per binary node id
    int32_t *left, *right, *parent; uint32_t *counter;
    spira::LbvhPending *pending[2]; spira::LbvhMade *made;
    uint32_t *child_base, *tri_base, *next_at, *order;
};
struct LbvhTopo { uint32_t n_slots = 0; int depth = 0; std::vector<uint32_t> level_first; };

// Every device buffer of a context, and nothing else: release_all walks the struct as an array of DevBuf, so a buffer declared here is released at
// shutdown without being named there.  (What is not a DevBuf belongs in Ctx.)
struct CtxBuffers {
    DevBuf qA[2], qB[2], qC[2], qR[2], qK[2], qX[2], mesh_list, mesh_count, redo, L, accum, counts, blkstats, stats, out_tmp, trace, rng;
    DevBuf hyb_state, hyb_mat, hyb_flags;          // SPIRA_SEM_HYBRID: per-pixel ray state between its launches
    DevBuf spd32, spd64;                          // SPIRA_EXT_SPECTRAL: the SPD table, uploaded once per precision
    DevBuf multi_tile, multi_stack, multi_full;   // spira_render_multi_*: this device's tile; device 0: the gathered tiles, the frame
    DevBuf ad_q, ad_n, ad_list[2], ad_count;      // spira_render_adaptive_*: per-pixel Q and sample count, the two active lists, their two lengths
    DevBuf dn_rec[2], dn_guide, dn_io;            // spira_denoise_*: the ping-pong colour records, the guide records, the host form's staged planes
    DevBuf list_io;                               // the list calls (cast, closest point, radiance, the gathers): a host form's staged list and outputs.  ONE buffer for all
                                                  // of them: a host-form call synchronises before it returns, so a later call of another kind may reuse or regrow it
                                                  // (ensure only grows); the device forms never touch it
    DevBuf refit_status;                          // spira_scene_update_device_*: the status word of the check kernel
    DevBuf lbvh_ws, lbvh_nodes, lbvh_small;      // spira_scene_rebuild_*: keys / binary tree / level lists, the new node slots, status + bounds + counts
    void release_all();
};
static_assert(std::is_standard_layout_v<CtxBuffers> && sizeof(CtxBuffers) % sizeof(DevBuf) == 0, "CtxBuffers holds DevBuf members only");
inline void CtxBuffers::release_all() {
    DevBuf *b = reinterpret_cast<DevBuf *>(this);
    for (size_t i = 0; i < sizeof(CtxBuffers) / sizeof(DevBuf); ++i) b[i].release();
}

struct Ctx : CtxBuffers {
    bool init = false;
    int device = -1;
    int num_cus = 256;
    hipStream_t stream = nullptr;
    hipStream_t copy_stream = nullptr;        // host-output frames rendered as row slabs: a slab's copies run here, beside the next slab's kernels
    hipEvent_t ev_slab = nullptr;
    uint32_t *h_ad_count = nullptr;           // pinned: the length of an adaptive render's active list (ad_count), read by the host once per round
    uint32_t *h_refit_status = nullptr;       // pinned: where the host reads refit_status
    struct LbvhSmall *h_lbvh = nullptr;       // pinned: where the host reads lbvh_small
    std::vector<void *> lbvh_retired;         // node scratch outgrown in the middle of a rebuild: freed by the next one (a free waits for the device)
    SceneStore scene;                         // the scene of the current call (host-array entry points)
    spira::Stats *h_stats = nullptr;          // pinned
    void *h_stage = nullptr; size_t h_stage_cap = 0;   // pinned staging of a host-output frame (copy_out below)
    std::vector<hipEvent_t> stage_ev;         // one per chunk in flight
    hipEvent_t ev_start = nullptr, ev_stop = nullptr;
    hipEvent_t ev_done = nullptr;             // end of the last call that used the workspaces, on whatever stream it ran
    bool have_done = false;
    std::vector<hipEvent_t> ev_pool;          // profile mode: pairs around bounce launches
    size_t ev_used = 0;
    std::vector<hipEvent_t> ev_mid;           // mesh passes run as two launches: one event between them (-> spira_counters.walk_kernel_ms)
    std::vector<size_t> ev_mid_end;           // ... and the ev_pool index of the event that closes that pass's bracket
    size_t ev_mid_used = 0;
    spira_counters last{};
    uint64_t own_passes = 0;                  // passes of the call being enqueued that run k_path_own (counted as they are enqueued; slabs add up) ...
    uint64_t last_own_passes = 0;             // ... and spira_get_own_passes: that count as end_counters latched it, of the render spira_get_counters describes
    uint64_t last_sky_pixels = 0;             // spira_get_sky_pixels: Stats::sky_pixels of the same render (spira_counters keeps its layout)
    bool last_valid = false, last_pending = false;
    hipStream_t last_stream = nullptr;
    std::recursive_mutex mu;                  // (recursive: a host-output frame rendered as row slabs holds it across its slabs' render calls)
};

constexpr int kMaxDevices = 16;
inline Ctx g_ctx[kMaxDevices];

}  // namespace spira_host
using namespace spira_host;
namespace spira_tu {      // defined in the SPIRA_TU_MAIN unit (or the single one): sort, radix tree, boxes and collapse of a rebuild — nothing of it reads T
int lbvh_topology(Ctx &c, hipStream_t st, uint32_t n, const LbvhWs &w, LbvhTopo &out);
}

// The opaque scene handle of the C ABI (spira_scene_create_* / spira_scene_destroy).
struct spira_scene {
    uint32_t magic;        // kSceneMagic while alive
    int device;
    int prec;              // sizeof(T) the scene was created in
    SceneStore store;
    bool multi = false;    // made by spira_scene_create_multi_* (whatever its device count): spira_scene_update_* does not take it
    // spira_scene_create_multi_*: the same scene resident on devices 1 .. n_replicas-1 as well (this handle is device 0's)
    int n_replicas = 1;
    spira_scene *replica[16] = {};
};

namespace {
constexpr uint32_t kSceneMagic = 0x53504952u;   // "SPIR"

int get_ctx(Ctx **out) {
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n <= 0)
        return fail(SPIRA_E_NO_DEVICE, std::string("no HIP device: ") + (e != hipSuccess ? hipGetErrorString(e) : "device count is 0"));
    if (tl_device < 0 || tl_device >= n || tl_device >= kMaxDevices) return fail(SPIRA_E_INVALID, "device index out of range");
    Ctx &c = g_ctx[tl_device];
    HIP_TRY(hipSetDevice(tl_device));
    std::lock_guard<std::recursive_mutex> init_lock(c.mu);     // two threads must not initialise one context twice
    if (!c.init) {
        hipDeviceProp_t prop;
        HIP_TRY(hipGetDeviceProperties(&prop, tl_device));
        if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0)
            return fail(SPIRA_E_NO_DEVICE, std::string("libspira_hip is built for gfx950 only, found ") + prop.gcnArchName);
        c.num_cus = prop.multiProcessorCount;
        c.device = tl_device;
        HIP_TRY(hipStreamCreateWithFlags(&c.stream, hipStreamNonBlocking));
        HIP_TRY(hipEventCreate(&c.ev_start));
        HIP_TRY(hipEventCreate(&c.ev_stop));
        HIP_TRY(hipEventCreateWithFlags(&c.ev_done, hipEventDisableTiming));
        HIP_TRY(hipHostMalloc((void **)&c.h_stats, sizeof(spira::Stats), hipHostMallocDefault));
        c.init = true;
    }
    *out = &c;
    return 0;
}

// SPIRA_LOG_TIMING=1: host-side phase times of a call on stderr (where a first call's milliseconds go: context, validation, tree build, uploads, launches)
struct Lap {
    bool on; const char *what; std::chrono::steady_clock::time_point t0, t;
    explicit Lap(const char *w) : on(std::getenv("SPIRA_LOG_TIMING") != nullptr), what(w) { if (on) { t0 = t = std::chrono::steady_clock::now(); std::fprintf(stderr, "[spira %s]", what); } }
    void operator()(const char *phase) {
        if (!on) return;
        const auto n = std::chrono::steady_clock::now();
        std::fprintf(stderr, " %s %.3f", phase, std::chrono::duration<double, std::milli>(n - t).count());
        t = n;
    }
    ~Lap() { if (on) std::fprintf(stderr, " | total %.3f ms\n", std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count()); }
};

uint32_t env_u32(const char *name, uint32_t dflt) {
    const char *s = std::getenv(name);
    if (!s || !*s) return dflt;
    return (uint32_t)std::strtoul(s, nullptr, 10);
}

uint32_t stripe_rows(uint32_t height, uint32_t sh, uint32_t n, uint32_t r) {
    if (sh == 0 || n == 0) return 0;
    uint32_t rows = 0;
    for (uint32_t y0 = r * sh; y0 < height; y0 += n * sh) rows += std::min(sh, height - y0);
    return rows;
}

// Scene arrays: pointers, counts, material indices, finiteness (spira_validate.h) and the LDS budget.
template <class T>
int validate_scene(const T *spheres5, const T *materials8, const T *triangles10, uint32_t n_spheres, uint32_t n_materials, uint32_t nt) {
    if (n_spheres > SPIRA_MAX_LDS_SPHERES) return fail(SPIRA_E_LIMIT, "more than 1024 spheres");
    if (nt > SPIRA_MAX_TRIANGLES) return fail(SPIRA_E_LIMIT, "more than 2^24 triangles");
    const char *msg = nullptr;
    if (int rc = spira::scene_arrays_check<T>(spheres5, materials8, triangles10, n_spheres, n_materials, nt, &msg)) return fail(rc, msg);
    if (spira::scene_lds_bytes<T>(n_spheres, n_materials, nt > SPIRA_LDS_TRIANGLES ? 0 : nt) > 120 * 1024)
        return fail(SPIRA_E_LIMIT, "scene does not fit in LDS");
    return 0;
}

// Render parameters (nt = triangles actually present in the scene of this call).
int validate_params(const void *camera12, const spira_params *p, uint32_t nt, uint32_t *rows_out) {
    if (!p) return fail(SPIRA_E_INVALID, "params is NULL");
    if (!camera12) return fail(SPIRA_E_INVALID, "camera12 is NULL");
    if (p->width < 2 || p->height < 2) return fail(SPIRA_E_INVALID, "width and height must be >= 2 (u = (i-1+rand)/(W-1))");
    if ((uint64_t)p->width * p->height > 0x7FFFFFFFull) return fail(SPIRA_E_LIMIT, "image larger than 2^31 pixels");
    if (p->spp < 1 || p->spp > SPIRA_MAX_SPP) return fail(SPIRA_E_LIMIT, "spp out of range [1, 2^24]");
    if (p->max_depth > SPIRA_MAX_DEPTH) return fail(SPIRA_E_LIMIT, "max_depth > 255");
    const uint32_t sem = p->flags & SPIRA_SEM_MASK;
    if (sem != SPIRA_SEM_A && sem != SPIRA_SEM_CPU && sem != SPIRA_SEM_METAL && sem != SPIRA_SEM_HYBRID) return fail(SPIRA_E_UNSUPPORTED, "unknown integrator semantics");
    if (sem != SPIRA_SEM_A && nt) return fail(SPIRA_E_UNSUPPORTED, "SPIRA_SEM_CPU / SPIRA_SEM_METAL / SPIRA_SEM_HYBRID are sphere-only, like their sources");
    if (sem == SPIRA_SEM_HYBRID && p->rows != 0)
        return fail(SPIRA_E_UNSUPPORTED, "SPIRA_SEM_HYBRID renders whole images only (the reference ends a sample when no ray of the IMAGE hits anything): rows must be 0");
    uint32_t kern = p->flags & SPIRA_KERNEL_MASK;
    if (kern != SPIRA_KERNEL_DEFAULT && kern != SPIRA_KERNEL_WAVEFRONT && kern != SPIRA_KERNEL_MEGA && kern != SPIRA_KERNEL_BOUNCE) return fail(SPIRA_E_UNSUPPORTED, "unknown kernel organisation");
    if (p->flags & (SPIRA_EXT_DIELECTRIC | SPIRA_EXT_SPECTRAL)) {
        if (sem != SPIRA_SEM_A) return fail(SPIRA_E_UNSUPPORTED, "SPIRA_EXT_* extensions apply to SPIRA_SEM_A only");
        if (kern == SPIRA_KERNEL_BOUNCE) return fail(SPIRA_E_UNSUPPORTED, "SPIRA_EXT_* extensions are not built into the per-bounce organisation");
    }
    uint32_t rows = p->rows;
    if (rows == 0) rows = p->height;
    else if (p->stripe_count > 1) {
        if (p->stripe_h == 0 || p->stripe_rank >= p->stripe_count) return fail(SPIRA_E_INVALID, "bad stripe parameters");
        if (rows != stripe_rows(p->height, p->stripe_h, p->stripe_count, p->stripe_rank))
            return fail(SPIRA_E_INVALID, "rows != spira_stripe_rows(height, stripe_h, stripe_count, stripe_rank)");
    } else if ((uint64_t)p->row0 + rows > p->height) return fail(SPIRA_E_INVALID, "row0 + rows > height");
    *rows_out = rows;
    return 0;
}

template <class T>
void fill_const(spira::RenderConst<T> &rc, const T *cam, const spira_params *p, uint32_t rows, uint32_t slots) {
    rc.cam_origin = {cam[0], cam[1], cam[2]};
    rc.cam_llc = {cam[3], cam[4], cam[5]};
    rc.cam_hor = {cam[6], cam[7], cam[8]};
    rc.cam_ver = {cam[9], cam[10], cam[11]};
    rc.width = p->width; rc.height = p->height; rc.spp = p->spp; rc.max_depth = p->max_depth;
    uint32_t lo = (uint32_t)p->seed, hi = (uint32_t)(p->seed >> 32);
    rc.sA = spira::mix32(spira::mix32(lo + 0x9E3779B9u) ^ hi);
    rc.sB = spira::mix32(spira::mix32(hi + 0x85EBCA6Bu) ^ lo);
    rc.flags = p->flags;
    rc.rows = rows;
    if (p->rows == 0) { rc.row0 = 0; rc.stripe_h = 0; rc.stripe_count = 0; rc.stripe_rank = 0; }
    else { rc.row0 = p->row0; rc.stripe_h = p->stripe_h; rc.stripe_count = p->stripe_count; rc.stripe_rank = p->stripe_rank; }
    rc.tile_pixels = rows * p->width;
    rc.slots = slots;
    rc.sample0 = 0;
    rc.fd_tile = spira::fastdiv_make(rc.tile_pixels);
    rc.fd_width = spira::fastdiv_make(rc.width);
    rc.fd_stripe = spira::fastdiv_make(rc.stripe_h ? rc.stripe_h : 1);
}

// The magic-number division is exact by construction; verify it anyway on the values a render can see.
bool fastdiv_selfcheck(uint32_t d, uint32_t n_max) {
    const spira::FastDiv f = spira::fastdiv_make(d);
    uint32_t probes[] = {0u, 1u, d - 1, d, d + 1, 2 * d - 1, 2 * d, n_max / 2, n_max - 1, n_max, 0x7FFFFFFFu, 0xFFFFFFFFu};
    for (uint32_t n : probes)
        if (spira::fastdiv(n, f) != n / d) return false;
    uint32_t x = 0x12345u;
    for (int i = 0; i < 512; ++i) {
        x = spira::mix32(x + i);
        if (spira::fastdiv(x, f) != x / d) return false;
    }
    return true;
}

template <class T>
void scene_pointers(const SceneStore &s, spira::SceneGlobal<T> &g) {
    const bool use_bvh = s.nt > SPIRA_LDS_TRIANGLES;
    const uint32_t nt_lds = use_bvh ? 0 : s.nt;
    auto up = [](size_t b) { return (b + 255) & ~(size_t)255; };
    const size_t ns_b = (size_t)s.ns * 5 * sizeof(T), nm_b = (size_t)s.nm * 8 * sizeof(T);
    char *base = (char *)s.arrays.p;
    g.spheres5 = (const T *)base;
    g.materials8 = (const T *)(base + up(ns_b));
    g.triangles10 = (const T *)(base + up(ns_b) + up(nm_b));
    g.n_spheres = s.ns; g.n_materials = s.nm; g.n_triangles = nt_lds;
    g.bvh_nodes = use_bvh ? (const uint4 *)s.bvh_nodes.p : nullptr;
    g.bvh_frame = use_bvh ? (const spira::Pack4<T> *)s.bvh_tris.p : nullptr;          // 3 packets ahead of the triangles
    g.bvh_tris = use_bvh ? (const spira::Pack4<T> *)s.bvh_tris.p + 3 : nullptr;
    g.bvh_tris32 = (use_bvh && sizeof(T) == 8) ? (const uint4 *)s.bvh_tris32.p : nullptr;
    g.n_bvh_tris = use_bvh ? s.nt : 0;
    g.bvh_slots = use_bvh ? s.bvh_slots : 0;
}

// A mesh's tree as built on the host: one build can be uploaded to several devices (spira_scene_create_multi_*).
template <class T> struct HostBvh {
    spira::RawVec<uint32_t> nodes;
    spira::RawVec<spira::HostPack4<T>> tris;
    spira::RawVec<spira::HostPack4<float>> tris32;          // Float64 only
    spira::HostPack4<T> frame[3];
    uint32_t slots = 0; int depth = 0; bool built = false;
    std::vector<uint32_t> level_first;                      // BvhFrame::level_first[0 .. depth]
};
template <class T>
int host_bvh_build(const T *triangles10, uint32_t nt, HostBvh<T> &hb) {
    spira::BvhFrame<T> fr{};
#ifdef SPIRA_BVH_SCREEN
    constexpr bool kScreenRecords = sizeof(T) == 8;      // experiment build: Float64 walks screen their triangles in Float32 (spira_device.h, tri_screen_f32)
#else
    constexpr bool kScreenRecords = false;
#endif
    if (!spira::bvh_build<T>(triangles10, nt, hb.nodes, hb.tris, fr, 0, kScreenRecords ? &hb.tris32 : nullptr))
        return fail(SPIRA_E_LIMIT, "BVH build failed (tree too deep / too many triangles)");
    hb.frame[0] = {fr.root_mn[0], fr.root_mn[1], fr.root_mn[2], (T)0}; hb.frame[1] = {fr.root_mx[0], fr.root_mx[1], fr.root_mx[2], (T)0};
    hb.frame[2] = {fr.centre[0], fr.centre[1], fr.centre[2], fr.scale};
    hb.slots = fr.n_slots; hb.depth = fr.depth; hb.built = true;
    hb.level_first.assign(fr.level_first, fr.level_first + fr.depth + 1);
    return 0;
}

// Upload host arrays into `s`.  The small arrays go asynchronously on `st`; a mesh above SPIRA_LDS_TRIANGLES gets a
// BVH built on the host (once per distinct triangle array: keyed by a hash of its bytes) and copied synchronously —
// `prev_done` (the event of the last call that may still be traversing the old tree) is waited for first.
template <class T>
int scene_upload(SceneStore &s, hipStream_t st, hipEvent_t prev_done, const T *spheres5, const T *materials8, const T *triangles10,
                 uint32_t n_spheres, uint32_t n_materials, uint32_t nt, HostBvh<T> *shared = nullptr) {
    const bool use_bvh = nt > SPIRA_LDS_TRIANGLES;
    const uint32_t nt_lds = use_bvh ? 0 : nt;
    auto up = [](size_t b) { return (b + 255) & ~(size_t)255; };
    const size_t ns_b = (size_t)n_spheres * 5 * sizeof(T), nm_b = (size_t)n_materials * 8 * sizeof(T), nt_b = (size_t)nt_lds * 10 * sizeof(T);
    Lap lap("scene_upload");
    if (int rc = s.arrays.ensure(up(ns_b) + up(nm_b) + up(nt_b) + 256)) return rc;
    s.ns = n_spheres; s.nm = n_materials; s.nt = nt;
    s.moderate_s = spira::scene_scale_moderate<T>(spheres5, nullptr, n_spheres, 0);
    s.moderate_t = spira::scene_scale_moderate<T>(nullptr, triangles10, 0, nt);
    s.moderate = s.moderate_s && s.moderate_t;
    lap("alloc+scale");
    spira::SceneGlobal<T> g;
    scene_pointers<T>(s, g);
    if (ns_b) HIP_TRY(hipMemcpyAsync((void *)g.spheres5, spheres5, ns_b, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync((void *)g.materials8, materials8, nm_b, hipMemcpyHostToDevice, st));
    if (nt_b) HIP_TRY(hipMemcpyAsync((void *)g.triangles10, triangles10, nt_b, hipMemcpyHostToDevice, st));
    if (use_bvh) {
        // the context's store keeps the tree of the last mesh it saw, found again by a hash of the triangle bytes; a handle's store is filled once (no hash)
        const uint64_t h = shared ? 0 : spira::bytes_hash64(triangles10, (size_t)nt * 10 * sizeof(T));
        lap("hash");
        if (shared || s.bvh_hash != h || s.bvh_n != nt || s.bvh_prec != (int)sizeof(T)) {
            HostBvh<T> local;
            HostBvh<T> &hb = shared ? *shared : local;
            if (!hb.built) { if (int rc = host_bvh_build<T>(triangles10, nt, hb)) return rc; }
            lap("bvh_build");
            if (prev_done) HIP_TRY(hipEventSynchronize(prev_done));      // nobody still reads the tree that is about to be replaced
            // (+ one record of padding each: a walk's trip loads 5 / 6 x 16 bytes from a node or a triangle alike, spira_device.h bvh8_step)
            if (int rc = s.bvh_nodes.ensure(hb.nodes.size() * sizeof(hb.nodes[0]) + 128)) return rc;
            if (int rc = s.bvh_tris.ensure(sizeof hb.frame + hb.tris.size() * sizeof(hb.tris[0]) + 128)) return rc;
            const size_t tris32_b = hb.tris32.size() * sizeof(spira::HostPack4<float>);
            if (tris32_b) { if (int rc = s.bvh_tris32.ensure(tris32_b + 128)) return rc; }
            lap("hipMalloc");
            // The three arrays go up as asynchronous copies out of the vectors pinned in place (hipHostRegister: ~11 MB for 82 k triangles in Float64;
            // a hipMemcpy from pageable memory is staged by the runtime chunk by chunk on this thread), one wait at the end: the host vectors may die
            // with this scope.  Pinning refused (a limit on locked memory): the plain copies.
            const size_t nodes_b = hb.nodes.size() * sizeof(hb.nodes[0]), tris_b = hb.tris.size() * sizeof(hb.tris[0]);
            const bool pin_n = hipHostRegister(hb.nodes.data(), nodes_b, hipHostRegisterDefault) == hipSuccess;
            const bool pin_t = hipHostRegister(hb.tris.data(), tris_b, hipHostRegisterDefault) == hipSuccess;
            const bool pin_s = tris32_b && hipHostRegister(hb.tris32.data(), tris32_b, hipHostRegisterDefault) == hipSuccess;
            if (!pin_n || !pin_t || (tris32_b && !pin_s)) (void)hipGetLastError();
            hipError_t e1 = hipMemcpyAsync(s.bvh_nodes.p, hb.nodes.data(), nodes_b, hipMemcpyHostToDevice, st);
            hipError_t e2 = hipMemcpyAsync(s.bvh_tris.p, hb.frame, sizeof hb.frame, hipMemcpyHostToDevice, st);
            hipError_t e3 = hipMemcpyAsync((char *)s.bvh_tris.p + sizeof hb.frame, hb.tris.data(), tris_b, hipMemcpyHostToDevice, st);
            hipError_t e5 = tris32_b ? hipMemcpyAsync(s.bvh_tris32.p, hb.tris32.data(), tris32_b, hipMemcpyHostToDevice, st) : hipSuccess;
            hipError_t e4 = hipStreamSynchronize(st);
            if (pin_n) (void)hipHostUnregister(hb.nodes.data());
            if (pin_t) (void)hipHostUnregister(hb.tris.data());
            if (pin_s) (void)hipHostUnregister(hb.tris32.data());
            HIP_TRY(e1); HIP_TRY(e2); HIP_TRY(e3); HIP_TRY(e5); HIP_TRY(e4);
            lap("pin+copy");
            const int depth = hb.depth;
            s.bvh_slots = hb.slots;
            s.bvh_hash = h; s.bvh_n = nt; s.bvh_prec = (int)sizeof(T); s.bvh_depth = depth;
            s.bvh_centre[0] = (double)hb.frame[2].x; s.bvh_centre[1] = (double)hb.frame[2].y; s.bvh_centre[2] = (double)hb.frame[2].z; s.bvh_scale = (double)hb.frame[2].w;
            s.bvh_level_first = hb.level_first;
        }
    }
    return 0;
}

// Launch with a dynamic LDS block; above 64 KB the function has to be told first (up to the CU's 160 KB).
// A refused opt-in launches nothing and is the call's error (SPIRA_E_LIMIT): every launch helper and enqueue function hands it up at once.
template <class K, class... Args>
int launch_lds(K kernel, dim3 grid, dim3 block, size_t lds, hipStream_t st, Args... args) {
    if (lds > 64 * 1024) {
        const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess)          // do not launch a kernel that cannot get its LDS
            return fail(SPIRA_E_LIMIT, std::string("the device refused the kernel's dynamic LDS size (hipFuncSetAttribute): ") + hipGetErrorString(e));
    }
    hipLaunchKernelGGL(kernel, grid, block, lds, st, args...);
    return 0;
}

template <class T, bool FIRST, bool BVH>
int launch_bounce_r(int R, dim3 grid, size_t lds, hipStream_t st, const spira::BounceArgs<T> &a) {
    switch (R) {
    case 2: return launch_lds(spira::k_bounce<T, FIRST, 2, BVH>, grid, dim3(spira::kBlock), lds, st, a);
    default: return launch_lds(spira::k_bounce<T, FIRST, 1, BVH>, grid, dim3(spira::kBlock), lds, st, a);
    }
}
template <class T, bool FIRST>
int launch_bounce(int R, dim3 grid, size_t lds, hipStream_t st, const spira::BounceArgs<T> &a) {
    if (a.scene.n_bvh_tris) return launch_bounce_r<T, FIRST, true>(R, grid, lds, st, a);
    return launch_bounce_r<T, FIRST, false>(R, grid, lds, st, a);
}

// k_path.  `spec`: the speculative-division instantiation first (PathArgs::redo = its per-wave report), then the exact one over the
// waves it reported (spira_device.h, SpecDiv) — two launches, the second normally a grid of workgroups that return at once.
// spec == 2 (SPIRA_SPEC_DIV=2, tests): every wave is reported, i.e. the whole pass is rendered twice.
// MODE: PathArgs::mesh_mode as a template argument (mesh scenes: 0 one launch, 1 the parking launch of two; 2 is launch_path_resume below).
// TRI = false: the scene holds no LDS-resident triangles (spheres only, or spheres + a BVH mesh): instantiations without the triangle scan
// own_kernel (spira_plan.h, own_kernel_ok; verify_path_args has checked it against `a`): k_path_own instead of k_path, the same two launches.
template <class T, bool BVH, int MODE>
int launch_path_mode(int R, dim3 grid, size_t lds, hipStream_t st, spira::PathArgs<T> a, int spec, bool own_kernel = false) {
    const bool ext = (a.rc.flags & (SPIRA_EXT_DIELECTRIC | SPIRA_EXT_SPECTRAL)) != 0;
    const bool tri = a.scene.n_triangles != 0;
    const dim3 blk(spira::kBlock);
    if (own_kernel) {
#if defined(SPIRA_TU_MAIN) || !(defined(SPIRA_TU_F32) || defined(SPIRA_TU_F64MESH))
        if constexpr (sizeof(T) == 8 && !BVH && MODE == 0) {
            if (spec) {
                a.redo_only = spec == 2 ? 2 : 0;
                if (int rc = launch_lds(spira::k_path_own<T, true>, grid, blk, lds, st, a)) return rc;
                if (spec == 2) HIP_TRY(hipMemsetD32Async((hipDeviceptr_t)a.redo, 1, (size_t)grid.x * (spira::kBlock / 64), st));
                a.redo_only = 1;
            } else { a.redo = nullptr; a.redo_only = 0; }
            return launch_lds(spira::k_path_own<T, false>, grid, blk, lds, st, a);
        }
#endif
        return fail(SPIRA_E_LIMIT, "internal: k_path_own exists for Float64 sphere passes only");      // a missing kernel is an error, never another kernel
    }
    if (ext) {           // extension instantiations (R = 2 only); like the default kernels, without the LDS triangle scan where the scene has none
        if (spec) {
            a.redo_only = spec == 2 ? 2 : 0;          // (2: every wave will be rendered again, whatever it reports)
            if (int rc = tri ? launch_lds(spira::k_path<T, 2, BVH, true, true, MODE, true>, grid, blk, lds, st, a)
                             : launch_lds(spira::k_path<T, 2, BVH, true, true, MODE, false>, grid, blk, lds, st, a)) return rc;
            if (spec == 2) HIP_TRY(hipMemsetD32Async((hipDeviceptr_t)a.redo, 1, (size_t)grid.x * (spira::kBlock / 64), st));
            a.redo_only = 1;
        } else { a.redo = nullptr; a.redo_only = 0; }
        return tri ? launch_lds(spira::k_path<T, 2, BVH, true, false, MODE, true>, grid, blk, lds, st, a)
                   : launch_lds(spira::k_path<T, 2, BVH, true, false, MODE, false>, grid, blk, lds, st, a);
    } else if (R == 2) {
        if (spec) {
            a.redo_only = spec == 2 ? 2 : 0;
            if (int rc = tri ? launch_lds(spira::k_path<T, 2, BVH, false, true, MODE, true>, grid, blk, lds, st, a)
                             : launch_lds(spira::k_path<T, 2, BVH, false, true, MODE, false>, grid, blk, lds, st, a)) return rc;
            if (spec == 2) HIP_TRY(hipMemsetD32Async((hipDeviceptr_t)a.redo, 1, (size_t)grid.x * (spira::kBlock / 64), st));
            a.redo_only = 1;
        } else { a.redo = nullptr; a.redo_only = 0; }
        return tri ? launch_lds(spira::k_path<T, 2, BVH, false, false, MODE, true>, grid, blk, lds, st, a)
                   : launch_lds(spira::k_path<T, 2, BVH, false, false, MODE, false>, grid, blk, lds, st, a);
    }
    a.redo = nullptr; a.redo_only = 0;
    return launch_lds(spira::k_path<T, 1, BVH, false, false, MODE>, grid, blk, lds, st, a);
}
template <class T>
int launch_path(int R, dim3 grid, size_t lds, hipStream_t st, const spira::PathArgs<T> &a, int spec, bool own_kernel) {
    if (!a.scene.n_bvh_tris) return launch_path_mode<T, false, 0>(R, grid, lds, st, a, spec, own_kernel);
    if (own_kernel) return fail(SPIRA_E_LIMIT, "internal: k_path_own exists for Float64 sphere passes only");
#ifdef SPIRA_TU_MAIN
    if constexpr (sizeof(T) == 8) return spira_tu::launch_path_mesh_f64(R, grid, lds, st, a, spec);
    else
#endif
    {
        if (a.mesh_mode == 1) return launch_path_mode<T, true, 1>(R, grid, lds, st, a, spec);
        return launch_path_mode<T, true, 0>(R, grid, lds, st, a, spec);
    }
}

// the second launch of a mesh pass (PathArgs::mesh_mode 2): the exact instantiation — its waves add to radiance the first launch
// already stored, so they could not be rendered again, and its divisions are a small share of the frame's
template <class T>
int launch_path_resume(int R, dim3 grid, size_t lds, hipStream_t st, spira::PathArgs<T> a) {
    const bool ext = (a.rc.flags & (SPIRA_EXT_DIELECTRIC | SPIRA_EXT_SPECTRAL)) != 0;
    const dim3 blk(spira::kBlock);
    a.redo = nullptr; a.redo_only = 0;
    if (ext && a.scene.n_triangles) return launch_lds(spira::k_path<T, 2, true, true, false, 2, true>, grid, blk, lds, st, a);
    if (ext) return launch_lds(spira::k_path<T, 2, true, true, false, 2, false>, grid, blk, lds, st, a);
    if (R == 2 && a.scene.n_triangles) return launch_lds(spira::k_path<T, 2, true, false, false, 2, true>, grid, blk, lds, st, a);
    if (R == 2) return launch_lds(spira::k_path<T, 2, true, false, false, 2, false>, grid, blk, lds, st, a);
    return launch_lds(spira::k_path<T, 1, true, false, false, 2>, grid, blk, lds, st, a);
}

// launch_path_resume<T> of whichever translation unit holds the mesh kernels of T
template <class T>
int launch_path_resume_entry(int R, dim3 grid, size_t lds, hipStream_t st, const spira::PathArgs<T> &a) {
#ifdef SPIRA_TU_MAIN
    if constexpr (sizeof(T) == 8) return spira_tu::launch_path_resume_f64(R, grid, lds, st, a);
    else
#endif
        return launch_path_resume<T>(R, grid, lds, st, a);
}

int profile_events(Ctx &c, size_t need) {
    while (c.ev_pool.size() < need) {
        hipEvent_t e;
        HIP_TRY(hipEventCreate(&e));
        c.ev_pool.push_back(e);
    }
    return 0;
}

// Every call that touches the context's workspaces first makes its stream wait for the previous call's end
// (which may have run on ANOTHER stream and not have been synchronised): the workspaces are shared per device.
int order_after_previous(Ctx &c, hipStream_t st) {
    if (c.have_done) HIP_TRY(hipStreamWaitEvent(st, c.ev_done, 0));
    return 0;
}
int mark_done(Ctx &c, hipStream_t st) {
    HIP_TRY(hipEventRecord(c.ev_done, st));
    c.have_done = true;
    return 0;
}

// One call on the calling thread's device context.  open: the context exists, its lock is held until the Session dies, `st` is the caller's stream
// (device outputs) or the context's own, and `st` already waits for the end of the last call that used the workspaces — whatever is enqueued on it
// from here on may use them.  close: after the call's LAST enqueue on `st` (a host caller's copies out included): launch errors, the event the next
// call will wait for, and for a host caller the wait for its outputs.  An entry point validates its arguments, opens, sizes what it needs, enqueues, closes.
struct Session {
    Ctx *cp = nullptr;
    std::unique_lock<std::recursive_mutex> lock;
    hipStream_t st = nullptr;
    bool host_out = false;
    static int open(Session &s, bool out_on_device, void *user_stream) {
        if (int rc = get_ctx(&s.cp)) return rc;
        s.lock = std::unique_lock<std::recursive_mutex>(s.cp->mu);
        s.host_out = !out_on_device;
        s.st = out_on_device ? (hipStream_t)user_stream : s.cp->stream;
        return order_after_previous(*s.cp, s.st);
    }
    int close() {
        HIP_TRY(hipGetLastError());
        if (int rc = mark_done(*cp, st)) return rc;
        if (host_out) HIP_TRY(hipStreamSynchronize(st));
        return 0;
    }
};

// The caller's output buffer is usually fresh from the allocator (`render` of either reference surface returns a new array): its pages do not exist yet,
// and the first touch of 12 000 of them inside the copy costs 2-3 ms.  The threads that will move the frame in ask the kernel for the pages (writable,
// contents untouched) while the GPU is still rendering; only pages that lie wholly inside the buffer.  A kernel that does not know the request says
// EINVAL and the copy faults the pages in as before.
void prefault_destination(char *p, size_t n) {
    const uintptr_t pg = 4096, a = ((uintptr_t)p + pg - 1) & ~(pg - 1), b = ((uintptr_t)p + n) & ~(pg - 1);
    if (b > a) (void)madvise((void *)a, b - a, 23 /* MADV_POPULATE_WRITE (Linux 5.14) */);
}

// The context's pinned staging buffer, grown to `total` bytes.  false: no pinned memory to be had — the caller's plain path still works.
bool stage_reserve(Ctx &c, size_t total) {
    if (c.h_stage_cap >= total) return true;
    if (c.h_stage) { (void)hipHostFree(c.h_stage); c.h_stage = nullptr; c.h_stage_cap = 0; }
    if (hipHostMalloc(&c.h_stage, total, hipHostMallocDefault) == hipSuccess) { c.h_stage_cap = total; return true; }
    c.h_stage = nullptr; (void)hipGetLastError();
    return false;
}

// Device memory on its way to a host-pointer caller through the pinned staging buffer: stage() enqueues one piece (device -> staging, and an event
// behind it), move() has SPIRA_STAGE_THREADS host threads (4) carry the pieces on into the caller's memory as their events complete.
struct StagedCopy {
    struct Piece { char *dst; size_t off, len; };
    Ctx &c;
    std::vector<Piece> pieces;
    size_t off = 0;
    explicit StagedCopy(Ctx &ctx) : c(ctx) {}
    hipError_t stage(hipStream_t st, void *dst, const void *src, size_t len) {
        hipError_t e = hipMemcpyAsync((char *)c.h_stage + off, src, len, hipMemcpyDeviceToHost, st);
        if (e != hipSuccess) return e;
        if (c.stage_ev.size() <= pieces.size()) {
            hipEvent_t ev;
            if ((e = hipEventCreateWithFlags(&ev, hipEventDisableTiming)) != hipSuccess) return e;
            c.stage_ev.push_back(ev);
        }
        e = hipEventRecord(c.stage_ev[pieces.size()], st);
        pieces.push_back({(char *)dst, off, len});
        off += len;
        return e;
    }
    hipError_t move() {
        const int n_thr = (int)std::min<size_t>(std::max<uint32_t>(1, env_u32("SPIRA_STAGE_THREADS", 4)), pieces.size());
        std::vector<hipError_t> errs((size_t)n_thr, hipSuccess);
        const bool prefault = env_u32("SPIRA_PREFAULT", 1) != 0;
        auto mover = [&](int t) {
            (void)hipSetDevice(c.device);
            if (prefault) for (size_t i = (size_t)t; i < pieces.size(); i += (size_t)n_thr) prefault_destination(pieces[i].dst, pieces[i].len);
            for (size_t i = (size_t)t; i < pieces.size(); i += (size_t)n_thr) {
                const hipError_t e = hipEventSynchronize(c.stage_ev[i]);
                if (e != hipSuccess) { errs[(size_t)t] = e; return; }
                std::memcpy(pieces[i].dst, (const char *)c.h_stage + pieces[i].off, pieces[i].len);
            }
        };
        std::vector<std::thread> thr;
        for (int t = 1; t < n_thr; ++t) thr.emplace_back(mover, t);
        mover(0);
        for (auto &t : thr) t.join();
        for (hipError_t e : errs) if (e != hipSuccess) return e;
        return hipSuccess;
    }
};

// A frame for a host-pointer caller (`render` of either reference surface returns a host array).  hipMemcpy into pageable memory runs at
// ~9 GB/s on this box (the runtime stages it on one thread): 5.7 ms for a 1080p Float64 frame, as long as rendering it.  Instead: device ->
// pinned staging in 8 MB chunks (one event each), and four host threads move the chunks on into the caller's memory as they arrive: 4.3 ms
// (most of what is left is the first touch of the caller's freshly allocated pages, which no copy strategy removes).
// Synchronous (the host-pointer entries are); small outputs take the plain copy.  Returns with the stream drained up to the copies.
int copy_out(Ctx &c, hipStream_t st, void *const dst[2], const void *const src[2], size_t bytes_each) {
    const size_t kChunk = (size_t)std::max<uint32_t>(1, env_u32("SPIRA_STAGE_CHUNK_MB", 8)) << 20, kMinStaged = 4u << 20, kMaxStaged = 512u << 20;      // (threads and chunk size: flat between 4 and 16 threads, 2 and 8 MB; frames beyond 512 MB take the plain copy rather than pin as much host memory)
    const int n_out = (dst[0] ? 1 : 0) + (dst[1] ? 1 : 0);
    if (!n_out) return 0;
    const size_t total = bytes_each * (size_t)n_out;
    if (bytes_each < kMinStaged || total > kMaxStaged || !stage_reserve(c, total)) {
        for (int k = 0; k < 2; ++k) if (dst[k]) HIP_TRY(hipMemcpyAsync(dst[k], src[k], bytes_each, hipMemcpyDeviceToHost, st));
        return 0;
    }
    StagedCopy sc(c);
    for (int k = 0; k < 2; ++k)
        for (size_t o = 0; dst[k] && o < bytes_each; o += kChunk)
            HIP_TRY(sc.stage(st, (char *)dst[k] + o, (const char *)src[k] + o, std::min(kChunk, bytes_each - o)));
    const hipError_t e = sc.move();
    if (e != hipSuccess) return fail(SPIRA_E_HIP, std::string("copy_out: ") + hipGetErrorString(e));
    return 0;
}

// The scene of a call: host arrays (uploaded into the context's store) or a handle (already resident).
template <class T>
int acquire_scene(Ctx &c, hipStream_t st, const spira_scene *h, const T *spheres5, const T *materials8, const T *triangles10,
                  const spira_params *p, spira::SceneGlobal<T> &g, bool reuse = false) {
    if (h) { scene_pointers<T>(h->store, g); return 0; }
    if (reuse) { scene_pointers<T>(c.scene, g); return 0; }      // (a later slab of the call that uploaded it)
    const uint32_t nt = triangles10 ? p->n_triangles : 0;
    if (int rc = scene_upload<T>(c.scene, st, c.have_done ? c.ev_done : nullptr, spheres5, materials8, triangles10, p->n_spheres, p->n_materials, nt)) return rc;
    scene_pointers<T>(c.scene, g);
    return 0;
}

// SPIRA_EXT_SPECTRAL: the SPD table of include/spira_spd.h in the render precision, resident per context.
template <class T>
int attach_spd(Ctx &c, hipStream_t st, uint32_t flags, spira::SceneGlobal<T> &g) {
    g.spd = nullptr;
    if (!(flags & SPIRA_EXT_SPECTRAL)) return 0;
    DevBuf &b = sizeof(T) == 4 ? c.spd32 : c.spd64;
    if (!b.p) {
        static_assert(SPIRA_SPD_N == spira::kSpdN && SPIRA_SPD_ROWS == spira::kSpdRows, "SPD table shape");
        T host[SPIRA_SPD_ROWS * SPIRA_SPD_N];
        for (int r = 0; r < SPIRA_SPD_ROWS; ++r)
            for (int i = 0; i < SPIRA_SPD_N; ++i) host[r * SPIRA_SPD_N + i] = (T)spira_spd_table[r][i];
        if (int rc = b.ensure(sizeof host)) return rc;
        HIP_TRY(hipMemcpy(b.p, host, sizeof host, hipMemcpyHostToDevice));
    }
    (void)st;
    g.spd = (const T *)b.p;
    return 0;
}
template <class T>
int attach_spd(Ctx &c, hipStream_t st, const spira_params *p, spira::SceneGlobal<T> &g) { return attach_spd<T>(c, st, p->flags, g); }

template <class T>
int check_handle(const spira_scene *h) {
    if (!h || h->magic != kSceneMagic) return fail(SPIRA_E_INVALID, "scene handle is NULL or was destroyed");
    if (h->prec != (int)sizeof(T)) return fail(SPIRA_E_INVALID, "scene handle was created in the other precision");
    if (h->device != tl_device) return fail(SPIRA_E_INVALID, "scene handle belongs to another device (spira_set_device)");
    return 0;
}

// ---- the launch plan of a call (spira_plan.h): what spira_device.h and the environment contribute to it
spira::Knobs read_knobs() {
    spira::Knobs k;
    k.batch_rays = env_u32("SPIRA_BATCH_RAYS", k.batch_rays);
    k.R = env_u32("SPIRA_R", k.R);
    k.blocks_per_cu = env_u32("SPIRA_BLOCKS_PER_CU", 0);
    k.defer_mesh = env_u32("SPIRA_DEFER_MESH", 1); k.mesh_two_pass = env_u32("SPIRA_MESH_TWO_PASS", 1);
    k.fused_resolve = env_u32("SPIRA_FUSED_RESOLVE", 1); k.private_l = env_u32("SPIRA_PRIVATE_L", 1);
    k.spec_div = env_u32("SPIRA_SPEC_DIV", 1);
    // dense continuation threshold (same device, S1 1080p spp 64 depth 8, Msamples/s): f64 100 %: 20 218, 90: 20 563, 80: 20 953,
    // 70: 20 963, 60: 20 052; f32 90: 30 222, 80: 30 141, 70: 29 567, 60: 28 354 — a packet costs twice the bytes in Float64, so it
    // pays to keep a little more in registers there.  On the closed box S3 any threshold > 0 gives the full +22 % (f64).
    // Round 4 (packets carry the RNG key words: a queued hit costs more), S1 ms per frame, two rounds on one box: f64 80: 5.302 / 5.277, 75: 5.245 / 5.229,
    // 70: 5.221 / 5.240, 65: 5.272 / 5.299; f32 80: 3.382 / 3.414, 75: 3.341 / 3.354, 70: 3.340 / 3.351, 65: 3.374 / 3.351; configs[4] the same at 70 and 80.
    k.dense_pct = std::min<uint32_t>(env_u32("SPIRA_DENSE_PCT", 70), 100);      // (Float32 re-measured on the no-SLP build of round 3, S1: 90: 37 900, 85: 38 500, 80: 38 500, 75: 38 500, 70: 37 500)
    k.mesh_min_batch = std::max<uint32_t>(1, env_u32("SPIRA_MESH_MIN_BATCH", 128));
    k.mesh_refill = std::min<uint32_t>(64, std::max<uint32_t>(1, env_u32("SPIRA_MESH_REFILL", 16)));
    k.mesh_fat_waves_per_cu = env_u32("SPIRA_MESH_FAT_WAVES_PER_CU", 16);
    k.cam_consts = env_u32("SPIRA_CAM_CONSTS", 1);
    k.sky_runs = env_u32("SPIRA_SKY_RUNS", 1);
    k.pixel_table = env_u32("SPIRA_PIXEL_TABLE", 1); k.reach_masks = env_u32("SPIRA_REACH_MASKS", 1);
    k.own_kernel = env_u32("SPIRA_OWN_KERNEL", 1);
    return k;
}
template <class T>
spira::PlanIn plan_input(const Ctx &c, const spira_params *p, uint32_t rows, uint32_t nt_scene, bool progressive, bool caller_rng, bool out_on_device) {
    spira::PlanIn in;
    in.width = p->width; in.rows = rows; in.spp = p->spp; in.max_depth = p->max_depth; in.flags = p->flags; in.batch_rays = p->batch_rays;
    in.n_triangles = nt_scene; in.num_cus = (uint32_t)c.num_cus;
    in.progressive = progressive; in.caller_rng = caller_rng; in.out_on_device = out_on_device;
    in.prec = sizeof(T); in.block = spira::kBlock; in.waves_per_simd = SPIRA_WAVES_PER_SIMD(T); in.carry_key = SPIRA_CARRY_KEY;
    in.pack4 = sizeof(spira::Pack4<T>); in.pack3 = sizeof(spira::Pack3<T>); in.pack2 = sizeof(spira::Pack2<T>);
    in.k = read_knobs();
    return in;
}

// Every workspace of the context at the size the plan gives it: the one place that sizes them.
int ensure_workspaces(Ctx &c, const spira::Workspace &w) {
    for (int i = 0; i < 2; ++i) {
        if (int rc = c.qA[i].ensure(w.queue4)) return rc;
        if (int rc = c.qB[i].ensure(w.queue4)) return rc;
        if (int rc = c.qC[i].ensure(w.queue2)) return rc;
        if (int rc = c.qR[i].ensure(w.q_ref)) return rc;
        if (int rc = c.qK[i].ensure(w.q_key)) return rc;
        if (int rc = c.qX[i].ensure(w.q_x)) return rc;
    }
    const struct { DevBuf &b; uint64_t bytes; } rest[] = {
        {c.mesh_list, w.mesh_list}, {c.mesh_count, w.mesh_count}, {c.redo, w.redo}, {c.blkstats, w.blkstats}, {c.L, w.L}, {c.counts, w.counts},
        {c.stats, sizeof(spira::Stats)}, {c.accum, w.accum}, {c.out_tmp, w.out_tmp}, {c.rng, w.rng},
        {c.hyb_state, w.hyb_state}, {c.hyb_mat, w.hyb_mat}, {c.hyb_flags, w.hyb_flags}};
    for (const auto &r : rest)
        if (int rc = r.b.ensure(r.bytes)) return rc;
    return 0;
}

// Called right before every k_path launch: each pointer of PathArgs against the capacity of the buffer it points into, for the grid about to be
// launched (spira_plan.h, path_need); a launch that would not fit is refused (SPIRA_E_LIMIT) instead of letting a kernel write past a buffer nobody
// sized.  (Round 3's fuzz found exactly that: a depth-1 mesh render writing parked rays' hits into queues only `max_depth > 1` used to size.)
static_assert(sizeof(spira::PixelEntry) == spira::kPixelEntryBytes && spira::kOwnRuns * SPIRA_RESOLVE_RUN == 64, "own_lds_bytes sizes what k_path's prologue writes");
// (R, own_knob: Plan::R and Plan::own_kernel, which own_kernel_ok reads beside the arguments)
template <class T>
spira::PathLaunch path_launch_of(const spira::PathArgs<T> &a, uint32_t first_launch_blocks, size_t own_lds, uint32_t R, bool own_knob) {
    spira::PathLaunch l;
    l.blocks = first_launch_blocks; l.cap = a.cap; l.n_first = a.n_first; l.k_eff = a.k_eff;
    l.tile_pixels = a.rc.tile_pixels; l.max_depth = a.rc.max_depth; l.flags = a.rc.flags; l.n_lds_triangles = a.scene.n_triangles;
    l.mesh_mode = a.mesh_mode; l.resume_k = a.resume_k; l.resume_nw = a.resume_nw;
    l.mesh = a.scene.n_bvh_tris != 0; l.pixel_owning = a.accum != nullptr; l.l_private = a.l_private != 0;
    l.prec = sizeof(T); l.wpb = spira::kBlock / 64; l.carry_key = SPIRA_CARRY_KEY;
    l.pixel_table = a.pixel_table != 0; l.reach_masks = a.reach_masks != 0; l.own_lds = own_lds;
    l.R = R; l.n_spheres = a.scene.n_spheres; l.sky_runs = a.sky_runs != 0; l.cam_consts = a.cam_consts != 0; l.own_kernel = own_knob;
    return l;
}
// own_kernel: the launch is k_path_own's — refused unless that is exactly what own_kernel_ok says of these arguments
template <class T>
int verify_path_args(const Ctx &c, const spira::PathArgs<T> &a, uint32_t first_launch_blocks, size_t own_lds = 0, uint32_t R = 0, bool own_knob = false, bool own_kernel = false) {
    using P4 = spira::Pack4<T>;
    using P2 = spira::Pack2<T>;
    const spira::PathLaunch l = path_launch_of<T>(a, first_launch_blocks, own_lds, R, own_knob);
    const spira::PathNeed need = spira::path_need(l);
    const uint64_t nw = need.nw, n = need.packets;
    auto covers = [](const DevBuf &b, const void *ptr, uint64_t bytes) { return ptr == b.p && b.p != nullptr && b.cap >= bytes; };
    const char *bad = need.fits ? nullptr : "the pass does not fit its queue regions";
    if (a.rc.max_depth > 1 || l.mesh)
        for (int i = 0; i < 2 && !bad; ++i) {
            if (!covers(c.qA[i], a.q[i].A, n * sizeof(P4)) || !covers(c.qB[i], a.q[i].B, n * sizeof(P4)) || !covers(c.qC[i], a.q[i].C, n * sizeof(P2))) bad = "hit queues";
            else if (sizeof(T) == 4 && !covers(c.qR[i], a.qref[i], n * sizeof(uint32_t))) bad = "hit reference arrays";
            else if (!l.mesh && !covers(c.qK[i], a.qkey[i], n * sizeof(uint2))) bad = "carried RNG keys";
        }
    if (!bad && a.mesh_list && !covers(c.mesh_list, a.mesh_list, 3 * n * sizeof(P4))) bad = "mesh lists";
    if (!bad && a.mesh_mode != 0 && (!a.mesh_list || !covers(c.mesh_count, a.mesh_count, nw * sizeof(uint32_t)) || !need.resume_ok)) bad = "parked-ray counts of a two-launch mesh pass";
    if (!bad && a.redo && !covers(c.redo, a.redo, nw * sizeof(uint32_t))) bad = "redo flags";
    if (!bad && !covers(c.blkstats, a.blk_stats, nw * 4 * sizeof(uint32_t))) bad = "per-wave statistics";
    if (!bad && !covers(c.L, a.L, need.l_entries * sizeof(spira::Pack3<T>))) bad = "per-path radiance";
    if (!bad && !covers(c.stats, a.stats, sizeof(spira::Stats))) bad = "counters";
    if (!bad && a.accum && (!covers(c.accum, a.accum, (uint64_t)a.rc.tile_pixels * sizeof(P4)) || !need.owning_ok)) bad = "pixel-owning pass";
    if (!bad && a.l_private && !need.private_ok) bad = "wave-private radiance blocks";
    if (!bad && !need.table_ok) bad = "pixel table and reach masks in LDS";
    // k_path_own holds as constants what these arguments say: it runs exactly where they say all of it (and the knob is on)
    if (!bad && own_kernel != spira::own_kernel_ok(l)) bad = "the kernel of a full pixel-owning pass";
    if (bad) return fail(SPIRA_E_LIMIT, std::string("internal: a workspace is smaller than the launch needs (") + bad + ")");
    return 0;
}

// Everything but the scene check of a render call's arguments, in the order the errors are documented in.  `rows`: of the tile.
template <class T>
int validate_call(const spira_scene *h, const T *spheres5, const T *materials8, const T *triangles10, const T *camera12, const spira_params *p,
                  const T *out_hdr, const T *out_img, bool progressive, uint32_t sample0, const uint32_t *rng_states, uint32_t *rows) {
    if (!p) return fail(SPIRA_E_INVALID, "params is NULL");
    const uint32_t nt = triangles10 ? p->n_triangles : 0;
    if (h) { if (int rc = check_handle<T>(h)) return rc; }
    else if (int rc = validate_scene<T>(spheres5, materials8, triangles10, p->n_spheres, p->n_materials, nt)) return rc;
    if (int rc = validate_params(camera12, p, h ? h->store.nt : nt, rows)) return rc;
    if (!out_hdr && !out_img) return fail(SPIRA_E_INVALID, "both outputs are NULL");
    const char *msg = nullptr;
    if (int rc = spira::sample_range_check(progressive, sample0, p->spp, &msg)) return fail(rc, msg);
    if (progressive && (p->flags & SPIRA_SEM_MASK) == SPIRA_SEM_HYBRID) return fail(SPIRA_E_UNSUPPORTED, "SPIRA_SEM_HYBRID has no accumulate entry (its image is a mean of tone-mapped samples)");
    if (progressive && (p->flags & SPIRA_SEM_MASK) == SPIRA_SEM_METAL && sample0 > 0 && !rng_states)
        return fail(SPIRA_E_INVALID, "SPIRA_SEM_METAL with sample0 > 0 needs rng_states (the LCG states the previous call left); "
                                     "without them every call would replay the samples of the first");
    return 0;
}

// ---- one enqueue function per kernel organisation.  A call's state, as they all see it:
template <class T> struct Call {
    Ctx &c;
    hipStream_t st;
    const spira_params *p;
    const spira::Plan &plan;
    spira::BounceArgs<T> a{};        // scene, render constants, L, stats: what every organisation's arguments start from
    size_t lds = 0;                  // the scene's share of a workgroup's LDS
    int spec = 0;                    // speculative division of this call (Plan::spec)
    bool progressive = false, profile = false;
    uint32_t sample0 = 0, *d_rng = nullptr;
    uint64_t launches = 0, metal_launches = 0;
    using P4 = spira::Pack4<T>;
    using P2 = spira::Pack2<T>;
    P4 *accum() const { return (P4 *)c.accum.p; }
    spira::Stats *stats() const { return (spira::Stats *)c.stats.p; }
    uint32_t *redo() const { return (uint32_t *)c.redo.p; }
    spira::RayQueue<T> queue(int i) const { return {(P4 *)c.qA[i].p, (P4 *)c.qB[i].p, (P2 *)c.qC[i].p}; }
    dim3 block() const { return dim3(spira::kBlock); }
    int resume() const { return progressive ? (sample0 > 0 ? 3 : 1) : 0; }      // SPIRA_SEM_METAL: bit 0 continue the sums, bit 1 continue the LCG states
};

// render_hybrid_gpu as written (spira_device.h, k_hybrid): the whole image in lock step, max_depth + 1 launches per sample, all on this stream
template <class T>
int enqueue_hybrid(Call<T> &k) {
    Ctx &c = k.c;
    const spira_params *p = k.p;
    const spira::Workspace &w = k.plan.ws;
    const uint32_t P = (uint32_t)k.plan.tile_pixels, hblocks = k.plan.blocks(P);
    HIP_TRY(hipMemsetAsync(c.hyb_flags.p, 0, w.hyb_flags, k.st));
    HIP_TRY(hipMemsetAsync(c.accum.p, 0, w.accum, k.st));
    HIP_TRY(hipMemsetAsync(c.hyb_mat.p, 0, w.hyb_mat, k.st));
    HIP_TRY(hipMemsetAsync(c.hyb_state.p, 0, w.hyb_state, k.st));
    hipLaunchKernelGGL(spira::k_hybrid_init, dim3(hblocks), k.block(), 0, k.st, (uint32_t *)c.rng.p, P, k.a.rc.sA, k.a.rc.sB);
    spira::HybridArgs<T> ha{};
    ha.scene = k.a.scene; ha.rc = k.a.rc; ha.state = (T *)c.hyb_state.p; ha.mat = (uint32_t *)c.hyb_mat.p; ha.rng = (uint32_t *)c.rng.p;
    ha.accum = k.accum(); ha.flags = (uint32_t *)c.hyb_flags.p; ha.stats = k.stats();
    for (uint32_t smp = 1; smp <= p->spp; ++smp)
        for (uint32_t ph = 0; ph <= p->max_depth; ++ph) {
            ha.sample = smp; ha.phase = ph;
            if (int rc = launch_lds(spira::k_hybrid<T>, dim3(hblocks), k.block(), k.lds, k.st, ha)) return rc;
        }
    k.launches += 1 + (uint64_t)p->spp * (p->max_depth + 1);
    return 0;
}

// the .metal estimator in wavefront form: every wave owns a block of pixels and walks sample after sample on it
template <class T>
int enqueue_metal_wavefront(Call<T> &k) {
    Ctx &c = k.c;
    const spira::Plan &plan = k.plan;
    const dim3 grid(plan.G_metal);
    spira::MetalArgs<T> ma{};
    ma.scene = k.a.scene; ma.rc = k.a.rc;
    ma.ppw = plan.ppw;
    for (int i = 0; i < 2; ++i) { ma.q[i] = k.queue(i); ma.qx[i] = (uint2 *)c.qX[i].p; }
    if (!k.d_rng) k.d_rng = (uint32_t *)c.rng.p;
    ma.L = k.a.L; ma.accum = k.accum(); ma.rng_states = k.d_rng; ma.blk_stats = (uint32_t *)c.blkstats.p;
    ma.resume = k.resume();
    if (int rc = profile_events(c, c.ev_used + 2)) return rc;      // (a later slab's bracket comes after slab 0's)
    HIP_TRY(hipEventRecord(c.ev_pool[c.ev_used++], k.st));
    ma.stats = k.stats(); ma.redo = nullptr; ma.redo_only = 0;
    if (k.spec) {                          // speculative division as in k_path
        ma.redo = k.redo();
        ma.redo_only = k.spec == 2 ? 2 : 0;
        if (int rc = launch_lds(spira::k_path_metal<T, 2, true>, grid, k.block(), k.lds, k.st, ma)) return rc;
        ma.redo_only = 1;
        ++k.launches;
    }
    if (int rc = plan.R == 2 ? launch_lds(spira::k_path_metal<T, 2, false>, grid, k.block(), k.lds, k.st, ma)
                             : launch_lds(spira::k_path_metal<T, 1, false>, grid, k.block(), k.lds, k.st, ma)) return rc;
    HIP_TRY(hipEventRecord(c.ev_pool[c.ev_used++], k.st));
    hipLaunchKernelGGL(spira::k_fold_stats, dim3(1), dim3(64), 0, k.st, (const uint32_t *)c.blkstats.p, plan.G_metal * plan.wpb, k.stats());
    k.launches += 2;
    k.metal_launches = 1;
    return 0;
}

// SPIRA_SEM_METAL in one launch: every lane owns a pixel and walks its spp samples (the LCG state runs through them); with speculative
// division (fresh renders of scenes of ordinary scale) the exact launch behind renders reported waves again
template <class T>
int enqueue_metal(Call<T> &k) {
    const dim3 grid(k.plan.blocks(k.plan.tile_pixels));
    k.a.pass = 0; k.a.n_first = (uint32_t)k.plan.tile_pixels;
    if (k.spec) {
        if (int rc = launch_lds(spira::k_variant_metal<T, true>, grid, k.block(), k.lds, k.st, k.a, k.accum(), k.d_rng, k.resume(), k.redo(), k.spec == 2 ? 2 : 0)) return rc;
        if (int rc = launch_lds(spira::k_variant_metal<T, false>, grid, k.block(), k.lds, k.st, k.a, k.accum(), k.d_rng, k.resume(), k.redo(), 1)) return rc;
    } else if (int rc = launch_lds(spira::k_variant_metal<T, false>, grid, k.block(), k.lds, k.st, k.a, k.accum(), k.d_rng, k.resume(), (uint32_t *)nullptr, 0))
        return rc;
    k.launches += k.spec ? 2 : 1;
    return 0;
}

// ---- organisations that render `slots` samples of every pixel per pass: the launches of pass k.a.pass (*stat_rows: rows of per-wave statistics k_resolve folds)
template <class T>
int enqueue_cpu_pass(Call<T> &k) {
    const dim3 grid(k.plan.blocks(k.a.n_first));
    if (k.spec) {                          // speculative division as in k_path / k_variant_metal
        if (int rc = launch_lds(spira::k_variant_cpu<T, true>, grid, k.block(), k.lds, k.st, k.a, k.redo(), k.spec == 2 ? 2 : 0)) return rc;
        if (int rc = launch_lds(spira::k_variant_cpu<T, false>, grid, k.block(), k.lds, k.st, k.a, k.redo(), 1)) return rc;
    } else if (int rc = launch_lds(spira::k_variant_cpu<T, false>, grid, k.block(), k.lds, k.st, k.a, (uint32_t *)nullptr, 0))
        return rc;
    k.launches += k.spec ? 2 : 1;
    return 0;
}

template <class T>
int enqueue_mega_pass(Call<T> &k) {
    const dim3 grid(k.plan.blocks(k.a.n_first));
    const bool ext = (k.p->flags & (SPIRA_EXT_DIELECTRIC | SPIRA_EXT_SPECTRAL)) != 0;
    int rc;
    if (k.a.scene.n_bvh_tris) rc = ext ? launch_lds(spira::k_mega<T, true, true>, grid, k.block(), k.lds, k.st, k.a) : launch_lds(spira::k_mega<T, true, false>, grid, k.block(), k.lds, k.st, k.a);
    else rc = ext ? launch_lds(spira::k_mega<T, false, true>, grid, k.block(), k.lds, k.st, k.a) : launch_lds(spira::k_mega<T, false, false>, grid, k.block(), k.lds, k.st, k.a);
    ++k.launches;
    return rc;
}

// k_path, one launch: every wave walks all max_depth stages on its own region of the hit queues (mesh scenes: a parking launch + a fat-wave launch)
template <class T>
int enqueue_path_pass(Call<T> &k, uint32_t *stat_rows) {
    using P4 = typename Call<T>::P4;
    Ctx &c = k.c;
    const spira::Plan &plan = k.plan;
    const spira::Knobs &kn = plan.in.k;
    spira::PathArgs<T> pa{};
    pa.scene = k.a.scene; pa.rc = k.a.rc; pa.L = k.a.L; pa.pass = k.a.pass; pa.n_first = k.a.n_first;
    pa.dense_pct = kn.dense_pct;
    pa.mesh_list = plan.defer_mesh ? (P4 *)c.mesh_list.p : nullptr;
    const spira::Geometry g = plan.geometry(pa.n_first);
    const uint32_t G = g.G;
    pa.cap = g.cap;
    *stat_rows = G * plan.wpb;
    for (int i = 0; i < 2; ++i) {
        pa.q[i] = k.queue(i);
        pa.qref[i] = (uint32_t *)c.qR[i].p;
        pa.qkey[i] = (uint2 *)c.qK[i].p;
    }
    pa.blk_stats = (uint32_t *)c.blkstats.p;
    pa.stats = k.stats();
    if (k.spec) pa.redo = k.redo();      // (sized by the plan whenever SPIRA_SPEC_DIV != 0)
    pa.mesh_mode = 0; pa.mesh_count = nullptr; pa.resume_k = 1; pa.resume_nw = 0;
    pa.mesh_min_batch = kn.mesh_min_batch;
    pa.refill_free = kn.mesh_refill;
    size_t lds_a = k.lds + (size_t)plan.wpb * plan.sub * sizeof(P4) + 128;             // + one work list per wave + the camera
    // ... + one packet per sphere: what a sphere test of a CAMERA ray does not depend on the ray for (closest_hit_local, CAM) — where the block has the room
    pa.cam_consts = (kn.cam_consts && pa.scene.n_spheres && lds_a + (size_t)pa.scene.n_spheres * sizeof(P4) <= (size_t)160 * 1024) ? 1u : 0u;
    if (pa.cam_consts) lds_a += (size_t)pa.scene.n_spheres * sizeof(P4);
    size_t own_lds = 0;
    if (plan.two_pass) {
        pa.mesh_mode = 1; pa.mesh_count = (uint32_t *)c.mesh_count.p;
        pa.resume_nw = G * plan.wpb; pa.resume_k = plan.fat_k(pa.resume_nw);
    }
    if (plan.fused) {
        pa.accum = k.accum(); pa.k_eff = plan.k_eff(pa.pass); pa.fd_keff = spira::fastdiv_make(pa.k_eff);
        pa.accum_first = (pa.pass == 0 && !k.progressive) ? 1u : 0u;
        pa.l_private = plan.l_private ? 1u : 0u;
        pa.sky_runs = plan.sky_runs ? 1u : 0u;
        // ... + the waves' pixel tables and run masks behind everything else (spira_plan.h, own_lds_bytes): these launches alone, and where the block has the room
        if ((plan.pixel_table || plan.reach_masks) && lds_a + spira::own_lds_bytes(plan.wpb) <= (size_t)160 * 1024) {
            own_lds = (size_t)spira::own_lds_bytes(plan.wpb);
            lds_a += own_lds;
            pa.pixel_table = plan.pixel_table ? 1u : 0u; pa.reach_masks = plan.reach_masks ? 1u : 0u;
        }
    }
    // a full pass of 64 slots with everything above granted runs k_path_own (spira_plan.h, own_kernel_ok): pass by pass, from the arguments as they stand
    const bool own_kernel = spira::own_kernel_ok(path_launch_of<T>(pa, G, own_lds, plan.R, plan.own_kernel));
    if (int rc = verify_path_args<T>(c, pa, G, own_lds, plan.R, plan.own_kernel, own_kernel)) return rc;     // every pointer against the capacity of its buffer, for THIS grid
    HIP_TRY(hipEventRecord(c.ev_pool[c.ev_used++], k.st));
    if (int rc = launch_path<T>((int)plan.R, dim3(G), lds_a, k.st, pa, k.spec, own_kernel)) return rc;
    if (own_kernel) ++c.own_passes;      // (a kernel that was refused its LDS did not run: nothing that consumes its output is enqueued)
    k.launches += k.spec ? 2 : 1;      // the speculative launch and its exact follow-up
    if (pa.mesh_mode == 1) {           // second launch: nw / k fat waves
        if (c.ev_mid.size() <= c.ev_mid_used) {
            hipEvent_t e;
            HIP_TRY(hipEventCreate(&e));
            c.ev_mid.push_back(e); c.ev_mid_end.push_back(0);
        }
        HIP_TRY(hipEventRecord(c.ev_mid[c.ev_mid_used], k.st));
        c.ev_mid_end[c.ev_mid_used++] = c.ev_used;      // (the closing event of this pass's bracket is recorded next)
        spira::PathArgs<T> pb = pa;
        pb.mesh_mode = 2; pb.n_first = 0;
        const uint32_t nwb = pa.resume_nw / pa.resume_k;
        if (int rc = launch_path_resume_entry<T>((int)plan.R, dim3((nwb + plan.wpb - 1) / plan.wpb), lds_a, k.st, pb)) return rc;
        ++k.launches;
    }
    HIP_TRY(hipEventRecord(c.ev_pool[c.ev_used++], k.st));
    return 0;
}

// round-1 organisation: one launch per bounce; bounce b writes queue b & 1 and reads the other
template <class T>
int enqueue_bounce_pass(Call<T> &k, uint32_t *stat_rows) {
    using P4 = typename Call<T>::P4;
    Ctx &c = k.c;
    const spira::Plan &plan = k.plan;
    const spira::Geometry g = plan.geometry(k.a.n_first);
    const size_t nw = (size_t)g.G * plan.wpb;
    k.a.cap = g.cap;
    *stat_rows = k.p->max_depth * g.G * plan.wpb;
    for (uint32_t b = 0; b < k.p->max_depth; ++b) {
        k.a.bounce = b;
        k.a.qout = k.queue(b & 1);
        k.a.qin = k.queue((b & 1) ^ 1);
        k.a.cnt_in = (const uint32_t *)c.counts.p + (size_t)b * nw;
        k.a.cnt_out = (uint32_t *)c.counts.p + (size_t)(b + 1) * nw;
        k.a.blk_stats = (uint32_t *)c.blkstats.p + (size_t)b * nw * 4;
        if (k.profile) HIP_TRY(hipEventRecord(c.ev_pool[c.ev_used++], k.st));
        const size_t lds_b = k.lds + (size_t)plan.wpb * plan.sub * sizeof(P4);   // + one work list per wave (one slot per ray of a sub-chunk)
        if (int rc = b == 0 ? launch_bounce<T, true>((int)plan.R, dim3(g.G), lds_b, k.st, k.a) : launch_bounce<T, false>((int)plan.R, dim3(g.G), lds_b, k.st, k.a)) return rc;
        if (k.profile) HIP_TRY(hipEventRecord(c.ev_pool[c.ev_used++], k.st));
        ++k.launches;
    }
    return 0;
}

// accum[pixel] += the pass's samples of L, in sample order (not after pixel-owning passes: their waves resolved their pixels and added their counters)
template <class T>
void enqueue_resolve(Call<T> &k, uint32_t stat_rows) {
    const spira::Plan &plan = k.plan;
    hipLaunchKernelGGL((spira::k_resolve<T>), dim3(plan.blocks(plan.tile_pixels)), k.block(), 0, k.st, k.accum(), (const spira::Pack3<T> *)k.c.L.p,
                       (uint32_t)plan.tile_pixels, plan.k_eff(k.a.pass), (k.a.pass == 0 && !k.progressive) ? 1 : 0,
                       stat_rows ? (const uint32_t *)k.c.blkstats.p : (const uint32_t *)nullptr, stat_rows, k.stats());
    ++k.launches;
}

template <class T>
void enqueue_finalize(Call<T> &k, T *d_hdr, T *d_img) {
    using P4 = typename Call<T>::P4;
    const spira::Plan &plan = k.plan;
    const dim3 grid(plan.blocks(plan.tile_pixels));
    if (k.progressive)      // hand the running sums back untouched (x / 1 is exact)
        hipLaunchKernelGGL((spira::k_finalize<T>), grid, k.block(), 0, k.st, (const P4 *)k.accum(), (uint32_t)plan.tile_pixels, 1u, (uint32_t)SPIRA_POST_NONE, d_hdr, (T *)nullptr);
    else
        hipLaunchKernelGGL((spira::k_finalize<T>), grid, k.block(), 0, k.st, (const P4 *)k.accum(), (uint32_t)plan.tile_pixels, k.p->spp,
                           (k.p->flags & SPIRA_SEM_MASK) == SPIRA_SEM_HYBRID ? (uint32_t)SPIRA_POST_NONE : (k.p->flags & SPIRA_POST_MASK), d_hdr, d_img);      // (HYBRID: the sum is already tone-mapped, K7 per sample)
    ++k.launches;
}

// What render and adaptive render share of a k_path call between the workspaces and the first launch: the scene, the constants and what
// every organisation's arguments start from (k.p: the parameters the plan was made from).
template <class T>
int prepare_path_call(Call<T> &k, const spira_scene *h, const T *spheres5, const T *materials8, const T *triangles10, const T *camera12, uint32_t rows, bool reuse_scene) {
    Ctx &c = k.c;
    if (int rc = acquire_scene<T>(c, k.st, h, spheres5, materials8, triangles10, k.p, k.a.scene, reuse_scene)) return rc;
    if (int rc = attach_spd<T>(c, k.st, k.p, k.a.scene)) return rc;
    k.spec = k.plan.spec((h ? h->store.moderate : c.scene.moderate) && spira::camera_scale_moderate<T>(camera12));
    fill_const<T>(k.a.rc, camera12, k.p, rows, k.plan.slots);
    if (!fastdiv_selfcheck(k.a.rc.tile_pixels, (uint32_t)k.plan.batch) || !fastdiv_selfcheck(k.a.rc.width, k.a.rc.tile_pixels) ||
        !fastdiv_selfcheck(k.a.rc.stripe_h ? k.a.rc.stripe_h : 1, rows))
        return fail(SPIRA_E_LIMIT, "internal: fast division self-check failed");
    k.a.L = (spira::Pack3<T> *)c.L.p;
    k.a.stats = k.stats();
    k.lds = spira::scene_lds_bytes<T>(k.a.scene.n_spheres, k.a.scene.n_materials, k.a.scene.n_triangles);
    return 0;
}

// Where the kernels write a call's two frames: the caller's device memory, or the two halves of out_tmp, which copy() then hands to the host caller.
template <class T> struct FrameOut {
    T *hdr, *img;
    FrameOut(const Session &s, T *out_hdr, T *out_img, uint64_t tile_pixels) : hdr(out_hdr), img(out_img) {
        if (!s.host_out) return;
        hdr = out_hdr ? (T *)s.cp->out_tmp.p : nullptr;
        img = out_img ? (T *)((char *)s.cp->out_tmp.p + 3 * tile_pixels * sizeof(T)) : nullptr;
    }
    int copy(const Session &s, T *out_hdr, T *out_img, uint64_t tile_pixels) const {
        if (!s.host_out) return 0;
        void *const dst[2] = {out_hdr, out_img};
        const void *const src[2] = {hdr, img};
        return copy_out(*s.cp, s.st, dst, src, 3 * tile_pixels * sizeof(T));
    }
};

// The bracket spira_get_counters reads: device counters and event brackets start from nothing (cont, a later slab: they go on from slab 0's) ...
int begin_counters(Session &s, bool cont) {
    Ctx &c = *s.cp;
    if (cont) return 0;
    c.ev_used = 0;
    c.ev_mid_used = 0;
    c.own_passes = 0;
    HIP_TRY(hipMemsetAsync(c.stats.p, 0, sizeof(spira::Stats), s.st));
    HIP_TRY(hipEventRecord(c.ev_start, s.st));
    return 0;
}
// ... and after the call's last kernel the device counters are read back and the host's share (`delta`) becomes, or with cont adds to, the context's
int end_counters(Session &s, const spira_counters &delta, bool cont) {
    Ctx &c = *s.cp;
    HIP_TRY(hipEventRecord(c.ev_stop, s.st));
    HIP_TRY(hipMemcpyAsync(c.h_stats, c.stats.p, sizeof(spira::Stats), hipMemcpyDeviceToHost, s.st));
    if (!cont) c.last = spira_counters{};
    c.last.samples += delta.samples;
    c.last.passes += delta.passes;
    c.last.launches += delta.launches;
    c.last.bounce_launches += delta.bounce_launches;
    c.last_own_passes = c.own_passes;
    c.last_valid = true;
    c.last_pending = true;
    c.last_stream = s.st;
    return 0;
}

}  // namespace
// Validation -> session -> plan -> workspaces -> scene -> prologue (events, a progressive call's running sums) -> the organisation's launches -> epilogue.
// (The kernels of a translation unit come out in the order in which their launches are first named from here, enqueue function by enqueue function:
// keep that order, and every launch but k_load_accum's inside one of them, and the code object does not change when this function does.)
template <class T>
int spira_tu::Impl<T>::render(const spira_scene *h, const T *spheres5, const T *materials8, const T *triangles10, const T *camera12, const spira_params *p,
                              T *out_hdr, T *out_img, bool out_on_device, void *user_stream,
                              bool progressive, uint32_t sample0, uint32_t *rng_states, const SlabCtl *slab) {
    // progressive: out_hdr is the caller's running SUM (in/out), samples [sample0, sample0 + spp) are added to it
    using spira::Org;
    using P4 = spira::Pack4<T>;
    uint32_t rows = 0;
    const bool cont = slab && slab->index > 0;      // a later slab of a host-output frame: continues slab 0's call (SlabCtl)
    Lap lap("render");
    if (slab) rows = p->rows;            // (render_host_slabs validated the frame its slabs are cut from)
    else if (int rc = validate_call<T>(h, spheres5, materials8, triangles10, camera12, p, out_hdr, out_img, progressive, sample0, rng_states, &rows)) return rc;
    lap("validate");
    Session s;
    if (int rc = Session::open(s, out_on_device, user_stream)) return rc;
    Ctx &c = *s.cp;
    const hipStream_t st = s.st;
    lap("context");

    spira::Plan plan;
    const char *msg = nullptr;
    const uint32_t nt_scene = h ? h->store.nt : (triangles10 ? p->n_triangles : 0);
    if (int rc = spira::make_plan(plan_input<T>(c, p, rows, nt_scene, progressive, progressive && rng_states, out_on_device), plan, &msg)) return fail(rc, msg);
    if (int rc = ensure_workspaces(c, plan.ws)) return rc;
    lap("workspaces");

    Call<T> k{c, st, p, plan};
    const uint64_t tile_pixels = plan.tile_pixels;
    if (int rc = prepare_path_call<T>(k, h, spheres5, materials8, triangles10, camera12, rows, cont)) return rc;
    lap("scene");
    k.progressive = progressive; k.sample0 = sample0;
    // k_path launches are always bracketed (2 events per pass); the per-bounce ones on request
    k.profile = plan.org == Org::Path || (plan.org == Org::Bounce && (p->flags & SPIRA_FLAG_PROFILE) != 0);

    const FrameOut<T> out(s, out_hdr, out_img, tile_pixels);
    T *const d_hdr = out.hdr, *const d_img = out.img;
    if (k.profile) {
        const size_t n_prof = (size_t)plan.n_pass * (plan.org == Org::Path ? 1 : p->max_depth) * 2;
        if (int rc = profile_events(c, (cont ? c.ev_used : 0) + n_prof)) return rc;
    }
    if (int rc = begin_counters(s, cont)) return rc;      // (a later slab adds its brackets and device counters to slab 0's)

    // progressive accumulation: the caller's running sums (and, METAL, LCG states) seed the accumulator
    k.a.rc.sample0 = progressive ? sample0 : 0;
    if (progressive) {
        if (!out_on_device) HIP_TRY(hipMemcpyAsync(d_hdr, out_hdr, 3 * tile_pixels * sizeof(T), hipMemcpyHostToDevice, st));
        hipLaunchKernelGGL((spira::k_load_accum<T>), dim3(plan.blocks(tile_pixels)), k.block(), 0, st, k.accum(), (const T *)d_hdr, (uint32_t)tile_pixels);
        ++k.launches;
        k.d_rng = (rng_states && !out_on_device) ? (uint32_t *)c.rng.p : rng_states;
        if (rng_states && !out_on_device && sample0 > 0) HIP_TRY(hipMemcpyAsync(k.d_rng, rng_states, tile_pixels * sizeof(uint32_t), hipMemcpyHostToDevice, st));
    }

    int rc = 0;
    switch (plan.org) {
    case Org::Black: if (!progressive) HIP_TRY(hipMemsetAsync(c.accum.p, 0, tile_pixels * sizeof(P4), st)); break;   // depth <= 0 -> Vec3(0,0,0), :330
    case Org::Hybrid: rc = enqueue_hybrid(k); break;
    case Org::MetalWavefront: rc = enqueue_metal_wavefront(k); break;
    case Org::Metal: rc = enqueue_metal(k); break;
    default:                             // `slots` samples of every pixel per pass, then the pass's resolve
        for (uint32_t pass = 0; pass < plan.n_pass && !rc; ++pass) {
            uint32_t stat_rows = 0;
            k.a.pass = pass;
            k.a.n_first = plan.n_first(pass);
            rc = plan.org == Org::Cpu ? enqueue_cpu_pass(k) : plan.org == Org::Mega ? enqueue_mega_pass(k) :
                 plan.org == Org::Path ? enqueue_path_pass(k, &stat_rows) : enqueue_bounce_pass(k, &stat_rows);
            if (!rc && !plan.fused) enqueue_resolve(k, stat_rows);
        }
    }
    if (rc) return rc;
    enqueue_finalize(k, d_hdr, d_img);
    if (progressive && rng_states && !out_on_device)
        HIP_TRY(hipMemcpyAsync(rng_states, k.d_rng, tile_pixels * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    const bool bounce_kernels = plan.org == Org::Path || plan.org == Org::Bounce;
    spira_counters delta{};
    delta.samples = (uint64_t)p->spp * tile_pixels;
    delta.passes = p->max_depth ? plan.n_pass : 0;
    delta.launches = k.launches;
    delta.bounce_launches = k.metal_launches ? k.metal_launches : !bounce_kernels ? 0 : (uint64_t)plan.n_pass * (plan.org == Org::Path ? 1 : p->max_depth);
    if (int rc2 = end_counters(s, delta, cont)) return rc2;
    lap("enqueue");

    if (int rc2 = out.copy(s, out_hdr, out_img, tile_pixels)) return rc2;
    rc = s.close();
    lap("copy_out+sync");
    return rc;
}
namespace {

#ifdef SPIRA_TU_MAIN
// A large frame for a host-pointer caller, rendered as row slabs: slab k's planes go device -> pinned staging on a second stream while slab k + 1
// renders, and the host threads of StagedCopy move them on into the caller's memory.  The copy of a 1080p frame (Float64 HDR: 49.8 MB, 5 ms into
// pageable memory — as long as rendering it) then hides behind the kernels but for the last slab's share.  The RNG is keyed by the global pixel, so
// the slabs are, bit for bit, the rows of the frame rendered whole (tests/test_gpu_runtime.py); the counters of the call add up over its slabs.
// *done = false: the frame is not of that kind (small, striped, progressive, ...) and nothing was touched — the caller takes the plain path.
template <class T>
int render_host_slabs(const spira_scene *h, const T *spheres5, const T *materials8, const T *triangles10, const T *camera12, const spira_params *p,
                      T *out_hdr, T *out_img, bool *done) {
    *done = false;
    const uint32_t S_env = env_u32("SPIRA_HOST_SLABS", 0xFFFFFFFFu);                // (unset: chosen below; 0 or 1: never)
    if (!p || S_env < 2) return 0;
    if ((p->flags & SPIRA_SEM_MASK) == SPIRA_SEM_HYBRID) return 0;                   // whole images only
    if (p->rows != 0 && p->stripe_count > 1) return 0;                               // an interleaved tile (its rows are not consecutive image rows)
    const uint64_t W = p->width, rows = p->rows ? p->rows : p->height, row0 = p->rows ? p->row0 : 0;
    if (rows * W > 0x7FFFFFFFull) return 0;                                          // (the plain path reports what is wrong)
    const uint64_t plane3 = 3 * rows * W * sizeof(T), total = plane3 * ((out_hdr ? 1 : 0) + (out_img ? 1 : 0));
    // a slab costs ~0.1 ms of device time (its own launches and their tails) and hides its share of the copy: two for a 1080p Float32 image (24.9 MB: 4.7 -> 4.0 ms
    // end to end), four from 32 MB on (1080p Float64 HDR, 49.8 MB: 7.3 -> 6.6 ms into touched memory; profiles/experiments/r04_host_slabs_probe.py)
    const uint32_t S = S_env != 0xFFFFFFFFu ? std::min<uint32_t>(S_env, 16) : (total < ((uint64_t)32 << 20) ? 2u : 4u);
    if (total < ((uint64_t)8 << 20) || total > ((uint64_t)512 << 20) || rows < 16 * S || rows * W * p->spp < ((uint64_t)16 << 20)) return 0;
    // a mesh pass ends with the tail of its fat waves, and four small passes have four of them: configs[4] 6.2 -> 7.8 ms of device time, more than the copy hides
    if (h) { if (int rc = check_handle<T>(h)) return rc; }                           // (the plain path's first check too)
    if ((h ? h->store.nt : (triangles10 ? p->n_triangles : 0)) > SPIRA_LDS_TRIANGLES) return 0;
    // the frame will be rendered as slabs: the whole call is validated here, once, before anything is sized or allocated (its slabs skip it: SlabCtl)
    uint32_t rows_checked = 0;
    if (int rc = validate_call<T>(h, spheres5, materials8, triangles10, camera12, p, out_hdr, out_img, false, 0, nullptr, &rows_checked)) return rc;
    Session ss;                          // (on the context's stream; out_tmp may still be read by the previous call.  The ending is this function's own: two streams)
    if (int rc = Session::open(ss, false, nullptr)) return rc;
    Ctx &c = *ss.cp;
    if (!stage_reserve(c, total)) return 0;
    if (!c.copy_stream) HIP_TRY(hipStreamCreateWithFlags(&c.copy_stream, hipStreamNonBlocking));
    if (!c.ev_slab) HIP_TRY(hipEventCreateWithFlags(&c.ev_slab, hipEventDisableTiming));
    if (int rc = c.out_tmp.ensure(2 * plane3)) return rc;
    *done = true;
    Lap lap("host slabs");
    StagedCopy sc(c);
    int rc_all = 0;
    for (uint32_t s = 0, r0 = 0; s < S && !rc_all; ++s) {
        const uint32_t rs = (uint32_t)(rows / S + (s < rows % S ? 1u : 0u));
        spira_params ps = *p;
        ps.row0 = (uint32_t)row0 + r0; ps.rows = rs; ps.stripe_h = 0; ps.stripe_count = 0; ps.stripe_rank = 0;
        // the slab's planar block [3][rs][W] sits at element 3 * W * r0 of its output's device frame
        T *d_hdr = out_hdr ? (T *)c.out_tmp.p + (size_t)3 * W * r0 : nullptr;
        T *d_img = out_img ? (T *)((char *)c.out_tmp.p + plane3) + (size_t)3 * W * r0 : nullptr;
        const SlabCtl ctl{s, S};
        rc_all = spira_tu::Impl<T>::render(h, spheres5, materials8, triangles10, camera12, &ps, d_hdr, d_img, true, (void *)c.stream, false, 0, nullptr, &ctl);
        if (rc_all) break;
        hipError_t e = hipEventRecord(c.ev_slab, c.stream);
        if (e == hipSuccess) e = hipStreamWaitEvent(c.copy_stream, c.ev_slab, 0);
        T *const dev[2] = {d_hdr, d_img};
        T *const host[2] = {out_hdr, out_img};
        for (int k = 0; k < 2; ++k)
            for (int pl = 0; host[k] && pl < 3 && e == hipSuccess; ++pl)
                e = sc.stage(c.copy_stream, host[k] + ((size_t)pl * rows + r0) * W, dev[k] + (size_t)pl * rs * W, (size_t)rs * W * sizeof(T));
        if (e != hipSuccess) rc_all = fail(SPIRA_E_HIP, std::string("host-output slabs: ") + hipGetErrorString(e));
        r0 += rs;
    }
    if (rc_all) {                        // drain what was enqueued; nothing of the frame is promised
        (void)hipStreamSynchronize(c.stream); (void)hipStreamSynchronize(c.copy_stream);
        return rc_all;
    }
    lap("enqueue");
    const hipError_t moved = sc.move();
    lap("movers");
    HIP_TRY(hipStreamSynchronize(c.copy_stream));
    HIP_TRY(hipStreamSynchronize(c.stream));
    if (moved != hipSuccess) return fail(SPIRA_E_HIP, std::string("host-output slabs: ") + hipGetErrorString(moved));
    return 0;
}
#endif

template <class T>
int render_entry(const spira_scene *h, const T *spheres5, const T *materials8, const T *triangles10, const T *camera12, const spira_params *p,
                 T *out_hdr, T *out_img, bool out_on_device, void *user_stream, bool progressive = false, uint32_t sample0 = 0, uint32_t *rng_states = nullptr) {
#ifdef SPIRA_TU_MAIN
    if (!out_on_device && !progressive) {
        bool done = false;
        const int rc = render_host_slabs<T>(h, spheres5, materials8, triangles10, camera12, p, out_hdr, out_img, &done);
        if (done || rc) return rc;
    }
#endif
    return spira_tu::Impl<T>::render(h, spheres5, materials8, triangles10, camera12, p, out_hdr, out_img, out_on_device, user_stream, progressive, sample0, rng_states, nullptr);
}

// ---- adaptive sampling (spira_render_adaptive_*; spira_adaptive.h).  Round 0 is a plain render of min_spp samples on the slot-major plan (PlanIn::adaptive)
// whose resolve launches are k_resolve_adaptive; every later round is one k_refine launch over the active list, sized by the list length the host reads
// back — ONE stream synchronisation per round, the device-output entries included; then k_finalize_adaptive.
template <class T, bool BVH>
int enqueue_refine(hipStream_t st, const spira::AdaptiveRound &g, size_t lds, const spira::RefineArgs<T> &ra) {
    // the launch against what the kernel assumes of it: its LDS block holds ppw * chunk entries per wave, a lane per owned pixel, a wave for every list entry
    if (g.ppw == 0 || g.chunk == 0 || (uint64_t)g.ppw * g.chunk > spira::kAdaptiveItems || g.ppw > 64 || g.waves * g.ppw < ra.n_active ||
        (uint64_t)g.grid * spira::kAdaptiveWpb < g.waves || spira::kAdaptiveWpb != spira::kBlock / 64)
        return fail(SPIRA_E_LIMIT, "internal: a refinement launch does not cover its list");
    return launch_lds(spira::k_refine<T, BVH>, dim3(g.grid), dim3(spira::kBlock), lds, st, ra);
}

}  // namespace
template <class T>
int spira_tu::Impl<T>::render_adaptive(const spira_scene *h, const T *spheres5, const T *materials8, const T *triangles10, const T *camera12, const spira_params *p,
                                       const spira_adaptive *ad, T *out_hdr, T *out_img, uint32_t *out_spp, T *out_q, bool out_on_device, void *user_stream) {
    using spira::Org;
    using P4 = spira::Pack4<T>;
    uint32_t rows = 0;
    if (!ad) return fail(SPIRA_E_INVALID, "adaptive is NULL");
    // (any one of the four outputs will do: validate_call asks for one of its two)
    const T *some_out = out_hdr ? out_hdr : out_img ? out_img : (out_spp || out_q) ? camera12 : nullptr;
    if (int rc = validate_call<T>(h, spheres5, materials8, triangles10, camera12, p, some_out, (const T *)nullptr, false, 0, nullptr, &rows)) return rc;
    if ((p->flags & SPIRA_SEM_MASK) != SPIRA_SEM_A) return fail(SPIRA_E_UNSUPPORTED, "adaptive sampling is built for SPIRA_SEM_A only");
    if ((p->flags & SPIRA_KERNEL_MASK) != SPIRA_KERNEL_DEFAULT) return fail(SPIRA_E_UNSUPPORTED, "adaptive sampling has one kernel organisation: SPIRA_KERNEL_DEFAULT");
    if (p->flags & (SPIRA_EXT_DIELECTRIC | SPIRA_EXT_SPECTRAL)) return fail(SPIRA_E_UNSUPPORTED, "SPIRA_EXT_* extensions are not built into the adaptive kernels");
    const char *msg = nullptr;
    spira::AdaptiveIn ain;
    ain.min_spp = ad->min_spp; ain.batch_spp = ad->batch_spp; ain.spp = p->spp; ain.tolerance = ad->tolerance; ain.floor = ad->floor;
    ain.tile_pixels = (uint64_t)rows * p->width; ain.prec = sizeof(T); ain.pack3 = sizeof(spira::Pack3<T>);
    if (int rc = spira::adaptive_check(ain.min_spp, ain.batch_spp, ain.spp, ain.tolerance, ain.floor, &msg)) return fail(rc, msg);
    if (p->max_depth < 1) return fail(SPIRA_E_INVALID, "max_depth must be >= 1");
    Session s;
    if (int rc = Session::open(s, out_on_device, user_stream)) return rc;
    Ctx &c = *s.cp;
    const hipStream_t st = s.st;

    ain.num_cus = (uint32_t)c.num_cus;
    spira::AdaptivePlan ap;
    if (int rc = spira::make_adaptive_plan(ain, ap, &msg)) return fail(rc, msg);
    spira_params p0 = *p;                // round 0: min_spp samples of every pixel
    p0.spp = ad->min_spp;
    spira::Plan plan;
    const uint32_t nt_scene = h ? h->store.nt : (triangles10 ? p->n_triangles : 0);
    spira::PlanIn pin = plan_input<T>(c, &p0, rows, nt_scene, false, false, out_on_device);
    pin.adaptive = true;
    if (int rc = spira::make_plan(pin, plan, &msg)) return fail(rc, msg);
    if (plan.org != Org::Path || plan.fused) return fail(SPIRA_E_LIMIT, "internal: round 0 of an adaptive render is not a slot-major k_path plan");
    if (int rc = ensure_workspaces(c, plan.ws)) return rc;
    if (int rc = c.ad_q.ensure(ap.q_bytes)) return rc;
    if (int rc = c.ad_n.ensure(ap.n_bytes)) return rc;
    for (int i = 0; i < 2; ++i) if (int rc = c.ad_list[i].ensure(ap.list_bytes)) return rc;
    if (int rc = c.ad_count.ensure(ap.count_bytes)) return rc;
    if (!c.h_ad_count) HIP_TRY(hipHostMalloc((void **)&c.h_ad_count, sizeof(uint32_t), hipHostMallocDefault));

    Call<T> k{c, st, &p0, plan};
    const uint64_t tile_pixels = plan.tile_pixels;
    if (int rc = prepare_path_call<T>(k, h, spheres5, materials8, triangles10, camera12, rows, false)) return rc;
    k.profile = true;
    const FrameOut<T> out(s, out_hdr, out_img, tile_pixels);
    if (int rc = profile_events(c, (size_t)plan.n_pass * 2)) return rc;
    HIP_TRY(hipMemsetAsync(c.ad_count.p, 0, ap.count_bytes, st));
    if (int rc = begin_counters(s, false)) return rc;

    spira::AdaptiveArgs<T> aa{};
    aa.accum = k.accum(); aa.Q = (T *)c.ad_q.p; aa.npix = (uint32_t *)c.ad_n.p;
    aa.tol = (T)ad->tolerance; aa.floor = (T)ad->floor; aa.cap = p->spp;
    uint32_t *const lists[2] = {(uint32_t *)c.ad_list[0].p, (uint32_t *)c.ad_list[1].p};
    uint32_t *const counts = (uint32_t *)c.ad_count.p;
    for (uint32_t pass = 0; pass < plan.n_pass; ++pass) {
        uint32_t stat_rows = 0;
        k.a.pass = pass;
        k.a.n_first = plan.n_first(pass);
        if (int rc = enqueue_path_pass(k, &stat_rows)) return rc;
        hipLaunchKernelGGL((spira::k_resolve_adaptive<T>), dim3(plan.blocks(tile_pixels)), k.block(), 0, st, (const spira::Pack3<T> *)c.L.p, (uint32_t)tile_pixels,
                           plan.k_eff(pass), pass == 0 ? 1 : 0, pass + 1 == plan.n_pass ? 1 : 0, ad->min_spp,
                           stat_rows ? (const uint32_t *)c.blkstats.p : (const uint32_t *)nullptr, stat_rows, k.stats(), aa, lists[0], counts);
        ++k.launches;
    }
    // rounds >= 1: the list the previous round left, until it is empty or every pixel on it has reached the cap
    uint64_t samples = tile_pixels * ad->min_spp, rounds = 0;
    int cur = 0;
    for (uint32_t r = 1; r < ap.levels; ++r) {
        HIP_TRY(hipMemcpyAsync(c.h_ad_count, counts + cur, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        const uint32_t n_active = *c.h_ad_count;
        if (!n_active) break;
        if (n_active > ap.list_cap) return fail(SPIRA_E_LIMIT, "internal: the active list is longer than the tile");
        HIP_TRY(hipMemsetAsync(counts + (cur ^ 1), 0, sizeof(uint32_t), st));
        const spira::AdaptiveRound g = ap.round(r, n_active);
        spira::RefineArgs<T> ra{};
        ra.scene = k.a.scene; ra.rc = k.a.rc; ra.ad = aa;
        ra.list_in = lists[cur]; ra.n_active = n_active; ra.list_out = lists[cur ^ 1]; ra.count_out = counts + (cur ^ 1);
        ra.sample_first = ap.level(r - 1); ra.samples = g.samples; ra.chunk = g.chunk; ra.ppw = g.ppw;
        ra.stats = k.stats();
        const size_t lds_r = k.lds + (size_t)ap.lds_round;
        if (int rc = k.a.scene.n_bvh_tris ? enqueue_refine<T, true>(st, g, lds_r, ra) : enqueue_refine<T, false>(st, g, lds_r, ra)) return rc;
        ++k.launches; ++rounds;
        samples += (uint64_t)n_active * g.samples;
        cur ^= 1;
    }
    hipLaunchKernelGGL((spira::k_finalize_adaptive<T>), dim3(plan.blocks(tile_pixels)), k.block(), 0, st, (const P4 *)k.accum(), (const uint32_t *)c.ad_n.p, (const T *)c.ad_q.p,
                       (uint32_t)tile_pixels, p->flags & SPIRA_POST_MASK, out.hdr, out.img, out_on_device ? out_spp : (uint32_t *)nullptr, out_on_device ? out_q : (T *)nullptr);
    ++k.launches;
    spira_counters delta{};
    delta.samples = samples;
    delta.passes = plan.n_pass + rounds;
    delta.launches = k.launches;
    delta.bounce_launches = plan.n_pass;
    if (int rc = end_counters(s, delta, false)) return rc;

    if (int rc = out.copy(s, out_hdr, out_img, tile_pixels)) return rc;
    if (!out_on_device) {
        if (out_spp) HIP_TRY(hipMemcpyAsync(out_spp, c.ad_n.p, tile_pixels * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
        if (out_q) HIP_TRY(hipMemcpyAsync(out_q, c.ad_q.p, tile_pixels * sizeof(T), hipMemcpyDeviceToHost, st));
    }
    return s.close();
}
namespace {

// The rule as host arithmetic: 1 converged, 0 not, or a negative code
template <class T>
int adaptive_converged_host(const T *sum3, T q, uint32_t n, double tolerance, double floor) {
    if (!sum3) return fail(SPIRA_E_INVALID, "sum3 is NULL");
    if (n < 1 || n > SPIRA_MAX_SPP) return fail(SPIRA_E_INVALID, "n out of range [1, 2^24]");
    if (!(tolerance >= 0) || !(floor >= 0)) return fail(SPIRA_E_INVALID, "tolerance and floor must be >= 0");
    return spira::adaptive_converged<T>(sum3[0], sum3[1], sum3[2], q, n, (T)tolerance, (T)floor) ? 1 : 0;
}

}  // namespace
// ---- first-hit feature buffers (spira_render_features_*; spira_denoise.h, k_features): one launch over the tile, one lane per pixel walking its samples.
// Asynchronous in the device-output form like every device entry; the counters of the last render are left as they are.
template <class T>
int spira_tu::Impl<T>::features(const spira_scene *h, const T *spheres5, const T *materials8, const T *triangles10, const T *camera12, const spira_params *p,
                                T *out_albedo, T *out_normal, T *out_depth, bool out_on_device, void *user_stream) {
    uint32_t rows = 0;
    const T *some_out = out_albedo ? out_albedo : out_normal ? out_normal : out_depth;
    if (int rc = validate_call<T>(h, spheres5, materials8, triangles10, camera12, p, some_out, (const T *)nullptr, false, 0, nullptr, &rows)) return rc;
    const char *msg = nullptr;
    if (int rc = spira::features_check(p->flags, some_out != nullptr, &msg)) return fail(rc, msg);
    Session s;
    if (int rc = Session::open(s, out_on_device, user_stream)) return rc;
    Ctx &c = *s.cp;
    const hipStream_t st = s.st;

    spira::FeatureArgs<T> fa{};
    if (int rc = acquire_scene<T>(c, st, h, spheres5, materials8, triangles10, p, fa.scene)) return rc;
    fa.scene.spd = nullptr;
    fill_const<T>(fa.rc, camera12, p, rows, 1);
    const uint64_t tile_pixels = (uint64_t)rows * p->width;
    if (!fastdiv_selfcheck(fa.rc.width, fa.rc.tile_pixels) || !fastdiv_selfcheck(fa.rc.stripe_h ? fa.rc.stripe_h : 1, rows))
        return fail(SPIRA_E_LIMIT, "internal: fast division self-check failed");
    fa.albedo = out_albedo; fa.normal = out_normal; fa.depth = out_depth;
    if (!out_on_device) {
        if (int rc = c.out_tmp.ensure(7 * tile_pixels * sizeof(T))) return rc;
        T *base = (T *)c.out_tmp.p;
        fa.albedo = out_albedo ? base : nullptr;
        fa.normal = out_normal ? base + 3 * tile_pixels : nullptr;
        fa.depth = out_depth ? base + 6 * tile_pixels : nullptr;
    }
    const size_t lds = spira::scene_lds_bytes<T>(fa.scene.n_spheres, fa.scene.n_materials, fa.scene.n_triangles);
    const dim3 grid(spira::features_grid(tile_pixels, spira::kBlock, (uint32_t)c.num_cus)), block(spira::kBlock);
    if (int rc = fa.scene.n_bvh_tris    ? launch_lds(spira::k_features<T, true, false>, grid, block, lds, st, fa)
                 : fa.scene.n_triangles ? launch_lds(spira::k_features<T, false, true>, grid, block, lds, st, fa)
                                        : launch_lds(spira::k_features<T, false, false>, grid, block, lds, st, fa)) return rc;
    if (!out_on_device) {
        if (out_albedo) HIP_TRY(hipMemcpyAsync(out_albedo, fa.albedo, 3 * tile_pixels * sizeof(T), hipMemcpyDeviceToHost, st));
        if (out_normal) HIP_TRY(hipMemcpyAsync(out_normal, fa.normal, 3 * tile_pixels * sizeof(T), hipMemcpyDeviceToHost, st));
        if (out_depth) HIP_TRY(hipMemcpyAsync(out_depth, fa.depth, tile_pixels * sizeof(T), hipMemcpyDeviceToHost, st));
    }
    return s.close();
}
namespace {

// ======================================================================= the list calls on a scene handle: what the queries, radiance and the gathers share
// Each answers a caller's list (rays, points, sweeps or boxes) entry by entry.  Written once for all of them: the opening, the staging of a host caller's
// arrays, the pass loop of the calls that split their samples, the two choices of a kernel by the scene's shape, and the whole call of a query that is
// one launch (list_query_call).  The counters of the last render are left as they are.
template <class T>
int open_list_call(Session &s, const spira_scene *h, bool on_device, void *user_stream, spira::SceneGlobal<T> &g) {
    if (int rc = check_handle<T>(h)) return rc;
    if (int rc = Session::open(s, on_device, user_stream)) return rc;
    scene_pointers<T>(h->store, g);
    g.spd = nullptr;
    return 0;
}

// The arrays of a list call.  A block names the caller's array, its size, its direction and the pointer field of the call's Args that the kernels read it
// through; stage_in fills that field, so no entry binds a staged address by its place in a table.  Device form: the caller's pointers pass through, no
// buffer of the context is touched and nothing is allocated.  Host form: the blocks lie in the context's list_io in the order given, each at a multiple
// of 16 bytes from its base (spira::stage_layout; list_io comes from hipMalloc), a NULL block taking no room and staying NULL — stage_in copies the
// kStageIn ones in, stage_out (after the launches) copies the kStageOut ones back, in the order given.
enum : unsigned { kStageIn = 1, kStageOut = 2 };
struct StageBlock {
    void *host; size_t bytes; unsigned dir;
    void *slot;      // the P * field of the Args
    void *dev = nullptr;
    template <class P>
    StageBlock(P *&field, P *array, size_t bytes_, unsigned dir_) : host((void *)array), bytes(bytes_), dir(dir_), slot(&field) {}
    void bind(void *d) { dev = d; std::memcpy(slot, &d, sizeof d); }
};
template <int N>
int stage_in(Session &s, StageBlock (&b)[N]) {
    if (!s.host_out) { for (StageBlock &k : b) k.bind(k.host); return 0; }
    size_t bytes[N], at[N];
    bool present[N];
    for (int k = 0; k < N; ++k) { bytes[k] = b[k].bytes; present[k] = b[k].host != nullptr; }
    if (int rc = s.cp->list_io.ensure(spira::stage_layout(bytes, present, N, at))) return rc;
    for (int k = 0; k < N; ++k) {
        b[k].bind(present[k] ? (char *)s.cp->list_io.p + at[k] : nullptr);
        if (present[k] && (b[k].dir & kStageIn)) HIP_TRY(hipMemcpyAsync(b[k].dev, b[k].host, b[k].bytes, hipMemcpyHostToDevice, s.st));
    }
    return 0;
}
template <int N>
int stage_out(Session &s, const StageBlock (&b)[N]) {
    if (!s.host_out) return 0;
    for (const StageBlock &k : b)
        if (k.host && (k.dir & kStageOut)) HIP_TRY(hipMemcpyAsync(k.host, k.dev, k.bytes, hipMemcpyDeviceToHost, s.st));
    return 0;
}

// The passes of a call that splits its samples (RadiancePlan; spira_plan.h): the pass's fields of `a` (RadianceArgs, GatherArgs or GatherVisibleArgs — the same
// names in all three), the checks every pass gets, then launch().  ws_room: the items the call's workspace holds (~0: the call has none).
template <class A, class Launch>
int run_passes(const spira::RadiancePlan &pl, uint32_t sample0, uint64_t ws_room, A &a, Launch launch) {
    for (uint32_t pass = 0; pass < pl.n_pass; ++pass) {
        const uint64_t items = pl.items(pass);
        if (items > spira::kRadianceMaxItems) return fail(SPIRA_E_LIMIT, "internal: a pass holds more items than an index reaches");
        a.sample_first = sample0 + pl.first(pass);
        a.spp_pass = pl.count(pass);
        a.n_items = (uint32_t)items;
        a.fd_spp = spira::fastdiv_make(a.spp_pass);
        a.write_valid = pass == 0 ? 1u : 0u;
        if (!fastdiv_selfcheck(a.spp_pass, a.n_items)) return fail(SPIRA_E_LIMIT, "internal: fast division self-check failed");
        if (items > ws_room) return fail(SPIRA_E_LIMIT, "internal: the workspace is smaller than the pass");
        if (int rc = launch()) return rc;
    }
    return 0;
}

// The kernels of a list query by the scene's shape.  A scene with a tree: the refilled sessions on cp.grid workgroups (lds_stack: with the waves' LDS stack
// levels behind the scene, where kCastLdsStack asks for some), or under SPIRA_CAST_INPLACE the one-lane-per-item kernel walking the tree; without a tree
// that kernel with the LDS triangle scan, or over spheres alone.  The one-lane-per-item kernels stride a flat grid.
template <class A> struct ListKernels { void (*session)(A), (*tree)(A), (*tri)(A), (*spheres)(A); bool lds_stack; };
template <class A>
int launch_list(const ListKernels<A> &k, const spira::CastPlan &cp, bool inplace, size_t lds, hipStream_t st, const A &a) {
    const dim3 block(spira::kBlock), flat(cp.grid_flat);
    if (a.scene.n_bvh_tris && !inplace)
        return launch_lds(k.session, dim3(cp.grid), block, lds + (k.lds_stack ? (size_t)spira::kCastLdsStack * 64 * sizeof(uint32_t) * cp.wpb : 0), st, a);
    return launch_lds(a.scene.n_bvh_tris ? k.tree : a.scene.n_triangles ? k.tri : k.spheres, flat, block, lds, st, a);
}
spira::CastKnobs read_cast_knobs() {
    spira::CastKnobs k;
    k.refill = env_u32("SPIRA_CAST_REFILL", SPIRA_CAST_REFILL);
    k.waves_per_cu = env_u32("SPIRA_CAST_WAVES_PER_CU", SPIRA_CAST_WAVES_PER_CU);
    return k;
}
// A query answered by one launch over the caller's n items (cast, closest point, multi-hit, K-nearest, sweep, box overlap, signed distance), once its
// entry has checked the arguments — so an argument error needs no device —, chosen the kernels, set the fields of `a` that are its own and listed the
// arrays: the session, the launch arithmetic (make_cast_plan; base, rem and refill_free have these names in every Args), the staging, the launch.  The
// device form touches no workspace of the context (it allocates nothing); the host form stages the blocks of io.
template <class T, class A, int N>
int list_query_call(const spira_scene *h, uint32_t n, uint32_t flags, bool on_device, void *user_stream, A &a, StageBlock (&io)[N], const ListKernels<A> &kernels) {
    Session s;
    if (int rc = open_list_call<T>(s, h, on_device, user_stream, a.scene)) return rc;
    const spira::CastPlan cp = spira::make_cast_plan(n, (uint32_t)s.cp->num_cus, spira::kBlock, read_cast_knobs());
    a.base = cp.base; a.rem = cp.rem; a.refill_free = cp.refill_free;
    if (int rc = stage_in(s, io)) return rc;
    const size_t lds = spira::scene_lds_bytes<T>(a.scene.n_spheres, a.scene.n_materials, a.scene.n_triangles);
    if (int rc = launch_list(kernels, cp, (flags & SPIRA_CAST_INPLACE) != 0, lds, s.st, a)) return rc;
    if (int rc = stage_out(s, io)) return rc;
    return s.close();
}
// The kernels of a path loop, k[BVH][EXT]: a scene with a tree or without, the material extensions or not.
template <class A>
int launch_paths(void (*const (&k)[2][2])(A), dim3 grid, size_t lds, hipStream_t st, const A &a) {
    const bool ext = (a.rc.flags & (SPIRA_EXT_DIELECTRIC | SPIRA_EXT_SPECTRAL)) != 0;
    return launch_lds(k[a.scene.n_bvh_tris ? 1 : 0][ext ? 1 : 0], grid, dim3(spira::kBlock), lds, st, a);
}

}  // namespace
// ======================================================================= spira_scene_cast_* / spira_scene_occluded_*: the caller's rays against a handle
// Kernels and the ray preparation: spira_query.h; the call: list_query_call.
template <class T>
int spira_tu::Impl<T>::cast(const spira_scene *h, const T *rays8, uint32_t n_rays, uint32_t flags, int *out_prim, T *out_t, T *out_normal, uint8_t *out_hit,
                            bool any, bool on_device, void *user_stream) {
    using A = spira::CastArgs<T>;
    const ListKernels<A> closest = {spira::k_cast_session<T, false>, spira::k_cast<T, true, false, false>, spira::k_cast<T, false, true, false>, spira::k_cast<T, false, false, false>, true};
    const ListKernels<A> occluded = {spira::k_cast_session<T, true>, spira::k_cast<T, true, false, true>, spira::k_cast<T, false, true, true>, spira::k_cast<T, false, false, true>, true};
    const char *msg = nullptr;
    if (int rc = spira::cast_check(rays8 != nullptr, n_rays, flags, any ? out_hit != nullptr : (out_prim || out_t || out_normal), &msg)) return fail(rc, msg);
    A a{};
    a.n_rays = n_rays;
    const size_t n = n_rays, t_b = n * sizeof(T);
    StageBlock io[] = {{a.rays, rays8, 8 * t_b, kStageIn}, {a.t, out_t, t_b, kStageOut}, {a.normal, out_normal, 3 * t_b, kStageOut}, {a.prim, out_prim, n * sizeof(int), kStageOut},
                       {a.hit, out_hit, n, kStageOut}};
    return list_query_call<T>(h, n_rays, flags, on_device, user_stream, a, io, any ? occluded : closest);
}

// ======================================================================= spira_scene_closest_point_*: the nearest surface point for the caller's points
// Kernels, the point preparation and the two closest-point functions: spira_nearest.h; the call: list_query_call.
template <class T>
int spira_tu::Impl<T>::nearest(const spira_scene *h, const T *points4, uint32_t n_points, uint32_t flags, int *out_prim, T *out_dist, T *out_point, uint32_t *out_trips,
                               bool on_device, void *user_stream) {
    using A = spira::NearestArgs<T>;
    const ListKernels<A> kernels = {spira::k_nearest_session<T>, spira::k_nearest<T, true, false>, spira::k_nearest<T, false, true>, spira::k_nearest<T, false, false>, false};
    const char *msg = nullptr;
    if (int rc = spira::nearest_check(points4 != nullptr, n_points, flags, out_prim || out_dist || out_point, &msg)) return fail(rc, msg);
    A a{};
    a.n_points = n_points;
    const size_t n = n_points, t_b = n * sizeof(T);
    StageBlock io[] = {{a.points, points4, 4 * t_b, kStageIn}, {a.dist, out_dist, t_b, kStageOut}, {a.point, out_point, 3 * t_b, kStageOut},
                       {a.prim, out_prim, n * sizeof(int), kStageOut}, {a.trips, out_trips, n * sizeof(uint32_t), kStageOut}};
    return list_query_call<T>(h, n_points, flags, on_device, user_stream, a, io, kernels);
}
namespace {

// ======================================================================= spira_scene_cast_hits_*: the first max_hits hits of every ray, in order
// Kernels, the list and the pruning argument: spira_hits.h; the call: list_query_call, with the kernels whose list capacity (1, 4 or 16) is the smallest
// that holds max_hits.
template <class T, int CAP>
ListKernels<spira::HitsArgs<T>> hits_kernels() {
    return {spira::k_hits_session<T, CAP>, spira::k_hits<T, true, false, CAP>, spira::k_hits<T, false, true, CAP>, spira::k_hits<T, false, false, CAP>, true};
}
}  // namespace
template <class T>
int spira_tu::Impl<T>::hits(const spira_scene *h, const T *rays8, uint32_t n_rays, uint32_t max_hits, uint32_t flags, int *out_prim, T *out_t, uint32_t *out_count,
                            bool on_device, void *user_stream) {
    using A = spira::HitsArgs<T>;
    const char *msg = nullptr;
    if (max_hits == 0) { out_prim = nullptr; out_t = nullptr; }      // (count only: the lists have no slots)
    if (int rc = spira::hits_check(rays8 != nullptr, n_rays, max_hits, flags, out_prim || out_t || out_count, &msg)) return fail(rc, msg);
    const ListKernels<A> kernels = max_hits <= 1 ? hits_kernels<T, 1>() : max_hits <= 4 ? hits_kernels<T, 4>() : hits_kernels<T, 16>();
    A a{};
    a.n_rays = n_rays; a.max_hits = max_hits; a.count_all = (flags & SPIRA_HITS_COUNT_ALL) ? 1u : 0u;
    const size_t n = n_rays, slots = n * max_hits;
    StageBlock io[] = {{a.rays, rays8, 8 * n * sizeof(T), kStageIn}, {a.t, out_t, slots * sizeof(T), kStageOut}, {a.prim, out_prim, slots * sizeof(int), kStageOut},
                       {a.count, out_count, n * sizeof(uint32_t), kStageOut}};
    return list_query_call<T>(h, n_rays, flags, on_device, user_stream, a, io, kernels);
}
namespace {

// ======================================================================= spira_scene_nearest_k_*: the max_near closest objects of every point, in order
// Kernels, the list and the pruning argument: spira_knearest.h; the call: list_query_call, with the kernels whose list capacity (1, 4 or 16) is the
// smallest that holds max_near.
template <class T, int CAP>
ListKernels<spira::KNearArgs<T>> knear_kernels() {
    return {spira::k_knear_session<T, CAP>, spira::k_knear<T, true, false, CAP>, spira::k_knear<T, false, true, CAP>, spira::k_knear<T, false, false, CAP>, false};
}
}  // namespace
template <class T>
int spira_tu::Impl<T>::nearest_k(const spira_scene *h, const T *points4, uint32_t n_points, uint32_t max_near, uint32_t flags, int *out_prim, T *out_dist, T *out_point,
                                 uint32_t *out_count, uint32_t *out_trips, bool on_device, void *user_stream) {
    using A = spira::KNearArgs<T>;
    const char *msg = nullptr;
    if (max_near == 0) { out_prim = nullptr; out_dist = nullptr; out_point = nullptr; }      // (count only: the lists have no slots)
    if (int rc = spira::nearest_k_check(points4 != nullptr, n_points, max_near, flags, out_prim || out_dist || out_point || out_count, &msg)) return fail(rc, msg);
    const ListKernels<A> kernels = max_near <= 1 ? knear_kernels<T, 1>() : max_near <= 4 ? knear_kernels<T, 4>() : knear_kernels<T, 16>();
    A a{};
    a.n_points = n_points; a.max_near = max_near; a.count_all = (flags & SPIRA_NEAR_COUNT_ALL) ? 1u : 0u;
    const size_t n = n_points, slots = n * max_near;
    StageBlock io[] = {{a.points, points4, 4 * n * sizeof(T), kStageIn}, {a.dist, out_dist, slots * sizeof(T), kStageOut}, {a.point, out_point, 3 * slots * sizeof(T), kStageOut},
                       {a.prim, out_prim, slots * sizeof(int), kStageOut}, {a.count, out_count, n * sizeof(uint32_t), kStageOut}, {a.trips, out_trips, n * sizeof(uint32_t), kStageOut}};
    return list_query_call<T>(h, n_points, flags, on_device, user_stream, a, io, kernels);
}

// ======================================================================= spira_scene_sweep_* / spira_scene_sweep_blocked_*: the first contact of a moving ball
// Kernels, the contract and the margin argument: spira_sweep.h; the call: list_query_call.
template <class T>
int spira_tu::Impl<T>::sweep(const spira_scene *h, const T *rays8, const T *radii, uint32_t n_sweeps, uint32_t flags, int *out_prim, T *out_t, T *out_point, T *out_normal,
                             uint8_t *out_hit, uint32_t *out_trips, bool any, bool on_device, void *user_stream) {
    using A = spira::SweepArgs<T>;
    const ListKernels<A> first = {spira::k_sweep_session<T, false>, spira::k_sweep<T, true, false, false>, spira::k_sweep<T, false, true, false>, spira::k_sweep<T, false, false, false>, false};
    const ListKernels<A> blocked = {spira::k_sweep_session<T, true>, spira::k_sweep<T, true, false, true>, spira::k_sweep<T, false, true, true>, spira::k_sweep<T, false, false, true>, false};
    const char *msg = nullptr;
    if (int rc = spira::sweep_check(rays8 != nullptr, radii != nullptr, n_sweeps, flags, any ? out_hit != nullptr : (out_prim || out_t || out_point || out_normal), &msg)) return fail(rc, msg);
    A a{};
    a.n = n_sweeps;
    const size_t n = n_sweeps, t_b = n * sizeof(T);
    StageBlock io[] = {{a.rays, rays8, 8 * t_b, kStageIn}, {a.radii, radii, t_b, kStageIn}, {a.t, out_t, t_b, kStageOut}, {a.point, out_point, 3 * t_b, kStageOut},
                       {a.normal, out_normal, 3 * t_b, kStageOut}, {a.prim, out_prim, n * sizeof(int), kStageOut}, {a.trips, out_trips, n * sizeof(uint32_t), kStageOut},
                       {a.hit, out_hit, n, kStageOut}};
    return list_query_call<T>(h, n_sweeps, flags, on_device, user_stream, a, io, any ? blocked : first);
}
namespace {

// ======================================================================= spira_scene_overlap_box_* / spira_scene_overlap_any_*: what touches an oriented box
// Kernels, the contract and the margin argument: spira_overlap.h; the call: list_query_call, with the kernels whose list capacity (1, 4 or 16) is the
// smallest that holds max_list.
template <class T, bool ANY, int CAP>
ListKernels<spira::OverlapArgs<T>> overlap_kernels() {
    return {spira::k_overlap_session<T, ANY, CAP>, spira::k_overlap<T, true, false, ANY, CAP>, spira::k_overlap<T, false, true, ANY, CAP>, spira::k_overlap<T, false, false, ANY, CAP>, false};
}
}  // namespace
template <class T>
int spira_tu::Impl<T>::overlap(const spira_scene *h, const T *boxes10, uint32_t n_boxes, uint32_t max_list, uint32_t flags, int *out_prim, uint32_t *out_count, uint8_t *out_hit,
                               uint32_t *out_trips, bool any, bool on_device, void *user_stream) {
    using A = spira::OverlapArgs<T>;
    const char *msg = nullptr;
    if (any) max_list = 0;
    if (max_list == 0) out_prim = nullptr;      // (count only: the lists have no slots)
    if (int rc = spira::overlap_check(boxes10 != nullptr, n_boxes, max_list, flags, any ? out_hit != nullptr : (out_prim || out_count), &msg)) return fail(rc, msg);
    const ListKernels<A> kernels = any ? overlap_kernels<T, true, 1>()
                                       : max_list <= 1 ? overlap_kernels<T, false, 1>() : max_list <= 4 ? overlap_kernels<T, false, 4>() : overlap_kernels<T, false, 16>();
    A a{};
    a.n = n_boxes; a.max_list = max_list;
    const size_t n = n_boxes, slots = n * max_list;
    StageBlock io[] = {{a.boxes, boxes10, 10 * n * sizeof(T), kStageIn}, {a.prim, out_prim, slots * sizeof(int), kStageOut}, {a.count, out_count, n * sizeof(uint32_t), kStageOut},
                       {a.trips, out_trips, n * sizeof(uint32_t), kStageOut}, {a.hit, out_hit, n, kStageOut}};
    return list_query_call<T>(h, n_boxes, flags, on_device, user_stream, a, io, kernels);
}
namespace {

// ======================================================================= spira_scene_overlap_tri_* / spira_scene_overlap_tri_any_*: what a triangle cuts
// Kernels, the contract and the margin argument: spira_trioverlap.h; the call is the box query's (its arguments, its check, its blocks) with these kernels.
template <class T, bool ANY, int CAP>
ListKernels<spira::TriOverlapArgs<T>> trioverlap_kernels() {
    return {spira::k_trioverlap_session<T, ANY, CAP>, spira::k_trioverlap<T, true, false, ANY, CAP>, spira::k_trioverlap<T, false, true, ANY, CAP>,
            spira::k_trioverlap<T, false, false, ANY, CAP>, false};
}
}  // namespace
template <class T>
int spira_tu::Impl<T>::overlap_tri(const spira_scene *h, const T *triangles10, uint32_t n_tris, uint32_t max_list, uint32_t flags, int *out_prim, uint32_t *out_count,
                                   uint8_t *out_hit, uint32_t *out_trips, bool any, bool on_device, void *user_stream) {
    using A = spira::TriOverlapArgs<T>;
    const char *msg = nullptr;
    if (any) max_list = 0;
    if (max_list == 0) out_prim = nullptr;      // (count only: the lists have no slots)
    if (int rc = spira::overlap_tri_check(triangles10 != nullptr, n_tris, max_list, flags, any ? out_hit != nullptr : (out_prim || out_count), &msg)) return fail(rc, msg);
    const ListKernels<A> kernels = any ? trioverlap_kernels<T, true, 1>()
                                       : max_list <= 1 ? trioverlap_kernels<T, false, 1>() : max_list <= 4 ? trioverlap_kernels<T, false, 4>() : trioverlap_kernels<T, false, 16>();
    A a{};
    a.n = n_tris; a.max_list = max_list;
    const size_t n = n_tris, slots = n * max_list;
    StageBlock io[] = {{a.boxes, triangles10, 10 * n * sizeof(T), kStageIn}, {a.prim, out_prim, slots * sizeof(int), kStageOut}, {a.count, out_count, n * sizeof(uint32_t), kStageOut},
                       {a.trips, out_trips, n * sizeof(uint32_t), kStageOut}, {a.hit, out_hit, n, kStageOut}};
    return list_query_call<T>(h, n_tris, flags, on_device, user_stream, a, io, kernels);
}
namespace {

// ======================================================================= spira_scene_signed_distance_*: the nearest surface of every point and which side of it
// Kernels and the contract: spira_sdf.h; the call: list_query_call, with the kernels with or without the nearest walk (out_prim, out_dist and out_point
// all NULL: the sign-only query).
static_assert(spira::kSdfSkipped == SPIRA_SDF_SKIPPED, "spira_sdf.h and the header disagree on SPIRA_SDF_SKIPPED");
template <class T, bool NEAR>
ListKernels<spira::SdfArgs<T>> sdf_kernels() {
    return {spira::k_sdf_session<T, NEAR>, spira::k_sdf<T, true, false, NEAR>, spira::k_sdf<T, false, true, NEAR>, spira::k_sdf<T, false, false, NEAR>, false};
}
}  // namespace
template <class T>
int spira_tu::Impl<T>::signed_distance(const spira_scene *h, const T *points4, uint32_t n_points, uint32_t flags, int *out_prim, T *out_dist, T *out_point, uint8_t *out_inside,
                                       uint32_t *out_crossings, uint32_t *out_trips, bool on_device, void *user_stream) {
    using A = spira::SdfArgs<T>;
    const char *msg = nullptr;
    if (int rc = spira::signed_distance_check(points4 != nullptr, n_points, flags, out_prim || out_dist || out_point || out_inside || out_crossings, &msg)) return fail(rc, msg);
    const ListKernels<A> kernels = spira::signed_distance_wants_nearest(out_prim, out_dist, out_point) ? sdf_kernels<T, true>() : sdf_kernels<T, false>();
    A a{};
    a.n_points = n_points;
    const size_t n = n_points, t_b = n * sizeof(T);
    StageBlock io[] = {{a.points, points4, 4 * t_b, kStageIn}, {a.dist, out_dist, t_b, kStageOut}, {a.point, out_point, 3 * t_b, kStageOut}, {a.prim, out_prim, n * sizeof(int), kStageOut},
                       {a.crossings, out_crossings, 3 * n * sizeof(uint32_t), kStageOut}, {a.trips, out_trips, n * sizeof(uint32_t), kStageOut}, {a.inside, out_inside, n, kStageOut}};
    return list_query_call<T>(h, n_points, flags, on_device, user_stream, a, io, kernels);
}
namespace {

// ======================================================================= spira_scene_radiance_*: path-traced radiance along the caller's rays; spira_camera_rays_*
// Kernels, the ray preparation and the generator: spira_radiance.h; launch arithmetic: spira_plan.h (make_radiance_plan).  One k_radiance launch per pass
// (+ k_radiance_sum where a pass holds more than one sample per ray).  The workspace of such a pass is the context's L, grown on the first call at a size;
// the host form stages rays, sums and valid bytes.
spira::RadianceKnobs read_radiance_knobs() {
    spira::RadianceKnobs k;
    k.waves_per_cu = env_u32("SPIRA_RADIANCE_WAVES_PER_CU", SPIRA_RADIANCE_WAVES_PER_CU);
    k.max_items = env_u32("SPIRA_RADIANCE_MAX_ITEMS", SPIRA_RADIANCE_MAX_ITEMS);
    return k;
}
// What Impl<T>::radiance, Impl<T>::gather and Impl<T>::probe_sh do with their Args (RadianceArgs, GatherArgs, ProbeArgs) once the list's own two fields are
// set: the path constants, the workspace, the staged list / sums / valid bytes, the passes.  list: the block of the caller's n rays or points;
// sum_width: the values of one entry's sums (3; the probe's 9 x 3).
template <class T, class A>
int path_list_call(Session &s, const spira::RadiancePlan &pl, const spira_radiance *rp, A &a, const StageBlock &list, uint32_t n, T *sum_rgb, uint8_t *out_valid,
                   void (*const (&paths)[2][2])(A), void (*sum)(A), size_t sum_width = 3) {
    Ctx &c = *s.cp;
    if (int rc = c.L.ensure(pl.ws_entries * sizeof(spira::Pack3<T>))) return rc;
    if (int rc = attach_spd<T>(c, s.st, rp->flags, a.scene)) return rc;
    spira::seed_halves(rp->seed, a.rc.sA, a.rc.sB);
    a.rc.flags = rp->flags; a.rc.max_depth = rp->max_depth; a.rc.spp = rp->spp;
    a.key0 = rp->key0;
    a.ws = pl.direct ? nullptr : (spira::Pack3<T> *)c.L.p;
    const size_t sum_b = sum_width * (size_t)n * sizeof(T);
    StageBlock io[] = {list, {a.sum, sum_rgb, sum_b, kStageIn | kStageOut}, {a.valid, out_valid, n, kStageOut}};
    if (int rc = stage_in(s, io)) return rc;
    const size_t lds = spira::scene_lds_bytes<T>(a.scene.n_spheres, a.scene.n_materials, a.scene.n_triangles);
    if (int rc = run_passes(pl, rp->sample0, a.ws ? c.L.cap / sizeof(spira::Pack3<T>) : ~0ull, a, [&]() -> int {
            if (int rc2 = launch_paths(paths, dim3(pl.grid), lds, s.st, a)) return rc2;
            if (a.ws) hipLaunchKernelGGL(sum, dim3(pl.grid_flat), dim3(spira::kBlock), 0, s.st, a);
            return 0;
        })) return rc;
    if (int rc = stage_out(s, io)) return rc;
    return s.close();
}
}  // namespace
template <class T>
int spira_tu::Impl<T>::radiance(const spira_scene *h, const T *rays6, uint32_t n_rays, const spira_radiance *rp, T *sum_rgb, uint8_t *out_valid, bool on_device, void *user_stream) {
    using A = spira::RadianceArgs<T>;
    void (*const paths[2][2])(A) = {{spira::k_radiance<T, false, false>, spira::k_radiance<T, false, true>}, {spira::k_radiance<T, true, false>, spira::k_radiance<T, true, true>}};
    const char *msg = nullptr;
    if (int rc = spira::radiance_check(rays6 != nullptr, rp != nullptr, sum_rgb != nullptr, n_rays, rp ? rp->spp : 1, rp ? rp->max_depth : 1, rp ? rp->flags : 0,
                                       rp ? rp->sample0 : 0, rp ? rp->key0 : 0, rp ? rp->reserved : 0, &msg)) return fail(rc, msg);
    Session s;
    A a{};
    if (int rc = open_list_call<T>(s, h, on_device, user_stream, a.scene)) return rc;
    a.n_rays = n_rays;
    const spira::RadiancePlan pl = spira::make_radiance_plan(n_rays, rp->spp, (uint32_t)s.cp->num_cus, spira::kBlock, read_radiance_knobs());
    return path_list_call<T>(s, pl, rp, a, {a.rays, rays6, 6 * (size_t)n_rays * sizeof(T), kStageIn}, n_rays, sum_rgb, out_valid, paths, spira::k_radiance_sum<T>);
}

// The generator: the host form runs camera_ray_generate<T> here, the device form launches k_camera_rays<T> over the same function.
template <class T>
int spira_tu::Impl<T>::camera_rays(const T *camera12, const spira_lens *lens, T *rays6, bool on_device, void *user_stream) {
    if (!camera12) return fail(SPIRA_E_INVALID, "camera12 is NULL");
    if (!lens) return fail(SPIRA_E_INVALID, "the spira_lens struct is NULL");
    if (!rays6) return fail(SPIRA_E_INVALID, "the ray array is NULL");
    const char *msg = nullptr;
    uint32_t rows = 0;
    if (int rc = spira::camera_rays_check(lens->model, lens->width, lens->height, lens->sample, lens->row0, lens->rows, lens->lens_radius, &rows, &msg)) return fail(rc, msg);
    const uint32_t row0 = lens->rows ? lens->row0 : 0, W = lens->width, n = rows * W;
    uint32_t sA, sB;
    spira::seed_halves(lens->seed, sA, sB);
    const T R = (T)lens->lens_radius;
    if (!on_device) {
        for (uint32_t r = 0; r < rows; ++r)
            for (uint32_t ix = 0; ix < W; ++ix)
                spira::camera_ray_generate<T>(camera12, lens->model, W, lens->height, sA, sB, ix, row0 + r, lens->sample, R, rays6 + 6 * ((size_t)r * W + ix));
        return 0;
    }
    Session s;
    if (int rc = Session::open(s, true, user_stream)) return rc;
    spira::CameraRaysArgs<T> a{};
    for (int k = 0; k < 12; ++k) a.cam[k] = camera12[k];
    a.lens_radius = R; a.rays = rays6;
    a.model = lens->model; a.width = W; a.height = lens->height; a.sample = lens->sample; a.sA = sA; a.sB = sB; a.row0 = row0; a.n = n;
    a.fd_width = spira::fastdiv_make(W);
    if (!fastdiv_selfcheck(W, n)) return fail(SPIRA_E_LIMIT, "internal: fast division self-check failed");
    hipLaunchKernelGGL(spira::k_camera_rays<T>, dim3((n + spira::kBlock - 1) / spira::kBlock), dim3(spira::kBlock), 0, s.st, a);
    return s.close();
}
namespace {

// ======================================================================= spira_scene_gather_* / spira_scene_gather_visible_* / spira_gather_rays_*: hemisphere gather at surface points
// Kernels and the sampling rule: spira_gather.h; launch arithmetic: spira_plan.h (make_gather_plan).  The radiance gather is Impl<T>::radiance's call over
// points (path_list_call): one k_gather launch per pass (+ k_gather_sum where a pass holds more than one sample per point), the workspace of such a pass the
// context's L.  The visibility gather runs the same passes with one launch each and no workspace: its device form allocates nothing.  The host forms stage
// points, sums or counts and valid bytes.
spira::GatherKnobs read_gather_knobs() {
    spira::GatherKnobs k;
    k.waves_per_cu = env_u32("SPIRA_GATHER_WAVES_PER_CU", SPIRA_GATHER_WAVES_PER_CU);
    k.max_items = env_u32("SPIRA_GATHER_MAX_ITEMS", SPIRA_GATHER_MAX_ITEMS);
    return k;
}
}  // namespace
template <class T>
int spira_tu::Impl<T>::gather(const spira_scene *h, const T *points6, uint32_t n_points, const spira_radiance *rp, T *sum_rgb, uint8_t *out_valid, bool on_device, void *user_stream) {
    using A = spira::GatherArgs<T>;
    void (*const paths[2][2])(A) = {{spira::k_gather<T, false, false>, spira::k_gather<T, false, true>}, {spira::k_gather<T, true, false>, spira::k_gather<T, true, true>}};
    const char *msg = nullptr;
    if (int rc = spira::gather_check(points6 != nullptr, rp != nullptr, sum_rgb != nullptr, n_points, rp ? rp->spp : 1, rp ? rp->max_depth : 1, rp ? rp->flags : 0,
                                     rp ? rp->sample0 : 0, rp ? rp->key0 : 0, rp ? rp->reserved : 0, &msg)) return fail(rc, msg);
    Session s;
    A a{};
    if (int rc = open_list_call<T>(s, h, on_device, user_stream, a.scene)) return rc;
    a.n_points = n_points;
    const spira::GatherPlan pl = spira::make_gather_plan(n_points, rp->spp, (uint32_t)s.cp->num_cus, spira::kBlock, read_gather_knobs());
    return path_list_call<T>(s, pl, rp, a, {a.points, points6, 6 * (size_t)n_points * sizeof(T), kStageIn}, n_points, sum_rgb, out_valid, paths, spira::k_gather_sum<T>);
}

template <class T>
int spira_tu::Impl<T>::gather_visible(const spira_scene *h, const T *points6, uint32_t n_points, const spira_gather_visible *gv, uint32_t *visible, uint8_t *out_valid,
                                      bool on_device, void *user_stream) {
    using A = spira::GatherVisibleArgs<T>;
    const ListKernels<A> kernels = {spira::k_gather_visible_session<T>, spira::k_gather_visible<T, true, false>, spira::k_gather_visible<T, false, true>,
                                           spira::k_gather_visible<T, false, false>, true};
    const char *msg = nullptr;
    if (int rc = spira::gather_visible_check(points6 != nullptr, gv != nullptr, visible != nullptr, n_points, gv ? gv->spp : 1, gv ? gv->sample0 : 0, gv ? gv->key0 : 0,
                                             gv ? gv->flags : 0, gv ? gv->t_min : 0.0, gv ? gv->t_max : 0.0, &msg)) return fail(rc, msg);
    Session s;
    A a{};
    if (int rc = open_list_call<T>(s, h, on_device, user_stream, a.scene)) return rc;
    const uint32_t num_cus = (uint32_t)s.cp->num_cus;
    const spira::GatherKnobs knobs = read_gather_knobs();
    const spira::GatherPlan pl = spira::make_gather_plan(n_points, gv->spp, num_cus, spira::kBlock, knobs);
    spira::seed_halves(gv->seed, a.sA, a.sB);
    a.n_points = n_points; a.key0 = gv->key0;
    a.t_min = (T)gv->t_min; a.t_max = (T)gv->t_max;
    const size_t n = n_points;
    StageBlock io[] = {{a.points, points6, 6 * n * sizeof(T), kStageIn}, {a.visible, visible, n * sizeof(uint32_t), kStageIn | kStageOut}, {a.valid, out_valid, n, kStageOut}};
    if (int rc = stage_in(s, io)) return rc;
    const size_t lds = spira::scene_lds_bytes<T>(a.scene.n_spheres, a.scene.n_materials, a.scene.n_triangles);
    const bool inplace = (gv->flags & SPIRA_CAST_INPLACE) != 0;
    if (int rc = run_passes(pl, gv->sample0, ~0ull, a, [&]() -> int {
            const spira::CastPlan cp = spira::make_gather_visible_plan(a.n_items, num_cus, spira::kBlock, knobs, read_cast_knobs());
            a.base = cp.base; a.rem = cp.rem; a.refill_free = cp.refill_free;
            return launch_list(kernels, cp, inplace, lds, s.st, a);
        })) return rc;
    if (int rc = stage_out(s, io)) return rc;
    return s.close();
}

// The generator: the host form runs gather_ray_generate<T> here, the device form launches k_gather_rays<T> over the same function.
template <class T>
int spira_tu::Impl<T>::gather_rays(const T *points6, uint32_t n_points, uint32_t sample, uint64_t seed, uint32_t key0, T *rays6, bool on_device, void *user_stream) {
    const char *msg = nullptr;
    if (int rc = spira::gather_rays_check(points6 != nullptr, rays6 != nullptr, n_points, sample, key0, &msg)) return fail(rc, msg);
    uint32_t sA, sB;
    spira::seed_halves(seed, sA, sB);
    if (!on_device) {
        for (uint32_t k = 0; k < n_points; ++k) spira::gather_ray_generate<T>(points6 + 6 * (size_t)k, sA, sB, key0 + k, sample, rays6 + 6 * (size_t)k);
        return 0;
    }
    Session s;
    if (int rc = Session::open(s, true, user_stream)) return rc;
    spira::GatherRaysArgs<T> a{};
    a.points = points6; a.rays = rays6; a.n = n_points; a.sample = sample; a.sA = sA; a.sB = sB; a.key0 = key0;
    hipLaunchKernelGGL(spira::k_gather_rays<T>, dim3((n_points + spira::kBlock - 1) / spira::kBlock), dim3(spira::kBlock), 0, s.st, a);
    return s.close();
}

// ======================================================================= spira_scene_probe_sh_* / spira_probe_rays_*: light probes, nine SH terms of the incoming radiance
// Kernels, the sampling rule and the basis: spira_probe.h.  The call is the gather's (path_list_call under make_gather_plan and the gather's knobs): one
// k_probe launch per pass (+ k_probe_sum where a pass holds more than one sample per point), the workspace the context's L, a row of sums 27 values.
template <class T>
int spira_tu::Impl<T>::probe_sh(const spira_scene *h, const T *points3, uint32_t n_points, const spira_radiance *rp, T *sum_sh, uint8_t *out_valid, bool on_device, void *user_stream) {
    using A = spira::ProbeArgs<T>;
    void (*const paths[2][2])(A) = {{spira::k_probe<T, false, false>, spira::k_probe<T, false, true>}, {spira::k_probe<T, true, false>, spira::k_probe<T, true, true>}};
    const char *msg = nullptr;
    if (int rc = spira::probe_check(points3 != nullptr, rp != nullptr, sum_sh != nullptr, n_points, rp ? rp->spp : 1, rp ? rp->max_depth : 1, rp ? rp->flags : 0,
                                    rp ? rp->sample0 : 0, rp ? rp->key0 : 0, rp ? rp->reserved : 0, &msg)) return fail(rc, msg);
    Session s;
    A a{};
    if (int rc = open_list_call<T>(s, h, on_device, user_stream, a.scene)) return rc;
    a.n_points = n_points;
    const spira::GatherPlan pl = spira::make_gather_plan(n_points, rp->spp, (uint32_t)s.cp->num_cus, spira::kBlock, read_gather_knobs());
    return path_list_call<T>(s, pl, rp, a, {a.points, points3, 3 * (size_t)n_points * sizeof(T), kStageIn}, n_points, sum_sh, out_valid, paths, spira::k_probe_sum<T>, 27);
}

// The generator: the host form runs probe_ray_generate<T> here, the device form launches k_probe_rays<T> over the same function.
template <class T>
int spira_tu::Impl<T>::probe_rays(const T *points3, uint32_t n_points, uint32_t sample, uint64_t seed, uint32_t key0, T *rays6, bool on_device, void *user_stream) {
    const char *msg = nullptr;
    if (int rc = spira::gather_rays_check(points3 != nullptr, rays6 != nullptr, n_points, sample, key0, &msg)) return fail(rc, msg);
    uint32_t sA, sB;
    spira::seed_halves(seed, sA, sB);
    if (!on_device) {
        for (uint32_t k = 0; k < n_points; ++k) spira::probe_ray_generate<T>(points3 + 3 * (size_t)k, sA, sB, key0 + k, sample, rays6 + 6 * (size_t)k);
        return 0;
    }
    Session s;
    if (int rc = Session::open(s, true, user_stream)) return rc;
    spira::ProbeRaysArgs<T> a{};
    a.points = points3; a.rays = rays6; a.n = n_points; a.sample = sample; a.sA = sA; a.sB = sB; a.key0 = key0;
    hipLaunchKernelGGL(spira::k_probe_rays<T>, dim3((n_points + spira::kBlock - 1) / spira::kBlock), dim3(spira::kBlock), 0, s.st, a);
    return s.close();
}
namespace {

// ======================================================================= spira_scene_update_*: new contents for a live handle, the tree refitted on the device
// The arithmetic is spira_refit.h's (one header, host and device); here are its three kernels and the entry that orders them.  Nothing of k_path, the
// walk or the node format is involved: a refit rewrites boxes, and the walk only prunes with them.
struct RefitFrame { double centre[3], scale, pad; };
constexpr uint32_t kRefitBlock = 256, kRefitLevelBlock = 64;      // (a level is a few thousand lanes at most: small workgroups spread it over the CUs)

// device form only: every triangle of the caller's array against the rules, the bits of all of them OR-ed into one word (vector atomics, and only from the
// lanes that have something to say: none, for a mesh that is accepted and of ordinary magnitude)
template <class T>
__global__ __launch_bounds__(kRefitBlock) void k_refit_check(const T *tri10, uint32_t n, uint32_t n_materials, RefitFrame f, int frame, uint32_t *status) {
    const uint32_t i = blockIdx.x * kRefitBlock + threadIdx.x;
    if (i >= n) return;
    T t[10];
#pragma unroll
    for (int k = 0; k < 10; ++k) t[k] = tri10[10 * (size_t)i + k];
    const uint32_t st = spira::refit_check_triangle<T>(t, n_materials, f.centre, f.scale, frame != 0);
    if (st) atomicOr(status, st);
}

// one lane per REORDERED triangle i < n: the original index sits in tris[3 i].w, the ten values are gathered from there, the three packets of the record
// (and of the screening record, where the store has one) go out as 16-byte stores, the padded box to the scratch.  `tris` points past the frame packets.
template <class T>
__global__ __launch_bounds__(kRefitBlock) void k_refit_tris(const T *tri10, uint32_t n, RefitFrame f, spira::RefitPack4<T> *tris, spira::RefitPack4<float> *tris32,
                                                            spira::RefitBox *tbox) {
    const uint32_t i = blockIdx.x * kRefitBlock + threadIdx.x;
    if (i >= n) return;
    const uint32_t oi = spira::refit_index_of<T>(tris[3 * (size_t)i].w);
    if (oi >= n) return;                                   // (cannot happen in a record the builder or this kernel wrote; never read outside the array)
    T t[10];
#pragma unroll
    for (int k = 0; k < 10; ++k) t[k] = tri10[10 * (size_t)oi + k];
    spira::RefitPack4<T> out[3];
    spira::RefitPack4<float> out32[3];
    spira::RefitBox box;
    spira::refit_triangle<T>(t, oi, f.centre, f.scale, f.pad, out, tris32 ? out32 : nullptr, box);
    tris[3 * (size_t)i + 0] = out[0]; tris[3 * (size_t)i + 1] = out[1]; tris[3 * (size_t)i + 2] = out[2];
    if (tris32) { tris32[3 * (size_t)i + 0] = out32[0]; tris32[3 * (size_t)i + 1] = out32[1]; tris32[3 * (size_t)i + 2] = out32[2]; }
    tbox[i] = box;
}

// one launch per level, deepest first (the stream orders them: a node reads the boxes its child nodes wrote in the launch before); one lane per slot in
// [first, end).  The node comes in through the walk's five 16-byte loads; a hole is left alone; words 0-3 and 8-19 go back as four 16-byte stores (words
// 4-7 are never written), the node's own box to the scratch, and slot 0 also rewrites the root box of the frame packets.
template <class T>
__global__ __launch_bounds__(kRefitLevelBlock) void k_refit_level(uint4 *nodes, uint32_t first, uint32_t end, uint32_t n_slots, const spira::RefitBox *tbox, uint32_t n,
                                                                  spira::RefitBox *nbox, RefitFrame f, spira::RefitPack4<T> *frame_packets) {
    const uint32_t s = first + blockIdx.x * kRefitLevelBlock + threadIdx.x;
    if (s >= end || s >= n_slots) return;
    uint4 *pn = nodes + 5 * (size_t)s;
    const uint4 n0 = pn[0], n1 = pn[1], n2 = pn[2], n3 = pn[3], n4 = pn[4];
    uint32_t w[20] = {n0.x, n0.y, n0.z, n0.w, n1.x, n1.y, n1.z, n1.w, n2.x, n2.y, n2.z, n2.w, n3.x, n3.y, n3.z, n3.w, n4.x, n4.y, n4.z, n4.w};
    spira::RefitBox self;
    if (!spira::refit_node(w, tbox, n, nbox, n_slots, self)) return;
    pn[0] = make_uint4(w[0], w[1], w[2], w[3]);
    pn[2] = make_uint4(w[8], w[9], w[10], w[11]); pn[3] = make_uint4(w[12], w[13], w[14], w[15]); pn[4] = make_uint4(w[16], w[17], w[18], w[19]);
    nbox[s] = self;
    if (s == 0) {
        spira::RefitPack4<T> mn, mx;
        spira::refit_root<T>(self, f.centre, f.scale, mn, mx);
        frame_packets[0] = mn; frame_packets[1] = mx;
    }
}

}  // namespace
// Host form (device_form false): any of the three host arrays, NULL = unchanged; validated in full before the device is touched; returns when the scene
// is ready.  Device form: d_triangles10 in the caller's layout, checked by k_refit_check (ONE synchronisation of the stream, to read the status word), then
// the refit is enqueued and the call returns.  Either way a refused update leaves the handle as it was.
template <class T>
int spira_tu::Impl<T>::scene_update(spira_scene *h, const T *spheres5, const T *materials8, const T *triangles10, const T *d_triangles10, bool device_form, void *user_stream) {
    if (int rc = check_handle<T>(h)) return rc;
    if (h->multi) return fail(SPIRA_E_UNSUPPORTED, "spira_scene_update_* does not take a handle made by spira_scene_create_multi_*");
    SceneStore &s = h->store;
    const bool use_bvh = s.nt > SPIRA_LDS_TRIANGLES;
    const char *msg = nullptr;
    bool mod_s = s.moderate_s, mod_t = s.moderate_t;
    RefitFrame f{};
    for (int k = 0; k < 3; ++k) f.centre[k] = s.bvh_centre[k];
    f.scale = s.bvh_scale;
    f.pad = spira::refit_pad<T>(f.centre, f.scale);
    const bool new_tris = device_form || triangles10 != nullptr;
    if (device_form) {
        if (!d_triangles10) return fail(SPIRA_E_INVALID, "d_triangles10 is NULL");
        if (!s.nt) return fail(SPIRA_E_INVALID, "the scene was created without triangles: the counts of a handle are fixed");
    } else {
        if (!spheres5 && !materials8 && !triangles10) return fail(SPIRA_E_INVALID, "spheres5, materials8 and triangles10 are all NULL: nothing to update");
        if ((spheres5 && !s.ns) || (triangles10 && !s.nt)) return fail(SPIRA_E_INVALID, "the scene was created without that array: the counts of a handle are fixed");
        if (spheres5) { if (int rc = spira::spheres_check<T>(spheres5, s.ns, s.nm, &msg)) return fail(rc, msg); }
        if (materials8) { if (int rc = spira::materials_check<T>(materials8, s.nm, &msg)) return fail(rc, msg); }
        if (triangles10) {
            if (int rc = spira::triangles_check<T>(triangles10, s.nt, s.nm, &msg)) return fail(rc, msg);
            uint32_t st = 0;
            for (uint32_t i = 0; i < s.nt; ++i) st |= spira::refit_check_triangle<T>(triangles10 + 10 * (size_t)i, s.nm, f.centre, f.scale, use_bvh);
            if (st & (spira::kRefitNonFinite | spira::kRefitMaterial)) return fail(SPIRA_E_INVALID, "triangle with a non-finite vertex or a material index out of range");
            if (st & spira::kRefitFrame) return fail(SPIRA_E_LIMIT, "a vertex leaves the frame the tree was built in (|(x - centre) * scale| <= 1): create a new handle for this mesh");
            mod_t = !(st & spira::kRefitImmoderate);
        }
        if (spheres5) mod_s = spira::scene_scale_moderate<T>(spheres5, nullptr, s.ns, 0);
    }
    if (use_bvh && new_tris) {
        const size_t d = (size_t)s.bvh_depth;
        bool ok = s.bvh_prec == (int)sizeof(T) && s.bvh_n == s.nt && d >= 1 && s.bvh_level_first.size() == d + 1 && s.bvh_level_first[0] == 0 && s.bvh_level_first[d] == s.bvh_slots;
        for (size_t l = 0; ok && l < d; ++l) ok = s.bvh_level_first[l] < s.bvh_level_first[l + 1];
        if (!ok) return fail(SPIRA_E_LIMIT, "internal: the handle's tree has no consistent level table");
        if (!(f.pad < 1e12)) return fail(SPIRA_E_LIMIT, "the mesh is too far from the origin for its size: its boxes cannot be padded in Float32");
    }
    Session sess;
    if (int rc = Session::open(sess, device_form, user_stream)) return rc;
    Ctx &c = *sess.cp;
    const hipStream_t st = sess.st;
    if (use_bvh && new_tris) {
        if (int rc = s.refit_tbox.ensure((size_t)s.nt * sizeof(spira::RefitBox))) return rc;
        if (int rc = s.refit_nbox.ensure((size_t)s.bvh_slots * sizeof(spira::RefitBox))) return rc;
        if (!device_form) { if (int rc = s.refit_stage.ensure((size_t)s.nt * 10 * sizeof(T))) return rc; }
    }
    const dim3 tri_grid((s.nt + kRefitBlock - 1) / kRefitBlock), tri_block(kRefitBlock);
    if (device_form) {
        if (int rc = c.refit_status.ensure(sizeof(uint32_t))) return rc;
        if (!c.h_refit_status) HIP_TRY(hipHostMalloc((void **)&c.h_refit_status, sizeof(uint32_t), hipHostMallocDefault));
        HIP_TRY(hipMemsetAsync(c.refit_status.p, 0, sizeof(uint32_t), st));
        hipLaunchKernelGGL((k_refit_check<T>), tri_grid, tri_block, 0, st, d_triangles10, s.nt, s.nm, f, use_bvh ? 1 : 0, (uint32_t *)c.refit_status.p);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(c.h_refit_status, c.refit_status.p, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        const uint32_t status = *c.h_refit_status;
        if (status & spira::kRefitNonFinite) return fail(SPIRA_E_INVALID, "triangle with a non-finite vertex");
        if (status & spira::kRefitMaterial) return fail(SPIRA_E_INVALID, "triangle material index out of range");
        if (status & spira::kRefitFrame) return fail(SPIRA_E_LIMIT, "a vertex leaves the frame the tree was built in (|(x - centre) * scale| <= 1): create a new handle for this mesh");
        mod_t = !(status & spira::kRefitImmoderate);
    }
    spira::SceneGlobal<T> g;
    scene_pointers<T>(s, g);
    if (spheres5) HIP_TRY(hipMemcpyAsync((void *)g.spheres5, spheres5, (size_t)s.ns * 5 * sizeof(T), hipMemcpyHostToDevice, st));
    if (materials8) HIP_TRY(hipMemcpyAsync((void *)g.materials8, materials8, (size_t)s.nm * 8 * sizeof(T), hipMemcpyHostToDevice, st));
    if (new_tris && !use_bvh) {          // an LDS-resident mesh has no tree: its update is the array
        HIP_TRY(hipMemcpyAsync((void *)g.triangles10, device_form ? d_triangles10 : triangles10, (size_t)s.nt * 10 * sizeof(T),
                               device_form ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, st));
    } else if (new_tris) {
        const T *src = d_triangles10;
        if (!device_form) {
            HIP_TRY(hipMemcpyAsync(s.refit_stage.p, triangles10, (size_t)s.nt * 10 * sizeof(T), hipMemcpyHostToDevice, st));
            src = (const T *)s.refit_stage.p;
        }
        spira::RefitPack4<T> *frame_packets = (spira::RefitPack4<T> *)s.bvh_tris.p;
        spira::RefitBox *tbox = (spira::RefitBox *)s.refit_tbox.p, *nbox = (spira::RefitBox *)s.refit_nbox.p;
        hipLaunchKernelGGL((k_refit_tris<T>), tri_grid, tri_block, 0, st, src, s.nt, f, frame_packets + 3, (spira::RefitPack4<float> *)s.bvh_tris32.p, tbox);
        for (int l = s.bvh_depth - 1; l >= 0; --l) {
            const uint32_t first = s.bvh_level_first[(size_t)l], end = s.bvh_level_first[(size_t)l + 1];
            hipLaunchKernelGGL((k_refit_level<T>), dim3((end - first + kRefitLevelBlock - 1) / kRefitLevelBlock), dim3(kRefitLevelBlock), 0, st, (uint4 *)s.bvh_nodes.p, first, end,
                               s.bvh_slots, (const spira::RefitBox *)tbox, s.nt, nbox, f, frame_packets);
        }
    }
    s.moderate_s = mod_s; s.moderate_t = mod_t; s.moderate = mod_s && mod_t;
    return sess.close();
}
namespace {

// ======================================================================= spira_scene_rebuild_*: a new triangle array for a live handle, the tree built anew on the device
// The arithmetic is spira_lbvh.h's (frame, Morton keys, radix tree, collapse) and spira_refit.h's (records and boxes).  A rebuild produces a frame and a
// topology in the context's scratch — nothing of the handle is written while anything can still refuse — then moves them in and lets the refit passes
// (k_refit_tris, k_refit_level) finish the tree.  The kernels that read T are here; the rest is spira_tu::lbvh_topology, compiled once.
inline int lbvh_carve(Ctx &c, uint32_t n, LbvhWs &w) {
    size_t off = 0;
    auto take = [&](size_t bytes) { const size_t o = off; off += (bytes + 255) & ~(size_t)255; return o; };
    const size_t nn = n, n_pad = spira::lbvh_sort_size(n), o_k0 = take(n_pad * 8), o_i0 = take(n_pad * 4), o_lb = take(nn * sizeof(spira::RefitBox)),
                 o_bb = take(2 * nn * sizeof(spira::RefitBox)), o_l = take(nn * 4), o_r = take(nn * 4), o_p = take(2 * nn * 4), o_c = take(nn * 4),
                 o_p0 = take(nn * sizeof(spira::LbvhPending)), o_p1 = take(nn * sizeof(spira::LbvhPending)), o_m = take(nn * sizeof(spira::LbvhMade)),
                 o_cb = take(nn * 4), o_tb = take(nn * 4), o_na = take(nn * 4), o_o = take(nn * 4);
    if (int rc = c.lbvh_ws.ensure(off)) return rc;
    char *b = (char *)c.lbvh_ws.p;
    w.keys = (uint64_t *)(b + o_k0); w.idx = (uint32_t *)(b + o_i0);
    w.leafbox = (spira::RefitBox *)(b + o_lb); w.bbox = (spira::RefitBox *)(b + o_bb);
    w.left = (int32_t *)(b + o_l); w.right = (int32_t *)(b + o_r); w.parent = (int32_t *)(b + o_p); w.counter = (uint32_t *)(b + o_c);
    w.pending[0] = (spira::LbvhPending *)(b + o_p0); w.pending[1] = (spira::LbvhPending *)(b + o_p1); w.made = (spira::LbvhMade *)(b + o_m);
    w.child_base = (uint32_t *)(b + o_cb); w.tri_base = (uint32_t *)(b + o_tb); w.next_at = (uint32_t *)(b + o_na); w.order = (uint32_t *)(b + o_o);
    return 0;
}

// one lane per triangle of the caller's array: the status bits of all of them OR-ed into one word and the exact bounds of all vertices, reduced in the wave
// (shuffles), in the workgroup (LDS), then by vector atomics on order-preserving integer codes — minimum and maximum are exact, so the order does not matter
template <class T>
__global__ __launch_bounds__(kRefitBlock) void k_lbvh_check(const T *tri10, uint32_t n, uint32_t n_materials, LbvhSmall *out) {
    const uint32_t i = blockIdx.x * kRefitBlock + threadIdx.x;
    double lo[3] = {__builtin_inf(), __builtin_inf(), __builtin_inf()}, hi[3] = {-__builtin_inf(), -__builtin_inf(), -__builtin_inf()};
    uint32_t st = 0;
    if (i < n) {
        T t[10];
#pragma unroll
        for (int k = 0; k < 10; ++k) t[k] = tri10[10 * (size_t)i + k];
        const double zero[3] = {0, 0, 0};
        st = spira::refit_check_triangle<T>(t, n_materials, zero, 1.0, false);
#pragma unroll
        for (int k = 0; k < 9; ++k) { const double x = (double)t[k]; lo[k % 3] = x < lo[k % 3] ? x : lo[k % 3]; hi[k % 3] = x > hi[k % 3] ? x : hi[k % 3]; }
    }
    for (int off = 32; off; off >>= 1) {
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const double a = __shfl_xor(lo[k], off), b = __shfl_xor(hi[k], off);
            lo[k] = a < lo[k] ? a : lo[k]; hi[k] = b > hi[k] ? b : hi[k];
        }
        st |= __shfl_xor(st, off);
    }
    __shared__ double s_lo[kRefitBlock / 64][3], s_hi[kRefitBlock / 64][3];
    __shared__ uint32_t s_st[kRefitBlock / 64];
    const uint32_t wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63u) == 0) { for (int k = 0; k < 3; ++k) { s_lo[wave][k] = lo[k]; s_hi[wave][k] = hi[k]; } s_st[wave] = st; }
    __syncthreads();
    if (threadIdx.x < 3) {
        const int k = (int)threadIdx.x;
        double a = s_lo[0][k], b = s_hi[0][k];
        for (uint32_t v = 1; v < kRefitBlock / 64; ++v) { a = s_lo[v][k] < a ? s_lo[v][k] : a; b = s_hi[v][k] > b ? s_hi[v][k] : b; }
        atomicMax(&out->nlo[k], (unsigned long long)~spira::lbvh_enc(a));
        atomicMax(&out->hi[k], (unsigned long long)spira::lbvh_enc(b));
    } else if (threadIdx.x == 3) {
        uint32_t all = 0;
        for (uint32_t v = 0; v < kRefitBlock / 64; ++v) all |= s_st[v];
        if (all) atomicOr(&out->status, all);
    }
}

// one lane per element i of the sort's padded array: triangle i's Morton key in the new frame, itself as the pair's second half, and its padded box
// (original order); beyond the mesh the pairs that sort last
template <class T>
__global__ __launch_bounds__(kRefitBlock) void k_lbvh_keys(const T *tri10, uint32_t n, uint32_t n_pad, RefitFrame f, uint64_t *keys, uint32_t *idx, spira::RefitBox *leafbox) {
    const uint32_t i = blockIdx.x * kRefitBlock + threadIdx.x;
    if (i >= n) { if (i < n_pad) { keys[i] = ~0ull; idx[i] = ~0u; } return; }
    T t[10];
#pragma unroll
    for (int k = 0; k < 10; ++k) t[k] = tri10[10 * (size_t)i + k];
    spira::RefitPack4<T> rec[3];
    spira::RefitBox box;
    spira::refit_triangle<T>(t, i, f.centre, f.scale, f.pad, rec, nullptr, box);
    keys[i] = spira::lbvh_key<T>(t, f.centre, f.scale);
    idx[i] = i;
    leafbox[i] = box;
}

// commit: the new triangle order into the records (tris[3 i].w = bits(original index): k_refit_tris gathers by it) and the new frame into packet 2
template <class T>
__global__ __launch_bounds__(kRefitBlock) void k_lbvh_commit(const uint32_t *order, uint32_t n, RefitFrame f, spira::RefitPack4<T> *frame_packets) {
    const uint32_t i = blockIdx.x * kRefitBlock + threadIdx.x;
    if (i >= n) return;
    frame_packets[3 + 3 * (size_t)i].w = spira::refit_index_bits<T>(order[i]);
    if (i == 0) { spira::RefitPack4<T> p; p.x = (T)f.centre[0]; p.y = (T)f.centre[1]; p.z = (T)f.centre[2]; p.w = (T)f.scale; frame_packets[2] = p; }
}

#if !defined(SPIRA_TU_F32) && !defined(SPIRA_TU_F64MESH)
// ---- the kernels of a rebuild that do not read T (this unit only)
constexpr uint32_t kLbvhScanBlock = 1024;
// the sort (spira_lbvh.h, lbvh_sort_schedule): a tile of kLbvhSortTile pairs in LDS, one lane per pair, every pass of stages k_first .. k_last that stays
// inside the tile; and one pass over the whole array for the strides that do not
__global__ __launch_bounds__(spira::kLbvhSortTile) void k_lbvh_sort_tile(uint64_t *keys, uint32_t *idx, uint32_t k_first, uint32_t k_last) {
    __shared__ uint64_t s_key[spira::kLbvhSortTile];
    __shared__ uint32_t s_idx[spira::kLbvhSortTile];
    const uint32_t t = threadIdx.x, g = blockIdx.x * spira::kLbvhSortTile + t;
    s_key[t] = keys[g]; s_idx[t] = idx[g];
    __syncthreads();
    for (uint32_t k = k_first; k <= k_last && k != 0; k <<= 1)
        for (uint32_t j = spira::lbvh_tile_first_j(k); j > 0; j >>= 1) {
            spira::lbvh_bitonic_cx(s_key, s_idx, t, g, j, k);
            __syncthreads();
        }
    keys[g] = s_key[t]; idx[g] = s_idx[t];
}
__global__ __launch_bounds__(kRefitBlock) void k_lbvh_sort_wide(uint64_t *keys, uint32_t *idx, uint32_t n_pad, uint32_t j, uint32_t k) {
    const uint32_t i = blockIdx.x * kRefitBlock + threadIdx.x;
    if (i < n_pad && (i ^ j) < n_pad) spira::lbvh_bitonic_cx(keys, idx, i, i, j, k);
}
// one lane per inner node of the binary radix tree; lane 0 also seeds the first level of the collapse.  The arrival counters are zeroed here.
__global__ __launch_bounds__(kRefitBlock) void k_lbvh_radix(const uint64_t *keys, uint32_t n, int32_t *left, int32_t *right, int32_t *parent, uint32_t *counter,
                                                            spira::LbvhPending *pending0) {
    const uint32_t i = blockIdx.x * kRefitBlock + threadIdx.x;
    if (i + 1 >= n) return;
    int32_t l, r;
    spira::lbvh_radix_node(keys, n, i, l, r);
    left[i] = l; right[i] = r; counter[i] = 0u;
    if ((uint32_t)l < 2 * n - 1) parent[l] = (int32_t)i;
    if ((uint32_t)r < 2 * n - 1) parent[r] = (int32_t)i;
    if (i == 0) { parent[0] = -1; pending0[0] = {0, 0u}; }
}

// One lane per leaf, walking up: it writes its node's box, bumps the parent's arrival counter, and goes on only if it came second — then the sibling's box
// is complete.  Nobody waits for anybody.  Another CU (another XCD, with an L2 of its own) reads what this lane wrote, so: the box goes out as agent-scope
// stores, a device fence (and the wait for it) stands between the box and the counter, the counter is an agent-scope atomic, and the lane that goes on fences
// again before it reads the sibling's box with agent-scope loads.  Unions of Float32 bounds are exact: the result does not depend on who came first.
__device__ inline void lbvh_box_publish(spira::RefitBox *dst, const spira::RefitBox &b) {
    uint32_t *d = (uint32_t *)dst;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        __hip_atomic_store(d + k, spira::refit_bits(b.lo[k]), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(d + 3 + k, spira::refit_bits(b.hi[k]), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}
__device__ inline void lbvh_box_fetch(const spira::RefitBox *src, spira::RefitBox &b) {
    uint32_t *s = (uint32_t *)src;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        b.lo[k] = spira::refit_f32(__hip_atomic_load(s + k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
        b.hi[k] = spira::refit_f32(__hip_atomic_load(s + 3 + k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
    }
}
__global__ __launch_bounds__(kRefitBlock) void k_lbvh_boxes(uint32_t n, const uint32_t *sorted_idx, const spira::RefitBox *leafbox, const int32_t *left, const int32_t *right,
                                                            const int32_t *parent, uint32_t *counter, spira::RefitBox *bbox) {
    const uint32_t j = blockIdx.x * kRefitBlock + threadIdx.x;
    if (j >= n) return;
    const uint32_t oi = sorted_idx[j];
    if (oi >= n) return;                                   // (cannot happen: the sort permutes 0 .. n-1)
    spira::RefitBox b = leafbox[oi];
    uint32_t cur = (n - 1) + j;
    for (int step = 0; step < 160; ++step) {               // (a path is at most 63 + 32 + 1 nodes long)
        lbvh_box_publish(bbox + cur, b);
        const int32_t p = parent[cur];
        if (p < 0 || (uint32_t)p + 1 >= n) return;         // the root is done
        __threadfence();
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        const uint32_t arrived = __hip_atomic_fetch_add(counter + p, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (arrived == 0u) return;                         // the first of the two: the second one goes on
        __threadfence();
        const int32_t l = left[p], r = right[p];
        const int32_t sib = (uint32_t)l == cur ? r : l;
        if ((uint32_t)sib >= 2 * n - 1) return;
        spira::RefitBox o;
        lbvh_box_fetch(bbox + sib, o);
        spira::lbvh_box_union(b, o, b);
        cur = (uint32_t)p;
    }
}

// collapse, per level: (1) one lane per node of the level works out its entries and slots; (2) ONE workgroup takes the three prefix sums over the level, in
// level order — wave scans by shuffles, the waves' totals through LDS — and leaves the new totals for the host; (3) one lane per node writes its slot, the
// holes of its child block, its leaves' places in the triangle order and its node children's entries in the next level's list
__global__ __launch_bounds__(kRefitLevelBlock) void k_lbvh_make(const spira::LbvhPending *level, uint32_t count, const int32_t *left, const int32_t *right, const spira::RefitBox *bbox,
                                                                uint32_t n_inner, spira::LbvhMade *made) {
    const uint32_t i = blockIdx.x * kRefitLevelBlock + threadIdx.x;
    if (i >= count) return;
    spira::LbvhMade m;
    spira::lbvh_make_node(level[i].bnode, left, right, bbox, n_inner, m);
    made[i] = m;
}
__global__ __launch_bounds__(kLbvhScanBlock) void k_lbvh_scan(const spira::LbvhMade *made, uint32_t count, uint32_t slots0, uint32_t tris0, uint32_t *child_base, uint32_t *tri_base,
                                                              uint32_t *next_at, uint32_t *totals) {
    __shared__ uint32_t s_wave[kLbvhScanBlock / 64][3], s_run[3];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    if (tid < 3) s_run[tid] = tid == 0 ? slots0 : tid == 1 ? tris0 : 0u;
    __syncthreads();
    for (uint32_t base = 0; base < count; base += kLbvhScanBlock) {
        const uint32_t i = base + tid;
        uint32_t v[3] = {0u, 0u, 0u}, inc[3];
        if (i < count) spira::lbvh_node_counts(made[i], v[0], v[1], v[2]);
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            inc[k] = v[k];
            for (uint32_t off = 1; off < 64; off <<= 1) { const uint32_t t = __shfl_up(inc[k], off); if (lane >= off) inc[k] += t; }
            if (lane == 63) s_wave[wave][k] = inc[k];
        }
        __syncthreads();
        uint32_t pre[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) { pre[k] = s_run[k]; for (uint32_t w = 0; w < wave; ++w) pre[k] += s_wave[w][k]; }
        if (i < count) { child_base[i] = v[0] ? pre[0] + inc[0] - v[0] : 0u; tri_base[i] = pre[1] + inc[1] - v[1]; next_at[i] = pre[2] + inc[2] - v[2]; }
        __syncthreads();
        if (tid == kLbvhScanBlock - 1) { for (int k = 0; k < 3; ++k) s_run[k] = pre[k] + inc[k]; }
        __syncthreads();
    }
    if (tid == 0) { totals[0] = s_run[0]; totals[1] = s_run[1]; totals[2] = s_run[2]; totals[3] = 0u; }
}
__global__ __launch_bounds__(kRefitLevelBlock) void k_lbvh_write(const spira::LbvhPending *level, uint32_t count, const spira::LbvhMade *made, const uint32_t *child_base,
                                                                 const uint32_t *tri_base, const uint32_t *next_at, uint32_t n_inner, const uint32_t *sorted_idx, uint32_t *nodes,
                                                                 uint32_t cap_slots, uint32_t *order, uint32_t n, spira::LbvhPending *next_level) {
    const uint32_t i = blockIdx.x * kRefitLevelBlock + threadIdx.x;
    if (i >= count) return;
    const spira::LbvhMade m = made[i];
    spira::lbvh_write_node(m, level[i].slot, child_base[i], tri_base[i], next_at[i], n_inner, sorted_idx, nodes, cap_slots, order, n, next_level);
}
#endif

}  // namespace
// Host form: triangles10 validated in full on the host before the device is touched, staged, then the same pipeline; returns when the scene is ready.
// Device form: d_triangles10 on the caller's stream.  The stream is synchronised once for the check kernel's status and bounds and once per level of the new
// tree (the level's counts); after the last of these the remaining work is enqueued and the call returns.  Whatever refuses, refuses before the handle's
// node array, records, frame packets or level fields are touched.
template <class T>
int spira_tu::Impl<T>::scene_rebuild(spira_scene *h, const T *triangles10, const T *d_triangles10, bool device_form, void *user_stream) {
    if (int rc = check_handle<T>(h)) return rc;
    if (h->multi) return fail(SPIRA_E_UNSUPPORTED, "spira_scene_rebuild_* does not take a handle made by spira_scene_create_multi_*");
    SceneStore &s = h->store;
    const T *given = device_form ? d_triangles10 : triangles10;
    if (!given) return fail(SPIRA_E_INVALID, device_form ? "d_triangles10 is NULL" : "triangles10 is NULL");
    if (!s.nt) return fail(SPIRA_E_INVALID, "the scene was created without triangles: the counts of a handle are fixed");
    const uint32_t n = s.nt;
    const bool use_bvh = n > SPIRA_LDS_TRIANGLES;
    bool mod_t = s.moderate_t;
    if (!device_form) {
        const char *msg = nullptr;
        if (int rc = spira::triangles_check<T>(triangles10, n, s.nm, &msg)) return fail(rc, msg);
        const double zero[3] = {0, 0, 0};
        uint32_t st = 0;
        for (uint32_t i = 0; i < n; ++i) st |= spira::refit_check_triangle<T>(triangles10 + 10 * (size_t)i, s.nm, zero, 1.0, false);
        if (st & (spira::kRefitNonFinite | spira::kRefitMaterial)) return fail(SPIRA_E_INVALID, "triangle with a non-finite vertex or a material index out of range");
        mod_t = !(st & spira::kRefitImmoderate);
    }
    if (use_bvh && (s.bvh_prec != (int)sizeof(T) || s.bvh_n != n || !s.bvh_nodes.p || !s.bvh_tris.p)) return fail(SPIRA_E_LIMIT, "internal: the handle has no tree to replace");
    Session sess;
    if (int rc = Session::open(sess, device_form, user_stream)) return rc;
    Ctx &c = *sess.cp;
    const hipStream_t st = sess.st;
    auto bail = [&](int rc) { (void)mark_done(c, st); return rc; };      // (scratch kernels may still be running: the next call is ordered after them)
    for (void *q : c.lbvh_retired) (void)hipFree(q);
    c.lbvh_retired.clear();
    if (int rc = c.lbvh_small.ensure(sizeof(LbvhSmall))) return rc;
    if (!c.h_lbvh) HIP_TRY(hipHostMalloc((void **)&c.h_lbvh, sizeof(LbvhSmall), hipHostMallocDefault));
    LbvhSmall *small = (LbvhSmall *)c.lbvh_small.p;
    LbvhWs w{};
    const T *src = given;
    if (use_bvh) {
        if (int rc = lbvh_carve(c, n, w)) return rc;
        if (!device_form) {
            if (int rc = s.refit_stage.ensure((size_t)n * 10 * sizeof(T))) return rc;
            HIP_TRY(hipMemcpyAsync(s.refit_stage.p, triangles10, (size_t)n * 10 * sizeof(T), hipMemcpyHostToDevice, st));
            src = (const T *)s.refit_stage.p;
        }
    }
    const dim3 tri_grid((n + kRefitBlock - 1) / kRefitBlock), tri_block(kRefitBlock);
    if (device_form || use_bvh) {
        HIP_TRY(hipMemsetAsync(small, 0, sizeof(LbvhSmall), st));
        hipLaunchKernelGGL((k_lbvh_check<T>), tri_grid, tri_block, 0, st, src, n, s.nm, small);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(c.h_lbvh, small, sizeof(LbvhSmall), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        const uint32_t status = c.h_lbvh->status;
        if (status & spira::kRefitNonFinite) return bail(fail(SPIRA_E_INVALID, "triangle with a non-finite vertex"));
        if (status & spira::kRefitMaterial) return bail(fail(SPIRA_E_INVALID, "triangle material index out of range"));
        mod_t = !(status & spira::kRefitImmoderate);
    }
    if (!use_bvh) {          // an LDS-resident mesh has no tree: its rebuild is the array
        spira::SceneGlobal<T> g;
        scene_pointers<T>(s, g);
        HIP_TRY(hipMemcpyAsync((void *)g.triangles10, given, (size_t)n * 10 * sizeof(T), device_form ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, st));
        s.moderate_t = mod_t; s.moderate = s.moderate_s && mod_t;
        return sess.close();
    }
    // ---- the new frame: what bvh_build would give this array
    double lo[3], hi[3];
    for (int k = 0; k < 3; ++k) { lo[k] = spira::lbvh_dec(~(uint64_t)c.h_lbvh->nlo[k]); hi[k] = spira::lbvh_dec((uint64_t)c.h_lbvh->hi[k]); }
    RefitFrame f{};
    spira::lbvh_frame<T>(lo, hi, f.centre, f.scale);
    f.pad = spira::refit_pad<T>(f.centre, f.scale);
    if (!(f.pad < 1e12)) return bail(fail(SPIRA_E_LIMIT, "the mesh is too far from the origin for its size: its boxes cannot be padded in Float32"));
    const uint32_t n_pad = spira::lbvh_sort_size(n);
    hipLaunchKernelGGL((k_lbvh_keys<T>), dim3(n_pad / kRefitBlock), tri_block, 0, st, src, n, n_pad, f, w.keys, w.idx, w.leafbox);
    HIP_TRY(hipGetLastError());
    LbvhTopo topo;
    if (int rc = spira_tu::lbvh_topology(c, st, n, w, topo)) return bail(rc);
    // ---- the last things that can fail: the handle's own allocations (a node array that has to grow is allocated BEFORE the old one is let go)
    if (int rc = s.refit_tbox.ensure((size_t)n * sizeof(spira::RefitBox))) return bail(rc);
    if (int rc = s.refit_nbox.ensure((size_t)topo.n_slots * sizeof(spira::RefitBox))) return bail(rc);
    const size_t nodes_b = (size_t)topo.n_slots * spira::kLbvhNodeDwords * sizeof(uint32_t);
    if (nodes_b + 128 > s.bvh_nodes.cap) {          // (+ one record of padding, as scene_upload leaves)
        void *np = nullptr;
        const hipError_t e = hipMalloc(&np, nodes_b + 128);
        if (e != hipSuccess) return bail(fail(SPIRA_E_HIP, std::string("hipMalloc: ") + hipGetErrorString(e)));
        (void)hipFree(s.bvh_nodes.p);               // (waits for whatever still walks the old tree)
        s.bvh_nodes.p = np; s.bvh_nodes.cap = nodes_b + 128;
    }
    // ---- commit: topology, triangle order and frame move in, the refit passes write every record and every box
    spira::RefitPack4<T> *frame_packets = (spira::RefitPack4<T> *)s.bvh_tris.p;
    spira::RefitBox *tbox = (spira::RefitBox *)s.refit_tbox.p, *nbox = (spira::RefitBox *)s.refit_nbox.p;
    HIP_TRY(hipMemcpyAsync(s.bvh_nodes.p, c.lbvh_nodes.p, nodes_b, hipMemcpyDeviceToDevice, st));
    hipLaunchKernelGGL((k_lbvh_commit<T>), tri_grid, tri_block, 0, st, (const uint32_t *)w.order, n, f, frame_packets);
    hipLaunchKernelGGL((k_refit_tris<T>), tri_grid, tri_block, 0, st, src, n, f, frame_packets + 3, (spira::RefitPack4<float> *)s.bvh_tris32.p, tbox);
    for (int l = topo.depth - 1; l >= 0; --l) {
        const uint32_t first = topo.level_first[(size_t)l], end = topo.level_first[(size_t)l + 1];
        hipLaunchKernelGGL((k_refit_level<T>), dim3((end - first + kRefitLevelBlock - 1) / kRefitLevelBlock), dim3(kRefitLevelBlock), 0, st, (uint4 *)s.bvh_nodes.p, first, end,
                           topo.n_slots, (const spira::RefitBox *)tbox, n, nbox, f, frame_packets);
    }
    s.bvh_slots = topo.n_slots; s.bvh_depth = topo.depth;
    for (int k = 0; k < 3; ++k) s.bvh_centre[k] = f.centre[k];
    s.bvh_scale = f.scale;
    s.bvh_level_first = topo.level_first;
    s.moderate_t = mod_t; s.moderate = s.moderate_s && mod_t;
    return sess.close();
}

// ---- the a-trous denoiser (spira_denoise_*; spira_denoise.h): prepare, then one launch per iteration between the context's two record buffers, the last
// one writing the outputs.  The device form enqueues and returns; it allocates only when a workspace has to grow (a first call at a size).
template <class T>
int spira_tu::Impl<T>::denoise(const T *color, const T *variance, const T *albedo, const T *normal, const T *depth, const spira_denoise *dn,
                               T *out_hdr, T *out_img, bool on_device, void *user_stream) {
    using P4 = spira::Pack4<T>;
    if (!dn) return fail(SPIRA_E_INVALID, "dn is NULL");
    if (!color) return fail(SPIRA_E_INVALID, "color is NULL");
    spira::DenoiseIn in;
    in.width = dn->width; in.height = dn->height; in.iterations = dn->iterations; in.post = dn->post; in.sigma_l = dn->sigma_l; in.sigma_z = dn->sigma_z;
    in.guides = (variance ? spira::kDenoiseVariance : 0u) | (albedo ? spira::kDenoiseAlbedo : 0u) | (normal ? spira::kDenoiseNormal : 0u) | (depth ? spira::kDenoiseDepth : 0u);
    in.want_hdr = out_hdr != nullptr; in.want_img = out_img != nullptr; in.host = !on_device;
    in.prec = sizeof(T); in.pack4 = sizeof(P4);
    spira::DenoisePlan dp;
    const char *msg = nullptr;
    if (int rc = spira::make_denoise_plan(in, dp, &msg)) return fail(rc, msg);
    Session s;
    if (int rc = Session::open(s, on_device, user_stream)) return rc;
    Ctx &c = *s.cp;
    const hipStream_t st = s.st;
    for (int i = 0; i < 2; ++i) if (int rc = c.dn_rec[i].ensure(dp.rec_bytes)) return rc;
    if (int rc = c.dn_guide.ensure(dp.guide_bytes)) return rc;
    if (int rc = c.dn_io.ensure(dp.io_bytes)) return rc;

    spira::DenoiseArgs<T> a{};
    a.color = color; a.variance = variance; a.albedo = albedo; a.normal = normal; a.depth = depth;
    a.out_hdr = out_hdr; a.out_img = out_img;
    const size_t npix = (size_t)dp.npix;
    if (!on_device) {                    // stage the given planes in, the wanted ones out
        T *base = (T *)c.dn_io.p;
        const T *host_in[5] = {color, variance, albedo, normal, depth};
        const T **dev_in[5] = {&a.color, &a.variance, &a.albedo, &a.normal, &a.depth};
        const size_t planes[5] = {3, 1, 3, 3, 1};
        for (int k = 0; k < 5; ++k)
            if (dp.in_off[k] >= 0) {
                T *d = base + (size_t)dp.in_off[k] * npix;
                HIP_TRY(hipMemcpyAsync(d, host_in[k], planes[k] * npix * sizeof(T), hipMemcpyHostToDevice, st));
                *dev_in[k] = d;
            }
        T *o = base + (size_t)dp.in_planes * npix;
        a.out_hdr = out_hdr ? o : nullptr;
        a.out_img = out_img ? o + (out_hdr ? 3 * npix : 0) : nullptr;
    }
    a.rec[0] = (P4 *)c.dn_rec[0].p; a.rec[1] = (P4 *)c.dn_rec[1].p;
    a.guide = dp.guide_bytes ? (P4 *)c.dn_guide.p : nullptr;
    a.width = dn->width; a.height = dn->height; a.npix = (uint32_t)dp.npix; a.tiles_x = dp.tiles_x;
    a.post = dn->post;
    a.sigma_l = (T)dn->sigma_l; a.sigma_z = (T)dn->sigma_z;
    if (!(a.sigma_l > (T)0) || !(a.sigma_z > (T)0)) return fail(SPIRA_E_INVALID, "spira_denoise: a sigma rounds to zero in the call's precision");
    const dim3 block(spira::kBlock);
    hipLaunchKernelGGL((spira::k_denoise_prepare<T>), dim3(dp.grid_flat), block, 0, st, a);
    int src = 0;
    for (uint32_t it = 0; it < dn->iterations; ++it, src ^= 1) {
        if (it + 1 < dn->iterations) hipLaunchKernelGGL((spira::k_denoise_iter<T, false>), dim3(dp.grid), block, 0, st, a, dp.step(it), src);
        else hipLaunchKernelGGL((spira::k_denoise_iter<T, true>), dim3(dp.grid), block, 0, st, a, dp.step(it), src);
    }
    if (!on_device) {
        if (out_hdr) HIP_TRY(hipMemcpyAsync(out_hdr, a.out_hdr, 3 * npix * sizeof(T), hipMemcpyDeviceToHost, st));
        if (out_img) HIP_TRY(hipMemcpyAsync(out_img, a.out_img, 3 * npix * sizeof(T), hipMemcpyDeviceToHost, st));
    }
    return s.close();
}

template <class T>
int spira_tu::Impl<T>::trace(const T *spheres5, const T *materials8, const T *triangles10, const T *camera12, const spira_params *p,
                             uint32_t n_paths, const uint32_t *ijs, int *prims, T *ts, T *dirs, T *radiance) {
    uint32_t rows = 0;
    if (!p) return fail(SPIRA_E_INVALID, "params is NULL");
    if (int rc = validate_scene<T>(spheres5, materials8, triangles10, p->n_spheres, p->n_materials, triangles10 ? p->n_triangles : 0)) return rc;
    if (int rc = validate_params(camera12, p, triangles10 ? p->n_triangles : 0, &rows)) return rc;
    if (!n_paths || !ijs || !prims || !ts || !dirs || !radiance) return fail(SPIRA_E_INVALID, "NULL argument");
    if (p->max_depth < 1) return fail(SPIRA_E_INVALID, "max_depth must be >= 1");
    if ((p->flags & SPIRA_SEM_MASK) == SPIRA_SEM_HYBRID) return fail(SPIRA_E_UNSUPPORTED, "SPIRA_SEM_HYBRID has no per-path trace (its samples advance image-wide in lock step)");
    for (uint32_t k = 0; k < n_paths; ++k)
        if (ijs[3 * k] < 1 || ijs[3 * k] > p->width || ijs[3 * k + 1] < 1 || ijs[3 * k + 1] > p->height || ijs[3 * k + 2] >= p->spp)
            return fail(SPIRA_E_INVALID, "path (i, j, sample) out of range");
    Session s;
    if (int rc = Session::open(s, false, nullptr)) return rc;
    Ctx &c = *s.cp;
    const hipStream_t st = s.st;
    spira::BounceArgs<T> a{};
    if (int rc = acquire_scene<T>(c, st, (const spira_scene *)nullptr, spheres5, materials8, triangles10, p, a.scene)) return rc;
    if (int rc = attach_spd<T>(c, st, p, a.scene)) return rc;
    fill_const<T>(a.rc, camera12, p, rows, 1);
    size_t nseg = (size_t)n_paths * p->max_depth;
    size_t b_ij = ((size_t)n_paths * 3 * sizeof(uint32_t) + 255) & ~(size_t)255;
    size_t b_pr = (nseg * sizeof(int) + 255) & ~(size_t)255;
    size_t b_ts = (nseg * sizeof(T) + 255) & ~(size_t)255;
    size_t b_di = (nseg * 3 * sizeof(T) + 255) & ~(size_t)255;
    size_t b_ra = ((size_t)n_paths * 3 * sizeof(T) + 255) & ~(size_t)255;
    if (int rc = c.trace.ensure(b_ij + b_pr + b_ts + b_di + b_ra)) return rc;
    char *base = (char *)c.trace.p;
    uint32_t *d_ij = (uint32_t *)base;
    int *d_pr = (int *)(base + b_ij);
    T *d_ts = (T *)(base + b_ij + b_pr);
    T *d_di = (T *)(base + b_ij + b_pr + b_ts);
    T *d_ra = (T *)(base + b_ij + b_pr + b_ts + b_di);
    HIP_TRY(hipMemcpyAsync(d_ij, ijs, (size_t)n_paths * 3 * sizeof(uint32_t), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemsetAsync(d_ts, 0, b_ts + b_di, st));
    const size_t lds = spira::scene_lds_bytes<T>(a.scene.n_spheres, a.scene.n_materials, a.scene.n_triangles);
    const uint32_t sem = p->flags & SPIRA_SEM_MASK;
    const bool ext = (p->flags & (SPIRA_EXT_DIELECTRIC | SPIRA_EXT_SPECTRAL)) != 0;
    const dim3 tg((n_paths + 63) / 64), tb(64);
    int rc;
    if (sem == SPIRA_SEM_CPU) rc = launch_lds(spira::k_trace_variant<T, 1>, tg, tb, lds, st, a, d_ij, n_paths, d_pr, d_ts, d_di, d_ra);
    else if (sem == SPIRA_SEM_METAL) rc = launch_lds(spira::k_trace_variant<T, 2>, tg, tb, lds, st, a, d_ij, n_paths, d_pr, d_ts, d_di, d_ra);
    else if (a.scene.n_bvh_tris) rc = ext ? launch_lds(spira::k_trace<T, true, true>, tg, tb, lds, st, a, d_ij, n_paths, d_pr, d_ts, d_di, d_ra) : launch_lds(spira::k_trace<T, true, false>, tg, tb, lds, st, a, d_ij, n_paths, d_pr, d_ts, d_di, d_ra);
    else rc = ext ? launch_lds(spira::k_trace<T, false, true>, tg, tb, lds, st, a, d_ij, n_paths, d_pr, d_ts, d_di, d_ra) : launch_lds(spira::k_trace<T, false, false>, tg, tb, lds, st, a, d_ij, n_paths, d_pr, d_ts, d_di, d_ra);
    if (rc) return rc;
    HIP_TRY(hipMemcpyAsync(prims, d_pr, nseg * sizeof(int), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(ts, d_ts, nseg * sizeof(T), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(dirs, d_di, nseg * 3 * sizeof(T), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(radiance, d_ra, (size_t)n_paths * 3 * sizeof(T), hipMemcpyDeviceToHost, st));
    return s.close();
}
namespace {

// Camera constructor arithmetic, host side.  Statement order of
// examples/julia-raytracer.jl:280-291 == src/spira-metal-optimized.jl:332-345 (focus_dist = 1).
template <class T> struct HV { T x, y, z; };
template <class T> HV<T> hsub(HV<T> a, HV<T> b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
template <class T> HV<T> hscale(HV<T> a, T s) { return {a.x * s, a.y * s, a.z * s}; }
template <class T> HV<T> hdiv(HV<T> a, T s) { return {a.x / s, a.y / s, a.z / s}; }
template <class T> T hdot(HV<T> a, HV<T> b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
template <class T> HV<T> hcross(HV<T> a, HV<T> b) { return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }
template <class T> HV<T> hnorm(HV<T> a) { return hdiv(a, (T)std::sqrt(hdot(a, a))); }

template <class T>
void camera_impl(const T *position, const T *look_at, const T *up, T fov_deg, T aspect, T focus_dist, T *out12) {
    HV<T> pos{position[0], position[1], position[2]}, la{look_at[0], look_at[1], look_at[2]}, vup{up[0], up[1], up[2]};
    T theta = fov_deg * ((T)3.14159265358979323846 / (T)180);     // deg2rad(z) = z * (oftype(z, pi) / 180)
    T h = std::tan(theta / 2);
    T vh = (T)2.0 * h;
    T vw = aspect * vh;
    HV<T> w = hnorm(hsub(pos, la));
    HV<T> u = hnorm(hcross(vup, w));
    HV<T> v = hcross(w, u);
    HV<T> hor = hscale(u, focus_dist * vw);
    HV<T> ver = hscale(v, focus_dist * vh);
    HV<T> llc = hsub(hsub(hsub(pos, hdiv(hor, (T)2)), hdiv(ver, (T)2)), hscale(w, focus_dist));
    T o[12] = {pos.x, pos.y, pos.z, llc.x, llc.y, llc.z, hor.x, hor.y, hor.z, ver.x, ver.y, ver.z};
    std::memcpy(out12, o, sizeof o);
}

// n_devices == 0: a handle on the calling thread's device; n_devices >= 1: one validated and built ONCE, resident on devices 0 .. n_devices-1
template <class T>
int scene_create(const T *spheres5, const T *materials8, const T *triangles10, uint32_t n_spheres, uint32_t n_materials,
                        uint32_t n_triangles, spira_scene **out, int n_devices = 0) {
    if (!out) return fail(SPIRA_E_INVALID, "out is NULL");
    *out = nullptr;
    const uint32_t nt = triangles10 ? n_triangles : 0;
    if (int rc = validate_scene<T>(spheres5, materials8, triangles10, n_spheres, n_materials, nt)) return rc;
    const bool multi = n_devices > 0;
    if (multi && (n_devices > kMaxDevices || (n_devices > spira_device_count() && !env_u32("SPIRA_MULTI_REHEARSE", 0))))
        return fail(SPIRA_E_INVALID, "n_devices out of range (1 .. spira_device_count())");
    const int caller_device = tl_device;
    const int n_phys = multi ? std::min(n_devices, std::max(1, spira_device_count())) : 1;      // (rehearsal: every rank renders on device 0)
    HostBvh<T> hb;                                      // the mesh's tree: built on the first upload, reused by the others
    spira_scene *first = nullptr;
    int rc = 0;
    for (int d = 0; d < n_phys && !rc; ++d) {
        if (multi) tl_device = d;
        Ctx *cp = nullptr;
        if ((rc = get_ctx(&cp))) break;                // also selects the device
        spira_scene *h = new (std::nothrow) spira_scene();
        if (!h) { rc = fail(SPIRA_E_HIP, "out of host memory"); break; }
        h->magic = kSceneMagic; h->device = tl_device; h->prec = (int)sizeof(T); h->multi = multi;
        if (!first) first = h; else { first->replica[d] = h; }
        rc = scene_upload<T>(h->store, nullptr, nullptr, spheres5, materials8, triangles10, n_spheres, n_materials, nt, &hb);
        if (!rc && hipStreamSynchronize(nullptr) != hipSuccess) rc = fail(SPIRA_E_HIP, "hipStreamSynchronize failed after the scene upload");
        if (!rc) first->n_replicas = d + 1;
    }
    tl_device = caller_device;
    (void)hipSetDevice(caller_device);
    if (rc) {
        const std::string keep = tl_err;
        if (first) {
            for (int d = 1; d < kMaxDevices; ++d) if (first->replica[d]) { (void)hipSetDevice(first->replica[d]->device); first->replica[d]->store.release(); first->replica[d]->magic = 0; delete first->replica[d]; }
            (void)hipSetDevice(first->device); first->store.release(); first->magic = 0; delete first;
            (void)hipSetDevice(caller_device);
        }
        tl_err = keep;
        return rc;
    }
    *out = first;
    return 0;
}


// ======================================================================= multi-device render (one node)
// RCCL is opened at run time: libspira_hip.so has no link-time dependency on it, and when the host process already
// carries an RCCL (PyTorch does) that copy is the one found.
struct Rccl {
    void *handle = nullptr;
    decltype(&ncclCommInitAll) CommInitAll = nullptr;
    decltype(&ncclCommDestroy) CommDestroy = nullptr;
    decltype(&ncclCommAbort) CommAbort = nullptr;
    decltype(&ncclGroupStart) GroupStart = nullptr;
    decltype(&ncclGroupEnd) GroupEnd = nullptr;
    decltype(&ncclSend) Send = nullptr;
    decltype(&ncclRecv) Recv = nullptr;
    decltype(&ncclGetErrorString) GetErrorString = nullptr;
    // one set of communicators per device count ever asked for (devices 0..n-1), kept until spira_shutdown: a host that alternates
    // between, say, 8-GPU frames and 4-GPU previews does not pay ncclCommInitAll (hundreds of ms) at every switch
    bool have[kMaxDevices + 1] = {};
    ncclComm_t comms_of[kMaxDevices + 1][kMaxDevices] = {};
    ncclComm_t *comms = nullptr;         // the set of the current call
    std::mutex mu;
};
Rccl g_rccl;

int rccl_load(Rccl &r) {
    if (r.handle) return 0;
    for (const char *name : {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"}) {
        r.handle = dlopen(name, RTLD_NOW | RTLD_GLOBAL);
        if (r.handle) break;
    }
    if (!r.handle) return fail(SPIRA_E_UNSUPPORTED, std::string("RCCL not found (dlopen librccl.so.1): ") + dlerror());
#define SPIRA_RCCL_SYM(field, sym)                                                        \
    r.field = reinterpret_cast<decltype(r.field)>(dlsym(r.handle, #sym));                \
    if (!r.field) { r.handle = nullptr; return fail(SPIRA_E_UNSUPPORTED, "RCCL symbol missing: " #sym); }
    SPIRA_RCCL_SYM(CommInitAll, ncclCommInitAll)
    SPIRA_RCCL_SYM(CommDestroy, ncclCommDestroy)
    SPIRA_RCCL_SYM(CommAbort, ncclCommAbort)
    SPIRA_RCCL_SYM(GroupStart, ncclGroupStart)
    SPIRA_RCCL_SYM(GroupEnd, ncclGroupEnd)
    SPIRA_RCCL_SYM(Send, ncclSend)
    SPIRA_RCCL_SYM(Recv, ncclRecv)
    SPIRA_RCCL_SYM(GetErrorString, ncclGetErrorString)
#undef SPIRA_RCCL_SYM
    return 0;
}

void rccl_release(Rccl &r) {
    for (int n = 1; n <= kMaxDevices; ++n) {
        if (!r.have[n]) continue;
        for (int i = 0; i < n; ++i) if (r.comms_of[n][i]) { (void)r.CommDestroy(r.comms_of[n][i]); r.comms_of[n][i] = nullptr; }
        r.have[n] = false;
    }
    r.comms = nullptr;
}

// after a failed exchange: the communicators of this device count may hold a half-issued group — abort them, the next call makes new ones
void rccl_abort(Rccl &r, int n) {
    if (!r.have[n]) return;
    for (int i = 0; i < n; ++i) if (r.comms_of[n][i]) { (void)r.CommAbort(r.comms_of[n][i]); r.comms_of[n][i] = nullptr; }
    r.have[n] = false;
    r.comms = nullptr;
}

int rccl_comms(Rccl &r, int n) {          // communicators for devices 0..n-1 (ncclCommInitAll once per n)
    if (int rc = rccl_load(r)) return rc;
    if (!r.have[n]) {
        int devs[kMaxDevices];
        for (int i = 0; i < n; ++i) devs[i] = i;
        ncclResult_t e = r.CommInitAll(r.comms_of[n], n, devs);
        if (e != ncclSuccess) return fail(SPIRA_E_HIP, std::string("ncclCommInitAll: ") + r.GetErrorString(e));
        r.have[n] = true;
    }
    r.comms = r.comms_of[n];
    return 0;
}

// Row permutation of the gathered tiles back to image order, for both outputs at once.
//   stack: [n][2][3][max_rows][W] (tile of rank r: hdr planes, then img planes; rows in the rank's local order)
//   full : [2][3][H][W]
// Global row y belongs to rank (y / stripe_h) % n, local row ((y / stripe_h) / n) * stripe_h + y % stripe_h (spira_params "Tiling").
template <class T>
__global__ void k_assemble(const T *stack, T *full, uint32_t n, uint32_t stripe_h, uint32_t max_rows, uint32_t W, uint32_t H) {
    const size_t total = (size_t)6 * H * W;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const uint32_t x = (uint32_t)(i % W);
        const uint32_t y = (uint32_t)((i / W) % H);
        const uint32_t pl = (uint32_t)(i / ((size_t)W * H));            // 0..5: output * 3 + channel
        const uint32_t sq = y / stripe_h, r = sq % n, lr = (sq / n) * stripe_h + y % stripe_h;
        full[i] = stack[(((size_t)r * 6 + pl) * max_rows + lr) * W + x];
    }
}

constexpr uint32_t kMultiStripeH = 1;      // (single rows: equal tiles whatever the height; 8-row stripes cost a world-8 rank 4 % — distributed.py)

// `mh`: a scene resident on the devices (spira_scene_create_multi_*) — nothing is validated, hashed, built or uploaded per call — or NULL: host arrays
template <class T>
int render_multi_impl(const spira_scene *mh, const T *spheres5, const T *materials8, const T *triangles10, const T *camera12, const spira_params *p, int n_devices,
                      T *out_hdr, T *out_img) {
    if (!p) return fail(SPIRA_E_INVALID, "params is NULL");
    if (!out_hdr && !out_img) return fail(SPIRA_E_INVALID, "both outputs are NULL");
    if (p->rows != 0 || p->stripe_count != 0) return fail(SPIRA_E_INVALID, "spira_render_multi tiles the frame itself: rows / stripe_* must be 0");
    const int avail = spira_device_count();
    // SPIRA_MULTI_REHEARSE=1 (a one-GPU box): all ranks render on device 0 one after the other and their tiles reach the stack by
    // device copies instead of RCCL — exercises tiling, re-pitching and reassembly for any n; not a measurement
    const bool rehearse = env_u32("SPIRA_MULTI_REHEARSE", 0) != 0;
    if (n_devices < 1 || n_devices > kMaxDevices || (!rehearse && n_devices > avail)) return fail(SPIRA_E_INVALID, "n_devices out of range (1 .. spira_device_count())");
    if (avail < 1) return fail(SPIRA_E_NO_DEVICE, "no HIP device");
    // validate once on the calling thread, so that argument errors are reported before any thread or communicator exists
    if (mh) {
        if (mh->magic != kSceneMagic) return fail(SPIRA_E_INVALID, "scene handle is NULL or was destroyed");
        if (mh->prec != (int)sizeof(T)) return fail(SPIRA_E_INVALID, "scene handle was created in the other precision");
        if (mh->device != 0 || (!rehearse && mh->n_replicas < n_devices)) return fail(SPIRA_E_INVALID, "scene handle is not resident on devices 0 .. n_devices-1 (spira_scene_create_multi_*)");
        uint32_t rows = 0;
        if (int rc = validate_params(camera12, p, mh->store.nt, &rows)) return rc;
    } else {
        uint32_t rows = 0;
        const uint32_t nt = triangles10 ? p->n_triangles : 0;
        if (int rc = validate_scene<T>(spheres5, materials8, triangles10, p->n_spheres, p->n_materials, nt)) return rc;
        if (int rc = validate_params(camera12, p, nt, &rows)) return rc;
    }
    const uint32_t n = (uint32_t)n_devices, W = p->width, H = p->height;
    if (stripe_rows(H, kMultiStripeH, n, n - 1) == 0) return fail(SPIRA_E_INVALID, "image has fewer rows than devices");
    const uint32_t max_rows = stripe_rows(H, kMultiStripeH, n, 0);
    const size_t tile_elems = (size_t)6 * max_rows * W;                 // hdr planes + img planes, padded to the largest tile
    std::lock_guard<std::mutex> rl(g_rccl.mu);                           // one multi-device render at a time
    if (!rehearse) { if (int rc = rccl_comms(g_rccl, n_devices)) return rc; }

    std::vector<int> rcs(n, 0);
    std::vector<std::string> errs(n);
    std::atomic<bool> exchange_failed{false};      // (set by any worker thread whose gate reports a failed exchange)
    const int caller_device = tl_device;
    // Every device finishes (or fails) its allocation + render-enqueue phase before any of them enters the exchange: a device that
    // failed early must not leave device 0 waiting on the stream for a tile that will never be sent.
    std::mutex gate_mu;
    std::condition_variable gate_cv;
    uint32_t gate_arrived = 0;
    bool gate_failed = false;
    uint32_t gate_round = 0;
    auto gate = [&](bool ok) -> bool {        // returns whether ALL devices got here without an error (reusable: the exchange has one behind it too)
        std::unique_lock<std::mutex> lk(gate_mu);
        if (!ok) gate_failed = true;
        const uint32_t my_round = gate_round;
        if (++gate_arrived == n) { gate_arrived = 0; ++gate_round; gate_cv.notify_all(); }
        else gate_cv.wait(lk, [&] { return gate_round != my_round; });
        return !gate_failed;
    };
    auto worker = [&](uint32_t r) {
        tl_device = rehearse ? 0 : (int)r;
        auto bail = [&](int rc) { rcs[r] = rc; errs[r] = tl_err; };
        Ctx *cp = nullptr;
        hipStream_t st = nullptr;
        const uint32_t rows_r_all = (n == 1) ? H : stripe_rows(H, kMultiStripeH, n, r);
        auto phase1 = [&]() -> int {          // workspaces + this device's tile, enqueued on its stream
            if (int rc = get_ctx(&cp)) return rc;
            Ctx &c = *cp;
            st = c.stream;
            {
                std::lock_guard<std::recursive_mutex> lock(c.mu);
                if (int rc = c.multi_tile.ensure(2 * tile_elems * sizeof(T))) return rc;      // the tile + a scratch copy for ragged tiles
                if (r == 0 || rehearse) {
                    if (int rc = c.multi_stack.ensure((size_t)n * tile_elems * sizeof(T))) return rc;
                    if (int rc = c.multi_full.ensure((size_t)6 * H * W * sizeof(T))) return rc;
                }
            }
            spira_params tp = *p;
            tp.rows = rows_r_all;
            tp.row0 = 0; tp.stripe_h = kMultiStripeH; tp.stripe_count = n; tp.stripe_rank = r;
            if (n == 1) { tp.rows = 0; tp.stripe_h = 0; tp.stripe_count = 0; tp.stripe_rank = 0; }
            T *d_hdr = (T *)c.multi_tile.p, *d_img = d_hdr + (size_t)3 * max_rows * W;
            // Impl<T>::render writes each output as [3][rows][W] contiguously; the gather wants every tile at the pitch of the largest one
            // ([6][max_rows][W]).  A tile with fewer rows (ragged last stripes) is rendered into the second half of the buffer and its
            // six planes are re-pitched with one strided device copy.
            const spira_scene *hr = !mh ? nullptr : ((rehearse || r == 0) ? mh : mh->replica[r]);
            if (rows_r_all != max_rows) {
                T *scratch = d_hdr + tile_elems;
                if (int rc = render_entry<T>(hr, spheres5, materials8, triangles10, camera12, &tp, scratch, scratch + (size_t)3 * rows_r_all * W, true, st)) return rc;
                hipError_t e = hipMemcpy2DAsync(d_hdr, (size_t)max_rows * W * sizeof(T), scratch, (size_t)rows_r_all * W * sizeof(T), (size_t)rows_r_all * W * sizeof(T), 6,
                                                hipMemcpyDeviceToDevice, st);
                if (e != hipSuccess) return fail(SPIRA_E_HIP, std::string("hipMemcpy2DAsync: ") + hipGetErrorString(e));
                return 0;
            }
            return render_entry<T>(hr, spheres5, materials8, triangles10, camera12, &tp, d_hdr, d_img, true, st);
        };
        const int rc1 = phase1();
        if (rc1) bail(rc1);
        if (!rehearse) { if (!gate(rc1 == 0)) { if (st) (void)hipStreamSynchronize(st); return; } }
        else if (rc1) return;
        Ctx &c = *cp;
        // ---- the one exchange of the path: every tile to device 0 (RCCL point-to-point over xGMI; n-1 transfers arrive at once)
        if (rehearse) {
            hipError_t he = hipMemcpyAsync((T *)c.multi_stack.p + (size_t)r * tile_elems, c.multi_tile.p, tile_elems * sizeof(T), hipMemcpyDeviceToDevice, st);
            if (he != hipSuccess) { tl_err = std::string("hipMemcpyAsync: ") + hipGetErrorString(he); return bail(SPIRA_E_HIP); }
            if (r + 1 < n) return;                 // the last rank assembles
        } else {
        const ncclDataType_t dt = sizeof(T) == 4 ? ncclFloat32 : ncclFloat64;
        ncclResult_t e = g_rccl.GroupStart();
        if (e == ncclSuccess) e = g_rccl.Send(c.multi_tile.p, tile_elems, dt, 0, g_rccl.comms[r], st);
        if (e == ncclSuccess && r == 0)
            for (uint32_t src = 0; src < n && e == ncclSuccess; ++src)
                e = g_rccl.Recv((T *)c.multi_stack.p + (size_t)src * tile_elems, tile_elems, dt, (int)src, g_rccl.comms[0], st);
        ncclResult_t e2 = g_rccl.GroupEnd();
        if (e == ncclSuccess) e = e2;
        if (e != ncclSuccess) { tl_err = std::string("RCCL gather: ") + g_rccl.GetErrorString(e); bail(SPIRA_E_HIP); }
        // A rank whose send could not be issued leaves device 0's receive waiting for ever: every rank learns here whether ALL of them
        // issued their part, and when one did not, nobody synchronises on the exchange — the communicators are aborted after the threads join.
        if (!gate(e == ncclSuccess)) { exchange_failed = true; return; }
        }
        if (rehearse || r == 0) {
            const uint32_t blocks = (uint32_t)std::min<size_t>(((size_t)6 * H * W + 255) / 256, (size_t)c.num_cus * 16);
            hipLaunchKernelGGL((k_assemble<T>), dim3(blocks), dim3(256), 0, st, (const T *)c.multi_stack.p, (T *)c.multi_full.p, n, kMultiStripeH, max_rows, W, H);
            const size_t plane3 = (size_t)3 * H * W * sizeof(T);
            void *const dst[2] = {out_hdr, out_img};
            const void *const src[2] = {c.multi_full.p, (const char *)c.multi_full.p + plane3};
            {
                std::lock_guard<std::recursive_mutex> lock(c.mu);          // (the staging buffer belongs to the context)
                if (int rc = copy_out(c, st, dst, src, plane3)) return bail(rc);
            }
        }
        {
            std::lock_guard<std::recursive_mutex> lock(c.mu);
            if (int rc = mark_done(c, st)) return bail(rc);
        }
        hipError_t he = hipStreamSynchronize(st);
        if (he != hipSuccess) { tl_err = std::string("hipStreamSynchronize: ") + hipGetErrorString(he); return bail(SPIRA_E_HIP); }
    };
    if (rehearse) {
        for (uint32_t r = 0; r < n && !rcs[r ? r - 1 : 0]; ++r) worker(r);
    } else {
        std::vector<std::thread> threads;
        for (uint32_t r = 1; r < n; ++r) threads.emplace_back(worker, r);
        worker(0);                                    // device 0 on the calling thread
        for (auto &t : threads) t.join();
    }
    tl_device = caller_device;
    (void)hipSetDevice(caller_device);
    if (exchange_failed) rccl_abort(g_rccl, n_devices);
    for (uint32_t r = 0; r < n; ++r)
        if (rcs[r]) return fail(rcs[r], "device " + std::to_string(r) + ": " + errs[r]);
    if (exchange_failed) return fail(SPIRA_E_HIP, "RCCL gather failed on another device");
    return 0;
}

}  // namespace

#if !defined(SPIRA_TU_F32) && !defined(SPIRA_TU_F64MESH)
// The part of a rebuild that does not read T: the sort of the (key, index) pairs (a bitonic network on the pairs: equal keys end up in index order, whatever
// the scheduling), the radix tree, its boxes, and the collapse to 8-wide slots in the context's node scratch.  w.keys / w.idx / w.leafbox are filled; on return
// c.lbvh_nodes holds out.n_slots slots without boxes and w.order the triangle order.  ONE synchronisation of `st` per level (the level's three counts);
// refuses (SPIRA_E_LIMIT) a tree of kBvhStack - 2 levels or more and more than 2^24 slots, having written scratch only.
int spira_tu::lbvh_topology(Ctx &c, hipStream_t st, uint32_t n, const LbvhWs &w, LbvhTopo &out) {
    if (n < 2 || n > spira::kBvhMaxTris) return fail(SPIRA_E_LIMIT, "internal: a rebuild needs 2 .. 2^24 triangles");
    const uint32_t n_pad = spira::lbvh_sort_size(n);
    spira::lbvh_sort_schedule(
        n_pad, [&](uint32_t k_first, uint32_t k_last) { hipLaunchKernelGGL(k_lbvh_sort_tile, dim3(n_pad / spira::kLbvhSortTile), dim3(spira::kLbvhSortTile), 0, st, w.keys, w.idx, k_first, k_last); },
        [&](uint32_t j, uint32_t k) { hipLaunchKernelGGL(k_lbvh_sort_wide, dim3(n_pad / kRefitBlock), dim3(kRefitBlock), 0, st, w.keys, w.idx, n_pad, j, k); });
    HIP_TRY(hipGetLastError());
    const uint64_t *keys = w.keys;
    const uint32_t *sorted_idx = w.idx;
    const uint32_t n_inner = n - 1;
    const dim3 blk(kRefitBlock);
    hipLaunchKernelGGL(k_lbvh_radix, dim3((n_inner + kRefitBlock - 1) / kRefitBlock), blk, 0, st, keys, n, w.left, w.right, w.parent, w.counter, w.pending[0]);
    hipLaunchKernelGGL(k_lbvh_boxes, dim3((n + kRefitBlock - 1) / kRefitBlock), blk, 0, st, n, sorted_idx, (const spira::RefitBox *)w.leafbox, (const int32_t *)w.left,
                       (const int32_t *)w.right, (const int32_t *)w.parent, w.counter, w.bbox);
    HIP_TRY(hipGetLastError());
    // the node scratch: n slots to begin with (a host build of n triangles has about n / 2), grown with its contents when a level needs more
    auto reserve = [&](uint32_t need_slots, uint32_t live_slots) -> int {
        const size_t need = (size_t)need_slots * spira::kLbvhNodeDwords * 4 + 128;
        if (need <= c.lbvh_nodes.cap) return 0;
        const size_t cap = std::max(need, 2 * c.lbvh_nodes.cap);
        void *np = nullptr;
        const hipError_t e = hipMalloc(&np, cap);
        if (e != hipSuccess) return fail(SPIRA_E_HIP, std::string("hipMalloc: ") + hipGetErrorString(e));
        if (c.lbvh_nodes.p) {
            if (live_slots) {
                const hipError_t e2 = hipMemcpyAsync(np, c.lbvh_nodes.p, (size_t)live_slots * spira::kLbvhNodeDwords * 4, hipMemcpyDeviceToDevice, st);
                if (e2 != hipSuccess) { (void)hipFree(np); return fail(SPIRA_E_HIP, std::string("hipMemcpyAsync: ") + hipGetErrorString(e2)); }
            }
            c.lbvh_retired.push_back(c.lbvh_nodes.p);      // (the copy may not have run yet: freed by the next rebuild)
        }
        c.lbvh_nodes.p = np; c.lbvh_nodes.cap = cap;
        return 0;
    };
    if (int rc = reserve(n, 0)) return rc;
    LbvhSmall *small = (LbvhSmall *)c.lbvh_small.p;
    uint32_t level_n = 1, slots = 1, n_order = 0;
    int depth = 0, cur = 0;
    out.level_first.assign(1, 0u);
    while (level_n) {
        ++depth;
        if (depth >= spira::kLbvhMaxDepth) return fail(SPIRA_E_LIMIT, "rebuild refused: the tree is too deep for the walk's stack");
        out.level_first.push_back(slots);          // the next level starts with the first block this level hands out (the last level hands out none: n_slots)
        const dim3 lgrid((level_n + kRefitLevelBlock - 1) / kRefitLevelBlock), lblk(kRefitLevelBlock);
        hipLaunchKernelGGL(k_lbvh_make, lgrid, lblk, 0, st, (const spira::LbvhPending *)w.pending[cur], level_n, (const int32_t *)w.left, (const int32_t *)w.right,
                           (const spira::RefitBox *)w.bbox, n_inner, w.made);
        hipLaunchKernelGGL(k_lbvh_scan, dim3(1), dim3(kLbvhScanBlock), 0, st, (const spira::LbvhMade *)w.made, level_n, slots, n_order, w.child_base, w.tri_base, w.next_at,
                           small->totals);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(c.h_lbvh->totals, small->totals, sizeof small->totals, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        const uint32_t new_slots = c.h_lbvh->totals[0], new_order = c.h_lbvh->totals[1], n_next = c.h_lbvh->totals[2];
        if (new_slots > spira::kLbvhMaxSlots) return fail(SPIRA_E_LIMIT, "rebuild refused: more than 2^24 node slots");
        if (new_slots < slots || new_order < n_order || new_order > n || n_next > n_inner || (n_next == 0) != (new_slots == slots))
            return fail(SPIRA_E_LIMIT, "internal: inconsistent level counts in a rebuild");
        if (int rc = reserve(new_slots, slots)) return rc;
        hipLaunchKernelGGL(k_lbvh_write, lgrid, lblk, 0, st, (const spira::LbvhPending *)w.pending[cur], level_n, (const spira::LbvhMade *)w.made, (const uint32_t *)w.child_base,
                           (const uint32_t *)w.tri_base, (const uint32_t *)w.next_at, n_inner, sorted_idx, (uint32_t *)c.lbvh_nodes.p, new_slots, w.order, n, w.pending[cur ^ 1]);
        HIP_TRY(hipGetLastError());
        slots = new_slots; n_order = new_order; level_n = n_next; cur ^= 1;
    }
    if (n_order != n) return fail(SPIRA_E_LIMIT, "internal: a rebuild lost triangles");
    out.n_slots = slots; out.depth = depth;
    return 0;
}
#endif

#ifdef SPIRA_TU_F64MESH
int spira_tu::launch_path_mesh_f64(int R, dim3 grid, size_t lds, hipStream_t st, const spira::PathArgs<double> &a, int spec) {
    if (a.mesh_mode == 1) return launch_path_mode<double, true, 1>(R, grid, lds, st, a, spec);
    return launch_path_mode<double, true, 0>(R, grid, lds, st, a, spec);
}
int spira_tu::launch_path_resume_f64(int R, dim3 grid, size_t lds, hipStream_t st, const spira::PathArgs<double> &a) {
    return launch_path_resume<double>(R, grid, lds, st, a);
}
#elif defined(SPIRA_TU_F32)
template struct spira_tu::Impl<float>;      // every member, and with them every Float32 kernel, is compiled in this unit
#else
// ======================================================================= C ABI (SPIRA_TU_MAIN, or the single translation unit)
extern "C" {

int spira_abi_version(void) { return SPIRA_ABI_VERSION; }
#ifndef SPIRA_BUILD_ID
#define SPIRA_BUILD_ID "unknown"
#endif
const char *spira_build_id(void) { return SPIRA_BUILD_ID; }
const char *spira_last_error(void) { return tl_err.c_str(); }

int spira_device_count(void) {
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess) { tl_err = std::string("hipGetDeviceCount: ") + hipGetErrorString(e); return 0; }
    return n;
}

int spira_set_device(int device) {
    int n = spira_device_count();
    if (device < 0 || device >= n || device >= kMaxDevices) return fail(SPIRA_E_INVALID, "device index out of range");
    tl_device = device;
    return 0;
}

#ifdef SPIRA_MESH_STATS
// experiment builds only (make stats; not part of include/spira_hip.h): the traversal counters of spira_device.h, optionally reset
extern "C" int spira_debug_mesh_stats(unsigned long long *out32, int reset) {
    if (hipDeviceSynchronize() != hipSuccess) return -1;
    if (out32 && hipMemcpyFromSymbol(out32, HIP_SYMBOL(spira::g_mesh_dbg), 32 * sizeof(unsigned long long)) != hipSuccess) return -1;
    if (reset) { unsigned long long z[32] = {0}; if (hipMemcpyToSymbol(HIP_SYMBOL(spira::g_mesh_dbg), z, sizeof z) != hipSuccess) return -1; }
    return 0;
}
#endif

// ---- ray queries on a scene handle (spira_query.h)
int spira_scene_cast_f32(const spira_scene *scene, const float *rays8, uint32_t n_rays, uint32_t flags, int *out_prim, float *out_t, float *out_normal) {
    return spira_tu::Impl<float>::cast(scene, rays8, n_rays, flags, out_prim, out_t, out_normal, nullptr, false, false, nullptr);
}
int spira_scene_cast_f64(const spira_scene *scene, const double *rays8, uint32_t n_rays, uint32_t flags, int *out_prim, double *out_t, double *out_normal) {
    return spira_tu::Impl<double>::cast(scene, rays8, n_rays, flags, out_prim, out_t, out_normal, nullptr, false, false, nullptr);
}
int spira_scene_cast_device_f32(const spira_scene *scene, const float *d_rays8, uint32_t n_rays, uint32_t flags, int *d_out_prim, float *d_out_t, float *d_out_normal, void *stream) {
    return spira_tu::Impl<float>::cast(scene, d_rays8, n_rays, flags, d_out_prim, d_out_t, d_out_normal, nullptr, false, true, stream);
}
int spira_scene_cast_device_f64(const spira_scene *scene, const double *d_rays8, uint32_t n_rays, uint32_t flags, int *d_out_prim, double *d_out_t, double *d_out_normal, void *stream) {
    return spira_tu::Impl<double>::cast(scene, d_rays8, n_rays, flags, d_out_prim, d_out_t, d_out_normal, nullptr, false, true, stream);
}
int spira_scene_occluded_f32(const spira_scene *scene, const float *rays8, uint32_t n_rays, uint32_t flags, uint8_t *out_hit) {
    return spira_tu::Impl<float>::cast(scene, rays8, n_rays, flags, nullptr, nullptr, nullptr, out_hit, true, false, nullptr);
}
int spira_scene_occluded_f64(const spira_scene *scene, const double *rays8, uint32_t n_rays, uint32_t flags, uint8_t *out_hit) {
    return spira_tu::Impl<double>::cast(scene, rays8, n_rays, flags, nullptr, nullptr, nullptr, out_hit, true, false, nullptr);
}
int spira_scene_occluded_device_f32(const spira_scene *scene, const float *d_rays8, uint32_t n_rays, uint32_t flags, uint8_t *d_out_hit, void *stream) {
    return spira_tu::Impl<float>::cast(scene, d_rays8, n_rays, flags, nullptr, nullptr, nullptr, d_out_hit, true, true, stream);
}
int spira_scene_occluded_device_f64(const spira_scene *scene, const double *d_rays8, uint32_t n_rays, uint32_t flags, uint8_t *d_out_hit, void *stream) {
    return spira_tu::Impl<double>::cast(scene, d_rays8, n_rays, flags, nullptr, nullptr, nullptr, d_out_hit, true, true, stream);
}
// ---- multi-hit ray queries (spira_hits.h)
int spira_scene_cast_hits_f32(const spira_scene *scene, const float *rays8, uint32_t n_rays, uint32_t max_hits, uint32_t flags, int *out_prim, float *out_t, uint32_t *out_count) {
    return spira_tu::Impl<float>::hits(scene, rays8, n_rays, max_hits, flags, out_prim, out_t, out_count, false, nullptr);
}
int spira_scene_cast_hits_f64(const spira_scene *scene, const double *rays8, uint32_t n_rays, uint32_t max_hits, uint32_t flags, int *out_prim, double *out_t, uint32_t *out_count) {
    return spira_tu::Impl<double>::hits(scene, rays8, n_rays, max_hits, flags, out_prim, out_t, out_count, false, nullptr);
}
int spira_scene_cast_hits_device_f32(const spira_scene *scene, const float *d_rays8, uint32_t n_rays, uint32_t max_hits, uint32_t flags, int *d_out_prim, float *d_out_t,
                                     uint32_t *d_out_count, void *stream) {
    return spira_tu::Impl<float>::hits(scene, d_rays8, n_rays, max_hits, flags, d_out_prim, d_out_t, d_out_count, true, stream);
}
int spira_scene_cast_hits_device_f64(const spira_scene *scene, const double *d_rays8, uint32_t n_rays, uint32_t max_hits, uint32_t flags, int *d_out_prim, double *d_out_t,
                                     uint32_t *d_out_count, void *stream) {
    return spira_tu::Impl<double>::hits(scene, d_rays8, n_rays, max_hits, flags, d_out_prim, d_out_t, d_out_count, true, stream);
}
// Test support, outside the ABI like spira_debug_scene_tree: the launch plan a cast of n_rays would get on a device of num_cus CUs, with the knobs of the
// environment as the entries read them.  out8: grid, wpb, waves, base, rem, refill_free, grid_flat, kCastMinRaysPerWave.  No device needed.
int spira_debug_cast_plan(uint32_t n_rays, uint32_t num_cus, uint32_t *out8) {
    if (!out8 || n_rays == 0 || n_rays > SPIRA_MAX_RAYS) return fail(SPIRA_E_INVALID, "spira_debug_cast_plan: out8 is NULL or n_rays outside 1 .. SPIRA_MAX_RAYS");
    const spira::CastPlan cp = spira::make_cast_plan(n_rays, num_cus, spira::kBlock, read_cast_knobs());
    const uint32_t v[8] = {cp.grid, cp.wpb, cp.waves, cp.base, cp.rem, cp.refill_free, cp.grid_flat, spira::kCastMinRaysPerWave};
    std::memcpy(out8, v, sizeof v);
    return 0;
}

// ---- closest-point queries on a scene handle (spira_nearest.h)
int spira_scene_closest_point_f32(const spira_scene *scene, const float *points4, uint32_t n_points, uint32_t flags, int *out_prim, float *out_dist, float *out_point,
                                  uint32_t *out_trips) {
    return spira_tu::Impl<float>::nearest(scene, points4, n_points, flags, out_prim, out_dist, out_point, out_trips, false, nullptr);
}
int spira_scene_closest_point_f64(const spira_scene *scene, const double *points4, uint32_t n_points, uint32_t flags, int *out_prim, double *out_dist, double *out_point,
                                  uint32_t *out_trips) {
    return spira_tu::Impl<double>::nearest(scene, points4, n_points, flags, out_prim, out_dist, out_point, out_trips, false, nullptr);
}
int spira_scene_closest_point_device_f32(const spira_scene *scene, const float *d_points4, uint32_t n_points, uint32_t flags, int *d_out_prim, float *d_out_dist,
                                         float *d_out_point, uint32_t *d_out_trips, void *stream) {
    return spira_tu::Impl<float>::nearest(scene, d_points4, n_points, flags, d_out_prim, d_out_dist, d_out_point, d_out_trips, true, stream);
}
int spira_scene_closest_point_device_f64(const spira_scene *scene, const double *d_points4, uint32_t n_points, uint32_t flags, int *d_out_prim, double *d_out_dist,
                                         double *d_out_point, uint32_t *d_out_trips, void *stream) {
    return spira_tu::Impl<double>::nearest(scene, d_points4, n_points, flags, d_out_prim, d_out_dist, d_out_point, d_out_trips, true, stream);
}
// ---- K-nearest point queries (spira_knearest.h)
int spira_scene_nearest_k_f32(const spira_scene *scene, const float *points4, uint32_t n_points, uint32_t max_near, uint32_t flags, int *out_prim, float *out_dist,
                              float *out_point, uint32_t *out_count, uint32_t *out_trips) {
    return spira_tu::Impl<float>::nearest_k(scene, points4, n_points, max_near, flags, out_prim, out_dist, out_point, out_count, out_trips, false, nullptr);
}
int spira_scene_nearest_k_f64(const spira_scene *scene, const double *points4, uint32_t n_points, uint32_t max_near, uint32_t flags, int *out_prim, double *out_dist,
                              double *out_point, uint32_t *out_count, uint32_t *out_trips) {
    return spira_tu::Impl<double>::nearest_k(scene, points4, n_points, max_near, flags, out_prim, out_dist, out_point, out_count, out_trips, false, nullptr);
}
int spira_scene_nearest_k_device_f32(const spira_scene *scene, const float *d_points4, uint32_t n_points, uint32_t max_near, uint32_t flags, int *d_out_prim,
                                     float *d_out_dist, float *d_out_point, uint32_t *d_out_count, uint32_t *d_out_trips, void *stream) {
    return spira_tu::Impl<float>::nearest_k(scene, d_points4, n_points, max_near, flags, d_out_prim, d_out_dist, d_out_point, d_out_count, d_out_trips, true, stream);
}
int spira_scene_nearest_k_device_f64(const spira_scene *scene, const double *d_points4, uint32_t n_points, uint32_t max_near, uint32_t flags, int *d_out_prim,
                                     double *d_out_dist, double *d_out_point, uint32_t *d_out_count, uint32_t *d_out_trips, void *stream) {
    return spira_tu::Impl<double>::nearest_k(scene, d_points4, n_points, max_near, flags, d_out_prim, d_out_dist, d_out_point, d_out_count, d_out_trips, true, stream);
}
// host arithmetic, no device: the triangle function the kernels and the scan call
void spira_closest_point_triangle_f32(const float v0[3], const float e1[3], const float e2[3], const float p[3], float out_q[3], float *out_d2) {
    float q[3], d2;
    spira::closest_point_triangle<float>(v0, e1, e2, p, q, d2);
    if (out_q) { out_q[0] = q[0]; out_q[1] = q[1]; out_q[2] = q[2]; }
    if (out_d2) *out_d2 = d2;
}
void spira_closest_point_triangle_f64(const double v0[3], const double e1[3], const double e2[3], const double p[3], double out_q[3], double *out_d2) {
    double q[3], d2;
    spira::closest_point_triangle<double>(v0, e1, e2, p, q, d2);
    if (out_q) { out_q[0] = q[0]; out_q[1] = q[1]; out_q[2] = q[2]; }
    if (out_d2) *out_d2 = d2;
}

// ---- sphere sweeps on a scene handle (spira_sweep.h)
int spira_scene_sweep_f32(const spira_scene *scene, const float *rays8, const float *radii, uint32_t n, uint32_t flags, int *out_prim, float *out_t, float *out_point,
                          float *out_normal, uint32_t *out_trips) {
    return spira_tu::Impl<float>::sweep(scene, rays8, radii, n, flags, out_prim, out_t, out_point, out_normal, nullptr, out_trips, false, false, nullptr);
}
int spira_scene_sweep_device_f32(const spira_scene *scene, const float *d_rays8, const float *d_radii, uint32_t n, uint32_t flags, int *d_out_prim, float *d_out_t,
                                 float *d_out_point, float *d_out_normal, uint32_t *d_out_trips, void *stream) {
    return spira_tu::Impl<float>::sweep(scene, d_rays8, d_radii, n, flags, d_out_prim, d_out_t, d_out_point, d_out_normal, nullptr, d_out_trips, false, true, stream);
}
int spira_scene_sweep_blocked_f32(const spira_scene *scene, const float *rays8, const float *radii, uint32_t n, uint32_t flags, uint8_t *out_hit) {
    return spira_tu::Impl<float>::sweep(scene, rays8, radii, n, flags, nullptr, nullptr, nullptr, nullptr, out_hit, nullptr, true, false, nullptr);
}
int spira_scene_sweep_blocked_device_f32(const spira_scene *scene, const float *d_rays8, const float *d_radii, uint32_t n, uint32_t flags, uint8_t *d_out_hit, void *stream) {
    return spira_tu::Impl<float>::sweep(scene, d_rays8, d_radii, n, flags, nullptr, nullptr, nullptr, nullptr, d_out_hit, nullptr, true, true, stream);
}
// host arithmetic, no device: the leaf function the kernels and the scan call, with bound = t_max.  A miss: t = t_max copied, q 0.
void spira_sweep_sphere_triangle_f32(const float v0[3], const float e1[3], const float e2[3], const float o[3], const float d_unit[3], float r, float t_min, float t_max,
                                     float *out_t, float out_q[3], int *out_hit) {
    float t, q[3] = {0, 0, 0};
    const bool hit = spira::sweep_sphere_triangle<float>(v0, e1, e2, o, d_unit, r, t_min, t_max, t, q);
    if (out_t) *out_t = hit ? t : t_max;
    if (out_q) { out_q[0] = hit ? q[0] : 0; out_q[1] = hit ? q[1] : 0; out_q[2] = hit ? q[2] : 0; }
    if (out_hit) *out_hit = hit ? 1 : 0;
}
int spira_scene_sweep_f64(const spira_scene *scene, const double *rays8, const double *radii, uint32_t n, uint32_t flags, int *out_prim, double *out_t, double *out_point,
                          double *out_normal, uint32_t *out_trips) {
    return spira_tu::Impl<double>::sweep(scene, rays8, radii, n, flags, out_prim, out_t, out_point, out_normal, nullptr, out_trips, false, false, nullptr);
}
int spira_scene_sweep_device_f64(const spira_scene *scene, const double *d_rays8, const double *d_radii, uint32_t n, uint32_t flags, int *d_out_prim, double *d_out_t,
                                 double *d_out_point, double *d_out_normal, uint32_t *d_out_trips, void *stream) {
    return spira_tu::Impl<double>::sweep(scene, d_rays8, d_radii, n, flags, d_out_prim, d_out_t, d_out_point, d_out_normal, nullptr, d_out_trips, false, true, stream);
}
int spira_scene_sweep_blocked_f64(const spira_scene *scene, const double *rays8, const double *radii, uint32_t n, uint32_t flags, uint8_t *out_hit) {
    return spira_tu::Impl<double>::sweep(scene, rays8, radii, n, flags, nullptr, nullptr, nullptr, nullptr, out_hit, nullptr, true, false, nullptr);
}
int spira_scene_sweep_blocked_device_f64(const spira_scene *scene, const double *d_rays8, const double *d_radii, uint32_t n, uint32_t flags, uint8_t *d_out_hit, void *stream) {
    return spira_tu::Impl<double>::sweep(scene, d_rays8, d_radii, n, flags, nullptr, nullptr, nullptr, nullptr, d_out_hit, nullptr, true, true, stream);
}
// host arithmetic, no device: the leaf function the kernels and the scan call, with bound = t_max.  A miss: t = t_max copied, q 0.
void spira_sweep_sphere_triangle_f64(const double v0[3], const double e1[3], const double e2[3], const double o[3], const double d_unit[3], double r, double t_min, double t_max,
                                     double *out_t, double out_q[3], int *out_hit) {
    double t, q[3] = {0, 0, 0};
    const bool hit = spira::sweep_sphere_triangle<double>(v0, e1, e2, o, d_unit, r, t_min, t_max, t, q);
    if (out_t) *out_t = hit ? t : t_max;
    if (out_q) { out_q[0] = hit ? q[0] : 0; out_q[1] = hit ? q[1] : 0; out_q[2] = hit ? q[2] : 0; }
    if (out_hit) *out_hit = hit ? 1 : 0;
}

// ---- box overlap queries on a scene handle (spira_overlap.h)
int spira_scene_overlap_box_f32(const spira_scene *scene, const float *boxes10, uint32_t n, uint32_t max_list, uint32_t flags, int *out_prim, uint32_t *out_count,
                                uint32_t *out_trips) {
    return spira_tu::Impl<float>::overlap(scene, boxes10, n, max_list, flags, out_prim, out_count, nullptr, out_trips, false, false, nullptr);
}
int spira_scene_overlap_box_device_f32(const spira_scene *scene, const float *d_boxes10, uint32_t n, uint32_t max_list, uint32_t flags, int *d_out_prim, uint32_t *d_out_count,
                                       uint32_t *d_out_trips, void *stream) {
    return spira_tu::Impl<float>::overlap(scene, d_boxes10, n, max_list, flags, d_out_prim, d_out_count, nullptr, d_out_trips, false, true, stream);
}
int spira_scene_overlap_any_f32(const spira_scene *scene, const float *boxes10, uint32_t n, uint32_t flags, uint8_t *out_hit) {
    return spira_tu::Impl<float>::overlap(scene, boxes10, n, 0u, flags, nullptr, nullptr, out_hit, nullptr, true, false, nullptr);
}
int spira_scene_overlap_any_device_f32(const spira_scene *scene, const float *d_boxes10, uint32_t n, uint32_t flags, uint8_t *d_out_hit, void *stream) {
    return spira_tu::Impl<float>::overlap(scene, d_boxes10, n, 0u, flags, nullptr, nullptr, d_out_hit, nullptr, true, true, stream);
}
int spira_scene_overlap_box_f64(const spira_scene *scene, const double *boxes10, uint32_t n, uint32_t max_list, uint32_t flags, int *out_prim, uint32_t *out_count,
                                uint32_t *out_trips) {
    return spira_tu::Impl<double>::overlap(scene, boxes10, n, max_list, flags, out_prim, out_count, nullptr, out_trips, false, false, nullptr);
}
int spira_scene_overlap_box_device_f64(const spira_scene *scene, const double *d_boxes10, uint32_t n, uint32_t max_list, uint32_t flags, int *d_out_prim, uint32_t *d_out_count,
                                       uint32_t *d_out_trips, void *stream) {
    return spira_tu::Impl<double>::overlap(scene, d_boxes10, n, max_list, flags, d_out_prim, d_out_count, nullptr, d_out_trips, false, true, stream);
}
int spira_scene_overlap_any_f64(const spira_scene *scene, const double *boxes10, uint32_t n, uint32_t flags, uint8_t *out_hit) {
    return spira_tu::Impl<double>::overlap(scene, boxes10, n, 0u, flags, nullptr, nullptr, out_hit, nullptr, true, false, nullptr);
}
int spira_scene_overlap_any_device_f64(const spira_scene *scene, const double *d_boxes10, uint32_t n, uint32_t flags, uint8_t *d_out_hit, void *stream) {
    return spira_tu::Impl<double>::overlap(scene, d_boxes10, n, 0u, flags, nullptr, nullptr, d_out_hit, nullptr, true, true, stream);
}
// host arithmetic, no device: the leaf functions the kernels and the scan call, on a box prepared without a frame.  SPIRA_RAY_INVALID: the box is invalid.
int spira_overlap_box_triangle_f32(const float v0[3], const float e1[3], const float e2[3], const float box10[10]) {
    spira::OverlapBox<float> B; float He[3];
    if (!spira::overlap_prepare<float>(box10, false, nullptr, B, He)) return SPIRA_RAY_INVALID;
    return spira::overlap_box_triangle<float>(B, v0, e1, e2) ? 1 : 0;
}
int spira_overlap_box_triangle_f64(const double v0[3], const double e1[3], const double e2[3], const double box10[10]) {
    spira::OverlapBox<double> B; double He[3];
    if (!spira::overlap_prepare<double>(box10, false, nullptr, B, He)) return SPIRA_RAY_INVALID;
    return spira::overlap_box_triangle<double>(B, v0, e1, e2) ? 1 : 0;
}
int spira_overlap_box_sphere_f32(const float centre[3], float radius, const float box10[10]) {
    spira::OverlapBox<float> B; float He[3];
    if (!spira::overlap_prepare<float>(box10, false, nullptr, B, He)) return SPIRA_RAY_INVALID;
    return spira::overlap_box_sphere<float>(B, centre, radius) ? 1 : 0;
}
int spira_overlap_box_sphere_f64(const double centre[3], double radius, const double box10[10]) {
    spira::OverlapBox<double> B; double He[3];
    if (!spira::overlap_prepare<double>(box10, false, nullptr, B, He)) return SPIRA_RAY_INVALID;
    return spira::overlap_box_sphere<double>(B, centre, radius) ? 1 : 0;
}

// ---- triangle overlap queries on a scene handle (spira_trioverlap.h)
int spira_scene_overlap_tri_f32(const spira_scene *scene, const float *triangles10, uint32_t n, uint32_t max_list, uint32_t flags, int *out_prim, uint32_t *out_count,
                                uint32_t *out_trips) {
    return spira_tu::Impl<float>::overlap_tri(scene, triangles10, n, max_list, flags, out_prim, out_count, nullptr, out_trips, false, false, nullptr);
}
int spira_scene_overlap_tri_device_f32(const spira_scene *scene, const float *d_triangles10, uint32_t n, uint32_t max_list, uint32_t flags, int *d_out_prim,
                                       uint32_t *d_out_count, uint32_t *d_out_trips, void *stream) {
    return spira_tu::Impl<float>::overlap_tri(scene, d_triangles10, n, max_list, flags, d_out_prim, d_out_count, nullptr, d_out_trips, false, true, stream);
}
int spira_scene_overlap_tri_any_f32(const spira_scene *scene, const float *triangles10, uint32_t n, uint32_t flags, uint8_t *out_hit) {
    return spira_tu::Impl<float>::overlap_tri(scene, triangles10, n, 0u, flags, nullptr, nullptr, out_hit, nullptr, true, false, nullptr);
}
int spira_scene_overlap_tri_any_device_f32(const spira_scene *scene, const float *d_triangles10, uint32_t n, uint32_t flags, uint8_t *d_out_hit, void *stream) {
    return spira_tu::Impl<float>::overlap_tri(scene, d_triangles10, n, 0u, flags, nullptr, nullptr, d_out_hit, nullptr, true, true, stream);
}
int spira_scene_overlap_tri_f64(const spira_scene *scene, const double *triangles10, uint32_t n, uint32_t max_list, uint32_t flags, int *out_prim, uint32_t *out_count,
                                uint32_t *out_trips) {
    return spira_tu::Impl<double>::overlap_tri(scene, triangles10, n, max_list, flags, out_prim, out_count, nullptr, out_trips, false, false, nullptr);
}
int spira_scene_overlap_tri_device_f64(const spira_scene *scene, const double *d_triangles10, uint32_t n, uint32_t max_list, uint32_t flags, int *d_out_prim,
                                       uint32_t *d_out_count, uint32_t *d_out_trips, void *stream) {
    return spira_tu::Impl<double>::overlap_tri(scene, d_triangles10, n, max_list, flags, d_out_prim, d_out_count, nullptr, d_out_trips, false, true, stream);
}
int spira_scene_overlap_tri_any_f64(const spira_scene *scene, const double *triangles10, uint32_t n, uint32_t flags, uint8_t *out_hit) {
    return spira_tu::Impl<double>::overlap_tri(scene, triangles10, n, 0u, flags, nullptr, nullptr, out_hit, nullptr, true, false, nullptr);
}
int spira_scene_overlap_tri_any_device_f64(const spira_scene *scene, const double *d_triangles10, uint32_t n, uint32_t flags, uint8_t *d_out_hit, void *stream) {
    return spira_tu::Impl<double>::overlap_tri(scene, d_triangles10, n, 0u, flags, nullptr, nullptr, d_out_hit, nullptr, true, true, stream);
}
// the leaf functions as host arithmetic: the same inline functions the kernels call, compiled for the host
int spira_overlap_tri_triangle_f32(const float v0[3], const float e1[3], const float e2[3], const float query10[10]) {
    spira::TriQuery<float> Q;
    if (!spira::trioverlap_prepare<float>(query10, false, nullptr, Q)) return SPIRA_RAY_INVALID;
    return spira::overlap_tri_triangle<float>(Q, v0, e1, e2) ? 1 : 0;
}
int spira_overlap_tri_triangle_f64(const double v0[3], const double e1[3], const double e2[3], const double query10[10]) {
    spira::TriQuery<double> Q;
    if (!spira::trioverlap_prepare<double>(query10, false, nullptr, Q)) return SPIRA_RAY_INVALID;
    return spira::overlap_tri_triangle<double>(Q, v0, e1, e2) ? 1 : 0;
}
int spira_overlap_tri_sphere_f32(const float centre[3], float radius, const float query10[10]) {
    spira::TriQuery<float> Q;
    if (!spira::trioverlap_prepare<float>(query10, false, nullptr, Q)) return SPIRA_RAY_INVALID;
    return spira::overlap_tri_sphere<float>(Q, centre, radius) ? 1 : 0;
}
int spira_overlap_tri_sphere_f64(const double centre[3], double radius, const double query10[10]) {
    spira::TriQuery<double> Q;
    if (!spira::trioverlap_prepare<double>(query10, false, nullptr, Q)) return SPIRA_RAY_INVALID;
    return spira::overlap_tri_sphere<double>(Q, centre, radius) ? 1 : 0;
}

// ---- signed distance queries on a scene handle (spira_sdf.h)
int spira_scene_signed_distance_f32(const spira_scene *scene, const float *points4, uint32_t n_points, uint32_t flags, int *out_prim, float *out_dist, float *out_point,
                                    uint8_t *out_inside, uint32_t *out_crossings, uint32_t *out_trips) {
    return spira_tu::Impl<float>::signed_distance(scene, points4, n_points, flags, out_prim, out_dist, out_point, out_inside, out_crossings, out_trips, false, nullptr);
}
int spira_scene_signed_distance_device_f32(const spira_scene *scene, const float *d_points4, uint32_t n_points, uint32_t flags, int *d_out_prim, float *d_out_dist,
                                           float *d_out_point, uint8_t *d_out_inside, uint32_t *d_out_crossings, uint32_t *d_out_trips, void *stream) {
    return spira_tu::Impl<float>::signed_distance(scene, d_points4, n_points, flags, d_out_prim, d_out_dist, d_out_point, d_out_inside, d_out_crossings, d_out_trips, true, stream);
}
int spira_scene_signed_distance_f64(const spira_scene *scene, const double *points4, uint32_t n_points, uint32_t flags, int *out_prim, double *out_dist, double *out_point,
                                    uint8_t *out_inside, uint32_t *out_crossings, uint32_t *out_trips) {
    return spira_tu::Impl<double>::signed_distance(scene, points4, n_points, flags, out_prim, out_dist, out_point, out_inside, out_crossings, out_trips, false, nullptr);
}
int spira_scene_signed_distance_device_f64(const spira_scene *scene, const double *d_points4, uint32_t n_points, uint32_t flags, int *d_out_prim, double *d_out_dist,
                                           double *d_out_point, uint8_t *d_out_inside, uint32_t *d_out_crossings, uint32_t *d_out_trips, void *stream) {
    return spira_tu::Impl<double>::signed_distance(scene, d_points4, n_points, flags, d_out_prim, d_out_dist, d_out_point, d_out_inside, d_out_crossings, d_out_trips, true, stream);
}

// ---- radiance along the caller's rays, and the camera ray generator (spira_radiance.h)
int spira_scene_radiance_f32(const spira_scene *scene, const float *rays6, uint32_t n_rays, const spira_radiance *rp, float *sum_rgb, uint8_t *out_valid) {
    return spira_tu::Impl<float>::radiance(scene, rays6, n_rays, rp, sum_rgb, out_valid, false, nullptr);
}
int spira_scene_radiance_f64(const spira_scene *scene, const double *rays6, uint32_t n_rays, const spira_radiance *rp, double *sum_rgb, uint8_t *out_valid) {
    return spira_tu::Impl<double>::radiance(scene, rays6, n_rays, rp, sum_rgb, out_valid, false, nullptr);
}
int spira_scene_radiance_device_f32(const spira_scene *scene, const float *d_rays6, uint32_t n_rays, const spira_radiance *rp, float *d_sum_rgb, uint8_t *d_out_valid, void *stream) {
    return spira_tu::Impl<float>::radiance(scene, d_rays6, n_rays, rp, d_sum_rgb, d_out_valid, true, stream);
}
int spira_scene_radiance_device_f64(const spira_scene *scene, const double *d_rays6, uint32_t n_rays, const spira_radiance *rp, double *d_sum_rgb, uint8_t *d_out_valid, void *stream) {
    return spira_tu::Impl<double>::radiance(scene, d_rays6, n_rays, rp, d_sum_rgb, d_out_valid, true, stream);
}
int spira_camera_rays_f32(const float camera12[12], const spira_lens *lens, float *rays6) { return spira_tu::Impl<float>::camera_rays(camera12, lens, rays6, false, nullptr); }
int spira_camera_rays_f64(const double camera12[12], const spira_lens *lens, double *rays6) { return spira_tu::Impl<double>::camera_rays(camera12, lens, rays6, false, nullptr); }
int spira_camera_rays_device_f32(const float camera12[12], const spira_lens *lens, float *d_rays6, void *stream) { return spira_tu::Impl<float>::camera_rays(camera12, lens, d_rays6, true, stream); }
int spira_camera_rays_device_f64(const double camera12[12], const spira_lens *lens, double *d_rays6, void *stream) { return spira_tu::Impl<double>::camera_rays(camera12, lens, d_rays6, true, stream); }
// Test support, outside the ABI like spira_debug_cast_plan: the plan a radiance call of n_rays x spp gets on a device of num_cus CUs, with the knobs of the
// environment as the entries read them.  out8: grid, wpb, spp_pass, n_pass, direct, workspace entries (low, high word), the item cap.  No device needed.
int spira_debug_radiance_plan(uint32_t n_rays, uint32_t spp, uint32_t num_cus, uint32_t *out8) {
    if (!out8 || n_rays == 0 || n_rays > SPIRA_MAX_RAYS || spp == 0 || spp > SPIRA_MAX_SPP)
        return fail(SPIRA_E_INVALID, "spira_debug_radiance_plan: out8 is NULL, n_rays outside 1 .. SPIRA_MAX_RAYS or spp outside 1 .. SPIRA_MAX_SPP");
    const spira::RadiancePlan pl = spira::make_radiance_plan(n_rays, spp, num_cus, spira::kBlock, read_radiance_knobs());
    const uint32_t v[8] = {pl.grid, pl.wpb, pl.spp_pass, pl.n_pass, pl.direct ? 1u : 0u, (uint32_t)pl.ws_entries, (uint32_t)(pl.ws_entries >> 32), pl.max_items};
    std::memcpy(out8, v, sizeof v);
    return 0;
}

// ---- hemisphere gather at surface points (spira_gather.h)
int spira_gather_rays_f32(const float *points6, uint32_t n_points, uint32_t sample, uint64_t seed, uint32_t key0, float *rays6) {
    return spira_tu::Impl<float>::gather_rays(points6, n_points, sample, seed, key0, rays6, false, nullptr);
}
int spira_gather_rays_f64(const double *points6, uint32_t n_points, uint32_t sample, uint64_t seed, uint32_t key0, double *rays6) {
    return spira_tu::Impl<double>::gather_rays(points6, n_points, sample, seed, key0, rays6, false, nullptr);
}
int spira_gather_rays_device_f32(const float *d_points6, uint32_t n_points, uint32_t sample, uint64_t seed, uint32_t key0, float *d_rays6, void *stream) {
    return spira_tu::Impl<float>::gather_rays(d_points6, n_points, sample, seed, key0, d_rays6, true, stream);
}
int spira_gather_rays_device_f64(const double *d_points6, uint32_t n_points, uint32_t sample, uint64_t seed, uint32_t key0, double *d_rays6, void *stream) {
    return spira_tu::Impl<double>::gather_rays(d_points6, n_points, sample, seed, key0, d_rays6, true, stream);
}
int spira_scene_gather_f32(const spira_scene *scene, const float *points6, uint32_t n_points, const spira_radiance *rp, float *sum_rgb, uint8_t *out_valid) {
    return spira_tu::Impl<float>::gather(scene, points6, n_points, rp, sum_rgb, out_valid, false, nullptr);
}
int spira_scene_gather_f64(const spira_scene *scene, const double *points6, uint32_t n_points, const spira_radiance *rp, double *sum_rgb, uint8_t *out_valid) {
    return spira_tu::Impl<double>::gather(scene, points6, n_points, rp, sum_rgb, out_valid, false, nullptr);
}
int spira_scene_gather_device_f32(const spira_scene *scene, const float *d_points6, uint32_t n_points, const spira_radiance *rp, float *d_sum_rgb, uint8_t *d_out_valid, void *stream) {
    return spira_tu::Impl<float>::gather(scene, d_points6, n_points, rp, d_sum_rgb, d_out_valid, true, stream);
}
int spira_scene_gather_device_f64(const spira_scene *scene, const double *d_points6, uint32_t n_points, const spira_radiance *rp, double *d_sum_rgb, uint8_t *d_out_valid, void *stream) {
    return spira_tu::Impl<double>::gather(scene, d_points6, n_points, rp, d_sum_rgb, d_out_valid, true, stream);
}
int spira_scene_gather_visible_f32(const spira_scene *scene, const float *points6, uint32_t n_points, const spira_gather_visible *gv, uint32_t *visible_u32, uint8_t *out_valid) {
    return spira_tu::Impl<float>::gather_visible(scene, points6, n_points, gv, visible_u32, out_valid, false, nullptr);
}
int spira_scene_gather_visible_f64(const spira_scene *scene, const double *points6, uint32_t n_points, const spira_gather_visible *gv, uint32_t *visible_u32, uint8_t *out_valid) {
    return spira_tu::Impl<double>::gather_visible(scene, points6, n_points, gv, visible_u32, out_valid, false, nullptr);
}
int spira_scene_gather_visible_device_f32(const spira_scene *scene, const float *d_points6, uint32_t n_points, const spira_gather_visible *gv, uint32_t *d_visible_u32,
                                          uint8_t *d_out_valid, void *stream) {
    return spira_tu::Impl<float>::gather_visible(scene, d_points6, n_points, gv, d_visible_u32, d_out_valid, true, stream);
}
int spira_scene_gather_visible_device_f64(const spira_scene *scene, const double *d_points6, uint32_t n_points, const spira_gather_visible *gv, uint32_t *d_visible_u32,
                                          uint8_t *d_out_valid, void *stream) {
    return spira_tu::Impl<double>::gather_visible(scene, d_points6, n_points, gv, d_visible_u32, d_out_valid, true, stream);
}
// ---- light probes (spira_probe.h)
int spira_probe_rays_f32(const float *points3, uint32_t n_points, uint32_t sample, uint64_t seed, uint32_t key0, float *rays6) {
    return spira_tu::Impl<float>::probe_rays(points3, n_points, sample, seed, key0, rays6, false, nullptr);
}
int spira_probe_rays_f64(const double *points3, uint32_t n_points, uint32_t sample, uint64_t seed, uint32_t key0, double *rays6) {
    return spira_tu::Impl<double>::probe_rays(points3, n_points, sample, seed, key0, rays6, false, nullptr);
}
int spira_probe_rays_device_f32(const float *d_points3, uint32_t n_points, uint32_t sample, uint64_t seed, uint32_t key0, float *d_rays6, void *stream) {
    return spira_tu::Impl<float>::probe_rays(d_points3, n_points, sample, seed, key0, d_rays6, true, stream);
}
int spira_probe_rays_device_f64(const double *d_points3, uint32_t n_points, uint32_t sample, uint64_t seed, uint32_t key0, double *d_rays6, void *stream) {
    return spira_tu::Impl<double>::probe_rays(d_points3, n_points, sample, seed, key0, d_rays6, true, stream);
}
int spira_scene_probe_sh_f32(const spira_scene *scene, const float *points3, uint32_t n_points, const spira_radiance *rp, float *sum_sh, uint8_t *out_valid) {
    return spira_tu::Impl<float>::probe_sh(scene, points3, n_points, rp, sum_sh, out_valid, false, nullptr);
}
int spira_scene_probe_sh_f64(const spira_scene *scene, const double *points3, uint32_t n_points, const spira_radiance *rp, double *sum_sh, uint8_t *out_valid) {
    return spira_tu::Impl<double>::probe_sh(scene, points3, n_points, rp, sum_sh, out_valid, false, nullptr);
}
int spira_scene_probe_sh_device_f32(const spira_scene *scene, const float *d_points3, uint32_t n_points, const spira_radiance *rp, float *d_sum_sh, uint8_t *d_out_valid, void *stream) {
    return spira_tu::Impl<float>::probe_sh(scene, d_points3, n_points, rp, d_sum_sh, d_out_valid, true, stream);
}
int spira_scene_probe_sh_device_f64(const spira_scene *scene, const double *d_points3, uint32_t n_points, const spira_radiance *rp, double *d_sum_sh, uint8_t *d_out_valid, void *stream) {
    return spira_tu::Impl<double>::probe_sh(scene, d_points3, n_points, rp, d_sum_sh, d_out_valid, true, stream);
}
void spira_sh9_basis_f32(const float d_unit[3], float out9[9]) { spira::sh9_basis<float>(d_unit, out9); }
void spira_sh9_basis_f64(const double d_unit[3], double out9[9]) { spira::sh9_basis<double>(d_unit, out9); }
// Test support, outside the ABI like spira_debug_radiance_plan: the plan a gather of n_points x spp gets on a device of num_cus CUs, with the knobs of the
// environment as the entries read them.  out8: grid, wpb, spp_pass, n_pass, direct, workspace entries (low, high word), the item cap.  No device needed.
int spira_debug_gather_plan(uint32_t n_points, uint32_t spp, uint32_t num_cus, uint32_t *out8) {
    if (!out8 || n_points == 0 || n_points > SPIRA_MAX_RAYS || spp == 0 || spp > SPIRA_MAX_SPP)
        return fail(SPIRA_E_INVALID, "spira_debug_gather_plan: out8 is NULL, n_points outside 1 .. SPIRA_MAX_RAYS or spp outside 1 .. SPIRA_MAX_SPP");
    const spira::GatherPlan pl = spira::make_gather_plan(n_points, spp, num_cus, spira::kBlock, read_gather_knobs());
    const uint32_t v[8] = {pl.grid, pl.wpb, pl.spp_pass, pl.n_pass, pl.direct ? 1u : 0u, (uint32_t)pl.ws_entries, (uint32_t)(pl.ws_entries >> 32), pl.max_items};
    std::memcpy(out8, v, sizeof v);
    return 0;
}

// Test support, always compiled but outside the ABI (not in include/spira_hip.h; tests/test_gpu_tree_bytes.py finds it by name): a single-device handle's
// tree as it lies on the device, to be compared byte for byte with the host twin of tests/native/tree_twin.h.  `what`:
//   0  summary: uint32 precision (4 / 8), n, bvh_slots, bvh_depth; double bvh_centre[3], bvh_scale; uint32 level_first[0 .. depth]
//   1  the node array: bvh_slots * 20 dwords
//   2  the three frame packets and the triangle records: (3 + 3 n) packets of four T
//   3  the Float32 screening records, 3 n packets of four floats (0 bytes where the store has none)
// Takes the context's lock and waits for the device to be idle — so it comes after a device-form update or rebuild on whatever stream — then copies.
// *need_bytes is written whenever the handle is accepted; nothing is copied unless cap_bytes suffices (SPIRA_E_INVALID).  Reads only.
int spira_debug_scene_tree(const spira_scene *scene, uint32_t what, void *out, uint64_t cap_bytes, uint64_t *need_bytes) {
    if (need_bytes) *need_bytes = 0;
    if (!scene || scene->magic != kSceneMagic) return fail(SPIRA_E_INVALID, "scene handle is NULL or was destroyed");
    if (!need_bytes) return fail(SPIRA_E_INVALID, "need_bytes is NULL");
    if (what > 3u) return fail(SPIRA_E_INVALID, "what: 0 summary, 1 nodes, 2 frame packets and triangle records, 3 screening records");
    if (scene->multi) return fail(SPIRA_E_UNSUPPORTED, "spira_debug_scene_tree does not take a handle made by spira_scene_create_multi_*");
    if (scene->device != tl_device) return fail(SPIRA_E_INVALID, "scene handle belongs to another device (spira_set_device)");
    const SceneStore &s = scene->store;
    if (s.nt <= SPIRA_LDS_TRIANGLES) return fail(SPIRA_E_INVALID, "the handle's mesh has no tree (at most SPIRA_LDS_TRIANGLES triangles)");
    const size_t depth = (size_t)s.bvh_depth;
    if (s.bvh_prec != scene->prec || s.bvh_n != s.nt || s.bvh_depth < 1 || s.bvh_level_first.size() != depth + 1 || !s.bvh_nodes.p || !s.bvh_tris.p)
        return fail(SPIRA_E_LIMIT, "internal: the handle's tree has no consistent level table");
    Ctx *cp = nullptr;
    if (int rc = get_ctx(&cp)) return rc;
    std::lock_guard<std::recursive_mutex> lock(cp->mu);
    HIP_TRY(hipDeviceSynchronize());
    const size_t packet = 4 * (size_t)scene->prec;
    if (what == 0u) {
        const uint32_t head[4] = {(uint32_t)scene->prec, s.nt, s.bvh_slots, (uint32_t)s.bvh_depth};
        const double fr[4] = {s.bvh_centre[0], s.bvh_centre[1], s.bvh_centre[2], s.bvh_scale};
        const size_t need = sizeof head + sizeof fr + (depth + 1) * sizeof(uint32_t);
        *need_bytes = need;
        if (!out || cap_bytes < need) return fail(SPIRA_E_INVALID, "out is NULL or cap_bytes is too small (see *need_bytes)");
        char *o = (char *)out;
        std::memcpy(o, head, sizeof head); std::memcpy(o + sizeof head, fr, sizeof fr);
        std::memcpy(o + sizeof head + sizeof fr, s.bvh_level_first.data(), (depth + 1) * sizeof(uint32_t));
        return 0;
    }
    const void *src = what == 1u ? s.bvh_nodes.p : what == 2u ? s.bvh_tris.p : s.bvh_tris32.p;
    const size_t need = what == 1u ? (size_t)s.bvh_slots * spira::kLbvhNodeDwords * sizeof(uint32_t)
                      : what == 2u ? (3 + 3 * (size_t)s.nt) * packet
                                   : (s.bvh_tris32.p ? 3 * (size_t)s.nt * 4 * sizeof(float) : 0);
    *need_bytes = need;
    if (need == 0) return 0;
    if (!out || cap_bytes < need) return fail(SPIRA_E_INVALID, "out is NULL or cap_bytes is too small (see *need_bytes)");
    const DevBuf &b = what == 1u ? s.bvh_nodes : what == 2u ? s.bvh_tris : s.bvh_tris32;
    if (need > b.cap) return fail(SPIRA_E_LIMIT, "internal: the handle's buffer is smaller than its tree");
    HIP_TRY(hipMemcpy(out, src, need, hipMemcpyDeviceToHost));
    return 0;
}

int spira_get_counters(spira_counters *out) {
    if (!out) return fail(SPIRA_E_INVALID, "out is NULL");
    Ctx *cp = nullptr;
    if (int rc = get_ctx(&cp)) return rc;
    Ctx &c = *cp;
    std::lock_guard<std::recursive_mutex> lock(c.mu);
    if (!c.last_valid) return fail(SPIRA_E_INVALID, "no render has run on this device");
    if (c.last_pending) {
        HIP_TRY(hipEventSynchronize(c.ev_stop));
        HIP_TRY(hipStreamSynchronize(c.last_stream));
        float ms = 0;
        HIP_TRY(hipEventElapsedTime(&ms, c.ev_start, c.ev_stop));
        c.last.kernel_ms = ms;
        c.last.segments = c.h_stats->segments;
        c.last.rays_enqueued = c.h_stats->rays_enqueued;
        c.last.radiance_rmw = c.h_stats->radiance_rmw;
        c.last.radiance_stores = c.h_stats->radiance_store;
        c.last.redone_waves = c.h_stats->redone_waves;
        c.last.rays_parked = c.h_stats->rays_parked;
        c.last.mesh_wave_trips = c.h_stats->mesh_wave_trips;
        c.last.mesh_lane_trips = c.h_stats->mesh_lane_trips;
        c.last_sky_pixels = c.h_stats->sky_pixels;
        double wms = 0;
        for (size_t i = 0; i < c.ev_mid_used; ++i) {
            float m = 0;
            HIP_TRY(hipEventElapsedTime(&m, c.ev_mid[i], c.ev_pool[c.ev_mid_end[i]]));
            wms += m;
        }
        c.last.walk_kernel_ms = wms;
        double bms = 0;
        for (size_t i = 0; i + 1 < c.ev_used; i += 2) {
            float m = 0;
            HIP_TRY(hipEventElapsedTime(&m, c.ev_pool[i], c.ev_pool[i + 1]));
            bms += m;
        }
        c.last.bounce_kernel_ms = bms;
        c.last_pending = false;
    }
    *out = c.last;
    return 0;
}

int spira_get_sky_pixels(uint64_t *out) {
    if (!out) return fail(SPIRA_E_INVALID, "out is NULL");
    spira_counters unused;
    if (int rc = spira_get_counters(&unused)) return rc;      // (waits for the render and reads its device counters back)
    Ctx *cp = nullptr;
    if (int rc = get_ctx(&cp)) return rc;
    std::lock_guard<std::recursive_mutex> lock(cp->mu);
    *out = cp->last_sky_pixels;
    return 0;
}

int spira_get_own_passes(uint64_t *out) {
    if (!out) return fail(SPIRA_E_INVALID, "out is NULL");
    Ctx *cp = nullptr;
    if (int rc = get_ctx(&cp)) return rc;
    std::lock_guard<std::recursive_mutex> lock(cp->mu);
    if (!cp->last_valid) return fail(SPIRA_E_INVALID, "no render has run on this device");
    *out = cp->last_own_passes;
    return 0;
}

void spira_shutdown(void) {
    { std::lock_guard<std::mutex> rl(g_rccl.mu); if (g_rccl.handle) rccl_release(g_rccl); }
    for (int d = 0; d < kMaxDevices; ++d) {
        Ctx &c = g_ctx[d];
        std::lock_guard<std::recursive_mutex> lock(c.mu);
        if (!c.init) continue;
        (void)hipSetDevice(d);
        (void)hipDeviceSynchronize();
        c.release_all(); c.scene.release();
        if (c.h_ad_count) { (void)hipHostFree(c.h_ad_count); c.h_ad_count = nullptr; }
        if (c.h_refit_status) { (void)hipHostFree(c.h_refit_status); c.h_refit_status = nullptr; }
        for (void *q : c.lbvh_retired) (void)hipFree(q);
        c.lbvh_retired.clear();
        if (c.h_lbvh) { (void)hipHostFree(c.h_lbvh); c.h_lbvh = nullptr; }
        for (hipEvent_t e : c.ev_pool) (void)hipEventDestroy(e);
        c.ev_pool.clear();
        for (hipEvent_t e : c.ev_mid) (void)hipEventDestroy(e);
        c.ev_mid.clear(); c.ev_mid_end.clear(); c.ev_mid_used = 0;
        (void)hipEventDestroy(c.ev_start); (void)hipEventDestroy(c.ev_stop); (void)hipEventDestroy(c.ev_done);
        c.have_done = false;
        (void)hipHostFree(c.h_stats);
        if (c.h_stage) { (void)hipHostFree(c.h_stage); c.h_stage = nullptr; c.h_stage_cap = 0; }
        for (hipEvent_t e : c.stage_ev) (void)hipEventDestroy(e);
        c.stage_ev.clear();
        (void)hipStreamDestroy(c.stream);
        if (c.copy_stream) { (void)hipStreamDestroy(c.copy_stream); c.copy_stream = nullptr; }
        if (c.ev_slab) { (void)hipEventDestroy(c.ev_slab); c.ev_slab = nullptr; }
        c.init = false; c.last_valid = false;
    }
}

int spira_camera_lookat_f32(const float lookfrom[3], const float lookat[3], const float vup[3], float vfov_deg, float aspect_ratio,
                            float out12[12]) {
    if (!lookfrom || !lookat || !vup || !out12) return fail(SPIRA_E_INVALID, "NULL argument");
    camera_impl<float>(lookfrom, lookat, vup, vfov_deg, aspect_ratio, 1.0f, out12);
    return 0;
}
int spira_camera_lookat_f64(const double position[3], const double look_at[3], const double up[3], double fov_deg, double aspect_ratio,
                            double focus_dist, double out12[12]) {
    if (!position || !look_at || !up || !out12) return fail(SPIRA_E_INVALID, "NULL argument");
    camera_impl<double>(position, look_at, up, fov_deg, aspect_ratio, focus_dist, out12);
    return 0;
}

int spira_render_f32(const float *s, const float *m, const float *t, const float cam[12], const spira_params *p, float *out_hdr, float *out_img) {
    return render_entry<float>(nullptr, s, m, t, cam, p, out_hdr, out_img, false, nullptr);
}
int spira_render_f64(const double *s, const double *m, const double *t, const double cam[12], const spira_params *p, double *out_hdr, double *out_img) {
    return render_entry<double>(nullptr, s, m, t, cam, p, out_hdr, out_img, false, nullptr);
}
int spira_render_device_f32(const float *s, const float *m, const float *t, const float cam[12], const spira_params *p, float *d_hdr,
                            float *d_img, void *stream) {
    return render_entry<float>(nullptr, s, m, t, cam, p, d_hdr, d_img, true, stream);
}
int spira_render_device_f64(const double *s, const double *m, const double *t, const double cam[12], const spira_params *p, double *d_hdr,
                            double *d_img, void *stream) {
    return render_entry<double>(nullptr, s, m, t, cam, p, d_hdr, d_img, true, stream);
}

int spira_accumulate_f32(const float *s, const float *m, const float *t, const float cam[12], const spira_params *p, uint32_t sample0,
                         float *sum_rgb, uint32_t *rng_states) {
    if (!sum_rgb) return fail(SPIRA_E_INVALID, "sum_rgb is NULL");
    return render_entry<float>(nullptr, s, m, t, cam, p, sum_rgb, nullptr, false, nullptr, true, sample0, rng_states);
}
int spira_accumulate_f64(const double *s, const double *m, const double *t, const double cam[12], const spira_params *p, uint32_t sample0,
                         double *sum_rgb, uint32_t *rng_states) {
    if (!sum_rgb) return fail(SPIRA_E_INVALID, "sum_rgb is NULL");
    return render_entry<double>(nullptr, s, m, t, cam, p, sum_rgb, nullptr, false, nullptr, true, sample0, rng_states);
}
int spira_accumulate_device_f32(const float *s, const float *m, const float *t, const float cam[12], const spira_params *p, uint32_t sample0,
                                float *d_sum_rgb, uint32_t *d_rng_states, void *stream) {
    if (!d_sum_rgb) return fail(SPIRA_E_INVALID, "d_sum_rgb is NULL");
    return render_entry<float>(nullptr, s, m, t, cam, p, d_sum_rgb, nullptr, true, stream, true, sample0, d_rng_states);
}
int spira_accumulate_device_f64(const double *s, const double *m, const double *t, const double cam[12], const spira_params *p, uint32_t sample0,
                                double *d_sum_rgb, uint32_t *d_rng_states, void *stream) {
    if (!d_sum_rgb) return fail(SPIRA_E_INVALID, "d_sum_rgb is NULL");
    return render_entry<double>(nullptr, s, m, t, cam, p, d_sum_rgb, nullptr, true, stream, true, sample0, d_rng_states);
}

// ---- scene handles: validate + build + upload once, render many times
int spira_scene_create_f32(const float *spheres5, const float *materials8, const float *triangles10, uint32_t n_spheres, uint32_t n_materials,
                           uint32_t n_triangles, spira_scene **out) {
    return scene_create<float>(spheres5, materials8, triangles10, n_spheres, n_materials, n_triangles, out);
}
int spira_scene_create_f64(const double *spheres5, const double *materials8, const double *triangles10, uint32_t n_spheres, uint32_t n_materials,
                           uint32_t n_triangles, spira_scene **out) {
    return scene_create<double>(spheres5, materials8, triangles10, n_spheres, n_materials, n_triangles, out);
}
int spira_scene_create_multi_f32(const float *spheres5, const float *materials8, const float *triangles10, uint32_t n_spheres, uint32_t n_materials,
                                 uint32_t n_triangles, int n_devices, spira_scene **out) {
    if (n_devices < 1) return fail(SPIRA_E_INVALID, "n_devices out of range (1 .. spira_device_count())");
    return scene_create<float>(spheres5, materials8, triangles10, n_spheres, n_materials, n_triangles, out, n_devices);
}
int spira_scene_create_multi_f64(const double *spheres5, const double *materials8, const double *triangles10, uint32_t n_spheres, uint32_t n_materials,
                                 uint32_t n_triangles, int n_devices, spira_scene **out) {
    if (n_devices < 1) return fail(SPIRA_E_INVALID, "n_devices out of range (1 .. spira_device_count())");
    return scene_create<double>(spheres5, materials8, triangles10, n_spheres, n_materials, n_triangles, out, n_devices);
}
int spira_render_multi_scene_f32(const spira_scene *scene, const float cam[12], const spira_params *p, int n_devices, float *out_hdr, float *out_img) {
    if (!scene) return fail(SPIRA_E_INVALID, "scene handle is NULL or was destroyed");
    return render_multi_impl<float>(scene, nullptr, nullptr, nullptr, cam, p, n_devices, out_hdr, out_img);
}
int spira_render_multi_scene_f64(const spira_scene *scene, const double cam[12], const spira_params *p, int n_devices, double *out_hdr, double *out_img) {
    if (!scene) return fail(SPIRA_E_INVALID, "scene handle is NULL or was destroyed");
    return render_multi_impl<double>(scene, nullptr, nullptr, nullptr, cam, p, n_devices, out_hdr, out_img);
}
int spira_scene_destroy(spira_scene *scene) {
    if (!scene) return 0;
    if (scene->magic != kSceneMagic) return fail(SPIRA_E_INVALID, "scene handle was already destroyed");
    for (int d = kMaxDevices - 1; d >= 0; --d) {           // the replicas of a multi-device handle first, then the handle itself
        spira_scene *h = d ? scene->replica[d] : scene;
        if (!h) continue;
        if (hipSetDevice(h->device) != hipSuccess) return fail(SPIRA_E_HIP, "hipSetDevice failed");
        h->store.release();                                // hipFree waits for work that still reads the buffers
        h->magic = 0;
        delete h;
    }
    (void)hipSetDevice(tl_device);
    return 0;
}
// ---- new contents for a live handle (host arrays, NULL = unchanged; a device triangle array on the caller's stream): the tree is refitted, not rebuilt
int spira_scene_update_f32(spira_scene *scene, const float *spheres5, const float *materials8, const float *triangles10) {
    return spira_tu::Impl<float>::scene_update(scene, spheres5, materials8, triangles10, nullptr, false, nullptr);
}
int spira_scene_update_f64(spira_scene *scene, const double *spheres5, const double *materials8, const double *triangles10) {
    return spira_tu::Impl<double>::scene_update(scene, spheres5, materials8, triangles10, nullptr, false, nullptr);
}
int spira_scene_update_device_f32(spira_scene *scene, const float *d_triangles10, void *stream) {
    return spira_tu::Impl<float>::scene_update(scene, nullptr, nullptr, nullptr, d_triangles10, true, stream);
}
int spira_scene_update_device_f64(spira_scene *scene, const double *d_triangles10, void *stream) {
    return spira_tu::Impl<double>::scene_update(scene, nullptr, nullptr, nullptr, d_triangles10, true, stream);
}
// ---- a new triangle array for a live handle, the tree built anew on the device: a new frame, a new topology, no frame rule
int spira_scene_rebuild_f32(spira_scene *scene, const float *triangles10) { return spira_tu::Impl<float>::scene_rebuild(scene, triangles10, nullptr, false, nullptr); }
int spira_scene_rebuild_f64(spira_scene *scene, const double *triangles10) { return spira_tu::Impl<double>::scene_rebuild(scene, triangles10, nullptr, false, nullptr); }
int spira_scene_rebuild_device_f32(spira_scene *scene, const float *d_triangles10, void *stream) { return spira_tu::Impl<float>::scene_rebuild(scene, nullptr, d_triangles10, true, stream); }
int spira_scene_rebuild_device_f64(spira_scene *scene, const double *d_triangles10, void *stream) { return spira_tu::Impl<double>::scene_rebuild(scene, nullptr, d_triangles10, true, stream); }
int spira_render_scene_f32(const spira_scene *scene, const float cam[12], const spira_params *p, float *out_hdr, float *out_img) {
    if (!scene) return fail(SPIRA_E_INVALID, "scene handle is NULL or was destroyed");
    return render_entry<float>(scene, nullptr, nullptr, nullptr, cam, p, out_hdr, out_img, false, nullptr);
}
int spira_render_scene_f64(const spira_scene *scene, const double cam[12], const spira_params *p, double *out_hdr, double *out_img) {
    if (!scene) return fail(SPIRA_E_INVALID, "scene handle is NULL or was destroyed");
    return render_entry<double>(scene, nullptr, nullptr, nullptr, cam, p, out_hdr, out_img, false, nullptr);
}
int spira_render_scene_device_f32(const spira_scene *scene, const float cam[12], const spira_params *p, float *d_hdr, float *d_img, void *stream) {
    if (!scene) return fail(SPIRA_E_INVALID, "scene handle is NULL or was destroyed");
    return render_entry<float>(scene, nullptr, nullptr, nullptr, cam, p, d_hdr, d_img, true, stream);
}
int spira_render_scene_device_f64(const spira_scene *scene, const double cam[12], const spira_params *p, double *d_hdr, double *d_img, void *stream) {
    if (!scene) return fail(SPIRA_E_INVALID, "scene handle is NULL or was destroyed");
    return render_entry<double>(scene, nullptr, nullptr, nullptr, cam, p, d_hdr, d_img, true, stream);
}

// ---- adaptive sampling: render to a noise target (host arrays; a handle; a handle and device outputs on the caller's stream)
int spira_render_adaptive_f32(const float *s, const float *m, const float *t, const float cam[12], const spira_params *p, const spira_adaptive *adaptive,
                              float *out_hdr, float *out_img, uint32_t *out_spp, float *out_q) {
    return spira_tu::Impl<float>::render_adaptive(nullptr, s, m, t, cam, p, adaptive, out_hdr, out_img, out_spp, out_q, false, nullptr);
}
int spira_render_adaptive_f64(const double *s, const double *m, const double *t, const double cam[12], const spira_params *p, const spira_adaptive *adaptive,
                              double *out_hdr, double *out_img, uint32_t *out_spp, double *out_q) {
    return spira_tu::Impl<double>::render_adaptive(nullptr, s, m, t, cam, p, adaptive, out_hdr, out_img, out_spp, out_q, false, nullptr);
}
int spira_render_adaptive_scene_f32(const spira_scene *scene, const float cam[12], const spira_params *p, const spira_adaptive *adaptive,
                                    float *out_hdr, float *out_img, uint32_t *out_spp, float *out_q) {
    if (!scene) return fail(SPIRA_E_INVALID, "scene handle is NULL or was destroyed");
    return spira_tu::Impl<float>::render_adaptive(scene, nullptr, nullptr, nullptr, cam, p, adaptive, out_hdr, out_img, out_spp, out_q, false, nullptr);
}
int spira_render_adaptive_scene_f64(const spira_scene *scene, const double cam[12], const spira_params *p, const spira_adaptive *adaptive,
                                    double *out_hdr, double *out_img, uint32_t *out_spp, double *out_q) {
    if (!scene) return fail(SPIRA_E_INVALID, "scene handle is NULL or was destroyed");
    return spira_tu::Impl<double>::render_adaptive(scene, nullptr, nullptr, nullptr, cam, p, adaptive, out_hdr, out_img, out_spp, out_q, false, nullptr);
}
int spira_render_adaptive_scene_device_f32(const spira_scene *scene, const float cam[12], const spira_params *p, const spira_adaptive *adaptive,
                                           float *d_hdr, float *d_img, uint32_t *d_spp, float *d_q, void *stream) {
    if (!scene) return fail(SPIRA_E_INVALID, "scene handle is NULL or was destroyed");
    return spira_tu::Impl<float>::render_adaptive(scene, nullptr, nullptr, nullptr, cam, p, adaptive, d_hdr, d_img, d_spp, d_q, true, stream);
}
int spira_render_adaptive_scene_device_f64(const spira_scene *scene, const double cam[12], const spira_params *p, const spira_adaptive *adaptive,
                                           double *d_hdr, double *d_img, uint32_t *d_spp, double *d_q, void *stream) {
    if (!scene) return fail(SPIRA_E_INVALID, "scene handle is NULL or was destroyed");
    return spira_tu::Impl<double>::render_adaptive(scene, nullptr, nullptr, nullptr, cam, p, adaptive, d_hdr, d_img, d_spp, d_q, true, stream);
}
int spira_sky_pixel_f64(const double cam[12], uint32_t width, uint32_t height, uint32_t i, uint32_t j, const double *spheres5, uint32_t n_spheres) {
    if (!cam || (n_spheres && !spheres5)) return fail(SPIRA_E_INVALID, "cam or spheres5 is NULL");
    return spira::sky_pixel(cam, width, height, i, j, spheres5, n_spheres) ? 1 : 0;
}
int spira_pixel_reach_f64(const double cam[12], uint32_t width, uint32_t height, uint32_t i, uint32_t j, const double *spheres5, uint32_t n_spheres, uint32_t *out_mask) {
    if (!cam || !out_mask || (n_spheres && !spheres5)) return fail(SPIRA_E_INVALID, "cam, out_mask or spheres5 is NULL");
    *out_mask = spira::pixel_reach(cam, width, height, i, j, spheres5, n_spheres);
    return 0;
}
int spira_adaptive_converged_f32(const float sum3[3], float q, uint32_t n, double tolerance, double floor) {
    return adaptive_converged_host<float>(sum3, q, n, tolerance, floor);
}
int spira_adaptive_converged_f64(const double sum3[3], double q, uint32_t n, double tolerance, double floor) {
    return adaptive_converged_host<double>(sum3, q, n, tolerance, floor);
}

// ---- first-hit feature buffers (host arrays; a handle; a handle and device outputs on the caller's stream)
int spira_render_features_f32(const float *s, const float *m, const float *t, const float cam[12], const spira_params *p,
                              float *out_albedo, float *out_normal, float *out_depth) {
    return spira_tu::Impl<float>::features(nullptr, s, m, t, cam, p, out_albedo, out_normal, out_depth, false, nullptr);
}
int spira_render_features_f64(const double *s, const double *m, const double *t, const double cam[12], const spira_params *p,
                              double *out_albedo, double *out_normal, double *out_depth) {
    return spira_tu::Impl<double>::features(nullptr, s, m, t, cam, p, out_albedo, out_normal, out_depth, false, nullptr);
}
int spira_render_features_scene_f32(const spira_scene *scene, const float cam[12], const spira_params *p, float *out_albedo, float *out_normal, float *out_depth) {
    if (!scene) return fail(SPIRA_E_INVALID, "scene handle is NULL or was destroyed");
    return spira_tu::Impl<float>::features(scene, nullptr, nullptr, nullptr, cam, p, out_albedo, out_normal, out_depth, false, nullptr);
}
int spira_render_features_scene_f64(const spira_scene *scene, const double cam[12], const spira_params *p, double *out_albedo, double *out_normal, double *out_depth) {
    if (!scene) return fail(SPIRA_E_INVALID, "scene handle is NULL or was destroyed");
    return spira_tu::Impl<double>::features(scene, nullptr, nullptr, nullptr, cam, p, out_albedo, out_normal, out_depth, false, nullptr);
}
int spira_render_features_scene_device_f32(const spira_scene *scene, const float cam[12], const spira_params *p,
                                           float *d_albedo, float *d_normal, float *d_depth, void *stream) {
    if (!scene) return fail(SPIRA_E_INVALID, "scene handle is NULL or was destroyed");
    return spira_tu::Impl<float>::features(scene, nullptr, nullptr, nullptr, cam, p, d_albedo, d_normal, d_depth, true, stream);
}
int spira_render_features_scene_device_f64(const spira_scene *scene, const double cam[12], const spira_params *p,
                                           double *d_albedo, double *d_normal, double *d_depth, void *stream) {
    if (!scene) return fail(SPIRA_E_INVALID, "scene handle is NULL or was destroyed");
    return spira_tu::Impl<double>::features(scene, nullptr, nullptr, nullptr, cam, p, d_albedo, d_normal, d_depth, true, stream);
}

// ---- the a-trous denoiser (host planes; device planes on the caller's stream)
int spira_denoise_f32(const float *color, const float *variance, const float *albedo, const float *normal, const float *depth, const spira_denoise *dn,
                      float *out_hdr, float *out_img) {
    return spira_tu::Impl<float>::denoise(color, variance, albedo, normal, depth, dn, out_hdr, out_img, false, nullptr);
}
int spira_denoise_f64(const double *color, const double *variance, const double *albedo, const double *normal, const double *depth, const spira_denoise *dn,
                      double *out_hdr, double *out_img) {
    return spira_tu::Impl<double>::denoise(color, variance, albedo, normal, depth, dn, out_hdr, out_img, false, nullptr);
}
int spira_denoise_device_f32(const float *d_color, const float *d_variance, const float *d_albedo, const float *d_normal, const float *d_depth, const spira_denoise *dn,
                             float *d_out_hdr, float *d_out_img, void *stream) {
    return spira_tu::Impl<float>::denoise(d_color, d_variance, d_albedo, d_normal, d_depth, dn, d_out_hdr, d_out_img, true, stream);
}
int spira_denoise_device_f64(const double *d_color, const double *d_variance, const double *d_albedo, const double *d_normal, const double *d_depth, const spira_denoise *dn,
                             double *d_out_hdr, double *d_out_img, void *stream) {
    return spira_tu::Impl<double>::denoise(d_color, d_variance, d_albedo, d_normal, d_depth, dn, d_out_hdr, d_out_img, true, stream);
}

// ---- multi-device render on one node: interleaved 8-row stripes, one host thread + stream per device, one RCCL gather
int spira_render_multi_f32(const float *s, const float *m, const float *t, const float cam[12], const spira_params *p, int n_devices,
                           float *out_hdr, float *out_img) {
    return render_multi_impl<float>(nullptr, s, m, t, cam, p, n_devices, out_hdr, out_img);
}
int spira_render_multi_f64(const double *s, const double *m, const double *t, const double cam[12], const spira_params *p, int n_devices,
                           double *out_hdr, double *out_img) {
    return render_multi_impl<double>(nullptr, s, m, t, cam, p, n_devices, out_hdr, out_img);
}

int spira_trace_paths_f32(const float *s, const float *m, const float *t, const float cam[12], const spira_params *p, uint32_t n_paths,
                          const uint32_t *ijs, int *prims, float *ts, float *dirs, float *radiance) {
    return spira_tu::Impl<float>::trace(s, m, t, cam, p, n_paths, ijs, prims, ts, dirs, radiance);
}
int spira_trace_paths_f64(const double *s, const double *m, const double *t, const double cam[12], const spira_params *p, uint32_t n_paths,
                          const uint32_t *ijs, int *prims, double *ts, double *dirs, double *radiance) {
    return spira_tu::Impl<double>::trace(s, m, t, cam, p, n_paths, ijs, prims, ts, dirs, radiance);
}

int spira_tonemap_f32(float *values, uint64_t n, uint32_t post) {
    if (!values && n) return fail(SPIRA_E_INVALID, "values is NULL");
    post &= SPIRA_POST_MASK;
    for (uint64_t i = 0; i < n; ++i) values[i] = spira::post1<float>(values[i], post);
    return 0;
}

uint32_t spira_stripe_rows(uint32_t height, uint32_t stripe_h, uint32_t stripe_count, uint32_t stripe_rank) {
    if (stripe_count == 0 || stripe_rank >= stripe_count) return 0;
    return stripe_rows(height, stripe_h, stripe_count, stripe_rank);
}

}  // extern "C"
#endif  // SPIRA_TU_MAIN, or the single translation unit
