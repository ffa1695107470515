// spira_plan.h — the launch plan of a render call: organisation, pass split, launch geometry and the size of every workspace, as pure integer
// arithmetic on the call's parameters (no HIP headers, no getenv: also built into the sanitizer harness tests/native/host_sanitize.cpp, which sweeps
// it under ASan + UBSan).  spira_hip.hip fills PlanIn — the constants of spira_device.h and the SPIRA_* knobs included — sizes the context's
// workspaces from Plan::ws and hands the plan to the organisation's enqueue function; verify_path_args() takes path_need() for its numbers.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>

#include "../../include/spira_hip.h"

namespace spira {

// Every SPIRA_* environment value the plan and the k_path arguments depend on (read once per call by spira_hip.hip, read_knobs: defaults and clamps there).
struct Knobs {
    uint32_t batch_rays = 160u << 20;          // SPIRA_BATCH_RAYS: rays per pass where spira_params::batch_rays is 0
    uint32_t R = 2;                            // SPIRA_R: rays per lane (1 or 2)
    uint32_t blocks_per_cu = 0;                // SPIRA_BLOCKS_PER_CU; 0: the organisation's own (make_plan)
    uint32_t defer_mesh = 1, mesh_two_pass = 1, fused_resolve = 1, private_l = 1;
    uint32_t spec_div = 1;                     // SPIRA_SPEC_DIV: 0 off, 1 where the scene's scale allows, 2 report every wave, 3 on whatever the scale
    uint32_t dense_pct = 70, mesh_min_batch = 128, mesh_refill = 16, mesh_fat_waves_per_cu = 16, cam_consts = 1;
    uint32_t sky_runs = 1;                     // SPIRA_SKY_RUNS: pixel-owning passes sum their all-sky runs ahead of the loop (0: every path goes through it; A/B, tests)
    uint32_t pixel_table = 1;                  // SPIRA_PIXEL_TABLE: their camera rows read pixel, i, j and the two inner key hashes from a per-wave LDS table (0: path_of and the mixes per path)
    uint32_t reach_masks = 1;                  // SPIRA_REACH_MASKS: their camera rows test only the spheres their pixel run can reach (0: every sphere)
    uint32_t own_kernel = 1;                   // SPIRA_OWN_KERNEL: their full passes of 64 slots run k_path_own where own_kernel_ok() holds (0: k_path everywhere; A/B, tests)
};

struct PlanIn {
    uint32_t width = 0, rows = 0;              // the tile (rows: after validate_params)
    uint32_t spp = 0, max_depth = 0, flags = 0, batch_rays = 0;
    uint32_t n_triangles = 0;                  // of the scene
    uint32_t num_cus = 0;
    bool progressive = false, caller_rng = false, out_on_device = false;      // (caller_rng: a progressive call that hands LCG states in and out)
    bool adaptive = false;                     // round 0 of an adaptive render: slot-major L and a resolve launch of its own (k_resolve_adaptive), never pixel-owning passes
    // the constants of spira_device.h the arithmetic needs (gfx950: 256, 5 / 4, 1, 16- and 32-byte packets)
    uint32_t prec = 0, block = 0, waves_per_simd = 0, carry_key = 0;          // sizeof(T), kBlock, SPIRA_WAVES_F32 / F64, SPIRA_CARRY_KEY
    uint32_t pack4 = 0, pack3 = 0, pack2 = 0;                                 // sizeof(Pack4<T>), ...
    Knobs k;
};

enum class Org { Black, Hybrid, MetalWavefront, Metal, Cpu, Mega, Path, Bounce };      // (Black: max_depth 0, every pixel is zero)

struct Geometry { uint32_t G, cap; };          // workgroups of a wavefront launch; rays of each of its waves' queue regions

// Bytes each workspace of the context must hold for the call (0: the call does not touch it).
struct Workspace {
    uint64_t queue4 = 0, queue2 = 0, q_ref = 0, q_key = 0, q_x = 0;          // per parity: qA / qB, qC, qR, qK, qX
    uint64_t mesh_list = 0, mesh_count = 0, redo = 0, blkstats = 0, L = 0, counts = 0, accum = 0, out_tmp = 0, rng = 0;
    uint64_t hyb_state = 0, hyb_mat = 0, hyb_flags = 0;
};

struct Plan {
    PlanIn in;
    Org org = Org::Black;
    uint32_t R = 2, wpb = 0, sub = 0, max_blocks = 0;      // rays per lane, waves per workgroup, rays per wave sub-chunk, grid limit
    uint64_t tile_pixels = 0, batch = 0;                   // batch: paths of the largest pass
    uint32_t slots = 0, n_pass = 0;                        // samples of every pixel per pass; passes (equal: spp 256 at 80 slots -> 4 x 64, not 3 x 80 + 16)
    bool mesh_scene = false, defer_mesh = false, two_pass = false;      // a BVH scene; its traversal deferred (mesh lists); ... as a second, fat-wave launch
    bool fused = false, l_private = false;                 // pixel-owning passes (PathArgs::accum); wave-private radiance blocks (PathArgs::l_private)
    bool sky_runs = false;                                 // ... whose all-sky runs never enter the loop (PathArgs::sky_runs)
    bool pixel_table = false, reach_masks = false;         // ... whose camera rows are fed from the wave's pixel table / scan by their run's reach mask (PathArgs, same names)
    bool own_kernel = false;                               // ... whose passes may run k_path_own (decided pass by pass: own_kernel_ok)
    bool spec_allowed = false;                             // the organisation has a speculative-division launch for this call
    uint32_t G_max = 0, cap_max = 0;                       // geometry of the largest pass
    uint64_t q_rays = 0;
    uint32_t ppw = 0, G_metal = 0;                         // MetalWavefront: pixels per wave, workgroups
    Workspace ws;

    Geometry geometry(uint64_t n_first) const {
        if (fused) {                                       // one wave per 64 pixels; its region holds all its paths
            const uint64_t k = n_first / tile_pixels;
            return {(uint32_t)((tile_pixels + 64 * wpb - 1) / (64 * wpb)), (uint32_t)((64 * k + sub - 1) / sub * sub)};
        }
        const uint64_t n_sub = (n_first + sub - 1) / sub;
        const uint32_t G = (uint32_t)std::min<uint64_t>((n_sub + wpb - 1) / wpb, max_blocks);
        const uint64_t nw = (uint64_t)G * wpb;
        return {G, (uint32_t)(((n_sub + nw - 1) / nw) * sub)};
    }
    uint32_t k_eff(uint32_t pass) const { return std::min(slots, in.spp - pass * slots); }
    uint32_t n_first(uint32_t pass) const { return (uint32_t)((uint64_t)k_eff(pass) * tile_pixels); }
    // grid of a kernel that gives every item (pixel, path) a lane
    uint32_t blocks(uint64_t n) const { return (uint32_t)std::min<uint64_t>((n + in.block - 1) / in.block, max_blocks); }
    // the fat waves of a mesh pass's second launch: about 16 per CU (4 per SIMD), each taking over k <= 16 of the first launch's nw waves; k divides nw
    uint32_t fat_k(uint32_t nw) const {
        const uint32_t fat = std::max<uint32_t>(1, in.num_cus * in.k.mesh_fat_waves_per_cu);
        uint32_t k = 16;
        while (k > 1 && (nw % k != 0 || nw / k < fat)) k >>= 1;
        return k;
    }
    // Speculative division (spira_device.h, SpecDiv): 0 off, 1 the speculative launch and the exact one over the waves it reported, 2 every wave
    // reported (the whole pass is rendered twice; tests).  +7 % on S1 while (almost) no wave has to be rendered again, which is what a scene and
    // camera of ordinary magnitudes give (`moderate`); a scene scaled to 1e-30 would have every wave rendered twice, so it is not tried there.
    int spec(bool moderate) const {
        uint32_t s = spec_allowed ? in.k.spec_div : 0;
        if (s == 1 && !moderate) s = 0;
        return s > 2 ? 1 : (int)s;
    }
};

inline int sample_range_check(bool progressive, uint32_t sample0, uint32_t spp, const char **msg) {
    if (progressive && (uint64_t)sample0 + spp > SPIRA_MAX_SPP) { *msg = "sample0 + spp exceeds 2^24"; return SPIRA_E_LIMIT; }
    return 0;
}

// Returns 0 or a negative SPIRA_E_* code and a static message.
inline int make_plan(const PlanIn &in, Plan &pl, const char **msg) {
    auto bad = [&](const char *m) { *msg = m; return SPIRA_E_LIMIT; };
    pl = Plan{};
    pl.in = in;
    const Knobs &k = in.k;
    const uint32_t sem = in.flags & SPIRA_SEM_MASK, kern = in.flags & SPIRA_KERNEL_MASK;
    const bool ext = (in.flags & (SPIRA_EXT_DIELECTRIC | SPIRA_EXT_SPECTRAL)) != 0;
    const uint64_t tp = pl.tile_pixels = (uint64_t)in.rows * in.width;
    // default pass size: 160 Mi rays (a 1080p x 64 spp frame is one pass); ~16 GB (f32) / 31 GB (f64) of the 288 GB
    const uint32_t target = in.batch_rays ? in.batch_rays : k.batch_rays;
    uint64_t slots = std::min<uint64_t>(std::max<uint64_t>(1, target / tp), in.spp);
    const uint64_t n_pass = (in.spp + slots - 1) / slots;
    slots = (in.spp + n_pass - 1) / n_pass;
    if (slots * tp > 0x7FFFFFFFull) return bad("tile too large: rows*width must be < 2^31");
    pl.slots = (uint32_t)slots;
    pl.n_pass = (in.spp + pl.slots - 1) / pl.slots;
    pl.batch = slots * tp;
    // the secondary estimators run one lane per path / per pixel (SPIRA_SEM_METAL: or one wave per block of pixels): no passes of bounce kernels
    pl.org = sem == SPIRA_SEM_HYBRID ? Org::Hybrid : sem == SPIRA_SEM_METAL ? (kern == SPIRA_KERNEL_WAVEFRONT ? Org::MetalWavefront : Org::Metal) :
             sem == SPIRA_SEM_CPU ? Org::Cpu : kern == SPIRA_KERNEL_MEGA ? Org::Mega : kern == SPIRA_KERNEL_BOUNCE ? Org::Bounce : Org::Path;
    const bool persistent = pl.org == Org::Path;                  // k_path: one launch per pass
    pl.R = (k.R == 1 && !ext) ? 1 : 2;                            // (the extension instantiations exist for R = 2 only)
    pl.mesh_scene = in.n_triangles > SPIRA_LDS_TRIANGLES;
    pl.defer_mesh = persistent && pl.mesh_scene && in.max_depth <= 128 && k.defer_mesh != 0;
    pl.two_pass = pl.defer_mesh && k.mesh_two_pass != 0;

    // ---- launch geometry: NW = 4*G autonomous waves per wavefront kernel, each owning `cap` rays of both queues
    // workgroups per CU: the persistent kernel runs a whole pass per launch, so its launch tail is one workgroup's share of the
    // pass: 32 per CU (8 rounds of resident workgroups) measured best on S1 (16: -3.5 %, 64: -1 %, 128: -5 %; S3 likes 64-128, +1.7 %)
    // Mesh scenes want fewer, fatter waves: a wave's round ends with the dense traversal of the rays it parked at the mesh's box, and a
    // traversal batch costs its slowest ray's chain of dependent node fetches whether it holds 64 rays or 10 (config 5, 81 920 triangles:
    // f32 32 per CU 7.54 ms, 16: 6.78, 8: 7.29, 4: 7.04; f64 32: 11.67, 8: 10.29, 4: 9.68; re-measured with the round's final kernels: f32 16: 6.83, 8: 7.02, 32: 7.39,
    // f64 4: 9.54, 8: 10.13, 16: 10.49 — and counts that are not powers of two lose 10-40 %: the grid no longer divides evenly over 8 XCDs x 32 CUs).
    const uint32_t blocks_per_cu = k.blocks_per_cu ? k.blocks_per_cu : !persistent ? 16 : (pl.mesh_scene && !pl.two_pass) ? 4 : 32;
    pl.max_blocks = (uint32_t)std::min<uint64_t>((uint64_t)in.num_cus * blocks_per_cu, 0x7FFFFFFFull);
    pl.wpb = in.block / 64;
    pl.sub = 64 * pl.R;
    // pixel-owning passes (PathArgs::accum): each wave sums its own 64 pixels at its end instead of k_resolve streaming the whole of L after the
    // launch — S1 Float64 -1.5 … -4.5 %.  Only where that was measured to pay: Float64 scenes of spheres alone, no extension, at most 64 slots per pass.
    // In Float32 the end-of-wave sum costs k_path what k_resolve costs (S1 +0.30 / 0.29 ms); in the kernels with the LDS triangle scan or the
    // extensions its code costs spilled registers (glass scene Float64 +15 %, S2 +4 %).  SPIRA_FUSED_RESOLVE=0: round-robin dealing + k_resolve (A/B, tests).
    // (R = 2 too: the instantiation of SPIRA_R=1 is compiled with the triangle scan.)
    pl.fused = persistent && in.prec == 8 && pl.R == 2 && in.n_triangles == 0 && !ext && pl.slots <= 64 && k.fused_resolve != 0 && !in.adaptive;
    const Geometry g = pl.geometry(pl.batch);
    pl.G_max = g.G; pl.cap_max = g.cap;
    const uint64_t waves = (uint64_t)g.G * pl.wpb;
    // ... and keep the radiance of their paths in one contiguous block per wave (PathArgs::l_private) wherever the queue word is free to address it: the
    // RNG key is carried through the queue for max_depth <= 128 (deeper renders derive it from the path index and keep the slot-major L), and the
    // queue word has 31 bits for the entry of L.  SPIRA_PRIVATE_L=0: the slot-major layout (A/B).
    pl.l_private = pl.fused && in.carry_key && in.max_depth <= 128 && k.private_l != 0 && 64ull * waves * pl.slots <= 0x7FFFFFFFull;
    pl.sky_runs = pl.fused && k.sky_runs != 0;
    pl.pixel_table = pl.fused && k.pixel_table != 0;
    pl.reach_masks = pl.fused && k.reach_masks != 0;
    pl.own_kernel = pl.fused && k.own_kernel != 0;
    pl.q_rays = (uint64_t)g.cap * waves;
    if (pl.q_rays > 0xFFFFFFFFull) return bad("pass too large");
    // the speculative launch: fresh renders only (a progressive SPIRA_SEM_METAL call updates sums and states in place), R = 2 instantiations only
    pl.spec_allowed = pl.org == Org::Cpu || (pl.org == Org::Metal && !in.progressive) || (pl.org == Org::MetalWavefront && !in.progressive && pl.R == 2) ||
                      (persistent && pl.R == 2);
    if (in.max_depth == 0) pl.org = Org::Black;

    // ---- workspaces (cached per device, grown on demand; sized for 288 GB HBM: no chunking of a pass)
    Workspace &w = pl.ws;
    const uint64_t redo_per_wave = (pl.spec_allowed && k.spec_div) ? sizeof(uint32_t) : 0, stat_row = 4 * sizeof(uint32_t);
    w.accum = tp * in.pack4;
    w.out_tmp = in.out_on_device ? 0 : 2 * 3 * tp * in.prec;
    if (in.caller_rng && !in.out_on_device) w.rng = tp * sizeof(uint32_t);
    switch (pl.org) {
    case Org::Black: break;
    case Org::Hybrid:                      // per-pixel ray state between its launches, one flag per launch
        if (tp > 0xFFFFFFFFull / 2) return bad("image too large for SPIRA_SEM_HYBRID");
        w.hyb_state = 12 * tp * in.prec; w.hyb_mat = w.rng = tp * sizeof(uint32_t);
        w.hyb_flags = (uint64_t)in.spp * (in.max_depth + 1) * sizeof(uint32_t);
        break;
    case Org::MetalWavefront: {            // every wave owns a block of ppw pixels: one resident round of workgroups
        const uint64_t nw0 = (uint64_t)in.num_cus * in.waves_per_simd * pl.wpb;
        pl.ppw = (uint32_t)((((tp + nw0 - 1) / nw0) + 63) / 64 * 64);
        pl.G_metal = (uint32_t)((tp + (uint64_t)pl.ppw * pl.wpb - 1) / ((uint64_t)pl.ppw * pl.wpb));
        const uint64_t nw = (uint64_t)pl.G_metal * pl.wpb, n = nw * pl.ppw;
        w.queue4 = n * in.pack4; w.queue2 = n * in.pack2; w.q_x = n * 2 * sizeof(uint32_t); w.L = n * in.pack3;
        if (!in.caller_rng) w.rng = tp * sizeof(uint32_t);
        w.blkstats = nw * stat_row; w.redo = nw * redo_per_wave;
        break;
    }
    case Org::Metal: case Org::Cpu: case Org::Mega:
        w.L = pl.batch * in.pack3; w.blkstats = waves * stat_row;
        w.redo = (pl.org == Org::Metal ? pl.blocks(tp) : pl.org == Org::Cpu ? pl.max_blocks : 0) * (uint64_t)pl.wpb * redo_per_wave;
        break;
    case Org::Bounce:                      // per-wave survivor counts and one row of statistics per wave per launch
        if (in.max_depth > 1) { w.queue4 = pl.q_rays * in.pack4; w.queue2 = pl.q_rays * in.pack2; }
        w.L = pl.batch * in.pack3;
        w.counts = (uint64_t)(in.max_depth + 2) * waves * sizeof(uint32_t); w.blkstats = (uint64_t)(in.max_depth + 1) * waves * stat_row;
        break;
    case Org::Path:
        // hit queues, one entry per ray of the largest pass (worst case: every path queued / parked once).  max_depth == 1 needs none — except on a
        // mesh scene: a parked camera ray's hit comes back from its traversal session as a packet.
        if (in.max_depth > 1 || pl.mesh_scene) {
            w.queue4 = pl.q_rays * in.pack4; w.queue2 = pl.q_rays * in.pack2;
            if (in.prec == 4) w.q_ref = pl.q_rays * sizeof(uint32_t);
            if (!pl.defer_mesh) w.q_key = pl.q_rays * 2 * sizeof(uint32_t);      // carried RNG keys (sphere scenes; the extension launches leave them unused)
        }
        if (pl.defer_mesh) w.mesh_list = 3 * pl.q_rays * in.pack4;               // the wave-owned lists of rays waiting for their dense traversal batch
        if (pl.two_pass) w.mesh_count = waves * sizeof(uint32_t);                // per-wave parked counts, from the parking launch to the fat-wave launch
        w.redo = waves * redo_per_wave; w.blkstats = waves * stat_row;
        // (a pixel-owning grid depends on the pixel count alone: G_max workgroups in every pass, each wave with a block of 64 * slots entries)
        w.L = (pl.l_private ? std::max<uint64_t>(pl.batch, 64ull * waves * pl.slots) : pl.batch) * in.pack3;
        break;
    }
    return 0;
}

// ---- what a k_path launch needs of the workspaces, on counts: verify_path_args() (spira_hip.hip) compares these with the buffers behind the
// pointers of the PathArgs about to be launched; the sanitizer harness with Plan::ws, for every pass of every plan of its sweep.
// The LDS a launch that can run a pixel-owning pass adds for the pixel table and the reach masks (k_path's prologue writes both, the camera rows read
// them): per wave 64 entries of kPixelEntryBytes — {mix32(sA + pixel), mix32(sB ^ pixel), i - 1, j - 1, pixel}, padded — and one mask word per run.
constexpr uint32_t kPixelEntryBytes = 32, kOwnRuns = 16;
inline uint64_t own_lds_bytes(uint32_t wpb) { return (uint64_t)wpb * (64 * kPixelEntryBytes + kOwnRuns * sizeof(uint32_t)); }
struct PathLaunch {
    uint32_t blocks = 0, cap = 0, n_first = 0, k_eff = 0;      // blocks: of the pass's first launch (a fat wave of the second owns the regions of the waves it takes over)
    uint32_t tile_pixels = 0, max_depth = 0, flags = 0, n_lds_triangles = 0;
    uint32_t mesh_mode = 0, resume_k = 1, resume_nw = 0;
    bool mesh = false, pixel_owning = false, l_private = false;
    bool pixel_table = false, reach_masks = false;             // PathArgs, same names
    uint64_t own_lds = 0;                                      // bytes the launch's LDS block holds for the pixel table and the run masks (own_lds_bytes)
    uint32_t prec = 0, wpb = 0, carry_key = 0;
    // what own_kernel_ok() reads on top: rays per lane, spheres of the scene, PathArgs::sky_runs / cam_consts, Plan::own_kernel
    uint32_t R = 0, n_spheres = 0;
    bool sky_runs = false, cam_consts = false, own_kernel = false;
};
struct PathNeed {
    uint64_t nw, packets, l_entries;       // waves; entries of every per-packet array; entries of L
    bool fits, resume_ok, owning_ok, private_ok, table_ok;
};
inline PathNeed path_need(const PathLaunch &a) {
    PathNeed n{};
    n.nw = (uint64_t)a.blocks * a.wpb;
    n.packets = n.nw * a.cap;
    n.fits = a.n_first <= n.packets;
    n.resume_ok = a.resume_k != 0 && a.resume_k <= 16 && n.nw % a.resume_k == 0 && a.resume_nw == n.nw;
    // (wave-private radiance blocks: 64 k_eff entries for every wave of the grid, more than n_first when the tile's pixel count is no multiple of 64 * waves per workgroup)
    n.l_entries = a.l_private ? std::max<uint64_t>(a.n_first, 64ull * n.nw * a.k_eff) : a.n_first;
    // pixel-owning pass: an instantiation that resolves, a wave for every pixel, every wave's paths in its region
    const uint64_t tp = a.tile_pixels;
    n.owning_ok = a.prec == 8 && !a.n_lds_triangles && !a.mesh && !(a.flags & (SPIRA_EXT_DIELECTRIC | SPIRA_EXT_SPECTRAL)) && a.k_eff != 0 && a.k_eff <= 64 &&
                  (uint64_t)a.k_eff * tp == a.n_first && 64 * n.nw >= tp && a.cap >= 64ull * a.k_eff;
    // wave-private radiance blocks: pixel-owning passes whose queue word need not be the path index (the RNG key is carried: max_depth <= 128)
    n.private_ok = a.pixel_owning && a.carry_key && a.max_depth <= 128 && n.l_entries <= 0x80000000ull;
    // pixel table / reach masks: pixel-owning passes alone, and the launch's LDS block has their region
    n.table_ok = (!a.pixel_table && !a.reach_masks) || (a.pixel_owning && a.own_lds >= own_lds_bytes(a.wpb));
    return n;
}

// k_path_own (spira_device.h; its statements: spira_path_body.h with FIXED) renders this pass instead of k_path: exactly the passes whose facts that kernel holds as constants.
// A full pixel-owning pass of 64 slots of a Float64 sphere scene (R = 2, no triangles of either kind, no extension, one launch), its radiance in
// wave-private blocks (so the RNG key is carried: max_depth <= 128), all-sky runs, pixel table, reach masks (their LDS region granted) and the camera's
// packets on, and a scene the reach mask has a bit for every sphere of.  Anything else — shorter passes above all (k_eff 1, 3, 6, a tail of 63) — is k_path's.
inline bool own_kernel_ok(const PathLaunch &a) {
    const PathNeed n = path_need(a);
    return a.own_kernel && a.prec == 8 && a.R == 2 && !a.mesh && !a.n_lds_triangles && !(a.flags & (SPIRA_EXT_DIELECTRIC | SPIRA_EXT_SPECTRAL)) && a.mesh_mode == 0 &&
           a.pixel_owning && n.owning_ok && a.l_private && n.private_ok &&
           a.sky_runs && a.pixel_table && a.reach_masks && a.own_lds >= own_lds_bytes(a.wpb) && a.cam_consts &&
           a.k_eff == 64 && a.n_spheres >= 1 && a.n_spheres <= 32 && a.max_depth <= 128 && a.carry_key != 0;
}

// ---- adaptive sampling (spira_render_adaptive_*; kernels in spira_adaptive.h): the sample schedule of a call and what its rounds need, as arithmetic.
// Round 0 gives every pixel of the tile min_spp samples (a plan of its own: make_plan with PlanIn::adaptive and spp = min_spp); round r >= 1 gives every
// pixel still active level(r) - level(r - 1) more, where level(r) = min(min_spp + r * batch_spp, spp): the levels min, min + batch, ..., spp.
struct AdaptiveIn {
    uint32_t min_spp = 0, batch_spp = 0, spp = 0;          // spira_adaptive + the cap (spira_params::spp)
    double tolerance = 0, floor = 0;
    uint64_t tile_pixels = 0;
    uint32_t prec = 0, pack3 = 0, num_cus = 0;             // sizeof(T), sizeof(Pack3<T>)
};
// a refinement launch: every wave owns `ppw` consecutive entries of the active list and walks their samples `chunk` at a time, ppw * chunk <= kAdaptiveItems
// radiance entries of LDS per wave; `grid` workgroups of kAdaptiveWpb waves
constexpr uint32_t kAdaptiveItems = 256, kAdaptiveWpb = 4;
struct AdaptiveRound { uint32_t samples, chunk, ppw, grid; uint64_t waves; };
struct AdaptivePlan {
    AdaptiveIn in;
    uint32_t levels = 0;                       // distinct sample counts a pixel can end with; rounds = levels (round 0 included)
    uint64_t list_cap = 0;                     // entries of each of the two active lists
    uint64_t list_bytes = 0, q_bytes = 0, n_bytes = 0, count_bytes = 0;      // per list; Q (one T per pixel); samples taken (one word per pixel); the two list lengths
    uint64_t lds_round = 0;                    // LDS a refinement workgroup adds to the scene's
    uint32_t level(uint32_t r) const { return (uint32_t)std::min<uint64_t>((uint64_t)in.min_spp + (uint64_t)r * in.batch_spp, in.spp); }
    // geometry of round r >= 1 over n_active list entries (n_active >= 1)
    AdaptiveRound round(uint32_t r, uint64_t n_active) const {
        AdaptiveRound a{};
        a.samples = level(r) - level(r - 1);
        a.chunk = std::min(a.samples, kAdaptiveItems);
        // small lists: fewer pixels per wave, so that the launch still has a few waves for every SIMD (the result does not depend on it)
        const uint64_t want_waves = std::max<uint64_t>(1, (uint64_t)in.num_cus * 16);
        const uint64_t spread = (n_active + want_waves - 1) / want_waves;
        a.ppw = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(std::min<uint32_t>(64, kAdaptiveItems / a.chunk), spread));
        a.waves = (n_active + a.ppw - 1) / a.ppw;
        a.grid = (uint32_t)((a.waves + kAdaptiveWpb - 1) / kAdaptiveWpb);
        return a;
    }
};
inline int adaptive_check(uint32_t min_spp, uint32_t batch_spp, uint32_t spp, double tolerance, double floor, const char **msg) {
    if (min_spp < 2) { *msg = "spira_adaptive: min_spp must be >= 2 (a variance needs two samples)"; return SPIRA_E_INVALID; }
    if (batch_spp < 1) { *msg = "spira_adaptive: batch_spp must be >= 1"; return SPIRA_E_INVALID; }
    if (min_spp > spp) { *msg = "spira_adaptive: min_spp exceeds params->spp (the cap)"; return SPIRA_E_INVALID; }
    if (!(tolerance >= 0) || !(floor >= 0)) { *msg = "spira_adaptive: tolerance and floor must be >= 0"; return SPIRA_E_INVALID; }
    return 0;
}
inline int make_adaptive_plan(const AdaptiveIn &in, AdaptivePlan &ap, const char **msg) {
    ap = AdaptivePlan{};
    ap.in = in;
    if (int rc = adaptive_check(in.min_spp, in.batch_spp, in.spp, in.tolerance, in.floor, msg)) return rc;
    if (in.tile_pixels == 0 || in.tile_pixels > 0x7FFFFFFFull) { *msg = "tile too large: rows*width must be < 2^31"; return SPIRA_E_LIMIT; }
    ap.levels = 1 + (uint32_t)(((uint64_t)(in.spp - in.min_spp) + in.batch_spp - 1) / in.batch_spp);
    ap.list_cap = in.tile_pixels;              // a list never holds a pixel twice
    ap.list_bytes = ap.list_cap * sizeof(uint32_t);
    ap.q_bytes = in.tile_pixels * in.prec;
    ap.n_bytes = in.tile_pixels * sizeof(uint32_t);
    ap.count_bytes = 2 * sizeof(uint32_t);
    ap.lds_round = (uint64_t)kAdaptiveWpb * kAdaptiveItems * in.pack3;
    return 0;
}

// ---- first-hit feature buffers (spira_render_features_*) and the a-trous denoiser (spira_denoise_*); kernels in spira_denoise.h.
// The scope of the feature entries: SPIRA_SEM_A with SPIRA_KERNEL_DEFAULT, no extension.
inline int features_check(uint32_t flags, bool any_output, const char **msg) {
    if (!any_output) { *msg = "all three feature outputs are NULL"; return SPIRA_E_INVALID; }
    if ((flags & SPIRA_SEM_MASK) != SPIRA_SEM_A) { *msg = "feature buffers are built for SPIRA_SEM_A only"; return SPIRA_E_UNSUPPORTED; }
    if ((flags & SPIRA_KERNEL_MASK) != SPIRA_KERNEL_DEFAULT) { *msg = "feature buffers have one kernel organisation: SPIRA_KERNEL_DEFAULT"; return SPIRA_E_UNSUPPORTED; }
    if (flags & (SPIRA_EXT_DIELECTRIC | SPIRA_EXT_SPECTRAL)) { *msg = "SPIRA_EXT_* extensions are not built into the feature kernel"; return SPIRA_E_UNSUPPORTED; }
    return 0;
}
// one lane per pixel of the tile, workgroups of `block` lanes, at most max_blocks of them (the kernel strides)
inline uint32_t features_grid(uint64_t tile_pixels, uint32_t block, uint32_t num_cus) {
    const uint64_t cap = std::max<uint64_t>(1, (uint64_t)num_cus * 64);
    return (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>((tile_pixels + block - 1) / block, cap));
}

// The denoiser works on whole frames.  A workgroup of kDenoiseTileH waves covers a tile of kDenoiseTileW x kDenoiseTileH pixels, a wave 64 contiguous
// pixels of one row; iteration `it` reaches 2 << it pixels to every side.  Per pixel: one colour record {c.rgb, v} in each of two ping-pong buffers and,
// when a normal or a depth plane is given, one guide record {n.xyz, z}, each a Pack4<T>.  The host form stages its planes in one input and one output block.
constexpr uint32_t kDenoiseTileW = 64, kDenoiseTileH = 4, kDenoiseMaxIter = 6;
enum : uint32_t { kDenoiseVariance = 1, kDenoiseAlbedo = 2, kDenoiseNormal = 4, kDenoiseDepth = 8 };
struct DenoiseIn {
    uint32_t width = 0, height = 0, iterations = 0, post = 0;
    double sigma_l = 0, sigma_z = 0;
    uint32_t guides = 0;                       // kDenoise* bits: the planes given
    bool want_hdr = false, want_img = false, host = false;
    uint32_t prec = 0, pack4 = 0;              // sizeof(T), sizeof(Pack4<T>)
};
struct DenoisePlan {
    DenoiseIn in;
    uint64_t npix = 0;
    uint32_t tiles_x = 0, tiles_y = 0, grid = 0;           // grid = tiles_x * tiles_y workgroups of kDenoiseTileW * kDenoiseTileH lanes
    uint32_t grid_flat = 0;                                // prepare: one lane per pixel
    uint64_t rec_bytes = 0, guide_bytes = 0;               // each ping-pong buffer; the guide records (0: no normal and no depth)
    uint64_t in_planes = 0, out_planes = 0, io_bytes = 0;  // host form: planes staged in, planes staged out, the block that holds both
    // host form: plane offset (in planes) of each input inside the staging block, in the order color, variance, albedo, normal, depth; -1: not given
    int64_t in_off[5] = {-1, -1, -1, -1, -1};
    uint32_t step(uint32_t it) const { return 1u << it; }
    uint32_t reach(uint32_t it) const { return 2u << it; }
};
inline int denoise_check(uint32_t width, uint32_t height, uint32_t iterations, uint32_t post, double sigma_l, double sigma_z, const char **msg) {
    if (width < 1 || height < 1) { *msg = "spira_denoise: width and height must be >= 1"; return SPIRA_E_INVALID; }
    if (iterations < 1 || iterations > kDenoiseMaxIter) { *msg = "spira_denoise: iterations must be 1 .. 6"; return SPIRA_E_INVALID; }
    if (!(sigma_l > 0) || !(sigma_z > 0)) { *msg = "spira_denoise: sigma_l and sigma_z must be > 0"; return SPIRA_E_INVALID; }
    if (post != SPIRA_POST_ACES && post != SPIRA_POST_ACES_GAMMA && post != SPIRA_POST_CLAMP_GAMMA && post != SPIRA_POST_NONE) {
        *msg = "spira_denoise: post must be one of SPIRA_POST_*"; return SPIRA_E_INVALID;
    }
    return 0;
}
inline int make_denoise_plan(const DenoiseIn &in, DenoisePlan &dp, const char **msg) {
    dp = DenoisePlan{};
    dp.in = in;
    if (int rc = denoise_check(in.width, in.height, in.iterations, in.post, in.sigma_l, in.sigma_z, msg)) return rc;
    if (!in.want_hdr && !in.want_img) { *msg = "both outputs are NULL"; return SPIRA_E_INVALID; }
    dp.npix = (uint64_t)in.width * in.height;
    if (dp.npix > 0x7FFFFFFFull) { *msg = "image larger than 2^31 pixels"; return SPIRA_E_LIMIT; }
    dp.tiles_x = (in.width + kDenoiseTileW - 1) / kDenoiseTileW;
    dp.tiles_y = (in.height + kDenoiseTileH - 1) / kDenoiseTileH;
    dp.grid = (uint32_t)((uint64_t)dp.tiles_x * dp.tiles_y);               // <= npix
    dp.grid_flat = (uint32_t)((dp.npix + kDenoiseTileW * kDenoiseTileH - 1) / (kDenoiseTileW * kDenoiseTileH));
    dp.rec_bytes = dp.npix * in.pack4;
    dp.guide_bytes = (in.guides & (kDenoiseNormal | kDenoiseDepth)) ? dp.npix * in.pack4 : 0;
    if (in.host) {
        const uint32_t bit[5] = {0, kDenoiseVariance, kDenoiseAlbedo, kDenoiseNormal, kDenoiseDepth}, planes[5] = {3, 1, 3, 3, 1};
        for (int k = 0; k < 5; ++k)
            if (k == 0 || (in.guides & bit[k])) { dp.in_off[k] = (int64_t)dp.in_planes; dp.in_planes += planes[k]; }
        dp.out_planes = (in.want_hdr ? 3 : 0) + (in.want_img ? 3 : 0);
        dp.io_bytes = (dp.in_planes + dp.out_planes) * dp.npix * in.prec;
    }
    return 0;
}

// ---- ray queries on a scene handle (spira_scene_cast_* / spira_scene_occluded_*); kernels in spira_query.h.
// The session kernel runs `waves` persistent waves in workgroups of wpb; wave w owns the contiguous range of base + (w < rem) rays that starts at
// w base + min(w, rem): the ranges are disjoint, cover [0, n_rays) and differ by at most one ray, so no wave is empty unless n_rays < waves.  The number
// of waves is what the device holds (waves_per_cu per CU) but never so many that a wave gets fewer than kCastMinRaysPerWave rays: a session lives on
// refills, and a wave with one fill of rays would be the in-place walk with extra bookkeeping.  The one-lane-per-ray kernels stride a flat grid.
constexpr uint32_t kCastMinRaysPerWave = 128;
struct CastKnobs { uint32_t refill = 16, waves_per_cu = 20; };      // SPIRA_CAST_REFILL (free lanes that trigger a refill, 1 .. 64), SPIRA_CAST_WAVES_PER_CU
struct CastPlan {
    uint32_t n_rays = 0;
    uint32_t grid = 0, wpb = 0, waves = 0;     // session: workgroups, waves per workgroup, grid * wpb
    uint32_t base = 0, rem = 0;                // rays per wave and how many waves take one more
    uint32_t refill_free = 0;
    uint32_t grid_flat = 0;                    // one lane per ray: workgroups (the kernel strides)
    uint32_t begin(uint32_t w) const { return w * base + std::min(w, rem); }
    uint32_t count(uint32_t w) const { return base + (w < rem ? 1u : 0u); }
};
inline int cast_check(bool rays, uint32_t n_rays, uint32_t flags, bool any_output, const char **msg) {
    if (!rays) { *msg = "the ray array is NULL"; return SPIRA_E_INVALID; }
    if (n_rays == 0) { *msg = "n_rays is 0"; return SPIRA_E_INVALID; }
    if (flags & ~SPIRA_CAST_INPLACE) { *msg = "unknown flag bits (SPIRA_CAST_INPLACE is the only one)"; return SPIRA_E_INVALID; }
    if (!any_output) { *msg = "every output is NULL"; return SPIRA_E_INVALID; }
    if (n_rays > SPIRA_MAX_RAYS) { *msg = "more than SPIRA_MAX_RAYS (2^26) rays"; return SPIRA_E_LIMIT; }
    return 0;
}
// spira_scene_closest_point_*: cast_check's rules for a point list
inline int nearest_check(bool points, uint32_t n_points, uint32_t flags, bool any_output, const char **msg) {
    if (!points) { *msg = "the point array is NULL"; return SPIRA_E_INVALID; }
    if (n_points == 0) { *msg = "n_points is 0"; return SPIRA_E_INVALID; }
    if (flags & ~SPIRA_CAST_INPLACE) { *msg = "unknown flag bits (SPIRA_CAST_INPLACE is the only one)"; return SPIRA_E_INVALID; }
    if (!any_output) { *msg = "out_prim, out_dist and out_point are all NULL"; return SPIRA_E_INVALID; }
    if (n_points > SPIRA_MAX_RAYS) { *msg = "more than SPIRA_MAX_RAYS (2^26) points"; return SPIRA_E_LIMIT; }
    return 0;
}
// spira_scene_cast_hits_*: cast's rules, then the list's.  any_output: out_prim, out_t or out_count is given — with max_hits == 0 only out_count is one.
inline int hits_check(bool rays, uint32_t n_rays, uint32_t max_hits, uint32_t flags, bool any_output, const char **msg) {
    if (!rays) { *msg = "the ray array is NULL"; return SPIRA_E_INVALID; }
    if (n_rays == 0) { *msg = "n_rays is 0"; return SPIRA_E_INVALID; }
    if (flags & ~(SPIRA_CAST_INPLACE | SPIRA_HITS_COUNT_ALL)) { *msg = "unknown flag bits (SPIRA_CAST_INPLACE and SPIRA_HITS_COUNT_ALL are the only ones)"; return SPIRA_E_INVALID; }
    if (max_hits > SPIRA_MAX_HITS) { *msg = "max_hits is above SPIRA_MAX_HITS (16)"; return SPIRA_E_INVALID; }
    if (max_hits == 0 && !(flags & SPIRA_HITS_COUNT_ALL)) { *msg = "max_hits is 0 without SPIRA_HITS_COUNT_ALL"; return SPIRA_E_INVALID; }
    if (!any_output) { *msg = max_hits ? "out_prim, out_t and out_count are all NULL" : "max_hits is 0 and out_count is NULL: nothing to write"; return SPIRA_E_INVALID; }
    if (n_rays > SPIRA_MAX_RAYS) { *msg = "more than SPIRA_MAX_RAYS (2^26) rays"; return SPIRA_E_LIMIT; }
    if ((uint64_t)n_rays * max_hits > SPIRA_MAX_RAYS) { *msg = "n_rays * max_hits is above SPIRA_MAX_RAYS (2^26) slots"; return SPIRA_E_LIMIT; }
    return 0;
}
// spira_scene_nearest_k_*: closest point's rules, then the list's.  any_output: out_prim, out_dist, out_point or out_count is given — with max_near == 0
// only out_count is one.
inline int nearest_k_check(bool points, uint32_t n_points, uint32_t max_near, uint32_t flags, bool any_output, const char **msg) {
    if (!points) { *msg = "the point array is NULL"; return SPIRA_E_INVALID; }
    if (n_points == 0) { *msg = "n_points is 0"; return SPIRA_E_INVALID; }
    if (flags & ~(SPIRA_CAST_INPLACE | SPIRA_NEAR_COUNT_ALL)) { *msg = "unknown flag bits (SPIRA_CAST_INPLACE and SPIRA_NEAR_COUNT_ALL are the only ones)"; return SPIRA_E_INVALID; }
    if (max_near > SPIRA_MAX_NEAR) { *msg = "max_near is above SPIRA_MAX_NEAR (16)"; return SPIRA_E_INVALID; }
    if (max_near == 0 && !(flags & SPIRA_NEAR_COUNT_ALL)) { *msg = "max_near is 0 without SPIRA_NEAR_COUNT_ALL"; return SPIRA_E_INVALID; }
    if (!any_output) { *msg = max_near ? "out_prim, out_dist, out_point and out_count are all NULL" : "max_near is 0 and out_count is NULL: nothing to write"; return SPIRA_E_INVALID; }
    if (n_points > SPIRA_MAX_RAYS) { *msg = "more than SPIRA_MAX_RAYS (2^26) points"; return SPIRA_E_LIMIT; }
    if ((uint64_t)n_points * max_near > SPIRA_MAX_RAYS) { *msg = "n_points * max_near is above SPIRA_MAX_RAYS (2^26) slots"; return SPIRA_E_LIMIT; }
    return 0;
}
// spira_scene_sweep_* / spira_scene_sweep_blocked_*: cast_check's rules for a ray list with one radius per ray.  any_output: out_prim, out_t, out_point or
// out_normal is given (blocked: out_hit); out_trips alone is no output.
inline int sweep_check(bool rays, bool radii, uint32_t n, uint32_t flags, bool any_output, const char **msg) {
    if (!rays) { *msg = "the ray array is NULL"; return SPIRA_E_INVALID; }
    if (!radii) { *msg = "the radius array is NULL"; return SPIRA_E_INVALID; }
    if (n == 0) { *msg = "n is 0"; return SPIRA_E_INVALID; }
    if (flags & ~SPIRA_CAST_INPLACE) { *msg = "unknown flag bits (SPIRA_CAST_INPLACE is the only one)"; return SPIRA_E_INVALID; }
    if (!any_output) { *msg = "every output is NULL"; return SPIRA_E_INVALID; }
    if (n > SPIRA_MAX_RAYS) { *msg = "more than SPIRA_MAX_RAYS (2^26) sweeps"; return SPIRA_E_LIMIT; }
    return 0;
}
// spira_scene_overlap_box_* / spira_scene_overlap_any_*: nearest_k_check's rules for a box list; there is no count flag (the count is always complete), so
// max_list may be 0 as it is.  any_output: out_prim or out_count is given — with max_list == 0 only out_count is one (the any form: out_hit); out_trips
// alone is no output.
inline int overlap_check(bool boxes, uint32_t n, uint32_t max_list, uint32_t flags, bool any_output, const char **msg) {
    if (!boxes) { *msg = "the box array is NULL"; return SPIRA_E_INVALID; }
    if (n == 0) { *msg = "n is 0"; return SPIRA_E_INVALID; }
    if (flags & ~SPIRA_CAST_INPLACE) { *msg = "unknown flag bits (SPIRA_CAST_INPLACE is the only one)"; return SPIRA_E_INVALID; }
    if (max_list > SPIRA_MAX_OVERLAP) { *msg = "max_list is above SPIRA_MAX_OVERLAP (16)"; return SPIRA_E_INVALID; }
    if (!any_output) { *msg = max_list ? "every output is NULL" : "max_list is 0 and out_count is NULL: nothing to write"; return SPIRA_E_INVALID; }
    if (n > SPIRA_MAX_RAYS) { *msg = "more than SPIRA_MAX_RAYS (2^26) boxes"; return SPIRA_E_LIMIT; }
    if ((uint64_t)n * max_list > SPIRA_MAX_RAYS) { *msg = "n * max_list is above SPIRA_MAX_RAYS (2^26) slots"; return SPIRA_E_LIMIT; }
    return 0;
}
// spira_scene_overlap_tri_* / spira_scene_overlap_tri_any_*: overlap_check's rules, case for case and in its order; only the two messages that name the
// list speak of triangles.
inline int overlap_tri_check(bool triangles, uint32_t n, uint32_t max_list, uint32_t flags, bool any_output, const char **msg) {
    if (!triangles) { *msg = "the query triangle array is NULL"; return SPIRA_E_INVALID; }
    const int rc = overlap_check(true, n, max_list, flags, any_output, msg);
    if (rc == SPIRA_E_LIMIT && n > SPIRA_MAX_RAYS) *msg = "more than SPIRA_MAX_RAYS (2^26) query triangles";
    return rc;
}
// spira_scene_signed_distance_*: closest point's rules; any_output: out_prim, out_dist, out_point, out_inside or out_crossings is given (out_trips alone is no
// output).  With out_prim, out_dist and out_point all NULL the call is the sign-only query: the nearest walk is not run (signed_distance_wants_nearest).
inline int signed_distance_check(bool points, uint32_t n_points, uint32_t flags, bool any_output, const char **msg) {
    if (!points) { *msg = "the point array is NULL"; return SPIRA_E_INVALID; }
    if (n_points == 0) { *msg = "n_points is 0"; return SPIRA_E_INVALID; }
    if (flags & ~SPIRA_CAST_INPLACE) { *msg = "unknown flag bits (SPIRA_CAST_INPLACE is the only one)"; return SPIRA_E_INVALID; }
    if (!any_output) { *msg = "out_prim, out_dist, out_point, out_inside and out_crossings are all NULL"; return SPIRA_E_INVALID; }
    if (n_points > SPIRA_MAX_RAYS) { *msg = "more than SPIRA_MAX_RAYS (2^26) points"; return SPIRA_E_LIMIT; }
    return 0;
}
inline bool signed_distance_wants_nearest(bool prim, bool dist, bool point) { return prim || dist || point; }
inline CastPlan make_cast_plan(uint32_t n_rays, uint32_t num_cus, uint32_t block, const CastKnobs &k) {
    CastPlan p;
    p.n_rays = n_rays;
    p.wpb = std::max<uint32_t>(1, block / 64);
    const uint64_t max_blocks = std::max<uint64_t>(1, (uint64_t)std::max<uint32_t>(1, num_cus) * std::max<uint32_t>(1, k.waves_per_cu) / p.wpb);
    const uint64_t want_blocks = std::max<uint64_t>(1, (uint64_t)n_rays / ((uint64_t)kCastMinRaysPerWave * p.wpb));
    p.grid = (uint32_t)std::min<uint64_t>(std::min(max_blocks, want_blocks), 1u << 20);
    p.waves = p.grid * p.wpb;
    p.base = n_rays / p.waves; p.rem = n_rays % p.waves;
    p.refill_free = std::min<uint32_t>(64, std::max<uint32_t>(1, k.refill));
    p.grid_flat = features_grid(n_rays, block, num_cus);
    return p;
}

// ---- the arrays of a host-form list call (stage_in; spira_hip.hip): where each block lies in the context's staging buffer.  The blocks keep their
// order; a present block starts at the next multiple of kStageAlign at or after the end of the present block before it — enough for every element type
// of the entries, whatever sizes precede it — and a block that is not present (a NULL array of the caller) takes no room.  offset[k] is written for
// every block (for one not present: where the next present one starts); returns the bytes the buffer must hold, the end of the last present block.
constexpr size_t kStageAlign = 16;
inline size_t stage_layout(const size_t *bytes, const bool *present, int n, size_t *offset) {
    size_t end = 0;
    for (int k = 0; k < n; ++k) {
        offset[k] = (end + (kStageAlign - 1)) & ~(kStageAlign - 1);
        if (present[k]) end = offset[k] + bytes[k];
    }
    return end;
}

// ---- radiance along the caller's rays (spira_scene_radiance_*) and the camera ray generator (spira_camera_rays_*); kernels in spira_radiance.h.
// A work item is (ray, sample), sample-minor.  A pass covers spp_pass consecutive samples of every ray — pass p the samples [p spp_pass, min((p + 1)
// spp_pass, spp)) of the call, ascending and contiguous, so that the sums see their samples in order whatever the split — and holds at most max_items
// items: what the workspace (one Pack3<T> per item) is capped by.  A pass of ONE sample per ray needs no workspace: the lane that owns the ray adds to its
// sum itself (`direct`).  The pass count is the least the cap admits and the passes are as equal as that count allows (spp 10, at most 6 per pass: 5 + 5).
constexpr uint32_t kRadianceMaxItems = 1u << 26;      // >= SPIRA_MAX_RAYS: one sample of every ray always fits a pass
struct RadianceKnobs { uint32_t waves_per_cu = 64, max_items = kRadianceMaxItems; };      // SPIRA_RADIANCE_WAVES_PER_CU (0: one workgroup), SPIRA_RADIANCE_MAX_ITEMS
struct RadiancePlan {
    uint32_t n_rays = 0, spp = 0;
    uint32_t spp_pass = 0, n_pass = 0;         // samples of every ray per pass (the last pass may hold fewer); passes
    uint32_t grid = 0, wpb = 0;                // workgroups of k_radiance (it strides over the pass's items), waves per workgroup
    uint32_t grid_flat = 0;                    // k_radiance_sum: one lane per ray (it strides)
    bool direct = false;                       // spp_pass == 1: no workspace
    uint64_t ws_entries = 0;                   // entries of the workspace: n_rays * spp_pass, or 0
    uint32_t max_items = 0;                    // the cap as applied
    uint32_t first(uint32_t p) const { return p * spp_pass; }                       // relative to the call's sample0
    uint32_t count(uint32_t p) const { return std::min(spp_pass, spp - p * spp_pass); }
    uint64_t items(uint32_t p) const { return (uint64_t)n_rays * count(p); }
};
inline int radiance_check(bool rays, bool params, bool sums, uint32_t n_rays, uint32_t spp, uint32_t max_depth, uint32_t flags, uint32_t sample0, uint32_t key0,
                          uint32_t reserved, const char **msg) {
    if (!rays) { *msg = "the ray array is NULL"; return SPIRA_E_INVALID; }
    if (!params) { *msg = "the spira_radiance struct is NULL"; return SPIRA_E_INVALID; }
    if (!sums) { *msg = "sum_rgb is NULL"; return SPIRA_E_INVALID; }
    if (n_rays == 0) { *msg = "n_rays is 0"; return SPIRA_E_INVALID; }
    if (spp == 0) { *msg = "spp is 0"; return SPIRA_E_INVALID; }
    if (max_depth < 1 || max_depth > SPIRA_MAX_DEPTH) { *msg = "max_depth must be 1 .. SPIRA_MAX_DEPTH (255)"; return SPIRA_E_INVALID; }
    if (reserved != 0) { *msg = "spira_radiance::reserved must be 0"; return SPIRA_E_INVALID; }
    if (flags & ~(SPIRA_EXT_DIELECTRIC | SPIRA_EXT_SPECTRAL)) { *msg = "flags: 0, SPIRA_EXT_DIELECTRIC and SPIRA_EXT_SPECTRAL are all the radiance entries take"; return SPIRA_E_UNSUPPORTED; }
    if (n_rays > SPIRA_MAX_RAYS) { *msg = "more than SPIRA_MAX_RAYS (2^26) rays"; return SPIRA_E_LIMIT; }
    if ((uint64_t)key0 + n_rays > (1ull << 32)) { *msg = "key0 + n_rays exceeds 2^32"; return SPIRA_E_LIMIT; }
    if ((uint64_t)sample0 + spp > SPIRA_MAX_SPP) { *msg = "sample0 + spp exceeds 2^24"; return SPIRA_E_LIMIT; }
    return 0;
}
// n_rays in 1 .. SPIRA_MAX_RAYS, spp in 1 .. SPIRA_MAX_SPP (radiance_check)
inline RadiancePlan make_radiance_plan(uint32_t n_rays, uint32_t spp, uint32_t num_cus, uint32_t block, const RadianceKnobs &k) {
    RadiancePlan p;
    p.n_rays = n_rays; p.spp = spp;
    p.max_items = std::min<uint32_t>(std::max<uint32_t>(1, k.max_items), kRadianceMaxItems);
    const uint32_t fit = std::max<uint32_t>(1, p.max_items / n_rays);              // samples of every ray the cap admits (1 even where it admits none: no workspace then)
    const uint32_t n_pass = (uint32_t)(((uint64_t)spp + std::min(fit, spp) - 1) / std::min(fit, spp));
    p.spp_pass = (spp + n_pass - 1) / n_pass;                                      // <= min(fit, spp)
    p.n_pass = (spp + p.spp_pass - 1) / p.spp_pass;
    p.direct = p.spp_pass == 1;
    p.ws_entries = p.direct ? 0 : (uint64_t)n_rays * p.spp_pass;
    p.wpb = std::max<uint32_t>(1, block / 64);
    const uint64_t max_blocks = k.waves_per_cu == 0 ? 1 : std::max<uint64_t>(1, (uint64_t)std::max<uint32_t>(1, num_cus) * k.waves_per_cu / p.wpb);
    const uint64_t items = (uint64_t)n_rays * p.spp_pass;
    p.grid = (uint32_t)std::min<uint64_t>(std::min<uint64_t>((items + block - 1) / block, max_blocks), 1u << 20);
    p.grid_flat = features_grid(n_rays, block, num_cus);
    return p;
}
// spira_camera_rays_*: everything but the pointers.  *rows_out: the rows generated (rows == 0: all).
inline int camera_rays_check(uint32_t model, uint32_t width, uint32_t height, uint32_t sample, uint32_t row0, uint32_t rows, double lens_radius,
                             uint32_t *rows_out, const char **msg) {
    if (model > 2u) { *msg = "spira_lens::model must be one of SPIRA_CAM_*"; return SPIRA_E_INVALID; }
    if (width < 2 || height < 2) { *msg = "width and height must be >= 2 (u = (i-1+rand)/(W-1))"; return SPIRA_E_INVALID; }
    if (!(lens_radius >= 0) || !(lens_radius - lens_radius == 0)) { *msg = "spira_lens::lens_radius must be finite and >= 0"; return SPIRA_E_INVALID; }
    if (rows != 0 && (uint64_t)row0 + rows > height) { *msg = "row0 + rows > height"; return SPIRA_E_INVALID; }      // (rows == 0: the whole image, row0 ignored, as in spira_params)
    if ((uint64_t)width * height > 0x7FFFFFFFull) { *msg = "image larger than 2^31 pixels"; return SPIRA_E_LIMIT; }
    if (sample >= SPIRA_MAX_SPP) { *msg = "sample index must be below 2^24"; return SPIRA_E_LIMIT; }
    const uint32_t r = rows ? rows : height;
    if ((uint64_t)r * width > SPIRA_MAX_RAYS) { *msg = "more than SPIRA_MAX_RAYS (2^26) rays: generate the image in row chunks"; return SPIRA_E_LIMIT; }
    *rows_out = r;
    return 0;
}

// ---- hemisphere gather at surface points (spira_scene_gather_*, spira_scene_gather_visible_*, spira_gather_rays_*); kernels in spira_gather.h.
// A work item is (point, sample), sample-minor, and a pass is split by samples under an item cap exactly as a radiance call's is: the plan IS
// make_radiance_plan's with the gather's own knobs.  n_points <= 2^26 and spp <= 2^24 multiply to 2^50 items in a call; no pass ever holds more than
// max(n_points, max_items) <= 2^26 of them, and every product here is formed in 64 bits.  The visibility entries split into the same passes and lay a
// CastPlan (make_cast_plan) over each pass's items for the session kernel.
struct GatherKnobs { uint32_t waves_per_cu = 64, max_items = kRadianceMaxItems; };      // SPIRA_GATHER_WAVES_PER_CU (0: one workgroup), SPIRA_GATHER_MAX_ITEMS
using GatherPlan = RadiancePlan;
// n_points in 1 .. SPIRA_MAX_RAYS, spp in 1 .. SPIRA_MAX_SPP (gather_check)
inline GatherPlan make_gather_plan(uint32_t n_points, uint32_t spp, uint32_t num_cus, uint32_t block, const GatherKnobs &k) {
    RadianceKnobs rk;
    rk.waves_per_cu = k.waves_per_cu; rk.max_items = k.max_items;
    return make_radiance_plan(n_points, spp, num_cus, block, rk);
}
// the session plan of one pass of a visibility gather: n_items of the pass, one workgroup where the gather's waves_per_cu is 0
inline CastPlan make_gather_visible_plan(uint32_t n_items, uint32_t num_cus, uint32_t block, const GatherKnobs &k, const CastKnobs &ck) {
    if (k.waves_per_cu != 0) return make_cast_plan(n_items, num_cus, block, ck);
    CastKnobs one = ck;
    one.waves_per_cu = std::max<uint32_t>(1, block / 64);
    CastPlan p = make_cast_plan(n_items, 1, block, one);
    p.grid_flat = 1;
    return p;
}
inline int gather_points_check(bool points, uint32_t n_points, uint32_t key0, const char **msg) {
    if (!points) { *msg = "the point array is NULL"; return SPIRA_E_INVALID; }
    if (n_points == 0) { *msg = "n_points is 0"; return SPIRA_E_INVALID; }
    if (n_points > SPIRA_MAX_RAYS) { *msg = "more than SPIRA_MAX_RAYS (2^26) points"; return SPIRA_E_LIMIT; }
    if ((uint64_t)key0 + n_points > (1ull << 32)) { *msg = "key0 + n_points exceeds 2^32"; return SPIRA_E_LIMIT; }
    return 0;
}
// spira_gather_rays_*
inline int gather_rays_check(bool points, bool rays, uint32_t n_points, uint32_t sample, uint32_t key0, const char **msg) {
    if (!rays) { *msg = "the ray array is NULL"; return SPIRA_E_INVALID; }
    if (int rc = gather_points_check(points, n_points, key0, msg)) return rc;
    if (sample >= SPIRA_MAX_SPP) { *msg = "sample index must be below 2^24"; return SPIRA_E_LIMIT; }
    return 0;
}
// spira_scene_gather_*: radiance_check's rules and order, on a point list
inline int gather_check(bool points, bool params, bool sums, uint32_t n_points, uint32_t spp, uint32_t max_depth, uint32_t flags, uint32_t sample0, uint32_t key0,
                        uint32_t reserved, const char **msg) {
    if (!points) { *msg = "the point array is NULL"; return SPIRA_E_INVALID; }
    if (!params) { *msg = "the spira_radiance struct is NULL"; return SPIRA_E_INVALID; }
    if (!sums) { *msg = "sum_rgb is NULL"; return SPIRA_E_INVALID; }
    if (n_points == 0) { *msg = "n_points is 0"; return SPIRA_E_INVALID; }
    if (spp == 0) { *msg = "spp is 0"; return SPIRA_E_INVALID; }
    if (max_depth < 1 || max_depth > SPIRA_MAX_DEPTH) { *msg = "max_depth must be 1 .. SPIRA_MAX_DEPTH (255)"; return SPIRA_E_INVALID; }
    if (reserved != 0) { *msg = "spira_radiance::reserved must be 0"; return SPIRA_E_INVALID; }
    if (flags & ~(SPIRA_EXT_DIELECTRIC | SPIRA_EXT_SPECTRAL)) { *msg = "flags: 0, SPIRA_EXT_DIELECTRIC and SPIRA_EXT_SPECTRAL are all the gather entries take"; return SPIRA_E_UNSUPPORTED; }
    if (int rc = gather_points_check(true, n_points, key0, msg)) return rc;
    if ((uint64_t)sample0 + spp > SPIRA_MAX_SPP) { *msg = "sample0 + spp exceeds 2^24"; return SPIRA_E_LIMIT; }
    return 0;
}
// spira_scene_probe_sh_*: gather_check's rules and order, on a list of points without normals (the codes are the gather's; two messages name the probe)
inline int probe_check(bool points, bool params, bool sums, uint32_t n_points, uint32_t spp, uint32_t max_depth, uint32_t flags, uint32_t sample0, uint32_t key0,
                       uint32_t reserved, const char **msg) {
    if (points && params && !sums) { *msg = "sum_sh is NULL"; return SPIRA_E_INVALID; }
    const int rc = gather_check(points, params, true, n_points, spp, max_depth, flags, sample0, key0, reserved, msg);
    if (rc == SPIRA_E_UNSUPPORTED) *msg = "flags: 0, SPIRA_EXT_DIELECTRIC and SPIRA_EXT_SPECTRAL are all the probe entries take";
    return rc;
}
// spira_scene_gather_visible_*
inline int gather_visible_check(bool points, bool params, bool counts, uint32_t n_points, uint32_t spp, uint32_t sample0, uint32_t key0, uint32_t flags,
                                double t_min, double t_max, const char **msg) {
    if (!points) { *msg = "the point array is NULL"; return SPIRA_E_INVALID; }
    if (!params) { *msg = "the spira_gather_visible struct is NULL"; return SPIRA_E_INVALID; }
    if (!counts) { *msg = "visible_u32 is NULL"; return SPIRA_E_INVALID; }
    if (n_points == 0) { *msg = "n_points is 0"; return SPIRA_E_INVALID; }
    if (spp == 0) { *msg = "spp is 0"; return SPIRA_E_INVALID; }
    if (t_min != t_min || t_max != t_max || t_min < 0 || t_max < t_min) { *msg = "t_min and t_max: no NaN, 0 <= t_min <= t_max (t_max may be +Inf)"; return SPIRA_E_INVALID; }
    if (flags & ~SPIRA_CAST_INPLACE) { *msg = "unknown flag bits (SPIRA_CAST_INPLACE is the only one)"; return SPIRA_E_INVALID; }
    if (int rc = gather_points_check(true, n_points, key0, msg)) return rc;
    if ((uint64_t)sample0 + spp > SPIRA_MAX_SPP) { *msg = "sample0 + spp exceeds 2^24"; return SPIRA_E_LIMIT; }
    return 0;
}

}  // namespace spira
