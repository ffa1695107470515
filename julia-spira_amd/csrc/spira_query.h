// spira_query.h — ray queries on a scene handle (spira_scene_cast_* / spira_scene_occluded_*): closest hit and occlusion for a caller's own ray list.
// Included by spira_hip.hip behind spira_device.h, whose device functions (scene staging, the LDS scan, the 8-wide BVH walk) the kernels are built from;
// no render kernel is touched.  Launch arithmetic: spira_plan.h (make_cast_plan).  The first part of this file needs no HIP header: a CPU program
// (tests/native/cast_plan.cpp) calls the very function the kernels classify and normalise a ray with.
//
// A ray is eight values of the call's precision T: [ox oy oz t_min dx dy dz t_max].  Preparation, in T, nothing fused (-ffp-contract=off):
//     s = (dx dx + dy dy) + dz dz,   d = (dx, dy, dz) / sqrt(s)            (normalize of spira_device.h; the walk assumes unit directions)
// t, t_min and t_max are distances along the unit direction.  The answer is the reference's scan (examples/julia-raytracer.jl:242-258) over spheres
// [0..) then triangles [0..) in the caller's order with `closest` starting at t_max: minimal t, ties to the later object, a hit at exactly t_max counts.
// A ray is INVALID (prim SPIRA_RAY_INVALID, t 0, normal 0; occlusion 255) when any of its eight values is NaN, an origin or direction component is
// infinite, s is not finite or below the smallest normal number of T, t_min < 0, t_max < t_min, or — scenes with a tree only — the origin rule fails:
//     |(o_k - centre_k) * scale| <= 64   on every axis k, evaluated in T with the frame packet {centre, scale} of the tree
// Why 64.  bvh8_enter computes the point where the ray enters the mesh's box, o + d te, in T: its error is a few ulps of max(|o_k|, te), and the Float32
// side of the walk starts from that point.  In normalised units (times scale) |o_k| <= amax_n + 64 and te <= the distance to a box about one unit wide,
// so every term of o_k + d_k te is below about amax_n + 64 + 111 d_k; three roundings (product, sum, the subtraction of the centre) give in Float32
//     error <= about 3 (amax_n + 64) 2^-24 = 1.2e-5 + 1.8e-7 amax_n
// against the builder's pad (spira_bvh.h, "Padding") of 1e-4 max(1, amax_n): a margin of 8 at amax_n <= 1, of more than 50 for a mesh far from the origin.
// A refitted tree pads with the bound A = max_k |centre_k| + 1 / scale in place of amax (spira_refit.h, refit_pad): A_n >= amax_n for every mesh inside
// the frame, so that pad is never the smaller one and the margin of the fresh build is the one that binds; 64 serves both.  In Float64 the error is
// 3 (amax_n + 64) 2^-53 against 1e-4 + 1e-9 amax_n: eleven orders of magnitude under.  A caller further away than 64 mesh sizes moves its origin along
// the ray (o' = o + d t0, t_min and t_max less t0) — or the scene has no tree (at most SPIRA_LDS_TRIANGLES triangles), where there is no rule.
// Valid origins at 60 .. 64 units, their twins just beyond the bound and the refitted and rebuilt trees are held to the scan by tests/test_gpu_cast_edges.py.
//
// Kernels (each stages the scene with stage_scene: one barrier; ExactDiv everywhere — the compiler's division and square root):
//   k_cast<T, BVH, TRI, ANY>      one lane per ray, grid-stride.  BVH = false: scenes without a tree, the LDS scan alone.  BVH = true: the plain
//                                 organisation SPIRA_CAST_INPLACE, bvh_closest_hit to the end as k_features walks — the comparison point.
//   k_cast_session<T, ANY>        scenes with a tree, the default: persistent waves, each owning one contiguous range of the ray list (CastPlan), run
//                                 a refilled traversal session over it — k_path's idea (spira_device.h, "traversal sessions") for this data flow: a free
//                                 lane takes the next ray of the range (ballot / popcount prefix, a wave-uniform `next`), prepares it, runs the LDS scan,
//                                 enters the tree; all walking lanes take bvh8_step trips together; the walk loop is left when refill_free lanes are free
//                                 and rays remain, or none walks.  A finished lane stores straight to out[ray]: no compaction, no queue.
//                                 The same loop runs k_nearest_session (spira_nearest.h) and k_gather_visible_session (spira_gather.h): for those two it
//                                 is written once, SPIRA_REFILLED_SESSION below, with the helpers session_range and session_lstack.
//   ANY = true                    occlusion: only `hit` is written; a lane whose LDS scan hit never walks, a walking lane leaves after the first trip that
//                                 set prim >= 0.
// Both organisations run the scan's own leaf test on the same values — the tree only prunes — so they give identical bytes.
#pragma once
#include <cstdint>

#include "spira_fastdiv.h"      // SPIRA_HD

namespace spira {

template <class T> struct CastLimits;
template <> struct CastLimits<float> { static constexpr float min_normal = 1.17549435e-38f; };
template <> struct CastLimits<double> { static constexpr double min_normal = 2.2250738585072014e-308; };
constexpr int kCastOriginBound = 64;      // the origin rule, see above

// One ray r[0..8) -> valid?  d: the unit direction (written for valid rays only).  frame: the scene has a tree, fr = {centre.x, centre.y, centre.z, scale}.
template <class T> SPIRA_HD inline bool cast_ray_prepare(const T *r, bool frame, const T *fr, T d[3]) {
    bool finite = true;
    for (int k = 0; k < 8; ++k) if (r[k] != r[k]) return false;                     // NaN anywhere
    for (int k = 0; k < 7; ++k) if (k != 3 && !((r[k] - r[k]) == (T)0)) finite = false;      // an infinite origin or direction component
    if (!finite) return false;
    const T s = (r[4] * r[4] + r[5] * r[5]) + r[6] * r[6];
    if (!((s - s) == (T)0) || s < CastLimits<T>::min_normal) return false;
    if (r[3] < (T)0 || r[7] < r[3]) return false;
    if (frame)
        for (int k = 0; k < 3; ++k) {
            const T x = (r[k] - fr[k]) * fr[3];
            if (!(x >= (T)-kCastOriginBound && x <= (T)kCastOriginBound)) return false;
        }
    T len;
    if constexpr (sizeof(T) == 4) len = __builtin_sqrtf(s); else len = __builtin_sqrt(s);
    d[0] = r[4] / len; d[1] = r[5] / len; d[2] = r[6] / len;
    return true;
}

}  // namespace spira

#if defined(__HIPCC__)
// Refill threshold and waves per CU of the session kernel, started from k_path's knobs (SPIRA_MESH_REFILL 16, SPIRA_MESH_FAT_WAVES_PER_CU 16) and swept
// on the device (docs/experiments.md section 26): 16 free lanes is the best threshold or within the spread of it on every set; 20 waves per CU — what a CU
// holds of the Float64 kernel (5 per SIMD) — is the best or within 1 % of it on every set, and the one count at which the sessions beat the in-place walk
// on coherent camera rays in Float64 too.  Both are also read from the environment per call, under the same names.
#ifndef SPIRA_CAST_REFILL
#define SPIRA_CAST_REFILL 16
#endif
#ifndef SPIRA_CAST_WAVES_PER_CU
#define SPIRA_CAST_WAVES_PER_CU 20
#endif
// stack levels of a session lane kept in the wave's LDS scratch ([level][lane]) instead of registers / scratch memory: 0 = none
#ifndef SPIRA_CAST_LDS_STACK
#define SPIRA_CAST_LDS_STACK 0
#endif

namespace spira {

constexpr int kCastLdsStack = SPIRA_CAST_LDS_STACK;

template <class T> struct CastArgs {
    SceneGlobal<T> scene;
    const T *rays;                   // n_rays x 8
    uint32_t n_rays;
    int *prim; T *t; T *normal;      // closest hit: n_rays, n_rays, n_rays x 3 (interleaved); any may be NULL
    uint8_t *hit;                    // occlusion (ANY): n_rays
    uint32_t base, rem;              // session: wave w owns base + (w < rem) rays from w base + min(w, rem)  (CastPlan)
    uint32_t refill_free;
};

template <class T, bool BVH, bool TRI, bool ANY>
__device__ __forceinline__ void cast_store(const CastArgs<T> &a, const SceneLds<T> &sc, uint32_t ray, bool valid, int prim, T closest, T t_max, Vec<T> o, Vec<T> d, uint32_t slot) {
    if (ANY) { a.hit[ray] = valid ? (prim >= 0 ? (uint8_t)1 : (uint8_t)0) : (uint8_t)255; return; }
    if (a.prim) a.prim[ray] = valid ? prim : SPIRA_RAY_INVALID;
    if (a.t) a.t[ray] = !valid ? (T)0 : (prim >= 0 ? closest : t_max);
    if (a.normal) {
        Vec<T> n = mk<T>(0, 0, 0);
        if (valid && prim >= 0) n = feature_normal<T, BVH, TRI>(sc, o + d * closest, prim, slot);
        a.normal[3 * (size_t)ray] = n.x; a.normal[3 * (size_t)ray + 1] = n.y; a.normal[3 * (size_t)ray + 2] = n.z;
    }
}

// The LDS part of a valid ray's scan.  closest_hit_local is used as it is and starts at +Inf; a result beyond t_max is discarded afterwards.  That equals
// the scan started at t_max: restricting the candidates to t <= t_max cannot change which one is minimal (or, among equal t, which one is last) when
// the minimum lies within t_max, and when it does not, no candidate does.  Out: closest = min(hit, t_max) — what the tree walk may still improve on.
template <class T, bool TRI>
__device__ __forceinline__ void cast_scan_local(const SceneLds<T> &sc, Vec<T> o, Vec<T> d, T t_min, T t_max, T &closest, int &prim) {
    ExactDiv exact;
    closest_hit_local<T, ExactDiv, TRI>(sc, o, d, t_min, closest, prim, exact);
    if (closest > t_max) { prim = -1; closest = t_max; }
}

template <class T>
__device__ __forceinline__ bool cast_load(const CastArgs<T> &a, const SceneLds<T> &sc, bool frame, uint32_t ray, Vec<T> &o, Vec<T> &d, T &t_min, T &t_max) {
    const T *rp = a.rays + 8 * (size_t)ray;
    T r[8], dd[3] = {(T)0, (T)0, (T)0}, fr[4] = {(T)0, (T)0, (T)0, (T)1};
#pragma unroll
    for (int k = 0; k < 8; ++k) r[k] = rp[k];
    if (frame) { const Pack4<T> f = sc.bvh_root[2]; fr[0] = f.x; fr[1] = f.y; fr[2] = f.z; fr[3] = f.w; }
    const bool ok = cast_ray_prepare<T>(r, frame, fr, dd);
    o = mk<T>(r[0], r[1], r[2]); d = mk<T>(dd[0], dd[1], dd[2]); t_min = r[3]; t_max = r[7];
    return ok;
}

// One lane per ray.  Launches: <T, false, false, .> spheres alone, <T, false, true, .> with LDS triangles, <T, true, false, .> a BVH mesh (SPIRA_CAST_INPLACE).
template <class T, bool BVH, bool TRI, bool ANY>
__global__ __launch_bounds__(kBlock) void k_cast(const CastArgs<T> a) {
    extern __shared__ __attribute__((aligned(32))) unsigned char lds_raw[];
    const SceneLds<T> sc = stage_scene<T>(a.scene, lds_raw);     // the only workgroup barrier of the kernel
    for (uint32_t i = blockIdx.x * kBlock + threadIdx.x; i < a.n_rays; i += gridDim.x * kBlock) {
        Vec<T> o, d; T t_min, t_max;
        const bool ok = cast_load<T>(a, sc, BVH, i, o, d, t_min, t_max);
        T closest = 0; int prim = -1; uint32_t slot = 0;
        if (ok) {
            cast_scan_local<T, TRI>(sc, o, d, t_min, t_max, closest, prim);
            if (BVH) bvh_closest_hit<T>(sc, o, d, t_min, closest, prim, slot);
        }
        cast_store<T, BVH, TRI, ANY>(a, sc, i, ok, prim, closest, t_max, o, d, slot);
    }
}

// A wave's range of a list split by a CastPlan: wave w owns base + (w < rem) items from w base + min(w, rem).
__device__ __forceinline__ void session_range(uint32_t base, uint32_t rem, uint32_t &begin, uint32_t &end) {
    const uint32_t wid = blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6);
    begin = wid * base + (wid < rem ? wid : rem); end = begin + base + (wid < rem ? 1u : 0u);
}
// The wave's LDS stack levels ([level][lane], kCastLdsStack of them) behind the staged scene: what bvh8_step takes as lstack.
template <class T>
__device__ __forceinline__ uint32_t *session_lstack(unsigned char *lds_raw, const SceneGlobal<T> &g) {
    return reinterpret_cast<uint32_t *>(lds_raw + scene_lds_bytes<T>(g.n_spheres, g.n_materials, g.n_triangles)) + (size_t)(threadIdx.x >> 6) * (kCastLdsStack > 0 ? kCastLdsStack : 1) * 64;
}

// The refilled session of one wave over the items [begin, end) — the loop of k_nearest_session and k_gather_visible_session (and k_cast_session's, which keeps its own copy below), and nothing
// else: the lane's query (ray or point, closest and prim, the walk, the stack) stays in the kernel, in locals the two callables capture by reference.
//   start(item) -> bool    a free lane takes `item`: loads and classifies it, scans LDS, tries to enter the tree.  true: the lane now walks; false: it
//                          finished at once and has stored its answer itself.
//   step() -> bool         one trip of a walking lane.  false: that was its last — the answer is stored, the lane is free.
// Free lanes take the next items in index order (ballot / popcount prefix; `next` is wave-uniform); the walk loop is left when refill_free lanes are
// free and items remain, or when nobody walks.
// A macro, not a function template, on a measurement (docs/experiments.md section 32): a function holding this loop is simplified on its own
// before it is inlined into the kernel, with the lane's state behind the closures' pointers; the values forwarded there stay beside the registers the
// kernel's locals become — 10 more VGPRs in Float64, one occupancy step, 10 % of the rays per second.  Expanded in the kernel it compiles as written out.
#define SPIRA_REFILLED_SESSION(begin, end, refill_free, start, step)                                                                         \
    do {                                                                                                                                     \
        const unsigned long long lt_mask_ = (1ull << (threadIdx.x & 63)) - 1ull;                                                             \
        const uint32_t end_ = (end), refill_free_ = (refill_free);                                                                           \
        uint32_t next_ = (begin);                                /* wave-uniform: the next item of the range nobody has taken */            \
        bool walking_ = false;                                                                                                               \
        while (true) {                                                                                                                       \
            /* ---- refill: the free lanes take the next items of the range, in index order */                                             \
            const unsigned long long mf_ = __ballot(!walking_);                                                                              \
            const uint32_t n_free_ = (uint32_t)__popcll(mf_), rank_ = (uint32_t)__popcll(mf_ & lt_mask_);                                    \
            const uint32_t take_ = min(n_free_, end_ - next_);                                                                               \
            if (!walking_ && rank_ < take_) walking_ = start(next_ + rank_);                                                                 \
            next_ += take_;                                                                                                                  \
            if (!__any(walking_)) { if (next_ < end_) continue; break; }                                                                     \
            /* ---- walk; leave the loop when enough lanes are free for a refill to pay (or, with the range exhausted, when all are done) */ \
            const bool more_ = next_ < end_;                                                                                                 \
            while (true) {                                                                                                                   \
                if (walking_) walking_ = step();                                                                                             \
                const uint32_t n_walk_ = (uint32_t)__popcll(__ballot(walking_));                                                             \
                if (n_walk_ == 0 || (more_ && 64u - n_walk_ >= refill_free_)) break;                                                         \
            }                                                                                                                                \
        }                                                                                                                                    \
    } while (0)

// Scenes with a tree: a refilled traversal session per wave over its range of the caller's list.  The loop is written out here and not taken from SPIRA_REFILLED_SESSION:
// with the macro the closest-hit Float32 instantiation lost 1.5 % on coherent camera rays (docs/experiments.md section 32.4); a change to the loop's exits
// is made in both places.
template <class T, bool ANY>
__global__ __launch_bounds__(kBlock) void k_cast_session(const CastArgs<T> a) {
    constexpr int KL = kCastLdsStack;
    extern __shared__ __attribute__((aligned(32))) unsigned char lds_raw[];
    const SceneLds<T> sc = stage_scene<T>(a.scene, lds_raw);     // the only workgroup barrier of the kernel
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint32_t wid = blockIdx.x * (kBlock / 64) + wave;
    const uint32_t begin = wid * a.base + (wid < a.rem ? wid : a.rem), end = begin + a.base + (wid < a.rem ? 1u : 0u);
    uint32_t *lstack = reinterpret_cast<uint32_t *>(lds_raw + scene_lds_bytes<T>(a.scene.n_spheres, a.scene.n_materials, a.scene.n_triangles)) + (size_t)wave * (KL > 0 ? KL : 1) * 64;
    uint32_t stack[kBvhStackD - KL];
    const unsigned long long lt_mask = (1ull << lane) - 1ull;
    const int base = (int)(sc.n_spheres + sc.n_triangles);
    uint32_t next = begin;                                       // wave-uniform: the next ray of the range nobody has taken
    bool walking = false;
    uint32_t ray = 0, slot = 0;
    Vec<T> o = mk<T>(0, 0, 0), d = mk<T>(0, 0, 1);
    T t_min = 0, t_max = 0, closest = 0;
    int prim = -1;
    Bvh8Ray ry{};
    Bvh8Walk<T> wk{};
    while (true) {
        // ---- refill: the free lanes take the next rays of the range, in index order
        const unsigned long long mf = __ballot(!walking);
        const uint32_t n_free = (uint32_t)__popcll(mf), rank = (uint32_t)__popcll(mf & lt_mask);
        const uint32_t take = min(n_free, end - next);
        if (!walking && rank < take) {
            ray = next + rank;
            const bool ok = cast_load<T>(a, sc, true, ray, o, d, t_min, t_max);
            prim = -1; slot = 0; closest = 0;
            bool done = true;
            if (ok) {
                cast_scan_local<T, false>(sc, o, d, t_min, t_max, closest, prim);
                T t0;
                if (!(ANY && prim >= 0) && bvh8_enter<T>(sc, o, d, closest, ry, t0)) { bvh8_begin<T>(wk, ry, t0, t_min, sc.bvh_root[2].w); walking = true; done = false; }
            }
            if (done) cast_store<T, true, false, ANY>(a, sc, ray, ok, prim, closest, t_max, o, d, slot);
        }
        next += take;
        if (!__any(walking)) { if (next < end) continue; break; }
        // ---- walk; leave the loop when enough lanes are free for a refill to pay (or, with the range exhausted, when all are done)
        const bool more = next < end;
        while (true) {
            if (walking) {
                bool on = bvh8_step<T, KL>(sc, wk, ry, o, d, t_min, base, closest, prim, slot, lstack, stack, lane);
                if (ANY && prim >= 0) on = false;                // occlusion: the first accepted hit ends the walk (pending Float64 candidates are dropped)
                if (!on) {
                    // the screened Float64 walk (experiment build): its pending candidates are resolved before the lane counts as finished
                    if (!(ANY && prim >= 0)) while (wk.nc) bvh8_resolve_one<T>(sc, wk, ry, o, d, t_min, base, closest, prim, slot);
                    walking = false;
                    cast_store<T, true, false, ANY>(a, sc, ray, true, prim, closest, t_max, o, d, slot);
                }
            }
            const uint32_t n_walk = (uint32_t)__popcll(__ballot(walking));
            if (n_walk == 0 || (more && 64u - n_walk >= a.refill_free)) break;
        }
    }
}

}  // namespace spira
#endif
