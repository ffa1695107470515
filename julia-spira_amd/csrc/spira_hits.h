// spira_hits.h — multi-hit ray queries on a scene handle (spira_scene_cast_hits_*): the first K hits of every ray of a caller's list, in order.
// Included by spira_hip.hip behind spira_nearest.h; built from spira_query.h (the ray preparation, cast_load, the refilled session's loop) and from
// spira_device.h (the scan's sphere and triangle arithmetic, the 8-wide tree and its trip).  No existing kernel is touched.  The first part of this file
// needs no HIP header: a CPU program (tests/native/hits_plan.cpp) calls the very function the kernels keep a lane's list with.
//
// The contract (include/spira_hip.h, "multi-hit ray queries").  Rays, their preparation, the invalid-ray rule and the origin rule are spira_scene_cast_*'s.
// Object k — spheres [0..) then triangles [0..) in the caller's order — is a CANDIDATE of a valid ray when the reference's per-object test (hit_sphere,
// hit_triangle; examples/julia-raytracer.jl:113-187) accepts it with the ray's own t_min and t_max; t_k is the t that test returns.  A sphere gives at most
// one candidate: the near root, or the far root when the near one lies below t_min.  The candidates are ordered by
//     t ascending, and among equal t by object index DESCENDING               (the later object first: the closest-hit scan's tie rule)
// and the answer is the first K = max_hits of that order.  The order is total (no two candidates share an index), so the order in which a walk meets the
// candidates cannot matter: the refilled sessions and the in-place walk give the same bytes, and K = 1 gives spira_scene_cast_*'s prim and t.
//
// Pruning.  Once a lane's list is full, an object is tested against the list's last t (the K-th hit so far) in place of the ray's t_max.  That is exact:
//   (a) the bits of an object's t do not depend on the bound it is tested against: both tests compute t first and compare afterwards (:130-132, :179);
//   (b) a candidate with t beyond the K-th t of ANY subset of the candidates is not among the first K of all of them: K candidates sort before it;
//   (c) a sphere whose near root lies beyond the bound has its far root beyond it too (-b + sq >= -b - sq over the same positive divisor, and a correctly
//       rounded division is monotone), so "beyond the bound" never hides a far root that would count — closest_hit_local's own argument;
//   (d) the bound only ever shrinks, and a candidate AT the bound (t == the K-th t) is still tested and accepted: hits_insert then decides by index.
// The tree prunes with the same bound through Bvh8Ray::best (rounded up, bvh8_best), as the closest-hit walk prunes with `closest`; while the list is not
// full, or under SPIRA_HITS_COUNT_ALL (where every candidate must be met to be counted), best stays what bvh8_enter made of t_max.
// The builder partitions the triangles: each sits in exactly one leaf, a walk meets it at most once, and no duplicate suppression is needed.
//
// Where a lane's list lives: in private arrays of a compile-time capacity CAP in {1, 4, 16}, the smallest that holds max_hits.  Capacities 1 and 4 are
// indexed by constants only and are registers; capacity 16 is indexed at run time and lives in scratch memory beside the tree walk's 256-byte stack.
// DESIGN.md section 13 has the resource table that decided it and what the alternatives (the wave's LDS, the output slots in global memory) would cost.
//
// Kernels (each stages the scene with stage_scene: one barrier; ExactDiv everywhere):
//   k_hits<T, BVH, TRI, CAP>     one lane per ray, grid-stride: hits_scan_local over the spheres and LDS triangles; BVH: then hits8_step to the end
//                                (SPIRA_CAST_INPLACE, or a scene without a tree).
//   k_hits_session<T, CAP>       scenes with a tree, the default: SPIRA_REFILLED_SESSION of spira_query.h over session_range of a CastPlan, the ray queries'
//                                knobs.  start = cast_load, hits_scan_local, bvh8_enter; step = hits8_step.  A finished lane's K slots and count go straight to
//                                out[ray], when the lane is next refilled or the session ends.
#pragma once
#include <cstdint>

#include "spira_query.h"        // SPIRA_HD

namespace spira {

constexpr uint32_t kHitsMax = 16;       // SPIRA_MAX_HITS

// One lane's list: n <= K <= CAP entries sorted by (t ascending, prim descending).
template <class T, int CAP> struct HitList {
    T t[CAP];
    int prim[CAP];
    uint32_t n;
};

// The order: t ascending, among equal t the later object first.  A NaN sorts before nothing and nothing sorts before it.
template <class T> SPIRA_HD inline bool hits_before(T ta, int pa, T tb, int pb) { return ta < tb || (ta == tb && pa > pb); }
constexpr int kHitsRegisterCap = 4;      // lists up to this capacity live in registers, larger ones in scratch memory (below)

// Inserts the candidate (t, prim) into a list of at most K entries (K <= CAP; K = 0: nothing is kept).  A full list drops its last entry — or the candidate,
// when that sorts after the last entry (t == the last t with a smaller index included).  Returns the pruning bound: the last entry's t when the list is
// full, else t_max.  A NaN t sorts before nothing: its place is the end of the list, where it is appended or dropped.  Two forms of one function:
//   CAP <= 4   on constant indices only, so that the list is registers: the candidate's place `pos` — the number of entries it does not sort before — is
//              found first; then slot j, from the last one down, takes its upper neighbour's entry (j > pos), the candidate (j == pos) or keeps its own.
//   CAP = 16   an insertion sort's inner loop on run-time indices, which keeps the list in scratch memory beside the walk's stack.  Both unrolled forms
//              that were tried at this capacity — the one above and a candidate carried down the list by compare-and-swap — hold 32 .. 48 VGPRs of list
//              (2 and 3 waves per SIMD in the sessions) and keep 16 steps' lane masks alive: 12 .. 88 spilled SGPRs in every capacity-16 kernel.
//              Entries at and beyond n are never read, so a list starts with n = 0 and nothing else.
template <class T, int CAP>
SPIRA_HD inline T hits_insert(HitList<T, CAP> &l, uint32_t K, T t, int prim, T t_max) {
    const uint32_t n = l.n;
    if constexpr (CAP > kHitsRegisterCap) {
        // the scratch-resident form: an insertion sort's inner loop on run-time indices
        if (K == 0) return t_max;
        uint32_t j = K - 1;
        if (n < K) { j = n; l.n = n + 1; }
        else if (!hits_before<T>(t, prim, l.t[j], l.prim[j])) return l.t[j];      // a full list and the candidate sorts after its last entry: dropped
#if defined(__HIPCC__)
#pragma nounroll
#endif
        while (j > 0 && hits_before<T>(t, prim, l.t[j - 1], l.prim[j - 1])) { l.t[j] = l.t[j - 1]; l.prim[j] = l.prim[j - 1]; --j; }
        l.t[j] = t; l.prim[j] = prim;
        return l.n == K ? l.t[K - 1] : t_max;
    }
    uint32_t pos = 0;
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int j = 0; j < CAP; ++j) {
        const bool before = hits_before<T>(t, prim, l.t[j], l.prim[j]);
        pos += ((uint32_t)j < n && !before) ? 1u : 0u;
    }
    const uint32_t top = n < K ? n : K - 1;          // the last slot written (K = 0: 2^32 - 1, and j < K below holds for no slot)
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int j = CAP - 1; j >= 0; --j) {
        const bool live = (uint32_t)j < K && (uint32_t)j <= top;
        if (j > 0) {
            const bool shift = live && (uint32_t)j > pos;
            l.t[j] = shift ? l.t[j - 1] : l.t[j];
            l.prim[j] = shift ? l.prim[j - 1] : l.prim[j];
        }
        const bool here = live && (uint32_t)j == pos;
        l.t[j] = here ? t : l.t[j];
        l.prim[j] = here ? prim : l.prim[j];
    }
    if (n < K) l.n = n + 1;
    T bound = t_max;
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int j = 0; j < CAP; ++j)
        if ((uint32_t)j + 1 == K && l.n == K) bound = l.t[j];
    return bound;
}

}  // namespace spira

#if defined(__HIPCC__)
namespace spira {

// CastArgs' scene, rays, n_rays, base / rem / refill_free as they are (cast_load and launch_list read them); prim and t are n_rays x max_hits, ray-major.
template <class T> struct HitsArgs : CastArgs<T> {
    uint32_t *count;                 // n_rays; may be NULL (as prim and t)
    uint32_t max_hits;               // K: 0 .. CAP of the kernel launched
    uint32_t count_all;              // SPIRA_HITS_COUNT_ALL: count every candidate, prune with t_max only
};

// One lane's query state beside the ray: the list, the candidates met, and the bound an object is tested against.
template <class T, int CAP> struct HitsLane {
    HitList<T, CAP> l;
    uint32_t total;                  // candidates accepted by the tests so far (all of them under COUNT_ALL)
    T bound, t_max;
};

template <class T, int CAP> __device__ __forceinline__ void hits_begin(HitsLane<T, CAP> &h, T t_max) {
    if constexpr (CAP <= kHitsRegisterCap) {
#pragma unroll
        for (int j = 0; j < CAP; ++j) { h.l.t[j] = t_max; h.l.prim[j] = SPIRA_RAY_MISS; }
    }
    h.l.n = 0; h.total = 0; h.bound = t_max; h.t_max = t_max;
}

// An accepted candidate.  true: the list is full and the bound is its last t — a walk recomputes Bvh8Ray::best from it.
template <class T, int CAP>
__device__ __forceinline__ bool hits_take(HitsLane<T, CAP> &h, uint32_t K, bool count_all, T t, int prim) {
    ++h.total;
    const T b = hits_insert<T, CAP>(h.l, K, t, prim, h.t_max);
    if (count_all) return false;
    h.bound = b;
    return h.l.n == K;
}

// Unused slots: SPIRA_RAY_MISS and t_max copied; every slot of an invalid ray: SPIRA_RAY_INVALID and 0.  count: the slots filled, or every candidate.
template <class T, int CAP>
__device__ __forceinline__ void hits_store(const HitsArgs<T> &a, uint32_t ray, bool valid, const HitsLane<T, CAP> &h) {
    const uint32_t K = a.max_hits;
    const size_t at = (size_t)ray * K;
    const auto slot = [&](uint32_t j, int lp, T lt) {
        const bool used = j < h.l.n;                 // (an invalid ray's list is empty)
        if (a.prim) a.prim[at + j] = used ? lp : (valid ? SPIRA_RAY_MISS : SPIRA_RAY_INVALID);
        if (a.t) a.t[at + j] = used ? lt : (valid ? h.t_max : (T)0);
    };
    if constexpr (CAP <= kHitsRegisterCap) {
#pragma unroll
        for (int j = 0; j < CAP; ++j)
            if ((uint32_t)j < K) slot((uint32_t)j, h.l.prim[j], h.l.t[j]);
    } else {
        // the scratch-resident list: a run-time loop over its slots, the filled ones read, the others not
#pragma nounroll
        for (uint32_t j = 0; j < K; ++j) {
            int lp = 0; T lt = 0;
            if (j < h.l.n) { lp = h.l.prim[j]; lt = h.l.t[j]; }
            slot(j, lp, lt);
        }
    }
    if (a.count) a.count[ray] = !valid ? 0u : (a.count_all ? h.total : h.l.n);
}

// The LDS part: EVERY sphere and LDS triangle in order, each tested against the lane's current bound with the scan's own arithmetic — the sphere test is
// closest_hit_local's, operation by operation (ExactDiv, the same root_* helpers), with the bound in the place of `closest`; triangle_test as it is.
template <class T, bool TRI, int CAP>
__device__ __forceinline__ void hits_scan_local(const SceneLds<T> &sc, Vec<T> o, Vec<T> d, T t_min, HitsLane<T, CAP> &h, uint32_t K, bool count_all) {
    ExactDiv pol;
    const T a = dot(d, d);                                     // :115
    const T two_a = (T)2.0 * a;
    const T four_a = (T)4 * a;
    const RootDiv<T> over_2a = root_divisor<T>(two_a, pol);
    root_t_min<T>(t_min, pol);
    Pack4<T> c_next = sc.sph[0];           // (slot 0 always exists in the LDS image)
    for (uint32_t s = 0; s < sc.n_spheres; ++s) {
        const Pack4<T> c = c_next;
        c_next = sc.sph[s + 1 < sc.n_spheres ? s + 1 : s];
        const Vec<T> oc = o - mk<T>(c.x, c.y, c.z);            // :114
        const T cc = dot(oc, oc) - c.w;                        // :117
        const T b = (T)2.0 * dot(oc, d);                       // :116
        const T bb = b * b;
        const T disc = bb - four_a * cc;                       // :118
        if (!(disc < 0)) {                                     // :120
            root_operands<T>(bb, disc, pol);
            const T sq = root_sqrt<T>(disc, pol);              // :125
            T root = root_over<T>(-b - sq, over_2a, pol);      // :126
            bool ok = !(root < t_min || root > h.bound);       // :130
            if (!ok && root < t_min) {                         // :127, :131-132 (a near root beyond the bound: the far one is too)
                root = root_over<T>(-b + sq, over_2a, pol);
                ok = !(root < t_min || root > h.bound);
            }
            if (ok) hits_take<T, CAP>(h, K, count_all, root, (int)s);
        }
    }
    if (TRI && sc.n_triangles) {
        Pack4<T> v0n = sc.tri[0], e1n = sc.tri[1], e2n = sc.tri[2];
        for (uint32_t i = 0; i < sc.n_triangles; ++i) {
            const Pack4<T> v0 = v0n, e1 = e1n, e2 = e2n;
            const uint32_t nx = i + 1 < sc.n_triangles ? i + 1 : i;
            v0n = sc.tri[3 * nx]; e1n = sc.tri[3 * nx + 1]; e2n = sc.tri[3 * nx + 2];
            T t;
            if (triangle_test<T>(v0, e1, e2, o, d, t_min, h.bound, t, pol)) hits_take<T, CAP>(h, K, count_all, t, (int)(sc.n_spheres + i));
        }
    }
}

// The leaf arm of a trip: the scan's own test of one tree triangle against the lane's bound; after an insertion into a full list the Float32 side's
// bound follows the new K-th t, as the closest-hit leaf's follows `closest`.
template <class T, int CAP>
__device__ __forceinline__ void hits8_leaf(const SceneLds<T> &sc, const Bvh8Walk<T> &w, Bvh8Ray &r, Vec<T> o, Vec<T> d, T t_min, int base, const Pack4<T> v0, const Pack4<T> e1,
                                           const Pack4<T> e2, HitsLane<T, CAP> &h, uint32_t K, bool count_all) {
    T t;
    if (triangle_test<T>(v0, e1, e2, o, d, t_min, h.bound, t)) {
        const int p = base + (int)Bits<T>::to_u32(v0.w);
        if (hits_take<T, CAP>(h, K, count_all, t, p)) r.best = bvh8_best((float)((h.bound - w.t0) * sc.bvh_root[2].w));
    }
}

// One trip of the multi-hit walk: bvh8_trip (spira_device.h) over the same Bvh8Walk, stack and node test as the closest-hit walk, with hits8_leaf as its
// leaf arm.  The Float32-screen experiment of the closest-hit walk is not carried over: Float64 tests every triangle exactly where it is met.  Returns
// false when the walk is over.
template <class T, int KL, int CAP>
__device__ __forceinline__ bool hits8_step(const SceneLds<T> &sc, Bvh8Walk<T> &w, Bvh8Ray &r, Vec<T> o, Vec<T> d, T t_min, int base, HitsLane<T, CAP> &h, uint32_t K, bool count_all,
                                           uint32_t *lds_stack, uint32_t *stack, uint32_t lane) {
    return bvh8_trip<T, KL>(sc, w, r, lds_stack, stack, lane, [&](uint32_t, const Pack4<T> v0, const Pack4<T> e1, const Pack4<T> e2) {
        hits8_leaf<T, CAP>(sc, w, r, o, d, t_min, base, v0, e1, e2, h, K, count_all);
    });
}

// One lane per ray.  Launches: <T, false, false, .> spheres alone, <T, false, true, .> with LDS triangles, <T, true, false, .> a BVH mesh (SPIRA_CAST_INPLACE).
template <class T, bool BVH, bool TRI, int CAP>
__global__ __launch_bounds__(kBlock) void k_hits(const HitsArgs<T> a) {
    extern __shared__ __attribute__((aligned(32))) unsigned char lds_raw[];
    const SceneLds<T> sc = stage_scene<T>(a.scene, lds_raw);     // the only workgroup barrier of the kernel
    const uint32_t K = a.max_hits;
    const bool count_all = a.count_all != 0;
    const int base = (int)(sc.n_spheres + sc.n_triangles);
    for (uint32_t i = blockIdx.x * kBlock + threadIdx.x; i < a.n_rays; i += gridDim.x * kBlock) {
        Vec<T> o, d; T t_min, t_max;
        const bool ok = cast_load<T>(a, sc, BVH, i, o, d, t_min, t_max);
        HitsLane<T, CAP> h;
        hits_begin<T, CAP>(h, t_max);
        if (ok) {
            hits_scan_local<T, TRI, CAP>(sc, o, d, t_min, h, K, count_all);
            if (BVH) {
                Bvh8Ray r; T t0;
                if (bvh8_enter<T>(sc, o, d, h.bound, r, t0)) {
                    Bvh8Walk<T> w;
                    bvh8_begin<T>(w, r, t0, t_min, sc.bvh_root[2].w);
                    uint32_t stack[kBvhStackD];
                    while (hits8_step<T, 0, CAP>(sc, w, r, o, d, t_min, base, h, K, count_all, nullptr, stack, threadIdx.x & 63)) {}
                }
            }
        }
        hits_store<T, CAP>(a, i, ok, h);
    }
}

// Scenes with a tree: a refilled session per wave over its range of the caller's list (SPIRA_REFILLED_SESSION of spira_query.h).
template <class T, int CAP>
__global__ __launch_bounds__(kBlock) void k_hits_session(const HitsArgs<T> a) {
    constexpr int KL = kCastLdsStack;
    extern __shared__ __attribute__((aligned(32))) unsigned char lds_raw[];
    const SceneLds<T> sc = stage_scene<T>(a.scene, lds_raw);     // the only workgroup barrier of the kernel
    uint32_t begin, end;
    session_range(a.base, a.rem, begin, end);
    uint32_t *lstack = session_lstack<T>(lds_raw, a.scene);
    uint32_t stack[kBvhStackD - KL];
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t K = a.max_hits;
    const bool count_all = a.count_all != 0;
    const int base = (int)(sc.n_spheres + sc.n_triangles);
    uint32_t ray = 0;
    Vec<T> o = mk<T>(0, 0, 0), d = mk<T>(0, 0, 1);
    T t_min = 0;
    HitsLane<T, CAP> h;
    hits_begin<T, CAP>(h, (T)0);
    Bvh8Ray ry{};
    Bvh8Walk<T> wk{};
    // A lane that finishes its walk does not store at once: with K slots to write, one lane storing while the other 63 wait made the sessions slower than
    // the in-place walk at K >= 4 (docs/experiments.md section 33).  Its answer stays in `h` until the lane is refilled — all the lanes of a refill store
    // together — or until the session ends.
    bool pending = false;
    const auto start = [&](uint32_t item) -> bool {
            if (pending) { hits_store<T, CAP>(a, ray, true, h); pending = false; }
            ray = item;
            T t_max;
            const bool ok = cast_load<T>(a, sc, true, ray, o, d, t_min, t_max);
            hits_begin<T, CAP>(h, t_max);
            bool walks = false;
            if (ok) {
                hits_scan_local<T, false, CAP>(sc, o, d, t_min, h, K, count_all);
                T t0;
                if (bvh8_enter<T>(sc, o, d, h.bound, ry, t0)) { bvh8_begin<T>(wk, ry, t0, t_min, sc.bvh_root[2].w); walks = true; }
            }
            if (!walks) hits_store<T, CAP>(a, ray, ok, h);
            return walks;
    };
    const auto step = [&]() -> bool {
            if (hits8_step<T, KL, CAP>(sc, wk, ry, o, d, t_min, base, h, K, count_all, lstack, stack, lane)) return true;
            pending = true;
            return false;
    };
    SPIRA_REFILLED_SESSION(begin, end, a.refill_free, start, step);
    if (pending) hits_store<T, CAP>(a, ray, true, h);
}

}  // namespace spira
#endif
