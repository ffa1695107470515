// spira_knearest.h — K-nearest point queries on a scene handle (spira_scene_nearest_k_*): for every point of a caller's list, the K closest objects in order.
// Included by spira_hip.hip behind spira_hits.h; built from spira_nearest.h (the point preparation, the two closest-point functions, near_load, near_enter,
// near_node, the distance walk's state and stack) and from spira_hits.h (the order, hits_before).  No existing kernel is touched.  The first part of this
// file needs no HIP header: a CPU program (tests/native/knearest_plan.cpp) calls the very functions the kernels keep a lane's list with.
//
// The contract (include/spira_hip.h, "K-nearest point queries").  Points, the validity rule and the origin rule are spira_scene_closest_point_*'s.
// Object k — spheres [0..) then triangles [0..) in the caller's order — is a CANDIDATE of a valid point when d2_k <= best0, best0 = r_max * r_max in T;
// d2_k and q_k are what closest_point_sphere / closest_point_triangle give on the values the LDS records and the tree's records hold (a sphere's radius
// from spheres5); a NaN d2 is never a candidate.  The candidates are ordered by
//     d2 ascending, and among equal d2 by object index DESCENDING              (the later object first: the closest-point scan's tie rule)
// and the answer is the first K = max_near of that order.  The order is total (no two candidates share an index), so the order in which a walk meets the
// candidates cannot matter: the refilled sessions and the in-place walk give the same bytes, and K = 1 gives spira_scene_closest_point_*'s answer.
//
// Pruning.  bound = best0 until the lane's list holds K entries, then the list's last d2 (the K-th so far); under SPIRA_NEAR_COUNT_ALL it stays best0.
// An object met — in LDS or in a leaf — is a candidate when d2 <= bound; near_insert places it by index.  The tree step is near_trip with `bound` in the
// place of `best`: bestn = near_bestn(bound, scale), recomputed whenever the list is full after an insertion; near_node's strict test, the nearest
// surviving child first and the one deferred-children entry per node are as they are, so the stack bound (one entry per level) is unchanged.  Exact:
//   (1) the safety proof of spira_nearest.h ("Why pruning is safe") shows that every triangle of a skipped child has a scan d2 STRICTLY beyond the value
//       the node test was given.  Nothing in it uses that the value is the best distance: it holds word for word with `bound` for `best`;
//   (2) a candidate with d2 beyond the K-th d2 of ANY subset of the candidates is not among the first K of all of them: K candidates sort before it;
//   (3) the bound only ever shrinks (an insertion into a full list drops its last entry for one that sorts before it), so what an earlier, larger bound
//       let through is never owed a second look, and a candidate AT the bound (d2 == the K-th d2) is still met — the node test is strict, the leaf test
//       is d2 <= bound — and near_insert then decides by index.
// The root box is tested by near_enter against the bound the LDS scan left, which is best0 while the list is not full (and always under the count flag);
// (2) covers a smaller one.  The builder partitions the triangles: each sits in exactly one leaf, a walk meets it at most once, no duplicate suppression.
//
// Where a lane's list lives: in private arrays of a compile-time capacity CAP in {1, 4, 16}, the smallest that holds max_near.  Capacities 1 and 4 are
// indexed by constants only and are registers; capacity 16 is indexed at run time and lives in scratch memory beside the walk's 256-byte stack.
// The point q of a slot: capacity 1 keeps q in the entry (three T: k_nearest's own state).  Capacities 4 and 16 keep, per entry, the tree's triangle
// record index (`ti` of the walk; nothing for LDS objects, whose record follows from prim) and compute q again when the slot is stored, with the same
// function on the same record: -ffp-contract=off and IEEE division make that the same bits.  near_keeps_q below is the table; DESIGN.md section 14 has the
// compiler's resource report that decided it.
//
// Kernels (each stages the scene with stage_scene: one barrier):
//   k_knear<T, BVH, TRI, CAP>    one lane per point, grid-stride: knear_scan_local over the spheres and LDS triangles; BVH: then knear_step to the end
//                                (SPIRA_CAST_INPLACE, or a scene without a tree).
//   k_knear_session<T, CAP>      scenes with a tree, the default: SPIRA_REFILLED_SESSION of spira_query.h over session_range of a CastPlan, the ray queries'
//                                knobs.  start = near_load, knear_scan_local, near_enter; step = knear_step.  A finished lane's K slots and count go straight
//                                to out[point], when the lane is next refilled or the session ends (k_hits_session's reason: docs/experiments.md section 33).
#pragma once
#include <cstdint>

#include "spira_nearest.h"      // SPIRA_HD (through spira_query.h), the closest-point functions
#include "spira_hits.h"         // hits_before: the order

namespace spira {

constexpr uint32_t kNearMax = 16;       // SPIRA_MAX_NEAR

// What an entry carries beside (d2, prim): the point itself, or where to compute it again.
template <class T> struct NearPoint { T q[3]; };
struct NearRef { uint32_t ref; };       // the tree's triangle record index; unused for LDS objects

// c ? a : b field by field: a conditional on whole entries would take their addresses and put a register list into memory.
template <class T> SPIRA_HD inline NearPoint<T> near_pick(bool c, const NearPoint<T> &a, const NearPoint<T> &b) { return {{c ? a.q[0] : b.q[0], c ? a.q[1] : b.q[1], c ? a.q[2] : b.q[2]}}; }
template <class T> SPIRA_HD inline NearRef near_pick(bool c, const NearRef &a, const NearRef &b) { return {c ? a.ref : b.ref}; }

// Which capacities keep q in the entry (header comment).  SPIRA_KNEAR_KEEP_Q: the A/B switch the table was made with — the sum of
// the capacities (4, 16) that keep q as well.
#ifndef SPIRA_KNEAR_KEEP_Q
#define SPIRA_KNEAR_KEEP_Q 0
#endif
template <class T, int CAP> constexpr bool near_keeps_q() { return CAP == 1 || (SPIRA_KNEAR_KEEP_Q & CAP) != 0; }

// One lane's list: n <= K <= CAP entries sorted by (d2 ascending, prim descending).
template <class T, int CAP, class P> struct NearList {
    T d2[CAP];
    int prim[CAP];
    P pay[CAP];
    uint32_t n;
};

// hits_insert (spira_hits.h) with a third field per entry, in two forms for the same reasons.  Inserts the candidate (d2, prim, pay) into a list of at most
// K entries (K <= CAP; K = 0: nothing is kept).  A full list drops its last entry — or the candidate, when that sorts after the last entry (d2 == the last d2
// with a smaller index included).  Returns the pruning bound: the last entry's d2 when the list is full, else best0.  A NaN d2 sorts before nothing; the
// kernels never offer one (near_offer).
//   CAP <= 4   on constant indices only, so that the list is registers: the candidate is carried down the list, changing places at every slot whose entry it
//              sorts before; the first free slot takes what is carried.  One comparison per slot, used at once — hits_insert's find-then-shift form with
//              a third field kept seven more lane masks alive and spilled SGPRs in the capacity-4 kernels.
//   CAP = 16   hits_insert's: an insertion sort's inner loop on run-time indices, which keeps the list in scratch memory beside the walk's stack.  Entries at
//              and beyond n are never read, so a list starts with n = 0 and nothing else.
template <class T, int CAP, class P>
SPIRA_HD inline T near_insert(NearList<T, CAP, P> &l, uint32_t K, T d2, int prim, const P &pay, T best0) {
    const uint32_t n = l.n;
    if constexpr (CAP > kHitsRegisterCap) {
        if (K == 0) return best0;
        uint32_t j = K - 1;
        if (n < K) { j = n; l.n = n + 1; }
        else if (!hits_before<T>(d2, prim, l.d2[j], l.prim[j])) return l.d2[j];      // a full list and the candidate sorts after its last entry: dropped
#if defined(__HIPCC__)
#pragma nounroll
#endif
        while (j > 0 && hits_before<T>(d2, prim, l.d2[j - 1], l.prim[j - 1])) { l.d2[j] = l.d2[j - 1]; l.prim[j] = l.prim[j - 1]; l.pay[j] = l.pay[j - 1]; --j; }
        l.d2[j] = d2; l.prim[j] = prim; l.pay[j] = pay;
        return l.n == K ? l.d2[K - 1] : best0;
    }
    // the candidate is carried down the list: at slot j it changes places with the entry it sorts before, the first free slot takes what is carried
#if defined(__HIP_DEVICE_COMPILE__)
    // K is wave-uniform.  Left a scalar, its comparisons with the slot numbers (j < K, j + 1 == K: seven at capacity 4) are hoisted out of the walk and held
    // as lane masks, 14 SGPRs, and two of the capacity-4 kernels still spilled a pair.  Taken per lane here, they are computed where they are used.
    asm volatile("" : "+v"(K));
#endif
    T cd = d2; int cp = prim; P cy = pay;
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int j = 0; j < CAP; ++j) {
        const bool take = (uint32_t)j < K && (((uint32_t)j < n && hits_before<T>(cd, cp, l.d2[j], l.prim[j])) || (uint32_t)j == n);
        const T td = l.d2[j]; const int tp = l.prim[j]; const P ty = l.pay[j];
        l.d2[j] = take ? cd : td; l.prim[j] = take ? cp : tp; l.pay[j] = near_pick<T>(take, cy, ty);
        cd = take ? td : cd; cp = take ? tp : cp; cy = near_pick<T>(take, ty, cy);
    }
    if (n < K) l.n = n + 1;
    T bound = best0;
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int j = 0; j < CAP; ++j)
        if ((uint32_t)j + 1 == K && l.n == K) bound = l.d2[j];
    return bound;
}

// One object met by a lane: the candidate test against the lane's bound, the count, the insertion, the new bound.  `bound` starts as best0 and stays
// best0 under count_all.  true: the list is full and `bound` is its last d2 — a walk recomputes bestn from it.
template <class T, int CAP, class P>
SPIRA_HD inline bool near_offer(NearList<T, CAP, P> &l, uint32_t K, bool count_all, T d2, int prim, const P &pay, T best0, T &bound, uint32_t &total) {
    if (!(d2 <= bound)) return false;                // beyond the bound, or NaN: never a candidate
    ++total;
    const T b = near_insert<T, CAP, P>(l, K, d2, prim, pay, best0);
    if (count_all) return false;
    bound = b;
    return l.n == K;
}

}  // namespace spira

#if defined(__HIPCC__)
#include <type_traits>
namespace spira {

// NearestArgs' scene, points, n_points, trips, base / rem / refill_free as they are (near_load and launch_list read them); prim and dist are
// n_points x max_near, point n_points x max_near x 3, point-major.
template <class T> struct KNearArgs : NearestArgs<T> {
    uint32_t *count;                 // n_points; may be NULL (as prim, dist and point)
    uint32_t max_near;               // K: 0 .. CAP of the kernel launched
    uint32_t count_all;              // SPIRA_NEAR_COUNT_ALL: count every candidate, prune with best0 only
};

template <class T, int CAP> using NearPay = std::conditional_t<near_keeps_q<T, CAP>(), NearPoint<T>, NearRef>;

// One lane's query state beside NearWalk (whose `best` is the bound here; its prim and q are not used): the list, the candidates met, best0.
template <class T, int CAP> struct KNearLane {
    NearList<T, CAP, NearPay<T, CAP>> l;
    uint32_t total;                  // candidates met so far (all of them under COUNT_ALL)
    T best0;
};

template <class T, int CAP> __device__ __forceinline__ NearPay<T, CAP> knear_pay(const T q[3], uint32_t ref) {
    NearPay<T, CAP> p;
    if constexpr (near_keeps_q<T, CAP>()) { p.q[0] = q[0]; p.q[1] = q[1]; p.q[2] = q[2]; } else p.ref = ref;
    return p;
}

template <class T, int CAP> __device__ __forceinline__ void knear_begin(KNearLane<T, CAP> &h, T best0) {
    if constexpr (CAP <= kHitsRegisterCap) {
        const T z[3] = {(T)0, (T)0, (T)0};
#pragma unroll
        for (int j = 0; j < CAP; ++j) { h.l.d2[j] = best0; h.l.prim[j] = SPIRA_RAY_MISS; h.l.pay[j] = knear_pay<T, CAP>(z, 0u); }
    }
    h.l.n = 0; h.total = 0; h.best0 = best0;
}

// The point of an entry that does not keep it: the scan's own function on the record the entry was made from — the LDS record of a sphere (its radius
// from spheres5) or of an LDS triangle, both found from prim, or the tree's triangle record `ref`.
template <class T>
__device__ __forceinline__ void knear_point(const KNearArgs<T> &a, const SceneLds<T> &sc, const T p[3], int prim, uint32_t ref, T q[3]) {
    constexpr bool kWide = sizeof(T) == 8;
    T d2;
    const uint32_t k = (uint32_t)prim;
    if (k < sc.n_spheres) {
        const Pack4<T> sp = sc.sph[k];
        const T c[3] = {sp.x, sp.y, sp.z};
        closest_point_sphere<T>(c, a.scene.spheres5[5 * (size_t)k + 3], p, q, d2);
        return;
    }
    Pack4<T> a0, a1, a2;
    if (k < sc.n_spheres + sc.n_triangles) {
        const uint32_t t = k - sc.n_spheres;
        a0 = sc.tri[3 * t]; a1 = sc.tri[3 * t + 1]; a2 = sc.tri[3 * t + 2];
    } else {
        const uint4 *ptr = reinterpret_cast<const uint4 *>(sc.bvh_tris + 3 * (size_t)ref);
        const uint4 w0 = ptr[0], w1 = ptr[1], w2 = ptr[2], wz = make_uint4(0, 0, 0, 0);
        uint4 w3 = wz, w4 = wz, w5 = wz;
        if constexpr (kWide) { w3 = ptr[3]; w4 = ptr[4]; w5 = ptr[5]; }
        bvh8_tri_words(w0, w1, w2, w3, w4, w5, a0, a1, a2);
    }
    const T v0[3] = {a0.x, a0.y, a0.z}, e1[3] = {a1.x, a1.y, a1.z}, e2[3] = {a2.x, a2.y, a2.z};
    closest_point_triangle<T>(v0, e1, e2, p, q, d2);
}

// Slot j of point i: used slots hold prim, sqrt(d2) and q; unused ones SPIRA_RAY_MISS, r_max copied and point 0; every slot of an invalid point
// SPIRA_RAY_INVALID, 0 and 0.  count: the slots filled, or every candidate.
template <class T, int CAP>
__device__ __forceinline__ void knear_store(const KNearArgs<T> &a, const SceneLds<T> &sc, uint32_t i, bool valid, const NearWalk<T> &w, const KNearLane<T, CAP> &h, T r_max) {
    const uint32_t K = a.max_near;
    const size_t at = (size_t)i * K;
    const auto slot = [&](uint32_t j, bool used, int lp, T ld2, const NearPay<T, CAP> &pay) {
        if (a.prim) a.prim[at + j] = used ? lp : (valid ? SPIRA_RAY_MISS : SPIRA_RAY_INVALID);
        if (a.dist) a.dist[at + j] = used ? near_sqrt<T>(ld2) : (valid ? r_max : (T)0);
        if (a.point) {
            T q[3] = {(T)0, (T)0, (T)0};
            if (used) {
                if constexpr (near_keeps_q<T, CAP>()) { q[0] = pay.q[0]; q[1] = pay.q[1]; q[2] = pay.q[2]; }
                else knear_point<T>(a, sc, w.p, lp, pay.ref, q);
            }
            T *o = a.point + 3 * (at + j);
            o[0] = q[0]; o[1] = q[1]; o[2] = q[2];
        }
    };
    if constexpr (CAP <= kHitsRegisterCap && near_keeps_q<T, CAP>()) {
#pragma unroll
        for (int j = 0; j < CAP; ++j)
            if ((uint32_t)j < K) slot((uint32_t)j, (uint32_t)j < h.l.n, h.l.prim[j], h.l.d2[j], h.l.pay[j]);      // (an invalid point's list is empty)
    } else if constexpr (CAP <= kHitsRegisterCap) {
        // the register list whose slots compute q again: ONE copy of that code in a run-time loop — j is wave-uniform, the entry is picked by constant indices
#pragma nounroll
        for (uint32_t j = 0; j < K; ++j) {
            int lp = h.l.prim[0]; T ld2 = h.l.d2[0]; NearPay<T, CAP> pay = h.l.pay[0];
#pragma unroll
            for (int k = 1; k < CAP; ++k) { const bool me = j == (uint32_t)k; lp = me ? h.l.prim[k] : lp; ld2 = me ? h.l.d2[k] : ld2; pay = near_pick<T>(me, h.l.pay[k], pay); }
            slot(j, j < h.l.n, lp, ld2, pay);
        }
    } else {
        // the scratch-resident list: a run-time loop over its slots, the filled ones read, the others not
#pragma nounroll
        for (uint32_t j = 0; j < K; ++j) {
            int lp = 0; T ld2 = 0; NearPay<T, CAP> pay{};
            const bool used = j < h.l.n;
            if (used) { lp = h.l.prim[j]; ld2 = h.l.d2[j]; pay = h.l.pay[j]; }
            slot(j, used, lp, ld2, pay);
        }
    }
    if (a.count) a.count[i] = !valid ? 0u : (a.count_all ? h.total : h.l.n);
    if (a.trips) a.trips[i] = w.trips;
}

// The LDS part: every sphere (radius from spheres5) and LDS triangle in order, each offered against the lane's current bound (w.best).
template <class T, bool TRI, int CAP>
__device__ __forceinline__ void knear_scan_local(const KNearArgs<T> &a, const SceneLds<T> &sc, NearWalk<T> &w, KNearLane<T, CAP> &h, uint32_t K, bool count_all) {
    for (uint32_t s = 0; s < sc.n_spheres; ++s) {
        const Pack4<T> sp = sc.sph[s];
        const T c[3] = {sp.x, sp.y, sp.z};
        T q[3], d2;
        closest_point_sphere<T>(c, a.scene.spheres5[5 * (size_t)s + 3], w.p, q, d2);
        near_offer<T, CAP>(h.l, K, count_all, d2, (int)s, knear_pay<T, CAP>(q, 0u), h.best0, w.best, h.total);
    }
    if (TRI)
        for (uint32_t t = 0; t < sc.n_triangles; ++t) {
            const Pack4<T> a0 = sc.tri[3 * t], a1 = sc.tri[3 * t + 1], a2 = sc.tri[3 * t + 2];
            const T v0[3] = {a0.x, a0.y, a0.z}, e1[3] = {a1.x, a1.y, a1.z}, e2[3] = {a2.x, a2.y, a2.z};
            T q[3], d2;
            closest_point_triangle<T>(v0, e1, e2, w.p, q, d2);
            near_offer<T, CAP>(h.l, K, count_all, d2, (int)(sc.n_spheres + t), knear_pay<T, CAP>(q, 0u), h.best0, w.best, h.total);
        }
}

// One trip of the K-nearest walk: near_trip (spira_nearest.h) over the same NearWalk, stack and node test as the closest-point walk; the triangle is
// offered to the list, and bestn follows the bound when the list is full.  Returns false when the walk is over.
template <class T, int CAP>
__device__ __forceinline__ bool knear_step(const SceneLds<T> &sc, NearWalk<T> &w, int base, KNearLane<T, CAP> &h, uint32_t K, bool count_all, uint32_t *stack) {
    return near_trip<T>(sc, w, base, stack, [&](uint32_t ti, const T q[3], T d2, int p) {
        if (near_offer<T, CAP>(h.l, K, count_all, d2, p, knear_pay<T, CAP>(q, ti), h.best0, w.best, h.total)) w.bestn = near_bestn<T>(w.best, sc.bvh_root[2].w);
    });
}

// One lane per point.  Launches: <T, false, false, .> spheres alone, <T, false, true, .> with LDS triangles, <T, true, false, .> a BVH mesh (SPIRA_CAST_INPLACE).
template <class T, bool BVH, bool TRI, int CAP>
__global__ __launch_bounds__(kBlock) void k_knear(const KNearArgs<T> a) {
    extern __shared__ __attribute__((aligned(32))) unsigned char lds_raw[];
    const SceneLds<T> sc = stage_scene<T>(a.scene, lds_raw);     // the only workgroup barrier of the kernel
    const uint32_t K = a.max_near;
    const bool count_all = a.count_all != 0;
    const int base = (int)(sc.n_spheres + sc.n_triangles);
    for (uint32_t i = blockIdx.x * kBlock + threadIdx.x; i < a.n_points; i += gridDim.x * kBlock) {
        NearWalk<T> w; T r_max;
        const bool ok = near_load<T>(a, sc, BVH, i, w, r_max);
        KNearLane<T, CAP> h;
        knear_begin<T, CAP>(h, w.best);
        if (ok) {
            knear_scan_local<T, TRI, CAP>(a, sc, w, h, K, count_all);
            if (BVH) {
                uint32_t stack[kBvhStackD];
                if (near_enter<T>(sc, w)) while (knear_step<T, CAP>(sc, w, base, h, K, count_all, stack)) {}
            }
        }
        knear_store<T, CAP>(a, sc, i, ok, w, h, r_max);
    }
}

// Scenes with a tree: a refilled session per wave over its range of the caller's list (SPIRA_REFILLED_SESSION of spira_query.h).
template <class T, int CAP>
__global__ __launch_bounds__(kBlock) void k_knear_session(const KNearArgs<T> a) {
    extern __shared__ __attribute__((aligned(32))) unsigned char lds_raw[];
    const SceneLds<T> sc = stage_scene<T>(a.scene, lds_raw);     // the only workgroup barrier of the kernel
    uint32_t begin, end;
    session_range(a.base, a.rem, begin, end);
    uint32_t stack[kBvhStackD];
    const uint32_t K = a.max_near;
    const bool count_all = a.count_all != 0;
    const int base = (int)(sc.n_spheres + sc.n_triangles);
    uint32_t pt = 0;
    T r_max = 0;
    NearWalk<T> w{};
    KNearLane<T, CAP> h;
    knear_begin<T, CAP>(h, (T)0);
    // A lane that finishes its walk stores when it is next refilled (all the lanes of a refill store together) or when the session ends: k_hits_session's way.
    bool pending = false;
    const auto start = [&](uint32_t item) -> bool {
            if (pending) { knear_store<T, CAP>(a, sc, pt, true, w, h, r_max); pending = false; }
            pt = item;
            const bool ok = near_load<T>(a, sc, true, pt, w, r_max);
            knear_begin<T, CAP>(h, w.best);
            bool walks = false;
            if (ok) {
                knear_scan_local<T, false, CAP>(a, sc, w, h, K, count_all);
                walks = near_enter<T>(sc, w);
            }
            if (!walks) knear_store<T, CAP>(a, sc, pt, ok, w, h, r_max);
            return walks;
    };
    const auto step = [&]() -> bool {
            if (knear_step<T, CAP>(sc, w, base, h, K, count_all, stack)) return true;
            pending = true;
            return false;
    };
    SPIRA_REFILLED_SESSION(begin, end, a.refill_free, start, step);
    if (pending) knear_store<T, CAP>(a, sc, pt, true, w, h, r_max);
}

}  // namespace spira
#endif
