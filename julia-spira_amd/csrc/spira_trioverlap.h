// spira_trioverlap.h — triangle overlap queries on a scene handle (spira_scene_overlap_tri_* / spira_scene_overlap_tri_any_*): which objects of this scene does
// this triangle cut?  Included by spira_hip.hip behind spira_overlap.h, whose walk this is with another enclosing box and another leaf test: overlap_node,
// OverlapList, overlap_insert, overlap_take, overlap_store, overlap_trip and the plan check (overlap_check) are that file's, used and not copied.  The first
// part of this file needs no HIP header: a CPU program (tests/native/trioverlap_plan.cpp) and the exported host arithmetic (spira_overlap_tri_triangle_*,
// spira_overlap_tri_sphere_*) call the very functions the kernels call.  This comment is the contract; the numpy twins (spira_hip.query: prepare_triangles,
// overlap_tri_triangle, overlap_tri_sphere) restate it operation for operation.
//
// All arithmetic in the call's precision T, in the written order, nothing fused (-ffp-contract=off); dot(a, b) is ALWAYS (a.x b.x + a.y b.y) + a.z b.z
// (near_dot); cross(a, b) = (a.y b.z - a.z b.y, a.z b.x - a.x b.z, a.x b.y - a.y b.x), as in spira_overlap.h.
//
// The query list is n x [q0 q1 q2 mat], ten values a triangle: the layout of triangles10, so the array another handle was created from or updated with is
// a query list as it is, on the host or on the device.  The tenth value is never read: it may be anything, NaN included.
//     g1 = q1 - q0,  g2 = q2 - q0,  g3 = g2 - g1,  m = cross(g1, g2)
// Validity (trioverlap_prepare), in this order: any of the nine coordinates NaN; any of them infinite; a component of m not finite; m exactly (0, 0, 0) —
// a segment or a point is no triangle query: rays and boxes with h = 0 serve those —; and, scenes with a tree only, the origin rule of the ray queries
// (|(q_k - centre_k) scale| <= kCastOriginBound = 64 in T) fails for q0, q1 or q2 (in this order).  There is no extent rule: three vertices within the
// origin bound bound the enclosing box, |lo|, |hi| <= 64.
//
// The objects are the spheres [0..) then the triangles [0..) in the caller's order.
// Scene triangle against the query (overlap_tri_triangle): a 20-axis separating-axis test on the record's own v0, e1 = v1 - v0, e2 = v2 - v0, everything
// relative to q0:
//     u0 = v0 - q0,  u1 = u0 + e1,  u2 = u0 + e2,  e3 = e2 - e1,  n = cross(e1, e2)
// On an axis L the scene triangle projects to pS = (dot(L, u0), dot(L, u1), dot(L, u2)) and the query to pQ = (0, dot(L, g1), dot(L, g2)).  The axis
// OVERLAPS when none of the six values is NaN and
//     min(pS) <= max(pQ)  &&  min(pQ) <= max(pS)                              (closed: touching counts)
// The 20 axes (every one is evaluated, & and not &&, as in overlap_box_triangle; their order cannot matter):
//     the world unit axes k = 0, 1, 2:          the projections are the components themselves, no products: pS = (u0[k], u1[k], u2[k]), pQ = (0, g1[k], g2[k])
//     n:                                        the single value dot(n, u0) taken for all of pS;  pQ = (0, dot(n, g1), dot(n, g2))
//     m:                                        pS = (dot(m, u0), dot(m, u1), dot(m, u2));  0 taken for all of pQ
//     L = cross(g_i, e_j), i, j = 1, 2, 3:      pS and pQ by the general formula above, every dot computed (none replaced by the value it has in exact arithmetic)
//     L = cross(n, e_j), j = 1, 2, 3, and L = cross(m, g_i), i = 1, 2, 3: likewise.  These six separate COPLANAR pairs, which the first fourteen cannot
//     (there n and m are parallel and every cross(g_i, e_j) is parallel to them: all project both triangles to one value each).
// The triangle is a CANDIDATE when all 20 overlap.  A NaN anywhere makes it no candidate; so does n == (0, 0, 0) exactly (zero area), as in the box query
// and for its reason: the point queries never pick such a triangle either.
// Why the world axes are there.  In exact arithmetic they are redundant.  With them a scene triangle beyond the query's axis-aligned enclosing box is
// rejected by a test that has no product in it — two roundings per vertex, below — so the tree provably only prunes, and the conditioning gap that
// spira_overlap.h leaves to its tests (kappa: through which of 13 axes a gap along a world axis shows) does not arise here.
// Sphere against the query (overlap_tri_sphere): a sphere is a SHELL, as everywhere; centre C and radius R as the caller gave them (the kernels read R from
// spheres5).  dmin2 = the d2 of closest_point_triangle(q0, g1, g2, C) (spira_nearest.h);  dmax2 = max(near_d2(C, q0), near_d2(C, q1), near_d2(C, q2)) over
// the caller's own three vertices (the farthest point of a triangle from C is a vertex);  R2 = R R;  candidate when  dmin2 <= R2 && dmax2 >= R2.  A NaN
// means no candidate (dmin2: the comparison is false; the three d2 are NaN only when C is, and then dmin2 is).
//
// The answer is spira_overlap.h's, word for word: out_count[i] the number of ALL candidates; out_prim (n x max_list) the first max_list candidates in
// ASCENDING object index, unused slots SPIRA_RAY_MISS, every slot of an invalid query SPIRA_RAY_INVALID and its count 0; max_list in 0 .. SPIRA_MAX_OVERLAP.
// The any form: out_hit[i] = 1 exactly where count > 0, else 0, 255 for an invalid query; its kernels leave at the first candidate.
//
// The walk.  The enclosing box  lo_k = min(q0_k, q1_k, q2_k),  hi_k = max(q0_k, q1_k, q2_k)  (in T, exact) is taken to the tree's frame and rounded to Float32,
//     lo_k = fl32((lo_k - centre_k) scale),  hi_k = fl32((hi_k - centre_k) scale),
// and grown by  g = (max_k max(|lo_k|, |hi_k|) + 1) 2^-12  exactly as overlap_enter grows its box.  Then overlap_node, one group entry per level on the
// private stack, one memory round trip per trip: overlap_trip with this file's leaf arm, the SAT above in T on the record's own values.
//
// Why the growth suffices (normalised units; M = max(|lo|, |hi|) <= 64 by the origin rule, A = amax_n, u = 2^-24, u_T that of T).  A child is wrongly skipped
// only if a triangle the SAT accepts lies in a child box that misses [qlo, qhi].  Suppose the child box ends below qlo on axis k (above qhi: mirrored).
//   (a) the query box: min and max are exact; less the centre, times scale, in T, then rounded to Float32: <= 2 u_T (M + A) + u M   <= 3 u M + 2 u A = 1.3e-5
//       at M = 64, A <= 1
//   (b) the child planes: grid + q step rounds once at a magnitude <= A + 1 (near_node's (b))                                       <= 6e-8 (1 + A)
//   (c) the leaf's world axis k: the accepted triangle has min(pS) <= max(pQ) on it, that is some computed u_m[k] <= max(0, g1[k], g2[k]).  g_i[k] is
//       q_i[k] - q0[k] rounded once, u0[k] = v0[k] - q0[k] rounded once, u_m[k] = u0[k] + e_m[k] rounded once more (e_m is the record's, the value the
//       triangle HAS: its vertex is v0 + e_m): two roundings of u_m against one of g_i, each at a magnitude <= 2 (M + A), so the vertex v_m[k] lies below
//       hi_k + eta,  eta <= 3 u_T 2 (M + A) = 2.4e-5 at M = 64 in Float32, and mirrored above lo_k - eta.
//   Every triangle lies inside its child box shrunk by the builder's pad, 1e-4 max(1, A) (spira_bvh.h; the refit pad is never smaller).
// The growth is g = 2^-12 (M + 1) >= 2.4e-4, at M = 64 1.6e-2; half of it is what tests/test_trioverlap_cpu.py places triangles beyond the enclosing box by,
// at offsets of 0 and 60 units, 10^5 per precision, and the leaf rejects every one.  Against HALF the growth (a) + (b) + eta = 1.3e-5 + 1.2e-7 + 2.4e-5 =
// 3.7e-5 at M = 64 in Float32: a margin of 210 there, of 2^-13 / (9 u) = 220 at every M >= 1 and more below, before the pad.  In Float64 eta vanishes and (a)
// is the conversion's u M.  No kappa: the axis the gap lies along is itself one of the 20.
//
// Kernels (each stages the scene with stage_scene: one barrier), the siblings of k_overlap / k_overlap_session with the same parameters:
//   k_trioverlap<T, BVH, TRI, ANY, CAP>    one lane per query, grid-stride: the LDS scan over spheres and LDS triangles; BVH: then the walk to the end
//                                          (SPIRA_CAST_INPLACE, or a scene without a tree).
//   k_trioverlap_session<T, ANY, CAP>      scenes with a tree, the default: SPIRA_REFILLED_SESSION over session_range of a CastPlan, the ray queries' knobs.
//   ANY, CAP in {1, 4, 16}                 as in spira_overlap.h.
#pragma once
#include <cstdint>

#include "spira_overlap.h"      // ovl_min3, ovl_max3, OverlapList, overlap_insert; spira_nearest.h: near_dot, near_d2, closest_point_triangle

namespace spira {

// A prepared query: the caller's vertices, the edges from q0 and their cross product.
template <class T> struct TriQuery { T q0[3], q1[3], q2[3], g1[3], g2[3], m[3]; };

template <class T> SPIRA_HD inline void tri_cross(const T a[3], const T b[3], T out[3]) {
    out[0] = a[1] * b[2] - a[2] * b[1]; out[1] = a[2] * b[0] - a[0] * b[2]; out[2] = a[0] * b[1] - a[1] * b[0];
}

// One query t[0..9) (the tenth value is not read) -> valid?  Q is written for every query without NaN or infinite coordinates.
// frame: the scene has a tree, fr = {centre.x, centre.y, centre.z, scale} (as cast_ray_prepare).
template <class T> SPIRA_HD inline bool trioverlap_prepare(const T *t, bool frame, const T *fr, TriQuery<T> &Q) {
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int k = 0; k < 9; ++k) if (t[k] != t[k]) return false;                          // NaN in a coordinate
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int k = 0; k < 9; ++k) if (!((t[k] - t[k]) == (T)0)) return false;              // an infinite coordinate
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int k = 0; k < 3; ++k) {
        Q.q0[k] = t[k]; Q.q1[k] = t[3 + k]; Q.q2[k] = t[6 + k];
        Q.g1[k] = t[3 + k] - t[k]; Q.g2[k] = t[6 + k] - t[k];
    }
    tri_cross<T>(Q.g1, Q.g2, Q.m);
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int k = 0; k < 3; ++k) if (!((Q.m[k] - Q.m[k]) == (T)0)) return false;
    if (Q.m[0] == (T)0 && Q.m[1] == (T)0 && Q.m[2] == (T)0) return false;                // a segment or a point
    if (frame)
#if defined(__HIPCC__)
#pragma unroll
#endif
        for (int k = 0; k < 9; ++k) {
            const T x = (t[k] - fr[k % 3]) * fr[3];
            if (!(x >= (T)-kCastOriginBound && x <= (T)kCastOriginBound)) return false;
        }
    return true;
}

// One axis: the scene triangle's projections s0, s1, s2 against the query's (0, p1, p2) (header comment).  __builtin_isunordered(a, b): a or b is NaN.
template <class T> SPIRA_HD inline bool tri_axis(T s0, T s1, T s2, T p1, T p2) {
    if (__builtin_isunordered(s0, s1) || __builtin_isunordered(s2, p1) || __builtin_isunordered(p2, p2)) return false;
    return ovl_min3<T>(s0, s1, s2) <= ovl_max3<T>((T)0, p1, p2) && ovl_min3<T>((T)0, p1, p2) <= ovl_max3<T>(s0, s1, s2);
}

// The axis L = cross(a, b) by the general formula.
template <class T> SPIRA_HD inline bool tri_cross_axis(const T a[3], const T b[3], const T u0[3], const T u1[3], const T u2[3], const T g1[3], const T g2[3]) {
    T L[3];
    tri_cross<T>(a, b, L);
    return tri_axis<T>(near_dot<T>(L, u0), near_dot<T>(L, u1), near_dot<T>(L, u2), near_dot<T>(L, g1), near_dot<T>(L, g2));
}

// The triangle (v0, v0 + e1, v0 + e2) against the query: all 20 axes overlap.
template <class T> SPIRA_HD inline bool overlap_tri_triangle(const TriQuery<T> &Q, const T v0[3], const T e1[3], const T e2[3]) {
    const T u0[3] = {v0[0] - Q.q0[0], v0[1] - Q.q0[1], v0[2] - Q.q0[2]};
    const T u1[3] = {u0[0] + e1[0], u0[1] + e1[1], u0[2] + e1[2]}, u2[3] = {u0[0] + e2[0], u0[1] + e2[1], u0[2] + e2[2]};
    const T e3[3] = {e2[0] - e1[0], e2[1] - e1[1], e2[2] - e1[2]};
    const T g3[3] = {Q.g2[0] - Q.g1[0], Q.g2[1] - Q.g1[1], Q.g2[2] - Q.g1[2]};
    T n[3];
    tri_cross<T>(e1, e2, n);
    bool ok = true;      // every axis is evaluated (&, not &&): a lane's early exit would only split its wave
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int k = 0; k < 3; ++k) ok &= tri_axis<T>(u0[k], u1[k], u2[k], Q.g1[k], Q.g2[k]);
    const T pn = near_dot<T>(n, u0);
    ok &= tri_axis<T>(pn, pn, pn, near_dot<T>(n, Q.g1), near_dot<T>(n, Q.g2));
    ok &= n[0] != (T)0 || n[1] != (T)0 || n[2] != (T)0;      // zero area: never a candidate
    ok &= tri_axis<T>(near_dot<T>(Q.m, u0), near_dot<T>(Q.m, u1), near_dot<T>(Q.m, u2), (T)0, (T)0);
    const T *const g[3] = {Q.g1, Q.g2, g3}, *const e[3] = {e1, e2, e3};
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int i = 0; i < 3; ++i)
#if defined(__HIPCC__)
#pragma unroll
#endif
        for (int j = 0; j < 3; ++j) ok &= tri_cross_axis<T>(g[i], e[j], u0, u1, u2, Q.g1, Q.g2);
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int j = 0; j < 3; ++j) ok &= tri_cross_axis<T>(n, e[j], u0, u1, u2, Q.g1, Q.g2);
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int i = 0; i < 3; ++i) ok &= tri_cross_axis<T>(Q.m, g[i], u0, u1, u2, Q.g1, Q.g2);
    return ok;
}

// The shell of the sphere (centre C, radius R) against the query.
template <class T> SPIRA_HD inline bool overlap_tri_sphere(const TriQuery<T> &Q, const T C[3], T R) {
    T q[3], dmin2;
    closest_point_triangle<T>(Q.q0, Q.g1, Q.g2, C, q, dmin2);
    const T dmax2 = ovl_max3<T>(near_d2<T>(C, Q.q0), near_d2<T>(C, Q.q1), near_d2<T>(C, Q.q2)), R2 = R * R;
    return dmin2 <= R2 && dmax2 >= R2;
}

}  // namespace spira

#if defined(__HIPCC__)
namespace spira {

// The arguments are the box query's, field for field: `boxes` holds the n x 10 query triangles.
template <class T> using TriOverlapArgs = OverlapArgs<T>;

// One lane's query: the prepared triangle, the grown enclosing box in the tree's frame, the walk, the candidates (the walk's fields are OverlapWalk's).
template <class T, int CAP> struct TriOverlapWalk {
    TriQuery<T> Q;
    float qlo[3], qhi[3];
    uint32_t G;
    uint32_t tw, rank;
    uint32_t sp;
    uint32_t trips;
    uint32_t total;
    OverlapList<CAP> l;
};

// Loads query i (nine values: the tenth is not read), classifies it and starts the lane's state.  Returns the validity.
template <class T, int CAP>
__device__ __forceinline__ bool trioverlap_load(const TriOverlapArgs<T> &a, const SceneLds<T> &sc, bool frame, uint32_t i, TriOverlapWalk<T, CAP> &w) {
    const T *tp = a.boxes + 10 * (size_t)i;
    T t[9], fr[4] = {(T)0, (T)0, (T)0, (T)1};
#pragma unroll
    for (int k = 0; k < 9; ++k) t[k] = tp[k];
    if (frame) { const Pack4<T> f = sc.bvh_root[2]; fr[0] = f.x; fr[1] = f.y; fr[2] = f.z; fr[3] = f.w; }
#pragma unroll
    for (int k = 0; k < 3; ++k) w.Q.q0[k] = w.Q.q1[k] = w.Q.q2[k] = w.Q.g1[k] = w.Q.g2[k] = w.Q.m[k] = (T)0;
    const bool ok = trioverlap_prepare<T>(t, frame, fr, w.Q);
    w.G = 0; w.tw = 0; w.rank = 0; w.sp = 0; w.trips = 0; w.total = 0;
    if constexpr (CAP <= kOverlapRegisterCap) {
#pragma unroll
        for (int j = 0; j < CAP; ++j) w.l.prim[j] = SPIRA_RAY_MISS;
    }
    w.l.n = 0;
    return ok;
}

// The LDS part of the scan, in scan order: spheres (radius from spheres5), then the LDS triangles.
template <class T, bool TRI, bool ANY, int CAP>
__device__ __forceinline__ void trioverlap_scan_local(const TriOverlapArgs<T> &a, const SceneLds<T> &sc, TriOverlapWalk<T, CAP> &w, uint32_t K) {
    for (uint32_t s = 0; s < sc.n_spheres; ++s) {
        const Pack4<T> sp = sc.sph[s];
        const T c[3] = {sp.x, sp.y, sp.z};
        if (overlap_tri_sphere<T>(w.Q, c, a.scene.spheres5[5 * (size_t)s + 3])) {
            overlap_take<T, CAP>(w, K, (int)s);
            if (ANY) return;
        }
    }
    if (TRI)
        for (uint32_t i = 0; i < sc.n_triangles; ++i) {
            const Pack4<T> a0 = sc.tri[3 * i], a1 = sc.tri[3 * i + 1], a2 = sc.tri[3 * i + 2];
            const T v0[3] = {a0.x, a0.y, a0.z}, e1[3] = {a1.x, a1.y, a1.z}, e2[3] = {a2.x, a2.y, a2.z};
            if (overlap_tri_triangle<T>(w.Q, v0, e1, e2)) {
                overlap_take<T, CAP>(w, K, (int)(sc.n_spheres + i));
                if (ANY) return;
            }
        }
}

// The enclosing box of the three vertices in the tree's frame, Float32, grown (header comment, "The walk"); the walk starts at the root node.
template <class T, int CAP>
__device__ __forceinline__ void trioverlap_enter(const SceneLds<T> &sc, TriOverlapWalk<T, CAP> &w) {
    const Pack4<T> fr = sc.bvh_root[2];
    const T ctr[3] = {fr.x, fr.y, fr.z};
    float m = 0.0f;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        w.qlo[k] = (float)((ovl_min3<T>(w.Q.q0[k], w.Q.q1[k], w.Q.q2[k]) - ctr[k]) * fr.w);
        w.qhi[k] = (float)((ovl_max3<T>(w.Q.q0[k], w.Q.q1[k], w.Q.q2[k]) - ctr[k]) * fr.w);
        m = __builtin_fmaxf(m, __builtin_fmaxf(__builtin_fabsf(w.qlo[k]), __builtin_fabsf(w.qhi[k])));
    }
    const float g = (m + 1.0f) * 0.000244140625f;      // 2^-12
#pragma unroll
    for (int k = 0; k < 3; ++k) { w.qlo[k] -= g; w.qhi[k] += g; }
    w.G = 1u; w.tw = 0; w.rank = 0; w.sp = 0;           // the root: a group holding only slot 0 of base 0
}

// One trip of the triangle walk: overlap_trip with the SAT of this file as its leaf arm.  Returns false when the walk is over.
template <class T, int CAP>
__device__ __forceinline__ bool trioverlap_step(const SceneLds<T> &sc, TriOverlapWalk<T, CAP> &w, int base, uint32_t K, uint32_t *stack) {
    return overlap_trip<T>(sc, w, stack, [&](const T v0[3], const T e1[3], const T e2[3], uint32_t id) {
        if (overlap_tri_triangle<T>(w.Q, v0, e1, e2)) overlap_take<T, CAP>(w, K, base + (int)id);
    });
}

// One lane per query.  Launches: <T, false, false, ..> spheres alone, <T, false, true, ..> with LDS triangles, <T, true, false, ..> a BVH mesh (SPIRA_CAST_INPLACE).
template <class T, bool BVH, bool TRI, bool ANY, int CAP>
__global__ __launch_bounds__(kBlock) void k_trioverlap(const TriOverlapArgs<T> a) {
    extern __shared__ __attribute__((aligned(32))) unsigned char lds_raw[];
    const SceneLds<T> sc = stage_scene<T>(a.scene, lds_raw);     // the only workgroup barrier of the kernel
    const uint32_t K = ANY ? 0u : a.max_list;
    const int base = (int)(sc.n_spheres + sc.n_triangles);
    for (uint32_t i = blockIdx.x * kBlock + threadIdx.x; i < a.n; i += gridDim.x * kBlock) {
        TriOverlapWalk<T, CAP> w;
        const bool ok = trioverlap_load<T, CAP>(a, sc, BVH, i, w);
        if (ok) {
            trioverlap_scan_local<T, TRI, ANY, CAP>(a, sc, w, K);
            if (BVH && !(ANY && w.total)) {
                uint32_t stack[kBvhStackD];
                trioverlap_enter<T, CAP>(sc, w);
                while (trioverlap_step<T, CAP>(sc, w, base, K, stack) && !(ANY && w.total)) {}
            }
        }
        overlap_store<T, ANY, CAP>(a, i, ok, w);
    }
}

// Scenes with a tree: a refilled session per wave over its range of the caller's list (SPIRA_REFILLED_SESSION of spira_query.h).
template <class T, bool ANY, int CAP>
__global__ __launch_bounds__(kBlock) void k_trioverlap_session(const TriOverlapArgs<T> a) {
    extern __shared__ __attribute__((aligned(32))) unsigned char lds_raw[];
    const SceneLds<T> sc = stage_scene<T>(a.scene, lds_raw);     // the only workgroup barrier of the kernel
    uint32_t begin, end;
    session_range(a.base, a.rem, begin, end);
    uint32_t stack[kBvhStackD];
    const uint32_t K = ANY ? 0u : a.max_list;
    const int base = (int)(sc.n_spheres + sc.n_triangles);
    uint32_t item_ = 0;
    TriOverlapWalk<T, CAP> w{};
    const auto start = [&](uint32_t item) -> bool {
            item_ = item;
            const bool ok = trioverlap_load<T, CAP>(a, sc, true, item_, w);
            bool walks = false;
            if (ok) {
                trioverlap_scan_local<T, false, ANY, CAP>(a, sc, w, K);
                if (!(ANY && w.total)) { trioverlap_enter<T, CAP>(sc, w); walks = true; }
            }
            if (!walks) overlap_store<T, ANY, CAP>(a, item_, ok, w);
            return walks;
    };
    const auto step = [&]() -> bool {
            if (trioverlap_step<T, CAP>(sc, w, base, K, stack) && !(ANY && w.total)) return true;
            overlap_store<T, ANY, CAP>(a, item_, true, w);
            return false;
    };
    SPIRA_REFILLED_SESSION(begin, end, a.refill_free, start, step);
}

}  // namespace spira
#endif
