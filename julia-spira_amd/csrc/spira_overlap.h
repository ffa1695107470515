// spira_overlap.h — box overlap queries on a scene handle (spira_scene_overlap_box_* / spira_scene_overlap_any_*): which objects touch this oriented box?
// Included by spira_hip.hip behind spira_nearest.h (near_dot, near_sqrt) and spira_query.h (CastLimits, kCastOriginBound, the refilled session's loop); the
// tree is the one create, update and rebuild maintain, walked a fourth way: the query's enclosing axis-aligned box against the child boxes, six compares per
// child.  The first part of this file needs no HIP header: a CPU program (tests/native/overlap_plan.cpp) and the exported host arithmetic
// (spira_overlap_box_triangle_*, spira_overlap_box_sphere_*) call the very functions the kernels call.  This comment is the contract; the numpy twins
// (spira_hip.query: prepare_boxes, box_axes, overlap_box_triangle, overlap_box_sphere) restate it operation for operation.
//
// All arithmetic in the call's precision T, in the written order, nothing fused (-ffp-contract=off); dot(a, b) is ALWAYS (a.x b.x + a.y b.y) + a.z b.z;
// cross(a, b) = (a.y b.z - a.z b.y, a.z b.x - a.x b.z, a.x b.y - a.y b.x); divisions and square roots are IEEE; |x| clears the sign bit.
//
// A box is ten values [cx cy cz hx hy hz qx qy qz qw]: centre c, half extents h, and a rotation quaternion the library normalises, as it normalises ray
// directions:  n2 = (qx qx + qy qy) + (qz qz + qw qw),  l = sqrt(n2),  (x, y, z, w) = (qx / l, qy / l, qz / l, qw / l).  With the nine products xx = x x,
// yy, zz, xy = x y, xz, yz, xw = x w, yw, zw the box axes in world coordinates are
//     A0 = (1 - 2 (yy + zz),  2 (xy + zw),      2 (xz - yw))
//     A1 = (2 (xy - zw),      1 - 2 (xx + zz),  2 (yz + xw))
//     A2 = (2 (xz + yw),      2 (yz - xw),      1 - 2 (xx + yy))
// and a world vector a has the box-frame coordinates frame(a) = (dot(A0, a), dot(A1, a), dot(A2, a)).  The identity quaternion (0, 0, 0, 1) gives the unit
// axes exactly, and frame(a) = a then in value: an axis-aligned box is tested in the caller's own coordinates with no rotation rounding.
// The enclosing axis-aligned half extent:  He_k = (|A0_k| h0 + |A1_k| h1) + |A2_k| h2  (A0_k: component k of A0).
//
// The objects are the spheres [0..) then the triangles [0..) in the caller's order.
// Triangle against box (overlap_box_triangle): the 13-axis separating-axis test of Akenine-Moller, on the record's own v0, e1 = v1 - v0, e2 = v2 - v0:
//     u0 = frame(v0 - c),  f1 = frame(e1),  f2 = frame(e2),  u1 = u0 + f1,  u2 = u0 + f2,  f3 = f2 - f1
// An axis with the projections p0, p1, p2 of u0, u1, u2 and the radius rad OVERLAPS when none of p0, p1, p2, rad is NaN and
//     min(p0, p1, p2) <= rad  &&  max(p0, p1, p2) >= -rad                     (closed: touching counts)
// The 13 axes (every one is evaluated; their order cannot matter):
//     the box axes k = 0, 1, 2:                 p_m = u_m[k],  rad = h_k
//     the face normal n = cross(f1, f2):        the single projection p = dot(n, u0) (taken for p0, p1 and p2),  rad = (|n.x| hx + |n.y| hy) + |n.z| hz
//     cross(unit_i, f_j), i = 0, 1, 2, j = 1, 2, 3, with a = (i + 1) mod 3, b = (i + 2) mod 3 — the axis has the components [i] = 0,
//     [a] = -f_j[b], [b] = f_j[a]:             p_m = u_m[b] f_j[a] - u_m[a] f_j[b],  rad = |f_j[b]| h_a + |f_j[a]| h_b
//     (dot(axis, u_m) and the radius "formed the same way", with the products by the zero component left out: the same values.)
// The triangle is a CANDIDATE when all 13 overlap.  A NaN in any projection or radius makes it no candidate — as a NaN d2 is never one for the point queries.
// A triangle whose computed normal is exactly n = (0, 0, 0) — zero area: a segment or a point — is NO candidate, wherever it lies: the face-normal axis
// would pass it (0 <= 0), and the point queries never pick such a triangle either (its d2 is NaN), so the candidates of a box stay within those of its
// enclosing ball.
// Sphere against box (overlap_box_sphere): a sphere is a SHELL, as for the point queries and the sweeps; centre C and radius R as the caller gave them
// (the kernels read R from spheres5).  p = frame(C - c), a_k = |p_k|, e_k = a_k - h_k taken as 0 unless e_k > 0, g_k = a_k + h_k,
//     dmin2 = (e0 e0 + e1 e1) + e2 e2,   dmax2 = (g0 g0 + g1 g1) + g2 g2,   R2 = R R;     candidate when  dmin2 <= R2 && dmax2 >= R2
// (the nearest and the farthest point of the box from C: the shell meets the box exactly when R lies between them).  A NaN makes it no candidate.
//
// The answer.  out_count[i]: the number of ALL candidates of box i.  out_prim (n x max_list): the first max_list candidates in ASCENDING object index;
// unused slots SPIRA_RAY_MISS; every slot of an invalid box SPIRA_RAY_INVALID and its count 0.  max_list in 0 .. SPIRA_MAX_OVERLAP = 16; 0 counts only.
// Index order carries no spatial bound, so the walk never prunes with the list: the count is always complete and there is no COUNT_ALL flag.  The order is
// total, so the order in which a walk meets the candidates cannot matter: both organisations give the same bytes.  The any form: out_hit[i] = 1 exactly
// where count > 0, else 0, 255 for an invalid box; its kernels leave at the first candidate.
//
// Validity (overlap_prepare), in this order: any of the ten values NaN; any of them infinite; some h_k < 0; n2 not finite or below the smallest normal
// number of T; and — scenes with a tree only — the origin rule of the ray queries fails for c (|(c_k - centre_k) scale| <= 64 in T), or
// He_k scale > kOverlapExtentBound = 64 on some axis.  h = 0 is valid: a box may be a point, a segment or a rectangle.
//
// The walk.  The query's enclosing box c +- He is taken to the tree's normalised frame in T and rounded to Float32:
//     lo_k = fl32(((c_k - He_k) - centre_k) scale),  hi_k = fl32(((c_k + He_k) - centre_k) scale)
// and grown outward by  g = (max_k max(|lo_k|, |hi_k|) + 1) 2^-12  (Float32): qlo = lo - g, qhi = hi + g.  A child (lo <= hi on x: present — an empty
// child has lo 255, hi 0) survives when its dequantised box [grid + ql step, grid + qh step] (near_node's planes: the product exact, the sum rounded once)
// meets [qlo, qhi] on all three axes: six compares.  The bound is fixed, every surviving child is visited, a node with surviving siblings left keeps ONE
// stack entry (child_base << 8 | their mask: the ray walks' group, with no octant order), so the stack holds at most one entry per level.  overlap_step
// is the one trip of the project's walks (spira_device.h, "one TRIP") on its pieces: the leaf arm is the SAT above, in T, on the record's own values — the
// tree only prunes — the node arm overlap_node.  The builder partitions the triangles: a walk meets each at most once, and the list needs no duplicate suppression.
//
// Why the growth suffices (normalised units; M = max(|lo|, |hi|) <= 128 by the origin and the extent rule, A = amax_n, u = 2^-24, u_T that of T).  A child
// is wrongly skipped only if a triangle the SAT accepts lies in a child box that misses [qlo, qhi].
//   (a) the query box: c -+ He, less the centre, times scale, in T, then rounded to Float32; He itself is five roundings of T at a magnitude <= 64:
//       <= 3 u_T (M + A) + 5 u_T 64 + u M                                                                    <= 4 u M + 3 u A + 2e-5 = 5.0e-5 at M = 128
//   (b) the child planes: grid + q step rounds once at a magnitude <= A + 1 (near_node's (b))                 <= 6e-8 (1 + A)
//   (c) the SAT's own roundings: the frame transform (the axes are orthonormal to 4 u_T; a dot is three products and two sums) and a projection (two
//       products, one difference; the radius likewise) are each the exact value for vertices moved by eta <= 8 u_T M — the error of
//       u.b f.a - u.a f.b is at most 3 u_T (|u.b f.a| + |u.a f.b|), what moving u by 3 u_T |u| does to it.  So a triangle the SAT accepts is, on every one
//       of the 13 axes, within eta of overlapping the box.  A triangle beyond the ENCLOSING box by a gap d along a world axis is disjoint from the box by
//       at least d; the exact SAT then separates it on one of the 13 axes by d / kappa, where kappa >= 1 depends on which features are closest (1 for
//       face-vertex and edge-edge pairs; a vertex-vertex or vertex-edge pair projects onto a box axis or a cross axis at an angle).  No closed form for
//       kappa is claimed here.  What is held instead: tests/test_overlap_cpu.py places triangles beyond the enclosing box by HALF the growth, 2^-13 (M + 1),
//       along world axes and by 1e-3 (1 + off / 16) along random directions, 10^5 of each per precision at offsets of 0 and 60 units with identity, quarter-turn
//       and random rotations, and the SAT in T rejects every one: kappa eta < 2^-13 (M + 1) on all of them.
//   Every triangle lies inside its child box shrunk by the builder's pad, 1e-4 max(1, A) (spira_bvh.h; the refit pad is never smaller).
// The growth is g = 2^-12 (M + 1) >= 2.4e-4, at M = 128 3.1e-2.  Against it (a) + (b) + eta = 5.0e-5 + 6.1e-5 = 1.1e-4 at M = 128, A <= 1 in Float32: a
// margin of 280 there (of 340 over eta alone at every M: 2^-12 / (8 2^-24) = 512 less the (M + 1) / M), before the pad; that is the room kappa has, and the
// tests above use half of it.  In Float64 eta vanishes and (a) is the conversion's u M.  The growth costs visits only where a box's enclosing box ends
// within g of a child box: at M <= 2 that is 7e-4 of the mesh's size.  The extent bound stays 64: Float32 holds it with this margin, rotated boxes included.
// Valid boxes at 60 .. 64 units with extents just under the bound are held to the scan by tests/test_gpu_overlap.py.
//
// Kernels (each stages the scene with stage_scene: one barrier):
//   k_overlap<T, BVH, TRI, ANY, CAP>    one lane per box, grid-stride: the LDS scan over spheres and LDS triangles (up to 32); BVH: then the walk to the
//                                       end (SPIRA_CAST_INPLACE, or a scene without a tree).
//   k_overlap_session<T, ANY, CAP>      scenes with a tree, the default: SPIRA_REFILLED_SESSION of spira_query.h over session_range of a CastPlan, the ray
//                                       queries' knobs.  start = overlap_load, overlap_scan_local, overlap_enter; step = overlap_step.
//   ANY = true                          only `hit` is written (CAP = 1, unused); a lane whose LDS scan found a candidate never walks, a walking lane leaves
//                                       after the first trip that found one.
//   CAP in {1, 4, 16}                   the list's capacity, the smallest that holds max_list: 1 and 4 on constant indices (registers), 16 indexed at run
//                                       time (scratch memory beside the walk's stack), as the K-nearest lists.
#pragma once
#include <cstdint>

#include "spira_nearest.h"      // near_dot, near_sqrt; spira_query.h: CastLimits, kCastOriginBound, SPIRA_HD

namespace spira {

constexpr uint32_t kOverlapMax = 16;          // SPIRA_MAX_OVERLAP
constexpr int kOverlapExtentBound = 64;       // He_k * scale <= 64 in scenes with a tree, see above
constexpr int kOverlapRegisterCap = 4;        // lists up to this capacity are indexed by constants only

template <class T> SPIRA_HD inline T ovl_abs(T x) {
    if constexpr (sizeof(T) == 4) return __builtin_fabsf(x); else return __builtin_fabs(x);
}
template <class T> SPIRA_HD inline T ovl_min3(T a, T b, T c) {
    if constexpr (sizeof(T) == 4) return __builtin_fminf(__builtin_fminf(a, b), c); else return __builtin_fmin(__builtin_fmin(a, b), c);
}
template <class T> SPIRA_HD inline T ovl_max3(T a, T b, T c) {
    if constexpr (sizeof(T) == 4) return __builtin_fmaxf(__builtin_fmaxf(a, b), c); else return __builtin_fmax(__builtin_fmax(a, b), c);
}

// A prepared box: centre, half extents, the three axes in world coordinates.
template <class T> struct OverlapBox { T c[3], h[3], A[3][3]; };

// The axes of the quaternion q[0..4) = (qx, qy, qz, qw) and n2; A is written whatever n2 is.
template <class T> SPIRA_HD inline T overlap_axes(const T *q, T A[3][3]) {
    const T n2 = (q[0] * q[0] + q[1] * q[1]) + (q[2] * q[2] + q[3] * q[3]);
    const T l = near_sqrt<T>(n2);
    const T x = q[0] / l, y = q[1] / l, z = q[2] / l, w = q[3] / l;
    const T xx = x * x, yy = y * y, zz = z * z, xy = x * y, xz = x * z, yz = y * z, xw = x * w, yw = y * w, zw = z * w;
    A[0][0] = (T)1 - (T)2 * (yy + zz); A[0][1] = (T)2 * (xy + zw);        A[0][2] = (T)2 * (xz - yw);
    A[1][0] = (T)2 * (xy - zw);        A[1][1] = (T)1 - (T)2 * (xx + zz); A[1][2] = (T)2 * (yz + xw);
    A[2][0] = (T)2 * (xz + yw);        A[2][1] = (T)2 * (yz - xw);        A[2][2] = (T)1 - (T)2 * (xx + yy);
    return n2;
}

template <class T> SPIRA_HD inline void overlap_frame(const OverlapBox<T> &B, const T a[3], T out[3]) {
    out[0] = near_dot<T>(B.A[0], a); out[1] = near_dot<T>(B.A[1], a); out[2] = near_dot<T>(B.A[2], a);
}

// One box b[0..10) -> valid?  B: the prepared box; He: the enclosing axis-aligned half extents (both written for boxes valid without a frame).
// frame: the scene has a tree, fr = {centre.x, centre.y, centre.z, scale} (as cast_ray_prepare).
template <class T> SPIRA_HD inline bool overlap_prepare(const T *b, bool frame, const T *fr, OverlapBox<T> &B, T He[3]) {
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int k = 0; k < 10; ++k) if (b[k] != b[k]) return false;                         // NaN anywhere
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int k = 0; k < 10; ++k) if (!((b[k] - b[k]) == (T)0)) return false;             // an infinite value
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int k = 3; k < 6; ++k) if (b[k] < (T)0) return false;
    const T n2 = overlap_axes<T>(b + 6, B.A);
    if (!((n2 - n2) == (T)0) || n2 < CastLimits<T>::min_normal) return false;
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int k = 0; k < 3; ++k) { B.c[k] = b[k]; B.h[k] = b[3 + k]; }
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int k = 0; k < 3; ++k) He[k] = (ovl_abs<T>(B.A[0][k]) * B.h[0] + ovl_abs<T>(B.A[1][k]) * B.h[1]) + ovl_abs<T>(B.A[2][k]) * B.h[2];
    if (frame)
#if defined(__HIPCC__)
#pragma unroll
#endif
        for (int k = 0; k < 3; ++k) {
            const T x = (b[k] - fr[k]) * fr[3];
            if (!(x >= (T)-kCastOriginBound && x <= (T)kCastOriginBound)) return false;
            if (!(He[k] * fr[3] <= (T)kOverlapExtentBound)) return false;
        }
    return true;
}

// One axis: the projections p0, p1, p2 against rad (header comment).  __builtin_isunordered(a, b): a or b is NaN.
template <class T> SPIRA_HD inline bool overlap_axis(T p0, T p1, T p2, T rad) {
    if (__builtin_isunordered(p0, p1) || __builtin_isunordered(p2, rad)) return false;
    return ovl_min3<T>(p0, p1, p2) <= rad && ovl_max3<T>(p0, p1, p2) >= -rad;
}

// The three axes cross(unit_i, f), i = 0, 1, 2, of one edge vector f (box frame).
template <class T> SPIRA_HD inline bool overlap_edge_axes(const T h[3], const T u0[3], const T u1[3], const T u2[3], const T f[3]) {
    bool ok = true;
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int i = 0; i < 3; ++i) {
        const int a = (i + 1) % 3, b = (i + 2) % 3;
        const T fa = f[a], fb = f[b];
        ok &= overlap_axis<T>(u0[b] * fa - u0[a] * fb, u1[b] * fa - u1[a] * fb, u2[b] * fa - u2[a] * fb, ovl_abs<T>(fb) * h[a] + ovl_abs<T>(fa) * h[b]);
    }
    return ok;
}

// The triangle (v0, v0 + e1, v0 + e2) against the box: all 13 axes overlap.
template <class T> SPIRA_HD inline bool overlap_box_triangle(const OverlapBox<T> &B, const T v0[3], const T e1[3], const T e2[3]) {
    const T d0[3] = {v0[0] - B.c[0], v0[1] - B.c[1], v0[2] - B.c[2]};
    T u0[3], f1[3], f2[3];
    overlap_frame<T>(B, d0, u0); overlap_frame<T>(B, e1, f1); overlap_frame<T>(B, e2, f2);
    const T u1[3] = {u0[0] + f1[0], u0[1] + f1[1], u0[2] + f1[2]}, u2[3] = {u0[0] + f2[0], u0[1] + f2[1], u0[2] + f2[2]};
    const T f3[3] = {f2[0] - f1[0], f2[1] - f1[1], f2[2] - f1[2]};
    bool ok = true;      // every axis is evaluated (&, not &&): a lane's early exit would only split its wave
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int k = 0; k < 3; ++k) ok &= overlap_axis<T>(u0[k], u1[k], u2[k], B.h[k]);
    const T n[3] = {f1[1] * f2[2] - f1[2] * f2[1], f1[2] * f2[0] - f1[0] * f2[2], f1[0] * f2[1] - f1[1] * f2[0]};
    const T pn = near_dot<T>(n, u0);
    ok &= overlap_axis<T>(pn, pn, pn, (ovl_abs<T>(n[0]) * B.h[0] + ovl_abs<T>(n[1]) * B.h[1]) + ovl_abs<T>(n[2]) * B.h[2]);
    ok &= n[0] != (T)0 || n[1] != (T)0 || n[2] != (T)0;      // zero area: never a candidate
    ok &= overlap_edge_axes<T>(B.h, u0, u1, u2, f1);
    ok &= overlap_edge_axes<T>(B.h, u0, u1, u2, f2);
    ok &= overlap_edge_axes<T>(B.h, u0, u1, u2, f3);
    return ok;
}

// The shell of the sphere (centre C, radius R) against the box.
template <class T> SPIRA_HD inline bool overlap_box_sphere(const OverlapBox<T> &B, const T C[3], T R) {
    const T d0[3] = {C[0] - B.c[0], C[1] - B.c[1], C[2] - B.c[2]};
    T p[3], e[3], g[3];
    overlap_frame<T>(B, d0, p);
    for (int k = 0; k < 3; ++k) {
        const T a = ovl_abs<T>(p[k]), ek = a - B.h[k];
        e[k] = ek > (T)0 ? ek : (T)0;
        g[k] = a + B.h[k];
    }
    const T dmin2 = near_dot<T>(e, e), dmax2 = near_dot<T>(g, g), R2 = R * R;
    return dmin2 <= R2 && dmax2 >= R2;
}

// One lane's list: n <= K <= CAP object indices, ascending.
template <int CAP> struct OverlapList { int prim[CAP]; uint32_t n; };

// Inserts the candidate `prim` into a list of at most K entries (K <= CAP; K = 0: nothing is kept); a full list drops its last entry, or the candidate when
// that is the larger.  Two forms, near_insert's (spira_knearest.h) and for its reasons: up to capacity 4 the candidate is carried down the list on constant
// indices, so that the list is registers; capacity 16 is an insertion sort's inner loop on run-time indices, which keeps the list in scratch memory.
template <int CAP> SPIRA_HD inline void overlap_insert(OverlapList<CAP> &l, uint32_t K, int prim) {
    const uint32_t n = l.n;
    if constexpr (CAP > kOverlapRegisterCap) {
        if (K == 0) return;
        uint32_t j = K - 1;
        if (n < K) { j = n; l.n = n + 1; }
        else if (!(prim < l.prim[j])) return;
#if defined(__HIPCC__)
#pragma nounroll
#endif
        while (j > 0 && prim < l.prim[j - 1]) { l.prim[j] = l.prim[j - 1]; --j; }
        l.prim[j] = prim;
    } else {
        int cp = prim;
#if defined(__HIPCC__)
#pragma unroll
#endif
        for (int j = 0; j < CAP; ++j) {
            const bool take = (uint32_t)j < K && (((uint32_t)j < n && cp < l.prim[j]) || (uint32_t)j == n);
            const int tp = l.prim[j];
            l.prim[j] = take ? cp : tp;
            cp = take ? tp : cp;
        }
        if (n < K) l.n = n + 1;
    }
}

}  // namespace spira

#if defined(__HIPCC__)
// Refill threshold and waves per CU of the session kernel: the loop k_cast_session runs, with its knobs (SPIRA_CAST_REFILL, SPIRA_CAST_WAVES_PER_CU; CastKnobs,
// read per call as cast reads them); docs/experiments.md, "box overlap queries", says what has and has not been measured.
namespace spira {

template <class T> struct OverlapArgs {
    SceneGlobal<T> scene;
    const T *boxes;                  // n x 10
    uint32_t n;
    int *prim;                       // n x max_list; may be NULL
    uint32_t *count;                 // n; may be NULL
    uint8_t *hit;                    // the any form (ANY): n
    uint32_t *trips;                 // diagnostic, may be NULL
    uint32_t max_list;               // K: 0 .. CAP of the kernel launched
    uint32_t base, rem;              // session: wave w owns base + (w < rem) boxes from w base + min(w, rem)  (CastPlan)
    uint32_t refill_free;
};

// One lane's query: the box, the grown enclosing box in the tree's frame, the walk, the candidates.
template <class T, int CAP> struct OverlapWalk {
    OverlapBox<T> B;
    T He[3];
    float qlo[3], qhi[3];
    uint32_t G;              // child_base << 8 | children still to visit, bit = slot
    uint32_t tw, rank;       // as NearWalk: surviving leaf slots << 24 | tri_base; the node's leaf ranks
    uint32_t sp;
    uint32_t trips;
    uint32_t total;          // candidates met
    OverlapList<CAP> l;
};

// (W: OverlapWalk<T, CAP>, or the walk of a query that shares the answer — spira_trioverlap.h.)
template <class T, bool ANY, int CAP, class W>
__device__ __forceinline__ void overlap_store(const OverlapArgs<T> &a, uint32_t i, bool valid, const W &w) {
    if (ANY) { a.hit[i] = valid ? (w.total ? (uint8_t)1 : (uint8_t)0) : (uint8_t)255; if (a.trips) a.trips[i] = w.trips; return; }
    const uint32_t K = a.max_list;
    if (a.prim) {
        int *o = a.prim + (size_t)i * K;
        const int none = valid ? SPIRA_RAY_MISS : SPIRA_RAY_INVALID;
        if constexpr (CAP <= kOverlapRegisterCap) {
#pragma unroll
            for (int j = 0; j < CAP; ++j)
                if ((uint32_t)j < K) o[j] = (uint32_t)j < w.l.n ? w.l.prim[j] : none;      // (an invalid box's list is empty)
        } else {
#pragma nounroll
            for (uint32_t j = 0; j < K; ++j) {
                int p = none;
                if (j < w.l.n) p = w.l.prim[j];
                o[j] = p;
            }
        }
    }
    if (a.count) a.count[i] = valid ? w.total : 0u;
    if (a.trips) a.trips[i] = w.trips;
}

// Loads box i, classifies it and starts the lane's state.  Returns the validity.
template <class T, int CAP>
__device__ __forceinline__ bool overlap_load(const OverlapArgs<T> &a, const SceneLds<T> &sc, bool frame, uint32_t i, OverlapWalk<T, CAP> &w) {
    const T *bp = a.boxes + 10 * (size_t)i;
    T b[10], fr[4] = {(T)0, (T)0, (T)0, (T)1};
#pragma unroll
    for (int k = 0; k < 10; ++k) b[k] = bp[k];
    if (frame) { const Pack4<T> f = sc.bvh_root[2]; fr[0] = f.x; fr[1] = f.y; fr[2] = f.z; fr[3] = f.w; }
#pragma unroll
    for (int k = 0; k < 3; ++k) { w.B.c[k] = (T)0; w.B.h[k] = (T)0; w.He[k] = (T)0; w.B.A[k][0] = w.B.A[k][1] = w.B.A[k][2] = (T)0; }
    const bool ok = overlap_prepare<T>(b, frame, fr, w.B, w.He);
    w.G = 0; w.tw = 0; w.rank = 0; w.sp = 0; w.trips = 0; w.total = 0;
    if constexpr (CAP <= kOverlapRegisterCap) {
#pragma unroll
        for (int j = 0; j < CAP; ++j) w.l.prim[j] = SPIRA_RAY_MISS;
    }
    w.l.n = 0;
    return ok;
}

template <class T, int CAP, class W> __device__ __forceinline__ void overlap_take(W &w, uint32_t K, int p) {
    ++w.total;
    overlap_insert<CAP>(w.l, K, p);
}

// The LDS part of the scan, in scan order: spheres (radius from spheres5), then the LDS triangles.
template <class T, bool TRI, bool ANY, int CAP>
__device__ __forceinline__ void overlap_scan_local(const OverlapArgs<T> &a, const SceneLds<T> &sc, OverlapWalk<T, CAP> &w, uint32_t K) {
    for (uint32_t s = 0; s < sc.n_spheres; ++s) {
        const Pack4<T> sp = sc.sph[s];
        const T c[3] = {sp.x, sp.y, sp.z};
        if (overlap_box_sphere<T>(w.B, c, a.scene.spheres5[5 * (size_t)s + 3])) {
            overlap_take<T, CAP>(w, K, (int)s);
            if (ANY) return;
        }
    }
    if (TRI)
        for (uint32_t i = 0; i < sc.n_triangles; ++i) {
            const Pack4<T> a0 = sc.tri[3 * i], a1 = sc.tri[3 * i + 1], a2 = sc.tri[3 * i + 2];
            const T v0[3] = {a0.x, a0.y, a0.z}, e1[3] = {a1.x, a1.y, a1.z}, e2[3] = {a2.x, a2.y, a2.z};
            if (overlap_box_triangle<T>(w.B, v0, e1, e2)) {
                overlap_take<T, CAP>(w, K, (int)(sc.n_spheres + i));
                if (ANY) return;
            }
        }
}

// The enclosing box in the tree's frame, Float32, grown (header comment, "The walk"); the walk starts at the root node.
template <class T, int CAP>
__device__ __forceinline__ void overlap_enter(const SceneLds<T> &sc, OverlapWalk<T, CAP> &w) {
    const Pack4<T> fr = sc.bvh_root[2];
    const T ctr[3] = {fr.x, fr.y, fr.z};
    float m = 0.0f;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        w.qlo[k] = (float)(((w.B.c[k] - w.He[k]) - ctr[k]) * fr.w);
        w.qhi[k] = (float)(((w.B.c[k] + w.He[k]) - ctr[k]) * fr.w);
        m = __builtin_fmaxf(m, __builtin_fmaxf(__builtin_fabsf(w.qlo[k]), __builtin_fabsf(w.qhi[k])));
    }
    const float g = (m + 1.0f) * 0.000244140625f;      // 2^-12
#pragma unroll
    for (int k = 0; k < 3; ++k) { w.qlo[k] -= g; w.qhi[k] += g; }
    w.G = 1u; w.tw = 0; w.rank = 0; w.sp = 0;           // the root: a group holding only slot 0 of base 0
}

// One node: its 8 dequantised child boxes against [qlo, qhi].  Returns the present children that meet it, bit = slot.
__device__ __forceinline__ uint32_t overlap_node(const uint4 w0, const uint4 w2, const uint4 w3, const uint4 w4, const float qlo[3], const float qhi[3]) {
    const float sx = __uint_as_float((w0.w & 0xFFu) << 23), sy = __uint_as_float(((w0.w >> 8) & 0xFFu) << 23), sz = __uint_as_float(((w0.w >> 16) & 0xFFu) << 23);
    const float gx = __uint_as_float(w0.x), gy = __uint_as_float(w0.y), gz = __uint_as_float(w0.z);
    const uint32_t lox[2] = {w2.x, w2.y}, loy[2] = {w2.z, w2.w}, loz[2] = {w3.x, w3.y}, hix[2] = {w3.z, w3.w}, hiy[2] = {w4.x, w4.y}, hiz[2] = {w4.z, w4.w};
    uint32_t surv = 0;
#pragma unroll
    for (int s = 0; s < 8; ++s) {
        const int h = s >> 2, sh = 8 * (s & 3);
        const float qlx = (float)((lox[h] >> sh) & 0xFFu), qhx = (float)((hix[h] >> sh) & 0xFFu);
        const float qly = (float)((loy[h] >> sh) & 0xFFu), qhy = (float)((hiy[h] >> sh) & 0xFFu);
        const float qlz = (float)((loz[h] >> sh) & 0xFFu), qhz = (float)((hiz[h] >> sh) & 0xFFu);
        const bool hit = qlx <= qhx                                       // present: an empty child has lo 255, hi 0
                         && gx + qlx * sx <= qhi[0] && gx + qhx * sx >= qlo[0]
                         && gy + qly * sy <= qhi[1] && gy + qhy * sy >= qlo[1]
                         && gz + qlz * sz <= qhi[2] && gz + qhz * sz >= qlo[2];
        if (hit) surv |= 1u << s;
    }
    return surv;
}

// One trip of an overlap walk = ONE memory round trip (header comment, "The walk"), on the pieces of spira_device.h ("one TRIP") with the overlap's own
// node arm; no octant (the children are taken in slot order), the stack is private.  leaf(v0, e1, e2, id): the query's leaf arm on the record's own values
// and the triangle's index within the mesh.  Returns false when the walk is over.
template <class T, class W, class Leaf>
__device__ __forceinline__ bool overlap_trip(const SceneLds<T> &sc, W &w, uint32_t *stack, Leaf &&leaf) {
    const bool is_tri = (w.tw >> 24) != 0;
    const uint4 *ptr;
    if (is_tri) ptr = reinterpret_cast<const uint4 *>(sc.bvh_tris + 3 * (size_t)walk_take_tri(w));
    else ptr = sc.bvh_nodes + 5 * (size_t)walk_take_group(w, 0u, stack);
    ++w.trips;
    uint4 w0, w1, w2, w3, w4, w5;
    walk_load_one<kTriWords<T>, false>(ptr, w0, w1, w2, w3, w4, w5);
    if (is_tri) {
        Pack4<T> a0, a1, a2;
        bvh8_tri_words(w0, w1, w2, w3, w4, w5, a0, a1, a2);
        const T v0[3] = {a0.x, a0.y, a0.z}, e1[3] = {a1.x, a1.y, a1.z}, e2[3] = {a2.x, a2.y, a2.z};
        leaf(v0, e1, e2, Bits<T>::to_u32(a0.w));
    } else {
        const uint32_t imask = w0.w >> 24;
        const uint32_t surv = overlap_node(w0, w2, w3, w4, w.qlo, w.qhi);
        w.G = (w1.x << 8) | (surv & imask);
        w.tw = w1.y | ((surv & ~imask) << 24);
        w.rank = w1.z;
    }
    return walk_pop(w, stack);
}

// One trip of the box walk: the leaf arm is the 13-axis SAT.
template <class T, int CAP>
__device__ __forceinline__ bool overlap_step(const SceneLds<T> &sc, OverlapWalk<T, CAP> &w, int base, uint32_t K, uint32_t *stack) {
    return overlap_trip<T>(sc, w, stack, [&](const T v0[3], const T e1[3], const T e2[3], uint32_t id) {
        if (overlap_box_triangle<T>(w.B, v0, e1, e2)) overlap_take<T, CAP>(w, K, base + (int)id);
    });
}

// One lane per box.  Launches: <T, false, false, ..> spheres alone, <T, false, true, ..> with LDS triangles, <T, true, false, ..> a BVH mesh (SPIRA_CAST_INPLACE).
template <class T, bool BVH, bool TRI, bool ANY, int CAP>
__global__ __launch_bounds__(kBlock) void k_overlap(const OverlapArgs<T> a) {
    extern __shared__ __attribute__((aligned(32))) unsigned char lds_raw[];
    const SceneLds<T> sc = stage_scene<T>(a.scene, lds_raw);     // the only workgroup barrier of the kernel
    const uint32_t K = ANY ? 0u : a.max_list;
    const int base = (int)(sc.n_spheres + sc.n_triangles);
    for (uint32_t i = blockIdx.x * kBlock + threadIdx.x; i < a.n; i += gridDim.x * kBlock) {
        OverlapWalk<T, CAP> w;
        const bool ok = overlap_load<T, CAP>(a, sc, BVH, i, w);
        if (ok) {
            overlap_scan_local<T, TRI, ANY, CAP>(a, sc, w, K);
            if (BVH && !(ANY && w.total)) {
                uint32_t stack[kBvhStackD];
                overlap_enter<T, CAP>(sc, w);
                while (overlap_step<T, CAP>(sc, w, base, K, stack) && !(ANY && w.total)) {}
            }
        }
        overlap_store<T, ANY, CAP>(a, i, ok, w);
    }
}

// Scenes with a tree: a refilled session per wave over its range of the caller's list (SPIRA_REFILLED_SESSION of spira_query.h).
template <class T, bool ANY, int CAP>
__global__ __launch_bounds__(kBlock) void k_overlap_session(const OverlapArgs<T> a) {
    extern __shared__ __attribute__((aligned(32))) unsigned char lds_raw[];
    const SceneLds<T> sc = stage_scene<T>(a.scene, lds_raw);     // the only workgroup barrier of the kernel
    uint32_t begin, end;
    session_range(a.base, a.rem, begin, end);
    uint32_t stack[kBvhStackD];
    const uint32_t K = ANY ? 0u : a.max_list;
    const int base = (int)(sc.n_spheres + sc.n_triangles);
    uint32_t item_ = 0;
    OverlapWalk<T, CAP> w{};
    const auto start = [&](uint32_t item) -> bool {
            item_ = item;
            const bool ok = overlap_load<T, CAP>(a, sc, true, item_, w);
            bool walks = false;
            if (ok) {
                overlap_scan_local<T, false, ANY, CAP>(a, sc, w, K);
                if (!(ANY && w.total)) { overlap_enter<T, CAP>(sc, w); walks = true; }
            }
            if (!walks) overlap_store<T, ANY, CAP>(a, item_, ok, w);
            return walks;
    };
    const auto step = [&]() -> bool {
            if (overlap_step<T, CAP>(sc, w, base, K, stack) && !(ANY && w.total)) return true;
            overlap_store<T, ANY, CAP>(a, item_, true, w);
            return false;
    };
    SPIRA_REFILLED_SESSION(begin, end, a.refill_free, start, step);
}

}  // namespace spira
#endif
