// spira_nearest.h — closest-point queries on a scene handle (spira_scene_closest_point_*): for every point of a caller's list, the nearest point of the
// scene's surface.  Included by spira_hip.hip behind spira_query.h (CastLimits, kCastOriginBound, CastPlan's knobs, the refilled session's loop); the
// tree is the one create, update and rebuild maintain — it is walked a second way.  The first part of this file needs no HIP header: a CPU program
// (tests/native/nearest_plan.cpp) and the exported host arithmetic (spira_closest_point_triangle_*) call the very functions the kernels call.
//
// A point is four values of the call's precision T: [px py pz r_max].  The answer is that of a scan over spheres [0..) then triangles [0..) in the caller's
// order: best = r_max * r_max (in T); object k replaces the winner exactly when d2_k <= best (ties to the LATER object, a NaN d2 never wins), then
// best = d2_k.  All arithmetic in T, in the written order, nothing fused (-ffp-contract=off).  dot(a, b) is ALWAYS (a.x b.x + a.y b.y) + a.z b.z.
//
// Triangle (closest_point_triangle), on the values the LDS records and the tree's triangle records hold: v0, e1 = v1 - v0, e2 = v2 - v0 (differences in T).
// Ericson's region walk (Real-Time Collision Detection, 5.1.5) with ap = p - v0, bp = ap - e1, cp = ap - e2.  The tests, in THIS order, first match wins:
//   1. d1 = dot(e1, ap), d2 = dot(e2, ap);            d1 <= 0 && d2 <= 0                        vertex v0:  q = v0
//   2. d3 = dot(e1, bp), d4 = dot(e2, bp);            d3 >= 0 && d4 <= d3                       vertex v1:  q = v0 + e1
//   3. vc = d1 d4 - d3 d2;                            vc <= 0 && d1 >= 0 && d3 <= 0             edge v0 v1: v = d1 / (d1 - d3),  q = v0 + e1 v
//   4. d5 = dot(e1, cp), d6 = dot(e2, cp);            d6 >= 0 && d5 <= d6                       vertex v2:  q = v0 + e2
//   5. vb = d5 d2 - d1 d6;                            vb <= 0 && d2 >= 0 && d6 <= 0             edge v0 v2: w = d2 / (d2 - d6),  q = v0 + e2 w
//   6. va = d3 d6 - d5 d4, g = d4 - d3, h = d5 - d6;  va <= 0 && g >= 0 && h >= 0               edge v1 v2: w = g / (g + h),     q = (v0 + e1) + (e2 - e1) w
//   7. otherwise the face:                            s = 1 / ((va + vb) + vc), v = vb s, w = vc s,         q = (v0 + e1 v) + e2 w
// Divisions: the three quotients of 3, 5, 6 and the one reciprocal of 7, the compiler's IEEE division; nothing else divides.  Every comparison is false
// for a NaN, so a triangle of zero area falls through to 7 (or divides 0 by 0 on the way) and comes out as NaN, which the scan never picks.
// Then, for both kinds of object:  r = p - q,  d2 = (r.x r.x + r.y r.y) + r.z r.z.
// Sphere (closest_point_sphere), centre c and radius r as the caller gave them: w = p - c, l = sqrt(dot(w, w)); l >= the smallest normal number of T:
// q = c + w (r / l) (one division, then three products); otherwise q = c + (r, 0, 0).  The LDS sphere record holds fl(r r), whose square root need not be
// r again (r r rounds, and underflows or overflows for extreme radii), so the kernels read the radius from spheres5.
//
// Validity (nearest_point_prepare): a point is INVALID when any of its four values is NaN, a coordinate is infinite, r_max < 0, or — scenes with a tree
// only — the origin rule of the ray queries fails for p: |(p_k - centre_k) * scale| <= 64 on every axis, in T (spira_query.h).  r_max = +Inf is valid.
//
// Why pruning is safe.  The walk computes, in Float32 and in the tree's normalised frame, a lower bound lb of the squared distance from the point to a
// child's quantised box, and skips the child when  lb (1 - 2^-18) > bestn,  bestn = fl32((best scale) scale) (1 + 2^-20) + 2^-100  (rounded UP: the factor
// covers the conversion's half ulp, the addend a result that underflows).  That must imply that the SCAN's d2 of every triangle of the child exceeds best.
// In normalised units, with A = amax_n (the mesh's largest coordinate) and u = 2^-24 (Float32; 2^-53 for T = double, where only the box side stays Float32):
//   (a) the point: p_n = fl((p - centre) scale) in T, then rounded to Float32.  |p_n| <= 64 by the rule, so each coordinate is off by at most
//       u (|p| + |centre|) scale + 2 u 64 <= u (2 A + 64) + 128 u                                         <= 1.2e-5 + 1.2e-7 A
//   (b) the box: plane = p_grid + q step with q <= 255 and step a power of two: the product is exact, the sum rounds once at a magnitude <= A + 1:
//       <= u (A + 1); the builder already placed the planes outside the padded child box in exact arithmetic (spira_bvh.h)    <= 6e-8 (1 + A)
//   (c) the squared sum: three differences, three squares, two sums, each within u relative: lb is within 6 u of the squared distance between the rounded
//       point and the rounded box, and the factor (1 - 2^-18) = 1 - 64 u shrinks it by ten times that.
//   (d) the scan's side: q of the leaf test lies within a few ulps of the coordinates — 4 u (A + 1) — of a point of the triangle whenever its barycentric
//       coordinates come out within [0, 1], which regions 1 .. 6 guarantee by construction (each quotient is n / (n + m) with n, m >= 0) and region 7 up to the
//       rounding of va, vb, vc; r = p - q adds u (64 + A); so sqrt(d2_scan) >= dist(p, triangle) - 6 u (A + 64).                  <= 2.3e-5 + 3.6e-7 A
// Every triangle of a child lies inside the child's box SHRUNK by the builder's pad, 1e-4 max(1, A) (the refit pad is never smaller: spira_refit.h), and a
// child is only ever skipped when the point is outside its box (lb > 0).  For a point outside a box, moving every face inward by `pad` raises the distance
// by at least pad (sum_k (g_k + pad)^2 >= (sqrt(sum_k g_k^2) + pad)^2 over the axes it is outside on).  So dist(p, triangle) >= dist(p, box) + pad, and the
// errors (a) + (b) + (d) total about 3.6e-5 + 5.4e-7 A against 1e-4 max(1, A): a margin of 2.7 at A <= 1, of more than 100 for a mesh far from the origin —
// somewhat less than the cast's 8 (the point's two roundings and the leaf's q both count here) but closed, so the origin bound stays 64 for this entry.
// In Float64 (a) and (d) are 2^-29 times smaller and (b) alone remains, 6e-8 (1 + A) against 1e-4 + 1e-9 A: holds while A <= about 1 600 mesh sizes;
// beyond that the Float64 pad is the renderer's own limit (spira_bvh.h, "Padding"), not this walk's.  The test is STRICT and the margin is on the side of
// keeping: a child at exactly the winning distance is visited, so among equal distances the later triangle is still reached.
// The root box (caller's coordinates, T, rounded outward by the builder) is tested the same way in T: skipped when d2_root 0.99999 > best.
//
// Kernels (each stages the scene with stage_scene: one barrier):
//   k_nearest<T, BVH, TRI>     one lane per point, grid-stride: the LDS scan over spheres and LDS triangles; BVH: then the walk to the end (SPIRA_CAST_INPLACE).
//   k_nearest_session<T>       scenes with a tree, the default: SPIRA_REFILLED_SESSION of spira_query.h, the loop k_cast_session runs — persistent waves own
//                              contiguous ranges of the point list (session_range over a CastPlan), free lanes refill by ballot and popcount prefix while
//                              the others keep walking, a finished lane stores straight to out[point].  The kernel is the two callables: start = near_load,
//                              near_scan_local, near_enter; step = near_step.
// The walk (near_trip, whose leaf near_step supplies; the pieces of a trip: spira_device.h, "one TRIP"): ONE memory round trip per trip — a triangle record for a lane with leaf children pending (the scan's own function on the record's
// own values, in T: the tree only prunes), else a node: its eight child boxes are dequantised, each child's squared distance is computed, children
// proven farther than best are dropped, the surviving leaves become the pending triangles and the NEAREST surviving child node is visited next.
// The stack: the other surviving child nodes are deferred as ONE entry, (slot of THIS node) << 8 | their bit mask.  A popped entry is a trip that fetches that
// node again and decides among the deferred children with the best of THAT moment — nearest first again, the rest pushed back as one entry.  So a node on the
// current root-to-leaf path owns at most one entry and the stack never holds more than the tree's depth (< kBvhStack - 2 <= kBvhStackD), the bound of the
// ray walk; a stack of (child, distance) pairs would need 7 per level and spill.  The entry is 24 bits of slot (the builder's limit) and 8 of mask.
#pragma once
#include <cstdint>

#include "spira_query.h"        // CastLimits, kCastOriginBound, SPIRA_HD

namespace spira {

template <class T> SPIRA_HD inline T near_dot(const T a[3], const T b[3]) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }
template <class T> SPIRA_HD inline T near_sqrt(T x) {
    if constexpr (sizeof(T) == 4) return __builtin_sqrtf(x); else return __builtin_sqrt(x);
}
// r = p - q, d2 = dot(r, r): the one formula of both object kinds
template <class T> SPIRA_HD inline T near_d2(const T p[3], const T q[3]) {
    const T r[3] = {p[0] - q[0], p[1] - q[1], p[2] - q[2]};
    return near_dot<T>(r, r);
}

// The closest point q of the triangle (v0, v0 + e1, v0 + e2) to p and its squared distance (header comment: the region order, the dots, the divisions).
template <class T> SPIRA_HD inline void closest_point_triangle(const T v0[3], const T e1[3], const T e2[3], const T p[3], T q[3], T &d2out) {
    const T ap[3] = {p[0] - v0[0], p[1] - v0[1], p[2] - v0[2]};
    const T d1 = near_dot<T>(e1, ap), d2 = near_dot<T>(e2, ap);
    const T bp[3] = {ap[0] - e1[0], ap[1] - e1[1], ap[2] - e1[2]};
    const T d3 = near_dot<T>(e1, bp), d4 = near_dot<T>(e2, bp);
    const T cp[3] = {ap[0] - e2[0], ap[1] - e2[1], ap[2] - e2[2]};
    const T d5 = near_dot<T>(e1, cp), d6 = near_dot<T>(e2, cp);
    if (d1 <= (T)0 && d2 <= (T)0) { for (int k = 0; k < 3; ++k) q[k] = v0[k]; }
    else if (d3 >= (T)0 && d4 <= d3) { for (int k = 0; k < 3; ++k) q[k] = v0[k] + e1[k]; }
    else {
        const T vc = d1 * d4 - d3 * d2;
        if (vc <= (T)0 && d1 >= (T)0 && d3 <= (T)0) { const T v = d1 / (d1 - d3); for (int k = 0; k < 3; ++k) q[k] = v0[k] + e1[k] * v; }
        else if (d6 >= (T)0 && d5 <= d6) { for (int k = 0; k < 3; ++k) q[k] = v0[k] + e2[k]; }
        else {
            const T vb = d5 * d2 - d1 * d6;
            if (vb <= (T)0 && d2 >= (T)0 && d6 <= (T)0) { const T w = d2 / (d2 - d6); for (int k = 0; k < 3; ++k) q[k] = v0[k] + e2[k] * w; }
            else {
                const T va = d3 * d6 - d5 * d4, g = d4 - d3, h = d5 - d6;
                if (va <= (T)0 && g >= (T)0 && h >= (T)0) { const T w = g / (g + h); for (int k = 0; k < 3; ++k) q[k] = (v0[k] + e1[k]) + (e2[k] - e1[k]) * w; }
                else { const T s = (T)1 / ((va + vb) + vc), v = vb * s, w = vc * s; for (int k = 0; k < 3; ++k) q[k] = (v0[k] + e1[k] * v) + e2[k] * w; }
            }
        }
    }
    d2out = near_d2<T>(p, q);
}

// The closest point of the sphere (centre c, radius r) to p and its squared distance.
template <class T> SPIRA_HD inline void closest_point_sphere(const T c[3], T r, const T p[3], T q[3], T &d2out) {
    const T w[3] = {p[0] - c[0], p[1] - c[1], p[2] - c[2]};
    const T l = near_sqrt<T>(near_dot<T>(w, w));
    if (l >= CastLimits<T>::min_normal) { const T s = r / l; for (int k = 0; k < 3; ++k) q[k] = c[k] + w[k] * s; }
    else { q[0] = c[0] + r; q[1] = c[1] + (T)0; q[2] = c[2] + (T)0; }
    d2out = near_d2<T>(p, q);
}

// One point pt[0..4) = [px py pz r_max] -> valid?  frame: the scene has a tree, fr = {centre.x, centre.y, centre.z, scale} (as cast_ray_prepare).
template <class T> SPIRA_HD inline bool nearest_point_prepare(const T *pt, bool frame, const T *fr) {
    for (int k = 0; k < 4; ++k) if (pt[k] != pt[k]) return false;                       // NaN anywhere
    for (int k = 0; k < 3; ++k) if (!((pt[k] - pt[k]) == (T)0)) return false;           // an infinite coordinate
    if (pt[3] < (T)0) return false;
    if (frame)
        for (int k = 0; k < 3; ++k) {
            const T x = (pt[k] - fr[k]) * fr[3];
            if (!(x >= (T)-kCastOriginBound && x <= (T)kCastOriginBound)) return false;
        }
    return true;
}

}  // namespace spira

#if defined(__HIPCC__)
// Refill threshold and waves per CU of the session kernel: the loop k_cast_session runs, so its knobs (SPIRA_CAST_REFILL, SPIRA_CAST_WAVES_PER_CU; CastKnobs, read
// per call as cast reads them) are the starting point; docs/experiments.md, "closest-point queries", says what a sweep on the device kept.
namespace spira {

template <class T> struct NearestArgs {
    SceneGlobal<T> scene;
    const T *points;                 // n_points x 4
    uint32_t n_points;
    int *prim; T *dist; T *point;    // n_points, n_points, n_points x 3 (interleaved); any may be NULL
    uint32_t *trips;                 // diagnostic, may be NULL
    uint32_t base, rem;              // session: wave w owns base + (w < rem) points from w base + min(w, rem)  (CastPlan)
    uint32_t refill_free;
};

// One lane's query: the point, the scan's state and the walk's.
template <class T> struct NearWalk {
    T p[3], q[3];            // the point; the winner's closest point
    T best;                  // the scan's best (squared distance)
    int prim;
    float nx, ny, nz;        // the point in the tree's normalised frame
    float bestn;             // best in normalised units, rounded up
    uint32_t G;              // the node to visit next: slot << 8 | the children that may be taken (0xFF: a first visit; a popped entry: the deferred ones); 0: none
    uint32_t tw;             // triangles of the last node still to test: surviving leaf slots << 24 | the node's tri_base
    uint32_t rank;           // the node's leaf ranks (4 bits per slot)
    uint32_t sp;
    uint32_t trips;
};

template <class T> __device__ __forceinline__ float near_bestn(T best, T scale) {
    return (float)((best * scale) * scale) * 1.00000095367431640625f + 7.888609052210118e-31f;      // (1 + 2^-20), 2^-100: rounded up for sure
}

template <class T>
__device__ __forceinline__ void near_store(const NearestArgs<T> &a, uint32_t i, bool valid, const NearWalk<T> &w, T r_max) {
    const bool hit = valid && w.prim >= 0;
    if (a.prim) a.prim[i] = valid ? w.prim : SPIRA_RAY_INVALID;
    if (a.dist) a.dist[i] = !valid ? (T)0 : (hit ? near_sqrt<T>(w.best) : r_max);
    if (a.point) { a.point[3 * (size_t)i] = hit ? w.q[0] : (T)0; a.point[3 * (size_t)i + 1] = hit ? w.q[1] : (T)0; a.point[3 * (size_t)i + 2] = hit ? w.q[2] : (T)0; }
    if (a.trips) a.trips[i] = w.trips;
}

// Loads point i, classifies it and starts the scan's state.  Returns the validity; r_max out.
template <class T>
__device__ __forceinline__ bool near_load(const NearestArgs<T> &a, const SceneLds<T> &sc, bool frame, uint32_t i, NearWalk<T> &w, T &r_max) {
    const T *pp = a.points + 4 * (size_t)i;
    T pt[4], fr[4] = {(T)0, (T)0, (T)0, (T)1};
#pragma unroll
    for (int k = 0; k < 4; ++k) pt[k] = pp[k];
    if (frame) { const Pack4<T> f = sc.bvh_root[2]; fr[0] = f.x; fr[1] = f.y; fr[2] = f.z; fr[3] = f.w; }
    const bool ok = nearest_point_prepare<T>(pt, frame, fr);
    w.p[0] = pt[0]; w.p[1] = pt[1]; w.p[2] = pt[2];
    w.q[0] = w.q[1] = w.q[2] = (T)0;
    r_max = pt[3];
    w.best = pt[3] * pt[3]; w.prim = -1; w.trips = 0;
    w.G = 0; w.tw = 0; w.rank = 0; w.sp = 0;
    return ok;
}

template <class T> __device__ __forceinline__ void near_take(NearWalk<T> &w, const T q[3], T d2, int p) {
    if (d2 <= w.best) { w.best = d2; w.prim = p; w.q[0] = q[0]; w.q[1] = q[1]; w.q[2] = q[2]; }      // in scan order: ties to the later object, NaN never
}

// The LDS part of the scan: spheres (radius from spheres5, see the header comment), then the LDS triangles.
template <class T, bool TRI>
__device__ __forceinline__ void near_scan_local(const NearestArgs<T> &a, const SceneLds<T> &sc, NearWalk<T> &w) {
    for (uint32_t s = 0; s < sc.n_spheres; ++s) {
        const Pack4<T> sp = sc.sph[s];
        const T c[3] = {sp.x, sp.y, sp.z};
        T q[3], d2;
        closest_point_sphere<T>(c, a.scene.spheres5[5 * (size_t)s + 3], w.p, q, d2);
        near_take<T>(w, q, d2, (int)s);
    }
    if (TRI)
        for (uint32_t t = 0; t < sc.n_triangles; ++t) {
            const Pack4<T> a0 = sc.tri[3 * t], a1 = sc.tri[3 * t + 1], a2 = sc.tri[3 * t + 2];
            const T v0[3] = {a0.x, a0.y, a0.z}, e1[3] = {a1.x, a1.y, a1.z}, e2[3] = {a2.x, a2.y, a2.z};
            T q[3], d2;
            closest_point_triangle<T>(v0, e1, e2, w.p, q, d2);
            near_take<T>(w, q, d2, (int)(sc.n_spheres + t));
        }
}

// The root box in T, then the Float32 side.  false: no triangle of the mesh can be within best.
template <class T>
__device__ __forceinline__ bool near_enter(const SceneLds<T> &sc, NearWalk<T> &w) {
    const Pack4<T> mn = sc.bvh_root[0], mx = sc.bvh_root[1], fr = sc.bvh_root[2];
    const T dx = max_nn(max_nn(mn.x - w.p[0], w.p[0] - mx.x), (T)0), dy = max_nn(max_nn(mn.y - w.p[1], w.p[1] - mx.y), (T)0),
            dz = max_nn(max_nn(mn.z - w.p[2], w.p[2] - mx.z), (T)0);
    const T d2r = (dx * dx + dy * dy) + dz * dz;
    if (d2r * (T)0.99999 > w.best) return false;
    w.nx = (float)((w.p[0] - fr.x) * fr.w); w.ny = (float)((w.p[1] - fr.y) * fr.w); w.nz = (float)((w.p[2] - fr.z) * fr.w);
    w.bestn = near_bestn<T>(w.best, fr.w);
    w.G = 0xFFu; w.tw = 0; w.rank = 0; w.sp = 0;          // the root: slot 0, every child allowed
    return true;
}

// One node: the squared distance from the point to each of the 8 child boxes.  Out: surv = children that are present and not proven farther than bestn.
__device__ __forceinline__ uint32_t near_node(const uint4 w0, const uint4 w2, const uint4 w3, const uint4 w4, float nx, float ny, float nz, float bestn, float d2[8]) {
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
        const float dx = __builtin_fmaxf(__builtin_fmaxf((gx + qlx * sx) - nx, nx - (gx + qhx * sx)), 0.0f);
        const float dy = __builtin_fmaxf(__builtin_fmaxf((gy + qly * sy) - ny, ny - (gy + qhy * sy)), 0.0f);
        const float dz = __builtin_fmaxf(__builtin_fmaxf((gz + qlz * sz) - nz, nz - (gz + qhz * sz)), 0.0f);
        const float d = (dx * dx + dy * dy) + dz * dz;
        d2[s] = d;
        // present (an empty child has lo 255, hi 0) and not proven farther: lb (1 - 2^-18) > bestn drops it — strictly, so equal distances are kept
        if (qlx <= qhx && !(d * 0.999996185302734375f > bestn)) surv |= 1u << s;
    }
    return surv;
}

// One trip of the distance walks = ONE memory round trip (header comment, "The walk"; the pieces and why the loads are what they are: spira_device.h,
// "one TRIP").  The leaf arm is the scan's own function on the record; what becomes of the triangle is the caller's, `leaf(ti, q, d2, p)`.  The node arm
// visits the nearest surviving child first and keeps ONE deferred entry per node.  Returns false when the walk is over.
template <class T, class Leaf>
__device__ __forceinline__ bool near_trip(const SceneLds<T> &sc, NearWalk<T> &w, int base, uint32_t *stack, const Leaf &leaf) {
    const bool is_tri = (w.tw >> 24) != 0;
    const uint4 *ptr;
    uint32_t idx = 0, allow = 0, ti = 0;
    if (is_tri) {
        ti = walk_take_tri(w);
        ptr = reinterpret_cast<const uint4 *>(sc.bvh_tris + 3 * (size_t)ti);
    } else {
        idx = w.G >> 8; allow = w.G & 0xFFu;                               // (never empty here)
        w.G = 0;
        ptr = sc.bvh_nodes + 5 * (size_t)idx;
    }
    ++w.trips;
    uint4 w0, w1, w2, w3, w4, w5;
    walk_load_one<kTriWords<T>, false>(ptr, w0, w1, w2, w3, w4, w5);
    if (is_tri) {
        Pack4<T> a0, a1, a2;
        bvh8_tri_words(w0, w1, w2, w3, w4, w5, a0, a1, a2);
        const T v0[3] = {a0.x, a0.y, a0.z}, e1[3] = {a1.x, a1.y, a1.z}, e2[3] = {a2.x, a2.y, a2.z};
        T q[3], d2;
        closest_point_triangle<T>(v0, e1, e2, w.p, q, d2);
        leaf(ti, q, d2, base + (int)Bits<T>::to_u32(a0.w));
    } else {
        float d2[8];
        const uint32_t imask = w0.w >> 24;
        const uint32_t surv = near_node(w0, w2, w3, w4, w.nx, w.ny, w.nz, w.bestn, d2) & allow;
        const uint32_t ih = surv & imask;
        w.tw = w1.y | ((surv & ~imask) << 24);
        w.rank = w1.z;
        if (ih) {
            uint32_t j = 0; float dj = 3.0e38f;
#pragma unroll
            for (int s = 0; s < 8; ++s) if (((ih >> s) & 1u) && d2[s] < dj) { dj = d2[s]; j = (uint32_t)s; }
            if (!((ih >> j) & 1u)) j = (uint32_t)__builtin_ctz(ih);        // (distances beyond 3e38 cannot occur inside the origin rule; kept total)
            const uint32_t rest = ih & ~(1u << j);
            if (rest) stack[w.sp++] = (idx << 8) | rest;                   // ONE entry for this node: its deferred children
            w.G = ((w1.x + j) << 8) | 0xFFu;
        }
    }
    if ((w.tw >> 24) == 0 && w.G == 0) {
        if (w.sp == 0) return false;
        w.G = stack[--w.sp];
    }
    return true;
}

// One trip of the closest-point walk: a closer triangle replaces the winner, and bestn follows it.
template <class T>
__device__ __forceinline__ bool near_step(const SceneLds<T> &sc, NearWalk<T> &w, int base, uint32_t *stack) {
    return near_trip<T>(sc, w, base, stack, [&](uint32_t, const T q[3], T d2, int p) {
        if (d2 < w.best || (d2 == w.best && p > w.prim)) {                 // d2 == best: the later object wins, whatever the order of the visits
            w.best = d2; w.prim = p; w.q[0] = q[0]; w.q[1] = q[1]; w.q[2] = q[2];
            w.bestn = near_bestn<T>(d2, sc.bvh_root[2].w);
        }
    });
}

// One lane per point.  Launches: <T, false, false> spheres alone, <T, false, true> with LDS triangles, <T, true, false> a BVH mesh (SPIRA_CAST_INPLACE).
template <class T, bool BVH, bool TRI>
__global__ __launch_bounds__(kBlock) void k_nearest(const NearestArgs<T> a) {
    extern __shared__ __attribute__((aligned(32))) unsigned char lds_raw[];
    const SceneLds<T> sc = stage_scene<T>(a.scene, lds_raw);     // the only workgroup barrier of the kernel
    const int base = (int)(sc.n_spheres + sc.n_triangles);
    for (uint32_t i = blockIdx.x * kBlock + threadIdx.x; i < a.n_points; i += gridDim.x * kBlock) {
        NearWalk<T> w; T r_max;
        const bool ok = near_load<T>(a, sc, BVH, i, w, r_max);
        if (ok) {
            near_scan_local<T, TRI>(a, sc, w);
            if (BVH) {
                uint32_t stack[kBvhStackD];
                if (near_enter<T>(sc, w)) while (near_step<T>(sc, w, base, stack)) {}
            }
        }
        near_store<T>(a, i, ok, w, r_max);
    }
}

// Scenes with a tree: a refilled session per wave over its range of the caller's list (SPIRA_REFILLED_SESSION of spira_query.h).
template <class T>
__global__ __launch_bounds__(kBlock) void k_nearest_session(const NearestArgs<T> a) {
    extern __shared__ __attribute__((aligned(32))) unsigned char lds_raw[];
    const SceneLds<T> sc = stage_scene<T>(a.scene, lds_raw);     // the only workgroup barrier of the kernel
    uint32_t begin, end;
    session_range(a.base, a.rem, begin, end);
    uint32_t stack[kBvhStackD];
    const int base = (int)(sc.n_spheres + sc.n_triangles);
    uint32_t pt = 0;
    T r_max = 0;
    NearWalk<T> w{};
    const auto start = [&](uint32_t item) -> bool {
            pt = item;
            const bool ok = near_load<T>(a, sc, true, pt, w, r_max);
            bool walks = false;
            if (ok) {
                near_scan_local<T, false>(a, sc, w);
                walks = near_enter<T>(sc, w);
            }
            if (!walks) near_store<T>(a, pt, ok, w, r_max);
            return walks;
    };
    const auto step = [&]() -> bool {
            if (near_step<T>(sc, w, base, stack)) return true;
            near_store<T>(a, pt, true, w, r_max);
            return false;
    };
    SPIRA_REFILLED_SESSION(begin, end, a.refill_free, start, step);
}

}  // namespace spira
#endif
