// spira_sweep.h — sphere sweeps on a scene handle (spira_scene_sweep_* / spira_scene_sweep_blocked_*): a ball of radius r moves from o along d; when and
// where does it first touch the scene's surface?  Included by spira_hip.hip behind spira_nearest.h (the two closest-point functions, near_dot, near_d2) and
// spira_query.h (cast_ray_prepare, CastLimits, the refilled session's loop); the tree is the one create, update and rebuild maintain, walked a third way:
// slab tests against boxes grown by the radius.  The first part of this file needs no HIP header: a CPU program (tests/native/sweep_plan.cpp) and the
// exported host arithmetic (spira_sweep_sphere_triangle_*) call the very functions the kernels call.  This comment is the contract; the numpy twins
// (spira_hip.query: sweep_sphere_triangle, sweep_sphere_sphere, prepare_sweeps) restate it operation for operation.
//
// A sweep is a ray of the ray queries, eight values of the call's precision T [ox oy oz t_min dx dy dz t_max] prepared by cast_ray_prepare (the library
// normalises d), and a radius r.  t is the distance of the ball's CENTRE along the unit direction: c(t) = o + d t, evaluated per coordinate as o_k + d_k t.
// All arithmetic in T, in the written order, nothing fused (-ffp-contract=off); dot(a, b) is ALWAYS (a.x b.x + a.y b.y) + a.z b.z; divisions and square
// roots are IEEE.  With  r2 = r r,  rs = r + r 2^-10,  rs2 = rs rs.
//
// The objects are the spheres [0..) then the triangles [0..) in the caller's order; the surface is the object (a sphere is a shell, as for closest_point).
// Object k yields at most one t_k:
//   1. Start overlap.  (q0, d2_0) = the object's closest-point function (spira_nearest.h; a sphere's radius from spheres5) at c(t_min).  d2_0 <= r2:
//      t_k = t_min, q_k = q0.  That is the candidate rule of nearest_k / count_within: a sweep with t_min = 0 starts blocked exactly where
//      count_within(o, r) > 0.
//   2. Otherwise, proposals: closed-form roots of "distance = r", solved about the foot of the object's anchor on the ray, so that the quadratics' terms
//      are of the object's size and not of the origin's distance.  Anchor a = v0 (sphere: its centre C):  t_b = dot(d, a - o),  b = o + d t_b,
//      w = b - a;  a root tau is relative to b, its proposal is t = t_b + tau.
//      Triangle (v0, e1, e2), seven proposals in this order:
//        face      n = cross(e1, e2) = (e1.y e2.z - e1.z e2.y, e1.z e2.x - e1.x e2.z, e1.x e2.y - e1.y e2.x),  nl = sqrt(dot(n, n))  (the one sqrt),
//                  s0 = dot(n, c(t_min) - v0),  nd = dot(n, d),  nw = dot(n, w),  off = r nl,  taken as -off when s0 < 0: the plane offset by r toward
//                  the side of c(t_min);  tau = (off - nw) / nd.  Skipped (NaN) when nd is 0 or NaN, and kept only when the contact lies inside the
//                  triangle, as an edge's root is kept only within the edge: g = w + d tau (the contact relative to v0, up to its offset along n),
//                  p1 = dot(e1, g), p2 = dot(e2, g), a11 = dot(e1, e1), a12 = dot(e1, e2), a22 = dot(e2, e2);  bv = a22 p1 - a12 p2,
//                  bw = a11 p2 - a12 p1, det = a11 a22 - a12 a12;  kept when bv >= 0 && bw >= 0 && bv + bw <= det (barycentric numerators, no division).
//                  Why, when verification decides anyway: verification accepts up to rs, so a face root whose contact lies just OUTSIDE the triangle
//                  — the edge beyond is then within rs of c(t) although not within r — would be taken a distance of up to r 2^-10 before the true
//                  contact with that edge.  With the test every kept proposal is a true contact of a feature, none can precede the first contact, and
//                  the smallest verified one IS the first contact up to rounding.  A contact the test wrongly drops by a rounding at an edge is
//                  that edge's cylinder root a moment later (delta^2 / 2 r for a contact delta inside the edge).
//        edges     (v0, e1), (v0, e2), (v0 + e1, e2 - e1): with the edge (A, e) and m = w - (A - v0) (m = w, w, w - e1):
//                  ee = dot(e, e), de = dot(d, e), me = dot(m, e), md = dot(m, d), mm = dot(m, m);
//                  qa = ee - de de,  qb = ee md - de me,  qc = ee (mm - r2) - me me;  tau = (-qb - sqrt(qb qb - qa qc)) / qa  (the near root of the
//                  infinite cylinder);  the foot parameter f = (me + de tau) / ee;  kept only when 0 <= f <= 1 (else NaN).
//        vertices  v0, v0 + e1, v0 + e2: m = w, w - e1, w - e2;  md = dot(m, d), mm = dot(m, m);  tau = -md - sqrt(md md - (mm - r2))  (the near root
//                  of the sphere of radius r about the vertex).
//      Sphere (C, R), two proposals:  m = w,  md = dot(m, d),  mm = dot(m, m);  Rp = R + r:  tau = -md - sqrt(md md - (mm - Rp Rp))  (the near root);
//      and, only when R > r (else NaN),  Rm = R - r:  tau = -md + sqrt(md md - (mm - Rm Rm))  (the far root: a ball inside the shell reaches it from within).
//      A proposal that is NaN or < t_min is dropped.
//   3. Verification decides.  For a proposal t the closest-point function is evaluated at c(t); it is VERIFIED when d2 <= rs2.  t_k is the smallest
//      verified proposal — the first verified one in ascending order — and q_k, d2_k are that evaluation's.  None verified: no t_k.  Every proposal is a true
//      contact of its feature, so two evaluations (the start, one proposal) are the expected cost; the slack of rs over r is for the roots' own rounding.
//      The functions below take a bound and skip proposals beyond it (and, once one is verified, proposals not below it): the bits of t_k do not depend on
//      the bound, because every proposal and every verdict is computed from the object and the sweep alone — the bound only removes proposals from a set
//      whose minimum is asked for; when the unbounded t_k is within the bound it is still the minimum of what is left, and when it is not, nothing at or
//      below the bound is verified and the object is no candidate either way.  (Equal proposals evaluate the same point: the same q and d2.)
//   4. Candidate and order.  Object k is a candidate when !(t_k < t_min || t_k > closest), closest starting at t_max; the scan keeps the minimal t and ties
//      go to the LATER object (start overlaps all tie at t_min).  A NaN anywhere verifies nothing: such an object is never a candidate.
//   5. Outputs of the winner: out_t = t_k, out_point = q_k, out_normal = (c(t_k) - q_k) / l with l = sqrt(d2_k), d2_k = dot(c(t_k) - q_k, c(t_k) - q_k),
//      or -d when l is below the smallest normal number of T.  A miss: prim SPIRA_RAY_MISS, t = t_max copied, point 0, normal 0.
//   6. blocked is 1 exactly where the sweep gives prim >= 0; its kernels stop at the first candidate.
//
// Validity (sweep_prepare): the ray is valid by cast's rule (cast_ray_prepare, the origin rule included); r is not NaN, finite and >= 0; and — scenes with
// a tree only — rs scale <= kSweepRadiusBound = 64 in T.  Invalid: prim SPIRA_RAY_INVALID, t 0, point 0, normal 0, blocked 255.
//
// Why verification and not the roots alone.  In Float32 a near-grazing root can be off by more than the builder's box pad, and a tree that prunes
// geometrically would then disagree with the scan.  An accepted t_k PROVES that c(t_k) — a point ON the path at a parameter <= closest, as the scan computes
// it — lies within rs (1 + 3 u) of the point q_k, and q_k lies within a few ulps of the object ((d) of spira_nearest.h).  So the path is inside the child's
// box grown by rs no later than t_k: what the walk tests.
//
// The walk.  The root box (caller's coordinates, T) is grown by rs, rounded outward ((|plane| + rs) 2^-20 further out), and the ray's Float32 side starts
// where the path enters THAT box (sweep8_enter, bvh8_enter's arithmetic).  sweep8_node is bvh8_node with every near plane moved out and every far plane moved
// out by rn = fl32(rs scale) (1 + 2^-20) + 2^-100 (rounded UP): per axis the base (grid - origin) of bvh8_node becomes two, ((grid - origin) -+ rn) 1/d for the
// near planes and ((grid - origin) +- rn) 1/d for the far ones (upper signs: d_k >= 0), so the loop over the children costs what bvh8_node's does.  The
// radius is added BEFORE the product with the clamped reciprocal: a ray parallel to a slab and inside its grown extent sees (-huge, +huge) as in bvh8_node,
// one outside it an empty interval.  A grown empty child (lo 255, hi 0) could pass the slab test, so children are masked by lo <= hi, as near_node does.
// sweep8_step is the one trip of the project's walks (spira_device.h, "one TRIP") on its pieces: the leaf arm is the leaf test above, in T, on the record's
// own values — the tree only prunes — the node arm sweep8_node.  best is tightened on every win; the tie rule is t < closest || p > prim.
//
// Why 64 holds for the radius too.  Normalised units, A = amax_n, R = rs scale <= 64, u = 2^-24; a child is wrongly skipped only if the Float32 slab
// test misses the path although c(t_k) lies inside the child's TRUE box grown by R.  Every triangle lies inside its child box shrunk by the builder's pad,
// 1e-4 max(1, A) (spira_bvh.h; the refit pad is never smaller), and rn exceeds R by 2^-20 R = 6.1e-5 at R = 64.  Against that:
//   (a) the entry point o + d te in T, less the centre, times scale, rounded to Float32: |o_n| <= 64 + A, te is a distance to a box 1 + 2 R wide:
//       three roundings at magnitudes <= A + 64 + R                                                             <= 3 u (A + 128)  = 2.3e-5 + 1.8e-7 A
//   (b) the two bases: fl(grid - origin) at a magnitude <= 1 + R (the origin lies inside the grown root box), -+ rn at <= 1 + 2 R   <= 3 u (1 + R) = 1.2e-5
//   (c) the slab parameters: 1/d is v_rcp_f32 (one ulp = 2 u), the product and the fma round once each: 4 u of a parameter that is at most the diagonal
//       of the grown root box, sqrt(3) (1 + 2 R) = 224; a parameter error dt moves a plane by dt |d_k| <= dt                         <= 4 u 224     = 5.4e-5
//       (bvh8_node's own term; there the box is one unit wide and the term 4e-7.  This is what r_n <= 64 adds.)
//   (d) the scan's side: c(t_k) = o + d t_k in T with t_k <= 111 + R + 2: u (2 t_k + A + 1 + R) = 2.5e-5 + 6e-8 A; sqrt(d2) <= rs (1 + 3 u): 1.2e-5;
//       q: 4 u (A + 1)                                                                                                               <= 3.8e-5 + 3e-7 A
// Total 1.27e-4 + 5e-7 A against 1e-4 max(1, A) + 6.1e-5 = 1.61e-4: a margin of 1.27 at A <= 1, R = 64, origin at 64 units and the longest path all at
// once — closed, thinner than the point walk's 2.7; at R <= 16 the same sum is 5.2e-5 against 1.15e-4, a margin of 2.2, and for a mesh far from the
// origin the pad's A outgrows every term.  In Float64 (a) shrinks to the conversion's u (A + 1 + R) = 3.9e-6 and (d) vanishes: 7.0e-5 against 1.61e-4.
// best is the distance from the entry point to c(closest) in normalised units, clamped at 0 (a contact at the entry point itself may come out a rounding
// before it) and rounded up, as bvh8_best; the comparisons are not strict, so children at exactly the winning parameter are visited and among equal t
// the later triangle is still reached.  Valid sweeps at 60 .. 64 units with radii just under the bound are held to the scan by tests/test_gpu_sweep.py.
//
// Kernels (each stages the scene with stage_scene: one barrier):
//   k_sweep<T, BVH, TRI, ANY>     one lane per sweep, grid-stride: the LDS scan over spheres and LDS triangles; BVH: then the walk to the end (SPIRA_CAST_INPLACE).
//   k_sweep_session<T, ANY>       scenes with a tree, the default: SPIRA_REFILLED_SESSION of spira_query.h; start = sweep_load, sweep_scan_local, sweep8_enter;
//                                 step = sweep8_step.
//   ANY = true                    blocked: only `hit` is written; a lane whose LDS scan found a candidate never walks, a walking lane leaves after the first
//                                 trip that set prim >= 0.
// The lane keeps q (three T) and computes c(t_k), d2 and the normal again at the store — the same operations on the same values, the same bits.
#pragma once
#include <cstdint>

#include "spira_nearest.h"      // closest_point_triangle, closest_point_sphere, near_dot, near_sqrt, near_d2; spira_query.h: cast_ray_prepare, CastLimits

namespace spira {

constexpr int kSweepRadiusBound = 64;      // rs * scale <= 64 in scenes with a tree, see above

template <class T> SPIRA_HD inline T sweep_nan() { return (T)__builtin_nanf(""); }

template <class T> struct SweepRadii { T r2, rs, rs2; };
template <class T> SPIRA_HD inline SweepRadii<T> sweep_radii(T r) {
    SweepRadii<T> k;
    k.r2 = r * r; k.rs = r + r * (T)0.0009765625; k.rs2 = k.rs * k.rs;
    return k;
}

// One sweep: ray[0..8) as cast's, radius r -> valid?  d: the unit direction (written for rays valid by cast's rule).  frame: the scene has a tree.
template <class T> SPIRA_HD inline bool sweep_prepare(const T *ray, T r, bool frame, const T *fr, T d[3]) {
    if (!cast_ray_prepare<T>(ray, frame, fr, d)) return false;
    if (r != r || !((r - r) == (T)0) || r < (T)0) return false;
    if (frame) {
        const T rs = r + r * (T)0.0009765625;
        if (!(rs * fr[3] <= (T)kSweepRadiusBound)) return false;
    }
    return true;
}

// The anchor's foot: t_b = dot(d, a - o), w = (o + d t_b) - a.
template <class T> SPIRA_HD inline void sweep_foot(const T a[3], const T o[3], const T d[3], T &t_b, T w[3]) {
    const T ao[3] = {a[0] - o[0], a[1] - o[1], a[2] - o[2]};
    t_b = near_dot<T>(d, ao);
    for (int k = 0; k < 3; ++k) w[k] = (o[k] + d[k] * t_b) - a[k];
}
// near root (sign -1) or far root (sign +1) of the sphere of squared radius rr about the point the path passes at m + d tau
template <class T> SPIRA_HD inline T sweep_root_point(const T m[3], const T d[3], T rr, bool far_root) {
    const T md = near_dot<T>(m, d), mm = near_dot<T>(m, m);
    const T s = near_sqrt<T>(md * md - (mm - rr));
    return far_root ? -md + s : -md - s;
}
// near root of the infinite cylinder of squared radius r2 about the line m0 + e f, kept when the foot parameter is within the edge
template <class T> SPIRA_HD inline T sweep_root_edge(const T m[3], const T e[3], const T d[3], T r2) {
    const T ee = near_dot<T>(e, e), de = near_dot<T>(d, e), me = near_dot<T>(m, e), md = near_dot<T>(m, d), mm = near_dot<T>(m, m);
    const T qa = ee - de * de, qb = ee * md - de * me, qc = ee * (mm - r2) - me * me;
    const T tau = (-qb - near_sqrt<T>(qb * qb - qa * qc)) / qa;
    const T f = (me + de * tau) / ee;
    return (f >= (T)0 && f <= (T)1) ? tau : sweep_nan<T>();
}

// The seven proposals of a triangle (header comment, 2): face, edges (v0, e1), (v0, e2), (v0 + e1, e2 - e1), vertices v0, v0 + e1, v0 + e2.  p0 = c(t_min).
template <class T> SPIRA_HD inline void sweep_triangle_proposals(const T v0[3], const T e1[3], const T e2[3], const T o[3], const T d[3], T r, T r2, const T p0[3], T tp[7]) {
    T t_b, w[3];
    sweep_foot<T>(v0, o, d, t_b, w);
    const T n[3] = {e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0]};
    const T nl = near_sqrt<T>(near_dot<T>(n, n));
    const T ap0[3] = {p0[0] - v0[0], p0[1] - v0[1], p0[2] - v0[2]};
    const T s0 = near_dot<T>(n, ap0), nd = near_dot<T>(n, d), nw = near_dot<T>(n, w);
    T off = r * nl;
    if (s0 < (T)0) off = -off;
    const T tau = (off - nw) / nd;
    const T g[3] = {w[0] + d[0] * tau, w[1] + d[1] * tau, w[2] + d[2] * tau};
    const T p1 = near_dot<T>(e1, g), p2 = near_dot<T>(e2, g), a11 = near_dot<T>(e1, e1), a12 = near_dot<T>(e1, e2), a22 = near_dot<T>(e2, e2);
    const T bv = a22 * p1 - a12 * p2, bw = a11 * p2 - a12 * p1, det = a11 * a22 - a12 * a12;
    tp[0] = (nd == nd && nd != (T)0 && bv >= (T)0 && bw >= (T)0 && bv + bw <= det) ? t_b + tau : sweep_nan<T>();
    const T w1[3] = {w[0] - e1[0], w[1] - e1[1], w[2] - e1[2]}, w2[3] = {w[0] - e2[0], w[1] - e2[1], w[2] - e2[2]};
    const T e3[3] = {e2[0] - e1[0], e2[1] - e1[1], e2[2] - e1[2]};
    tp[1] = t_b + sweep_root_edge<T>(w, e1, d, r2);
    tp[2] = t_b + sweep_root_edge<T>(w, e2, d, r2);
    tp[3] = t_b + sweep_root_edge<T>(w1, e3, d, r2);
    tp[4] = t_b + sweep_root_point<T>(w, d, r2, false);
    tp[5] = t_b + sweep_root_point<T>(w1, d, r2, false);
    tp[6] = t_b + sweep_root_point<T>(w2, d, r2, false);
}

// A proposal is worth an evaluation: not NaN, not before t_min, within the bound, and below what is already verified.
template <class T> SPIRA_HD inline bool sweep_try(T t, T t_min, T bound, bool found, T tk) {
    if (!(t >= t_min)) return false;
    return found ? t < tk : !(t > bound);
}

// The first contact of the ball with the triangle (v0, v0 + e1, v0 + e2) within `bound`.  true: a candidate — t, q = the contact point on the triangle.
template <class T> SPIRA_HD inline bool sweep_sphere_triangle(const T v0[3], const T e1[3], const T e2[3], const T o[3], const T d[3], T r, T t_min, T bound, T &t_out, T q_out[3]) {
    const SweepRadii<T> k = sweep_radii<T>(r);
    T p[3] = {o[0] + d[0] * t_min, o[1] + d[1] * t_min, o[2] + d[2] * t_min};
    T q[3], d2, tk = t_min;
    closest_point_triangle<T>(v0, e1, e2, p, q, d2);
    bool found = d2 <= k.r2;
    if (found) { q_out[0] = q[0]; q_out[1] = q[1]; q_out[2] = q[2]; }
    else {
        T tp[7];
        sweep_triangle_proposals<T>(v0, e1, e2, o, d, r, k.r2, p, tp);
        for (int j = 0; j < 7; ++j) {
            const T t = tp[j];
            if (!sweep_try<T>(t, t_min, bound, found, tk)) continue;
            for (int c = 0; c < 3; ++c) p[c] = o[c] + d[c] * t;
            closest_point_triangle<T>(v0, e1, e2, p, q, d2);
            if (d2 <= k.rs2) { found = true; tk = t; q_out[0] = q[0]; q_out[1] = q[1]; q_out[2] = q[2]; }
        }
    }
    t_out = tk;
    return found && !(tk < t_min || tk > bound);
}

// The first contact of the ball with the shell of the sphere (centre c, radius R) within `bound`.
template <class T> SPIRA_HD inline bool sweep_sphere_sphere(const T c[3], T R, const T o[3], const T d[3], T r, T t_min, T bound, T &t_out, T q_out[3]) {
    const SweepRadii<T> k = sweep_radii<T>(r);
    T p[3] = {o[0] + d[0] * t_min, o[1] + d[1] * t_min, o[2] + d[2] * t_min};
    T q[3], d2, tk = t_min;
    closest_point_sphere<T>(c, R, p, q, d2);
    bool found = d2 <= k.r2;
    if (found) { q_out[0] = q[0]; q_out[1] = q[1]; q_out[2] = q[2]; }
    else {
        T t_b, w[3];
        sweep_foot<T>(c, o, d, t_b, w);
        const T Rp = R + r, Rm = R - r;
        const T tp[2] = {t_b + sweep_root_point<T>(w, d, Rp * Rp, false), R > r ? t_b + sweep_root_point<T>(w, d, Rm * Rm, true) : sweep_nan<T>()};
        for (int j = 0; j < 2; ++j) {
            const T t = tp[j];
            if (!sweep_try<T>(t, t_min, bound, found, tk)) continue;
            for (int a = 0; a < 3; ++a) p[a] = o[a] + d[a] * t;
            closest_point_sphere<T>(c, R, p, q, d2);
            if (d2 <= k.rs2) { found = true; tk = t; q_out[0] = q[0]; q_out[1] = q[1]; q_out[2] = q[2]; }
        }
    }
    t_out = tk;
    return found && !(tk < t_min || tk > bound);
}

// The winner's normal: (c(t) - q) / l, l = sqrt(dot(c(t) - q, c(t) - q)), or -d when l is below the smallest normal number.
template <class T> SPIRA_HD inline void sweep_normal(const T o[3], const T d[3], T t, const T q[3], T nrm[3]) {
    const T rv[3] = {(o[0] + d[0] * t) - q[0], (o[1] + d[1] * t) - q[1], (o[2] + d[2] * t) - q[2]};
    const T l = near_sqrt<T>(near_dot<T>(rv, rv));
    if (l >= CastLimits<T>::min_normal) { nrm[0] = rv[0] / l; nrm[1] = rv[1] / l; nrm[2] = rv[2] / l; }
    else { nrm[0] = -d[0]; nrm[1] = -d[1]; nrm[2] = -d[2]; }
}

}  // namespace spira

#if defined(__HIPCC__)
// Refill threshold and waves per CU of the session kernel: the loop k_cast_session runs, with its knobs (SPIRA_CAST_REFILL, SPIRA_CAST_WAVES_PER_CU; CastKnobs,
// read per call as cast reads them); docs/experiments.md, "sphere sweeps", says what has and has not been measured.
namespace spira {

template <class T> struct SweepArgs {
    SceneGlobal<T> scene;
    const T *rays;                   // n x 8
    const T *radii;                  // n
    uint32_t n;
    int *prim; T *t; T *point; T *normal;      // n, n, n x 3, n x 3 (interleaved); any may be NULL
    uint8_t *hit;                    // blocked (ANY): n
    uint32_t *trips;                 // diagnostic, may be NULL
    uint32_t base, rem;              // session: wave w owns base + (w < rem) sweeps from w base + min(w, rem)  (CastPlan)
    uint32_t refill_free;
};

// the ray's Float32 side: bvh8_node's, and the radius in normalised units
struct Sweep8Ray {
    float ox, oy, oz;        // where the path enters the grown root box (or its own origin inside it), normalised frame
    float ix, iy, iz;        // 1 / d, clamped as bvh8_rcp
    uint32_t oct;            // bit k: d_k < 0
    float best;              // c(closest) as a distance from (ox, oy, oz), normalised units, >= 0, rounded up
    float rn;                // rs * scale, rounded up
};

// One lane's sweep: the ray, the scan's state and the walk's.
template <class T> struct SweepWalk {
    T o[3], d[3], q[3];
    T t_min, t_max, r;
    T closest;
    int prim;
    T t0;                    // ray parameter of (ox, oy, oz)
    uint32_t G;              // as Bvh8Walk: child_base << 8 | hit children still to visit, bit (slot ^ oct)
    uint32_t tw, rank;
    uint32_t sp;
    uint32_t trips;
};

__device__ __forceinline__ float sweep8_best(float x) { return __builtin_fmaxf(x, 0.0f) * 1.00000095367431640625f; }      // clamped at 0, then (1 + 2^-20)

template <class T, bool ANY>
__device__ __forceinline__ void sweep_store(const SweepArgs<T> &a, uint32_t i, bool valid, const SweepWalk<T> &w) {
    const bool hit = valid && w.prim >= 0;
    if (ANY) { a.hit[i] = valid ? (hit ? (uint8_t)1 : (uint8_t)0) : (uint8_t)255; if (a.trips) a.trips[i] = w.trips; return; }
    if (a.prim) a.prim[i] = valid ? w.prim : SPIRA_RAY_INVALID;
    if (a.t) a.t[i] = !valid ? (T)0 : (hit ? w.closest : w.t_max);
    if (a.point) { a.point[3 * (size_t)i] = hit ? w.q[0] : (T)0; a.point[3 * (size_t)i + 1] = hit ? w.q[1] : (T)0; a.point[3 * (size_t)i + 2] = hit ? w.q[2] : (T)0; }
    if (a.normal) {
        T nrm[3] = {(T)0, (T)0, (T)0};
        if (hit) sweep_normal<T>(w.o, w.d, w.closest, w.q, nrm);
        a.normal[3 * (size_t)i] = nrm[0]; a.normal[3 * (size_t)i + 1] = nrm[1]; a.normal[3 * (size_t)i + 2] = nrm[2];
    }
    if (a.trips) a.trips[i] = w.trips;
}

// Loads sweep i, classifies it and starts the scan's state.  Returns the validity.
template <class T>
__device__ __forceinline__ bool sweep_load(const SweepArgs<T> &a, const SceneLds<T> &sc, bool frame, uint32_t i, SweepWalk<T> &w) {
    const T *rp = a.rays + 8 * (size_t)i;
    T ray[8], dd[3] = {(T)0, (T)0, (T)0}, fr[4] = {(T)0, (T)0, (T)0, (T)1};
#pragma unroll
    for (int k = 0; k < 8; ++k) ray[k] = rp[k];
    const T r = a.radii[i];
    if (frame) { const Pack4<T> f = sc.bvh_root[2]; fr[0] = f.x; fr[1] = f.y; fr[2] = f.z; fr[3] = f.w; }
    const bool ok = sweep_prepare<T>(ray, r, frame, fr, dd);
#pragma unroll
    for (int k = 0; k < 3; ++k) { w.o[k] = ray[k]; w.d[k] = dd[k]; w.q[k] = (T)0; }
    w.t_min = ray[3]; w.t_max = ray[7]; w.r = r;
    w.closest = ray[7]; w.prim = -1; w.trips = 0;
    w.t0 = (T)0; w.G = 0; w.tw = 0; w.rank = 0; w.sp = 0;
    return ok;
}

template <class T> __device__ __forceinline__ void sweep_take(SweepWalk<T> &w, T t, const T q[3], int p) {
    w.closest = t; w.prim = p; w.q[0] = q[0]; w.q[1] = q[1]; w.q[2] = q[2];
}

// The LDS part of the scan, in scan order (a candidate has t <= closest: ties go to the later object): spheres (radius from spheres5), then the LDS triangles.
template <class T, bool TRI, bool ANY>
__device__ __forceinline__ void sweep_scan_local(const SweepArgs<T> &a, const SceneLds<T> &sc, SweepWalk<T> &w) {
    for (uint32_t s = 0; s < sc.n_spheres; ++s) {
        const Pack4<T> sp = sc.sph[s];
        const T c[3] = {sp.x, sp.y, sp.z};
        T t, q[3];
        if (sweep_sphere_sphere<T>(c, a.scene.spheres5[5 * (size_t)s + 3], w.o, w.d, w.r, w.t_min, w.closest, t, q)) {
            sweep_take<T>(w, t, q, (int)s);
            if (ANY) return;
        }
    }
    if (TRI)
        for (uint32_t i = 0; i < sc.n_triangles; ++i) {
            const Pack4<T> a0 = sc.tri[3 * i], a1 = sc.tri[3 * i + 1], a2 = sc.tri[3 * i + 2];
            const T v0[3] = {a0.x, a0.y, a0.z}, e1[3] = {a1.x, a1.y, a1.z}, e2[3] = {a2.x, a2.y, a2.z};
            T t, q[3];
            if (sweep_sphere_triangle<T>(v0, e1, e2, w.o, w.d, w.r, w.t_min, w.closest, t, q)) {
                sweep_take<T>(w, t, q, (int)(sc.n_spheres + i));
                if (ANY) return;
            }
        }
}

// The root box grown by rs (rounded outward) in T, then the ray's Float32 side.  false: no triangle of the mesh can be touched before `closest`.
template <class T>
__device__ __forceinline__ bool sweep8_enter(const SceneLds<T> &sc, SweepWalk<T> &w, Sweep8Ray &r) {
    const T rs = w.r + w.r * (T)0.0009765625, out = (T)9.5367431640625e-7;      // 2^-20
    Pack4<T> mn = sc.bvh_root[0], mx = sc.bvh_root[1];
    const Pack4<T> fr = sc.bvh_root[2];
    mn.x = (mn.x - rs) - (abs_t(mn.x) + rs) * out; mn.y = (mn.y - rs) - (abs_t(mn.y) + rs) * out; mn.z = (mn.z - rs) - (abs_t(mn.z) + rs) * out;
    mx.x = (mx.x + rs) + (abs_t(mx.x) + rs) * out; mx.y = (mx.y + rs) + (abs_t(mx.y) + rs) * out; mx.z = (mx.z + rs) + (abs_t(mx.z) + rs) * out;
    const Vec<T> o = mk<T>(w.o[0], w.o[1], w.o[2]), d = mk<T>(w.d[0], w.d[1], w.d[2]);
    const Vec<T> inv = mk<T>(rcp_fast(d.x), rcp_fast(d.y), rcp_fast(d.z));
    const T te = box_entry<T>(mn, mx, o, inv, w.closest);
    if (te < (T)0) return false;
    w.t0 = te;
    const Vec<T> on = ((o + d * te) - mk<T>(fr.x, fr.y, fr.z)) * fr.w;
    r.ox = (float)on.x; r.oy = (float)on.y; r.oz = (float)on.z;
    const float dx = (float)d.x, dy = (float)d.y, dz = (float)d.z;
    const bool nx = dx < 0.0f, ny = dy < 0.0f, nz = dz < 0.0f;
    r.oct = (nx ? 1u : 0u) | (ny ? 2u : 0u) | (nz ? 4u : 0u);
    r.ix = bvh8_rcp(dx, nx); r.iy = bvh8_rcp(dy, ny); r.iz = bvh8_rcp(dz, nz);
    r.best = sweep8_best((float)((w.closest - te) * fr.w));
    r.rn = (float)(rs * fr.w) * 1.00000095367431640625f + 7.888609052210118e-31f;      // (1 + 2^-20), 2^-100: rounded up for sure
    w.G = 1u << r.oct; w.tw = 0; w.rank = 0; w.sp = 0;                                  // the root: a group holding only slot 0 (bvh8_begin)
    return true;
}

// One node: slab tests of its 8 children against their boxes grown by rn, two at a time.  Out: ih = hit child NODES, bit (slot ^ oct); lh = hit leaf slots.
__device__ __forceinline__ void sweep8_node(const uint4 w0, const uint4 w2, const uint4 w3, const uint4 w4, const Sweep8Ray &r, uint32_t &ih, uint32_t &lh) {
    const float sx = __uint_as_float((w0.w & 0xFFu) << 23), sy = __uint_as_float(((w0.w >> 8) & 0xFFu) << 23), sz = __uint_as_float(((w0.w >> 16) & 0xFFu) << 23);
    const uint32_t imask = w0.w >> 24;
    const bool nx = (r.oct & 1u) != 0, ny = (r.oct & 2u) != 0, nz = (r.oct & 4u) != 0;
    const float ax = sx * r.ix, ay = sy * r.iy, az = sz * r.iz;
    const float gx = __uint_as_float(w0.x) - r.ox, gy = __uint_as_float(w0.y) - r.oy, gz = __uint_as_float(w0.z) - r.oz;
    const float rx = nx ? -r.rn : r.rn, ry = ny ? -r.rn : r.rn, rz = nz ? -r.rn : r.rn;      // toward the near side of each axis
    const float bnx = (gx - rx) * r.ix, bny = (gy - ry) * r.iy, bnz = (gz - rz) * r.iz;     // near planes moved out
    const float bfx = (gx + rx) * r.ix, bfy = (gy + ry) * r.iy, bfz = (gz + rz) * r.iz;     // far planes moved out
    const F2 ax2 = {ax, ax}, ay2 = {ay, ay}, az2 = {az, az};
    const F2 bnx2 = {bnx, bnx}, bny2 = {bny, bny}, bnz2 = {bnz, bnz}, bfx2 = {bfx, bfx}, bfy2 = {bfy, bfy}, bfz2 = {bfz, bfz};
    // near / far planes per axis by the sign of the direction, as bvh8_node
    const uint32_t nxw[2] = {nx ? w3.z : w2.x, nx ? w3.w : w2.y}, fxw[2] = {nx ? w2.x : w3.z, nx ? w2.y : w3.w};
    const uint32_t nyw[2] = {ny ? w4.x : w2.z, ny ? w4.y : w2.w}, fyw[2] = {ny ? w2.z : w4.x, ny ? w2.w : w4.y};
    const uint32_t nzw[2] = {nz ? w4.z : w3.x, nz ? w4.w : w3.y}, fzw[2] = {nz ? w3.x : w4.z, nz ? w3.y : w4.w};
    uint32_t hlo = 0, hhi = 0;
#pragma unroll
    for (int k = 3; k >= 0; --k) {
        const F2 qnx = bvh8_bytes(nxw[0], nxw[1], k), qfx = bvh8_bytes(fxw[0], fxw[1], k);
        const F2 tnx = __builtin_elementwise_fma(qnx, ax2, bnx2), tfx = __builtin_elementwise_fma(qfx, ax2, bfx2);
        const F2 tny = __builtin_elementwise_fma(bvh8_bytes(nyw[0], nyw[1], k), ay2, bny2), tfy = __builtin_elementwise_fma(bvh8_bytes(fyw[0], fyw[1], k), ay2, bfy2);
        const F2 tnz = __builtin_elementwise_fma(bvh8_bytes(nzw[0], nzw[1], k), az2, bnz2), tfz = __builtin_elementwise_fma(bvh8_bytes(fzw[0], fzw[1], k), az2, bfz2);
        const float tn0 = __builtin_fmaxf(__builtin_fmaxf(tnx.x, tny.x), __builtin_fmaxf(tnz.x, 0.0f)), tf0 = __builtin_fminf(__builtin_fminf(tfx.x, tfy.x), __builtin_fminf(tfz.x, r.best));
        const float tn1 = __builtin_fmaxf(__builtin_fmaxf(tnx.y, tny.y), __builtin_fmaxf(tnz.y, 0.0f)), tf1 = __builtin_fminf(__builtin_fminf(tfx.y, tfy.y), __builtin_fminf(tfz.y, r.best));
        // present: lo_x <= hi_x (an empty child has lo 255, hi 0 — grown by rn it could pass the slab test)
        const bool p0 = nx ? qfx.x <= qnx.x : qnx.x <= qfx.x, p1 = nx ? qfx.y <= qnx.y : qnx.y <= qfx.y;
        hlo = hlo + hlo + ((p0 && tn0 <= tf0) ? 1u : 0u);
        hhi = hhi + hhi + ((p1 && tn1 <= tf1) ? 1u : 0u);
    }
    const uint32_t hits = hlo | (hhi << 4);
    uint32_t ihs = hits & imask;
    lh = hits & ~imask;
    if (nx) ihs = ((ihs & 0x55u) << 1) | ((ihs >> 1) & 0x55u);       // bit s -> bit s ^ oct
    if (ny) ihs = ((ihs & 0x33u) << 2) | ((ihs >> 2) & 0x33u);
    if (nz) ihs = ((ihs & 0x0Fu) << 4) | (ihs >> 4);
    ih = ihs;
}

// One trip of the sweep = ONE memory round trip (header comment, "The walk"), on the pieces of spira_device.h ("one TRIP": what they do and why the
// loads are what they are) with the sweep's own arms; the stack is private.  Returns false when the walk is over.
template <class T>
__device__ __forceinline__ bool sweep8_step(const SceneLds<T> &sc, SweepWalk<T> &w, Sweep8Ray &r, int base, uint32_t *stack) {
    const bool is_tri = (w.tw >> 24) != 0;
    const uint4 *ptr;
    if (is_tri) ptr = reinterpret_cast<const uint4 *>(sc.bvh_tris + 3 * (size_t)walk_take_tri(w));
    else ptr = sc.bvh_nodes + 5 * (size_t)walk_take_group(w, r.oct, stack);
    ++w.trips;
    uint4 w0, w1, w2, w3, w4, w5;
    walk_load_one<kTriWords<T>, false>(ptr, w0, w1, w2, w3, w4, w5);
    if (is_tri) {
        Pack4<T> a0, a1, a2;
        bvh8_tri_words(w0, w1, w2, w3, w4, w5, a0, a1, a2);
        const T v0[3] = {a0.x, a0.y, a0.z}, e1[3] = {a1.x, a1.y, a1.z}, e2[3] = {a2.x, a2.y, a2.z};
        T t, q[3];
        if (sweep_sphere_triangle<T>(v0, e1, e2, w.o, w.d, w.r, w.t_min, w.closest, t, q)) {
            const int p = base + (int)Bits<T>::to_u32(a0.w);
            if (t < w.closest || p > w.prim) {                             // t == closest: the later object wins, whatever the order of the visits
                sweep_take<T>(w, t, q, p);
                r.best = sweep8_best((float)((t - w.t0) * sc.bvh_root[2].w));
            }
        }
    } else {
        uint32_t ih, lh;
        sweep8_node(w0, w2, w3, w4, r, ih, lh);
        walk_set_node(w, w1, ih, lh);
    }
    return walk_pop(w, stack);
}

// One lane per sweep.  Launches: <T, false, false, .> spheres alone, <T, false, true, .> with LDS triangles, <T, true, false, .> a BVH mesh (SPIRA_CAST_INPLACE).
template <class T, bool BVH, bool TRI, bool ANY>
__global__ __launch_bounds__(kBlock) void k_sweep(const SweepArgs<T> a) {
    extern __shared__ __attribute__((aligned(32))) unsigned char lds_raw[];
    const SceneLds<T> sc = stage_scene<T>(a.scene, lds_raw);     // the only workgroup barrier of the kernel
    const int base = (int)(sc.n_spheres + sc.n_triangles);
    for (uint32_t i = blockIdx.x * kBlock + threadIdx.x; i < a.n; i += gridDim.x * kBlock) {
        SweepWalk<T> w;
        const bool ok = sweep_load<T>(a, sc, BVH, i, w);
        if (ok) {
            sweep_scan_local<T, TRI, ANY>(a, sc, w);
            if (BVH && !(ANY && w.prim >= 0)) {
                uint32_t stack[kBvhStackD];
                Sweep8Ray r;
                if (sweep8_enter<T>(sc, w, r)) while (sweep8_step<T>(sc, w, r, base, stack) && !(ANY && w.prim >= 0)) {}
            }
        }
        sweep_store<T, ANY>(a, i, ok, w);
    }
}

// Scenes with a tree: a refilled session per wave over its range of the caller's list (SPIRA_REFILLED_SESSION of spira_query.h).
template <class T, bool ANY>
__global__ __launch_bounds__(kBlock) void k_sweep_session(const SweepArgs<T> a) {
    extern __shared__ __attribute__((aligned(32))) unsigned char lds_raw[];
    const SceneLds<T> sc = stage_scene<T>(a.scene, lds_raw);     // the only workgroup barrier of the kernel
    uint32_t begin, end;
    session_range(a.base, a.rem, begin, end);
    uint32_t stack[kBvhStackD];
    const int base = (int)(sc.n_spheres + sc.n_triangles);
    uint32_t item_ = 0;
    SweepWalk<T> w{};
    Sweep8Ray r{};
    const auto start = [&](uint32_t item) -> bool {
            item_ = item;
            const bool ok = sweep_load<T>(a, sc, true, item_, w);
            bool walks = false;
            if (ok) {
                sweep_scan_local<T, false, ANY>(a, sc, w);
                if (!(ANY && w.prim >= 0)) walks = sweep8_enter<T>(sc, w, r);
            }
            if (!walks) sweep_store<T, ANY>(a, item_, ok, w);
            return walks;
    };
    const auto step = [&]() -> bool {
            if (sweep8_step<T>(sc, w, r, base, stack) && !(ANY && w.prim >= 0)) return true;
            sweep_store<T, ANY>(a, item_, true, w);
            return false;
    };
    SPIRA_REFILLED_SESSION(begin, end, a.refill_free, start, step);
}

}  // namespace spira
#endif
