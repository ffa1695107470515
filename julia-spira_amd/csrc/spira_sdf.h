// spira_sdf.h — signed distance queries on a scene handle (spira_scene_signed_distance_*): for every point of a caller's list the nearest surface AND which
// side of it the point is on.  Included by spira_hip.hip behind spira_hits.h; built from spira_nearest.h (the point's load and validity rule, the LDS scan,
// the distance-pruned walk near_step) and from spira_hits.h (the crossing count: hits8_step with K = 0 under count_all), through the loop of spira_query.h
// (SPIRA_REFILLED_SESSION).  No existing device function is changed; every one used is used as it is.  The first part of this file needs no HIP header.
//
// The contract (include/spira_hip.h, "signed distance queries"), per valid point p, every step in T, in the written order, nothing fused:
//   1. nearest surface: the closest-point scan of spira_scene_closest_point_* unchanged — prim and point are that entry's bytes, dist is its value with the
//      sign bit set where the point is inside.
//   2. inside a sphere: w = p - c, l = sqrt(w.w) (closest_point_sphere's values), the radius as given (spheres5[5 s + 3]): inside when l < r.
//   3. inside the mesh: ray j = [p, t_min 0, D_j, t_max +Inf], D_j = sdf_direction(j), spira_hip.query.INSIDE_DIRECTIONS[j] rounded to T, prepared by
//      cast_ray_prepare; c_j = the number of TRIANGLE candidates of that ray under the multi-hit candidate rule (hit_triangle with the ray's own t_min and
//      t_max; spheres are not tested).  Rays 0 and 1 are always walked; equal parities decide and c_2 = SPIRA_SDF_SKIPPED; otherwise ray 2 is walked and its
//      parity decides — the majority of three votes, as query.inside_mesh forms it.  No triangle in the scene: all three SPIRA_SDF_SKIPPED, not inside a mesh.
//   4. inside = step 2 or step 3.
// The ray of a valid point is always valid: its origin is finite and (scenes with a tree) inside the origin rule, because the point is — the two rules are
// the same expression on the same values — its direction is a constant of length about 1, t_min = 0 <= t_max.  So cast_ray_prepare is called for the unit
// direction alone, without the frame.
//
// Kernels (each stages the scene with stage_scene: one barrier; ExactDiv everywhere):
//   k_sdf<T, BVH, TRI, NEAR>    one lane per point, grid-stride: near_load; NEAR: near_scan_local and the near_step loop; the sphere test; then for each ray
//                               it needs the LDS triangle count (TRI; sdf_count_local, new here: hits_scan_local would count spheres) or bvh8_enter /
//                               bvh8_begin and a hits8_step<T, 0, 1> loop with K = 0 under count_all, whose `total` is c_j.
//   k_sdf_session<T, NEAR>      scenes with a tree, the default: ONE refilled session whose lane is a small phase machine — phase 0 the nearest walk, phases
//                               1 .. 3 the rays.  step() takes one trip of whichever walk the lane is in; when that walk ends the next phase is entered (a ray
//                               that misses the root box ends at once with c_j = 0) and only after the last one the lane stores and is free.
//   NEAR = false                the sign-only query (out_prim, out_dist and out_point all NULL): no scan, no nearest walk — a template parameter.
// The two walks are never live in one lane together: they share one stack array.  Lanes of a wave may sit in different phases, so a trip of the session may
// execute both arms; docs/experiments.md says what that costs against k_sdf.
#pragma once
#include <cstdint>

#include "spira_nearest.h"
#include "spira_hits.h"

namespace spira {

constexpr uint32_t kSdfSkipped = 0xFFFFFFFFu;      // SPIRA_SDF_SKIPPED

// D_j of the contract, in T: spira_hip.query.INSIDE_DIRECTIONS — fixed, parallel to no axis and no diagonal.
template <class T> SPIRA_HD inline void sdf_direction(int j, T D[3]) {
    if (j == 0) { D[0] = (T)0.5377; D[1] = (T)0.7211; D[2] = (T)0.4366; }
    else if (j == 1) { D[0] = (T)-0.6123; D[1] = (T)0.3142; D[2] = (T)0.7255; }
    else { D[0] = (T)0.2873; D[1] = (T)-0.4691; D[2] = (T)-0.8351; }
}
// Ray j of the point p as a caller would hand it to cast: [p, 0, D_j, +Inf].
template <class T> SPIRA_HD inline void sdf_ray(const T p[3], int j, T r[8]) {
    r[0] = p[0]; r[1] = p[1]; r[2] = p[2]; r[3] = (T)0;
    sdf_direction<T>(j, r + 4);
    r[7] = (T)__builtin_inf();
}
// After rays 0 and 1: is ray 2 needed?
SPIRA_HD inline bool sdf_needs_third(uint32_t c0, uint32_t c1) { return ((c0 ^ c1) & 1u) != 0; }
// c_j = n, written as three selects: as an if / else chain over the slots the compiler forms ONE store through a selected address, and a session lane whose
// address is taken lives in scratch memory (seen: 208 bytes a lane in the sign-only session).
SPIRA_HD inline void sdf_record(uint32_t &c0, uint32_t &c1, uint32_t &c2, int j, uint32_t n) {
    c0 = j == 0 ? n : c0; c1 = j == 1 ? n : c1; c2 = j == 2 ? n : c2;
}
// The mesh's verdict from the three slots (c2 == kSdfSkipped: the first two agreed).
SPIRA_HD inline bool sdf_mesh_inside(uint32_t c0, uint32_t c2) { return ((c2 == kSdfSkipped ? c0 : c2) & 1u) != 0; }

}  // namespace spira

#if defined(__HIPCC__)
namespace spira {

// NearestArgs' scene, points, n_points, prim, dist, point, trips, base / rem / refill_free as they are (near_load, near_scan_local and launch_list read them).
template <class T> struct SdfArgs : NearestArgs<T> {
    uint8_t *inside;                 // n_points; may be NULL (as prim, dist, point)
    uint32_t *crossings;             // n_points x 3; may be NULL
};

// Step 2: is p inside one of the spheres?  w and l are the values closest_point_sphere forms; the radius is the caller's.
template <class T>
__device__ __forceinline__ bool sdf_in_spheres(const SdfArgs<T> &a, const SceneLds<T> &sc, const T p[3]) {
    bool in = false;
    for (uint32_t s = 0; s < sc.n_spheres; ++s) {
        const Pack4<T> sp = sc.sph[s];
        const T w[3] = {p[0] - sp.x, p[1] - sp.y, p[2] - sp.z};
        const T l = near_sqrt<T>(near_dot<T>(w, w));
        if (l < a.scene.spheres5[5 * (size_t)s + 3]) in = true;
    }
    return in;
}

// The unit direction of ray j from p, as cast_ray_prepare makes it (header comment: the ray is valid because the point is).
template <class T>
__device__ __forceinline__ Vec<T> sdf_unit_direction(const T p[3], int j) {
    T r[8], d[3] = {(T)0, (T)0, (T)1};
    const T fr[4] = {(T)0, (T)0, (T)0, (T)1};
    sdf_ray<T>(p, j, r);
    cast_ray_prepare<T>(r, false, fr, d);
    return mk<T>(d[0], d[1], d[2]);
}

// The LDS triangles of a scene without a tree: the candidates of one ray, counted — the per-object test hits_scan_local runs, and no sphere.
template <class T>
__device__ __forceinline__ uint32_t sdf_count_local(const SceneLds<T> &sc, Vec<T> o, Vec<T> d, T t_min, T t_max) {
    ExactDiv pol;
    uint32_t c = 0;
    for (uint32_t i = 0; i < sc.n_triangles; ++i) {
        const Pack4<T> v0 = sc.tri[3 * i], e1 = sc.tri[3 * i + 1], e2 = sc.tri[3 * i + 2];
        T t;
        if (triangle_test<T>(v0, e1, e2, o, d, t_min, t_max, t, pol)) ++c;
    }
    return c;
}

template <class T, bool NEAR>
__device__ __forceinline__ void sdf_store(const SdfArgs<T> &a, uint32_t i, bool valid, const NearWalk<T> &w, T r_max, bool inside, uint32_t c0, uint32_t c1, uint32_t c2) {
    if constexpr (NEAR) {
        const bool hit = valid && w.prim >= 0;
        if (a.prim) a.prim[i] = valid ? w.prim : SPIRA_RAY_INVALID;
        if (a.dist) {
            const T x = !valid ? (T)0 : (hit ? near_sqrt<T>(w.best) : r_max);
            a.dist[i] = (valid && inside) ? -abs_t(x) : x;               // the sign bit set where the point is inside: -0 can occur
        }
        if (a.point) { a.point[3 * (size_t)i] = hit ? w.q[0] : (T)0; a.point[3 * (size_t)i + 1] = hit ? w.q[1] : (T)0; a.point[3 * (size_t)i + 2] = hit ? w.q[2] : (T)0; }
    }
    if (a.inside) a.inside[i] = !valid ? (uint8_t)255 : (inside ? (uint8_t)1 : (uint8_t)0);
    if (a.crossings) { a.crossings[3 * (size_t)i] = valid ? c0 : 0u; a.crossings[3 * (size_t)i + 1] = valid ? c1 : 0u; a.crossings[3 * (size_t)i + 2] = valid ? c2 : 0u; }
    if (a.trips) a.trips[i] = w.trips;
}

// One lane per point.  Launches: <T, false, false, .> spheres alone, <T, false, true, .> with LDS triangles, <T, true, false, .> a BVH mesh (SPIRA_CAST_INPLACE).
template <class T, bool BVH, bool TRI, bool NEAR>
__global__ __launch_bounds__(kBlock) void k_sdf(const SdfArgs<T> a) {
    extern __shared__ __attribute__((aligned(32))) unsigned char lds_raw[];
    const SceneLds<T> sc = stage_scene<T>(a.scene, lds_raw);     // the only workgroup barrier of the kernel
    const int base = (int)(sc.n_spheres + sc.n_triangles);
    const T t_min = (T)0, t_max = (T)__builtin_inf();
    for (uint32_t i = blockIdx.x * kBlock + threadIdx.x; i < a.n_points; i += gridDim.x * kBlock) {
        NearWalk<T> w; T r_max;
        const bool ok = near_load<T>(a, sc, BVH, i, w, r_max);
        uint32_t c0 = kSdfSkipped, c1 = kSdfSkipped, c2 = kSdfSkipped;
        bool inside = false;
        if (ok) {
            uint32_t stack[kBvhStackD];                          // one array: the nearest walk's, then each ray's
            if constexpr (NEAR) {
                near_scan_local<T, TRI>(a, sc, w);
                if (BVH) { if (near_enter<T>(sc, w)) while (near_step<T>(sc, w, base, stack)) {} }
            }
            inside = sdf_in_spheres<T>(a, sc, w.p);
            if (BVH || TRI) {
                const Vec<T> o = mk<T>(w.p[0], w.p[1], w.p[2]);
#pragma nounroll
                for (int j = 0; j < 3; ++j) {
                    if (j == 2 && !sdf_needs_third(c0, c1)) break;
                    const Vec<T> d = sdf_unit_direction<T>(w.p, j);
                    uint32_t n = 0;
                    if (TRI) n = sdf_count_local<T>(sc, o, d, t_min, t_max);
                    if (BVH) {
                        HitsLane<T, 1> h;
                        hits_begin<T, 1>(h, t_max);
                        Bvh8Ray r; T t0;
                        if (bvh8_enter<T>(sc, o, d, h.bound, r, t0)) {
                            Bvh8Walk<T> wk;
                            bvh8_begin<T>(wk, r, t0, t_min, sc.bvh_root[2].w);
                            bool on = true;
                            while (on) { ++w.trips; on = hits8_step<T, 0, 1>(sc, wk, r, o, d, t_min, base, h, 0u, true, nullptr, stack, threadIdx.x & 63); }
                        }
                        n += h.total;
                    }
                    sdf_record(c0, c1, c2, j, n);
                }
                if (sdf_mesh_inside(c0, c2)) inside = true;
            }
        }
        sdf_store<T, NEAR>(a, i, ok, w, r_max, inside, c0, c1, c2);
    }
}

// One session lane: the point with the nearest walk's state, and the state of the ray walk of phases 1 .. 3.  The walks are never live together.
template <class T> struct SdfLane {
    NearWalk<T> w; T r_max;
    Vec<T> d;                        // the unit direction of the ray being walked
    HitsLane<T, 1> h;
    Bvh8Ray ry;
    Bvh8Walk<T> wk;
    uint32_t pt, phase;              // phase 0: the nearest walk; 1 + j: ray j
    uint32_t c0, c1, c2;
    bool in_sphere;
};

// The walk of the lane's phase has ended (and a ray's count is recorded): enters the next phase that has something to walk.  false: that was the last one.
template <class T>
__device__ __forceinline__ bool sdf_advance(const SceneLds<T> &sc, SdfLane<T> &L) {
    const T t_min = (T)0, t_max = (T)__builtin_inf();
    while (true) {
        if (L.phase == 3 || (L.phase == 2 && !sdf_needs_third(L.c0, L.c1))) return false;
        ++L.phase;
        const int j = (int)L.phase - 1;
        L.d = sdf_unit_direction<T>(L.w.p, j);
        hits_begin<T, 1>(L.h, t_max);
        T t0;
        if (bvh8_enter<T>(sc, mk<T>(L.w.p[0], L.w.p[1], L.w.p[2]), L.d, L.h.bound, L.ry, t0)) { bvh8_begin<T>(L.wk, L.ry, t0, t_min, sc.bvh_root[2].w); return true; }
        sdf_record(L.c0, L.c1, L.c2, j, 0u);                                   // the ray misses the mesh's box: no crossing
    }
}
template <class T, bool NEAR>
__device__ __forceinline__ void sdf_finish(const SdfArgs<T> &a, const SdfLane<T> &L, bool ok) {
    const bool inside = ok && (L.in_sphere || sdf_mesh_inside(L.c0, L.c2));
    sdf_store<T, NEAR>(a, L.pt, ok, L.w, L.r_max, inside, L.c0, L.c1, L.c2);
}

// Scenes with a tree: one refilled session per wave over its range of the caller's list; the lane is a phase machine (header comment).
template <class T, bool NEAR>
__global__ __launch_bounds__(kBlock) void k_sdf_session(const SdfArgs<T> a) {
    extern __shared__ __attribute__((aligned(32))) unsigned char lds_raw[];
    const SceneLds<T> sc = stage_scene<T>(a.scene, lds_raw);     // the only workgroup barrier of the kernel
    uint32_t begin, end;
    session_range(a.base, a.rem, begin, end);
    uint32_t stack[kBvhStackD];                                  // one array: the walk of the phase the lane is in
    const uint32_t lane = threadIdx.x & 63;
    const int base = (int)(sc.n_spheres + sc.n_triangles);
    const T t_min = (T)0;
    SdfLane<T> L{};
    const auto start = [&](uint32_t item) -> bool {
            L.pt = item;
            const bool ok = near_load<T>(a, sc, true, L.pt, L.w, L.r_max);
            L.phase = 0; L.c0 = 0; L.c1 = 0; L.c2 = kSdfSkipped; L.in_sphere = false;
            bool walks = false;
            if (ok) {
                if constexpr (NEAR) near_scan_local<T, false>(a, sc, L.w);
                L.in_sphere = sdf_in_spheres<T>(a, sc, L.w.p);
                if constexpr (NEAR) walks = near_enter<T>(sc, L.w);
                if (!walks) walks = sdf_advance<T>(sc, L);
            }
            if (!walks) sdf_finish<T, NEAR>(a, L, ok);
            return walks;
    };
    const auto step = [&]() -> bool {
            if (NEAR && L.phase == 0) {
                if (near_step<T>(sc, L.w, base, stack)) return true;
            } else {
                ++L.w.trips;
                if (hits8_step<T, 0, 1>(sc, L.wk, L.ry, mk<T>(L.w.p[0], L.w.p[1], L.w.p[2]), L.d, t_min, base, L.h, 0u, true, nullptr, stack, lane)) return true;
                sdf_record(L.c0, L.c1, L.c2, (int)L.phase - 1, L.h.total);
            }
            if (sdf_advance<T>(sc, L)) return true;
            sdf_finish<T, NEAR>(a, L, true);
            return false;
    };
    SPIRA_REFILLED_SESSION(begin, end, a.refill_free, start, step);
}

}  // namespace spira
#endif
