// spira_gather.h — hemisphere gather at surface points on a scene handle: per-point radiance sums (spira_scene_gather_*), per-point counts of unoccluded
// directions (spira_scene_gather_visible_*) and the generator that writes one sample's rays as a list (spira_gather_rays_*).  Included by spira_hip.hip
// behind spira_radiance.h: the path loop is k_radiance's (trace_segment<T, BVH, EXT> of spira_device.h, unedited), the occlusion walk
// k_cast_session's (SPIRA_REFILLED_SESSION, cast_scan_local, bvh8_enter / bvh8_begin / bvh8_step, cast_ray_prepare of spira_query.h).  Launch arithmetic:
// spira_plan.h (make_gather_plan).  The first part of this file needs no HIP header: a CPU program (tests/native/gather_plan.cpp) calls the very
// function the kernels and the host entry generate a ray with.
//
// A point is six values of the call's precision T: [px py pz nx ny nz].  The sampling rule (gather_ray_generate), in T, in exactly this order, nothing
// fused (-ffp-contract=off):
//     validity    radiance_ray_prepare on the six values: INVALID when any is NaN or infinite, or (nx nx + ny ny) + nz nz is not finite or below the
//                 smallest normal number of T; else nh = n / sqrt(n.n) (that function's unit direction)
//     q           point k, sample s: tries t = 1 .. 64 of rng3(rng_key(sA, sB, key0 + k, s, 255), t) with the scale 2^-20 (2 u, exact),
//                 q = (u0 - 1, u1 - 1, u2 - 1), accepted when (q.x q.x + q.y q.y) + q.z q.z < 1, else q = 0 — random_in_unit_sphere of spira_device.h
//                 under bounce 255, the lens's slot: no path reaches it (bounces 0 .. 254) and a gather has no lens.  Try 0 of bounce 0, whose third
//                 uniform is the spectral wavelength, and every key of the path are left alone.
//     qh          q / sqrt(q.q);  q.q below the smallest normal number of T: qh = 0
//     v           nh + qh: a unit normal plus a uniform point ON the unit sphere is an exactly cosine-weighted direction.  Where [p, v] is no valid ray
//                 by radiance_ray_prepare (v cancelled to nothing): v = nh
//     ray         [p, v], v NOT normalised: the radiance entry and the ray queries normalise with one formula, and the gather kernels take their unit
//                 direction from radiance_ray_prepare / cast_ray_prepare on these very six values, so the bits agree
//     invalid     six zeros — which the radiance entry and the ray queries classify as invalid themselves
//
// Kernels:
//   k_gather<T, BVH, EXT>            k_radiance's loop: persistent lanes with path regeneration; a work item is (point, sample), sample-minor; the lane
//                                    GENERATES its ray at regeneration.  A pass of one sample per point: the owning lane adds to sum[k] and writes the
//                                    valid byte.  More samples per pass: L goes to the Pack3<T> workspace, entry = item.
//   k_gather_sum<T>                  one lane per point: adds the point's workspace entries in sample order and writes the valid byte (path_sum_loop).
//   k_gather_visible_session<T>      scenes with a tree: k_cast_session<T, true>'s organisation over the pass's items, on the same loop
//                                    (SPIRA_REFILLED_SESSION of spira_query.h) — each wave owns a contiguous item range, free lanes refill
//                                    (ballot / popcount) and generate their ray, all walking lanes take bvh8_step trips together and leave at the
//                                    first accepted hit.
//   k_gather_visible<T, BVH, TRI>    one lane per item: scenes without a tree, and the SPIRA_CAST_INPLACE comparison point on scenes with one.
//   k_gather_rays<T>                 one lane per point, the six values through LDS so that the workgroup's stores are contiguous (rays_through_tile, as k_camera_rays).
// Counts: a finished item whose ray is unoccluded adds 1 to its point's uint32 with a vector atomic; integer additions commute, so both organisations,
// any grid and any pass split leave the same bytes.  The valid byte of a point is written by the item of its first sample in the call's first pass.
#pragma once
#include <cstdint>

#include "spira_fastdiv.h"      // SPIRA_HD
#include "spira_query.h"        // CastLimits, cast_ray_prepare
#include "spira_radiance.h"     // radiance_ray_prepare, cam_rng_key, cam_rng3, kLensBounce, kLensTries

namespace spira {

constexpr uint32_t kGatherBounce = kLensBounce;      // the RNG key of a gather direction: the lens's slot
constexpr uint32_t kGatherTries = kLensTries;        // kMaxTries of spira_device.h

// The ray of point pt[0..6) for pixel key `key` and `sample`: out6 = [p, v], v not normalised; six zeros and false for an invalid point.
// d: the unit direction radiance_ray_prepare gives for out6 (written for valid points only).
template <class T>
SPIRA_HD inline bool gather_ray_generate(const T *pt, uint32_t sA, uint32_t sB, uint32_t key, uint32_t sample, T out6[6], T d[3]) {
    T nh[3];
    if (!radiance_ray_prepare<T>(pt, nh)) {
        for (int k = 0; k < 6; ++k) out6[k] = (T)0;
        return false;
    }
    const CamKey rk = cam_rng_key(sA, sB, key, sample, kGatherBounce);
    T q[3] = {(T)0, (T)0, (T)0};
    for (uint32_t t = 1; t <= kGatherTries; ++t) {
        T u0, u1, u2;
        cam_rng3<T>(rk, t, (T)(1.0 / 1048576.0), u0, u1, u2);
        const T a0 = u0 - (T)1, a1 = u1 - (T)1, a2 = u2 - (T)1;
        if ((a0 * a0 + a1 * a1) + a2 * a2 < (T)1) { q[0] = a0; q[1] = a1; q[2] = a2; break; }
    }
    const T qq = (q[0] * q[0] + q[1] * q[1]) + q[2] * q[2];
    T qh[3] = {(T)0, (T)0, (T)0};
    if (!(qq < CastLimits<T>::min_normal)) {
        T len;
        if constexpr (sizeof(T) == 4) len = __builtin_sqrtf(qq); else len = __builtin_sqrt(qq);
        qh[0] = q[0] / len; qh[1] = q[1] / len; qh[2] = q[2] / len;
    }
    for (int k = 0; k < 3; ++k) { out6[k] = pt[k]; out6[3 + k] = nh[k] + qh[k]; }
    if (!radiance_ray_prepare<T>(out6, d)) {
        for (int k = 0; k < 3; ++k) out6[3 + k] = nh[k];
        radiance_ray_prepare<T>(out6, d);                // a unit vector at a finite point: always a valid ray
    }
    return true;
}
template <class T>
SPIRA_HD inline bool gather_ray_generate(const T *pt, uint32_t sA, uint32_t sB, uint32_t key, uint32_t sample, T out6[6]) {
    T d[3];
    return gather_ray_generate<T>(pt, sA, sB, key, sample, out6, d);
}

}  // namespace spira

#if defined(__HIPCC__)
// Workgroups of the gather kernel per CU, in waves (SPIRA_GATHER_WAVES_PER_CU; 0: ONE workgroup — small tests reach path regeneration and the session's
// refills with it) and the cap on work items (point, sample) of one pass = entries of the workspace (SPIRA_GATHER_MAX_ITEMS).  The defaults are the
// radiance kernel's, whose loop this is.  The visibility session takes its refill threshold and its waves per CU from the ray queries' knobs
// (SPIRA_CAST_REFILL, SPIRA_CAST_WAVES_PER_CU): it is their kernel over generated rays.
#ifndef SPIRA_GATHER_WAVES_PER_CU
#define SPIRA_GATHER_WAVES_PER_CU 64
#endif
#ifndef SPIRA_GATHER_MAX_ITEMS
#define SPIRA_GATHER_MAX_ITEMS (1u << 26)
#endif

namespace spira {

template <class T> struct GatherArgs {
    SceneGlobal<T> scene;
    RenderConst<T> rc;               // sA, sB, flags, max_depth: what trace_segment and the extensions read; the camera and tile fields are unused
    const T *points;                 // n_points x 6
    uint32_t n_points;
    T *sum;                          // n_points x 3, interleaved
    uint8_t *valid;                  // n_points, or NULL
    Pack3<T> *ws;                    // n_points * spp_pass entries, item-major; NULL: spp_pass == 1, the lanes add to sum themselves
    uint32_t key0, sample_first, spp_pass, n_items;      // n_items = n_points * spp_pass <= SPIRA_GATHER_MAX_ITEMS
    FastDiv fd_spp;
    uint32_t write_valid;            // the first pass of a call writes the valid bytes
};

// The point's six values -> the ray of (key, sample): origin and the unit direction radiance_ray_prepare gives for the generated ray.
template <class T>
__device__ __forceinline__ bool gather_load(const T *points, uint32_t point, uint32_t sA, uint32_t sB, uint32_t key, uint32_t sample, Vec<T> &o, Vec<T> &d) {
    const T *pp = points + 6 * (size_t)point;
    T pt[6], out6[6], dd[3] = {(T)0, (T)0, (T)1};
#pragma unroll
    for (int k = 0; k < 6; ++k) pt[k] = pp[k];
    const bool ok = gather_ray_generate<T>(pt, sA, sB, key, sample, out6, dd);
    o = mk<T>(out6[0], out6[1], out6[2]); d = mk<T>(dd[0], dd[1], dd[2]);
    return ok;
}

// Launch bounds: the workgroup size alone, as k_radiance and k_mega — the body is theirs.
template <class T, bool BVH, bool EXT>
__global__ __launch_bounds__(kBlock) void k_gather(const GatherArgs<T> a) {
    extern __shared__ __attribute__((aligned(32))) unsigned char lds_raw[];
    const SceneLds<T> sc = stage_scene<T>(a.scene, lds_raw);     // the only workgroup barrier of the kernel
    const RenderConst<T> &rc = a.rc;
    const uint32_t stride = gridDim.x * kBlock;
    uint32_t idx = blockIdx.x * kBlock + threadIdx.x;
    bool fresh = true;
    uint32_t point = 0, pixel = 0, sample = 0, b = 0;
    Vec<T> o = mk<T>(0, 0, 0), d = mk<T>(0, 0, 1), beta = mk<T>(1, 1, 1), Lacc = mk<T>(0, 0, 0);
    ExtState<T> ex; ex.flags = rc.flags; ex.bR = 0; ex.bG = 0; ex.bB = 0;
    while (idx < a.n_items) {
        if (fresh) {
            point = fastdiv(idx, a.fd_spp);
            const uint32_t s = idx - point * a.spp_pass;
            pixel = a.key0 + point; sample = a.sample_first + s;
            const bool ok = gather_load<T>(a.points, point, rc.sA, rc.sB, pixel, sample, o, d);
            if (!a.ws && a.valid && a.write_valid) a.valid[point] = ok ? (uint8_t)1 : (uint8_t)0;
            if (!ok) { idx += stride; continue; }                // an invalid point: nothing traced, nothing added (k_gather_sum skips it as well)
            beta = mk<T>(1, 1, 1); Lacc = mk<T>(0, 0, 0); b = 0;
            if (EXT && (rc.flags & kExtSpectral)) beta = ext_wavelength<T>(sc, rc.sA, rc.sB, pixel, sample, ex);
            fresh = false;
        }
        Vec<T> contrib; T t_hit;
        SegInfo si = trace_segment<T, BVH, EXT>(sc, rc, o, d, beta, pixel, sample, b, b + 1 < rc.max_depth, contrib, t_hit, &ex);
        if (b == 0) { if (si.has_contrib) Lacc = contrib; }
        else if (si.has_contrib) Lacc = Lacc + contrib;
        ++b;
        if (!si.alive || b == rc.max_depth) {
            if (a.ws) {
                Pack3<T> l; l.x = Lacc.x; l.y = Lacc.y; l.z = Lacc.z;
                a.ws[idx] = l;
            } else {                                             // one sample of this point in the pass: this lane is the point's only owner
                T *sp = a.sum + 3 * (size_t)point;
                sp[0] = sp[0] + Lacc.x; sp[1] = sp[1] + Lacc.y; sp[2] = sp[2] + Lacc.z;
            }
            idx += stride;
            fresh = true;
        }
    }
}

// The pass's workspace entries of every valid point, added in sample order.
template <class T>
__global__ __launch_bounds__(kBlock) void k_gather_sum(const GatherArgs<T> a) {
    path_sum_loop<T>(a, a.n_points, [&](uint32_t point) -> bool {
        const T *pp = a.points + 6 * (size_t)point;
        T pt[6], nh[3];
#pragma unroll
        for (int k = 0; k < 6; ++k) pt[k] = pp[k];
        return radiance_ray_prepare<T>(pt, nh);
    });
}

template <class T> struct GatherVisibleArgs {
    SceneGlobal<T> scene;
    const T *points;                 // n_points x 6
    uint32_t n_points;
    uint32_t *visible;               // n_points: added to
    uint8_t *valid;                  // n_points, or NULL
    uint32_t sA, sB, key0, sample_first, spp_pass, n_items;      // n_items = n_points * spp_pass <= SPIRA_GATHER_MAX_ITEMS
    FastDiv fd_spp;
    T t_min, t_max;                  // the call's, rounded to T once
    uint32_t write_valid;            // the first pass of a call writes the valid bytes
    uint32_t base, rem;              // session: wave w owns base + (w < rem) items from w base + min(w, rem)  (CastPlan over the pass's items)
    uint32_t refill_free;
};

// Item -> (point, sample), the generated ray [p, t_min, v, t_max] through cast_ray_prepare (the ray queries' classification, the origin rule of scenes
// with a tree included).  The item of a point's first sample in the first pass writes the point's valid byte.
template <class T>
__device__ __forceinline__ bool gather_visible_load(const GatherVisibleArgs<T> &a, const SceneLds<T> &sc, bool frame, uint32_t item, uint32_t &point, Vec<T> &o, Vec<T> &d) {
    point = fastdiv(item, a.fd_spp);
    const uint32_t s = item - point * a.spp_pass;
    const T *pp = a.points + 6 * (size_t)point;
    T pt[6], out6[6], r[8], dd[3] = {(T)0, (T)0, (T)0}, fr[4] = {(T)0, (T)0, (T)0, (T)1};
#pragma unroll
    for (int k = 0; k < 6; ++k) pt[k] = pp[k];
    gather_ray_generate<T>(pt, a.sA, a.sB, a.key0 + point, a.sample_first + s, out6);
    r[0] = out6[0]; r[1] = out6[1]; r[2] = out6[2]; r[3] = a.t_min; r[4] = out6[3]; r[5] = out6[4]; r[6] = out6[5]; r[7] = a.t_max;
    if (frame) { const Pack4<T> f = sc.bvh_root[2]; fr[0] = f.x; fr[1] = f.y; fr[2] = f.z; fr[3] = f.w; }
    const bool ok = cast_ray_prepare<T>(r, frame, fr, dd);       // (an invalid point is six zeros: a zero direction, invalid here as well)
    o = mk<T>(r[0], r[1], r[2]); d = mk<T>(dd[0], dd[1], dd[2]);
    if (s == 0 && a.valid && a.write_valid) a.valid[point] = ok ? (uint8_t)1 : (uint8_t)0;
    return ok;
}

// One lane per item.  Launches: <T, false, false> spheres alone, <T, false, true> with LDS triangles, <T, true, false> a BVH mesh (SPIRA_CAST_INPLACE).
template <class T, bool BVH, bool TRI>
__global__ __launch_bounds__(kBlock) void k_gather_visible(const GatherVisibleArgs<T> a) {
    extern __shared__ __attribute__((aligned(32))) unsigned char lds_raw[];
    const SceneLds<T> sc = stage_scene<T>(a.scene, lds_raw);     // the only workgroup barrier of the kernel
    for (uint32_t i = blockIdx.x * kBlock + threadIdx.x; i < a.n_items; i += gridDim.x * kBlock) {
        Vec<T> o, d; uint32_t point;
        if (!gather_visible_load<T>(a, sc, BVH, i, point, o, d)) continue;
        T closest = 0; int prim = -1; uint32_t slot = 0;
        cast_scan_local<T, TRI>(sc, o, d, a.t_min, a.t_max, closest, prim);
        if (BVH && prim < 0) bvh_closest_hit<T>(sc, o, d, a.t_min, closest, prim, slot);
        if (prim < 0) atomicAdd(a.visible + point, 1u);
    }
}

// Scenes with a tree: a refilled traversal session per wave over its range of the pass's items (SPIRA_REFILLED_SESSION of spira_query.h; k_cast_session<T, true>'s
// two callables with generated rays and a count in place of the hit byte).
template <class T>
__global__ __launch_bounds__(kBlock) void k_gather_visible_session(const GatherVisibleArgs<T> a) {
    constexpr int KL = kCastLdsStack;
    extern __shared__ __attribute__((aligned(32))) unsigned char lds_raw[];
    const SceneLds<T> sc = stage_scene<T>(a.scene, lds_raw);     // the only workgroup barrier of the kernel
    uint32_t begin, end;
    session_range(a.base, a.rem, begin, end);
    uint32_t *lstack = session_lstack<T>(lds_raw, a.scene);
    uint32_t stack[kBvhStackD - KL];
    const uint32_t lane = threadIdx.x & 63;
    const int base = (int)(sc.n_spheres + sc.n_triangles);
    uint32_t point = 0, slot = 0;
    Vec<T> o = mk<T>(0, 0, 0), d = mk<T>(0, 0, 1);
    T closest = 0;
    int prim = -1;
    Bvh8Ray ry{};
    Bvh8Walk<T> wk{};
    const auto start = [&](uint32_t item) -> bool {
            prim = -1; slot = 0; closest = 0;
            if (gather_visible_load<T>(a, sc, true, item, point, o, d)) {
                cast_scan_local<T, false>(sc, o, d, a.t_min, a.t_max, closest, prim);
                T t0;
                if (prim < 0 && bvh8_enter<T>(sc, o, d, closest, ry, t0)) { bvh8_begin<T>(wk, ry, t0, a.t_min, sc.bvh_root[2].w); return true; }
                else if (prim < 0) atomicAdd(a.visible + point, 1u);      // nothing in LDS and the ray misses the mesh's box
            }
            return false;
    };
    const auto step = [&]() -> bool {
            bool on = bvh8_step<T, KL>(sc, wk, ry, o, d, a.t_min, base, closest, prim, slot, lstack, stack, lane);
            if (prim >= 0) on = false;                           // the first accepted hit ends the walk (pending Float64 candidates are dropped)
            if (on) return true;
            // the screened Float64 walk (experiment build): its pending candidates are resolved before the lane counts as finished
            if (prim < 0) while (wk.nc) bvh8_resolve_one<T>(sc, wk, ry, o, d, a.t_min, base, closest, prim, slot);
            if (prim < 0) atomicAdd(a.visible + point, 1u);
            return false;
    };
    SPIRA_REFILLED_SESSION(begin, end, a.refill_free, start, step);
}

template <class T> struct GatherRaysArgs {
    const T *points;                 // n x 6
    T *rays;                         // n x 6
    uint32_t n, sample, sA, sB, key0;
};

template <class T>
__global__ __launch_bounds__(kBlock) void k_gather_rays(const GatherRaysArgs<T> a) {
    __shared__ T tile[kBlock * 6];
    rays_through_tile<T>(tile, a.rays, a.n, [&](uint32_t k, T out6[6]) {
        const T *pp = a.points + 6 * (size_t)k;
        T pt[6];
#pragma unroll
        for (int c = 0; c < 6; ++c) pt[c] = pp[c];
        gather_ray_generate<T>(pt, a.sA, a.sB, a.key0 + k, a.sample, out6);
    });
}

}  // namespace spira
#endif
