// spira_radiance.h — path-traced radiance along the CALLER'S rays on a scene handle (spira_scene_radiance_*) and the camera ray generator that feeds
// it (spira_camera_rays_*).  Included by spira_hip.hip behind spira_device.h, whose trace_segment<T, BVH, EXT> — one whole segment by one lane, the body of
// k_mega — the radiance kernel is built from, unedited; no render kernel is touched.  Launch arithmetic: spira_plan.h (make_radiance_plan).  The first part
// of this file needs no HIP header: a CPU program (tests/native/radiance_plan.cpp) calls the very functions the kernels classify a ray and generate one with.
//
// A ray is six values of the call's precision T: [ox oy oz dx dy dz].  Preparation, in T, nothing fused (-ffp-contract=off):
//     s = (dx dx + dy dy) + dz dz,   d = (dx, dy, dz) / sqrt(s)            (normalize of spira_device.h, cast_ray_prepare of spira_query.h)
// A ray is INVALID (out_valid 0, nothing added to its sums) when any of its six values is NaN or infinite, or s is not finite or below the smallest normal
// number of T.  There is no origin rule: every segment of the path, the first included, is the renderer's own (t_min 0.001, closest_hit).
// Ray k, sample s is the path the renderer traces for a camera ray of that origin and unit direction at pixel key key0 + k: rng_key(sA, sB, key0 + k, s,
// bounce) with sA, sB derived from the seed as fill_const derives them; scatter while bounce + 1 < max_depth; the sums take one addition per sample in
// ascending sample order, sum = sum + L_s — the contract of spira_accumulate_*.
//
// The generator (camera_ray_generate), for reference pixel (i, j) (1-based, j = 1 the bottom row), ix = i - 1, jy = j - 1, pixel = jy W + ix, in T, in
// exactly this order, nothing fused:
//     (xu, xv) = the first two uniforms of rng3(rng_key(sA, sB, pixel, sample, 0), 0)                 (camera_ray of spira_device.h)
//     u = (ix + xu) / (W - 1),  v = (jy + xv) / (H - 1),  P = (llc + hor u) + ver v
//     PINHOLE     o = origin,  d = P - origin                                                         (the renderer's camera ray before normalisation)
//     THIN_LENS   lens_radius == 0: PINHOLE.  Else eu = hor / sqrt((hor.x hor.x + hor.y hor.y) + hor.z hor.z), ev likewise of ver;
//                 the lens point p: tries t = 1 .. kMaxTries of rng3(rng_key(sA, sB, pixel, sample, 255), t) with the scale 2^-20 (2 u, exact),
//                 p = (u0 - 1, u1 - 1), accepted when p.x p.x + p.y p.y < 1, else p = 0 (random_in_unit_disk of the reference, the idiom of
//                 random_in_unit_sphere); bounce 255 is no path's (max_depth <= 255: bounces 0 .. 254);
//                 off = eu (R p.x) + ev (R p.y),  o = origin + off,  d = (P - origin) - off          (R = lens_radius rounded to T once)
//     ORTHO       o = P,  d = ((llc + hor / 2) + ver / 2) - origin                                    (every ray along the camera axis)
// Rays are ordered by reference pixel, k = (jy - row0) W + ix; the key of ray k for the radiance entry is its global pixel, key0 = row0 W.
//
// Kernels:
//   k_radiance<T, BVH, EXT>   persistent lanes with path regeneration, k_mega's loop: a work item is (ray, sample), sample-minor (item = ray * spp_pass +
//                             s, decoded with fastdiv), so neighbouring lanes share a first segment; a lane whose path ended takes its next item at once.
//                             A pass of one sample per ray (the camera case): the owning lane does sum[k] = sum[k] + L — one owner per ray, no atomics —
//                             and writes the valid byte.  More samples per pass: L goes to the Pack3<T> workspace, entry = item.
//   k_radiance_sum<T>         one lane per ray: adds the ray's workspace entries in sample order and writes the valid byte.
//   k_camera_rays<T>          one lane per ray, the six values through LDS so that the workgroup's stores are contiguous.
// Two bodies are written once, here, for these kernels and their twins of spira_gather.h: path_sum_loop (the two sum kernels: the callable is the validity
// of an entry) and rays_through_tile (the two generators: the callable writes the six values of ray k).  k_radiance and k_gather keep a loop each: one body
// for both, taking the fresh-item block as a callable, measured 1-4 % slower on the Float64 instantiations (docs/experiments.md section 32).
#pragma once
#include <cstdint>

#include "spira_fastdiv.h"      // SPIRA_HD
#include "spira_query.h"        // CastLimits

namespace spira {

constexpr uint32_t kCamPinhole = 0, kCamThinLens = 1, kCamOrtho = 2;      // SPIRA_CAM_* (include/spira_hip.h)
constexpr uint32_t kLensBounce = 255;                                     // the RNG key of the lens point: a bounce index no path reaches
constexpr uint32_t kLensTries = 64;                                       // kMaxTries of spira_device.h

// One ray r[0..6) -> valid?  d: the unit direction (written for valid rays only).
template <class T> SPIRA_HD inline bool radiance_ray_prepare(const T *r, T d[3]) {
    for (int k = 0; k < 6; ++k) if (!((r[k] - r[k]) == (T)0)) return false;         // NaN or infinite anywhere
    const T s = (r[3] * r[3] + r[4] * r[4]) + r[5] * r[5];
    if (!((s - s) == (T)0) || s < CastLimits<T>::min_normal) return false;
    T len;
    if constexpr (sizeof(T) == 4) len = __builtin_sqrtf(s); else len = __builtin_sqrt(s);
    d[0] = r[3] / len; d[1] = r[4] / len; d[2] = r[5] / len;
    return true;
}

// The counter RNG of spira_device.h (mix32, rng_key, rng3) restated for host and device: integer hashing and one exact conversion, so the same bits.
SPIRA_HD inline uint32_t cam_mix32(uint32_t x) {
    x ^= x >> 16; x *= 0x7feb352dU;
    x ^= x >> 15; x *= 0x846ca68bU;
    x ^= x >> 16;
    return x;
}
struct CamKey { uint32_t hA, hB, hBr; };
SPIRA_HD inline CamKey cam_rng_key(uint32_t sA, uint32_t sB, uint32_t pixel, uint32_t sample, uint32_t bounce) {
    const uint32_t sb = (sample << 8) | bounce;
    CamKey k;
    k.hA = cam_mix32(cam_mix32(sA + pixel) ^ sb);
    k.hB = cam_mix32(cam_mix32(sB ^ pixel) + sb);
    k.hBr = (k.hB << 16) | (k.hB >> 16);
    return k;
}
template <class T> SPIRA_HD inline void cam_rng3(const CamKey &k, uint32_t t, T s, T &u0, T &u1, T &u2) {
    const uint32_t a = cam_mix32((k.hA + t * 0x9E3779B9u) ^ k.hBr);
    const uint32_t b = cam_mix32(a + k.hB);
    u0 = (T)(a >> 11) * s;
    u1 = (T)(b >> 11) * s;
    u2 = (T)(((a & 0x7FFu) << 10) | (b & 0x3FFu)) * s;
}
// the mixed seed halves every entry derives its keys from (fill_const of spira_hip.hip)
SPIRA_HD inline void seed_halves(uint64_t seed, uint32_t &sA, uint32_t &sB) {
    const uint32_t lo = (uint32_t)seed, hi = (uint32_t)(seed >> 32);
    sA = cam_mix32(cam_mix32(lo + 0x9E3779B9u) ^ hi);
    sB = cam_mix32(cam_mix32(hi + 0x85EBCA6Bu) ^ lo);
}

// The ray of pixel (ix, jy) (0-based, jy = 0 the bottom row) and `sample`: out6 = [o, d], d not normalised.  cam: origin, llc, hor, ver.
template <class T>
SPIRA_HD inline void camera_ray_generate(const T *cam, uint32_t model, uint32_t width, uint32_t height, uint32_t sA, uint32_t sB,
                                         uint32_t ix, uint32_t jy, uint32_t sample, T lens_radius, T out6[6]) {
    const uint32_t pixel = jy * width + ix;
    T xu, xv, unused;
    cam_rng3<T>(cam_rng_key(sA, sB, pixel, sample, 0), 0, (T)(1.0 / 2097152.0), xu, xv, unused);
    const T u = ((T)ix + xu) / (T)(width - 1);
    const T v = ((T)jy + xv) / (T)(height - 1);
    T P[3], q[3];
    for (int k = 0; k < 3; ++k) P[k] = (cam[3 + k] + cam[6 + k] * u) + cam[9 + k] * v;
    for (int k = 0; k < 3; ++k) q[k] = P[k] - cam[k];
    if (model == kCamOrtho) {
        for (int k = 0; k < 3; ++k) { out6[k] = P[k]; out6[3 + k] = ((cam[3 + k] + cam[6 + k] / (T)2) + cam[9 + k] / (T)2) - cam[k]; }
        return;
    }
    if (model == kCamThinLens && lens_radius != (T)0) {
        const T su = (cam[6] * cam[6] + cam[7] * cam[7]) + cam[8] * cam[8], sv = (cam[9] * cam[9] + cam[10] * cam[10]) + cam[11] * cam[11];
        T lu, lv;
        if constexpr (sizeof(T) == 4) { lu = __builtin_sqrtf(su); lv = __builtin_sqrtf(sv); } else { lu = __builtin_sqrt(su); lv = __builtin_sqrt(sv); }
        const CamKey key = cam_rng_key(sA, sB, pixel, sample, kLensBounce);
        T px = 0, py = 0;
        for (uint32_t t = 1; t <= kLensTries; ++t) {
            T u0, u1, u2;
            cam_rng3<T>(key, t, (T)(1.0 / 1048576.0), u0, u1, u2);
            const T ax = u0 - (T)1, ay = u1 - (T)1;
            if (ax * ax + ay * ay < (T)1) { px = ax; py = ay; break; }
        }
        const T rx = lens_radius * px, ry = lens_radius * py;
        for (int k = 0; k < 3; ++k) {
            const T off = (cam[6 + k] / lu) * rx + (cam[9 + k] / lv) * ry;
            out6[k] = cam[k] + off; out6[3 + k] = q[k] - off;
        }
        return;
    }
    for (int k = 0; k < 3; ++k) { out6[k] = cam[k]; out6[3 + k] = q[k]; }
}

}  // namespace spira

#if defined(__HIPCC__)
// Workgroups of the radiance kernel per CU, in waves (SPIRA_RADIANCE_WAVES_PER_CU; 0: ONE workgroup, the smallest grid there is — small tests reach
// path regeneration with it) and the cap on work items (ray, sample) of one pass = entries of the workspace (SPIRA_RADIANCE_MAX_ITEMS).
// 64 waves per CU is k_mega's grid (make_plan: 16 workgroups per CU for the organisations that are not k_path), whose loop this kernel runs.
#ifndef SPIRA_RADIANCE_WAVES_PER_CU
#define SPIRA_RADIANCE_WAVES_PER_CU 64
#endif
#ifndef SPIRA_RADIANCE_MAX_ITEMS
#define SPIRA_RADIANCE_MAX_ITEMS (1u << 26)
#endif

namespace spira {

template <class T> struct RadianceArgs {
    SceneGlobal<T> scene;
    RenderConst<T> rc;               // sA, sB, flags, max_depth: what trace_segment and the extensions read; the camera and tile fields are unused
    const T *rays;                   // n_rays x 6
    uint32_t n_rays;
    T *sum;                          // n_rays x 3, interleaved
    uint8_t *valid;                  // n_rays, or NULL
    Pack3<T> *ws;                    // n_rays * spp_pass entries, item-major; NULL: spp_pass == 1, the lanes add to sum themselves
    uint32_t key0, sample_first, spp_pass, n_items;      // n_items = n_rays * spp_pass <= SPIRA_RADIANCE_MAX_ITEMS
    FastDiv fd_spp;
    uint32_t write_valid;            // the first pass of a call writes the valid bytes
};

template <class T>
__device__ __forceinline__ bool radiance_load(const T *rays, uint32_t ray, Vec<T> &o, Vec<T> &d) {
    const T *rp = rays + 6 * (size_t)ray;
    T r[6], dd[3] = {(T)0, (T)0, (T)1};
#pragma unroll
    for (int k = 0; k < 6; ++k) r[k] = rp[k];
    const bool ok = radiance_ray_prepare<T>(r, dd);
    o = mk<T>(r[0], r[1], r[2]); d = mk<T>(dd[0], dd[1], dd[2]);
    return ok;
}

// The body of k_radiance_sum and k_gather_sum: one lane per list entry; the pass's workspace entries of every entry valid(k) accepts, added in sample order.
template <class T, class Args, class Valid>
__device__ __forceinline__ void path_sum_loop(const Args &a, uint32_t n, Valid valid) {
    for (uint32_t k = blockIdx.x * kBlock + threadIdx.x; k < n; k += gridDim.x * kBlock) {
        const bool ok = valid(k);
        if (a.valid && a.write_valid) a.valid[k] = ok ? (uint8_t)1 : (uint8_t)0;
        if (!ok) continue;
        T *sp = a.sum + 3 * (size_t)k;
        T x = sp[0], y = sp[1], z = sp[2];
        const Pack3<T> *l = a.ws + (size_t)k * a.spp_pass;
        for (uint32_t s = 0; s < a.spp_pass; ++s) { x = x + l[s].x; y = y + l[s].y; z = z + l[s].z; }
        sp[0] = x; sp[1] = y; sp[2] = z;
    }
}

// The body of k_camera_rays and k_gather_rays: one lane per ray, gen(k, out6) for k < n, the six values through the workgroup's LDS tile so that its stores
// are contiguous.  The grid covers n: one workgroup per kBlock rays.
template <class T, class Gen>
__device__ __forceinline__ void rays_through_tile(T *tile, T *rays, uint32_t n, Gen gen) {
    const uint32_t first = blockIdx.x * kBlock, k = first + threadIdx.x;
    if (k < n) {
        T out6[6];
        gen(k, out6);
#pragma unroll
        for (int c = 0; c < 6; ++c) tile[6 * threadIdx.x + c] = out6[c];
    }
    __syncthreads();
    const uint32_t n_here = min((uint32_t)kBlock, n - first) * 6;              // first < n for every workgroup of the grid
    T *dst = rays + 6 * (size_t)first;
    for (uint32_t v = threadIdx.x; v < n_here; v += kBlock) dst[v] = tile[v];
}

// Launch bounds: the workgroup size alone, as k_mega — the body is k_mega's, and the resource report shows the same registers.
template <class T, bool BVH, bool EXT>
__global__ __launch_bounds__(kBlock) void k_radiance(const RadianceArgs<T> a) {
    extern __shared__ __attribute__((aligned(32))) unsigned char lds_raw[];
    const SceneLds<T> sc = stage_scene<T>(a.scene, lds_raw);     // the only workgroup barrier of the kernel
    const RenderConst<T> &rc = a.rc;
    const uint32_t stride = gridDim.x * kBlock;
    uint32_t idx = blockIdx.x * kBlock + threadIdx.x;
    bool fresh = true;
    uint32_t ray = 0, pixel = 0, sample = 0, b = 0;
    Vec<T> o = mk<T>(0, 0, 0), d = mk<T>(0, 0, 1), beta = mk<T>(1, 1, 1), Lacc = mk<T>(0, 0, 0);
    ExtState<T> ex; ex.flags = rc.flags; ex.bR = 0; ex.bG = 0; ex.bB = 0;
    while (idx < a.n_items) {
        if (fresh) {
            ray = fastdiv(idx, a.fd_spp);
            const uint32_t s = idx - ray * a.spp_pass;
            const bool ok = radiance_load<T>(a.rays, ray, o, d);
            if (!a.ws && a.valid && a.write_valid) a.valid[ray] = ok ? (uint8_t)1 : (uint8_t)0;
            if (!ok) { idx += stride; continue; }                // an invalid ray: nothing traced, nothing added (k_radiance_sum skips it as well)
            pixel = a.key0 + ray; sample = a.sample_first + s;
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
            } else {                                             // one sample of this ray in the pass: this lane is the ray's only owner
                T *sp = a.sum + 3 * (size_t)ray;
                sp[0] = sp[0] + Lacc.x; sp[1] = sp[1] + Lacc.y; sp[2] = sp[2] + Lacc.z;
            }
            idx += stride;
            fresh = true;
        }
    }
}

// The pass's workspace entries of every valid ray, added in sample order.
template <class T>
__global__ __launch_bounds__(kBlock) void k_radiance_sum(const RadianceArgs<T> a) {
    path_sum_loop<T>(a, a.n_rays, [&](uint32_t ray) -> bool {
        Vec<T> o, d;
        return radiance_load<T>(a.rays, ray, o, d);
    });
}

template <class T> struct CameraRaysArgs {
    T cam[12];
    T lens_radius;
    T *rays;                         // n x 6
    uint32_t model, width, height, sample, sA, sB, row0, n;      // n = rows * width
    FastDiv fd_width;
};

template <class T>
__global__ __launch_bounds__(kBlock) void k_camera_rays(const CameraRaysArgs<T> a) {
    __shared__ T tile[kBlock * 6];
    rays_through_tile<T>(tile, a.rays, a.n, [&](uint32_t k, T out6[6]) {
        const uint32_t r = fastdiv(k, a.fd_width), ix = k - r * a.width;
        camera_ray_generate<T>(a.cam, a.model, a.width, a.height, a.sA, a.sB, ix, a.row0 + r, a.sample, a.lens_radius, out6);
    });
}

}  // namespace spira
#endif
