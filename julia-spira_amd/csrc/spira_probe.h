// spira_probe.h — light probes on a scene handle: the radiance arriving at free points from the whole sphere, projected onto the first nine real spherical
// harmonics (spira_scene_probe_sh_*), the generator that writes one sample's rays as a list (spira_probe_rays_*) and the basis itself (spira_sh9_basis_*).
// Included by spira_hip.hip behind spira_gather.h: the path loop is k_gather's (trace_segment<T, BVH, EXT> of spira_device.h, unedited), the passes and
// the workspace are the gather's (make_gather_plan, the context's Pack3<T> entries, SPIRA_GATHER_WAVES_PER_CU / SPIRA_GATHER_MAX_ITEMS).  The first part
// of this file needs no HIP header: a CPU program (tests/native/probe_plan.cpp) calls the very functions the kernels and the host entries call.
//
// A point is three values of the call's precision T: [px py pz]; it has no normal.  INVALID when any of the three is NaN or infinite; there is no origin
// rule.  The sampling rule (probe_ray_generate), in T, in exactly this order, nothing fused (-ffp-contract=off):
//     q           the gather's draw, exactly: point k, sample s, tries t = 1 .. 64 of rng3(rng_key(sA, sB, key0 + k, s, 255), t) with the scale 2^-20,
//                 a = (u0 - 1, u1 - 1, u2 - 1), accepted when (a.x a.x + a.y a.y) + a.z a.z < 1, else q = 0.  Written a second time here, so that no
//                 k_gather* listing moves.
//     qh          q / sqrt(q.q);  q.q below the smallest normal number of T (no try accepted): qh = (0, 0, 1).  A uniform point in the ball,
//                 normalised, is uniform on the sphere.
//     ray         [p, qh], qh NOT normalised again: the radiance entry normalises with radiance_ray_prepare, and the probe kernels take their unit
//                 direction d from that function on these very six values, so the bits agree.  Every valid point has a valid ray for every sample.
//     invalid     six zeros.
// The basis (sh9_basis), x y z = d, the constants double literals rounded to T once, no Condon-Shortley sign:
//     Y0 = c0   Y1 = c1 y   Y2 = c1 z   Y3 = c1 x   Y4 = c2 (x y)   Y5 = c2 (y z)   Y6 = c3 (3 (z z) - 1)   Y7 = c2 (x z)   Y8 = c4 (x x - y y)
// The sums: sum[k][j][c] = sum[k][j][c] + Y_j(d_s) * L_s[c] for s ascending — one product, then one addition.
//
// Kernels:
//   k_probe<T, BVH, EXT>     k_gather's loop with the fresh-item block replaced: persistent lanes with path regeneration over items (point, sample),
//                            sample-minor; the lane keeps the unit direction d0 of bounce 0 (the path overwrites d).  A pass of one sample per point: the
//                            owning lane forms Y(d0), does the 27 read-modify-writes and writes the valid byte.  More samples per pass: L goes to the
//                            Pack3<T> workspace, entry = item.
//   k_probe_sum<T>           one lane per point, 27 accumulators: adds the point's workspace entries in sample order, each times Y of the direction it
//                            REGENERATES from the key (integer hashing and a handful of flops; the direction is not stored, so the workspace and its plan
//                            are the gather's), and writes the valid byte.  path_sum_loop adds three sums per entry: the loop is written here.
//   k_probe_rays<T>          one lane per point, the six values through LDS (rays_through_tile).
#pragma once
#include <cstdint>

#include "spira_fastdiv.h"      // SPIRA_HD
#include "spira_query.h"        // CastLimits
#include "spira_radiance.h"     // radiance_ray_prepare, cam_rng_key, cam_rng3, kLensBounce, kLensTries

namespace spira {

constexpr uint32_t kProbeBounce = kLensBounce;       // the RNG key of a probe direction: the gather's slot (the lens's), which no path reaches
constexpr uint32_t kProbeTries = kLensTries;         // kMaxTries of spira_device.h

template <class T> SPIRA_HD inline bool probe_point_valid(const T *p) {
    return (p[0] - p[0]) == (T)0 && (p[1] - p[1]) == (T)0 && (p[2] - p[2]) == (T)0;      // false for a NaN or an infinity
}
// The ray of point p[0..3) for pixel key `key` and `sample`: out6 = [p, qh]; six zeros and false for an invalid point.
// d: the unit direction radiance_ray_prepare gives for out6 (written for valid points only) — that function's formula on qh, which is finite and of
// squared length about 1, so its refusals cannot occur; written out on the three values, because the function's loop over an array of six left that
// array in scratch memory in every probe kernel.  tests/native/probe_plan.cpp and the twin hold the two to the same bits.
template <class T>
SPIRA_HD inline bool probe_ray_generate(const T *p, uint32_t sA, uint32_t sB, uint32_t key, uint32_t sample, T out6[6], T d[3]) {
    const bool ok = probe_point_valid<T>(p);             // (an invalid point takes the draw as well and selects zeros at the end: no second exit)
    const CamKey rk = cam_rng_key(sA, sB, key, sample, kProbeBounce);
    T q[3] = {(T)0, (T)0, (T)0};
    for (uint32_t t = 1; t <= kProbeTries; ++t) {
        T u0, u1, u2;
        cam_rng3<T>(rk, t, (T)(1.0 / 1048576.0), u0, u1, u2);
        const T a0 = u0 - (T)1, a1 = u1 - (T)1, a2 = u2 - (T)1;
        if ((a0 * a0 + a1 * a1) + a2 * a2 < (T)1) { q[0] = a0; q[1] = a1; q[2] = a2; break; }
    }
    const T qq = (q[0] * q[0] + q[1] * q[1]) + q[2] * q[2];
    T qh[3] = {(T)0, (T)0, (T)1};
    if (!(qq < CastLimits<T>::min_normal)) {
        T len;
        if constexpr (sizeof(T) == 4) len = __builtin_sqrtf(qq); else len = __builtin_sqrt(qq);
        qh[0] = q[0] / len; qh[1] = q[1] / len; qh[2] = q[2] / len;
    }
    for (int k = 0; k < 3; ++k) { out6[k] = ok ? p[k] : (T)0; out6[3 + k] = ok ? qh[k] : (T)0; }
    if (!ok) return false;
    const T s = (qh[0] * qh[0] + qh[1] * qh[1]) + qh[2] * qh[2];
    T ls;
    if constexpr (sizeof(T) == 4) ls = __builtin_sqrtf(s); else ls = __builtin_sqrt(s);
    d[0] = qh[0] / ls; d[1] = qh[1] / ls; d[2] = qh[2] / ls;
    return true;
}
template <class T>
SPIRA_HD inline bool probe_ray_generate(const T *p, uint32_t sA, uint32_t sB, uint32_t key, uint32_t sample, T out6[6]) {
    T d[3];
    return probe_ray_generate<T>(p, sA, sB, key, sample, out6, d);
}

// The nine real spherical harmonics of bands 0 .. 2 at the unit direction d.
template <class T>
SPIRA_HD inline void sh9_basis(const T d[3], T Y[9]) {
    const T c0 = (T)0.28209479177387814, c1 = (T)0.4886025119029199, c2 = (T)1.0925484305920792, c3 = (T)0.31539156525252005, c4 = (T)0.5462742152960396;
    const T x = d[0], y = d[1], z = d[2];
    Y[0] = c0;
    Y[1] = c1 * y;
    Y[2] = c1 * z;
    Y[3] = c1 * x;
    Y[4] = c2 * (x * y);
    Y[5] = c2 * (y * z);
    Y[6] = c3 * ((T)3 * (z * z) - (T)1);
    Y[7] = c2 * (x * z);
    Y[8] = c4 * (x * x - y * y);
}

}  // namespace spira

#if defined(__HIPCC__)
namespace spira {

// The fields the passes set (run_passes) and the path constants carry GatherArgs' names: the call is the gather's (path_list_call).
template <class T> struct ProbeArgs {
    SceneGlobal<T> scene;
    RenderConst<T> rc;               // sA, sB, flags, max_depth: what trace_segment and the extensions read; the camera and tile fields are unused
    const T *points;                 // n_points x 3
    uint32_t n_points;
    T *sum;                          // n_points x 9 x 3, interleaved [k][j][channel]
    uint8_t *valid;                  // n_points, or NULL
    Pack3<T> *ws;                    // n_points * spp_pass entries, item-major; NULL: spp_pass == 1, the lanes add to sum themselves
    uint32_t key0, sample_first, spp_pass, n_items;      // n_items = n_points * spp_pass <= SPIRA_GATHER_MAX_ITEMS
    FastDiv fd_spp;
    uint32_t write_valid;            // the first pass of a call writes the valid bytes
};

// The point's three values -> the ray of (key, sample): origin and the unit direction radiance_ray_prepare gives for the generated ray.
template <class T>
__device__ __forceinline__ bool probe_load(const T *points, uint32_t point, uint32_t sA, uint32_t sB, uint32_t key, uint32_t sample, Vec<T> &o, Vec<T> &d) {
    const T *pp = points + 3 * (size_t)point;
    T p[3], out6[6], dd[3] = {(T)0, (T)0, (T)1};
#pragma unroll
    for (int k = 0; k < 3; ++k) p[k] = pp[k];
    if (!probe_point_valid<T>(p)) return false;          // (o and d are read for valid points only)
    probe_ray_generate<T>(p, sA, sB, key, sample, out6, dd);
    o = mk<T>(out6[0], out6[1], out6[2]); d = mk<T>(dd[0], dd[1], dd[2]);
    return true;
}

// sum[0..27) += Y_j(d) * L[c]: one product, then one addition, per term.
template <class T>
__device__ __forceinline__ void probe_project(T acc[27], const Vec<T> &d, T Lx, T Ly, T Lz) {
    const T dd[3] = {d.x, d.y, d.z};
    T Y[9];
    sh9_basis<T>(dd, Y);
#pragma unroll
    for (int j = 0; j < 9; ++j) {
        acc[3 * j + 0] = acc[3 * j + 0] + Y[j] * Lx;
        acc[3 * j + 1] = acc[3 * j + 1] + Y[j] * Ly;
        acc[3 * j + 2] = acc[3 * j + 2] + Y[j] * Lz;
    }
}

// Launch bounds: the workgroup size alone, as k_radiance and k_gather — the body is theirs.
template <class T, bool BVH, bool EXT>
__global__ __launch_bounds__(kBlock) void k_probe(const ProbeArgs<T> a) {
    extern __shared__ __attribute__((aligned(32))) unsigned char lds_raw[];
    const SceneLds<T> sc = stage_scene<T>(a.scene, lds_raw);     // the only workgroup barrier of the kernel
    const RenderConst<T> &rc = a.rc;
    const uint32_t stride = gridDim.x * kBlock;
    uint32_t idx = blockIdx.x * kBlock + threadIdx.x;
    bool fresh = true;
    uint32_t point = 0, pixel = 0, sample = 0, b = 0;
    Vec<T> o = mk<T>(0, 0, 0), d = mk<T>(0, 0, 1), d0 = mk<T>(0, 0, 1), beta = mk<T>(1, 1, 1), Lacc = mk<T>(0, 0, 0);
    ExtState<T> ex; ex.flags = rc.flags; ex.bR = 0; ex.bG = 0; ex.bB = 0;
    while (idx < a.n_items) {
        if (fresh) {
            point = fastdiv(idx, a.fd_spp);
            const uint32_t s = idx - point * a.spp_pass;
            pixel = a.key0 + point; sample = a.sample_first + s;
            const bool ok = probe_load<T>(a.points, point, rc.sA, rc.sB, pixel, sample, o, d);
            if (!a.ws && a.valid && a.write_valid) a.valid[point] = ok ? (uint8_t)1 : (uint8_t)0;
            if (!ok) { idx += stride; continue; }                // an invalid point: nothing traced, nothing added (k_probe_sum skips it as well)
            d0 = d;
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
                T *sp = a.sum + 27 * (size_t)point;
                const T dd[3] = {d0.x, d0.y, d0.z};
                T Y[9];
                sh9_basis<T>(dd, Y);
#pragma unroll
                for (int j = 0; j < 9; ++j) {
                    sp[3 * j + 0] = sp[3 * j + 0] + Y[j] * Lacc.x;
                    sp[3 * j + 1] = sp[3 * j + 1] + Y[j] * Lacc.y;
                    sp[3 * j + 2] = sp[3 * j + 2] + Y[j] * Lacc.z;
                    asm volatile("" ::: "memory");               // three sums in flight, not 27: the loads hoisted above the loop cost an occupancy step
                }
            }
            idx += stride;
            fresh = true;
        }
    }
}

// The pass's workspace entries of every valid point, each times the basis at its regenerated direction, added in sample order.
template <class T>
__global__ __launch_bounds__(kBlock) void k_probe_sum(const ProbeArgs<T> a) {
    for (uint32_t k = blockIdx.x * kBlock + threadIdx.x; k < a.n_points; k += gridDim.x * kBlock) {
        const T *pp = a.points + 3 * (size_t)k;
        const T p[3] = {pp[0], pp[1], pp[2]};
        const bool ok = probe_point_valid<T>(p);                 // (validity reads the point only: all samples of a point or none)
        if (a.valid && a.write_valid) a.valid[k] = ok ? (uint8_t)1 : (uint8_t)0;
        if (!ok) continue;
        const Pack3<T> *l = a.ws + (size_t)k * a.spp_pass;
        T *sp = a.sum + 27 * (size_t)k;
        T acc[27];
#pragma unroll
        for (int c = 0; c < 27; ++c) acc[c] = sp[c];
        for (uint32_t s = 0; s < a.spp_pass; ++s) {
            Vec<T> o, d;
            probe_load<T>(a.points, k, a.rc.sA, a.rc.sB, a.key0 + k, a.sample_first + s, o, d);
            const Pack3<T> ls = l[s];
            probe_project<T>(acc, d, ls.x, ls.y, ls.z);
        }
#pragma unroll
        for (int c = 0; c < 27; ++c) sp[c] = acc[c];
    }
}

template <class T> struct ProbeRaysArgs {
    const T *points;                 // n x 3
    T *rays;                         // n x 6
    uint32_t n, sample, sA, sB, key0;
};

template <class T>
__global__ __launch_bounds__(kBlock) void k_probe_rays(const ProbeRaysArgs<T> a) {
    __shared__ T tile[kBlock * 6];
    rays_through_tile<T>(tile, a.rays, a.n, [&](uint32_t k, T out6[6]) {
        const T *pp = a.points + 3 * (size_t)k;
        T p[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) p[c] = pp[c];
        probe_ray_generate<T>(p, a.sA, a.sB, a.key0 + k, a.sample, out6);
    });
}

}  // namespace spira
#endif
