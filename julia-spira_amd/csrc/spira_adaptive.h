// spira_adaptive.h — adaptive sampling (spira_render_adaptive_*): the stopping rule and the three kernels that apply it.  Included by spira_hip.hip
// behind spira_device.h, whose device functions (camera ray, closest hit with the in-place BVH walk, shade, scatter, RNG) the refinement kernel is
// built from; k_path and the other render kernels are not touched.  The schedule and the workspace sizes are spira_plan.h's (AdaptivePlan).
//
// Per pixel, all in T, in the written order, nothing fused (-ffp-contract=off):
//   sum = the RGB sums in sample order (what every render entry keeps);  Q = sum over the samples, in order, of y_s * y_s with
//   y_s = (0.2126 r + 0.7152 g) + 0.0722 b, the luminance of sample s.  After n samples:
//       Y   = (0.2126 sum.r + 0.7152 sum.g) + 0.0722 sum.b
//       V   = max(n Q - Y Y, 0)
//       rhs = ((tol (Y + n floor)) (tol (Y + n floor))) (n - 1)
//       converged  <=>  tol > 0 and V <= rhs            (a NaN in V or rhs: not converged)
// which is "standard error of the mean luminance <= tol * (mean + floor)" multiplied through by n^2 (n - 1): no division, no square root.
// n Q - Y Y cancels: its error is about 2^-23 Y Y in Float32 (2^-52 in Float64) against a threshold of about tol^2 Y Y n, harmless for tol >= 1e-3.
// A per-pixel stopping rule biases the estimate slightly downward in noisy pixels (a pixel whose first samples happen to agree stops before it has
// seen its rare bright ones): min_spp is there to bound that.
#pragma once

namespace spira {

template <class T> __host__ __device__ inline T adaptive_luma(T r, T g, T b) { return ((T)0.2126 * r + (T)0.7152 * g) + (T)0.0722 * b; }

// The rule: the one function behind spira_adaptive_converged_* (host) and the kernels below.
template <class T> __host__ __device__ inline bool adaptive_converged(T sr, T sg, T sb, T q, uint32_t n, T tol, T floor) {
    if (!(tol > (T)0)) return false;                       // tolerance 0: every pixel runs to the cap
    const T nn = (T)n;
    const T Y = adaptive_luma<T>(sr, sg, sb);
    const T d = nn * q - Y * Y;
    const T V = d > (T)0 ? d : (T)0;
    const T a = tol * (Y + nn * floor);
    const T rhs = (a * a) * (T)(n - 1);
    return d == d && V <= rhs;
}

// Per-pixel state of an adaptive render (tile-local pixel index) and the rule's constants.
template <class T> struct AdaptiveArgs {
    Pack4<T> *accum;                 // RGB sums (the accumulator of every render entry)
    T *Q;                            // sum of squared sample luminances
    uint32_t *npix;                  // samples taken
    T tol, floor;
    uint32_t cap;                    // spira_params::spp
};

// Append the wave's `active` pixels to a list: ballot + popcount prefix, one vector atomic per wave on the list's length.  Every lane of the wave calls it.
__device__ __forceinline__ void adaptive_append(bool active, uint32_t p, uint32_t *list, uint32_t *count) {
    const unsigned long long m = __ballot(active);
    if (!m) return;                                        // wave-uniform
    const uint32_t lane = threadIdx.x & 63, leader = (uint32_t)__ffsll((long long)m) - 1;
    uint32_t base = 0;
    if (lane == leader) base = atomicAdd(count, (uint32_t)__popcll(m));
    base = __shfl(base, (int)leader);
    if (active) list[base + (uint32_t)__popcll(m & ((1ull << lane) - 1ull))] = p;
}

// Round 0's resolve, in place of k_resolve: accum[p] (+)= the pass's samples of L in sample order (resolve_pixel's statements) and Q[p] (+)= their squared
// luminances; after the last pass of round 0 (`last_pass`: the pixel then has n_after = min_spp samples) the rule is evaluated, the count stored and the
// pixels that go on are compacted into list_out.  Workgroup 0 folds the pass's per-wave statistics like k_resolve.
template <class T>
__global__ __launch_bounds__(kBlock) void k_resolve_adaptive(const Pack3<T> *L, uint32_t tile_pixels, uint32_t k_eff, int first_pass, int last_pass, uint32_t n_after,
                                                             const uint32_t *blk_stats, uint32_t n_rows, Stats *stats, const AdaptiveArgs<T> ad,
                                                             uint32_t *list_out, uint32_t *count_out) {
    for (uint32_t base = blockIdx.x * kBlock; base < tile_pixels; base += gridDim.x * kBlock) {      // (workgroup-uniform bound: whole waves reach the ballot)
        const uint32_t p = base + threadIdx.x;
        bool active = false;
        if (p < tile_pixels) {
            Pack4<T> acc; T q;
            if (first_pass) { acc.x = 0; acc.y = 0; acc.z = 0; acc.w = 0; q = 0; } else { acc = ad.accum[p]; q = ad.Q[p]; }
            uint32_t s = 0;
            for (; s + 8 <= k_eff; s += 8) {
                Pack3<T> l[8];
#pragma unroll
                for (int k = 0; k < 8; ++k) l[k] = L[(size_t)(s + k) * tile_pixels + p];
#pragma unroll
                for (int k = 0; k < 8; ++k) {
                    acc.x = acc.x + l[k].x; acc.y = acc.y + l[k].y; acc.z = acc.z + l[k].z;
                    const T y = adaptive_luma<T>(l[k].x, l[k].y, l[k].z);
                    q = q + y * y;
                }
            }
            for (; s < k_eff; ++s) {
                const Pack3<T> l = L[(size_t)s * tile_pixels + p];
                acc.x = acc.x + l.x; acc.y = acc.y + l.y; acc.z = acc.z + l.z;
                const T y = adaptive_luma<T>(l.x, l.y, l.z);
                q = q + y * y;
            }
            ad.accum[p] = acc; ad.Q[p] = q;
            if (last_pass) {
                ad.npix[p] = n_after;
                active = n_after < ad.cap && !adaptive_converged<T>(acc.x, acc.y, acc.z, q, n_after, ad.tol, ad.floor);
            }
        }
        if (last_pass) adaptive_append(active, p, list_out, count_out);
    }
    if (blockIdx.x == 0 && blk_stats) {
        __shared__ unsigned long long red[4];
        if (threadIdx.x < 4) red[threadIdx.x] = 0;
        __syncthreads();
        unsigned long long seg = 0, enq = 0, rmw = 0, sto = 0;
        for (uint32_t i = threadIdx.x; i < n_rows; i += kBlock) {
            seg += blk_stats[4 * i];
            rmw += blk_stats[4 * i + 1];
            sto += blk_stats[4 * i + 2];
            enq += blk_stats[4 * i + 3];
        }
        for (int sft = 32; sft > 0; sft >>= 1) { seg += __shfl_down(seg, sft); enq += __shfl_down(enq, sft); rmw += __shfl_down(rmw, sft); sto += __shfl_down(sto, sft); }
        if ((threadIdx.x & 63) == 0) { atomicAdd(&red[0], seg); atomicAdd(&red[1], enq); atomicAdd(&red[2], rmw); atomicAdd(&red[3], sto); }
        __syncthreads();
        if (threadIdx.x == 0) { stats->segments += red[0]; stats->rays_enqueued += red[1]; stats->radiance_rmw += red[2]; stats->radiance_store += red[3]; }
    }
}

// Rounds >= 1: `samples` more samples, [sample_first, sample_first + samples), for every pixel of the active list.
// Wave w owns the list entries [w ppw, (w + 1) ppw) and all of their samples, `chunk` at a time: item e of a chunk is sample e % chunk of the wave's pixel
// e / chunk, the items dealt to the lanes e = lane, lane + 64, ...; a lane walks its path to the end in registers (trace_segment: the statements of every
// other organisation, so the sample's bits) and starts its next item at once (k_mega's regeneration), leaving each radiance in the wave's LDS block.  Then
// lane l < ppw adds the chunk's samples of pixel l, in sample order, to its sums and Q — no L buffer, no resolve launch — and after the last chunk evaluates
// the rule and the wave appends its survivors to list_out.  Nothing depends on which wave or lane a pixel falls to, nor on the order of the list.
template <class T> struct RefineArgs {
    SceneGlobal<T> scene;
    RenderConst<T> rc;
    AdaptiveArgs<T> ad;
    const uint32_t *list_in;         // tile-local pixel indices (lr * width + lx, mapped to the global pixel like path_of does)
    uint32_t n_active;
    uint32_t *list_out, *count_out;
    uint32_t sample_first, samples, chunk, ppw;      // ppw * chunk <= kAdaptiveItems, ppw <= 64 (spira_plan.h, AdaptivePlan::round)
    Stats *stats;
};
template <class T, bool BVH>
__global__ __launch_bounds__(kBlock) void k_refine(const RefineArgs<T> a) {
    extern __shared__ __attribute__((aligned(32))) unsigned char lds_raw[];
    const SceneLds<T> sc = stage_scene<T>(a.scene, lds_raw);     // the only workgroup barrier of the kernel
    const RenderConst<T> &rc = a.rc;
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    Pack3<T> *s_L = reinterpret_cast<Pack3<T> *>(lds_raw + scene_lds_bytes<T>(a.scene.n_spheres, a.scene.n_materials, a.scene.n_triangles)) + wave * kAdaptiveItems;
    const unsigned long long e0 = (unsigned long long)(blockIdx.x * (kBlock / 64) + wave) * a.ppw;
    if (e0 >= a.n_active) return;                                // (wave-uniform; behind the barrier)
    const uint32_t first = (uint32_t)e0, n_pix = min(a.ppw, a.n_active - first);
    uint32_t my_p = 0;
    Pack4<T> acc; acc.x = 0; acc.y = 0; acc.z = 0; acc.w = 0;
    T q = 0;
    if (lane < n_pix) { my_p = a.list_in[first + lane]; acc = a.ad.accum[my_p]; q = a.ad.Q[my_p]; }
    unsigned long long nseg = 0;
    for (uint32_t s0 = 0; s0 < a.samples; s0 += a.chunk) {
        const uint32_t ce = min(a.chunk, a.samples - s0), items = n_pix * ce;
        uint32_t e = lane, pixel = 0, sample = 0, b = 0;
        bool fresh = true;
        Vec<T> o = mk<T>(0, 0, 0), d = mk<T>(0, 0, 1), beta = mk<T>(1, 1, 1), Lacc = mk<T>(0, 0, 0);
        while (e < items) {
            if (fresh) {
                const uint32_t pl = e / ce, p = a.list_in[first + pl];
                const uint32_t lr = fastdiv(p, rc.fd_width), lx = p - lr * rc.width;
                const uint32_t pj = ref_row_j(rc, lr), pi = lx + 1;
                pixel = (pj - 1) * rc.width + lx;
                sample = a.sample_first + s0 + (e - pl * ce);
                camera_ray<T>(rc, pi, pj, pixel, sample, o, d);
                beta = mk<T>(1, 1, 1); Lacc = mk<T>(0, 0, 0); b = 0;
                fresh = false;
            }
            Vec<T> contrib; T t_hit;
            SegInfo si = trace_segment<T, BVH, false>(sc, rc, o, d, beta, pixel, sample, b, b + 1 < rc.max_depth, contrib, t_hit);
            ++nseg;
            if (b == 0) { if (si.has_contrib) Lacc = contrib; }
            else if (si.has_contrib) Lacc = Lacc + contrib;
            ++b;
            if (!si.alive || b == rc.max_depth) {
                Pack3<T> l; l.x = Lacc.x; l.y = Lacc.y; l.z = Lacc.z;
                s_L[e] = l;
                e += 64;
                fresh = true;
            }
        }
        wave_lds_sync();
        if (lane < n_pix)
            for (uint32_t k = 0; k < ce; ++k) {
                const Pack3<T> l = s_L[lane * ce + k];
                acc.x = acc.x + l.x; acc.y = acc.y + l.y; acc.z = acc.z + l.z;
                const T y = adaptive_luma<T>(l.x, l.y, l.z);
                q = q + y * y;
            }
        wave_lds_sync();                                         // the next chunk writes the block again
    }
    bool active = false;
    if (lane < n_pix) {
        const uint32_t n_after = a.sample_first + a.samples;
        a.ad.accum[my_p] = acc; a.ad.Q[my_p] = q; a.ad.npix[my_p] = n_after;
        active = n_after < a.ad.cap && !adaptive_converged<T>(acc.x, acc.y, acc.z, q, n_after, a.ad.tol, a.ad.floor);
    }
    adaptive_append(active, my_p, a.list_out, a.count_out);
    for (int sft = 32; sft > 0; sft >>= 1) nseg += __shfl_down(nseg, sft);
    if (lane == 0 && nseg) atomicAdd(&a.stats->segments, nseg);
}

// Finalize with the pixel's own count: out_hdr = sum / n_p (k_finalize's division), the display transform, and the two per-pixel outputs.
template <class T>
__global__ __launch_bounds__(kBlock) void k_finalize_adaptive(const Pack4<T> *accum, const uint32_t *npix, const T *Q, uint32_t tile_pixels, uint32_t post,
                                                              T *out_hdr, T *out_img, uint32_t *out_spp, T *out_q) {
    for (uint32_t p = blockIdx.x * kBlock + threadIdx.x; p < tile_pixels; p += gridDim.x * kBlock) {
        const Pack4<T> acc = accum[p];
        const uint32_t n = npix[p];
        T r = acc.x / (T)n, g = acc.y / (T)n, b = acc.z / (T)n;
        if (out_hdr) { out_hdr[p] = r; out_hdr[tile_pixels + p] = g; out_hdr[2 * (size_t)tile_pixels + p] = b; }
        if (out_img) {
            out_img[p] = post1<T>(r, post); out_img[tile_pixels + p] = post1<T>(g, post);
            out_img[2 * (size_t)tile_pixels + p] = post1<T>(b, post);
        }
        if (out_spp) out_spp[p] = n;
        if (out_q) out_q[p] = Q[p];
    }
}

}  // namespace spira
