// spira_denoise.h — first-hit feature buffers (spira_render_features_*) and the variance-guided a-trous filter that spends them (spira_denoise_*).
// Included by spira_hip.hip behind spira_device.h, whose device functions (scene staging, camera ray, closest hit with the in-place BVH walk) the
// feature kernel is built from; no render kernel is touched.  Launch and workspace arithmetic: spira_plan.h (features_grid, DenoisePlan).
//
// Features, per pixel: for samples 0 .. spp - 1 the camera ray every render entry takes (RNG key: global pixel, sample, bounce 0) and its closest hit
// (t_min 0.001, later object wins ties, the BVH walk for meshes).  A hit contributes the material's albedo, the `n` of shade_hit (outward for a sphere,
// the unflipped unit geometric normal for a triangle) and t; a miss contributes albedo (1, 1, 1), normal 0, depth 0.  Each output is the sum in sample
// order divided once by (T)spp.
//
// Denoiser, everything in T in the written order, nothing fused (-ffp-contract=off), constants rounded to T once; k = [1/16, 1/4, 3/8, 1/4, 1/16]:
//   prepare   a = albedo + 0.001 (or 1), c = color / a (or color), ya = luma(a) (or 1), v = variance / (ya ya) (or variance)
//   iterate   s = 1 << it.  y_p = luma(c_p); g_p = 3 x 3 blur of v (clamped coordinates, row-major, weights (1/4, 1/2, 1/4)^2), den = (sigma_l sigma_l) g_p + 1e-12;
//             over the 25 taps q = p + s (dx, dy), dy outer, taps outside the image skipped:  w = k[dy + 2] k[dx + 2];
//             depth given: hit = z > 0; hit_p != hit_q -> w = 0; both hit -> normal factor (below), t = max(1 - |z_p - z_q| / (sigma_z max(z_p, z_q)), 0), w = w (t t);
//             depth not given, normal given: the normal factor alone.  Normal factor: e = max((n_p.x n_q.x + n_p.y n_q.y) + n_p.z n_q.z, 0), squared six times, w = w e;
//             variance given: dl = y_p - y_q, t = max(1 - (dl dl) / den, 0), w = w (t t);
//             the centre tap (dx = dy = 0) takes none of the three factors: its w is 9/64 whatever the guides hold, so sw >= 9/64.  (In exact arithmetic its
//             depth and luminance factors are 1 anyway; its normal factor is |n_p|^128, and n_p is a MEAN of unit normals and zeros — at a silhouette
//             pixel it is short, |n|^128 underflows to 0 in Float32, every other tap is cut by the edge, and the pixel would be 0 / 0.)
//             sw += w, sc += w c_q, sv += (w w) v_q;   c'_p = sc / sw, v'_p = sv / (sw sw)
//   finish    out_hdr = c a, out_img = post(out_hdr)   (fused into the last iteration)
// spira_hip/denoise.py restates this in numpy, bit for bit.
#pragma once

namespace spira {

// ------------------------------------------------------------------ feature buffers
template <class T> struct FeatureArgs {
    SceneGlobal<T> scene;
    RenderConst<T> rc;
    T *albedo, *normal, *depth;      // planar rows*width: 3, 3, 1 planes; any may be NULL
};

// the `n` of shade_hit (same operations on the same values)
template <class T, bool BVH, bool TRI>
__device__ __forceinline__ Vec<T> feature_normal(const SceneLds<T> &sc, const Vec<T> pos, int prim, uint32_t slot) {
    if ((!TRI && !BVH) || prim < (int)sc.n_spheres) {
        const Pack4<T> c = sc.sph[prim];
        return normalize(pos - mk<T>(c.x, c.y, c.z));
    } else if (TRI && (!BVH || prim < (int)(sc.n_spheres + sc.n_triangles))) {
        const int ti = prim - (int)sc.n_spheres;
        return mk<T>(sc.tri[3 * ti].w, sc.tri[3 * ti + 1].w, sc.tri[3 * ti + 2].w);
    }
    const Pack4<T> e1p = sc.bvh_tris[3 * (size_t)slot + 1], e2p = sc.bvh_tris[3 * (size_t)slot + 2];
    return normalize(cross(mk<T>(e1p.x, e1p.y, e1p.z), mk<T>(e2p.x, e2p.y, e2p.z)));
}

// One lane per pixel of the tile walks the pixel's samples.  Launches: <T, false, false> spheres alone, <T, false, true> with LDS triangles, <T, true, false> a BVH mesh.
template <class T, bool BVH, bool TRI>
__global__ __launch_bounds__(kBlock) void k_features(const FeatureArgs<T> a) {
    extern __shared__ __attribute__((aligned(32))) unsigned char lds_raw[];
    const SceneLds<T> sc = stage_scene<T>(a.scene, lds_raw);     // the only workgroup barrier of the kernel
    const RenderConst<T> &rc = a.rc;
    const size_t tp = rc.tile_pixels;
    for (uint32_t p = blockIdx.x * kBlock + threadIdx.x; p < rc.tile_pixels; p += gridDim.x * kBlock) {
        const uint32_t lr = fastdiv(p, rc.fd_width), lx = p - lr * rc.width;
        const uint32_t pj = ref_row_j(rc, lr), pi = lx + 1;
        const uint32_t pixel = (pj - 1) * rc.width + lx;
        Vec<T> alb = mk<T>(0, 0, 0), nrm = mk<T>(0, 0, 0);
        T z = 0;
        for (uint32_t s = 0; s < rc.spp; ++s) {
            Vec<T> o, d;
            camera_ray<T>(rc, pi, pj, pixel, s, o, d);
            T t; uint32_t slot;
            ExactDiv exact;
            const int prim = closest_hit<T, BVH, ExactDiv, TRI>(sc, o, d, (T)0.001, t, slot, exact);
            if (prim < 0) { alb = alb + mk<T>(1, 1, 1); continue; }
            const Vec<T> pos = o + d * t;
            const Vec<T> n = feature_normal<T, BVH, TRI>(sc, pos, prim, slot);
            const Pack4<T> ma = sc.mat[2 * material_of<T, BVH, TRI>(sc, prim, slot)];
            alb = alb + mk<T>(ma.x, ma.y, ma.z);
            nrm = nrm + n;
            z = z + t;
        }
        const T nn = (T)rc.spp;
        if (a.albedo) { a.albedo[p] = alb.x / nn; a.albedo[tp + p] = alb.y / nn; a.albedo[2 * tp + p] = alb.z / nn; }
        if (a.normal) { a.normal[p] = nrm.x / nn; a.normal[tp + p] = nrm.y / nn; a.normal[2 * tp + p] = nrm.z / nn; }
        if (a.depth) a.depth[p] = z / nn;
    }
}

// ------------------------------------------------------------------ denoiser
template <class T> struct DenoiseArgs {
    const T *color, *variance, *albedo, *normal, *depth;      // planar, npix values per plane; all but color may be NULL
    Pack4<T> *rec[2];                // ping-pong colour records {c.rgb, v}
    Pack4<T> *guide;                 // {n.xyz, z}; NULL when neither normal nor depth is given
    T *out_hdr, *out_img;
    uint32_t width, height, npix, tiles_x;
    uint32_t post;
    T sigma_l, sigma_z;
};

template <class T>
__global__ __launch_bounds__(kBlock) void k_denoise_prepare(const DenoiseArgs<T> a) {
    const uint32_t p = blockIdx.x * kBlock + threadIdx.x;
    if (p >= a.npix) return;
    const size_t n = a.npix;
    Pack4<T> c;
    c.x = a.color[p]; c.y = a.color[n + p]; c.z = a.color[2 * n + p]; c.w = 0;
    T ya = 1;
    if (a.albedo) {
        const T ar = a.albedo[p] + (T)0.001, ag = a.albedo[n + p] + (T)0.001, ab = a.albedo[2 * n + p] + (T)0.001;
        c.x = c.x / ar; c.y = c.y / ag; c.z = c.z / ab;
        ya = adaptive_luma<T>(ar, ag, ab);
    }
    if (a.variance) c.w = a.albedo ? a.variance[p] / (ya * ya) : a.variance[p];
    a.rec[0][p] = c;
    if (a.guide) {
        Pack4<T> g; g.x = 0; g.y = 0; g.z = 0; g.w = 0;
        if (a.normal) { g.x = a.normal[p]; g.y = a.normal[n + p]; g.z = a.normal[2 * n + p]; }
        if (a.depth) g.w = a.depth[p];
        a.guide[p] = g;
    }
}

template <class T> __device__ __forceinline__ T max0(T x) { return x > (T)0 ? x : (T)0; }

// One a-trous iteration, rec[src] -> rec[src ^ 1]; LAST: -> out_hdr / out_img instead (the finish).  A workgroup covers a tile of 64 x 4 pixels, a wave 64
// contiguous pixels of a row: a tap is one 16- (32-) byte load per record, contiguous across the wave.  No barrier, no atomics, no cross-wave traffic.
template <class T, bool LAST>
__global__ __launch_bounds__(kBlock) void k_denoise_iter(const DenoiseArgs<T> a, uint32_t s, int src) {
    const uint32_t ty = blockIdx.x / a.tiles_x, tx = blockIdx.x - ty * a.tiles_x;
    const uint32_t x = tx * kDenoiseTileW + (threadIdx.x & 63), y = ty * kDenoiseTileH + (threadIdx.x >> 6);
    if (x >= a.width || y >= a.height) return;
    const Pack4<T> *__restrict__ in = a.rec[src];
    const Pack4<T> *__restrict__ gd = a.guide;
    const uint32_t W = a.width, H = a.height;
    const uint32_t p = y * W + x;
    const bool has_var = a.variance != nullptr, has_n = a.normal != nullptr, has_z = a.depth != nullptr;
    const Pack4<T> cp = in[p];
    Pack4<T> gp; gp.x = 0; gp.y = 0; gp.z = 0; gp.w = 0;
    if (gd) gp = gd[p];
    const T yp = adaptive_luma<T>(cp.x, cp.y, cp.z);
    T den = 0;
    if (has_var) {
        const T b3[3] = {(T)0.25, (T)0.5, (T)0.25};
        T g = 0;
#pragma unroll
        for (int j = -1; j <= 1; ++j) {
            const uint32_t yy = (j < 0 && y == 0) ? 0 : (j > 0 && y + 1 == H) ? y : y + j;
#pragma unroll
            for (int i = -1; i <= 1; ++i) {
                const uint32_t xx = (i < 0 && x == 0) ? 0 : (i > 0 && x + 1 == W) ? x : x + i;
                g = g + (b3[j + 1] * b3[i + 1]) * in[yy * W + xx].w;
            }
        }
        den = (a.sigma_l * a.sigma_l) * g + (T)1e-12;
    }
    const T k5[5] = {(T)0.0625, (T)0.25, (T)0.375, (T)0.25, (T)0.0625};
    T sw = 0, sr = 0, sg = 0, sb = 0, sv = 0;
#pragma unroll
    for (int dy = -2; dy <= 2; ++dy) {
        const uint32_t qy = y + (uint32_t)(dy * (int)s);         // (wraps below 0: >= H then)
        if (qy >= H) continue;
#pragma unroll
        for (int dx = -2; dx <= 2; ++dx) {
            const uint32_t qx = x + (uint32_t)(dx * (int)s);
            if (qx >= W) continue;
            const uint32_t q = qy * W + qx;
            const Pack4<T> cq = in[q];
            T w = k5[dy + 2] * k5[dx + 2];
            const bool centre = dx == 0 && dy == 0;              // (compile-time: the loops are unrolled) the centre tap keeps its 9/64
            if (!centre && (has_n || has_z)) {
                const Pack4<T> gq = gd[q];
                bool both = true;
                if (has_z) {
                    const bool hp = gp.w > (T)0, hq = gq.w > (T)0;
                    if (hp != hq) w = 0;
                    both = hp && hq;
                }
                if (both) {
                    if (has_n) {
                        T e = max0<T>((gp.x * gq.x + gp.y * gq.y) + gp.z * gq.z);
                        e = e * e; e = e * e; e = e * e; e = e * e; e = e * e; e = e * e;
                        w = w * e;
                    }
                    if (has_z) {
                        const T zm = gp.w > gq.w ? gp.w : gq.w;
                        const T t = max0<T>((T)1 - abs_t(gp.w - gq.w) / (a.sigma_z * zm));
                        w = w * (t * t);
                    }
                }
            }
            if (!centre && has_var) {
                const T dl = yp - adaptive_luma<T>(cq.x, cq.y, cq.z);
                const T t = max0<T>((T)1 - (dl * dl) / den);
                w = w * (t * t);
            }
            sw = sw + w;
            sr = sr + w * cq.x; sg = sg + w * cq.y; sb = sb + w * cq.z;
            sv = sv + (w * w) * cq.w;
        }
    }
    const T r = sr / sw, g = sg / sw, b = sb / sw;
    if (!LAST) {
        Pack4<T> o; o.x = r; o.y = g; o.z = b; o.w = sv / (sw * sw);
        a.rec[src ^ 1][p] = o;
    } else {
        const size_t n = a.npix;
        T hr = r, hg = g, hb = b;
        if (a.albedo) { hr = r * (a.albedo[p] + (T)0.001); hg = g * (a.albedo[n + p] + (T)0.001); hb = b * (a.albedo[2 * n + p] + (T)0.001); }
        else { hr = r * (T)1; hg = g * (T)1; hb = b * (T)1; }
        if (a.out_hdr) { a.out_hdr[p] = hr; a.out_hdr[n + p] = hg; a.out_hdr[2 * n + p] = hb; }
        if (a.out_img) { a.out_img[p] = post1<T>(hr, a.post); a.out_img[n + p] = post1<T>(hg, a.post); a.out_img[2 * n + p] = post1<T>(hb, a.post); }
    }
}

}  // namespace spira
