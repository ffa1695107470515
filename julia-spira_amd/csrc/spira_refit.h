// spira_refit.h — refit of a mesh's tree (spira_scene_update_*): the arithmetic that recomputes the triangle records and the node boxes of an existing
// 8-wide BVH (spira_bvh.h) from moved vertices, topology untouched.  No HIP headers: the kernels of spira_hip.hip (k_refit_check / k_refit_tris /
// k_refit_level) and a CPU program (tests/native/refit_plan.cpp) call the very same functions, so the host-array form and the device form of an update
// write the same bytes.  Everything is computed in double, as the builder does, nothing fused (-ffp-contract=off), and every operation used is exactly
// rounded or exact (+ - * /, conversions, floor / ceil, powers of two made from bits): host and device agree bit for bit.
//
// What a refit keeps: the node slots and their order, imask, child_base, tri_base, rank, word 7, the holes, the order of the triangle records, and the
// tree's normalised frame (centre, power-of-two scale) — the frame is fixed at creation, so an update has to stay inside it (the frame rule):
//     |(x - centre_k) * scale| <= 1    for every vertex coordinate x on axis k
// (a fresh build puts the mesh within about +-0.5).  What it rewrites: the three packets of every triangle (and the Float32 screening record where the
// store has one), per node the grid origin, the three grid exponents and the 48 quantised child-box bytes, and the root box of the frame packets.
//
// Padding: the builder's formula (spira_bvh.h, "Padding") with the bound A = max_k |centre_k| + 1 / scale in place of amax — no vertex inside the frame
// has a larger coordinate, so the pad is never smaller than a fresh build's, and it needs no reduction over the mesh.
//
// Boxes between the passes are Float32, rounded outward once (the triangle's padded box); a node's own box is the union of its children's and therefore
// exact in Float32, and its grid origin p is that box's lower corner.
#pragma once
#include <cstdint>

#include "spira_fastdiv.h"      // SPIRA_HD
#include "spira_validate.h"     // magnitude_moderate

namespace spira {

// status bits of refit_check_triangle
constexpr uint32_t kRefitNonFinite = 1u;      // a vertex coordinate is inf / NaN                         -> SPIRA_E_INVALID
constexpr uint32_t kRefitMaterial = 2u;       // material index outside 1 .. n_materials or no integer    -> SPIRA_E_INVALID
constexpr uint32_t kRefitFrame = 4u;          // a vertex leaves the tree's frame                         -> SPIRA_E_LIMIT
constexpr uint32_t kRefitImmoderate = 8u;     // not an error: the mesh is not of "ordinary magnitude" (spira_validate.h, scene_scale_moderate)
constexpr int kRefitMinExp = -120, kRefitMaxExp = 120;      // grid exponents, as the builder's

struct RefitBox { float lo[3], hi[3]; };                                            // normalised frame
template <class T> struct alignas(4 * sizeof(T)) RefitPack4 { T x, y, z, w; };      // one packet of a triangle record / of the frame (16 / 32 bytes)

SPIRA_HD inline uint32_t refit_bits(float f) { uint32_t u; __builtin_memcpy(&u, &f, 4); return u; }
SPIRA_HD inline uint64_t refit_bits(double f) { uint64_t u; __builtin_memcpy(&u, &f, 8); return u; }
SPIRA_HD inline float refit_f32(uint32_t u) { float f; __builtin_memcpy(&f, &u, 4); return f; }
SPIRA_HD inline double refit_f64(uint64_t u) { double f; __builtin_memcpy(&f, &u, 8); return f; }
SPIRA_HD inline double refit_pow2(int e) { return refit_f64((uint64_t)(e + 1023) << 52); }      // -1022 <= e <= 1023

// std::nextafter of a FINITE value towards -inf / +inf (the largest finite value stays where it is, as with nextafter(x, max))
SPIRA_HD inline float refit_below(float f) {
    const uint32_t u = refit_bits(f);
    const uint32_t r = (u << 1) == 0 ? 0x80000001u : (u >> 31) ? u + 1 : u - 1;
    return (r & 0x7F800000u) == 0x7F800000u ? f : refit_f32(r);
}
SPIRA_HD inline float refit_above(float f) {
    const uint32_t u = refit_bits(f);
    const uint32_t r = (u << 1) == 0 ? 0x00000001u : (u >> 31) ? u - 1 : u + 1;
    return (r & 0x7F800000u) == 0x7F800000u ? f : refit_f32(r);
}
SPIRA_HD inline double refit_below(double f) {
    const uint64_t u = refit_bits(f);
    const uint64_t r = (u << 1) == 0 ? 0x8000000000000001ull : (u >> 63) ? u + 1 : u - 1;
    return (r & 0x7FF0000000000000ull) == 0x7FF0000000000000ull ? f : refit_f64(r);
}
SPIRA_HD inline double refit_above(double f) {
    const uint64_t u = refit_bits(f);
    const uint64_t r = (u << 1) == 0 ? 0x0000000000000001ull : (u >> 63) ? u - 1 : u + 1;
    return (r & 0x7FF0000000000000ull) == 0x7FF0000000000000ull ? f : refit_f64(r);
}
// a double as a Float32 that is not above / not below it
SPIRA_HD inline float refit_f32_down(double x) { const float f = (float)x; return (double)f > x ? refit_below(f) : f; }
SPIRA_HD inline float refit_f32_up(double x) { const float f = (float)x; return (double)f < x ? refit_above(f) : f; }

// the pad of every triangle box of a refit, normalised units (see the head of this file)
template <class T> SPIRA_HD inline double refit_pad(const double centre[3], double scale) {
    double cm = 0;
    for (int k = 0; k < 3; ++k) { const double a = centre[k] < 0 ? -centre[k] : centre[k]; cm = a > cm ? a : cm; }
    const double A = cm + 1.0 / scale;
    const double A_n = A * scale;
    return sizeof(T) == 4 ? 1e-4 * (A_n > 1.0 ? A_n : 1.0) : 1e-4 + 1e-9 * A_n;
}

// One triangle of an update (the caller's triangles10 layout) against the rules of spira_scene_update_*: 0 or kRefit* bits.  `frame`: the mesh has a
// tree (more than SPIRA_LDS_TRIANGLES triangles); without one there is no frame to leave.
template <class T> SPIRA_HD inline uint32_t refit_check_triangle(const T *t, uint32_t n_materials, const double centre[3], double scale, bool frame) {
    uint32_t st = 0;
    for (int k = 0; k < 9; ++k) {
        const T x = t[k];
        if (!((x - x) == (T)0)) { st |= kRefitNonFinite; continue; }
        if (frame) {
            const double xn = ((double)x - centre[k % 3]) * scale;
            if (!(xn >= -1.0 && xn <= 1.0)) st |= kRefitFrame;
        }
        if (!magnitude_moderate<T>(x, true)) st |= kRefitImmoderate;
    }
    const T m = t[9];
    if (!(m >= (T)1 && m <= (T)n_materials) || m != (T)__builtin_floor((double)m)) st |= kRefitMaterial;
    return st;
}

template <class T> SPIRA_HD inline T refit_index_bits(uint32_t u);      // bits_to_real of spira_bvh.h
template <> SPIRA_HD inline float refit_index_bits<float>(uint32_t u) { return refit_f32(u); }
template <> SPIRA_HD inline double refit_index_bits<double>(uint32_t u) { return refit_f64((uint64_t)u); }
template <class T> SPIRA_HD inline uint32_t refit_index_of(T w);         // ... and back: the original index kept in tris[3 i].w
template <> SPIRA_HD inline uint32_t refit_index_of<float>(float w) { return refit_bits(w); }
template <> SPIRA_HD inline uint32_t refit_index_of<double>(double w) { return (uint32_t)refit_bits(w); }

// One triangle: t = its ten values in the caller's array, oi = its index there.  out[3]: the record of spira_bvh.h (v0 | index, e1 | material, e2 | 0, the
// edges subtracted in T); out32 (or NULL): the Float32 screening record; box: its padded box in the normalised frame, rounded outward to Float32.
template <class T>
SPIRA_HD inline void refit_triangle(const T *t, uint32_t oi, const double centre[3], double scale, double pad, RefitPack4<T> out[3], RefitPack4<float> *out32, RefitBox &box) {
    const T e1[3] = {(T)(t[3] - t[0]), (T)(t[4] - t[1]), (T)(t[5] - t[2])};
    const T e2[3] = {(T)(t[6] - t[0]), (T)(t[7] - t[1]), (T)(t[8] - t[2])};
    out[0].x = t[0]; out[0].y = t[1]; out[0].z = t[2]; out[0].w = refit_index_bits<T>(oi);
    out[1].x = e1[0]; out[1].y = e1[1]; out[1].z = e1[2]; out[1].w = refit_index_bits<T>((uint32_t)t[9] - 1u);
    out[2].x = e2[0]; out[2].y = e2[1]; out[2].z = e2[2]; out[2].w = (T)0;
    for (int k = 0; k < 3; ++k) {
        const double a = ((double)t[k] - centre[k]) * scale, b = ((double)t[3 + k] - centre[k]) * scale, c = ((double)t[6 + k] - centre[k]) * scale;
        const double bc_mn = c < b ? c : b, bc_mx = c > b ? c : b;
        box.lo[k] = refit_f32_down((bc_mn < a ? bc_mn : a) - pad);
        box.hi[k] = refit_f32_up((bc_mx > a ? bc_mx : a) + pad);
    }
    if (out32) {
        float v[3], f1[3], f2[3], L = 0.0f;
        for (int k = 0; k < 3; ++k) {
            v[k] = (float)(((double)t[k] - centre[k]) * scale);
            f1[k] = (float)((double)e1[k] * scale); f2[k] = (float)((double)e2[k] * scale);
            const float a1 = f1[k] < 0 ? -f1[k] : f1[k], a2 = f2[k] < 0 ? -f2[k] : f2[k], m = a1 > a2 ? a1 : a2;
            L = m > L ? m : L;
        }
        L = refit_above(L);
        out32[0].x = v[0]; out32[0].y = v[1]; out32[0].z = v[2]; out32[0].w = refit_f32(oi);
        out32[1].x = f1[0]; out32[1].y = f1[1]; out32[1].z = f1[2]; out32[1].w = L;
        out32[2].x = f2[0]; out32[2].y = f2[1]; out32[2].z = f2[2]; out32[2].w = 0.0f;
    }
}

// The smallest grid exponent e >= kRefitMinExp with p + 255 * 2^e >= mx (the grid must reach the far side), at most kRefitMaxExp.
SPIRA_HD inline int refit_grid_exp(double p, double mx) {
    int e = kRefitMinExp;
    const double span = mx - p;
    if (span > 0) {
        const int g = (int)((refit_bits(span * (1.0 / 255.0)) >> 52) & 0x7FFu) - 1022;      // a first guess: 2^g > span / 255
        e = g < kRefitMinExp ? kRefitMinExp : g > kRefitMaxExp ? kRefitMaxExp : g;
    }
    while (e > kRefitMinExp && p + 255.0 * refit_pow2(e - 1) >= mx) --e;
    while (e < kRefitMaxExp && p + 255.0 * refit_pow2(e) < mx) ++e;
    return e;
}

SPIRA_HD inline uint32_t refit_child_byte(const uint32_t *w, int plane, int s) { return (w[8 + 2 * plane + (s >> 2)] >> (8 * (s & 3))) & 0xFFu; }

// One node slot: w = its 20 words.  Child s is EMPTY where its x bytes are lo 255, hi 0 (as the builder leaves an absent child, and as this function
// leaves it again); a slot whose eight children are all empty is a hole: nothing is done, false is returned.  Otherwise child s is a node (imask bit s:
// its box is node_boxes[child_base + s], written by the level below) or a leaf (the box of triangle tri_base + rank_s); w[0..3] and w[8..19] are
// rewritten (of w[3] only the three exponent bytes change), `self` is the union of the child boxes.
SPIRA_HD inline bool refit_node(uint32_t *w, const RefitBox *tri_boxes, uint32_t n_tris, const RefitBox *node_boxes, uint32_t n_slots, RefitBox &self) {
    const uint32_t imask = w[3] >> 24, child_base = w[4], tri_base = w[5], rank = w[6];
    RefitBox cb[8];
    uint32_t present = 0;
    for (int k = 0; k < 3; ++k) { self.lo[k] = __builtin_inff(); self.hi[k] = -__builtin_inff(); }
    for (int s = 0; s < 8; ++s) {
        if (refit_child_byte(w, 0, s) == 255u && refit_child_byte(w, 3, s) == 0u) continue;
        if (imask & (1u << s)) {
            const uint32_t idx = child_base + (uint32_t)s;
            if (idx >= n_slots) continue;                       // (cannot happen in a tree the builder made)
            cb[s] = node_boxes[idx];
        } else {
            const uint32_t ti = tri_base + ((rank >> (4 * s)) & 15u);
            if (ti >= n_tris) continue;                         // (likewise)
            cb[s] = tri_boxes[ti];
        }
        present |= 1u << s;
        for (int k = 0; k < 3; ++k) { self.lo[k] = cb[s].lo[k] < self.lo[k] ? cb[s].lo[k] : self.lo[k]; self.hi[k] = cb[s].hi[k] > self.hi[k] ? cb[s].hi[k] : self.hi[k]; }
    }
    if (!present) return false;
    uint32_t q[6][2] = {{0xFFFFFFFFu, 0xFFFFFFFFu}, {0xFFFFFFFFu, 0xFFFFFFFFu}, {0xFFFFFFFFu, 0xFFFFFFFFu}, {0u, 0u}, {0u, 0u}, {0u, 0u}};
    uint32_t eb[3];
    for (int k = 0; k < 3; ++k) {
        const double p = (double)self.lo[k], nmx = (double)self.hi[k];
        const int e = refit_grid_exp(p, nmx);
        eb[k] = (uint32_t)(e + 127);
        const double step = refit_pow2(e), inv = refit_pow2(-e);
        for (int s = 0; s < 8; ++s) {
            if (!(present & (1u << s))) continue;
            const double mn = (double)cb[s].lo[k], mx = (double)cb[s].hi[k];
            double ql = __builtin_floor((mn - p) * inv), qh = __builtin_ceil((mx - p) * inv);
            ql = ql < 0.0 ? 0.0 : ql > 255.0 ? 255.0 : ql; qh = qh < 0.0 ? 0.0 : qh > 255.0 ? 255.0 : qh;
            if (p + ql * step > mn && ql > 0) ql -= 1;
            if (p + qh * step < mx && qh < 255) qh += 1;
            if (p + ql * step > mn || p + qh * step < mx) { ql = 0.0; qh = 255.0; }      // (cannot happen: p <= mn and p + 255 * step >= the node's far side)
            const int sh = 8 * (s & 3);
            q[k][s >> 2] = (q[k][s >> 2] & ~(0xFFu << sh)) | ((uint32_t)ql << sh);
            q[3 + k][s >> 2] |= (uint32_t)qh << sh;
        }
    }
    w[0] = refit_bits(self.lo[0]); w[1] = refit_bits(self.lo[1]); w[2] = refit_bits(self.lo[2]);
    w[3] = eb[0] | (eb[1] << 8) | (eb[2] << 16) | (w[3] & 0xFF000000u);
    for (int a = 0; a < 6; ++a) { w[8 + 2 * a] = q[a][0]; w[9 + 2 * a] = q[a][1]; }
    return true;
}

// The root's box in the caller's coordinates (frame packets 0 and 1): as the builder's, two steps outward in T.
template <class T>
SPIRA_HD inline void refit_root(const RefitBox &b, const double centre[3], double scale, RefitPack4<T> &mn, RefitPack4<T> &mx) {
    T lo[3], hi[3];
    for (int k = 0; k < 3; ++k) {
        const double mnw = (double)b.lo[k] / scale + centre[k], mxw = (double)b.hi[k] / scale + centre[k];
        lo[k] = refit_below(refit_below((T)mnw)); hi[k] = refit_above(refit_above((T)mxw));
    }
    mn.x = lo[0]; mn.y = lo[1]; mn.z = lo[2]; mn.w = (T)0;
    mx.x = hi[0]; mx.y = hi[1]; mx.z = hi[2]; mx.w = (T)0;
}

}  // namespace spira
