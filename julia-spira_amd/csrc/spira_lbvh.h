// spira_lbvh.h — rebuild of a mesh's tree on the device (spira_scene_rebuild_*): the arithmetic that gives a triangle array a NEW frame and a NEW topology
// of the 8-wide BVH of spira_bvh.h.  No HIP headers: the kernels of spira_hip.hip (k_lbvh_*) and a CPU program (tests/native/lbvh_plan.cpp) call the very
// same functions.  Everything is double or integer arithmetic, nothing fused (-ffp-contract=off), every operation exactly rounded or exact: host and device
// agree bit for bit, and nothing here depends on the order in which lanes run.
//
// A rebuild produces only what a refit keeps (spira_refit.h, "What a refit keeps"): the slots and their order, imask, child_base, tri_base, rank, word 7,
// the holes, the order of the triangle records, and the frame.  The refit passes (refit_triangle / refit_node / refit_root) then write every record, every
// quantised box, the grid origins and exponents and the root box.  The steps:
//   frame     centre and power-of-two scale from the exact bounds of all vertices — bvh_build's formula, so a rebuild's frame is a fresh build's
//   keys      63-bit Morton code of the centroid (a + b + c) / 3 in the normalised frame, 21 bits per axis; the (key, original index) pairs sorted: equal keys stay in index order
//   radix     Karras 2012: one binary radix tree node per adjacent pair of sorted keys; equal keys are told apart by their sorted position
//   boxes     leaf box = refit_triangle's padded Float32 box; an inner node's box is the union of its children's (exact in Float32)
//   collapse  the builder's make_node rules, level by level: open the inner entry with the largest box area (the first of equal areas) until 8 entries,
//             slots by the greedy rule on centroid offsets; a prefix sum over the level, in level order, hands out child blocks and triangle positions
// Binary node ids: inner node i of n - 1 is id i (0 = the root), the leaf at sorted position j is id (n - 1) + j.
#pragma once
#include <cstdint>

#include "spira_refit.h"

namespace spira {

constexpr uint32_t kLbvhNodeDwords = 20;            // kBvhNodeDwords of spira_bvh.h (not included here: it is host-only)
constexpr uint32_t kLbvhMaxSlots = 1u << 24;        // a stack entry of the walk holds 24 bits of a child base
constexpr int kLbvhMaxDepth = 64 - 2;               // kBvhStack - 2: a tree this deep (or deeper) is refused

// ---- order-preserving integer code of a double (no NaN): a < b  <=>  lbvh_enc(a) < lbvh_enc(b); -0.0 sorts below +0.0
SPIRA_HD inline uint64_t lbvh_enc(double x) { const uint64_t u = refit_bits(x); return (u >> 63) ? ~u : (u | 0x8000000000000000ull); }
SPIRA_HD inline double lbvh_dec(uint64_t e) { return refit_f64((e >> 63) ? (e & 0x7FFFFFFFFFFFFFFFull) : ~e); }

// ---- frame: centre and power-of-two scale (spira_bvh.h, "frame: centre and power-of-two scale": halves first, frexp, the emax clamp)
template <class T> SPIRA_HD inline void lbvh_frame(const double lo[3], const double hi[3], double centre[3], double &scale) {
    double ext = 0;
    for (int k = 0; k < 3; ++k) {
        centre[k] = (double)(T)(lo[k] * 0.5 + hi[k] * 0.5);
        const double a = hi[k] - centre[k], b = centre[k] - lo[k];
        const double e = (a < b ? b : a) * 2;
        ext = ext < e ? e : ext;
    }
    const int emax = sizeof(T) == 8 ? 1000 : 120;
    const bool finite = (ext - ext) == 0;
    int se = 0;
    if (ext > 0 && finite) {
        const int field = (int)((refit_bits(ext) >> 52) & 0x7FFu);
        const int e2 = field ? field - 1022 : -1022;          // frexp's exponent (a subnormal's is below -1022: clamped either way)
        se = -e2 < -emax ? -emax : -e2 > emax ? emax : -e2;
    } else if (!finite) se = -emax;
    scale = refit_pow2(se);
}

// ---- Morton key of one triangle (the caller's triangles10 layout)
SPIRA_HD inline uint64_t lbvh_expand21(uint32_t v) {
    uint64_t x = v & 0x1FFFFFu;
    x = (x | x << 32) & 0x001F00000000FFFFull;
    x = (x | x << 16) & 0x001F0000FF0000FFull;
    x = (x | x << 8) & 0x100F00F00F00F00Full;
    x = (x | x << 4) & 0x10C30C30C30C30C3ull;
    x = (x | x << 2) & 0x1249249249249249ull;
    return x;
}
SPIRA_HD inline uint32_t lbvh_quant21(double c) {          // a fresh frame holds the mesh within about +-0.5
    double x = (c + 0.5) * 2097152.0;
    if (!(x >= 0.0)) x = 0.0;
    if (x > 2097151.0) x = 2097151.0;
    return (uint32_t)x;
}
template <class T> SPIRA_HD inline uint64_t lbvh_key(const T *t, const double centre[3], double scale) {
    uint32_t q[3];
    for (int k = 0; k < 3; ++k) {
        const double a = ((double)t[k] - centre[k]) * scale, b = ((double)t[3 + k] - centre[k]) * scale, c = ((double)t[6 + k] - centre[k]) * scale;
        q[k] = lbvh_quant21((a + b + c) / 3.0);
    }
    return (lbvh_expand21(q[0]) << 2) | (lbvh_expand21(q[1]) << 1) | lbvh_expand21(q[2]);
}

// ---- the sort: a bitonic network over the (key, original index) PAIRS, compared lexicographically.  The pairs are all different, so the sorted order is
// unique — equal keys end up in index order, as a stable sort of the keys alone would leave them — and it does not depend on how the network is scheduled.
// The array is padded to a power of two (at least kLbvhSortTile) with pairs that sort last (key ~0: a real key has 63 bits).
constexpr uint32_t kLbvhSortTile = 1024;
SPIRA_HD inline uint32_t lbvh_sort_size(uint32_t n) { uint32_t p = kLbvhSortTile; while (p < n) p <<= 1; return p; }
SPIRA_HD inline bool lbvh_pair_less(uint64_t ka, uint32_t ia, uint64_t kb, uint32_t ib) { return ka < kb || (ka == kb && ia < ib); }
// one compare-exchange: element i of keys / idx with its partner i ^ j (done by the lower of the two); gi = i's position in the whole array (it decides the
// direction of stage k) — keys / idx may be a tile of the array held elsewhere, aligned to more than j
SPIRA_HD inline void lbvh_bitonic_cx(uint64_t *keys, uint32_t *idx, uint32_t i, uint32_t gi, uint32_t j, uint32_t k) {
    const uint32_t l = i ^ j;
    if (l <= i) return;
    const uint64_t ka = keys[i], kb = keys[l];
    const uint32_t ia = idx[i], ib = idx[l];
    const bool up = (gi & k) == 0;
    if (up ? lbvh_pair_less(kb, ib, ka, ia) : lbvh_pair_less(ka, ia, kb, ib)) { keys[i] = kb; keys[l] = ka; idx[i] = ib; idx[l] = ia; }
}
// the schedule: stages k = 2, 4, .. n_pad, each with passes j = k/2 .. 1.  Passes with j < kLbvhSortTile stay inside aligned tiles of kLbvhSortTile elements:
// `tile(k_first, k_last)` runs, per tile, every such pass of stages k_first .. k_last; `wide(j, k)` is one pass over the whole array.
template <class Tile, class Wide> inline void lbvh_sort_schedule(uint32_t n_pad, Tile tile, Wide wide) {
    tile(2u, kLbvhSortTile < n_pad ? kLbvhSortTile : n_pad);
    for (uint32_t k = 2 * kLbvhSortTile; k <= n_pad && k != 0; k <<= 1) {
        for (uint32_t j = k >> 1; j >= kLbvhSortTile; j >>= 1) wide(j, k);
        tile(k, k);
    }
}
// the first pass of stage k that stays inside a tile
SPIRA_HD inline uint32_t lbvh_tile_first_j(uint32_t k) { return (k >> 1) < kLbvhSortTile ? (k >> 1) : (kLbvhSortTile >> 1); }

// ---- binary radix tree over the sorted keys (Karras 2012)
// length of the common prefix of sorted positions i and j; equal keys: 64 + that of the positions themselves; j outside the array: -1
SPIRA_HD inline int lbvh_delta(const uint64_t *keys, uint32_t n, int64_t i, int64_t j) {
    if (j < 0 || j >= (int64_t)n) return -1;
    const uint64_t a = keys[i], b = keys[j];
    if (a != b) return __builtin_clzll(a ^ b);
    return 64 + __builtin_clz((uint32_t)i ^ (uint32_t)j);      // (i != j wherever this is called)
}
// inner node i < n - 1 (n >= 2): the ids of its two children
SPIRA_HD inline void lbvh_radix_node(const uint64_t *keys, uint32_t n, uint32_t i, int32_t &left, int32_t &right) {
    const int64_t ii = (int64_t)i;
    const int64_t d = lbvh_delta(keys, n, ii, ii + 1) > lbvh_delta(keys, n, ii, ii - 1) ? 1 : -1;
    const int dmin = lbvh_delta(keys, n, ii, ii - d);
    int64_t lmax = 2;
    while (lbvh_delta(keys, n, ii, ii + lmax * d) > dmin) lmax *= 2;
    int64_t l = 0;
    for (int64_t t = lmax / 2; t >= 1; t /= 2)
        if (lbvh_delta(keys, n, ii, ii + (l + t) * d) > dmin) l += t;
    const int64_t j = ii + l * d;
    const int dnode = lbvh_delta(keys, n, ii, j);
    int64_t s = 0, t = l;
    do {
        t = (t + 1) >> 1;
        if (lbvh_delta(keys, n, ii, ii + (s + t) * d) > dnode) s += t;
    } while (t > 1);
    const int64_t gamma = ii + s * d + (d < 0 ? -1 : 0);
    const int64_t first = ii < j ? ii : j, last = ii < j ? j : ii;
    left = (int32_t)(first == gamma ? (int64_t)(n - 1) + gamma : gamma);
    right = (int32_t)(last == gamma + 1 ? (int64_t)(n - 1) + gamma + 1 : gamma + 1);
}

SPIRA_HD inline void lbvh_box_union(const RefitBox &a, const RefitBox &b, RefitBox &u) {
    for (int k = 0; k < 3; ++k) { u.lo[k] = a.lo[k] < b.lo[k] ? a.lo[k] : b.lo[k]; u.hi[k] = a.hi[k] > b.hi[k] ? a.hi[k] : b.hi[k]; }
}

// ---- collapse: one 8-wide node out of the binary node `bnode` (the rules of bvh_build's make_node)
struct LbvhPending { int32_t bnode; uint32_t slot; };
struct LbvhMade { int32_t ent_at[8]; uint32_t imask, n_int, n_leaf, rank; };      // ent_at[s]: the binary node in child slot s, or -1

SPIRA_HD inline double lbvh_area(const RefitBox &b) {
    const double d0 = (double)b.hi[0] - (double)b.lo[0], d1 = (double)b.hi[1] - (double)b.lo[1], d2 = (double)b.hi[2] - (double)b.lo[2];
    const double e0 = d0 > 0 ? d0 : 0, e1 = d1 > 0 ? d1 : 0, e2 = d2 > 0 ? d2 : 0;
    return e0 * e1 + e1 * e2 + e2 * e0;
}

// n_inner = n - 1: ids below it are inner nodes.  left / right: the children of the inner nodes; box: one per binary node id.
SPIRA_HD inline void lbvh_make_node(int32_t bnode, const int32_t *left, const int32_t *right, const RefitBox *box, uint32_t n_inner, LbvhMade &m) {
    int32_t ent[8];
    int ne = 0;
    if ((uint32_t)bnode >= n_inner) ent[ne++] = bnode;
    else { ent[ne++] = left[bnode]; ent[ne++] = right[bnode]; }
    while (ne < 8) {          // open the inner entry with the largest box; the first of equal areas
        int pick = -1;
        double pa = -1;
        for (int i = 0; i < ne; ++i)
            if ((uint32_t)ent[i] < n_inner) { const double a = lbvh_area(box[ent[i]]); if (a > pa) { pa = a; pick = i; } }
        if (pick < 0) break;
        const int32_t o = ent[pick];
        ent[pick] = left[o]; ent[ne++] = right[o];
    }
    double nmn[3], nmx[3], off[8][3];
    for (int k = 0; k < 3; ++k) { nmn[k] = __builtin_inf(); nmx[k] = -__builtin_inf(); }
    for (int i = 0; i < ne; ++i)
        for (int k = 0; k < 3; ++k) {
            const double lo = (double)box[ent[i]].lo[k], hi = (double)box[ent[i]].hi[k];
            nmn[k] = lo < nmn[k] ? lo : nmn[k]; nmx[k] = hi > nmx[k] ? hi : nmx[k];
        }
    for (int i = 0; i < ne; ++i)
        for (int k = 0; k < 3; ++k) off[i][k] = 0.5 * ((double)box[ent[i]].lo[k] + (double)box[ent[i]].hi[k]) - 0.5 * (nmn[k] + nmx[k]);
    // greedy slot assignment: slot bit k set <=> the child sits on the positive side along axis k
    uint32_t slot_used = 0, ent_done = 0;
    for (int s = 0; s < 8; ++s) m.ent_at[s] = -1;
    for (int round = 0; round < ne; ++round) {
        double bestc = -__builtin_inf();
        int bi = -1, bs = -1;
        for (int i = 0; i < ne; ++i) {
            if (ent_done & (1u << i)) continue;
            for (int s = 0; s < 8; ++s) {
                if (slot_used & (1u << s)) continue;
                const double c = ((s & 1) ? off[i][0] : -off[i][0]) + ((s & 2) ? off[i][1] : -off[i][1]) + ((s & 4) ? off[i][2] : -off[i][2]);
                if (c > bestc || bi < 0) { bestc = c; bi = i; bs = s; }
            }
        }
        ent_done |= 1u << bi; slot_used |= 1u << bs; m.ent_at[bs] = ent[bi];
    }
    m.imask = 0; m.n_int = 0; m.n_leaf = 0; m.rank = 0;
    for (int s = 0; s < 8; ++s) {
        if (m.ent_at[s] < 0) continue;
        if ((uint32_t)m.ent_at[s] < n_inner) { m.imask |= 1u << s; ++m.n_int; }
        else { m.rank |= m.n_leaf << (4 * s); ++m.n_leaf; }
    }
}

// what one node adds to the three running sums of its level (the prefix sum is taken in level order): slots, triangle positions, next level's nodes
SPIRA_HD inline void lbvh_node_counts(const LbvhMade &m, uint32_t &slots, uint32_t &tris, uint32_t &next) { slots = m.n_int ? 8u : 0u; tris = m.n_leaf; next = m.n_int; }

SPIRA_HD inline void lbvh_write_hole(uint32_t *h) {          // as the builder writes an unused slot: empty children, so that a stray visit finds nothing
    for (uint32_t k = 0; k < kLbvhNodeDwords; ++k) h[k] = 0u;
    for (uint32_t k = 8; k < 14; ++k) h[k] = 0xFFFFFFFFu;
}

// The node's slot, the holes of its child block, its leaves' places in the triangle order and its inner children's entries in the next level's list.
// child_base: the block of 8 slots (0: the node has no node child); tri_base / next_at: this node's share of the level's prefix sums.  Present children get
// NON-EMPTY placeholder bytes (lo 0, hi 255), absent ones lo 255 / hi 0: refit_node tells them apart by exactly that and writes the real boxes.
// `cap_slots` / `n` bound every store (a consistent input never reaches them).
SPIRA_HD inline void lbvh_write_node(const LbvhMade &m, uint32_t slot, uint32_t child_base, uint32_t tri_base, uint32_t next_at, uint32_t n_inner, const uint32_t *sorted_idx,
                                     uint32_t *nodes, uint32_t cap_slots, uint32_t *order, uint32_t n, LbvhPending *next_level) {
    uint32_t lo[2] = {0xFFFFFFFFu, 0xFFFFFFFFu}, hi[2] = {0u, 0u}, t = 0, at = next_at;
    for (int s = 0; s < 8; ++s) {
        const int32_t e = m.ent_at[s];
        if (e < 0) continue;
        const int sh = 8 * (s & 3);
        lo[s >> 2] &= ~(0xFFu << sh); hi[s >> 2] |= 0xFFu << sh;
        if (m.imask & (1u << s)) { if (at < n) next_level[at] = {e, child_base + (uint32_t)s}; ++at; }
        else { if (tri_base + t < n) order[tri_base + t] = sorted_idx[(uint32_t)e - n_inner]; ++t; }
    }
    if (m.n_int)
        for (uint32_t s = 0; s < 8; ++s)
            if (!(m.imask & (1u << s)) && child_base + s < cap_slots) lbvh_write_hole(nodes + (size_t)(child_base + s) * kLbvhNodeDwords);
    if (slot >= cap_slots) return;
    uint32_t *w = nodes + (size_t)slot * kLbvhNodeDwords;
    w[0] = w[1] = w[2] = 0u;
    w[3] = m.imask << 24; w[4] = child_base; w[5] = tri_base; w[6] = m.rank; w[7] = 0u;
    for (int a = 0; a < 3; ++a) { w[8 + 2 * a] = lo[0]; w[9 + 2 * a] = lo[1]; w[14 + 2 * a] = hi[0]; w[15 + 2 * a] = hi[1]; }
}

}  // namespace spira
