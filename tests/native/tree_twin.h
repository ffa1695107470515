// tree_twin.h — the host twins of the library's three ways to give a scene handle a tree, shared by refit_plan.cpp, lbvh_plan.cpp and tree_twin_dump.cpp:
//   create    bvh_build (spira_bvh.h), as scene_upload calls it                                   build / host_build
//   update    spira_scene_update_*: the refit passes of spira_refit.h over the level table          host_refit
//   rebuild   spira_scene_rebuild_*: frame, keys, sort, radix tree, boxes, collapse (spira_lbvh.h)  host_rebuild
// Every twin runs serially through the very functions the kernels call, with std::stable_sort in the place of the device's pair sort (whose result is
// unique).  Compiled with -ffp-contract=off, they write the bytes the device writes: tests/test_gpu_tree_bytes.py compares the two.
// The includer may define CHECK before including this file; otherwise the counting CHECK of the harnesses is defined here.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <numeric>
#include <vector>

#include "../../julia-spira_amd/csrc/spira_bvh.h"
#include "../../julia-spira_amd/csrc/spira_refit.h"
#include "../../julia-spira_amd/csrc/spira_lbvh.h"

#ifndef CHECK
static int g_fail = 0;
#define CHECK(c) do { if (!(c)) { if (g_fail < 50) std::fprintf(stderr, "CHECK failed %s:%d: %s\n", __FILE__, __LINE__, #c); ++g_fail; } } while (0)
#endif

using spira::kBvhNodeDwords;

// ---- a tree as bvh_build leaves it (refit_plan.cpp's view)
template <class T> struct Tree {
    spira::RawVec<uint32_t> nodes;
    spira::RawVec<spira::HostPack4<T>> tris;
    spira::RawVec<spira::HostPack4<float>> tris32;
    spira::BvhFrame<T> fr{};
    T root_mn[3], root_mx[3];
    double centre[3], scale;
    uint32_t n = 0;
};

// ---- what spira_scene_update_* / spira_scene_rebuild_* keep or replace in a handle (lbvh_plan.cpp's view, and the dump's)
template <class T> struct Handle {
    std::vector<uint32_t> nodes;
    std::vector<spira::RefitPack4<T>> tris;
    std::vector<spira::RefitPack4<float>> tris32;
    spira::RefitPack4<T> frame[3];
    std::vector<uint32_t> level_first;
    uint32_t n_slots = 0, n = 0;
    int depth = 0;
    double centre[3] = {0, 0, 0}, scale = 1;
};
template <class T> static bool same(const Handle<T> &a, const Handle<T> &b) {
    return a.nodes == b.nodes && a.tris.size() == b.tris.size() && std::memcmp(a.tris.data(), b.tris.data(), a.tris.size() * sizeof(a.tris[0])) == 0 &&
           std::memcmp(a.frame, b.frame, sizeof a.frame) == 0 && a.level_first == b.level_first && a.n_slots == b.n_slots && a.depth == b.depth &&
           std::memcmp(a.centre, b.centre, sizeof a.centre) == 0 && a.scale == b.scale;
}

static bool slot_child_empty(const uint32_t *w, int s) { return spira::refit_child_byte(w, 0, s) == 255u && spira::refit_child_byte(w, 3, s) == 0u; }
static bool slot_is_hole(const uint32_t *w) { for (int s = 0; s < 8; ++s) if (!slot_child_empty(w, s)) return false; return true; }
static void decode_child(const uint32_t *w, int s, double lo[3], double hi[3], double step[3]) {
    for (int k = 0; k < 3; ++k) {
        step[k] = std::ldexp(1.0, (int)((w[3] >> (8 * k)) & 0xFFu) - 127);
        const double p = (double)spira::bits_float(w[k]);
        lo[k] = p + (double)spira::refit_child_byte(w, k, s) * step[k];
        hi[k] = p + (double)spira::refit_child_byte(w, 3 + k, s) * step[k];
    }
}

// ---- create
template <class T>
static bool build(Tree<T> &tr, const std::vector<T> &tri10, bool screen) {
    tr.n = (uint32_t)(tri10.size() / 10);
    if (!spira::bvh_build<T>(tri10.data(), tr.n, tr.nodes, tr.tris, tr.fr, 1, screen ? &tr.tris32 : nullptr)) return false;
    for (int k = 0; k < 3; ++k) { tr.root_mn[k] = tr.fr.root_mn[k]; tr.root_mx[k] = tr.fr.root_mx[k]; tr.centre[k] = (double)tr.fr.centre[k]; }
    tr.scale = (double)tr.fr.scale;
    return true;
}
template <class T>
static bool host_build(Handle<T> &h, const std::vector<T> &tri10, bool screen) {
    spira::RawVec<uint32_t> nodes; spira::RawVec<spira::HostPack4<T>> tris; spira::RawVec<spira::HostPack4<float>> t32; spira::BvhFrame<T> fr{};
    h.n = (uint32_t)(tri10.size() / 10);
    if (!spira::bvh_build<T>(tri10.data(), h.n, nodes, tris, fr, 1, screen ? &t32 : nullptr)) return false;
    h.nodes.assign(nodes.begin(), nodes.end());
    h.tris.resize(tris.size()); std::memcpy(h.tris.data(), tris.data(), tris.size() * sizeof(tris[0]));
    h.tris32.resize(t32.size()); if (!t32.empty()) std::memcpy(h.tris32.data(), t32.data(), t32.size() * sizeof(t32[0]));
    h.frame[0] = {fr.root_mn[0], fr.root_mn[1], fr.root_mn[2], (T)0}; h.frame[1] = {fr.root_mx[0], fr.root_mx[1], fr.root_mx[2], (T)0};
    h.frame[2] = {fr.centre[0], fr.centre[1], fr.centre[2], fr.scale};
    h.level_first.assign(fr.level_first, fr.level_first + fr.depth + 1);
    h.n_slots = fr.n_slots; h.depth = fr.depth;
    for (int k = 0; k < 3; ++k) h.centre[k] = (double)fr.centre[k];
    h.scale = (double)fr.scale;
    return true;
}

// ---- update.  The host twin of spira_scene_update_*: check every triangle first (nothing is written on a refusal), then the triangle pass and one node
// pass per level, deepest first.  Returns the status bits.  P / P32: the packet types of the caller's arrays (HostPack4 or RefitPack4: the same 4 values).
template <class T, class P, class P32>
static uint32_t host_refit_arrays(uint32_t n, uint32_t n_slots, int depth, const uint32_t *level_first, const double centre[3], double scale, uint32_t *nodes, P *tris, P32 *tris32,
                                  T root_mn[3], T root_mx[3], const std::vector<T> &tri10, uint32_t n_materials) {
    static_assert(sizeof(P) == sizeof(spira::RefitPack4<T>) && sizeof(P32) == sizeof(spira::RefitPack4<float>), "packets of four values");
    uint32_t status = 0;
    for (uint32_t i = 0; i < n; ++i) status |= spira::refit_check_triangle<T>(&tri10[10 * (size_t)i], n_materials, centre, scale, true);
    if (status & (spira::kRefitNonFinite | spira::kRefitMaterial | spira::kRefitFrame)) return status;
    const double pad = spira::refit_pad<T>(centre, scale);
    std::vector<spira::RefitBox> tbox(n), nbox(n_slots);
    for (uint32_t i = 0; i < n; ++i) {
        const uint32_t oi = spira::refit_index_of<T>(tris[3 * (size_t)i].w);
        CHECK(oi < n);
        if (oi >= n) continue;
        spira::RefitPack4<T> out[3]; spira::RefitPack4<float> o32[3];
        spira::refit_triangle<T>(&tri10[10 * (size_t)oi], oi, centre, scale, pad, out, tris32 ? o32 : nullptr, tbox[i]);
        std::memcpy(&tris[3 * (size_t)i], out, sizeof out);
        if (tris32) std::memcpy(&tris32[3 * (size_t)i], o32, sizeof o32);
    }
    for (int d = depth - 1; d >= 0; --d)
        for (uint32_t s = level_first[d]; s < level_first[d + 1]; ++s) {
            uint32_t *w = &nodes[(size_t)s * kBvhNodeDwords];
            if (!spira::refit_node(w, tbox.data(), n, nbox.data(), n_slots, nbox[s])) continue;
            if (s == 0) {
                spira::RefitPack4<T> mn, mx;
                spira::refit_root<T>(nbox[0], centre, scale, mn, mx);
                root_mn[0] = mn.x; root_mn[1] = mn.y; root_mn[2] = mn.z; root_mx[0] = mx.x; root_mx[1] = mx.y; root_mx[2] = mx.z;
            }
        }
    return status;
}
template <class T>
static uint32_t host_refit(Tree<T> &tr, const std::vector<T> &tri10, uint32_t n_materials) {
    return host_refit_arrays<T>(tr.n, tr.fr.n_slots, tr.fr.depth, tr.fr.level_first, tr.centre, tr.scale, tr.nodes.data(), tr.tris.data(),
                                tr.tris32.empty() ? (spira::HostPack4<float> *)nullptr : tr.tris32.data(), tr.root_mn, tr.root_mx, tri10, n_materials);
}
template <class T>
static uint32_t host_refit(Handle<T> &h, const std::vector<T> &tri10, uint32_t n_materials) {
    T mn[3] = {h.frame[0].x, h.frame[0].y, h.frame[0].z}, mx[3] = {h.frame[1].x, h.frame[1].y, h.frame[1].z};
    const uint32_t st = host_refit_arrays<T>(h.n, h.n_slots, h.depth, h.level_first.data(), h.centre, h.scale, h.nodes.data(), h.tris.data(),
                                             h.tris32.empty() ? (spira::RefitPack4<float> *)nullptr : h.tris32.data(), mn, mx, tri10, n_materials);
    h.frame[0] = {mn[0], mn[1], mn[2], (T)0}; h.frame[1] = {mx[0], mx[1], mx[2], (T)0};      // (w is 0 in what the builder and refit_root write alike)
    return st;
}

// ---- identity: a refit with the vertices the tree was built from.  Every decoded child bound within one grid step of the built one, plus the two things a
// refit adds (spira_refit.h): its pad bound A instead of amax, and one outward Float32 rounding of the triangle boxes; the root box of the frame packets
// not inside the built one and no further out than that.  Returns the largest move of a child bound, in grid steps.
template <class T>
static double builder_pad(const std::vector<T> &A, double built_scale) {          // the builder's own pad (spira_bvh.h "Padding")
    double amax = 0;
    for (size_t i = 0; i < A.size() / 10; ++i) for (int k = 0; k < 9; ++k) amax = std::max(amax, std::fabs((double)A[10 * i + k]));
    return sizeof(T) == 4 ? 1e-4 * std::max(1.0, amax * built_scale) : 1e-4 + 1e-9 * amax * built_scale;
}
template <class T>
static double check_identity_bounds(const uint32_t *built_nodes, const uint32_t *ident_nodes, uint32_t n_slots, const T built_mn[3], const T built_mx[3], const T ident_mn[3],
                                    const T ident_mx[3], double built_scale, double pad, double pad_built) {
    const double slack = (pad - pad_built) + std::ldexp(1.0, -23) * std::max(1.0, 1.0 + pad);
    double worst = 0;
    for (uint32_t s = 0; s < n_slots; ++s) {
        const uint32_t *a = &built_nodes[(size_t)s * kBvhNodeDwords], *b = &ident_nodes[(size_t)s * kBvhNodeDwords];
        if (slot_is_hole(a)) continue;
        for (int c = 0; c < 8; ++c) {
            if (slot_child_empty(a, c)) continue;
            double lo0[3], hi0[3], st0[3], lo1[3], hi1[3], st1[3];
            decode_child(a, c, lo0, hi0, st0); decode_child(b, c, lo1, hi1, st1);
            for (int k = 0; k < 3; ++k) {
                const double step = std::max(st0[k], st1[k]);
                CHECK(std::fabs(lo1[k] - lo0[k]) <= step + slack && std::fabs(hi1[k] - hi0[k]) <= step + slack);
                worst = std::max(worst, std::max(std::fabs(lo1[k] - lo0[k]), std::fabs(hi1[k] - hi0[k])) / step);
            }
        }
    }
    for (int k = 0; k < 3; ++k) {          // the root box of the frame packets: not inside the built one, and no further out than pad difference + roundings
        const double tol = slack / built_scale + 8 * std::fabs((double)built_mn[k]) * std::numeric_limits<T>::epsilon();
        CHECK(ident_mn[k] <= built_mn[k] + (T)0 && (double)built_mn[k] - (double)ident_mn[k] <= tol);
        CHECK(ident_mx[k] >= built_mx[k] && (double)ident_mx[k] - (double)built_mx[k] <= tol);
    }
    return worst;
}

// ---- rebuild.  The host twin of spira_scene_rebuild_*: 0, or the status bits / -4 of a refusal.  Everything up to "commit" writes locals (the device's
// scratch) only.
template <class T>
static int host_rebuild(Handle<T> &h, const std::vector<T> &tri10, uint32_t n_materials, int depth_cap) {
    const uint32_t n = h.n;
    const double zero[3] = {0, 0, 0};
    // 1. check and bounds (through the integer codes the device reduces with)
    uint32_t status = 0;
    uint64_t nlo[3] = {0, 0, 0}, ehi[3] = {0, 0, 0};
    for (uint32_t i = 0; i < n; ++i) {
        status |= spira::refit_check_triangle<T>(&tri10[10 * (size_t)i], n_materials, zero, 1.0, false);
        for (int k = 0; k < 9; ++k) {
            const double x = (double)tri10[10 * (size_t)i + k];
            if (!(x == x)) continue;
            nlo[k % 3] = std::max(nlo[k % 3], ~spira::lbvh_enc(x)); ehi[k % 3] = std::max(ehi[k % 3], spira::lbvh_enc(x));
        }
    }
    if (status & (spira::kRefitNonFinite | spira::kRefitMaterial)) return (int)status;
    double lo[3], hi[3], centre[3], scale;
    for (int k = 0; k < 3; ++k) { lo[k] = spira::lbvh_dec(~nlo[k]); hi[k] = spira::lbvh_dec(ehi[k]); }
    spira::lbvh_frame<T>(lo, hi, centre, scale);
    const double pad = spira::refit_pad<T>(centre, scale);
    if (!(pad < 1e12)) return -4;
    // 2. keys, stable sort
    std::vector<uint64_t> key0(n), keys(n);
    std::vector<uint32_t> sorted_idx(n);
    std::vector<spira::RefitBox> leafbox(n);
    for (uint32_t i = 0; i < n; ++i) {
        spira::RefitPack4<T> rec[3];
        spira::refit_triangle<T>(&tri10[10 * (size_t)i], i, centre, scale, pad, rec, nullptr, leafbox[i]);
        key0[i] = spira::lbvh_key<T>(&tri10[10 * (size_t)i], centre, scale);
        CHECK(key0[i] < (1ull << 63));
    }
    std::iota(sorted_idx.begin(), sorted_idx.end(), 0u);
    std::stable_sort(sorted_idx.begin(), sorted_idx.end(), [&](uint32_t a, uint32_t b) { return key0[a] < key0[b]; });
    for (uint32_t j = 0; j < n; ++j) keys[j] = key0[sorted_idx[j]];
    {   // the device's sort — the bitonic network on the padded (key, index) pairs, in the kernels' schedule of tiles and wide passes — gives that very order
        const uint32_t n_pad = spira::lbvh_sort_size(n);
        std::vector<uint64_t> dk(n_pad, ~0ull);
        std::vector<uint32_t> di(n_pad, ~0u);
        for (uint32_t i = 0; i < n; ++i) { dk[i] = key0[i]; di[i] = i; }
        uint32_t launches = 0;
        spira::lbvh_sort_schedule(
            n_pad,
            [&](uint32_t k_first, uint32_t k_last) {
                ++launches;
                for (uint32_t base = 0; base < n_pad; base += spira::kLbvhSortTile)
                    for (uint32_t k = k_first; k <= k_last; k <<= 1)
                        for (uint32_t j = spira::lbvh_tile_first_j(k); j > 0; j >>= 1)
                            for (uint32_t t = 0; t < spira::kLbvhSortTile; ++t) spira::lbvh_bitonic_cx(&dk[base], &di[base], t, base + t, j, k);
            },
            [&](uint32_t j, uint32_t k) { ++launches; for (uint32_t i = 0; i < n_pad; ++i) spira::lbvh_bitonic_cx(dk.data(), di.data(), i, i, j, k); });
        CHECK(launches >= 1);
        for (uint32_t j = 0; j < n; ++j) CHECK(di[j] == sorted_idx[j] && dk[j] == keys[j]);
        for (uint32_t j = n; j < n_pad; ++j) CHECK(di[j] == ~0u && dk[j] == ~0ull);
    }
    // 3. radix tree
    const uint32_t n_inner = n - 1;
    std::vector<int32_t> left(n_inner), right(n_inner), parent(2 * (size_t)n - 1, -2);
    for (uint32_t i = 0; i < n_inner; ++i) {
        spira::lbvh_radix_node(keys.data(), n, i, left[i], right[i]);
        CHECK(left[i] >= 0 && (uint32_t)left[i] < 2 * n - 1 && right[i] >= 0 && (uint32_t)right[i] < 2 * n - 1 && left[i] != right[i]);
        CHECK(parent[left[i]] == -2 && parent[right[i]] == -2);          // every node is somebody's child once
        parent[left[i]] = (int32_t)i; parent[right[i]] = (int32_t)i;
    }
    CHECK(parent[0] == -2);
    parent[0] = -1;
    for (size_t k = 1; k < parent.size(); ++k) CHECK(parent[k] >= 0);
    // 4. boxes, bottom-up with arrival counters (serially: the second arrival at a node is simply the later leaf)
    std::vector<spira::RefitBox> bbox(2 * (size_t)n - 1);
    std::vector<uint32_t> counter(n_inner, 0);
    for (uint32_t j = 0; j < n; ++j) {
        spira::RefitBox b = leafbox[sorted_idx[j]];
        uint32_t cur = n_inner + j;
        for (;;) {
            bbox[cur] = b;
            const int32_t p = parent[cur];
            if (p < 0) break;
            if (counter[p]++ == 0) break;
            const int32_t sib = (uint32_t)left[p] == cur ? right[p] : left[p];
            spira::lbvh_box_union(b, bbox[sib], b);
            cur = (uint32_t)p;
        }
    }
    for (uint32_t i = 0; i < n_inner; ++i) CHECK(counter[i] == 2);
    // 5. collapse, level by level
    std::vector<uint32_t> nodes(kBvhNodeDwords, 0xDEADBEEFu), order(n, 0xFFFFFFFFu), level_first(1, 0u);
    std::vector<spira::LbvhPending> level(1, spira::LbvhPending{0, 0u}), next_level;
    uint32_t slots = 1, n_order = 0;
    int depth = 0;
    while (!level.empty()) {
        ++depth;
        if (depth >= depth_cap) return -4;
        level_first.push_back(slots);
        std::vector<spira::LbvhMade> made(level.size());
        std::vector<uint32_t> cb(level.size()), tb(level.size()), na(level.size());
        uint32_t n_next = 0;
        for (size_t i = 0; i < level.size(); ++i) {
            spira::lbvh_make_node(level[i].bnode, left.data(), right.data(), bbox.data(), n_inner, made[i]);
            uint32_t a, b, c;
            spira::lbvh_node_counts(made[i], a, b, c);
            cb[i] = a ? slots : 0u; tb[i] = n_order; na[i] = n_next;
            slots += a; n_order += b; n_next += c;
        }
        if (slots > spira::kLbvhMaxSlots) return -4;
        nodes.resize((size_t)slots * kBvhNodeDwords, 0xDEADBEEFu);
        next_level.assign(n_next, spira::LbvhPending{-1, 0u});
        for (size_t i = 0; i < level.size(); ++i)
            spira::lbvh_write_node(made[i], level[i].slot, cb[i], tb[i], na[i], n_inner, sorted_idx.data(), nodes.data(), slots, order.data(), n, next_level.data());
        level.swap(next_level);
    }
    CHECK(n_order == n);
    for (uint32_t w : nodes) CHECK(w != 0xDEADBEEFu);          // every word of every slot was written: a node's or a hole's
    // 6. commit and finish: the refit passes over the new level table
    h.nodes = nodes; h.n_slots = slots; h.depth = depth; h.level_first = level_first;
    for (int k = 0; k < 3; ++k) h.centre[k] = centre[k];
    h.scale = scale;
    h.frame[2] = {(T)centre[0], (T)centre[1], (T)centre[2], (T)scale};
    for (uint32_t i = 0; i < n; ++i) h.tris[3 * (size_t)i].w = spira::refit_index_bits<T>(order[i]);
    std::vector<spira::RefitBox> tbox(n), nbox(slots);
    for (uint32_t i = 0; i < n; ++i) {
        const uint32_t oi = spira::refit_index_of<T>(h.tris[3 * (size_t)i].w);
        CHECK(oi < n);
        if (oi >= n) return -99;
        spira::RefitPack4<T> out[3]; spira::RefitPack4<float> o32[3];
        spira::refit_triangle<T>(&tri10[10 * (size_t)oi], oi, centre, scale, pad, out, h.tris32.empty() ? nullptr : o32, tbox[i]);
        std::memcpy(&h.tris[3 * (size_t)i], out, sizeof out);
        if (!h.tris32.empty()) std::memcpy(&h.tris32[3 * (size_t)i], o32, sizeof o32);
    }
    for (int d = depth - 1; d >= 0; --d)
        for (uint32_t s = level_first[d]; s < level_first[d + 1]; ++s) {
            if (!spira::refit_node(&h.nodes[(size_t)s * kBvhNodeDwords], tbox.data(), n, nbox.data(), slots, nbox[s])) continue;
            if (s == 0) spira::refit_root<T>(nbox[0], centre, scale, h.frame[0], h.frame[1]);
        }
    return 0;
}
