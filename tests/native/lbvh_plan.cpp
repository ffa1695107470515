// lbvh_plan.cpp — host-only harness built with -fsanitize=address,undefined (tests/test_rebuild_cpu.py), in the manner of refit_plan.cpp: the whole pipeline
// of spira_scene_rebuild_* (host_rebuild of tree_twin.h) run serially through the very functions the kernels call (spira_lbvh.h: frame, Morton keys, radix tree, collapse; spira_refit.h:
// records and boxes), with std::stable_sort in the place of the device's radix sort.  Float32 and Float64 on a 1 280-triangle icosphere, a 900-triangle
// soup, 33 triangles (the smallest mesh that gets a tree), 200 copies of one triangle (all keys equal) and a flat 512-triangle grid (one axis without extent):
//   coverage     every original index once in the triangle order; every triangle reached from the root exactly once
//   topology     a consistent level table, holes byte-identical to the builder's, word 7 zero, child_base zero exactly where there is no node child
//   containment  every decoded child box contains the padded bounds of every triangle beneath it; the root box holds the mesh
//   frame        centre and scale equal bvh_build's on the same array, bit for bit
//   refusal      a depth cap given to the level loop makes the collapse refuse, and the handle's arrays are untouched
// and per mesh the surface-area cost of the rebuilt tree over that of bvh_build's tree is printed (the test caps it).
#include <algorithm>
#include <array>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <map>
#include <numeric>
#include <random>
#include <utility>
#include <vector>

#include "tree_twin.h"      // Handle, host_build, host_rebuild (the twins, shared with tree_twin_dump.cpp), CHECK

// ---- meshes (double; converted to T per run).  icosphere and soup are refit_plan.cpp's.
static std::vector<double> icosphere(int level) {
    const double t = (1.0 + std::sqrt(5.0)) / 2.0;
    std::vector<std::array<double, 3>> v = {{-1, t, 0}, {1, t, 0}, {-1, -t, 0}, {1, -t, 0}, {0, -1, t}, {0, 1, t}, {0, -1, -t}, {0, 1, -t}, {t, 0, -1}, {t, 0, 1}, {-t, 0, -1}, {-t, 0, 1}};
    for (auto &p : v) { const double l = std::sqrt(p[0] * p[0] + p[1] * p[1] + p[2] * p[2]); for (double &x : p) x /= l; }
    std::vector<std::array<int, 3>> f = {{0, 11, 5}, {0, 5, 1}, {0, 1, 7}, {0, 7, 10}, {0, 10, 11}, {1, 5, 9}, {5, 11, 4}, {11, 10, 2}, {10, 7, 6}, {7, 1, 8},
                                         {3, 9, 4}, {3, 4, 2}, {3, 2, 6}, {3, 6, 8}, {3, 8, 9}, {4, 9, 5}, {2, 4, 11}, {6, 2, 10}, {8, 6, 7}, {9, 8, 1}};
    for (int l = 0; l < level; ++l) {
        std::map<std::pair<int, int>, int> mid;
        auto midpoint = [&](int a, int b) {
            const auto key = std::make_pair(std::min(a, b), std::max(a, b));
            auto it = mid.find(key);
            if (it != mid.end()) return it->second;
            std::array<double, 3> p = {v[a][0] + v[b][0], v[a][1] + v[b][1], v[a][2] + v[b][2]};
            const double len = std::sqrt(p[0] * p[0] + p[1] * p[1] + p[2] * p[2]);
            for (double &x : p) x /= len;
            v.push_back(p);
            return mid[key] = (int)v.size() - 1;
        };
        std::vector<std::array<int, 3>> g;
        for (auto &tr : f) {
            const int a = midpoint(tr[0], tr[1]), b = midpoint(tr[1], tr[2]), c = midpoint(tr[2], tr[0]);
            g.push_back({tr[0], a, c}); g.push_back({tr[1], b, a}); g.push_back({tr[2], c, b}); g.push_back({a, b, c});
        }
        f.swap(g);
    }
    std::vector<double> out;
    for (size_t i = 0; i < f.size(); ++i) {
        for (int k = 0; k < 3; ++k) for (int a = 0; a < 3; ++a) out.push_back(v[f[i][k]][a] + (a == 0 ? 0.3 : a == 2 ? -2.0 : 0.0));
        out.push_back(1.0 + (double)(i % 3));
    }
    return out;
}
static std::vector<double> soup(uint32_t n, uint64_t seed) {
    std::mt19937_64 rng(seed);
    std::uniform_real_distribution<double> U(-1.0, 1.0);
    std::vector<double> out;
    for (uint32_t i = 0; i < n; ++i) {
        const double c[3] = {U(rng) * 1.5 + 4.0, U(rng), U(rng) * 0.7 - 1.0};
        for (int k = 0; k < 3; ++k) for (int a = 0; a < 3; ++a) out.push_back(c[a] + 0.15 * U(rng));
        out.push_back(1.0 + (double)(i % 3));
    }
    return out;
}
static std::vector<double> copies(uint32_t n) {
    const double t[10] = {0.25, 1.0, -2.0, 1.5, 1.25, -2.5, 0.75, 2.5, -1.75, 2.0};
    std::vector<double> out;
    for (uint32_t i = 0; i < n; ++i) out.insert(out.end(), t, t + 10);
    return out;
}
static std::vector<double> flat_grid(int q) {          // q x q quads, two triangles each, every z equal
    std::vector<double> out;
    for (int j = 0; j < q; ++j)
        for (int i = 0; i < q; ++i) {
            const double x0 = -1.0 + 0.125 * i, x1 = x0 + 0.125, y0 = 0.5 + 0.125 * j, y1 = y0 + 0.125, z = -1.5;
            const double a[10] = {x0, y0, z, x1, y0, z, x1, y1, z, 1.0 + (double)((i + j) % 3)}, b[10] = {x0, y0, z, x1, y1, z, x0, y1, z, 1.0 + (double)((i + 2 * j) % 3)};
            out.insert(out.end(), a, a + 10); out.insert(out.end(), b, b + 10);
        }
    return out;
}

static bool child_empty(const uint32_t *w, int s) { return spira::refit_child_byte(w, 0, s) == 255u && spira::refit_child_byte(w, 3, s) == 0u; }
static bool is_hole_pattern(const uint32_t *w) {
    for (uint32_t k = 0; k < kBvhNodeDwords; ++k) if (w[k] != ((k >= 8 && k < 14) ? 0xFFFFFFFFu : 0u)) return false;
    return true;
}
static void decode_child(const uint32_t *w, int s, double lo[3], double hi[3]) {
    for (int k = 0; k < 3; ++k) {
        const double step = std::ldexp(1.0, (int)((w[3] >> (8 * k)) & 0xFFu) - 127), p = (double)spira::bits_float(w[k]);
        lo[k] = p + (double)spira::refit_child_byte(w, k, s) * step;
        hi[k] = p + (double)spira::refit_child_byte(w, 3 + k, s) * step;
    }
}
static double area(const double lo[3], const double hi[3]) {
    const double e0 = std::max(0.0, hi[0] - lo[0]), e1 = std::max(0.0, hi[1] - lo[1]), e2 = std::max(0.0, hi[2] - lo[2]);
    return e0 * e1 + e1 * e2 + e2 * e0;
}

// coverage + containment + topology of one slot, recursively; returns the (reordered) triangles beneath it.  `level`: the slot's level.
template <class T>
static std::vector<uint32_t> walk(const Handle<T> &h, uint32_t slot, int level, const std::vector<double> &tb, std::vector<char> &slot_seen, double &cost_sum) {
    const uint32_t *w = &h.nodes[(size_t)slot * kBvhNodeDwords];
    std::vector<uint32_t> all;
    CHECK(slot < h.n_slots && !slot_seen[slot]);
    slot_seen[slot] = 1;
    CHECK(level < h.depth && slot >= h.level_first[level] && slot < h.level_first[level + 1]);
    const uint32_t imask = w[3] >> 24;
    uint32_t n_int = 0, n_leaf = 0;
    CHECK(w[7] == 0u);
    for (int s = 0; s < 8; ++s) {
        if (child_empty(w, s)) { CHECK(!(imask & (1u << s))); CHECK(((w[6] >> (4 * s)) & 15u) == 0u); continue; }
        std::vector<uint32_t> sub;
        if (imask & (1u << s)) {
            ++n_int;
            CHECK(w[4] != 0u && w[4] + s < h.n_slots);
            if (w[4] + s < h.n_slots && level + 1 < h.depth) sub = walk(h, w[4] + (uint32_t)s, level + 1, tb, slot_seen, cost_sum);
        } else {
            CHECK(((w[6] >> (4 * s)) & 15u) == n_leaf);          // ranks count the leaf slots in slot order
            ++n_leaf;
            sub.push_back(w[5] + ((w[6] >> (4 * s)) & 15u));
        }
        double lo[3], hi[3];
        decode_child(w, s, lo, hi);
        cost_sum += area(lo, hi);
        for (uint32_t t : sub) { CHECK(t < h.n); if (t < h.n) for (int k = 0; k < 3; ++k) CHECK(lo[k] <= tb[6 * (size_t)t + k] && hi[k] >= tb[6 * (size_t)t + 3 + k]); }
        all.insert(all.end(), sub.begin(), sub.end());
    }
    CHECK(n_int + n_leaf >= 1);
    CHECK((w[4] == 0u) == (n_int == 0u));
    if (n_int) {
        CHECK(w[4] % 8u == 1u);          // blocks of 8 behind the root's slot
        for (int s = 0; s < 8; ++s)
            if (!(imask & (1u << s)) && w[4] + s < h.n_slots) { CHECK(is_hole_pattern(&h.nodes[(size_t)(w[4] + s) * kBvhNodeDwords])); slot_seen[w[4] + s] = 1; }
    }
    return all;
}

// all the checks of one tree; returns its surface-area cost (sum over nodes of child box area over root area)
template <class T>
static double check_tree(const Handle<T> &h, const std::vector<T> &tri10, double pad) {
    const uint32_t n = h.n;
    CHECK(h.depth >= 1 && h.level_first.size() == (size_t)h.depth + 1 && h.level_first[0] == 0 && h.level_first[h.depth] == h.n_slots);
    for (int d = 0; d < h.depth; ++d) CHECK(h.level_first[d] < h.level_first[d + 1]);
    CHECK(h.nodes.size() == (size_t)h.n_slots * kBvhNodeDwords && h.n_slots <= (1u << 24) && h.depth < spira::kBvhStack - 2);
    std::vector<char> seen(n, 0);
    std::vector<double> tb(6 * (size_t)n);
    for (uint32_t i = 0; i < n; ++i) {
        const uint32_t oi = spira::refit_index_of<T>(h.tris[3 * (size_t)i].w);
        CHECK(oi < n && !seen[oi < n ? oi : 0]);
        if (oi >= n) return std::numeric_limits<double>::quiet_NaN();
        seen[oi] = 1;
        for (int k = 0; k < 3; ++k) {
            double mn = 1e300, mx = -1e300;
            for (int v = 0; v < 3; ++v) { const double x = ((double)tri10[10 * (size_t)oi + 3 * v + k] - h.centre[k]) * h.scale; mn = std::min(mn, x); mx = std::max(mx, x); }
            tb[6 * (size_t)i + k] = mn - pad; tb[6 * (size_t)i + 3 + k] = mx + pad;
        }
        const T *t = &tri10[10 * (size_t)oi];
        const spira::RefitPack4<T> *r = &h.tris[3 * (size_t)i];
        CHECK(r[0].x == t[0] && r[0].y == t[1] && r[0].z == t[2] && r[1].x == (T)(t[3] - t[0]) && r[2].z == (T)(t[8] - t[2]) && r[2].w == (T)0);
        CHECK(spira::refit_index_of<T>(r[1].w) == (uint32_t)t[9] - 1u);
    }
    std::vector<char> slot_seen(h.n_slots, 0);
    double cost_sum = 0;
    std::vector<uint32_t> all = walk(h, 0, 0, tb, slot_seen, cost_sum);
    CHECK(all.size() == n);
    std::vector<char> reached(n, 0);
    for (uint32_t t : all) { CHECK(t < n && !reached[t < n ? t : 0]); if (t < n) reached[t] = 1; }
    for (uint32_t s = 0; s < h.n_slots; ++s) CHECK(slot_seen[s]);          // every slot is a reached node or a hole of a reached block
    for (uint32_t i = 0; i < n; ++i)
        for (int k = 0; k < 9; ++k) { const T x = tri10[10 * (size_t)i + k]; CHECK(x > (&h.frame[0].x)[k % 3] && x < (&h.frame[1].x)[k % 3]); }
    CHECK((double)h.frame[2].x == h.centre[0] && (double)h.frame[2].y == h.centre[1] && (double)h.frame[2].z == h.centre[2] && (double)h.frame[2].w == h.scale);
    // root area: the union of the root's decoded child boxes
    double rlo[3] = {1e300, 1e300, 1e300}, rhi[3] = {-1e300, -1e300, -1e300};
    for (int s = 0; s < 8; ++s) {
        if (child_empty(&h.nodes[0], s)) continue;
        double lo[3], hi[3];
        decode_child(&h.nodes[0], s, lo, hi);
        for (int k = 0; k < 3; ++k) { rlo[k] = std::min(rlo[k], lo[k]); rhi[k] = std::max(rhi[k], hi[k]); }
    }
    return cost_sum / area(rlo, rhi);
}

template <class T>
static void run_mesh(const char *name, const std::vector<double> &mesh_d, bool screen) {
    const std::vector<T> A(mesh_d.begin(), mesh_d.end());
    const char *pn = sizeof(T) == 4 ? "f32" : "f64";
    Handle<T> built;
    if (!host_build(built, A, screen)) { CHECK(!"bvh_build failed"); return; }
    double amax = 0;
    for (size_t i = 0; i < A.size(); ++i) if (i % 10 != 9) amax = std::max(amax, std::fabs((double)A[i]));
    const double pad_built = sizeof(T) == 4 ? 1e-4 * std::max(1.0, amax * built.scale) : 1e-4 + 1e-9 * amax * built.scale;
    const double cost_built = check_tree(built, A, 0.0 * pad_built);          // (the builder's own pad is not larger than the refit's: containment of the bare bounds)
    // a handle that holds ANOTHER mesh's tree of the same size: a shifted, scaled copy — the rebuild must not depend on what was there
    std::vector<T> other = A;
    for (size_t i = 0; i < other.size(); ++i) if (i % 10 != 9) other[i] = (T)((double)other[i] * 2.5 + (i % 10 % 3 == 1 ? 7.0 : 0.0));
    Handle<T> h;
    if (!host_build(h, other, screen)) { CHECK(!"bvh_build failed"); return; }
    // ---- refusals leave the handle as it was: the depth cap in the level loop, a NaN, a material index
    {
        const Handle<T> before = h;
        CHECK(host_rebuild(h, A, 3, 2) == -4 && same(h, before));
        std::vector<T> bad = A;
        bad[10 * (size_t)(h.n - 1) + 8] = std::numeric_limits<T>::quiet_NaN();
        CHECK((host_rebuild(h, bad, 3, spira::kLbvhMaxDepth) & (int)spira::kRefitNonFinite) && same(h, before));
        bad = A; bad[10 * (size_t)7 + 9] = (T)0;
        CHECK((host_rebuild(h, bad, 3, spira::kLbvhMaxDepth) & (int)spira::kRefitMaterial) && same(h, before));
    }
    const int rc = host_rebuild(h, A, 3, spira::kLbvhMaxDepth);
    CHECK(rc == 0);
    if (rc) return;
    // ---- frame: bvh_build's, bit for bit
    CHECK(std::memcmp(&h.frame[2], &built.frame[2], sizeof h.frame[2]) == 0);
    for (int k = 0; k < 3; ++k) CHECK(std::memcmp(&h.centre[k], &built.centre[k], 8) == 0);
    CHECK(h.scale == built.scale);
    const double pad = spira::refit_pad<T>(h.centre, h.scale);
    CHECK(pad >= pad_built);
    const double cost = check_tree(h, A, pad);
    // ---- a rebuild does not depend on history: the same array through another handle gives the same bytes
    Handle<T> h2 = built;
    CHECK(host_rebuild(h2, A, 3, spira::kLbvhMaxDepth) == 0 && same(h, h2));
    // ---- and the rebuilt handle is an ordinary one: the slot count and depth are within the walk's limits (checked above)
    std::printf("%s %s: %u triangles, rebuilt %u slots depth %d, built %u slots depth %d, cost ratio %.4f\n", name, pn, h.n, h.n_slots, h.depth, built.n_slots, built.depth,
                cost / cost_built);
}

static void check_pieces() {
    std::mt19937_64 rng(3);
    for (int i = 0; i < 200000; ++i) {
        uint64_t a = rng(), b = rng();
        double x, y; std::memcpy(&x, &a, 8); std::memcpy(&y, &b, 8);
        if (!(x == x) || !(y == y)) continue;
        CHECK(spira::lbvh_dec(spira::lbvh_enc(x)) == x && std::memcmp(&x, &x, 8) == 0);
        if (x < y) CHECK(spira::lbvh_enc(x) < spira::lbvh_enc(y));
        if (x > y) CHECK(spira::lbvh_enc(x) > spira::lbvh_enc(y));
    }
    CHECK(spira::lbvh_enc(-0.0) < spira::lbvh_enc(0.0) && spira::lbvh_enc(-std::numeric_limits<double>::infinity()) < spira::lbvh_enc(-1e308));
    for (uint32_t v : {0u, 1u, 2u, 0x155555u, 0x1FFFFFu, 0xAAAAAu}) {
        uint64_t want = 0;
        for (int b = 0; b < 21; ++b) if (v & (1u << b)) want |= 1ull << (3 * b);
        CHECK(spira::lbvh_expand21(v) == want);
    }
    {   // the sort at sizes with wide passes (more than one tile), many equal keys
        for (uint32_t n : {5000u, 1025u, 4096u}) {
            const uint32_t n_pad = spira::lbvh_sort_size(n);
            std::vector<uint64_t> dk(n_pad, ~0ull); std::vector<uint32_t> di(n_pad, ~0u), want(n);
            for (uint32_t i = 0; i < n; ++i) { dk[i] = (rng() % 97) << 40; di[i] = i; }
            const std::vector<uint64_t> k0(dk.begin(), dk.begin() + n);
            std::iota(want.begin(), want.end(), 0u);
            std::stable_sort(want.begin(), want.end(), [&](uint32_t a, uint32_t b) { return k0[a] < k0[b]; });
            spira::lbvh_sort_schedule(
                n_pad,
                [&](uint32_t k_first, uint32_t k_last) {
                    for (uint32_t base = 0; base < n_pad; base += spira::kLbvhSortTile)
                        for (uint32_t k = k_first; k <= k_last; k <<= 1)
                            for (uint32_t j = spira::lbvh_tile_first_j(k); j > 0; j >>= 1)
                                for (uint32_t t = 0; t < spira::kLbvhSortTile; ++t) spira::lbvh_bitonic_cx(&dk[base], &di[base], t, base + t, j, k);
                },
                [&](uint32_t j, uint32_t k) { for (uint32_t i = 0; i < n_pad; ++i) spira::lbvh_bitonic_cx(dk.data(), di.data(), i, i, j, k); });
            for (uint32_t j = 0; j < n; ++j) CHECK(di[j] == want[j]);
        }
    }
    CHECK(spira::lbvh_quant21(-0.5) == 0u && spira::lbvh_quant21(-7.0) == 0u && spira::lbvh_quant21(0.5) == 2097151u && spira::lbvh_quant21(9.0) == 2097151u && spira::lbvh_quant21(0.0) == 1048576u);
    // frame: frexp by bits against std::frexp over many extents
    std::uniform_real_distribution<double> U(-1.0, 1.0);
    for (int i = 0; i < 100000; ++i) {
        const double c = std::ldexp(U(rng), (int)(rng() % 80) - 40), e = std::ldexp(std::fabs(U(rng)) + 1e-3, (int)(rng() % 300) - 150);
        const double lo[3] = {c - e, c, c - 0.25 * e}, hi[3] = {c + e, c, c + 0.5 * e};
        double ce[3], sc;
        spira::lbvh_frame<double>(lo, hi, ce, sc);
        double ext = 0;
        for (int k = 0; k < 3; ++k) { const double cc = lo[k] * 0.5 + hi[k] * 0.5; CHECK(ce[k] == cc); ext = std::max(ext, std::max(hi[k] - cc, cc - lo[k]) * 2); }
        int e2; std::frexp(ext, &e2);
        CHECK(sc == std::ldexp(1.0, std::max(-1000, std::min(1000, -e2))));
    }
}

int main() {
    check_pieces();
    const std::vector<double> ico = icosphere(3), sp = soup(900, 5), tiny = soup(33, 9), same_tri = copies(200), grid = flat_grid(16);
    if (ico.size() != 12800u || grid.size() != 5120u) { std::fprintf(stderr, "mesh sizes: %zu %zu\n", ico.size(), grid.size()); return 2; }
    run_mesh<float>("icosphere", ico, false);
    run_mesh<double>("icosphere", ico, true);        // (Float64 with the screening records of the SPIRA_BVH_SCREEN build)
    run_mesh<float>("soup", sp, false);
    run_mesh<double>("soup", sp, false);
    run_mesh<float>("tiny33", tiny, false);
    run_mesh<double>("tiny33", tiny, false);
    run_mesh<float>("copies200", same_tri, false);
    run_mesh<double>("copies200", same_tri, false);
    run_mesh<float>("flatgrid", grid, false);
    run_mesh<double>("flatgrid", grid, false);
    if (g_fail) { std::fprintf(stderr, "%d checks failed\n", g_fail); return 1; }
    std::printf("all checks passed\n");
    return 0;
}
