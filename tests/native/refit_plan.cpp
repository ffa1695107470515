// refit_plan.cpp — host-only harness built with -fsanitize=address,undefined (tests/test_refit_cpu.py), in the manner of adaptive_plan.cpp: the refit
// arithmetic of spira_refit.h — the very functions k_refit_check / k_refit_tris / k_refit_level call — run on trees that bvh_build made.  A 1 280-triangle
// icosphere and a 900-triangle soup, Float32 and Float64: build, deform (twist + sine, about 0.3 of the extent), refit level by level, then
//   containment  every decoded child box contains the padded bounds of every triangle beneath it; the decoded root box and root_mn / root_mx hold the mesh
//   topology     imask, child_base, tri_base, rank, word 7 and every hole slot are byte-identical to the built tree, the triangle order too
//   identity     a refit with the ORIGINAL vertices: containment again, and every decoded child bound within one grid step of the built one (plus the
//                two things a refit adds: its pad bound A instead of amax, and one outward Float32 rounding of the triangle boxes)
//   refusal      a vertex at normalised 1.5, a NaN coordinate, material index 0: each refused by the shared check, the arrays untouched
//   vacuity      more than half of the deformed triangles leave their old, un-refitted leaf box: a stale tree could not pass the containment check
#include <algorithm>
#include <array>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <map>
#include <random>
#include <utility>
#include <vector>

#include "tree_twin.h"      // Tree, build, host_refit, check_identity_bounds (the twins, shared with tree_twin_dump.cpp), CHECK

// ---- meshes (double; converted to T per run)
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
        for (int k = 0; k < 3; ++k) for (int a = 0; a < 3; ++a) out.push_back(v[f[i][k]][a] + (a == 0 ? 0.3 : a == 2 ? -2.0 : 0.0));      // (off the origin: the frame's centre is not 0)
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
// twist about the vertical axis through the mesh's middle + a sine displacement of 0.3 x the extent
static std::vector<double> deform(const std::vector<double> &tri) {
    double lo[3] = {1e300, 1e300, 1e300}, hi[3] = {-1e300, -1e300, -1e300};
    const size_t n = tri.size() / 10;
    for (size_t i = 0; i < n; ++i) for (int k = 0; k < 9; ++k) { lo[k % 3] = std::min(lo[k % 3], tri[10 * i + k]); hi[k % 3] = std::max(hi[k % 3], tri[10 * i + k]); }
    const double c[3] = {0.5 * (lo[0] + hi[0]), 0.5 * (lo[1] + hi[1]), 0.5 * (lo[2] + hi[2])};
    const double ext = std::max(hi[0] - lo[0], std::max(hi[1] - lo[1], hi[2] - lo[2]));
    std::vector<double> out = tri;
    for (size_t i = 0; i < n; ++i)
        for (int v = 0; v < 3; ++v) {
            double *p = &out[10 * i + 3 * v];
            const double x = p[0] - c[0], y = p[1] - c[1], z = p[2] - c[2];
            const double ang = 2.5 * y / ext * 2.0, cs = std::cos(ang), sn = std::sin(ang);
            p[0] = c[0] + cs * x - sn * z + 0.3 * ext * std::sin(5.0 * y / ext);
            p[1] = c[1] + y + 0.1 * ext * std::sin(7.0 * x / ext);
            p[2] = c[2] + sn * x + cs * z;
        }
    return out;
}

// the levels of BvhFrame: every slot belongs to one level, children of a level-d node lie in level d + 1, the root is level 0
template <class T>
static void check_levels(const Tree<T> &tr) {
    CHECK(tr.fr.depth >= 1 && tr.fr.level_first[0] == 0 && tr.fr.level_first[1] == 1 && tr.fr.level_first[tr.fr.depth] == tr.fr.n_slots);
    for (int d = 0; d < tr.fr.depth; ++d) {
        CHECK(tr.fr.level_first[d] < tr.fr.level_first[d + 1]);
        for (uint32_t s = tr.fr.level_first[d]; s < tr.fr.level_first[d + 1]; ++s) {
            const uint32_t *w = &tr.nodes[(size_t)s * kBvhNodeDwords];
            if (slot_is_hole(w)) continue;
            const uint32_t imask = w[3] >> 24;
            for (int c = 0; c < 8; ++c)
                if (imask & (1u << c)) {
                    CHECK(d + 1 < tr.fr.depth && w[4] + c >= tr.fr.level_first[d + 1] && w[4] + c < tr.fr.level_first[d + 2]);
                    CHECK(!slot_is_hole(&tr.nodes[(size_t)(w[4] + c) * kBvhNodeDwords]));
                }
        }
    }
}

// containment, recursively: returns the (reordered) triangles beneath `slot`; `tb`: exact padded bounds per reordered triangle (6 doubles)
template <class T>
static std::vector<uint32_t> check_contain(const Tree<T> &tr, uint32_t slot, const std::vector<double> &tb, uint64_t &n_checked) {
    const uint32_t *w = &tr.nodes[(size_t)slot * kBvhNodeDwords];
    std::vector<uint32_t> all;
    const uint32_t imask = w[3] >> 24;
    for (int s = 0; s < 8; ++s) {
        if (slot_child_empty(w, s)) { CHECK(!(imask & (1u << s))); continue; }
        std::vector<uint32_t> sub;
        if (imask & (1u << s)) sub = check_contain(tr, w[4] + s, tb, n_checked);
        else sub.push_back(w[5] + ((w[6] >> (4 * s)) & 15u));
        double lo[3], hi[3], st[3];
        decode_child(w, s, lo, hi, st);
        for (uint32_t t : sub)
            for (int k = 0; k < 3; ++k) { CHECK(lo[k] <= tb[6 * (size_t)t + k] && hi[k] >= tb[6 * (size_t)t + 3 + k]); ++n_checked; }
        all.insert(all.end(), sub.begin(), sub.end());
    }
    return all;
}

template <class T>
static std::vector<double> padded_bounds(const Tree<T> &tr, const std::vector<T> &tri10, double pad) {
    std::vector<double> tb(6 * (size_t)tr.n);
    for (uint32_t i = 0; i < tr.n; ++i) {
        const uint32_t oi = spira::refit_index_of<T>(tr.tris[3 * (size_t)i].w);
        for (int k = 0; k < 3; ++k) {
            double mn = 1e300, mx = -1e300;
            for (int v = 0; v < 3; ++v) { const double x = ((double)tri10[10 * (size_t)oi + 3 * v + k] - tr.centre[k]) * tr.scale; mn = std::min(mn, x); mx = std::max(mx, x); }
            tb[6 * (size_t)i + k] = mn - pad; tb[6 * (size_t)i + 3 + k] = mx + pad;
        }
    }
    return tb;
}

template <class T>
static void check_tree(const Tree<T> &tr, const std::vector<T> &tri10, double pad) {
    const std::vector<double> tb = padded_bounds(tr, tri10, pad);
    uint64_t n_checked = 0;
    std::vector<uint32_t> all = check_contain(tr, 0, tb, n_checked);
    CHECK(all.size() == tr.n && n_checked >= 3ull * tr.n);
    std::vector<char> seen(tr.n, 0);
    for (uint32_t t : all) { CHECK(t < tr.n && !seen[t]); if (t < tr.n) seen[t] = 1; }
    // the mesh inside the root box of the frame packets (caller's coordinates), and inside the decoded boxes of the root's children (checked above)
    for (uint32_t i = 0; i < tr.n; ++i)
        for (int k = 0; k < 9; ++k) CHECK(tri10[10 * (size_t)i + k] > tr.root_mn[k % 3] && tri10[10 * (size_t)i + k] < tr.root_mx[k % 3]);
    // the triangle records: what the builder would have written for these vertices
    for (uint32_t i = 0; i < tr.n; ++i) {
        const uint32_t oi = spira::refit_index_of<T>(tr.tris[3 * (size_t)i].w);
        const T *t = &tri10[10 * (size_t)oi];
        const spira::HostPack4<T> *r = &tr.tris[3 * (size_t)i];
        CHECK(r[0].x == t[0] && r[0].y == t[1] && r[0].z == t[2]);
        CHECK(r[1].x == (T)(t[3] - t[0]) && r[1].y == (T)(t[4] - t[1]) && r[1].z == (T)(t[5] - t[2]));
        CHECK(r[2].x == (T)(t[6] - t[0]) && r[2].y == (T)(t[7] - t[1]) && r[2].z == (T)(t[8] - t[2]) && r[2].w == (T)0);
        const T mbits = spira::bits_to_real<T>((uint32_t)t[9] - 1u);
        CHECK(std::memcmp(&r[1].w, &mbits, sizeof(T)) == 0);
    }
}

template <class T>
static void run_mesh(const char *name, const std::vector<double> &mesh_d, bool screen) {
    std::vector<T> A(mesh_d.begin(), mesh_d.end());
    const std::vector<double> Bd = deform(mesh_d);
    std::vector<T> B(Bd.begin(), Bd.end());
    for (size_t i = 0; i < B.size() / 10; ++i) B[10 * i + 9] = (T)(1.0 + (double)((i + 1) % 3));      // the material column changes too
    Tree<T> built;
    if (!build(built, A, screen)) { CHECK(!"bvh_build failed"); return; }
    check_levels(built);
    const uint32_t n = built.n, n_slots = built.fr.n_slots;
    const double pad = spira::refit_pad<T>(built.centre, built.scale);
    // the builder's own pad, for the identity bound (spira_bvh.h "Padding")
    const double pad_built = builder_pad<T>(A, built.scale);
    CHECK(pad >= pad_built);
    check_tree(built, A, pad_built);                       // the harness itself: the built tree passes its own checks

    // ---- vacuity guard: a stale tree would fail — more than half of the deformed triangles leave their old leaf box
    {
        const std::vector<double> tb = padded_bounds(built, B, 0.0);
        uint32_t outside = 0, leaves = 0;
        for (uint32_t s = 0; s < n_slots; ++s) {
            const uint32_t *w = &built.nodes[(size_t)s * kBvhNodeDwords];
            for (int c = 0; c < 8; ++c) {
                if (slot_child_empty(w, c) || ((w[3] >> 24) & (1u << c))) continue;
                const uint32_t t = w[5] + ((w[6] >> (4 * c)) & 15u);
                double lo[3], hi[3], st[3];
                decode_child(w, c, lo, hi, st);
                bool in = true;
                for (int k = 0; k < 3; ++k) in = in && lo[k] <= tb[6 * (size_t)t + k] && hi[k] >= tb[6 * (size_t)t + 3 + k];
                ++leaves; outside += in ? 0 : 1;
            }
        }
        CHECK(leaves == n);
        CHECK(2 * outside > n);
        std::printf("%s %s: %u triangles, %u slots, depth %d, %u of %u deformed triangles outside their old leaf box\n", name, sizeof(T) == 4 ? "f32" : "f64", n, n_slots,
                    built.fr.depth, outside, n);
    }

    // ---- refit to the deformed mesh
    Tree<T> moved = built;
    CHECK(host_refit(moved, B, 3) == 0 || host_refit(moved, B, 3) == spira::kRefitImmoderate);
    check_tree(moved, B, pad);
    if (screen) {
        CHECK(moved.tris32.size() == 3 * (size_t)n);
        // the screening record is what the builder writes for the same vertices in the same frame: compare through a fresh build's formula on triangle 0 .. n-1
        for (uint32_t i = 0; i < n; ++i) {
            const uint32_t oi = spira::refit_index_of<T>(moved.tris[3 * (size_t)i].w);
            const T *t = &B[10 * (size_t)oi];
            const spira::HostPack4<float> *r = &moved.tris32[3 * (size_t)i];
            float L = 0;
            for (int k = 0; k < 3; ++k) {
                CHECK(r[0].x == (float)(((double)t[0] - moved.centre[0]) * moved.scale));
                const float f1 = (float)((double)(T)(t[3 + k] - t[k]) * moved.scale), f2 = (float)((double)(T)(t[6 + k] - t[k]) * moved.scale);
                L = std::max(L, std::max(std::fabs(f1), std::fabs(f2)));
            }
            CHECK(r[1].w == std::nextafter(L, std::numeric_limits<float>::infinity()) && spira::float_bits(r[0].w) == oi);
        }
    }
    // topology: only w[0..2], the exponent bytes of w[3] and w[8..19] of REAL nodes may differ
    for (uint32_t s = 0; s < n_slots; ++s) {
        const uint32_t *a = &built.nodes[(size_t)s * kBvhNodeDwords], *b = &moved.nodes[(size_t)s * kBvhNodeDwords];
        if (slot_is_hole(a)) { CHECK(std::memcmp(a, b, kBvhNodeDwords * 4) == 0); continue; }
        CHECK((a[3] >> 24) == (b[3] >> 24) && a[4] == b[4] && a[5] == b[5] && a[6] == b[6] && a[7] == b[7]);
        for (int c = 0; c < 8; ++c) CHECK(slot_child_empty(a, c) == slot_child_empty(b, c));
    }
    for (uint32_t i = 0; i < n; ++i) CHECK(std::memcmp(&built.tris[3 * (size_t)i].w, &moved.tris[3 * (size_t)i].w, sizeof(T)) == 0);

    // ---- A -> B -> A gives the bytes of A -> A: a refit does not depend on history
    Tree<T> ident = built, back = moved;
    CHECK(host_refit(ident, A, 3) == 0);
    CHECK(host_refit(back, A, 3) == 0);
    CHECK(ident.nodes.size() == back.nodes.size() && std::memcmp(ident.nodes.data(), back.nodes.data(), ident.nodes.size() * 4) == 0);
    CHECK(std::memcmp(ident.tris.data(), back.tris.data(), ident.tris.size() * sizeof(ident.tris[0])) == 0);
    for (int k = 0; k < 3; ++k) CHECK(ident.root_mn[k] == back.root_mn[k] && ident.root_mx[k] == back.root_mx[k]);

    // ---- identity: containment, the records bit for bit, and every child bound within one grid step of the built one (+ the pad difference + one Float32 ulp)
    check_tree(ident, A, pad);
    CHECK(std::memcmp(ident.tris.data(), built.tris.data(), ident.tris.size() * sizeof(ident.tris[0])) == 0);
    const double worst = check_identity_bounds<T>(built.nodes.data(), ident.nodes.data(), n_slots, built.root_mn, built.root_mx, ident.root_mn, ident.root_mx, built.scale, pad, pad_built);
    std::printf("%s %s: identity refit moves a child bound by at most %.3f grid steps\n", name, sizeof(T) == 4 ? "f32" : "f64", worst);

    // ---- refusals: the shared check says no and nothing is written
    {
        Tree<T> t0 = moved;
        auto untouched = [&]() {
            return std::memcmp(t0.nodes.data(), moved.nodes.data(), t0.nodes.size() * 4) == 0 &&
                   std::memcmp(t0.tris.data(), moved.tris.data(), t0.tris.size() * sizeof(t0.tris[0])) == 0 && t0.root_mn[0] == moved.root_mn[0] && t0.root_mx[2] == moved.root_mx[2];
        };
        std::vector<T> bad = A;
        bad[10 * (size_t)(n / 2) + 4] = (T)(moved.centre[1] + 1.5 / moved.scale);            // normalised 1.5 on y
        CHECK((host_refit(t0, bad, 3) & 7u) == spira::kRefitFrame && untouched());
        bad = A; bad[10 * (size_t)(n - 1) + 8] = std::numeric_limits<T>::quiet_NaN();
        CHECK((host_refit(t0, bad, 3) & 7u) == spira::kRefitNonFinite && untouched());
        bad = A; bad[10 * (size_t)3 + 0] = std::numeric_limits<T>::infinity();
        CHECK((host_refit(t0, bad, 3) & spira::kRefitNonFinite) && untouched());
        bad = A; bad[10 * (size_t)7 + 9] = (T)0;
        CHECK((host_refit(t0, bad, 3) & 7u) == spira::kRefitMaterial && untouched());
        bad = A; bad[10 * (size_t)7 + 9] = (T)4;                                             // n_materials = 3
        CHECK((host_refit(t0, bad, 3) & 7u) == spira::kRefitMaterial && untouched());
        bad = A; bad[10 * (size_t)7 + 9] = (T)1.5;
        CHECK((host_refit(t0, bad, 3) & 7u) == spira::kRefitMaterial && untouched());
        // exactly on the frame's edge is still inside; without a tree (`frame` false) nothing can leave it
        T edge[10] = {(T)(moved.centre[0] + 1.0 / moved.scale), (T)moved.centre[1], (T)moved.centre[2], (T)moved.centre[0], (T)moved.centre[1], (T)moved.centre[2],
                      (T)moved.centre[0], (T)moved.centre[1], (T)(moved.centre[2] - 1.0 / moved.scale), (T)1};
        if (((double)edge[0] - moved.centre[0]) * moved.scale <= 1.0 && ((double)edge[8] - moved.centre[2]) * moved.scale >= -1.0) CHECK((spira::refit_check_triangle<T>(edge, 3, moved.centre, moved.scale, true) & 7u) == 0);
        T far_[10] = {(T)1e6, 0, 0, 0, (T)1e6, 0, 0, 0, (T)1e6, (T)2};
        CHECK((spira::refit_check_triangle<T>(far_, 3, moved.centre, moved.scale, false) & 7u) == 0);
        CHECK((spira::refit_check_triangle<T>(far_, 3, moved.centre, moved.scale, true) & 7u) == spira::kRefitFrame);
        T huge[10] = {(T)1e10, 0, 0, 0, 1, 0, 0, 0, 1, (T)2};
        CHECK((spira::refit_check_triangle<T>(huge, 3, moved.centre, moved.scale, false) & spira::kRefitImmoderate) == (sizeof(T) == 4 ? spira::kRefitImmoderate : 0u));
    }
}

static void check_rounding() {
    std::mt19937_64 rng(11);
    const float finf = std::numeric_limits<float>::infinity();
    const double dinf = std::numeric_limits<double>::infinity();
    for (int i = 0; i < 200000; ++i) {
        const uint64_t r = rng();
        float f; uint32_t u = (uint32_t)r; std::memcpy(&f, &u, 4);
        double d; std::memcpy(&d, &r, 8);
        if (i < 8) { const float fs[8] = {0.0f, -0.0f, 1.0f, -1.0f, std::numeric_limits<float>::denorm_min(), -std::numeric_limits<float>::denorm_min(), std::numeric_limits<float>::min(), 0.5f}; f = fs[i]; d = (double)fs[i]; }
        if (std::isfinite(f) && std::fabs(f) < std::numeric_limits<float>::max()) {
            const float a = spira::refit_below(f), b = spira::refit_above(f), ea = std::nextafter(f, -finf), eb = std::nextafter(f, finf);
            CHECK(std::memcmp(&a, &ea, 4) == 0 && std::memcmp(&b, &eb, 4) == 0);
        }
        if (std::isfinite(d) && std::fabs(d) < std::numeric_limits<double>::max()) {
            const double a = spira::refit_below(d), b = spira::refit_above(d), ea = std::nextafter(d, -dinf), eb = std::nextafter(d, dinf);
            CHECK(std::memcmp(&a, &ea, 8) == 0 && std::memcmp(&b, &eb, 8) == 0);
            if (std::fabs(d) < 1e38) {
                const float lo = spira::refit_f32_down(d), hi = spira::refit_f32_up(d);
                CHECK((double)lo <= d && (double)hi >= d && (lo == hi || std::nextafter(lo, finf) == hi));
            }
        }
    }
    CHECK(spira::refit_above(std::numeric_limits<float>::max()) == std::numeric_limits<float>::max());
    CHECK(spira::refit_below(-std::numeric_limits<double>::max()) == -std::numeric_limits<double>::max());
    for (int e = -130; e <= 130; ++e) CHECK(spira::refit_pow2(e) == std::ldexp(1.0, e));
    // the grid exponent: the smallest that reaches the far side
    std::uniform_real_distribution<double> U(-1.0, 1.0);
    for (int i = 0; i < 100000; ++i) {
        const double p = (double)(float)U(rng), mx = p + std::ldexp(std::fabs(U(rng)), (int)(rng() % 40) - 36);
        const int e = spira::refit_grid_exp(p, mx);
        CHECK(e >= -120 && e <= 120 && p + 255.0 * std::ldexp(1.0, e) >= mx);
        CHECK(e == -120 || p + 255.0 * std::ldexp(1.0, e - 1) < mx);
    }
    CHECK(spira::refit_grid_exp(0.25, 0.25) == -120 && spira::refit_grid_exp(0.0, 255.0) == 0 && spira::refit_grid_exp(0.0, 255.5) == 1);
}

int main() {
    check_rounding();
    const std::vector<double> ico = icosphere(3), sp = soup(900, 5);
    if (ico.size() != 12800u) { std::fprintf(stderr, "icosphere(3) has %zu values\n", ico.size()); return 2; }
    run_mesh<float>("icosphere", ico, false);
    run_mesh<double>("icosphere", ico, true);        // (Float64 with the screening records of the SPIRA_BVH_SCREEN build)
    run_mesh<float>("soup", sp, false);
    run_mesh<double>("soup", sp, false);
    if (g_fail) { std::fprintf(stderr, "%d checks failed\n", g_fail); return 1; }
    std::printf("all checks passed\n");
    return 0;
}
