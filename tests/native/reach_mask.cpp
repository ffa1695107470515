// reach_mask.cpp — host-only harness built with -fsanitize=address,undefined (tests/test_reach_mask_cpu.py), next to sky_cull.cpp: the per-sphere
// reach mask of the pixel-owning passes (csrc/spira_sky.h, pixel_reach) against the sphere scan's own discriminant.  For every CLEAR bit of a
// pixel's mask, every checked camera ray of the pixel — the four corner jitters (0 and 1 - 2^-21 in each axis) and 16 random ones — must have
// disc < 0 for that sphere, disc being the statements of closest_hit_local (csrc/spira_device.h; examples/julia-raytracer.jl:114-118) on the camera ray
// of :398-399 and :303, restated here in Float64 in the written order (-ffp-contract=off).  On every input sky_pixel must answer as the function
// it replaced does (kept here verbatim), whatever the number of spheres.  The plan's two fields (csrc/spira_plan.h) are checked at the end.
//
// usage: reach_mask <file>     the file holds the S1 scene as the library hands it out: 12 camera values, then 5 values per sphere ("%la" each)
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <random>
#include <vector>

#include "../../julia-spira_amd/csrc/spira_sky.h"
#include "../../julia-spira_amd/csrc/spira_plan.h"

static int g_fail = 0;
#define CHECK(c) do { if (!(c)) { if (g_fail < 20) std::fprintf(stderr, "CHECK failed %s:%d: %s\n", __FILE__, __LINE__, #c); ++g_fail; } } while (0)

// ---- sky_pixel as it was before pixel_reach existed, verbatim
namespace parent {
inline bool sky_pixel(const double *cam, uint32_t W, uint32_t H, uint32_t i, uint32_t j, const double *spheres5, uint32_t n_spheres) {
    const double kSlack = 1.0 / 1048576.0, kHuge = 1.0e100, kTiny = 1.0e-100;
    const double w1 = (double)W - 1.0, h1 = (double)H - 1.0;
    const double uc = ((double)i - 0.5) / w1, vc = ((double)j - 0.5) / h1;
    const double hn = __builtin_sqrt((cam[6] * cam[6] + cam[7] * cam[7]) + cam[8] * cam[8]);
    const double vn = __builtin_sqrt((cam[9] * cam[9] + cam[10] * cam[10]) + cam[11] * cam[11]);
    const double rho = (0.5 * (hn / w1 + vn / h1)) * (1.0 + kSlack);
    const double dx = ((cam[3] + cam[6] * uc) + cam[9] * vc) - cam[0];
    const double dy = ((cam[4] + cam[7] * uc) + cam[10] * vc) - cam[1];
    const double dz = ((cam[5] + cam[8] * uc) + cam[11] * vc) - cam[2];
    const double dd = (dx * dx + dy * dy) + dz * dz, dn = __builtin_sqrt(dd);
    if (!(rho >= 0.0 && dn > rho && dn > kTiny && dn < kHuge)) return false;
    const double q = __builtin_sqrt(dd - rho * rho);                 // |Dc| cos delta
    for (uint32_t s = 0; s < n_spheres; ++s) {
        const double *sp = spheres5 + 5 * (uint64_t)s;
        const double r = sp[3];
        const double cx = sp[0] - cam[0], cy = sp[1] - cam[1], cz = sp[2] - cam[2];
        const double cn = __builtin_sqrt((cx * cx + cy * cy) + cz * cz);
        const double xx = cy * dz - cz * dy, xy = cz * dx - cx * dz, xz = cx * dy - cy * dx;
        const double xn = __builtin_sqrt((xx * xx + xy * xy) + xz * xz);
        const double cd = __builtin_fabs((cx * dx + cy * dy) + cz * dz);
        if (!(r > 0.0 && r < kHuge && cn > kTiny && cn < kHuge)) return false;
        if (!(xn * q - cd * rho > (r * (1.0 + kSlack) + cn * kSlack) * dd)) return false;
    }
    return true;
}
}  // namespace parent

struct V { double x, y, z; };
static V operator+(V a, V b) { return {a.x + b.x, a.y + b.y, a.z + b.z}; }
static V operator-(V a, V b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
static V operator*(V a, double s) { return {a.x * s, a.y * s, a.z * s}; }
static V operator/(V a, double s) { return {a.x / s, a.y / s, a.z / s}; }
static double dot(V a, V b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
static V cross(V a, V b) { return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }
static V unit(V a) { return a / std::sqrt(dot(a, a)); }

// Bit s of the result: the scan's disc of the camera ray of pixel (i, j) with jitter (xu, xv) is not negative for sphere s < 32 (NaN counts as a hit)
static uint32_t discs_not_negative(const double *cam, uint32_t W, uint32_t H, uint32_t i, uint32_t j, double xu, double xv, const std::vector<double> &sph) {
    const V o{cam[0], cam[1], cam[2]}, llc{cam[3], cam[4], cam[5]}, hor{cam[6], cam[7], cam[8]}, ver{cam[9], cam[10], cam[11]};
    const double u = ((double)(i - 1) + xu) / (double)(W - 1);              // :398
    const double v = ((double)(j - 1) + xv) / (double)(H - 1);              // :399
    const V d = unit(((llc + hor * u) + ver * v) - o);                      // :303
    const double a = dot(d, d), four_a = 4.0 * a;                           // :115
    uint32_t hit = 0;
    for (size_t s = 0; s < sph.size() / 5 && s < 32; ++s) {
        const V oc = o - V{sph[5 * s], sph[5 * s + 1], sph[5 * s + 2]};      // :114
        const double cc = dot(oc, oc) - sph[5 * s + 3] * sph[5 * s + 3];     // :117
        const double b = 2.0 * dot(oc, d);                                   // :116
        const double bb = b * b;
        const double disc = bb - four_a * cc;                                // :118
        if (!(disc < 0)) hit |= 1u << s;                                     // :120
    }
    return hit;
}

struct Tally { uint64_t pairs = 0, unreachable = 0, pixels = 0; };

// every pixel of the frame: the mask against the scan, sky_pixel against the parent's; returns the (pixel, sphere) pairs and how many are unreachable
static Tally check_frame(const double *cam, uint32_t W, uint32_t H, const std::vector<double> &sph, std::mt19937_64 &rng, int n_random = 16) {
    const double top = 1.0 - 1.0 / 2097152.0;                                // the largest jitter rng3 gives: (2^21 - 1) 2^-21
    const uint32_t n = (uint32_t)(sph.size() / 5), bits = n < 32 ? n : 32;
    const uint32_t all = bits == 32 ? 0xFFFFFFFFu : (1u << bits) - 1u;
    Tally t;
    for (uint32_t j = 1; j <= H; ++j)
        for (uint32_t i = 1; i <= W; ++i) {
            bool beyond = false;
            const uint32_t reach = spira::pixel_reach(cam, W, H, i, j, sph.data(), n, &beyond);
            const bool was = parent::sky_pixel(cam, W, H, i, j, sph.data(), n), is = spira::sky_pixel(cam, W, H, i, j, sph.data(), n);
            if (was != is) { if (g_fail < 20) std::fprintf(stderr, "pixel (%u, %u) of %u x %u, %u spheres: sky_pixel %d, before %d\n", i, j, W, H, n, (int)is, (int)was); ++g_fail; }
            if (n <= 32) CHECK(is == (reach == 0) && !beyond);
            CHECK(spira::pixel_reach(cam, W, H, i, j, sph.data(), n) == reach);      // with and without the optional argument
            ++t.pixels; t.pairs += bits; t.unreachable += (uint64_t)__builtin_popcount(~reach & all);
            const uint32_t clear = ~reach & all;
            if (!clear) continue;
            uint32_t hit = 0;
            for (int k = 0; k < 4; ++k) hit |= discs_not_negative(cam, W, H, i, j, (k & 1) ? top : 0.0, (k & 2) ? top : 0.0, sph);
            for (int k = 0; k < n_random; ++k) {
                const double xu = (double)(rng() >> 43) / 2097152.0, xv = (double)(rng() >> 43) / 2097152.0;      // multiples of 2^-21, as rng3's
                hit |= discs_not_negative(cam, W, H, i, j, xu, xv, sph);
            }
            if (hit & clear) {
                if (g_fail < 20) std::fprintf(stderr, "pixel (%u, %u) of %u x %u: mask %08x calls spheres %08x unreachable and a ray of it has disc >= 0\n", i, j, W, H, reach, hit & clear);
                ++g_fail;
            }
        }
    return t;
}

// the reference's camera (:373-389) in Float64: origin, lower-left corner, horizontal, vertical
static void lookat(V from, V at, V up, double fov_deg, double aspect, double *cam) {
    const double h = std::tan(fov_deg * 3.14159265358979323846 / 180.0 / 2.0);
    const double vh = 2.0 * h, vw = aspect * vh;
    const V w = unit(from - at), u = unit(cross(up, w)), v = cross(w, u);
    const V hor = u * vw, ver = v * vh, llc = ((from - hor / 2.0) - ver / 2.0) - w;
    const V parts[4] = {from, llc, hor, ver};
    for (int k = 0; k < 4; ++k) { cam[3 * k] = parts[k].x; cam[3 * k + 1] = parts[k].y; cam[3 * k + 2] = parts[k].z; }
}

static spira::PlanIn plan_in(uint32_t prec, uint32_t w, uint32_t rows, uint32_t spp, uint32_t n_triangles) {
    spira::PlanIn in;
    in.width = w; in.rows = rows; in.spp = spp; in.max_depth = 8; in.n_triangles = n_triangles; in.num_cus = 256;
    in.prec = prec; in.block = 256; in.waves_per_simd = prec == 8 ? 4 : 5; in.carry_key = 1;
    in.pack4 = 4 * prec; in.pack3 = 3 * prec; in.pack2 = 2 * prec;
    return in;
}

int main(int argc, char **argv) {
    if (argc < 2) { std::fprintf(stderr, "usage: reach_mask <scene file>\n"); return 2; }
    std::vector<double> s1;
    {
        FILE *f = std::fopen(argv[1], "r");
        if (!f) { std::fprintf(stderr, "cannot read %s\n", argv[1]); return 2; }
        double x;
        while (std::fscanf(f, "%la", &x) == 1) s1.push_back(x);
        std::fclose(f);
    }
    if (s1.size() != 12 + 5 * 5) { std::fprintf(stderr, "scene file: %zu values\n", s1.size()); return 2; }
    const std::vector<double> s1_cam(s1.begin(), s1.begin() + 12), s1_sph(s1.begin() + 12, s1.end());
    std::mt19937_64 rng(20261021);

    // ---- the S1 camera at the benchmark's size, at a size whose runs straddle row ends and at a tiny one
    {
        const Tally t = check_frame(s1_cam.data(), 1920, 1080, s1_sph, rng);
        std::printf("S1 1920x1080: %llu of %llu (pixel, sphere) pairs unreachable (%.2f %%)\n", (unsigned long long)t.unreachable, (unsigned long long)t.pairs,
                    100.0 * (double)t.unreachable / (double)t.pairs);
        CHECK(t.pairs == 5ull * 1920 * 1080);
        CHECK(t.unreachable * 100 >= 75 * t.pairs);       // the mask must not pass by clearing nothing
        const Tally m = check_frame(s1_cam.data(), 97, 55, s1_sph, rng);
        std::printf("S1 97x55: %llu of %llu pairs unreachable\n", (unsigned long long)m.unreachable, (unsigned long long)m.pairs);
        CHECK(m.unreachable > 0 && m.unreachable < m.pairs);
        const Tally s = check_frame(s1_cam.data(), 9, 5, s1_sph, rng);
        std::printf("S1 9x5: %llu of %llu pairs unreachable\n", (unsigned long long)s.unreachable, (unsigned long long)s.pairs);
        CHECK(s.pairs == 5ull * 9 * 5);
    }
    // ---- random cameras and sphere sets
    {
        std::uniform_real_distribution<double> U(-1.0, 1.0);
        Tally sum;
        for (int k = 0; k < 200; ++k) {
            const uint32_t W = 2 + (uint32_t)(rng() % 95), H = 2 + (uint32_t)(rng() % 63);
            const double scale = std::pow(10.0, 3.0 * U(rng));                     // scenes from 1e-3 to 1e3 across
            double cam[12];
            lookat(V{4 * U(rng), 4 * U(rng), 4 * U(rng)} * scale, V{U(rng), U(rng), U(rng)} * scale, unit(V{0.3 * U(rng), 1.0, 0.3 * U(rng)}), 10.0 + 50.0 * (U(rng) + 1.0),
                   (double)W / (double)H, cam);
            std::vector<double> sph;
            const int ns = 1 + (int)(rng() % 8);
            for (int s = 0; s < ns; ++s) {
                const double r = scale * std::pow(10.0, -2.0 + 1.5 * (U(rng) + 1.0)) * ((k % 7 == 0 && s == 0) ? 1e-4 : 1.0);      // some: tiny against their distance
                const double d = scale * 6.0 * U(rng);
                sph.insert(sph.end(), {d, scale * 6.0 * U(rng), scale * 6.0 * U(rng), r, 1.0});
            }
            if (k % 5 == 0) sph.insert(sph.end(), {0.0, -1000.0 * scale - 2.0 * scale, 0.0, 1000.0 * scale, 1.0});                  // a ground sphere
            const Tally t = check_frame(cam, W, H, sph, rng);
            sum.pairs += t.pairs; sum.unreachable += t.unreachable;
        }
        std::printf("random scenes: %llu of %llu pairs unreachable\n", (unsigned long long)sum.unreachable, (unsigned long long)sum.pairs);
        CHECK(sum.unreachable > sum.pairs / 20);                                     // they do exercise the function
    }
    // ---- edge cases (all on the S1 camera, 97 x 55)
    {
        const double *cam = s1_cam.data();
        const V o{cam[0], cam[1], cam[2]};
        const V fwd = unit(V{cam[3] + 0.5 * cam[6] + 0.5 * cam[9], cam[4] + 0.5 * cam[7] + 0.5 * cam[10], cam[5] + 0.5 * cam[8] + 0.5 * cam[11]} - o);
        auto one = [&](V c, double r) { return std::vector<double>{c.x, c.y, c.z, r, 1.0}; };
        auto with_s1 = [&](std::vector<double> first) { first.insert(first.end(), s1_sph.begin(), s1_sph.end()); return first; };      // the odd sphere is bit 0, S1's follow
        // the camera inside a sphere, and on its surface (exactly, and a rounding to either side): its bit is set everywhere; S1's bits are as they are alone
        for (const auto &sp : {one(o + fwd * 0.1, 0.5), one(o, 1.0), one(o + V{0.0, 2.0, 0.0}, 2.0), one(o + V{0.0, 2.0, 0.0}, std::nextafter(2.0, 3.0))}) {
            const Tally t = check_frame(cam, 97, 55, sp, rng);
            CHECK(t.unreachable == 0);
            for (uint32_t j = 1; j <= 55; j += 9)
                for (uint32_t i = 1; i <= 97; i += 7) {
                    const std::vector<double> both = with_s1(sp);
                    CHECK(spira::pixel_reach(cam, 97, 55, i, j, both.data(), 6) == (1u | (spira::pixel_reach(cam, 97, 55, i, j, s1_sph.data(), 5) << 1)));
                }
        }
        (void)check_frame(cam, 97, 55, one(o + V{0.0, 2.0, 0.0}, std::nextafter(2.0, 0.0)), rng);
        // a sphere behind the camera (the folded angle): the scan's disc knows no direction — the bit is set where the LINE of sight meets it
        {
            const std::vector<double> behind = one(o - fwd * 3.0, 0.5);
            const Tally t = check_frame(cam, 97, 55, behind, rng);
            CHECK(t.unreachable > 0 && t.unreachable < t.pairs);
            CHECK(spira::pixel_reach(cam, 97, 55, 49, 28, behind.data(), 1) == 1u);      // the centre pixel looks straight away from it
            (void)check_frame(cam, 97, 55, with_s1(behind), rng);
        }
        // a radius that is zero, negative or NaN, a centre that is NaN, infinite or huge: that sphere's bit is set everywhere, the others are untouched
        for (const auto &sp : {one(o + fwd * 3.0, 0.0), one(o + fwd * 3.0, -0.5), one(o + fwd * 3.0, std::nan("")), one(V{std::nan(""), 0.0, 0.0}, 0.5),
                               one(V{INFINITY, 0.0, 0.0}, 0.5), one(V{1e200, 1e200, 0.0}, 1e10)}) {
            CHECK(check_frame(cam, 97, 55, sp, rng).unreachable == 0);
            const Tally t = check_frame(cam, 97, 55, with_s1(sp), rng);
            CHECK(t.unreachable > 0);
            CHECK((spira::pixel_reach(cam, 97, 55, 3, 55, with_s1(sp).data(), 6) & 1u) == 1u);
        }
        // W or H below 2, a camera of zeros, a NaN in the camera: every bit is set
        CHECK(spira::pixel_reach(cam, 1, 55, 1, 7, s1_sph.data(), 5) == 0xFFFFFFFFu && spira::pixel_reach(cam, 97, 1, 7, 1, s1_sph.data(), 5) == 0xFFFFFFFFu);
        CHECK(spira::pixel_reach(cam, 0, 0, 1, 1, s1_sph.data(), 5) == 0xFFFFFFFFu);
        CHECK(!spira::sky_pixel(cam, 1, 55, 1, 7, s1_sph.data(), 5) && !spira::sky_pixel(cam, 97, 1, 7, 1, s1_sph.data(), 5) && !spira::sky_pixel(cam, 0, 0, 1, 1, s1_sph.data(), 5));
        (void)check_frame(cam, 1, 5, s1_sph, rng); (void)check_frame(cam, 7, 1, s1_sph, rng);
        double zero[12] = {0};
        CHECK(spira::pixel_reach(zero, 97, 55, 3, 3, s1_sph.data(), 5) == 0xFFFFFFFFu && !spira::sky_pixel(zero, 97, 55, 3, 3, s1_sph.data(), 5));
        double nanc[12];
        for (int k = 0; k < 12; ++k) nanc[k] = k == 7 ? std::nan("") : cam[k];
        CHECK(spira::pixel_reach(nanc, 97, 55, 3, 3, s1_sph.data(), 5) == 0xFFFFFFFFu && !spira::sky_pixel(nanc, 97, 55, 3, 3, s1_sph.data(), 5));
        // 0, 1, 32, 33 and 40 spheres: small ones on a grid across the lower half of the view, so that rows of the frame see none, some and the last ones only
        for (uint32_t n : {0u, 1u, 32u, 33u, 40u}) {
            const V right = unit(V{cam[6], cam[7], cam[8]}), upv = unit(V{cam[9], cam[10], cam[11]});
            std::vector<double> sph;
            for (uint32_t s = 0; s < n; ++s) {
                const V c = o + fwd * 6.0 + right * (-2.8 + 0.8 * (double)(s % 8)) + upv * (-1.6 + 0.55 * (double)(s / 8));
                sph.insert(sph.end(), {c.x, c.y, c.z, 0.2, 1.0});
            }
            const Tally t = check_frame(cam, 97, 55, sph, rng);
            uint64_t sky = 0, sky_low_bits_only = 0;
            for (uint32_t j = 1; j <= 55; ++j)
                for (uint32_t i = 1; i <= 97; ++i) {
                    const bool is = spira::sky_pixel(cam, 97, 55, i, j, sph.data(), n);
                    sky += is ? 1 : 0;
                    sky_low_bits_only += (spira::pixel_reach(cam, 97, 55, i, j, sph.data(), n) == 0 && !is) ? 1 : 0;
                }
            std::printf("%u spheres at 97x55: %llu of %llu pairs unreachable, %llu pixels sky, %llu reach only spheres past the mask\n", n, (unsigned long long)t.unreachable,
                        (unsigned long long)t.pairs, (unsigned long long)sky, (unsigned long long)sky_low_bits_only);
            CHECK(n == 0 ? sky == 97 * 55 : (sky > 0 && sky < 97 * 55));
            CHECK(n == 0 || t.unreachable > 0);
            CHECK(n <= 32 ? sky_low_bits_only == 0 : sky_low_bits_only > 0);      // the overflow case exists in the test: a pixel that sees sphere 32 + alone
        }
    }
    // ---- the plan's two fields and the launch check's (csrc/spira_plan.h)
    {
        const char *msg = nullptr;
        spira::Plan pl;
        CHECK(spira::make_plan(plan_in(8, 1920, 1080, 64, 0), pl, &msg) == 0 && pl.fused && pl.pixel_table && pl.reach_masks);
        spira::PlanIn in = plan_in(8, 1920, 1080, 64, 0);
        in.k.pixel_table = 0;
        CHECK(spira::make_plan(in, pl, &msg) == 0 && pl.fused && !pl.pixel_table && pl.reach_masks && pl.sky_runs);
        in.k.pixel_table = 1; in.k.reach_masks = 0;
        CHECK(spira::make_plan(in, pl, &msg) == 0 && pl.fused && pl.pixel_table && !pl.reach_masks && pl.sky_runs);
        in.k.reach_masks = 1; in.k.fused_resolve = 0;
        CHECK(spira::make_plan(in, pl, &msg) == 0 && !pl.fused && !pl.pixel_table && !pl.reach_masks);
        CHECK(spira::make_plan(plan_in(4, 1920, 1080, 64, 0), pl, &msg) == 0 && !pl.pixel_table && !pl.reach_masks);          // Float32: no pixel-owning pass
        CHECK(spira::make_plan(plan_in(8, 1920, 1080, 64, 12), pl, &msg) == 0 && !pl.pixel_table && !pl.reach_masks);         // LDS triangles: none either
        CHECK(spira::own_lds_bytes(4) == 4 * (64 * 32 + 16 * 4));
        CHECK(spira::make_plan(plan_in(8, 97, 55, 3, 0), pl, &msg) == 0 && pl.fused);
        spira::PathLaunch l;
        const spira::Geometry g = pl.geometry(pl.n_first(0));
        l.blocks = g.G; l.cap = g.cap; l.n_first = pl.n_first(0); l.k_eff = pl.k_eff(0); l.tile_pixels = 97 * 55; l.max_depth = 8;
        l.pixel_owning = true; l.l_private = pl.l_private; l.prec = 8; l.wpb = pl.wpb; l.carry_key = 1;
        CHECK(spira::path_need(l).table_ok && spira::path_need(l).owning_ok);                                                    // neither asked for
        l.pixel_table = true;
        CHECK(!spira::path_need(l).table_ok);                                                                                   // no room in the launch's LDS
        l.own_lds = spira::own_lds_bytes(l.wpb) - 1;
        CHECK(!spira::path_need(l).table_ok);
        l.own_lds = spira::own_lds_bytes(l.wpb);
        CHECK(spira::path_need(l).table_ok);
        l.pixel_table = false; l.reach_masks = true;
        CHECK(spira::path_need(l).table_ok);
        l.pixel_owning = false;
        CHECK(!spira::path_need(l).table_ok);                                                                                   // not a pixel-owning pass
    }
    if (g_fail) { std::fprintf(stderr, "%d checks failed\n", g_fail); return 1; }
    std::printf("all checks passed\n");
    return 0;
}
