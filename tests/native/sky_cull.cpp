// sky_cull.cpp — host-only harness built with -fsanitize=address,undefined (tests/test_sky_cull_cpu.py), in the manner of host_sanitize.cpp: the
// all-sky classifier of the pixel-owning passes (csrc/spira_sky.h, sky_pixel) against the sphere scan's own discriminant.  For every pixel the
// function calls sky, every checked camera ray of the pixel — the four corner jitters (0 and 1 - 2^-21 in each axis) and 16 random ones — must
// have disc < 0 for every sphere, disc being the scan's statements (examples/julia-raytracer.jl:114-118) on the camera ray of :398-399 and :303,
// restated here in Float64 in the written order (-ffp-contract=off).
//
// usage: sky_cull <file>     the file holds the S1 scene as the library hands it out: 12 camera values, then 5 values per sphere ("%la" each)
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <random>
#include <vector>

#include "../../julia-spira_amd/csrc/spira_sky.h"

static int g_fail = 0;
#define CHECK(c) do { if (!(c)) { if (g_fail < 20) std::fprintf(stderr, "CHECK failed %s:%d: %s\n", __FILE__, __LINE__, #c); ++g_fail; } } while (0)

struct V { double x, y, z; };
static V operator+(V a, V b) { return {a.x + b.x, a.y + b.y, a.z + b.z}; }
static V operator-(V a, V b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
static V operator*(V a, double s) { return {a.x * s, a.y * s, a.z * s}; }
static V operator/(V a, double s) { return {a.x / s, a.y / s, a.z / s}; }
static double dot(V a, V b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
static V cross(V a, V b) { return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }
static V unit(V a) { return a / std::sqrt(dot(a, a)); }

// the scan's discriminant of the camera ray of pixel (i, j) with jitter (xu, xv) against sphere s: the largest over the spheres (NaN counts as a hit)
static bool any_disc_not_negative(const double *cam, uint32_t W, uint32_t H, uint32_t i, uint32_t j, double xu, double xv, const std::vector<double> &sph) {
    const V o{cam[0], cam[1], cam[2]}, llc{cam[3], cam[4], cam[5]}, hor{cam[6], cam[7], cam[8]}, ver{cam[9], cam[10], cam[11]};
    const double u = ((double)(i - 1) + xu) / (double)(W - 1);              // :398
    const double v = ((double)(j - 1) + xv) / (double)(H - 1);              // :399
    const V d = unit(((llc + hor * u) + ver * v) - o);                      // :303
    for (size_t s = 0; s < sph.size() / 5; ++s) {
        const V oc = o - V{sph[5 * s], sph[5 * s + 1], sph[5 * s + 2]};      // :114
        const double a = dot(d, d);                                          // :115
        const double b = 2.0 * dot(oc, d);                                   // :116
        const double c = dot(oc, oc) - sph[5 * s + 3] * sph[5 * s + 3];      // :117
        const double disc = b * b - 4.0 * a * c;                             // :118
        if (!(disc < 0)) return true;                                        // :120
    }
    return false;
}

// every pixel of the frame (or a sample of them: step > 1): returns the number of pixels called sky
static uint64_t check_frame(const double *cam, uint32_t W, uint32_t H, const std::vector<double> &sph, std::mt19937_64 &rng, uint32_t step = 1, int n_random = 16) {
    const double top = 1.0 - 1.0 / 2097152.0;                                // the largest jitter rng3 gives: (2^21 - 1) 2^-21
    uint64_t n_sky = 0;
    for (uint32_t j = 1; j <= H; j += step)
        for (uint32_t i = 1; i <= W; i += step) {
            if (!spira::sky_pixel(cam, W, H, i, j, sph.data(), (uint32_t)(sph.size() / 5))) continue;
            ++n_sky;
            bool hit = false;
            for (int k = 0; k < 4; ++k) hit = hit || any_disc_not_negative(cam, W, H, i, j, (k & 1) ? top : 0.0, (k & 2) ? top : 0.0, sph);
            for (int k = 0; k < n_random; ++k) {
                const double xu = (double)(rng() >> 43) / 2097152.0, xv = (double)(rng() >> 43) / 2097152.0;      // multiples of 2^-21, as rng3's
                hit = hit || any_disc_not_negative(cam, W, H, i, j, xu, xv, sph);
            }
            if (hit) { if (g_fail < 20) std::fprintf(stderr, "pixel (%u, %u) of %u x %u is called sky and a ray of it has disc >= 0\n", i, j, W, H); ++g_fail; }
        }
    return n_sky;
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

static uint64_t count_all(const double *cam, uint32_t W, uint32_t H, const std::vector<double> &sph) {
    uint64_t n = 0;
    for (uint32_t j = 1; j <= H; ++j) for (uint32_t i = 1; i <= W; ++i) n += spira::sky_pixel(cam, W, H, i, j, sph.data(), (uint32_t)(sph.size() / 5)) ? 1 : 0;
    return n;
}

int main(int argc, char **argv) {
    if (argc < 2) { std::fprintf(stderr, "usage: sky_cull <scene file>\n"); return 2; }
    std::vector<double> s1;
    {
        FILE *f = std::fopen(argv[1], "r");
        if (!f) { std::fprintf(stderr, "cannot read %s\n", argv[1]); return 2; }
        double x;
        while (std::fscanf(f, "%la", &x) == 1) s1.push_back(x);
        std::fclose(f);
    }
    if (s1.size() < 17 || (s1.size() - 12) % 5 != 0) { std::fprintf(stderr, "scene file: %zu values\n", s1.size()); return 2; }
    const std::vector<double> s1_cam(s1.begin(), s1.begin() + 12), s1_sph(s1.begin() + 12, s1.end());
    std::mt19937_64 rng(20261018);

    // ---- the S1 camera at the benchmark's size and at a size whose runs straddle row ends
    {
        const uint64_t n = check_frame(s1_cam.data(), 1920, 1080, s1_sph, rng);
        std::printf("S1 1920x1080: %llu of %llu pixels sky (%.2f %%)\n", (unsigned long long)n, 1920ull * 1080ull, 100.0 * (double)n / (1920.0 * 1080.0));
        CHECK(n * 100 >= 24ull * 1920 * 1080);        // the classifier must not pass by classifying nothing: 27.1 % of the centre rays miss everything
        const uint64_t m = check_frame(s1_cam.data(), 97, 55, s1_sph, rng);
        std::printf("S1 97x55: %llu of %u pixels sky\n", (unsigned long long)m, 97 * 55);
        CHECK(m > 0 && m < 97 * 55);
    }
    // ---- random cameras and sphere sets
    {
        std::uniform_real_distribution<double> U(-1.0, 1.0);
        uint64_t total = 0, sky = 0;
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
            sky += check_frame(cam, W, H, sph, rng);
            total += (uint64_t)W * H;
        }
        std::printf("random scenes: %llu of %llu pixels sky\n", (unsigned long long)sky, (unsigned long long)total);
        CHECK(sky > total / 20);                                                     // they do exercise the function
    }
    // ---- edge cases (all on the S1 camera, 97 x 55)
    {
        const double *cam = s1_cam.data();
        const V o{cam[0], cam[1], cam[2]};
        const V fwd = unit(V{cam[3] + 0.5 * cam[6] + 0.5 * cam[9], cam[4] + 0.5 * cam[7] + 0.5 * cam[10], cam[5] + 0.5 * cam[8] + 0.5 * cam[11]} - o);
        auto one = [&](V c, double r) { return std::vector<double>{c.x, c.y, c.z, r, 1.0}; };
        // the camera inside a sphere, and on its surface (exactly, and a rounding away): every ray has disc >= 0 — nothing may be called sky
        CHECK(count_all(cam, 97, 55, one(o + fwd * 0.1, 0.5)) == 0);
        CHECK(count_all(cam, 97, 55, one(o, 1.0)) == 0);
        CHECK(count_all(cam, 97, 55, one(o + V{0.0, 2.0, 0.0}, 2.0)) == 0);
        CHECK(count_all(cam, 97, 55, one(o + V{0.0, 2.0, 0.0}, std::nextafter(2.0, 3.0))) == 0);
        (void)check_frame(cam, 97, 55, one(o + V{0.0, 2.0, 0.0}, std::nextafter(2.0, 0.0)), rng);
        // a sphere behind the camera: the scan's disc knows no direction — pixels whose LINE of sight meets it are not sky
        {
            const std::vector<double> behind = one(o - fwd * 3.0, 0.5);
            const uint64_t n = check_frame(cam, 97, 55, behind, rng);
            CHECK(n > 0 && n < 97 * 55);
            CHECK(!spira::sky_pixel(cam, 97, 55, 49, 28, behind.data(), 1));       // the centre pixel looks straight away from it
        }
        // radius 0 (disc == 0 for a ray through the centre), a negative and a NaN radius, a NaN centre: "may hit" everywhere
        CHECK(count_all(cam, 97, 55, one(o + fwd * 3.0, 0.0)) == 0);
        CHECK(count_all(cam, 97, 55, one(o + fwd * 3.0, -0.5)) == 0);
        CHECK(count_all(cam, 97, 55, one(o + fwd * 3.0, std::nan(""))) == 0);
        CHECK(count_all(cam, 97, 55, one(V{std::nan(""), 0.0, 0.0}, 0.5)) == 0);
        CHECK(count_all(cam, 97, 55, one(V{INFINITY, 0.0, 0.0}, 0.5)) == 0);
        CHECK(count_all(cam, 97, 55, one(V{1e200, 1e200, 0.0}, 1e10)) == 0);
        // a radius-100 sphere grazing the frame: from far outside to well inside, in steps of a fraction of a pixel
        for (int k = -40; k <= 40; ++k) {
            const V side = unit(V{cam[6], cam[7], cam[8]});
            const double edge = 0.5 * std::sqrt(dot(V{cam[6], cam[7], cam[8]}, V{cam[6], cam[7], cam[8]}));      // half the frame's width at distance 1
            const double dist = 300.0;
            const V c = o + fwd * dist + side * (dist * edge * (1.0 + 0.002 * k) + 100.0 * std::sqrt(1.0 + edge * edge));
            (void)check_frame(cam, 97, 55, one(c, 100.0), rng);
        }
        // no sphere at all: everything is sky; a degenerate frame or camera: nothing is
        CHECK(count_all(cam, 97, 55, std::vector<double>{}) == 97 * 55);
        CHECK(!spira::sky_pixel(cam, 1, 55, 1, 7, s1_sph.data(), 5) && !spira::sky_pixel(cam, 97, 1, 7, 1, s1_sph.data(), 5) && !spira::sky_pixel(cam, 0, 0, 1, 1, s1_sph.data(), 5));
        double zero[12] = {0};
        CHECK(!spira::sky_pixel(zero, 97, 55, 3, 3, s1_sph.data(), 5));
        double nanc[12];
        for (int k = 0; k < 12; ++k) nanc[k] = k == 7 ? std::nan("") : cam[k];
        CHECK(!spira::sky_pixel(nanc, 97, 55, 3, 3, s1_sph.data(), 5));
    }
    if (g_fail) { std::fprintf(stderr, "%d checks failed\n", g_fail); return 1; }
    std::printf("all checks passed\n");
    return 0;
}
