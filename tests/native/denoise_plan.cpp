// denoise_plan.cpp — host-only harness built with -fsanitize=address,undefined (tests/test_denoise_cpu.py), in the manner of adaptive_plan.cpp: the
// launch and workspace arithmetic of the feature and denoise entries (spira_plan.h: features_check, features_grid, denoise_check, make_denoise_plan)
// swept over the parameter space.  For every valid plan the launch is replayed on counts: every pixel has exactly one lane of the tiled grid and one
// of the flat grid, every tap a kernel may read lies inside the image or is skipped, the record buffers hold a record per pixel, and the planes of the
// host form lie side by side inside the staging block.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <random>
#include <vector>

#include "../../julia-spira_amd/csrc/spira_plan.h"
#include "../../include/spira_hip.h"

static int g_fail = 0;
#define CHECK(c) do { if (!(c)) { std::fprintf(stderr, "CHECK failed %s:%d: %s\n", __FILE__, __LINE__, #c); ++g_fail; } } while (0)

static void check_plan(uint32_t w, uint32_t h, uint32_t it, uint32_t post, double sl, double sz, uint32_t guides, bool hdr, bool img, bool host, uint32_t prec) {
    spira::DenoiseIn in;
    in.width = w; in.height = h; in.iterations = it; in.post = post; in.sigma_l = sl; in.sigma_z = sz; in.guides = guides;
    in.want_hdr = hdr; in.want_img = img; in.host = host; in.prec = prec; in.pack4 = 4 * prec;
    spira::DenoisePlan dp;
    const char *msg = nullptr;
    const int rc = spira::make_denoise_plan(in, dp, &msg);
    const bool post_ok = post == SPIRA_POST_ACES || post == SPIRA_POST_ACES_GAMMA || post == SPIRA_POST_CLAMP_GAMMA || post == SPIRA_POST_NONE;
    const bool valid = w >= 1 && h >= 1 && it >= 1 && it <= 6 && sl > 0 && sz > 0 && post_ok && (hdr || img);
    if (!valid) { CHECK(rc == SPIRA_E_INVALID && msg); return; }
    if ((uint64_t)w * h > 0x7FFFFFFFull) { CHECK(rc == SPIRA_E_LIMIT && msg); return; }
    CHECK(rc == 0);
    const uint64_t npix = (uint64_t)w * h;
    CHECK(dp.npix == npix);
    // the tiled grid: tiles of 64 x 4 cover the image, no tile lies wholly outside it, and the flat index of the last lane stays below 2^32
    CHECK((uint64_t)dp.tiles_x * spira::kDenoiseTileW >= w && (uint64_t)(dp.tiles_x - 1) * spira::kDenoiseTileW < w);
    CHECK((uint64_t)dp.tiles_y * spira::kDenoiseTileH >= h && (uint64_t)(dp.tiles_y - 1) * spira::kDenoiseTileH < h);
    CHECK(dp.grid == (uint64_t)dp.tiles_x * dp.tiles_y && dp.grid >= 1 && dp.grid <= npix);
    CHECK((uint64_t)dp.grid_flat * spira::kDenoiseTileW * spira::kDenoiseTileH >= npix && ((uint64_t)dp.grid_flat - 1) * spira::kDenoiseTileW * spira::kDenoiseTileH < npix);
    CHECK((uint64_t)dp.grid_flat * spira::kDenoiseTileW * spira::kDenoiseTileH <= 0xFFFFFFFFull);
    // a lane's pixel coordinates in 32-bit arithmetic, as the kernel computes them: the last tile's last lane
    {
        const uint32_t b = dp.grid - 1, ty = b / dp.tiles_x, tx = b - ty * dp.tiles_x;
        const uint64_t x = (uint64_t)tx * spira::kDenoiseTileW + 63, y = (uint64_t)ty * spira::kDenoiseTileH + 3;
        CHECK(x <= 0xFFFFFFFFull && y <= 0xFFFFFFFFull && tx == dp.tiles_x - 1 && ty == dp.tiles_y - 1);
    }
    // taps: q = p + s * d in wrapping 32-bit arithmetic is either inside the image or >= the extent (and then skipped), for the corners of the image
    for (uint32_t i = 0; i < it; ++i) {
        const uint32_t s = dp.step(i);
        CHECK(s == (1u << i) && dp.reach(i) == 2 * s && dp.reach(i) <= 64);
        for (uint32_t x : {0u, w / 2, w - 1})
            for (int d = -2; d <= 2; ++d) {
                const uint32_t q = x + (uint32_t)(d * (int)s);
                const int64_t exact = (int64_t)x + (int64_t)d * s;
                CHECK((q < w) == (exact >= 0 && exact < (int64_t)w));
                if (q < w) CHECK((int64_t)q == exact);
            }
        for (uint32_t y : {0u, h / 2, h - 1})
            for (int d = -2; d <= 2; ++d) {
                const uint32_t q = y + (uint32_t)(d * (int)s);
                const int64_t exact = (int64_t)y + (int64_t)d * s;
                CHECK((q < h) == (exact >= 0 && exact < (int64_t)h));
            }
    }
    // workspaces
    CHECK(dp.rec_bytes == npix * 4 * prec);
    const bool guide = (guides & (spira::kDenoiseNormal | spira::kDenoiseDepth)) != 0;
    CHECK(dp.guide_bytes == (guide ? npix * 4 * prec : 0));
    if (!host) { CHECK(dp.io_bytes == 0 && dp.in_planes == 0 && dp.out_planes == 0); return; }
    const uint32_t bit[5] = {0, spira::kDenoiseVariance, spira::kDenoiseAlbedo, spira::kDenoiseNormal, spira::kDenoiseDepth}, planes[5] = {3, 1, 3, 3, 1};
    uint64_t next = 0;
    for (int k = 0; k < 5; ++k) {
        const bool given = k == 0 || (guides & bit[k]);
        if (!given) { CHECK(dp.in_off[k] == -1); continue; }
        CHECK(dp.in_off[k] == (int64_t)next);                                   // side by side, in argument order, no overlap
        next += planes[k];
    }
    CHECK(dp.in_planes == next && dp.in_planes >= 3 && dp.in_planes <= 11);
    CHECK(dp.out_planes == (hdr ? 3u : 0u) + (img ? 3u : 0u));
    CHECK(dp.io_bytes == (dp.in_planes + dp.out_planes) * npix * prec);
}

int main() {
    std::mt19937_64 rng(20261017);
    const uint32_t widths[] = {0, 1, 2, 19, 63, 64, 65, 67, 160, 1920, 65535, 65536, 1u << 20, 0x7FFFFFFFu, 0x80000000u, 0xFFFFFFFFu};
    const uint32_t heights[] = {0, 1, 3, 4, 5, 13, 35, 90, 1080, 32768, 65537, 0x7FFFFFFFu, 0xFFFFFFFFu};
    const uint32_t iters[] = {0, 1, 2, 5, 6, 7, 0xFFFFFFFFu};
    const uint32_t posts[] = {SPIRA_POST_ACES, SPIRA_POST_ACES_GAMMA, SPIRA_POST_CLAMP_GAMMA, SPIRA_POST_NONE, 0x400u, 1u, SPIRA_ROWS_BOTTOM_UP};
    long n = 0;
    for (uint32_t w : widths) for (uint32_t h : heights) for (uint32_t it : iters) for (uint32_t post : posts)
        for (uint32_t guides = 0; guides < 16; ++guides) for (int outs = 0; outs < 4; ++outs) for (int host = 0; host < 2; ++host) {
            check_plan(w, h, it, post, 4.0, 0.1, guides, outs & 1, outs & 2, host, (guides ^ outs) & 1 ? 4 : 8); ++n;
        }
    const double bad[] = {0.0, -0.0, -1.0, std::nan(""), -INFINITY};
    for (double b : bad) { check_plan(16, 9, 5, 0, b, 0.1, 15, true, true, true, 4); check_plan(16, 9, 5, 0, 4.0, b, 15, true, true, true, 8); n += 2; }
    check_plan(16, 9, 5, 0, 5e-324, INFINITY, 15, true, false, false, 8); ++n;      // (positive: valid here; the entry refuses a sigma that rounds to 0 in Float32)
    for (int i = 0; i < 20000; ++i) {
        const uint32_t w = 1 + (uint32_t)(rng() % 4096), h = 1 + (uint32_t)(rng() % 2400);
        check_plan(w, h, 1 + (uint32_t)(rng() % 6), (uint32_t)(rng() % 4) << 8, 4.0, 0.1, (uint32_t)(rng() % 16), true, rng() & 1, rng() & 1, (rng() & 1) ? 4 : 8); ++n;
    }
    // the scope of the feature entries and their grid
    const char *msg = nullptr;
    CHECK(spira::features_check(0, true, &msg) == 0 && spira::features_check(SPIRA_POST_NONE | SPIRA_ROWS_BOTTOM_UP, true, &msg) == 0);
    CHECK(spira::features_check(0, false, &msg) == SPIRA_E_INVALID);
    for (uint32_t f : {SPIRA_SEM_CPU, SPIRA_SEM_METAL, SPIRA_SEM_HYBRID, SPIRA_KERNEL_MEGA, SPIRA_KERNEL_BOUNCE, SPIRA_KERNEL_WAVEFRONT, SPIRA_EXT_DIELECTRIC, SPIRA_EXT_SPECTRAL})
        CHECK(spira::features_check(f, true, &msg) == SPIRA_E_UNSUPPORTED && msg);
    for (uint64_t tp : {(uint64_t)1, (uint64_t)255, (uint64_t)256, (uint64_t)257, (uint64_t)67 * 35, (uint64_t)1920 * 1080, (uint64_t)0x7FFFFFFF})
        for (uint32_t cus : {0u, 1u, 256u, 304u}) {
            const uint32_t g = spira::features_grid(tp, 256, cus);
            CHECK(g >= 1 && (uint64_t)g <= (tp + 255) / 256 && (uint64_t)g <= std::max<uint64_t>(1, (uint64_t)cus * 64));
            CHECK((uint64_t)g * 256 + tp <= 0xFFFFFFFFull);                    // the kernel's stride loop: p + grid * block never wraps
            ++n;
        }
    std::printf("%ld plans\n", n);
    if (g_fail) { std::printf("%d checks FAILED\n", g_fail); return 1; }
    std::printf("all checks passed\n");
    return 0;
}
