// adaptive_plan.cpp — host-only harness built with -fsanitize=address,undefined (tests/test_adaptive_cpu.py), in the manner of host_sanitize.cpp:
// the schedule and workspace arithmetic of an adaptive render (spira_plan.h: adaptive_check, make_adaptive_plan, AdaptivePlan::level / round, and
// make_plan with PlanIn::adaptive for round 0) swept over the parameter space.  For every plan a worst-case render is replayed on counts alone:
// the levels rise strictly to the cap and never past it, a list never needs more entries than it has, and every round's grid covers its list
// within the LDS block and the lane count the refinement kernel assumes (spira_adaptive.h, k_refine).
#include <cstdint>
#include <cstdio>
#include <random>
#include <vector>

#include "../../julia-spira_amd/csrc/spira_plan.h"
#include "../../include/spira_hip.h"

static int g_fail = 0;
#define CHECK(c) do { if (!(c)) { std::fprintf(stderr, "CHECK failed %s:%d: %s\n", __FILE__, __LINE__, #c); ++g_fail; } } while (0)

static void check_round(const spira::AdaptivePlan &ap, uint32_t r, uint64_t n_active) {
    const spira::AdaptiveRound g = ap.round(r, n_active);
    CHECK(g.samples == ap.level(r) - ap.level(r - 1) && g.samples >= 1 && g.samples <= ap.in.batch_spp);
    CHECK(g.chunk >= 1 && g.chunk <= g.samples && g.chunk <= spira::kAdaptiveItems);
    CHECK(g.ppw >= 1 && g.ppw <= 64 && (uint64_t)g.ppw * g.chunk <= spira::kAdaptiveItems);      // a lane per owned pixel, the wave's LDS block
    CHECK(g.waves * g.ppw >= n_active && (g.waves - 1) * g.ppw < n_active);                        // every entry has a wave, no wave is idle
    CHECK((uint64_t)g.grid * spira::kAdaptiveWpb >= g.waves && (uint64_t)(g.grid - 1) * spira::kAdaptiveWpb < g.waves);
    // the chunks of a round cover its samples exactly
    uint64_t covered = 0;
    for (uint32_t s0 = 0; s0 < g.samples; s0 += g.chunk) covered += std::min(g.chunk, g.samples - s0);
    CHECK(covered == g.samples);
}

static void check_plan(uint32_t mn, uint32_t batch, uint32_t spp, uint64_t tp, uint32_t prec, uint32_t cus, std::mt19937_64 &rng) {
    spira::AdaptiveIn in;
    in.min_spp = mn; in.batch_spp = batch; in.spp = spp; in.tolerance = 0.05; in.floor = 0.01;
    in.tile_pixels = tp; in.prec = prec; in.pack3 = 3 * prec; in.num_cus = cus;
    spira::AdaptivePlan ap;
    const char *msg = nullptr;
    const int rc = spira::make_adaptive_plan(in, ap, &msg);
    const bool valid = mn >= 2 && batch >= 1 && mn <= spp;
    if (!valid) { CHECK(rc == SPIRA_E_INVALID && msg); return; }
    if (tp == 0 || tp > 0x7FFFFFFFull) { CHECK(rc == SPIRA_E_LIMIT && msg); return; }
    CHECK(rc == 0);
    // levels: min, min + batch, ..., spp — strictly rising, the last one the cap, none past it
    CHECK(ap.levels >= 1 && ap.level(0) == mn && ap.level(ap.levels - 1) == spp);
    const uint32_t probe = ap.levels <= 4096 ? ap.levels : 4096;
    for (uint32_t r = 1; r < probe; ++r) CHECK(ap.level(r) > ap.level(r - 1) && ap.level(r) <= spp && (r + 1 == ap.levels || ap.level(r) == mn + (uint64_t)r * batch));
    CHECK(ap.level(ap.levels) == spp && ap.level(0xFFFFFFFFu) == spp);                             // (past the end: still the cap, no overflow)
    if (ap.levels >= 2) CHECK(ap.level(ap.levels - 2) < spp);
    // workspaces: a list holds every pixel of the tile, one Q and one count per pixel, two list lengths, the refinement LDS block
    CHECK(ap.list_cap == tp && ap.list_bytes == tp * 4 && ap.q_bytes == tp * prec && ap.n_bytes == tp * 4 && ap.count_bytes == 8);
    CHECK(ap.lds_round == (uint64_t)spira::kAdaptiveWpb * spira::kAdaptiveItems * in.pack3 && ap.lds_round <= 64 * 1024);
    // a render replayed on counts: the active set only shrinks, so no list outgrows list_cap; total samples stay within the cap
    uint64_t n_active = tp, total = tp * mn;
    for (uint32_t r = 1; r < ap.levels && r < 64 && n_active; ++r) {
        CHECK(n_active <= ap.list_cap);
        check_round(ap, r, n_active);
        total += n_active * (ap.level(r) - ap.level(r - 1));
        n_active = (r % 3 == 0) ? n_active : n_active - rng() % (n_active + 1);                    // some rounds nobody converges
    }
    CHECK(total <= tp * (uint64_t)spp);
    // the corners of a round's geometry: one entry, a full list, and the last round (its batch may be cut by the cap)
    for (uint32_t r : {1u, ap.levels - 1})
        if (r >= 1 && r < ap.levels)
            for (uint64_t n : {(uint64_t)1, (uint64_t)63, (uint64_t)64, (uint64_t)65, tp / 2 + 1, tp}) if (n >= 1 && n <= tp) check_round(ap, r, n);
}

// round 0 is a plan of the ordinary planner with PlanIn::adaptive: never pixel-owning, so its passes end in a resolve launch (k_resolve_adaptive) over a slot-major L
static void check_round0(uint32_t prec, uint32_t w, uint32_t rows, uint32_t mn, uint32_t nt, uint32_t batch_rays) {
    spira::PlanIn in;
    in.width = w; in.rows = rows; in.spp = mn; in.max_depth = 8; in.flags = 0; in.batch_rays = batch_rays; in.n_triangles = nt; in.num_cus = 256;
    in.prec = prec; in.block = 256; in.waves_per_simd = prec == 8 ? 4 : 5; in.carry_key = 1; in.pack4 = 4 * prec; in.pack3 = 3 * prec; in.pack2 = 2 * prec;
    spira::Plan plain, ad;
    const char *msg = nullptr;
    const int rc0 = spira::make_plan(in, plain, &msg);
    in.adaptive = true;
    const int rc1 = spira::make_plan(in, ad, &msg);
    CHECK(rc0 == rc1);
    if (rc1) return;
    CHECK(ad.org == spira::Org::Path && !ad.fused && !ad.l_private);
    CHECK(ad.slots == plain.slots && ad.n_pass == plain.n_pass && ad.batch == plain.batch);
    uint64_t samples = 0;
    for (uint32_t pass = 0; pass < ad.n_pass; ++pass) {
        const spira::Geometry g = ad.geometry(ad.n_first(pass));
        CHECK((uint64_t)g.G * ad.wpb * g.cap >= ad.n_first(pass));                                 // the pass fits its queue regions
        CHECK(ad.ws.L >= (uint64_t)ad.n_first(pass) * in.pack3);                                   // slot-major L: k_eff planes of tile_pixels entries
        samples += ad.k_eff(pass);
    }
    CHECK(samples == mn);
    CHECK(ad.ws.accum == ad.tile_pixels * in.pack4);
    if (prec == 8 && nt == 0 && plain.slots <= 64) CHECK(plain.fused);                             // (the plan the flag overrides)
}

int main() {
    std::mt19937_64 rng(20251017);
    const uint32_t mins[] = {0, 1, 2, 3, 8, 16, 63, 64, 65, 255, 256, 257, 1000, 1u << 24};
    const uint32_t batches[] = {0, 1, 2, 7, 8, 32, 63, 64, 65, 128, 255, 256, 257, 1000, 1u << 24, 0xFFFFFFFFu};
    const uint32_t spps[] = {1, 2, 3, 8, 40, 64, 257, 1024, 65536, 1u << 24};
    const uint64_t tiles[] = {0, 1, 4, 63, 64, 65, 160 * 90, 1920 * 1080, 0x7FFFFFFFull, 0x80000000ull};
    long n = 0;
    for (uint32_t mn : mins) for (uint32_t b : batches) for (uint32_t s : spps) for (uint64_t tp : tiles)
        for (uint32_t prec : {4u, 8u}) for (uint32_t cus : {1u, 64u, 256u}) { check_plan(mn, b, s, tp, prec, cus, rng); ++n; }
    for (int i = 0; i < 20000; ++i) {
        const uint32_t s = 2 + (uint32_t)(rng() % 4096), mn = 2 + (uint32_t)(rng() % (s - 1)), b = 1 + (uint32_t)(rng() % 300);
        check_plan(mn, b, s, 1 + rng() % (1920 * 1080), (rng() & 1) ? 4 : 8, 1 + (uint32_t)(rng() % 304), rng); ++n;
    }
    // bad tolerances
    const char *msg = nullptr;
    CHECK(spira::adaptive_check(2, 1, 2, 0.0, 0.0, &msg) == 0);
    CHECK(spira::adaptive_check(2, 1, 2, -1e-300, 0.0, &msg) == SPIRA_E_INVALID && spira::adaptive_check(2, 1, 2, 0.1, -1.0, &msg) == SPIRA_E_INVALID);
    CHECK(spira::adaptive_check(2, 1, 2, __builtin_nan(""), 0.0, &msg) == SPIRA_E_INVALID && spira::adaptive_check(2, 1, 2, 0.1, __builtin_nan(""), &msg) == SPIRA_E_INVALID);
    for (uint32_t prec : {4u, 8u}) for (uint32_t mn : {2u, 8u, 64u, 65u, 300u}) for (uint32_t nt : {0u, 1u, 32u, 33u, 1280u})
        for (uint32_t br : {0u, 1u << 16}) { check_round0(prec, 160, 90, mn, nt, br); check_round0(prec, 1920, 1080, mn, nt, br); n += 2; }
    std::printf("%ld plans\n", n);
    if (g_fail) { std::printf("%d checks FAILED\n", g_fail); return 1; }
    std::printf("all checks passed\n");
    return 0;
}
