// gather_plan.cpp — the host arithmetic of spira_scene_gather_*, spira_scene_gather_visible_* and spira_gather_rays_* as a stand-alone CPU program, built
// with -fsanitize=address,undefined by tests/test_gather_cpu.py and run directly:
//   1. make_gather_plan (spira_plan.h) swept over point counts, sample counts, caps and grids: every item (point, sample) is covered exactly once with
//      samples ascending, no pass holds more items than a 32-bit index reaches although a call may hold 2^50, the workspace stays within the cap; the
//      session plan of a visibility pass (make_gather_visible_plan) partitions the pass's items into disjoint wave ranges;
//   2. gather_check / gather_visible_check / gather_rays_check on their edges;
//   3. gather_ray_generate (spira_gather.h — the very function the kernels and the host entry call) over the inputs on stdin, printing bits:
//        line 1:  f32|f64
//        "gen sample seed key0 w0 .. w5"   the six values of a point as words in hex -> "gen <valid> r0 .. r5 d0 d1 d2"
//      (d: the unit direction radiance_ray_prepare gives for the generated ray — the one the gather kernels trace along)
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../julia-spira_amd/csrc/spira_plan.h"
#include "../../julia-spira_amd/csrc/spira_gather.h"

static long g_checks = 0;
#define CHECK(c)                                                                         \
    do {                                                                                 \
        ++g_checks;                                                                      \
        if (!(c)) { std::printf("CHECK FAILED line %d: %s\n", __LINE__, #c); std::exit(1); } \
    } while (0)

static void sweep_plans() {
    using namespace spira;
    const uint32_t ns[] = {1, 63, 64, 65, 257, 1000, 1u << 20, 1u << 26};
    const uint32_t spps[] = {1, 2, 3, 7, 8, 64, 1000, 1u << 24};
    const uint32_t caps[] = {0, 1, 999, 1000, 3000, 65536, 1u << 26, 0xFFFFFFFFu};
    const uint32_t wpcs[] = {0, 1, 16, 64, 1u << 20};
    const uint32_t cus[] = {0, 1, 256};
    long plans = 0;
    for (uint32_t n : ns) for (uint32_t spp : spps) for (uint32_t cap : caps) for (uint32_t wpc : wpcs) for (uint32_t cu : cus) {
        GatherKnobs k; k.max_items = cap; k.waves_per_cu = wpc;
        const GatherPlan p = make_gather_plan(n, spp, cu, 256, k);
        ++plans;
        CHECK(p.max_items >= 1 && p.max_items <= kRadianceMaxItems && (cap == 0 || p.max_items <= cap));
        CHECK(p.spp_pass >= 1 && p.spp_pass <= spp && p.n_pass >= 1);
        CHECK(p.direct == (p.spp_pass == 1));
        CHECK(p.ws_entries == (p.direct ? 0 : (uint64_t)n * p.spp_pass) && p.ws_entries <= p.max_items);
        CHECK((uint64_t)n * p.spp_pass <= kRadianceMaxItems);                  // a pass's items: an index (+ a grid's stride of at most 2^28) fits 32 bits
        // the passes: ascending, contiguous, covering [0, spp) exactly once; the call's items in 64 bits
        uint64_t next = 0, items = 0;
        const uint32_t walk = p.n_pass <= 4096 ? p.n_pass : 4096;             // (2^24 direct passes: the first 4096 and the last one, the rest by arithmetic)
        for (uint32_t q = 0; q < walk; ++q) {
            CHECK(p.first(q) == next && p.count(q) >= 1 && p.count(q) <= p.spp_pass);
            CHECK(p.items(q) == (uint64_t)n * p.count(q) && p.items(q) <= kRadianceMaxItems);
            next += p.count(q); items += p.items(q);
        }
        if (walk < p.n_pass) {
            CHECK(p.count(p.n_pass - 1) >= 1 && (uint64_t)p.first(p.n_pass - 1) + p.count(p.n_pass - 1) == spp);
        } else {
            CHECK(next == spp && items == (uint64_t)n * spp);
        }
        CHECK((uint64_t)(p.n_pass - 1) * p.spp_pass < spp && (uint64_t)p.n_pass * p.spp_pass >= spp);
        // within a pass item = point * count + s, sample-minor: the decode covers every (point, s) once, and a point's samples ascend with the item
        if ((uint64_t)n * p.spp_pass <= 4096) {
            std::vector<uint8_t> seen((size_t)n * p.spp_pass, 0);
            const FastDiv fd = fastdiv_make(p.spp_pass);
            uint32_t last_point = 0, last_s = 0;
            for (uint32_t i = 0; i < n * p.spp_pass; ++i) {
                const uint32_t point = fastdiv(i, fd), s = i - point * p.spp_pass;
                CHECK(point < n && s < p.spp_pass && !seen[(size_t)point * p.spp_pass + s]);
                CHECK(i == 0 || (point == last_point ? s == last_s + 1 : (point == last_point + 1 && s == 0)));
                seen[(size_t)point * p.spp_pass + s] = 1; last_point = point; last_s = s;
            }
        }
        CHECK(p.wpb == 4 && p.grid >= 1 && p.grid <= (1u << 20) && p.grid_flat >= 1);
        CHECK((uint64_t)(p.grid - 1) * 256 < (uint64_t)n * p.spp_pass);          // no workgroup without an item
        if (wpc == 0) CHECK(p.grid == 1);
        else CHECK(p.grid <= (uint64_t)(cu ? cu : 1) * wpc / 4 || p.grid == 1);
        // the session plan over the first pass's items: disjoint wave ranges covering [0, items)
        const uint32_t n_items = (uint32_t)p.items(0);
        const CastPlan cp = make_gather_visible_plan(n_items, cu, 256, k, CastKnobs());
        CHECK(cp.grid >= 1 && cp.wpb == 4 && cp.waves == cp.grid * cp.wpb && cp.grid_flat >= 1 && cp.refill_free >= 1 && cp.refill_free <= 64);
        CHECK((uint64_t)cp.base * cp.waves + cp.rem == n_items && cp.rem < cp.waves);
        CHECK(cp.begin(0) == 0 && (uint64_t)cp.begin(cp.waves - 1) + cp.count(cp.waves - 1) == n_items);
        if (cp.waves <= 4096) for (uint32_t w = 1; w < cp.waves; ++w) CHECK(cp.begin(w) == cp.begin(w - 1) + cp.count(w - 1));
        if (wpc == 0) CHECK(cp.grid == 1 && cp.grid_flat == 1);
    }
    // a call of more than 2^32 items: split into passes, never overflowed
    {
        const GatherPlan p = make_gather_plan(1u << 26, 1u << 24, 256, 256, GatherKnobs());
        CHECK(p.spp_pass == 1 && p.n_pass == (1u << 24) && p.direct && p.items(0) == (1ull << 26));
        const GatherPlan q = make_gather_plan(1u << 20, 1u << 16, 256, 256, GatherKnobs());
        CHECK(q.spp_pass == 64 && q.n_pass == 1024 && !q.direct && q.items(0) == (1ull << 26) && (uint64_t)q.n_pass * q.items(0) == (1ull << 36));
    }
    std::printf("%ld plans checked\n", plans);

    const char *msg = nullptr;
    CHECK(gather_check(true, true, true, 4, 1, 1, 0, 0, 0, 0, &msg) == 0);
    CHECK(gather_check(false, true, true, 4, 1, 1, 0, 0, 0, 0, &msg) == SPIRA_E_INVALID);
    CHECK(gather_check(true, false, true, 4, 1, 1, 0, 0, 0, 0, &msg) == SPIRA_E_INVALID);
    CHECK(gather_check(true, true, false, 4, 1, 1, 0, 0, 0, 0, &msg) == SPIRA_E_INVALID);
    CHECK(gather_check(true, true, true, 0, 1, 1, 0, 0, 0, 0, &msg) == SPIRA_E_INVALID);
    CHECK(gather_check(true, true, true, 4, 0, 1, 0, 0, 0, 0, &msg) == SPIRA_E_INVALID);
    CHECK(gather_check(true, true, true, 4, 1, 0, 0, 0, 0, 0, &msg) == SPIRA_E_INVALID);
    CHECK(gather_check(true, true, true, 4, 1, 256, 0, 0, 0, 0, &msg) == SPIRA_E_INVALID);
    CHECK(gather_check(true, true, true, 4, 1, 255, 0, 0, 0, 0, &msg) == 0);
    CHECK(gather_check(true, true, true, 4, 1, 1, 0, 0, 0, 1, &msg) == SPIRA_E_INVALID);
    CHECK(gather_check(true, true, true, 4, 1, 1, SPIRA_EXT_DIELECTRIC | SPIRA_EXT_SPECTRAL, 0, 0, 0, &msg) == 0);
    CHECK(gather_check(true, true, true, 4, 1, 1, SPIRA_KERNEL_MEGA, 0, 0, 0, &msg) == SPIRA_E_UNSUPPORTED);
    CHECK(gather_check(true, true, true, SPIRA_MAX_RAYS, 1 << 24, 1, 0, 0, 0, 0, &msg) == 0);
    CHECK(gather_check(true, true, true, SPIRA_MAX_RAYS + 1, 1, 1, 0, 0, 0, 0, &msg) == SPIRA_E_LIMIT);
    CHECK(gather_check(true, true, true, 4, 1, 1, 0, 0, 0xFFFFFFFCu, 0, &msg) == 0);
    CHECK(gather_check(true, true, true, 4, 1, 1, 0, 0, 0xFFFFFFFDu, 0, &msg) == SPIRA_E_LIMIT);
    CHECK(gather_check(true, true, true, 4, 8, 1, 0, SPIRA_MAX_SPP - 8, 0, 0, &msg) == 0);
    CHECK(gather_check(true, true, true, 4, 8, 1, 0, SPIRA_MAX_SPP - 7, 0, 0, &msg) == SPIRA_E_LIMIT);
    const double inf = __builtin_inf(), nan = __builtin_nan("");
    CHECK(gather_visible_check(true, true, true, 4, 8, 0, 0, 0, 1e-3, inf, &msg) == 0);
    CHECK(gather_visible_check(true, true, true, 4, 8, 0, 0, SPIRA_CAST_INPLACE, 0.0, 0.0, &msg) == 0);
    CHECK(gather_visible_check(false, true, true, 4, 8, 0, 0, 0, 1e-3, inf, &msg) == SPIRA_E_INVALID);
    CHECK(gather_visible_check(true, false, true, 4, 8, 0, 0, 0, 1e-3, inf, &msg) == SPIRA_E_INVALID);
    CHECK(gather_visible_check(true, true, false, 4, 8, 0, 0, 0, 1e-3, inf, &msg) == SPIRA_E_INVALID);
    CHECK(gather_visible_check(true, true, true, 0, 8, 0, 0, 0, 1e-3, inf, &msg) == SPIRA_E_INVALID);
    CHECK(gather_visible_check(true, true, true, 4, 0, 0, 0, 0, 1e-3, inf, &msg) == SPIRA_E_INVALID);
    CHECK(gather_visible_check(true, true, true, 4, 8, 0, 0, 0, nan, inf, &msg) == SPIRA_E_INVALID);
    CHECK(gather_visible_check(true, true, true, 4, 8, 0, 0, 0, 1e-3, nan, &msg) == SPIRA_E_INVALID);
    CHECK(gather_visible_check(true, true, true, 4, 8, 0, 0, 0, -1e-9, inf, &msg) == SPIRA_E_INVALID);
    CHECK(gather_visible_check(true, true, true, 4, 8, 0, 0, 0, 1.0, 0.5, &msg) == SPIRA_E_INVALID);
    CHECK(gather_visible_check(true, true, true, 4, 8, 0, 0, 0x2, 1e-3, inf, &msg) == SPIRA_E_INVALID);
    CHECK(gather_visible_check(true, true, true, SPIRA_MAX_RAYS + 1, 8, 0, 0, 0, 1e-3, inf, &msg) == SPIRA_E_LIMIT);
    CHECK(gather_visible_check(true, true, true, 4, 8, 0, 0xFFFFFFFDu, 0, 1e-3, inf, &msg) == SPIRA_E_LIMIT);
    CHECK(gather_visible_check(true, true, true, 4, 8, SPIRA_MAX_SPP - 8, 0, 0, 1e-3, inf, &msg) == 0);
    CHECK(gather_visible_check(true, true, true, 4, 8, SPIRA_MAX_SPP - 7, 0, 0, 1e-3, inf, &msg) == SPIRA_E_LIMIT);
    CHECK(gather_rays_check(true, true, 4, 0, 0, &msg) == 0);
    CHECK(gather_rays_check(false, true, 4, 0, 0, &msg) == SPIRA_E_INVALID);
    CHECK(gather_rays_check(true, false, 4, 0, 0, &msg) == SPIRA_E_INVALID);
    CHECK(gather_rays_check(true, true, 0, 0, 0, &msg) == SPIRA_E_INVALID);
    CHECK(gather_rays_check(true, true, SPIRA_MAX_RAYS, SPIRA_MAX_SPP - 1, 0, &msg) == 0);
    CHECK(gather_rays_check(true, true, SPIRA_MAX_RAYS + 1, 0, 0, &msg) == SPIRA_E_LIMIT);
    CHECK(gather_rays_check(true, true, 4, SPIRA_MAX_SPP, 0, &msg) == SPIRA_E_LIMIT);
    CHECK(gather_rays_check(true, true, 4, 0, 0xFFFFFFFDu, &msg) == SPIRA_E_LIMIT);
}

template <class T, class U> static T from_bits(U w) { T v; std::memcpy(&v, &w, sizeof v); return v; }
template <class T, class U> static U to_bits(T v) { U w; std::memcpy(&w, &v, sizeof w); return w; }

template <class T, class U> static void run_inputs() {
    char line[4096];
    while (std::fgets(line, sizeof line, stdin)) {
        char *tok = std::strtok(line, " \n");
        if (!tok) continue;
        const std::string kind = tok;
        std::vector<unsigned long long> w;
        while ((tok = std::strtok(nullptr, " \n"))) w.push_back(std::strtoull(tok, nullptr, 16));
        if (kind == "gen") {
            CHECK(w.size() == 3 + 6);
            const uint32_t sample = (uint32_t)w[0], key0 = (uint32_t)w[2];
            const uint64_t seed = w[1];
            T pt[6], out6[6], d[3] = {0, 0, 0};
            for (int k = 0; k < 6; ++k) pt[k] = from_bits<T, U>((U)w[3 + k]);
            uint32_t sA, sB;
            spira::seed_halves(seed, sA, sB);
            const bool ok = spira::gather_ray_generate<T>(pt, sA, sB, key0, sample, out6, d);
            std::printf("gen %d", ok ? 1 : 0);
            for (int c = 0; c < 6; ++c) std::printf(" %llx", (unsigned long long)to_bits<T, U>(out6[c]));
            for (int c = 0; c < 3; ++c) std::printf(" %llx", (unsigned long long)to_bits<T, U>(d[c]));
            std::printf("\n");
        } else CHECK(false);
    }
}

int main() {
    sweep_plans();
    char prec[16] = {0};
    if (std::scanf("%15s\n", prec) == 1) {
        if (!std::strcmp(prec, "f32")) run_inputs<float, uint32_t>();
        else if (!std::strcmp(prec, "f64")) run_inputs<double, uint64_t>();
        else CHECK(false);
    }
    std::printf("%ld checks, all checks passed\n", g_checks);
    return 0;
}
