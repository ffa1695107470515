// radiance_plan.cpp — the host arithmetic of spira_scene_radiance_* and spira_camera_rays_* as a stand-alone CPU program, built with
// -fsanitize=address,undefined by tests/test_radiance_cpu.py and run directly:
//   1. make_radiance_plan (spira_plan.h) swept over ray counts, sample counts, caps and grids: every item (ray, sample) is covered exactly once, passes
//      ascend and are contiguous, the workspace stays within the cap, the grid never exceeds the items or the device;
//   2. radiance_check / camera_rays_check on their edges;
//   3. radiance_ray_prepare and camera_ray_generate (spira_radiance.h — the very functions the kernels call) over the inputs on stdin, printing bits:
//        line 1:  f32|f64
//        "ray w0 .. w5"                                   six words in hex                  -> "ray <valid> d0 d1 d2"
//        "cam model W H sample seed row0 rows R c0 .. c11" R and the camera as words in hex -> "gen k w0 .. w5" for every ray of the rows
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../julia-spira_amd/csrc/spira_plan.h"
#include "../../julia-spira_amd/csrc/spira_radiance.h"

static long g_checks = 0;
#define CHECK(c)                                                                         \
    do {                                                                                 \
        ++g_checks;                                                                      \
        if (!(c)) { std::printf("CHECK FAILED line %d: %s\n", __LINE__, #c); std::exit(1); } \
    } while (0)

static void sweep_plans() {
    using namespace spira;
    const uint32_t ns[] = {1, 63, 64, 65, 1000, 1u << 26};
    const uint32_t spps[] = {1, 2, 3, 7, 8, 64, 1000, 1u << 24};
    const uint32_t caps[] = {0, 1, 999, 1000, 3000, 65536, 1u << 26, 0xFFFFFFFFu};
    const uint32_t wpcs[] = {0, 1, 16, 64, 1u << 20};
    const uint32_t cus[] = {0, 1, 256};
    long plans = 0;
    for (uint32_t n : ns) for (uint32_t spp : spps) for (uint32_t cap : caps) for (uint32_t wpc : wpcs) for (uint32_t cu : cus) {
        RadianceKnobs k; k.max_items = cap; k.waves_per_cu = wpc;
        const RadiancePlan p = make_radiance_plan(n, spp, cu, 256, k);
        ++plans;
        CHECK(p.max_items >= 1 && p.max_items <= kRadianceMaxItems && (cap == 0 || p.max_items <= cap));
        CHECK(p.spp_pass >= 1 && p.spp_pass <= spp && p.n_pass >= 1);
        CHECK(p.direct == (p.spp_pass == 1));
        CHECK(p.ws_entries == (p.direct ? 0 : (uint64_t)n * p.spp_pass));
        CHECK(p.ws_entries <= p.max_items);                                    // the workspace stays within the cap
        CHECK((uint64_t)n * p.spp_pass <= (1ull << 32) - (1u << 28));          // an item index (+ a grid's stride) fits 32 bits
        CHECK((uint64_t)n * p.spp_pass <= kRadianceMaxItems || p.direct);
        // the passes: ascending, contiguous, covering [0, spp) exactly once
        uint64_t next = 0, items = 0;
        const uint32_t walk = p.n_pass <= 4096 ? p.n_pass : 4096;             // (2^24 direct passes: the first 4096 and the last one, the rest by arithmetic)
        for (uint32_t q = 0; q < walk; ++q) {
            CHECK(p.first(q) == next && p.count(q) >= 1 && p.count(q) <= p.spp_pass);
            CHECK(p.items(q) == (uint64_t)n * p.count(q));
            next += p.count(q); items += p.items(q);
        }
        if (walk < p.n_pass) {
            CHECK(p.count(p.n_pass - 1) >= 1 && (uint64_t)p.first(p.n_pass - 1) + p.count(p.n_pass - 1) == spp);
            CHECK((uint64_t)(p.n_pass - 1) * p.spp_pass < spp);
        } else {
            CHECK(next == spp && items == (uint64_t)n * spp);
        }
        CHECK((uint64_t)(p.n_pass - 1) * p.spp_pass < spp && (uint64_t)p.n_pass * p.spp_pass >= spp);
        // within a pass item = ray * count + s: the decode covers every (ray, s) once
        if ((uint64_t)n * p.spp_pass <= 4096) {
            std::vector<uint8_t> seen((size_t)n * p.spp_pass, 0);
            const FastDiv fd = fastdiv_make(p.spp_pass);
            for (uint32_t i = 0; i < n * p.spp_pass; ++i) {
                const uint32_t ray = fastdiv(i, fd), s = i - ray * p.spp_pass;
                CHECK(ray < n && s < p.spp_pass && !seen[(size_t)ray * p.spp_pass + s]);
                seen[(size_t)ray * p.spp_pass + s] = 1;
            }
        }
        CHECK(p.wpb == 4 && p.grid >= 1 && p.grid <= (1u << 20) && p.grid_flat >= 1);
        CHECK((uint64_t)(p.grid - 1) * 256 < (uint64_t)n * p.spp_pass);          // no workgroup without an item
        if (wpc == 0) CHECK(p.grid == 1);
        else CHECK(p.grid <= (uint64_t)(cu ? cu : 1) * wpc / 4 || p.grid == 1);
    }
    std::printf("%ld plans checked\n", plans);

    const char *msg = nullptr;
    CHECK(radiance_check(true, true, true, 4, 1, 1, 0, 0, 0, 0, &msg) == 0);
    CHECK(radiance_check(false, true, true, 4, 1, 1, 0, 0, 0, 0, &msg) == SPIRA_E_INVALID);
    CHECK(radiance_check(true, false, true, 4, 1, 1, 0, 0, 0, 0, &msg) == SPIRA_E_INVALID);
    CHECK(radiance_check(true, true, false, 4, 1, 1, 0, 0, 0, 0, &msg) == SPIRA_E_INVALID);
    CHECK(radiance_check(true, true, true, 0, 1, 1, 0, 0, 0, 0, &msg) == SPIRA_E_INVALID);
    CHECK(radiance_check(true, true, true, 4, 0, 1, 0, 0, 0, 0, &msg) == SPIRA_E_INVALID);
    CHECK(radiance_check(true, true, true, 4, 1, 0, 0, 0, 0, 0, &msg) == SPIRA_E_INVALID);
    CHECK(radiance_check(true, true, true, 4, 1, 256, 0, 0, 0, 0, &msg) == SPIRA_E_INVALID);
    CHECK(radiance_check(true, true, true, 4, 1, 255, 0, 0, 0, 0, &msg) == 0);
    CHECK(radiance_check(true, true, true, 4, 1, 1, 0, 0, 0, 1, &msg) == SPIRA_E_INVALID);
    CHECK(radiance_check(true, true, true, 4, 1, 1, SPIRA_EXT_DIELECTRIC | SPIRA_EXT_SPECTRAL, 0, 0, 0, &msg) == 0);
    CHECK(radiance_check(true, true, true, 4, 1, 1, SPIRA_KERNEL_MEGA, 0, 0, 0, &msg) == SPIRA_E_UNSUPPORTED);
    CHECK(radiance_check(true, true, true, 4, 1, 1, SPIRA_SEM_CPU, 0, 0, 0, &msg) == SPIRA_E_UNSUPPORTED);
    CHECK(radiance_check(true, true, true, SPIRA_MAX_RAYS, 1, 1, 0, 0, 0, 0, &msg) == 0);
    CHECK(radiance_check(true, true, true, SPIRA_MAX_RAYS + 1, 1, 1, 0, 0, 0, 0, &msg) == SPIRA_E_LIMIT);
    CHECK(radiance_check(true, true, true, 4, 1, 1, 0, 0, 0xFFFFFFFCu, 0, &msg) == 0);
    CHECK(radiance_check(true, true, true, 4, 1, 1, 0, 0, 0xFFFFFFFDu, 0, &msg) == SPIRA_E_LIMIT);
    CHECK(radiance_check(true, true, true, 4, 8, 1, 0, SPIRA_MAX_SPP - 8, 0, 0, &msg) == 0);
    CHECK(radiance_check(true, true, true, 4, 8, 1, 0, SPIRA_MAX_SPP - 7, 0, 0, &msg) == SPIRA_E_LIMIT);
    uint32_t rows = 0;
    CHECK(camera_rays_check(0, 33, 17, 0, 0, 0, 0.0, &rows, &msg) == 0 && rows == 17);
    CHECK(camera_rays_check(2, 33, 17, 0, 6, 11, 0.5, &rows, &msg) == 0 && rows == 11);
    CHECK(camera_rays_check(3, 33, 17, 0, 0, 0, 0.0, &rows, &msg) == SPIRA_E_INVALID);
    CHECK(camera_rays_check(0, 1, 17, 0, 0, 0, 0.0, &rows, &msg) == SPIRA_E_INVALID);
    CHECK(camera_rays_check(0, 33, 1, 0, 0, 0, 0.0, &rows, &msg) == SPIRA_E_INVALID);
    CHECK(camera_rays_check(1, 33, 17, 0, 0, 0, -1e-9, &rows, &msg) == SPIRA_E_INVALID);
    CHECK(camera_rays_check(1, 33, 17, 0, 0, 0, __builtin_nan(""), &rows, &msg) == SPIRA_E_INVALID);
    CHECK(camera_rays_check(1, 33, 17, 0, 0, 0, __builtin_inf(), &rows, &msg) == SPIRA_E_INVALID);
    CHECK(camera_rays_check(0, 33, 17, 0, 7, 11, 0.0, &rows, &msg) == SPIRA_E_INVALID);
    CHECK(camera_rays_check(0, 33, 17, 0, 0xFFFFFFFFu, 2, 0.0, &rows, &msg) == SPIRA_E_INVALID);
    CHECK(camera_rays_check(0, 65536, 65536, 0, 0, 1, 0.0, &rows, &msg) == SPIRA_E_LIMIT);
    CHECK(camera_rays_check(0, 33, 17, SPIRA_MAX_SPP, 0, 0, 0.0, &rows, &msg) == SPIRA_E_LIMIT);
    CHECK(camera_rays_check(0, 16384, 8192, 0, 0, 0, 0.0, &rows, &msg) == SPIRA_E_LIMIT);
    CHECK(camera_rays_check(0, 16384, 8192, 0, 4096, 4096, 0.0, &rows, &msg) == 0 && rows == 4096);
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
        if (kind == "ray") {
            CHECK(w.size() == 6);
            T r[6], d[3] = {0, 0, 0};
            for (int k = 0; k < 6; ++k) r[k] = from_bits<T, U>((U)w[k]);
            const bool ok = spira::radiance_ray_prepare<T>(r, d);
            std::printf("ray %d %llx %llx %llx\n", ok ? 1 : 0, (unsigned long long)to_bits<T, U>(d[0]), (unsigned long long)to_bits<T, U>(d[1]),
                        (unsigned long long)to_bits<T, U>(d[2]));
        } else if (kind == "cam") {
            CHECK(w.size() == 8 + 12);
            const uint32_t model = (uint32_t)w[0], W = (uint32_t)w[1], H = (uint32_t)w[2], sample = (uint32_t)w[3], row0 = (uint32_t)w[5], rows_in = (uint32_t)w[6];
            const uint64_t seed = w[4];
            const T R = from_bits<T, U>((U)w[7]);
            T cam[12];
            for (int k = 0; k < 12; ++k) cam[k] = from_bits<T, U>((U)w[8 + k]);
            uint32_t rows = 0, sA, sB;
            const char *msg = nullptr;
            CHECK(spira::camera_rays_check(model, W, H, sample, row0, rows_in, (double)R, &rows, &msg) == 0);
            spira::seed_halves(seed, sA, sB);
            std::vector<T> out((size_t)rows * W * 6);
            for (uint32_t r = 0; r < rows; ++r)
                for (uint32_t ix = 0; ix < W; ++ix)
                    spira::camera_ray_generate<T>(cam, model, W, H, sA, sB, ix, (rows_in ? row0 : 0) + r, sample, R, out.data() + 6 * ((size_t)r * W + ix));
            for (size_t k = 0; k < (size_t)rows * W; ++k) {
                std::printf("gen %zu", k);
                for (int c = 0; c < 6; ++c) std::printf(" %llx", (unsigned long long)to_bits<T, U>(out[6 * k + c]));
                std::printf("\n");
            }
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
