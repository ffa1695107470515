// cast_plan.cpp — host-only harness built with -fsanitize=address,undefined (tests/test_cast_cpu.py), in the manner of refit_plan.cpp: the launch plan of
// the ray-query entries (spira_plan.h, make_cast_plan) and the very function their kernels classify and normalise a ray with (spira_query.h,
// cast_ray_prepare).
//   plan      for n_rays in {1, 63, 64, 65, 4 097, 20 011, 2^26} and 1 / 256 compute units: the wave ranges are disjoint, in order, cover [0, n) exactly,
//             and no wave is empty unless n < waves; a list of at least 128 rays gives every wave more rays than it has lanes
//   prepare   reads rays from stdin — a line "f32|f64 frame cx cy cz scale" then lines of 8 values as hexadecimal bit patterns — and prints per ray
//             the verdict and the bits of the unit direction, which tests/test_cast_cpu.py compares with spira_hip.query.normalize_rays
#include <cinttypes>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../julia-spira_amd/csrc/spira_plan.h"
#include "../../julia-spira_amd/csrc/spira_query.h"

static int failures = 0;
#define CHECK(c, ...) do { if (!(c)) { ++failures; std::printf("FAILED %s:%d %s: ", __FILE__, __LINE__, #c); std::printf(__VA_ARGS__); std::printf("\n"); } } while (0)

static void check_plans() {
    const uint32_t sizes[] = {1u, 63u, 64u, 65u, 4097u, 20011u, 1u << 26};
    const uint32_t cus[] = {1u, 256u};
    for (uint32_t n : sizes)
        for (uint32_t cu : cus)
            for (uint32_t refill : {8u, 16u, 32u, 0u, 1000u}) {
                spira::CastKnobs k; k.refill = refill;
                const spira::CastPlan p = spira::make_cast_plan(n, cu, 256, k);
                CHECK(p.grid >= 1 && p.wpb == 4 && p.waves == p.grid * p.wpb && p.waves <= std::max(4u, cu * k.waves_per_cu), "n %u cu %u: grid %u waves %u", n, cu, p.grid, p.waves);
                CHECK(p.refill_free >= 1 && p.refill_free <= 64, "refill %u -> %u", refill, p.refill_free);
                CHECK(p.grid_flat >= 1 && (uint64_t)p.grid_flat * 256 < (1ull << 31), "grid_flat %u", p.grid_flat);
                uint64_t at = 0; uint32_t empty = 0, least = ~0u;
                for (uint32_t w = 0; w < p.waves; ++w) {
                    CHECK(p.begin(w) == at, "n %u cu %u wave %u begins at %u, the previous one ended at %" PRIu64, n, cu, w, p.begin(w), at);
                    at += p.count(w);
                    empty += p.count(w) == 0;
                    least = std::min(least, p.count(w));
                }
                CHECK(at == n, "n %u cu %u: the ranges cover %" PRIu64, n, cu, at);
                CHECK(empty == 0 || n < p.waves, "n %u cu %u: %u empty waves of %u", n, cu, empty, p.waves);
                if (n >= spira::kCastMinRaysPerWave * p.wpb) CHECK(least > 64, "n %u cu %u: a wave with %u rays", n, cu, least);
            }
    std::printf("plans checked\n");
}

template <class T, class U> static void prepare_lines(bool frame, const double fr64[4]) {
    const T fr[4] = {(T)fr64[0], (T)fr64[1], (T)fr64[2], (T)fr64[3]};
    char line[512];
    while (std::fgets(line, sizeof line, stdin)) {
        unsigned long long w[8];
        if (std::sscanf(line, "%llx %llx %llx %llx %llx %llx %llx %llx", w, w + 1, w + 2, w + 3, w + 4, w + 5, w + 6, w + 7) != 8) continue;
        T r[8], d[3] = {0, 0, 0};
        for (int k = 0; k < 8; ++k) { const U u = (U)w[k]; std::memcpy(&r[k], &u, sizeof(T)); }
        const bool ok = spira::cast_ray_prepare<T>(r, frame, fr, d);
        U b[3];
        for (int k = 0; k < 3; ++k) std::memcpy(&b[k], &d[k], sizeof(T));
        std::printf("ray %d %llx %llx %llx\n", ok ? 1 : 0, (unsigned long long)b[0], (unsigned long long)b[1], (unsigned long long)b[2]);
    }
}

int main() {
    check_plans();
    char prec[8] = {0};
    int frame = 0;
    double fr[4] = {0, 0, 0, 1};
    if (std::scanf("%7s %d %lf %lf %lf %lf\n", prec, &frame, fr, fr + 1, fr + 2, fr + 3) == 6) {
        if (std::string(prec) == "f32") prepare_lines<float, uint32_t>(frame != 0, fr);
        else prepare_lines<double, uint64_t>(frame != 0, fr);
    }
    if (failures) { std::printf("%d checks FAILED\n", failures); return 1; }
    std::printf("all checks passed\n");
    return 0;
}
