// probe_plan.cpp — the host arithmetic of spira_scene_probe_sh_*, spira_probe_rays_* and spira_sh9_basis_* as a stand-alone CPU program, built with
// -fsanitize=address,undefined by tests/test_probe_cpu.py and run directly:
//   1. probe_check (spira_plan.h) on its edges: the gather's codes in the gather's order;
//   2. sh9_basis (spira_probe.h) at the six axis directions against the closed forms;
//   3. probe_ray_generate and sh9_basis (spira_probe.h — the very functions the kernels and the host entries call) over the inputs on stdin, printing bits:
//        line 1:  f32|f64
//        "gen sample seed key w0 w1 w2"   the three values of a point as words in hex -> "gen <valid> r0 .. r5 d0 d1 d2 y0 .. y8"
//      (d: the unit direction radiance_ray_prepare gives for the generated ray — the one the probe kernels trace along; y: sh9_basis at d)
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../julia-spira_amd/csrc/spira_plan.h"
#include "../../julia-spira_amd/csrc/spira_probe.h"

static long g_checks = 0;
#define CHECK(c)                                                                         \
    do {                                                                                 \
        ++g_checks;                                                                      \
        if (!(c)) { std::printf("CHECK FAILED line %d: %s\n", __LINE__, #c); std::exit(1); } \
    } while (0)

static void check_rules() {
    using namespace spira;
    const char *msg = nullptr;
    CHECK(probe_check(true, true, true, 4, 1, 1, 0, 0, 0, 0, &msg) == 0);
    CHECK(probe_check(false, true, true, 4, 1, 1, 0, 0, 0, 0, &msg) == SPIRA_E_INVALID && std::strstr(msg, "point array"));
    CHECK(probe_check(false, false, false, 4, 1, 1, 0, 0, 0, 0, &msg) == SPIRA_E_INVALID && std::strstr(msg, "point array"));
    CHECK(probe_check(true, false, false, 4, 1, 1, 0, 0, 0, 0, &msg) == SPIRA_E_INVALID && std::strstr(msg, "struct"));
    CHECK(probe_check(true, true, false, 4, 1, 1, 0, 0, 0, 0, &msg) == SPIRA_E_INVALID && std::strstr(msg, "sum_sh"));
    CHECK(probe_check(true, true, true, 0, 1, 1, 0, 0, 0, 0, &msg) == SPIRA_E_INVALID);
    CHECK(probe_check(true, true, true, 4, 0, 1, 0, 0, 0, 0, &msg) == SPIRA_E_INVALID);
    CHECK(probe_check(true, true, true, 4, 1, 0, 0, 0, 0, 0, &msg) == SPIRA_E_INVALID);
    CHECK(probe_check(true, true, true, 4, 1, 256, 0, 0, 0, 0, &msg) == SPIRA_E_INVALID);
    CHECK(probe_check(true, true, true, 4, 1, 255, 0, 0, 0, 0, &msg) == 0);
    CHECK(probe_check(true, true, true, 4, 1, 1, 0, 0, 0, 1, &msg) == SPIRA_E_INVALID);
    CHECK(probe_check(true, true, true, 4, 1, 1, SPIRA_EXT_DIELECTRIC | SPIRA_EXT_SPECTRAL, 0, 0, 0, &msg) == 0);
    CHECK(probe_check(true, true, true, 4, 1, 1, SPIRA_KERNEL_MEGA, 0, 0, 0, &msg) == SPIRA_E_UNSUPPORTED && std::strstr(msg, "probe"));
    CHECK(probe_check(true, true, true, SPIRA_MAX_RAYS, 1 << 24, 1, 0, 0, 0, 0, &msg) == 0);
    CHECK(probe_check(true, true, true, SPIRA_MAX_RAYS + 1, 1, 1, 0, 0, 0, 0, &msg) == SPIRA_E_LIMIT);
    CHECK(probe_check(true, true, true, 4, 1, 1, 0, 0, 0xFFFFFFFCu, 0, &msg) == 0);
    CHECK(probe_check(true, true, true, 4, 1, 1, 0, 0, 0xFFFFFFFDu, 0, &msg) == SPIRA_E_LIMIT);
    CHECK(probe_check(true, true, true, 4, 8, 1, 0, SPIRA_MAX_SPP - 8, 0, 0, &msg) == 0);
    CHECK(probe_check(true, true, true, 4, 8, 1, 0, SPIRA_MAX_SPP - 7, 0, 0, &msg) == SPIRA_E_LIMIT);
    // the axes: Y1, Y2, Y3 pick y, z, x; the products vanish; Y6 = 2 c3 on +-z and -c3 elsewhere; Y8 = +-c4 on the x and y axes
    const double c0 = 0.28209479177387814, c1 = 0.4886025119029199, c3 = 0.31539156525252005, c4 = 0.5462742152960396;
    for (int axis = 0; axis < 3; ++axis)
        for (int sign = -1; sign <= 1; sign += 2) {
            double d[3] = {0, 0, 0}, Y[9];
            d[axis] = sign;
            sh9_basis<double>(d, Y);
            CHECK(Y[0] == c0 && Y[1] == c1 * d[1] && Y[2] == c1 * d[2] && Y[3] == c1 * d[0]);
            CHECK(Y[4] == 0 && Y[5] == 0 && Y[7] == 0);
            CHECK(Y[6] == (axis == 2 ? c3 * 2.0 : -c3));
            CHECK(Y[8] == (axis == 0 ? c4 : axis == 1 ? -c4 : 0.0));
        }
    std::printf("rules checked\n");
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
            CHECK(w.size() == 3 + 3);
            const uint32_t sample = (uint32_t)w[0], key = (uint32_t)w[2];
            const uint64_t seed = w[1];
            T p[3], out6[6], d[3] = {0, 0, 0}, Y[9];
            for (int k = 0; k < 3; ++k) p[k] = from_bits<T, U>((U)w[3 + k]);
            uint32_t sA, sB;
            spira::seed_halves(seed, sA, sB);
            const bool ok = spira::probe_ray_generate<T>(p, sA, sB, key, sample, out6, d);
            spira::sh9_basis<T>(d, Y);
            std::printf("gen %d", ok ? 1 : 0);
            for (int c = 0; c < 6; ++c) std::printf(" %llx", (unsigned long long)to_bits<T, U>(out6[c]));
            for (int c = 0; c < 3; ++c) std::printf(" %llx", (unsigned long long)to_bits<T, U>(d[c]));
            for (int c = 0; c < 9; ++c) std::printf(" %llx", (unsigned long long)to_bits<T, U>(Y[c]));
            std::printf("\n");
        } else CHECK(false);
    }
}

int main() {
    check_rules();
    char prec[16] = {0};
    if (std::scanf("%15s\n", prec) == 1) {
        if (!std::strcmp(prec, "f32")) run_inputs<float, uint32_t>();
        else if (!std::strcmp(prec, "f64")) run_inputs<double, uint64_t>();
        else CHECK(false);
    }
    std::printf("%ld checks, all checks passed\n", g_checks);
    return 0;
}
