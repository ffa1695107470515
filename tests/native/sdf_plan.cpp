// sdf_plan.cpp — host-only harness built with -fsanitize=address,undefined (tests/test_sdf_cpu.py), in the manner of knearest_plan.cpp: the argument rules of
// spira_scene_signed_distance_* (spira_plan.h, signed_distance_check and signed_distance_wants_nearest) and the HIP-free part of spira_sdf.h — the three
// rays a point gets and the vote.
//   check     signed_distance_check swept over its arguments: every rule returns its own code; the 32 NULL-output combinations
//   rays      prints, per precision and ray j, the bit patterns of the ray sdf_ray makes for a point and of the unit direction cast_ray_prepare gives it
//             ("ray f32 j r0 .. r7 | d0 d1 d2", hexadecimal), which the test compares with spira_hip.query.INSIDE_DIRECTIONS under normalize_rays
//   vote      sdf_needs_third and sdf_mesh_inside on every pair of small counts, against the majority of three parities
#include <cinttypes>
#include <cstdint>
#include <cstdio>
#include <cstring>

#include "../../julia-spira_amd/csrc/spira_plan.h"
#include "../../julia-spira_amd/csrc/spira_sdf.h"

static int failures = 0;
#define CHECK(c, ...) do { if (!(c)) { ++failures; std::printf("FAILED %s:%d %s: ", __FILE__, __LINE__, #c); std::printf(__VA_ARGS__); std::printf("\n"); } } while (0)

static void check_rules() {
    const char *msg = nullptr;
    const uint32_t IN = SPIRA_CAST_INPLACE;
    CHECK(spira::signed_distance_check(false, 4, 0, true, &msg) == SPIRA_E_INVALID && std::strstr(msg, "point array is NULL"), "%s", msg);
    CHECK(spira::signed_distance_check(true, 0, 0, true, &msg) == SPIRA_E_INVALID && std::strstr(msg, "n_points is 0"), "%s", msg);
    for (uint32_t f : {2u, 4u, 8u, 0x80000000u, 0x13u, 0x3u})
        CHECK(spira::signed_distance_check(true, 4, f, true, &msg) == SPIRA_E_INVALID && std::strstr(msg, "unknown flag bits"), "%x %s", f, msg);
    for (uint32_t f : {0u, IN}) CHECK(spira::signed_distance_check(true, 4, f, true, &msg) == 0, "flags %x", f);
    CHECK(spira::signed_distance_check(true, 4, 0, false, &msg) == SPIRA_E_INVALID && std::strstr(msg, "all NULL"), "%s", msg);
    CHECK(spira::signed_distance_check(true, SPIRA_MAX_RAYS, 0, true, &msg) == 0, "the limit itself");
    CHECK(spira::signed_distance_check(true, SPIRA_MAX_RAYS + 1, IN, true, &msg) == SPIRA_E_LIMIT && std::strstr(msg, "SPIRA_MAX_RAYS"), "%s", msg);
    CHECK(spira::signed_distance_check(true, 0xFFFFFFFFu, 0, true, &msg) == SPIRA_E_LIMIT, "2^32 - 1");
    // the order of the rules: an argument error is reported before the limit, NULL points before everything
    CHECK(spira::signed_distance_check(false, 0, 2, false, &msg) == SPIRA_E_INVALID && std::strstr(msg, "point array is NULL"), "%s", msg);
    CHECK(spira::signed_distance_check(true, SPIRA_MAX_RAYS + 1, 0, false, &msg) == SPIRA_E_INVALID && std::strstr(msg, "all NULL"), "%s", msg);
    // the NULL-output combinations as the entry forms them: prim, dist, point, inside, crossings (trips alone is no output)
    int accepted = 0, sign_only = 0;
    for (uint32_t m = 0; m < 32; ++m) {
        const bool prim = m & 1, dist = m & 2, point = m & 4, inside = m & 8, crossings = m & 16;
        const int rc = spira::signed_distance_check(true, 4, 0, prim || dist || point || inside || crossings, &msg);
        CHECK(rc == (m ? 0 : SPIRA_E_INVALID), "outputs %x: %d", m, rc);
        accepted += rc == 0;
        const bool near = spira::signed_distance_wants_nearest(prim, dist, point);
        CHECK(near == ((m & 7) != 0), "outputs %x", m);
        sign_only += rc == 0 && !near;
    }
    CHECK(accepted == 31 && sign_only == 3, "%d %d", accepted, sign_only);
    CHECK(spira::kSdfSkipped == SPIRA_SDF_SKIPPED, "the constant");
    std::printf("rules checked\n");
}

template <class T, class U>
static void print_rays(const char *prec) {
    const T p[3] = {(T)0.25, (T)-1.5, (T)3.0};
    for (int j = 0; j < 3; ++j) {
        T r[8], d[3] = {0, 0, 0};
        const T fr[4] = {0, 0, 0, 1};
        spira::sdf_ray<T>(p, j, r);
        CHECK(spira::cast_ray_prepare<T>(r, false, fr, d), "ray %d of a valid point is valid", j);
        std::printf("ray %s %d", prec, j);
        for (int k = 0; k < 8; ++k) { U b; std::memcpy(&b, &r[k], sizeof b); std::printf(" %" PRIx64, (uint64_t)b); }
        std::printf(" |");
        for (int k = 0; k < 3; ++k) { U b; std::memcpy(&b, &d[k], sizeof b); std::printf(" %" PRIx64, (uint64_t)b); }
        std::printf("\n");
    }
}

static void check_vote() {
    for (uint32_t c0 = 0; c0 < 6; ++c0)
        for (uint32_t c1 = 0; c1 < 6; ++c1)
            for (uint32_t c2 = 0; c2 < 6; ++c2) {
                const bool third = spira::sdf_needs_third(c0, c1);
                CHECK(third == ((c0 % 2) != (c1 % 2)), "%u %u", c0, c1);
                const uint32_t slot2 = third ? c2 : spira::kSdfSkipped;
                const bool majority = (c0 % 2) + (c1 % 2) + (c2 % 2) >= 2;
                CHECK(spira::sdf_mesh_inside(c0, slot2) == majority, "%u %u %u", c0, c1, c2);
            }
    std::printf("vote checked\n");
}

int main() {
    check_rules();
    print_rays<float, uint32_t>("f32");
    print_rays<double, uint64_t>("f64");
    check_vote();
    if (failures) { std::printf("%d checks FAILED\n", failures); return 1; }
    std::printf("all checks passed\n");
    return 0;
}
