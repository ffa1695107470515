// trioverlap_plan.cpp — host-only harness built with -fsanitize=address,undefined (tests/test_trioverlap_cpu.py), in the manner of overlap_plan.cpp: the very
// functions the triangle overlap kernels call (spira_trioverlap.h) — trioverlap_prepare (the edges, their cross product, the verdict), overlap_tri_triangle,
// overlap_tri_sphere — on a table read from stdin, and the argument rules of the entries (spira_plan.h, overlap_tri_check) swept over their arguments.  A
// line "f32|f64 frame cx cy cz scale", then lines of hexadecimal bit patterns:
//   Q query[10]                      -> "tq <verdict with the frame> <verdict without> g1[3] g2[3] m[3]"   (bits; 0 where the query is invalid without a frame)
//   T v0[3] e1[3] e2[3] query[10]    -> "tri <1 | 0 | -3>"     (the query prepared without a frame, as the exported host functions do)
//   S c[3] R query[10]               -> "sph <1 | 0 | -3>"
// tests/test_trioverlap_cpu.py compares them with the numpy twins of spira_hip.query.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>

#include "../../julia-spira_amd/csrc/spira_plan.h"
#include "../../julia-spira_amd/csrc/spira_trioverlap.h"

static int failures = 0;
#define CHECK(c, ...) do { if (!(c)) { ++failures; std::printf("FAILED %s:%d %s: ", __FILE__, __LINE__, #c); std::printf(__VA_ARGS__); std::printf("\n"); } } while (0)

static void check_rules() {
    const char *msg = nullptr;
    CHECK(spira::overlap_tri_check(false, 4, 4, 0, true, &msg) == SPIRA_E_INVALID && std::strstr(msg, "query triangle array is NULL"), "%s", msg);
    CHECK(spira::overlap_tri_check(true, 0, 4, 0, true, &msg) == SPIRA_E_INVALID && std::strstr(msg, "n is 0"), "%s", msg);
    for (uint32_t f : {2u, 4u, 0x80000000u, 0x13u}) CHECK(spira::overlap_tri_check(true, 4, 4, f, true, &msg) == SPIRA_E_INVALID && std::strstr(msg, "unknown flag bits"), "%x %s", f, msg);
    for (uint32_t f : {0u, (uint32_t)SPIRA_CAST_INPLACE}) CHECK(spira::overlap_tri_check(true, 4, 4, f, true, &msg) == 0, "flags %x", f);
    for (uint32_t k = 0; k <= SPIRA_MAX_OVERLAP; ++k) CHECK(spira::overlap_tri_check(true, 4, k, 0, true, &msg) == 0, "max_list %u", k);
    CHECK(spira::overlap_tri_check(true, 4, SPIRA_MAX_OVERLAP + 1, 0, true, &msg) == SPIRA_E_INVALID && std::strstr(msg, "SPIRA_MAX_OVERLAP"), "%s", msg);
    CHECK(spira::overlap_tri_check(true, 4, 4, 0, false, &msg) == SPIRA_E_INVALID && std::strstr(msg, "every output is NULL"), "%s", msg);
    CHECK(spira::overlap_tri_check(true, 4, 0, 0, false, &msg) == SPIRA_E_INVALID && std::strstr(msg, "out_count is NULL"), "%s", msg);
    CHECK(spira::overlap_tri_check(true, SPIRA_MAX_RAYS, 1, 0, true, &msg) == 0, "the limit itself");
    CHECK(spira::overlap_tri_check(true, SPIRA_MAX_RAYS, 0, 0, true, &msg) == 0, "the limit itself, count only");
    CHECK(spira::overlap_tri_check(true, SPIRA_MAX_RAYS + 1, 0, 0, true, &msg) == SPIRA_E_LIMIT && std::strstr(msg, "query triangles"), "%s", msg);
    CHECK(spira::overlap_tri_check(true, SPIRA_MAX_RAYS / 16, 16, 0, true, &msg) == 0, "the slot limit itself");
    CHECK(spira::overlap_tri_check(true, SPIRA_MAX_RAYS / 16 + 1, 16, 0, true, &msg) == SPIRA_E_LIMIT && std::strstr(msg, "n * max_list"), "%s", msg);
    CHECK(spira::overlap_tri_check(true, 0xFFFFFFFFu, 16, 0, true, &msg) == SPIRA_E_LIMIT, "the product is formed in 64 bits");
    // every case decided as the box query decides it
    for (uint32_t n : {0u, 4u, (uint32_t)SPIRA_MAX_RAYS + 1u})
        for (uint32_t k : {0u, 4u, 16u, 17u})
            for (uint32_t f : {0u, 1u, 2u})
                for (int out = 0; out < 2; ++out) {
                    const char *m2 = nullptr;
                    CHECK(spira::overlap_tri_check(true, n, k, f, out != 0, &msg) == spira::overlap_check(true, n, k, f, out != 0, &m2), "n %u k %u f %u out %d", n, k, f, out);
                }
}

template <class T, class U> static void bits(T v) { U b; std::memcpy(&b, &v, sizeof(T)); std::printf(" %llx", (unsigned long long)b); }

template <class T, class U> static int lines(bool frame, const double fr64[4]) {
    const T fr[4] = {(T)fr64[0], (T)fr64[1], (T)fr64[2], (T)fr64[3]};
    char line[2048];
    int n = 0;
    while (std::fgets(line, sizeof line, stdin)) {
        unsigned long long w[19];
        char kind = 0;
        const int got = std::sscanf(line, " %c %llx %llx %llx %llx %llx %llx %llx %llx %llx %llx %llx %llx %llx %llx %llx %llx %llx %llx %llx", &kind, w, w + 1, w + 2, w + 3,
                                    w + 4, w + 5, w + 6, w + 7, w + 8, w + 9, w + 10, w + 11, w + 12, w + 13, w + 14, w + 15, w + 16, w + 17, w + 18);
        T v[19];
        for (int k = 0; k < 19; ++k) { const U u = k < got - 1 ? (U)w[k] : (U)0; std::memcpy(&v[k], &u, sizeof(T)); }
        spira::TriQuery<T> Q{};
        if (kind == 'Q' && got == 11) {
            spira::TriQuery<T> Qf{};
            const bool with = spira::trioverlap_prepare<T>(v, frame, fr, Qf), without = spira::trioverlap_prepare<T>(v, false, nullptr, Q);
            std::printf("tq %d %d", with ? 1 : 0, without ? 1 : 0);
            for (int k = 0; k < 3; ++k) bits<T, U>(without ? Q.g1[k] : (T)0);
            for (int k = 0; k < 3; ++k) bits<T, U>(without ? Q.g2[k] : (T)0);
            for (int k = 0; k < 3; ++k) bits<T, U>(without ? Q.m[k] : (T)0);
            std::printf("\n");
        } else if (kind == 'T' && got == 20) {
            const bool ok = spira::trioverlap_prepare<T>(v + 9, false, nullptr, Q);
            std::printf("tri %d\n", !ok ? -3 : (spira::overlap_tri_triangle<T>(Q, v, v + 3, v + 6) ? 1 : 0));
        } else if (kind == 'S' && got == 15) {
            const bool ok = spira::trioverlap_prepare<T>(v + 4, false, nullptr, Q);
            std::printf("sph %d\n", !ok ? -3 : (spira::overlap_tri_sphere<T>(Q, v, v[3]) ? 1 : 0));
        } else continue;
        ++n;
    }
    return n;
}

int main() {
    check_rules();
    char prec[8] = {0};
    int frame = 0, n = 0;
    double fr[4] = {0, 0, 0, 1};
    if (std::scanf("%7s %d %lf %lf %lf %lf\n", prec, &frame, fr, fr + 1, fr + 2, fr + 3) == 6) {
        if (std::string(prec) == "f32") n = lines<float, uint32_t>(frame != 0, fr);
        else n = lines<double, uint64_t>(frame != 0, fr);
    }
    std::printf("%d lines answered\n", n);
    if (failures) { std::printf("%d checks FAILED\n", failures); return 1; }
    std::printf("all checks passed\n");
    return 0;
}
