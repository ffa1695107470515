// overlap_plan.cpp — host-only harness built with -fsanitize=address,undefined (tests/test_overlap_cpu.py), in the manner of sweep_plan.cpp: the very
// functions the box overlap kernels call (spira_overlap.h) — overlap_prepare (the axes, the enclosing half extents, the verdict), overlap_box_triangle,
// overlap_box_sphere — on a table read from stdin; the lane's list (overlap_insert) at every capacity against a sort; and the argument rules of the
// entries (spira_plan.h, overlap_check) swept over their arguments.  A line "f32|f64 frame cx cy cz scale", then lines of hexadecimal bit patterns:
//   P box[10]                      -> "bx <verdict with the frame> <verdict without> A[9] He[3]"   (bits; 0 where the box is invalid without a frame)
//   T v0[3] e1[3] e2[3] box[10]    -> "tri <1 | 0 | -3>"     (the box prepared without a frame, as the exported host functions do)
//   S c[3] R box[10]               -> "sph <1 | 0 | -3>"
// tests/test_overlap_cpu.py compares them with the numpy twins of spira_hip.query.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../julia-spira_amd/csrc/spira_plan.h"
#include "../../julia-spira_amd/csrc/spira_overlap.h"

static int failures = 0;
#define CHECK(c, ...) do { if (!(c)) { ++failures; std::printf("FAILED %s:%d %s: ", __FILE__, __LINE__, #c); std::printf(__VA_ARGS__); std::printf("\n"); } } while (0)

static void check_rules() {
    const char *msg = nullptr;
    CHECK(spira::overlap_check(false, 4, 4, 0, true, &msg) == SPIRA_E_INVALID && std::strstr(msg, "box array is NULL"), "%s", msg);
    CHECK(spira::overlap_check(true, 0, 4, 0, true, &msg) == SPIRA_E_INVALID && std::strstr(msg, "n is 0"), "%s", msg);
    for (uint32_t f : {2u, 4u, 0x80000000u, 0x13u}) CHECK(spira::overlap_check(true, 4, 4, f, true, &msg) == SPIRA_E_INVALID && std::strstr(msg, "unknown flag bits"), "%x %s", f, msg);
    for (uint32_t f : {0u, (uint32_t)SPIRA_CAST_INPLACE}) CHECK(spira::overlap_check(true, 4, 4, f, true, &msg) == 0, "flags %x", f);
    for (uint32_t k = 0; k <= SPIRA_MAX_OVERLAP; ++k) CHECK(spira::overlap_check(true, 4, k, 0, true, &msg) == 0, "max_list %u", k);
    CHECK(spira::overlap_check(true, 4, SPIRA_MAX_OVERLAP + 1, 0, true, &msg) == SPIRA_E_INVALID && std::strstr(msg, "SPIRA_MAX_OVERLAP"), "%s", msg);
    CHECK(spira::overlap_check(true, 4, 4, 0, false, &msg) == SPIRA_E_INVALID && std::strstr(msg, "every output is NULL"), "%s", msg);
    CHECK(spira::overlap_check(true, 4, 0, 0, false, &msg) == SPIRA_E_INVALID && std::strstr(msg, "out_count is NULL"), "%s", msg);
    CHECK(spira::overlap_check(true, SPIRA_MAX_RAYS, 1, 0, true, &msg) == 0, "the limit itself");
    CHECK(spira::overlap_check(true, SPIRA_MAX_RAYS, 0, 0, true, &msg) == 0, "the limit itself, count only");
    CHECK(spira::overlap_check(true, SPIRA_MAX_RAYS + 1, 0, 0, true, &msg) == SPIRA_E_LIMIT && std::strstr(msg, "SPIRA_MAX_RAYS"), "%s", msg);
    CHECK(spira::overlap_check(true, SPIRA_MAX_RAYS / 16, 16, 0, true, &msg) == 0, "the slot limit itself");
    CHECK(spira::overlap_check(true, SPIRA_MAX_RAYS / 16 + 1, 16, 0, true, &msg) == SPIRA_E_LIMIT && std::strstr(msg, "n * max_list"), "%s", msg);
    CHECK(spira::overlap_check(true, 0xFFFFFFFFu, 16, 0, true, &msg) == SPIRA_E_LIMIT, "the product is formed in 64 bits");
}

// overlap_insert at capacity CAP, every K up to it, against the first K of the sorted sequence; the candidates are distinct, as a walk's are.
template <int CAP> static void check_list() {
    uint32_t seed = 12345u + CAP;
    for (uint32_t K = 0; K <= (uint32_t)CAP; ++K)
        for (int round = 0; round < 40; ++round) {
            const int n = round % 37;
            std::vector<int> seq;
            while ((int)seq.size() < n) {
                seed = seed * 1664525u + 1013904223u;
                const int p = (int)((seed >> 8) % 97u);
                if (std::find(seq.begin(), seq.end(), p) == seq.end()) seq.push_back(p);
            }
            spira::OverlapList<CAP> l;
            for (int j = 0; j < CAP; ++j) l.prim[j] = -1;
            l.n = 0;
            for (int p : seq) spira::overlap_insert<CAP>(l, K, p);
            std::sort(seq.begin(), seq.end());
            const uint32_t want = std::min<uint32_t>(K, (uint32_t)n);
            CHECK(l.n == want, "CAP %d K %u n %d: %u entries", CAP, K, n, l.n);
            for (uint32_t j = 0; j < want && j < l.n; ++j) CHECK(l.prim[j] == seq[j], "CAP %d K %u n %d slot %u: %d, not %d", CAP, K, n, j, l.prim[j], seq[j]);
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
        spira::OverlapBox<T> B;
        T He[3] = {0, 0, 0};
        if (kind == 'P' && got == 11) {
            spira::OverlapBox<T> Bf;
            T Hf[3];
            const bool with = spira::overlap_prepare<T>(v, frame, fr, Bf, Hf), without = spira::overlap_prepare<T>(v, false, nullptr, B, He);
            std::printf("bx %d %d", with ? 1 : 0, without ? 1 : 0);
            for (int i = 0; i < 3; ++i) for (int k = 0; k < 3; ++k) bits<T, U>(without ? B.A[i][k] : (T)0);
            for (int k = 0; k < 3; ++k) bits<T, U>(without ? He[k] : (T)0);
            std::printf("\n");
        } else if (kind == 'T' && got == 20) {
            const bool ok = spira::overlap_prepare<T>(v + 9, false, nullptr, B, He);
            std::printf("tri %d\n", !ok ? -3 : (spira::overlap_box_triangle<T>(B, v, v + 3, v + 6) ? 1 : 0));
        } else if (kind == 'S' && got == 15) {
            const bool ok = spira::overlap_prepare<T>(v + 4, false, nullptr, B, He);
            std::printf("sph %d\n", !ok ? -3 : (spira::overlap_box_sphere<T>(B, v, v[3]) ? 1 : 0));
        } else continue;
        ++n;
    }
    return n;
}

int main() {
    check_rules();
    check_list<1>(); check_list<4>(); check_list<16>();
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
