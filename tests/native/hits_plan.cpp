// hits_plan.cpp — host-only harness built with -fsanitize=address,undefined (tests/test_hits_cpu.py), in the manner of cast_plan.cpp: the very function the
// multi-hit kernels keep a lane's list with (spira_hits.h, hits_insert) and the argument rules of the entries (spira_plan.h, hits_check).
//   check     hits_check swept over its arguments: every rule returns its own code
//   insert    reads from stdin a line "f32|f64 K t_max_bits n" and then n lines "t_bits prim" (bit patterns in hexadecimal, indices in decimal); feeds them
//             to hits_insert in that order with the list capacities 1 (K = 1), 4 (K <= 4) and 16 and prints, per capacity that holds K, the final list
//             and the bound returned by the last insertion, which tests/test_hits_cpu.py compares bit for bit with sorted(...)[:K]
#include <cinttypes>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../julia-spira_amd/csrc/spira_plan.h"
#include "../../julia-spira_amd/csrc/spira_hits.h"

static int failures = 0;
#define CHECK(c, ...) do { if (!(c)) { ++failures; std::printf("FAILED %s:%d %s: ", __FILE__, __LINE__, #c); std::printf(__VA_ARGS__); std::printf("\n"); } } while (0)

static void check_rules() {
    const char *msg = nullptr;
    const uint32_t IN = SPIRA_CAST_INPLACE, ALL = SPIRA_HITS_COUNT_ALL;
    CHECK(spira::hits_check(false, 4, 1, 0, true, &msg) == SPIRA_E_INVALID && std::strstr(msg, "ray array is NULL"), "%s", msg);
    CHECK(spira::hits_check(true, 0, 1, 0, true, &msg) == SPIRA_E_INVALID && std::strstr(msg, "n_rays is 0"), "%s", msg);
    for (uint32_t f : {4u, 8u, 0x80000000u, 0x13u}) CHECK(spira::hits_check(true, 4, 1, f, true, &msg) == SPIRA_E_INVALID && std::strstr(msg, "unknown flag bits"), "%x %s", f, msg);
    for (uint32_t f : {0u, IN, ALL, IN | ALL})
        for (uint32_t k = 0; k <= 18; ++k) {
            const int rc = spira::hits_check(true, 4, k, f, true, &msg);
            const int want = k > SPIRA_MAX_HITS || (k == 0 && !(f & ALL)) ? SPIRA_E_INVALID : 0;
            CHECK(rc == want, "flags %x max_hits %u: %d", f, k, rc);
        }
    CHECK(spira::hits_check(true, 4, 17, 0, true, &msg) == SPIRA_E_INVALID && std::strstr(msg, "SPIRA_MAX_HITS"), "%s", msg);
    CHECK(spira::hits_check(true, 4, 0, 0, true, &msg) == SPIRA_E_INVALID && std::strstr(msg, "without SPIRA_HITS_COUNT_ALL"), "%s", msg);
    CHECK(spira::hits_check(true, 4, 2, 0, false, &msg) == SPIRA_E_INVALID && std::strstr(msg, "all NULL"), "%s", msg);
    CHECK(spira::hits_check(true, 4, 0, ALL, false, &msg) == SPIRA_E_INVALID && std::strstr(msg, "out_count is NULL"), "%s", msg);
    CHECK(spira::hits_check(true, SPIRA_MAX_RAYS, 1, 0, true, &msg) == 0, "the limit itself");
    CHECK(spira::hits_check(true, SPIRA_MAX_RAYS + 1, 1, 0, true, &msg) == SPIRA_E_LIMIT && std::strstr(msg, "SPIRA_MAX_RAYS"), "%s", msg);
    CHECK(spira::hits_check(true, SPIRA_MAX_RAYS + 1, 0, ALL, true, &msg) == SPIRA_E_LIMIT, "count only");
    CHECK(spira::hits_check(true, SPIRA_MAX_RAYS / 16, 16, 0, true, &msg) == 0, "2^26 slots");
    CHECK(spira::hits_check(true, SPIRA_MAX_RAYS / 16 + 1, 16, 0, true, &msg) == SPIRA_E_LIMIT && std::strstr(msg, "n_rays * max_hits"), "%s", msg);
    CHECK(spira::hits_check(true, 1u << 31, 2, 0, true, &msg) == SPIRA_E_LIMIT, "a product that wraps in 32 bits");
    CHECK(spira::hits_check(true, 1u << 28, 16, 0, true, &msg) == SPIRA_E_LIMIT, "2^32: the product is formed in 64 bits");
    std::printf("rules checked\n");
}

template <class T, class U, int CAP>
static void run_list(uint32_t K, T t_max, const std::vector<std::pair<T, int>> &seq) {
    spira::HitList<T, CAP> l;
    for (int j = 0; j < CAP; ++j) { l.t[j] = t_max; l.prim[j] = -1; }
    l.n = 0;
    T bound = t_max;
    for (const auto &e : seq) {
        bound = spira::hits_insert<T, CAP>(l, K, e.first, e.second, t_max);
        CHECK(l.n <= K && l.n <= (uint32_t)CAP, "n %u beyond K %u", l.n, K);
    }
    U bb; std::memcpy(&bb, &bound, sizeof(T));
    std::printf("list %d %u %llx", CAP, l.n, (unsigned long long)bb);
    for (uint32_t j = 0; j < l.n; ++j) { U b; std::memcpy(&b, &l.t[j], sizeof(T)); std::printf(" %llx:%d", (unsigned long long)b, l.prim[j]); }
    std::printf("\n");
}

template <class T, class U> static void insert_lines(uint32_t K, unsigned long long tmax_bits, uint32_t n) {
    T t_max; { const U u = (U)tmax_bits; std::memcpy(&t_max, &u, sizeof(T)); }
    std::vector<std::pair<T, int>> seq;
    for (uint32_t i = 0; i < n; ++i) {
        unsigned long long w; int p;
        if (std::scanf("%llx %d", &w, &p) != 2) { CHECK(false, "line %u", i); return; }
        T t; const U u = (U)w; std::memcpy(&t, &u, sizeof(T));
        seq.emplace_back(t, p);
    }
    if (K <= 1) run_list<T, U, 1>(K, t_max, seq);
    if (K <= 4) run_list<T, U, 4>(K, t_max, seq);
    run_list<T, U, 16>(K, t_max, seq);
}

int main() {
    check_rules();
    char prec[8] = {0};
    uint32_t K = 0, n = 0;
    unsigned long long tm = 0;
    while (std::scanf("%7s %u %llx %u", prec, &K, &tm, &n) == 4) {
        std::printf("case %s %u\n", prec, K);
        if (K > spira::kHitsMax) { CHECK(false, "K %u", K); break; }
        if (std::string(prec) == "f32") insert_lines<float, uint32_t>(K, tm, n);
        else insert_lines<double, uint64_t>(K, tm, n);
    }
    if (failures) { std::printf("%d checks FAILED\n", failures); return 1; }
    std::printf("all checks passed\n");
    return 0;
}
