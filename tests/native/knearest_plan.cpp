// knearest_plan.cpp — host-only harness built with -fsanitize=address,undefined (tests/test_knearest_cpu.py), in the manner of hits_plan.cpp: the very
// functions the K-nearest kernels keep a lane's list with (spira_knearest.h: near_offer, which calls near_insert) and the argument rules of the entries
// (spira_plan.h, nearest_k_check).
//   check     nearest_k_check swept over its arguments: every rule returns its own code
//   offer     reads from stdin a line "f32|f64 K best0_bits count_all n" and then n lines "d2_bits prim" (bit patterns in hexadecimal, indices in decimal);
//             offers them to a lane's list in that order — the candidate test against the bound, the insertion, the new bound: what a kernel does for every
//             object it meets — with every list capacity that holds K (1, 4, 16) and both kinds of entry (the point kept, the record index kept), and
//             prints per run the final list, the final bound and the candidates counted, which the test compares bit for bit with a sort.  Here it is
//             checked that an entry's third field travelled with it.
#include <cinttypes>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../julia-spira_amd/csrc/spira_plan.h"
#include "../../julia-spira_amd/csrc/spira_knearest.h"

static int failures = 0;
#define CHECK(c, ...) do { if (!(c)) { ++failures; std::printf("FAILED %s:%d %s: ", __FILE__, __LINE__, #c); std::printf(__VA_ARGS__); std::printf("\n"); } } while (0)

static void check_rules() {
    const char *msg = nullptr;
    const uint32_t IN = SPIRA_CAST_INPLACE, ALL = SPIRA_NEAR_COUNT_ALL;
    CHECK(spira::nearest_k_check(false, 4, 1, 0, true, &msg) == SPIRA_E_INVALID && std::strstr(msg, "point array is NULL"), "%s", msg);
    CHECK(spira::nearest_k_check(true, 0, 1, 0, true, &msg) == SPIRA_E_INVALID && std::strstr(msg, "n_points is 0"), "%s", msg);
    for (uint32_t f : {4u, 8u, 0x80000000u, 0x13u}) CHECK(spira::nearest_k_check(true, 4, 1, f, true, &msg) == SPIRA_E_INVALID && std::strstr(msg, "unknown flag bits"), "%x %s", f, msg);
    for (uint32_t f : {0u, IN, ALL, IN | ALL})
        for (uint32_t k = 0; k <= 18; ++k) {
            const int rc = spira::nearest_k_check(true, 4, k, f, true, &msg);
            const int want = k > SPIRA_MAX_NEAR || (k == 0 && !(f & ALL)) ? SPIRA_E_INVALID : 0;
            CHECK(rc == want, "flags %x max_near %u: %d", f, k, rc);
        }
    CHECK(spira::nearest_k_check(true, 4, 17, 0, true, &msg) == SPIRA_E_INVALID && std::strstr(msg, "SPIRA_MAX_NEAR"), "%s", msg);
    CHECK(spira::nearest_k_check(true, 4, 0, 0, true, &msg) == SPIRA_E_INVALID && std::strstr(msg, "without SPIRA_NEAR_COUNT_ALL"), "%s", msg);
    CHECK(spira::nearest_k_check(true, 4, 2, 0, false, &msg) == SPIRA_E_INVALID && std::strstr(msg, "all NULL"), "%s", msg);
    CHECK(spira::nearest_k_check(true, 4, 0, ALL, false, &msg) == SPIRA_E_INVALID && std::strstr(msg, "out_count is NULL"), "%s", msg);
    CHECK(spira::nearest_k_check(true, SPIRA_MAX_RAYS, 1, 0, true, &msg) == 0, "the limit itself");
    CHECK(spira::nearest_k_check(true, SPIRA_MAX_RAYS + 1, 1, 0, true, &msg) == SPIRA_E_LIMIT && std::strstr(msg, "SPIRA_MAX_RAYS"), "%s", msg);
    CHECK(spira::nearest_k_check(true, SPIRA_MAX_RAYS + 1, 0, ALL, true, &msg) == SPIRA_E_LIMIT, "count only");
    CHECK(spira::nearest_k_check(true, SPIRA_MAX_RAYS / 16, 16, 0, true, &msg) == 0, "2^26 slots");
    CHECK(spira::nearest_k_check(true, SPIRA_MAX_RAYS / 16 + 1, 16, 0, true, &msg) == SPIRA_E_LIMIT && std::strstr(msg, "n_points * max_near"), "%s", msg);
    CHECK(spira::nearest_k_check(true, 1u << 31, 2, 0, true, &msg) == SPIRA_E_LIMIT, "a product that wraps in 32 bits");
    CHECK(spira::nearest_k_check(true, 1u << 28, 16, 0, true, &msg) == SPIRA_E_LIMIT, "2^32: the product is formed in 64 bits");
    static_assert(spira::kNearMax == SPIRA_MAX_NEAR, "one limit");
    std::printf("rules checked\n");
}

// The third field of the entry made from (d2, prim), in both kinds, and whether an entry still carries its own.
template <class T> static spira::NearPoint<T> mark(T d2, int prim, spira::NearPoint<T> *) { return {{(T)prim, d2, (T)(-3 * prim)}}; }
template <class T> static spira::NearRef mark(T, int prim, spira::NearRef *) { return {(uint32_t)prim * 7u + 1u}; }
template <class T> static bool same(const spira::NearPoint<T> &a, const spira::NearPoint<T> &b) { return std::memcmp(&a, &b, sizeof a) == 0; }
template <class T> static bool same(const spira::NearRef &a, const spira::NearRef &b) { return a.ref == b.ref; }

template <class T, class U, int CAP, class P>
static void run_list(const char *kind, uint32_t K, T best0, bool count_all, const std::vector<std::pair<T, int>> &seq) {
    spira::NearList<T, CAP, P> l;
    for (int j = 0; j < CAP; ++j) { l.d2[j] = best0; l.prim[j] = -1; l.pay[j] = P{}; }
    l.n = 0;
    T bound = best0;
    uint32_t total = 0;
    for (const auto &e : seq) {
        const T before = bound;
        const bool full = spira::near_offer<T, CAP, P>(l, K, count_all, e.first, e.second, mark<T>(e.first, e.second, (P *)nullptr), best0, bound, total);
        CHECK(l.n <= K && l.n <= (uint32_t)CAP, "n %u beyond K %u", l.n, K);
        CHECK(bound <= before, "the bound grew");
        CHECK(!full || (!count_all && l.n == K), "full reported for n %u of K %u", l.n, K);
        if (count_all) CHECK(std::memcmp(&bound, &best0, sizeof(T)) == 0, "the bound moved under count_all");
    }
    for (uint32_t j = 0; j < l.n; ++j) CHECK(same<T>(l.pay[j], mark<T>(l.d2[j], l.prim[j], (P *)nullptr)), "%s cap %d slot %u lost its third field", kind, CAP, j);
    U bb; std::memcpy(&bb, &bound, sizeof(T));
    std::printf("list %s %d %u %llx %u", kind, CAP, l.n, (unsigned long long)bb, total);
    for (uint32_t j = 0; j < l.n; ++j) { U b; std::memcpy(&b, &l.d2[j], sizeof(T)); std::printf(" %llx:%d", (unsigned long long)b, l.prim[j]); }
    std::printf("\n");
}

template <class T, class U> static void offer_lines(uint32_t K, unsigned long long best_bits, bool count_all, uint32_t n) {
    T best0; { const U u = (U)best_bits; std::memcpy(&best0, &u, sizeof(T)); }
    std::vector<std::pair<T, int>> seq;
    for (uint32_t i = 0; i < n; ++i) {
        unsigned long long w; int p;
        if (std::scanf("%llx %d", &w, &p) != 2) { CHECK(false, "line %u", i); return; }
        T t; const U u = (U)w; std::memcpy(&t, &u, sizeof(T));
        seq.emplace_back(t, p);
    }
    if (K <= 1) { run_list<T, U, 1, spira::NearPoint<T>>("q", K, best0, count_all, seq); run_list<T, U, 1, spira::NearRef>("r", K, best0, count_all, seq); }
    if (K <= 4) { run_list<T, U, 4, spira::NearPoint<T>>("q", K, best0, count_all, seq); run_list<T, U, 4, spira::NearRef>("r", K, best0, count_all, seq); }
    run_list<T, U, 16, spira::NearPoint<T>>("q", K, best0, count_all, seq);
    run_list<T, U, 16, spira::NearRef>("r", K, best0, count_all, seq);
}

int main() {
    check_rules();
    char prec[8] = {0};
    uint32_t K = 0, n = 0, all = 0;
    unsigned long long bm = 0;
    while (std::scanf("%7s %u %llx %u %u", prec, &K, &bm, &all, &n) == 5) {
        std::printf("case %s %u %u\n", prec, K, all);
        if (K > spira::kNearMax) { CHECK(false, "K %u", K); break; }
        if (std::string(prec) == "f32") offer_lines<float, uint32_t>(K, bm, all != 0, n);
        else offer_lines<double, uint64_t>(K, bm, all != 0, n);
    }
    if (failures) { std::printf("%d checks FAILED\n", failures); return 1; }
    std::printf("all checks passed\n");
    return 0;
}
