// sweep_plan.cpp — host-only harness built with -fsanitize=address,undefined (tests/test_sweep_cpu.py), in the manner of nearest_plan.cpp: the very
// functions the sphere-sweep kernels call (spira_sweep.h) — sweep_prepare, sweep_sphere_triangle, sweep_sphere_sphere, sweep_normal — on a table read from
// stdin, and the argument rules of the entries (spira_plan.h, sweep_check) swept over their arguments.  A line "f32|f64 frame cx cy cz scale", then lines of
// hexadecimal bit patterns:
//   P ray[8] r                                  -> "sw <verdict>"
//   T v0[3] e1[3] e2[3] o[3] d[3] r t_min t_max -> "tri hit t q0 q1 q2 n0 n1 n2"   (bits; a miss: t = t_max, q and n 0)
//   S c[3] R o[3] d[3] r t_min t_max            -> "sph hit t q0 q1 q2 n0 n1 n2"
// tests/test_sweep_cpu.py compares them with the numpy twins of spira_hip.query.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>

#include "../../julia-spira_amd/csrc/spira_plan.h"
#include "../../julia-spira_amd/csrc/spira_sweep.h"

static int failures = 0;
#define CHECK(c, ...) do { if (!(c)) { ++failures; std::printf("FAILED %s:%d %s: ", __FILE__, __LINE__, #c); std::printf(__VA_ARGS__); std::printf("\n"); } } while (0)

static void check_rules() {
    const char *msg = nullptr;
    CHECK(spira::sweep_check(false, true, 4, 0, true, &msg) == SPIRA_E_INVALID && std::strstr(msg, "ray array is NULL"), "%s", msg);
    CHECK(spira::sweep_check(true, false, 4, 0, true, &msg) == SPIRA_E_INVALID && std::strstr(msg, "radius array is NULL"), "%s", msg);
    CHECK(spira::sweep_check(true, true, 0, 0, true, &msg) == SPIRA_E_INVALID && std::strstr(msg, "n is 0"), "%s", msg);
    for (uint32_t f : {2u, 4u, 0x80000000u, 0x13u}) CHECK(spira::sweep_check(true, true, 4, f, true, &msg) == SPIRA_E_INVALID && std::strstr(msg, "unknown flag bits"), "%x %s", f, msg);
    for (uint32_t f : {0u, (uint32_t)SPIRA_CAST_INPLACE}) CHECK(spira::sweep_check(true, true, 4, f, true, &msg) == 0, "flags %x", f);
    CHECK(spira::sweep_check(true, true, 4, 0, false, &msg) == SPIRA_E_INVALID && std::strstr(msg, "every output is NULL"), "%s", msg);
    CHECK(spira::sweep_check(true, true, SPIRA_MAX_RAYS, 0, true, &msg) == 0, "the limit itself");
    CHECK(spira::sweep_check(true, true, SPIRA_MAX_RAYS + 1, 0, true, &msg) == SPIRA_E_LIMIT && std::strstr(msg, "SPIRA_MAX_RAYS"), "%s", msg);
}

template <class T, class U> static void put(const char *tag, bool hit, T t, T t_max, const T q[3], const T o[3], const T d[3]) {
    T v[7] = {hit ? t : t_max, 0, 0, 0, 0, 0, 0};
    if (hit) { for (int k = 0; k < 3; ++k) v[1 + k] = q[k]; spira::sweep_normal<T>(o, d, t, q, v + 4); }
    std::printf("%s %d", tag, hit ? 1 : 0);
    for (int k = 0; k < 7; ++k) { U b; std::memcpy(&b, &v[k], sizeof(T)); std::printf(" %llx", (unsigned long long)b); }
    std::printf("\n");
}

template <class T, class U> static int lines(bool frame, const double fr64[4]) {
    const T fr[4] = {(T)fr64[0], (T)fr64[1], (T)fr64[2], (T)fr64[3]};
    char line[2048];
    int n = 0;
    while (std::fgets(line, sizeof line, stdin)) {
        unsigned long long w[18];
        char kind = 0;
        const int got = std::sscanf(line, " %c %llx %llx %llx %llx %llx %llx %llx %llx %llx %llx %llx %llx %llx %llx %llx %llx %llx %llx", &kind, w, w + 1, w + 2, w + 3, w + 4,
                                    w + 5, w + 6, w + 7, w + 8, w + 9, w + 10, w + 11, w + 12, w + 13, w + 14, w + 15, w + 16, w + 17);
        T v[18];
        for (int k = 0; k < 18; ++k) { const U u = k < got - 1 ? (U)w[k] : (U)0; std::memcpy(&v[k], &u, sizeof(T)); }
        if (kind == 'P' && got == 10) { T d[3]; std::printf("sw %d\n", spira::sweep_prepare<T>(v, v[8], frame, fr, d) ? 1 : 0); }
        else if (kind == 'T' && got == 19) {
            T t = 0, q[3] = {0, 0, 0};
            const bool hit = spira::sweep_sphere_triangle<T>(v, v + 3, v + 6, v + 9, v + 12, v[15], v[16], v[17], t, q);
            put<T, U>("tri", hit, t, v[17], q, v + 9, v + 12);
        } else if (kind == 'S' && got == 14) {
            T t = 0, q[3] = {0, 0, 0};
            const bool hit = spira::sweep_sphere_sphere<T>(v, v[3], v + 4, v + 7, v[10], v[11], v[12], t, q);
            put<T, U>("sph", hit, t, v[12], q, v + 4, v + 7);
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
