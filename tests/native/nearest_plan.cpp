// nearest_plan.cpp — host-only harness built with -fsanitize=address,undefined (tests/test_nearest_cpu.py), in the manner of cast_plan.cpp: the very
// functions the closest-point kernels call (spira_nearest.h) — nearest_point_prepare, closest_point_triangle, closest_point_sphere — on a table read from
// stdin.  A line "f32|f64 frame cx cy cz scale", then lines of hexadecimal bit patterns:
//   P px py pz r_max                 -> "pt <verdict>"
//   T v0[3] e1[3] e2[3] p[3]         -> "tri q0 q1 q2 d2"   (bits)
//   S c[3] r p[3]                    -> "sph q0 q1 q2 d2"   (bits)
// tests/test_nearest_cpu.py compares them with the numpy twins of spira_hip.query.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>

#include "../../julia-spira_amd/csrc/spira_nearest.h"

template <class T, class U> static void put(const char *tag, const T q[3], T d2) {
    U b[4];
    for (int k = 0; k < 3; ++k) std::memcpy(&b[k], &q[k], sizeof(T));
    std::memcpy(&b[3], &d2, sizeof(T));
    std::printf("%s %llx %llx %llx %llx\n", tag, (unsigned long long)b[0], (unsigned long long)b[1], (unsigned long long)b[2], (unsigned long long)b[3]);
}

template <class T, class U> static int lines(bool frame, const double fr64[4]) {
    const T fr[4] = {(T)fr64[0], (T)fr64[1], (T)fr64[2], (T)fr64[3]};
    char line[1024];
    int n = 0;
    while (std::fgets(line, sizeof line, stdin)) {
        unsigned long long w[12];
        char kind = 0;
        const int got = std::sscanf(line, " %c %llx %llx %llx %llx %llx %llx %llx %llx %llx %llx %llx %llx", &kind, w, w + 1, w + 2, w + 3, w + 4, w + 5, w + 6, w + 7,
                                    w + 8, w + 9, w + 10, w + 11);
        T v[12];
        for (int k = 0; k < 12; ++k) { const U u = k < got - 1 ? (U)w[k] : (U)0; std::memcpy(&v[k], &u, sizeof(T)); }
        if (kind == 'P' && got == 5) std::printf("pt %d\n", spira::nearest_point_prepare<T>(v, frame, fr) ? 1 : 0);
        else if (kind == 'T' && got == 13) { T q[3], d2; spira::closest_point_triangle<T>(v, v + 3, v + 6, v + 9, q, d2); put<T, U>("tri", q, d2); }
        else if (kind == 'S' && got == 8) { T q[3], d2; spira::closest_point_sphere<T>(v, v[3], v + 4, q, d2); put<T, U>("sph", q, d2); }
        else continue;
        ++n;
    }
    return n;
}

int main() {
    char prec[8] = {0};
    int frame = 0, n = 0;
    double fr[4] = {0, 0, 0, 1};
    if (std::scanf("%7s %d %lf %lf %lf %lf\n", prec, &frame, fr, fr + 1, fr + 2, fr + 3) == 6) {
        if (std::string(prec) == "f32") n = lines<float, uint32_t>(frame != 0, fr);
        else n = lines<double, uint64_t>(frame != 0, fr);
    }
    std::printf("%d lines answered\nall checks passed\n", n);
    return 0;
}
