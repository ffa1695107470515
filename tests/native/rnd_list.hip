// GPU check of the wave-cooperative drain of k_path's / k_bounce's random-vector list (spira_device.h: drain_unit_sphere_list, RndTry):
//   every entry of a list of n seeded RNG keys ends up holding exactly random_in_unit_sphere of its key — the point of the lowest accepted
//   try t <= MAXT, or the zero vector when tries 1 .. MAXT all fail — whichever lane, in the main phase or in a group of the tail, evaluated it.
// One wave per list.  Lists of n in {0, 1, 2, 3, 31, 32, 33, 63, 64, 65, 127, 128} keys, both precisions, the routine and a plain per-lane loop
// instantiated at MAXT = 64 (kMaxTries: there the per-lane loop is random_in_unit_sphere itself) and at 1, 2, 3, 5, 7 — so that exhaustion
// happens in the main phase, at the end of a group's span and inside one (7 is odd: no group size divides it), and entries still succeed on
// their last allowed try.  Slots behind the list must keep their contents (the tail's table lives in slots of the list itself).
// usage: rnd_list <lists per case> <seed>; one line per (precision, MAXT): entries, mismatches, exhausted, accepted, accepted on the last try;
// exit 0 iff no mismatch, no touched slot, and every MAXT < 64 shows both outcomes and an accept on the last try
#include <cstdio>
#include <cstdlib>
#include "../../julia-spira_amd/csrc/spira_device.h"

using namespace spira;

constexpr uint32_t kSlots = 128;

__device__ __forceinline__ bool same(double a, double b) { return __double_as_longlong(a) == __double_as_longlong(b); }
__device__ __forceinline__ bool same(float a, float b) { return __float_as_uint(a) == __float_as_uint(b); }

// random_in_unit_sphere (spira_device.h) with the bound as a parameter: a plain loop of one lane
template <class T, uint32_t MAXT> __device__ Vec<T> serial(const RngKey &k, uint32_t &accepted_at) {
    Vec<T> p = mk<T>(0, 0, 0);
    accepted_at = 0;
    for (uint32_t t = 1; t <= MAXT; ++t) {
        T u0, u1, u2;
        rng3<T>(k, t, u0, u1, u2, (T)(1.0 / 1048576.0));
        Vec<T> q = mk<T>(u0, u1, u2) - mk<T>(1, 1, 1);
        if (dot(q, q) < (T)1.0) { p = q; accepted_at = t; break; }
    }
    return p;
}

// out: [0] entries, [1] mismatches, [2] exhausted, [3] accepted, [4] accepted on try MAXT, [5] slots behind the list that changed
template <class T, uint32_t MAXT>
__global__ __launch_bounds__(64) void k_lists(uint32_t seed, uint32_t n, unsigned long long *out) {
    __shared__ __attribute__((aligned(32))) Pack4<T> s_rnd[kSlots];
    constexpr uint32_t W = sizeof(Pack4<T>) / 4;
    const uint32_t lane = threadIdx.x;
    uint32_t *words = reinterpret_cast<uint32_t *>(s_rnd);
    RngKey key[2];
    for (uint32_t i = 0; i < 2; ++i) {
        const uint32_t e = lane + 64 * i;
        const uint32_t h = mix32(seed ^ mix32(blockIdx.x * 0x9E3779B9u + n * 131u + e));
        key[i].hA = mix32(h + 1u); key[i].hB = mix32(h ^ 0x5bd1e995u); key[i].hBr = (key[i].hB << 16) | (key[i].hB >> 16);
        for (uint32_t w = 0; w < W; ++w) words[e * W + w] = 0xA5000000u + e * 16u + w;       // what a slot behind the list has to keep
        if (e < n) { words[e * W] = key[i].hA; words[e * W + 1] = key[i].hB; }
    }
    wave_lds_sync();
    drain_unit_sphere_list<T, MAXT>(s_rnd, n, lane);
    wave_lds_sync();
    unsigned long long cnt[6] = {0, 0, 0, 0, 0, 0};
    for (uint32_t i = 0; i < 2; ++i) {
        const uint32_t e = lane + 64 * i;
        if (e < n) {
            uint32_t at;
            const Vec<T> want = serial<T, MAXT>(key[i], at);
            const Vec<T> got = RndTry<T>::load(&s_rnd[e]);
            bool ok = same(want.x, got.x) && same(want.y, got.y) && same(want.z, got.z);
            if (MAXT == kMaxTries) {
                const Vec<T> ref = random_in_unit_sphere<T>(key[i]);
                ok = ok && same(ref.x, got.x) && same(ref.y, got.y) && same(ref.z, got.z);
            }
            ++cnt[0];
            if (!ok) ++cnt[1];
            if (at == 0) ++cnt[2]; else ++cnt[3];
            if (at == MAXT) ++cnt[4];
        } else {
            for (uint32_t w = 0; w < W; ++w) if (words[e * W + w] != 0xA5000000u + e * 16u + w) { ++cnt[5]; break; }
        }
    }
    for (int c = 0; c < 6; ++c) if (cnt[c]) atomicAdd(&out[c], cnt[c]);
}

static const uint32_t kLens[] = {0, 1, 2, 3, 31, 32, 33, 63, 64, 65, 127, 128};

template <class T, uint32_t MAXT> static int run(const char *name, uint32_t lists, uint32_t seed, unsigned long long *d_out) {
    if (hipMemset(d_out, 0, 6 * sizeof(unsigned long long)) != hipSuccess) return 1;
    for (uint32_t n : kLens) k_lists<T, MAXT><<<lists, 64>>>(seed + MAXT * 7919u, n, d_out);
    unsigned long long h[6];
    if (hipDeviceSynchronize() != hipSuccess || hipMemcpy(h, d_out, sizeof(h), hipMemcpyDeviceToHost) != hipSuccess) { printf("%s MAXT %u: HIP error %s\n", name, MAXT, hipGetErrorString(hipGetLastError())); return 1; }
    printf("%s MAXT %2u: %llu entries, %llu mismatching, %llu exhausted, %llu accepted, %llu on the last try, %llu slots behind a list touched\n", name, MAXT, h[0], h[1], h[2], h[3], h[4], h[5]);
    unsigned long long expect = 0;
    for (uint32_t n : kLens) expect += (unsigned long long)n * lists;
    bool ok = h[0] == expect && h[1] == 0 && h[5] == 0 && h[3] > 0;
    if (MAXT < kMaxTries) ok = ok && h[2] > 0 && h[4] > 0;
    return ok ? 0 : 1;
}

template <class T> static int run_all(const char *name, uint32_t lists, uint32_t seed, unsigned long long *d_out) {
    int bad = 0;
    bad += run<T, kMaxTries>(name, lists, seed, d_out);
    bad += run<T, 1>(name, lists, seed, d_out);
    bad += run<T, 2>(name, lists, seed, d_out);
    bad += run<T, 3>(name, lists, seed, d_out);
    bad += run<T, 5>(name, lists, seed, d_out);
    bad += run<T, 7>(name, lists, seed, d_out);
    return bad;
}

int main(int argc, char **argv) {
    const uint32_t lists = argc > 1 ? (uint32_t)atoi(argv[1]) : 64u, seed = argc > 2 ? (uint32_t)strtoul(argv[2], nullptr, 10) : 20261017u;
    unsigned long long *d_out = nullptr;
    if (hipMalloc(&d_out, 6 * sizeof(unsigned long long)) != hipSuccess) { printf("hipMalloc failed\n"); return 2; }
    int bad = run_all<double>("Float64", lists, seed, d_out) + run_all<float>("Float32", lists, seed, d_out);
    hipFree(d_out);
    printf("%s\n", bad ? "FAILED" : "ok");
    return bad ? 1 : 0;
}
