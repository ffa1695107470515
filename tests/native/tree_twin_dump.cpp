// tree_twin_dump.cpp — the host twins of tree_twin.h as a program that emits bytes: `tree_twin_dump JOB OUT` runs a chain of create / update / rebuild steps
// on one handle and appends, after every step, the four blobs spira_debug_scene_tree (spira_hip.hip) reads back from the device, in the same layout.  No
// HIP; built with g++ -std=c++17 -O2 -ffp-contract=off by tests/test_gpu_tree_bytes.py (and with ASan + UBSan by tests/test_tree_twin_cpu.py).
//
// JOB (little endian):  char magic[8] = "SPTWJOB1"; uint32 precision (4 | 8), n, n_materials, screen (1: the handle has Float32 screening records), n_steps;
//                       then per step: uint32 kind (0 create, 1 update, 2 rebuild), uint32 0, and n x 10 values of the precision (the caller's triangles10)
// OUT:                  per step: uint32 kind, int32 status, uint32 n_blobs, uint32 0; then n_blobs x { uint64 bytes; the bytes }
//   status 0: the step was taken and n_blobs is 4: summary (uint32 precision, n, n_slots, depth; double centre[3], scale; uint32 level_first[0 .. depth]),
//   the node array (n_slots x 20 dwords), the three frame packets + the triangle records ((3 + 3 n) packets of four T), the screening records (3 n packets
//   of four floats, or nothing).  Otherwise the step was refused, the handle is as it was and n_blobs is 0; status: the kRefit* bits of spira_refit.h
//   (1 non-finite, 2 material: SPIRA_E_INVALID; 4 frame: SPIRA_E_LIMIT), -4 for the other refusals of a rebuild or a failed build (SPIRA_E_LIMIT).
// An update that follows a create with the very same array is also put through the identity check of refit_plan.cpp (check_identity_bounds: what
// spira_refit.h lets a refit change), and a line says so on stdout.  Exit status: 0, 1 when a CHECK failed, 2 for a job that cannot be read.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "tree_twin.h"

static bool read_exact(std::FILE *f, void *p, size_t bytes) { return bytes == 0 || std::fread(p, 1, bytes, f) == bytes; }
static bool write_blob(std::FILE *f, const void *p, size_t bytes) {
    const uint64_t len = bytes;
    return std::fwrite(&len, 8, 1, f) == 1 && (bytes == 0 || std::fwrite(p, 1, bytes, f) == bytes);
}

template <class T>
static bool write_handle(std::FILE *f, const Handle<T> &h) {
    std::vector<unsigned char> sum(16 + 32 + 4 * ((size_t)h.depth + 1));
    const uint32_t head[4] = {(uint32_t)sizeof(T), h.n, h.n_slots, (uint32_t)h.depth};
    const double fr[4] = {h.centre[0], h.centre[1], h.centre[2], h.scale};
    CHECK(h.level_first.size() == (size_t)h.depth + 1 && h.nodes.size() >= (size_t)h.n_slots * kBvhNodeDwords && h.tris.size() == 3 * (size_t)h.n);
    if (h.level_first.size() != (size_t)h.depth + 1 || h.nodes.size() < (size_t)h.n_slots * kBvhNodeDwords) return false;
    std::memcpy(sum.data(), head, 16); std::memcpy(sum.data() + 16, fr, 32); std::memcpy(sum.data() + 48, h.level_first.data(), 4 * ((size_t)h.depth + 1));
    std::vector<spira::RefitPack4<T>> rec(3 + h.tris.size());
    std::memcpy(rec.data(), h.frame, sizeof h.frame);
    if (!h.tris.empty()) std::memcpy(rec.data() + 3, h.tris.data(), h.tris.size() * sizeof(h.tris[0]));
    return write_blob(f, sum.data(), sum.size()) && write_blob(f, h.nodes.data(), (size_t)h.n_slots * kBvhNodeDwords * 4) &&
           write_blob(f, rec.data(), rec.size() * sizeof(rec[0])) && write_blob(f, h.tris32.data(), h.tris32.size() * sizeof(spira::RefitPack4<float>));
}

template <class T>
static int run(std::FILE *job, std::FILE *out, uint32_t n, uint32_t n_materials, bool screen, uint32_t n_steps) {
    Handle<T> h, built;
    std::vector<T> tri((size_t)n * 10), built_from;
    bool have = false, after_create = false;
    for (uint32_t step = 0; step < n_steps; ++step) {
        uint32_t kind[2];
        if (!read_exact(job, kind, sizeof kind) || !read_exact(job, tri.data(), tri.size() * sizeof(T))) { std::fprintf(stderr, "job: step %u is cut short\n", step); return 2; }
        int status = 0;
        if (kind[0] == 0u) {
            Handle<T> fresh;
            if (host_build(fresh, tri, screen)) { h = fresh; built = fresh; built_from = tri; have = true; }
            else status = -4;
        } else if (!have) {
            std::fprintf(stderr, "job: step %u comes before a create\n", step);
            return 2;
        } else if (kind[0] == 1u) {
            status = (int)(host_refit(h, tri, n_materials) & 7u);
            if (status == 0 && after_create && std::memcmp(tri.data(), built_from.data(), tri.size() * sizeof(T)) == 0) {
                const double pad = spira::refit_pad<T>(built.centre, built.scale), pad_built = builder_pad<T>(tri, built.scale);
                CHECK(pad >= pad_built);
                CHECK(std::memcmp(h.tris.data(), built.tris.data(), h.tris.size() * sizeof(h.tris[0])) == 0);          // the records bit for bit
                const T bmn[3] = {built.frame[0].x, built.frame[0].y, built.frame[0].z}, bmx[3] = {built.frame[1].x, built.frame[1].y, built.frame[1].z};
                const T imn[3] = {h.frame[0].x, h.frame[0].y, h.frame[0].z}, imx[3] = {h.frame[1].x, h.frame[1].y, h.frame[1].z};
                const double worst = check_identity_bounds<T>(built.nodes.data(), h.nodes.data(), h.n_slots, bmn, bmx, imn, imx, built.scale, pad, pad_built);
                std::printf("step %u: identity refit moves a child bound by at most %.3f grid steps\n", step, worst);
            }
        } else if (kind[0] == 2u) {
            const int rc = host_rebuild(h, tri, n_materials, spira::kLbvhMaxDepth);
            status = rc > 0 ? (rc & 7) : rc;
        } else {
            std::fprintf(stderr, "job: step %u has kind %u\n", step, kind[0]);
            return 2;
        }
        after_create = kind[0] == 0u && status == 0;
        const uint32_t rec[4] = {kind[0], (uint32_t)status, status == 0 ? 4u : 0u, 0u};
        if (std::fwrite(rec, sizeof rec, 1, out) != 1 || (status == 0 && !write_handle(out, h))) { std::fprintf(stderr, "cannot write the output\n"); return 2; }
    }
    return g_fail ? 1 : 0;
}

int main(int argc, char **argv) {
    if (argc != 3) { std::fprintf(stderr, "usage: tree_twin_dump JOB OUT\n"); return 2; }
    std::FILE *job = std::fopen(argv[1], "rb");
    if (!job) { std::fprintf(stderr, "cannot read %s\n", argv[1]); return 2; }
    char magic[8];
    uint32_t head[5];
    if (!read_exact(job, magic, 8) || std::memcmp(magic, "SPTWJOB1", 8) != 0 || !read_exact(job, head, sizeof head) || (head[0] != 4u && head[0] != 8u) || head[1] < 2u ||
        head[1] > (1u << 24)) {
        std::fprintf(stderr, "%s is no job of this program\n", argv[1]);
        std::fclose(job);
        return 2;
    }
    std::FILE *out = std::fopen(argv[2], "wb");
    if (!out) { std::fprintf(stderr, "cannot write %s\n", argv[2]); std::fclose(job); return 2; }
    int rc = head[0] == 4u ? run<float>(job, out, head[1], head[2], head[3] != 0u, head[4]) : run<double>(job, out, head[1], head[2], head[3] != 0u, head[4]);
    std::fclose(job);
    if (std::fclose(out) != 0 && rc == 0) rc = 2;
    if (g_fail) std::fprintf(stderr, "%d checks failed\n", g_fail);
    return rc;
}
