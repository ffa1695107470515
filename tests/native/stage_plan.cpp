// stage_plan.cpp — host-only harness built with -fsanitize=address,undefined (tests/test_stage_cpu.py), in the manner of sdf_plan.cpp: the layout of a
// host-form list call's arrays in the staging buffer (spira_plan.h, stage_layout), which stage_in (spira_hip.hip) follows to the byte.
//   sweep     every present/NULL combination of 1 .. 8 blocks, under size assignments drawn from the sizes around the alignment (0, 1, 4, 12, 15, 16,
//             17, ...) and from the largest blocks an entry can form (SPIRA_MAX_RAYS x 16 slots x 3 x 8 bytes): all of them for up to 3 blocks, every
//             rotation and stride of the table and 64 drawn assignments for more
//   checks    a present block starts at a multiple of 16, at or after the end of the present block before it and less than 16 bytes after it (order kept,
//             no overlap, no hole a block would fit the alignment in); a NULL block has no room: the present blocks lie exactly where they lie in the
//             table without it; the total is the end of the last present block; nothing wraps in 64 bits
#include <cstdint>
#include <cstdio>

#include "../../julia-spira_amd/csrc/spira_plan.h"

static_assert(sizeof(size_t) == 8, "the staging arithmetic is in 64 bits");
static_assert(spira::kStageAlign == 16, "every present block starts at a multiple of 16 bytes");

static int failures = 0;
static long long cases = 0;
#define CHECK(c, ...) do { if (!(c)) { ++failures; std::printf("FAILED %s:%d %s: ", __FILE__, __LINE__, #c); std::printf(__VA_ARGS__); std::printf("\n"); } } while (0)

constexpr int kMaxBlocks = 8;
constexpr size_t kLargest = (size_t)SPIRA_MAX_RAYS * 16 * 3 * 8;      // n x K x 3 values of Float64: the points of a K-nearest call at its limits
static const size_t kSizes[] = {0, 1, 4, 12, 15, 16, 17, 31, 32, 33, 130 * 3 * 4, (size_t)SPIRA_MAX_RAYS * 4, kLargest - 8, kLargest};
constexpr int kNumSizes = (int)(sizeof kSizes / sizeof kSizes[0]);

static void check_case(const size_t *bytes, unsigned mask, int n) {
    bool present[kMaxBlocks];
    size_t offset[kMaxBlocks], packed_bytes[kMaxBlocks], packed_offset[kMaxBlocks];
    bool packed_present[kMaxBlocks];
    int m = 0;
    for (int k = 0; k < n; ++k) {
        present[k] = (mask >> k) & 1;
        offset[k] = ~(size_t)0;
        if (present[k]) { packed_bytes[m] = bytes[k]; packed_present[m] = true; ++m; }
    }
    const size_t total = spira::stage_layout(bytes, present, n, offset);
    const size_t packed_total = spira::stage_layout(packed_bytes, packed_present, m, packed_offset);
    size_t end = 0, sum = 0;
    int j = 0;
    for (int k = 0; k < n; ++k) {
        CHECK(offset[k] != ~(size_t)0, "block %d of %d (mask %x): no offset written", k, n, mask);
        if (!present[k]) continue;
        CHECK(offset[k] % 16 == 0, "block %d of %d (mask %x): offset %zu", k, n, mask, offset[k]);
        CHECK(offset[k] >= end && offset[k] - end < 16, "block %d of %d (mask %x): offset %zu after end %zu", k, n, mask, offset[k], end);
        CHECK(offset[k] + bytes[k] >= offset[k], "block %d of %d (mask %x): the end wraps", k, n, mask);
        CHECK(offset[k] == packed_offset[j], "block %d of %d (mask %x): %zu, without the NULL blocks %zu", k, n, mask, offset[k], packed_offset[j]);
        end = offset[k] + bytes[k];
        sum += bytes[k];
        ++j;
    }
    CHECK(total == end, "%d blocks (mask %x): total %zu, last end %zu", n, mask, total, end);
    CHECK(total == packed_total, "%d blocks (mask %x): total %zu, without the NULL blocks %zu", n, mask, total, packed_total);
    CHECK(total >= sum && total - sum < 16 * (size_t)kMaxBlocks, "%d blocks (mask %x): total %zu for %zu bytes", n, mask, total, sum);
    CHECK(total < ((size_t)1 << 63), "%d blocks (mask %x): total %zu", n, mask, total);
    ++cases;
}

static void all_masks(const size_t *bytes, int n) {
    for (unsigned mask = 0; mask < (1u << n); ++mask) check_case(bytes, mask, n);
}

int main() {
    size_t bytes[kMaxBlocks];
    // up to 3 blocks: every assignment of the sizes
    for (int n = 1; n <= 3; ++n) {
        int pick[3] = {0, 0, 0};
        for (;;) {
            for (int k = 0; k < n; ++k) bytes[k] = kSizes[pick[k]];
            all_masks(bytes, n);
            int k = 0;
            while (k < n && ++pick[k] == kNumSizes) pick[k++] = 0;
            if (k == n) break;
        }
    }
    std::printf("small tables checked\n");
    // 4 .. 8 blocks: every rotation and stride of the size table, all blocks of one size, and assignments drawn by a fixed generator
    for (int n = 4; n <= kMaxBlocks; ++n) {
        for (int stride = 0; stride < kNumSizes; ++stride)
            for (int shift = 0; shift < kNumSizes; ++shift) {
                for (int k = 0; k < n; ++k) bytes[k] = kSizes[(shift + k * stride) % kNumSizes];
                all_masks(bytes, n);
            }
        uint64_t state = 0x9E3779B97F4A7C15ull + (uint64_t)n;
        for (int draw = 0; draw < 64; ++draw) {
            for (int k = 0; k < n; ++k) {
                state = state * 6364136223846793005ull + 1442695040888963407ull;
                bytes[k] = kSizes[(state >> 33) % kNumSizes];
            }
            all_masks(bytes, n);
        }
    }
    std::printf("large tables checked\n");
    // the largest call: 8 blocks of the largest size, all present
    for (int k = 0; k < kMaxBlocks; ++k) bytes[k] = kLargest;
    bool present[kMaxBlocks];
    size_t offset[kMaxBlocks];
    for (int k = 0; k < kMaxBlocks; ++k) present[k] = true;
    const size_t total = spira::stage_layout(bytes, present, kMaxBlocks, offset);
    CHECK(total == kMaxBlocks * kLargest && offset[kMaxBlocks - 1] == (kMaxBlocks - 1) * kLargest, "the largest call: total %zu", total);
    // no block present: nothing to hold
    for (int k = 0; k < kMaxBlocks; ++k) present[k] = false;
    CHECK(spira::stage_layout(bytes, present, kMaxBlocks, offset) == 0, "no block present");
    CHECK(spira::stage_layout(bytes, present, 0, offset) == 0, "no block at all");
    std::printf("limits checked\n%lld cases\n", cases);
    if (failures) { std::printf("%d checks FAILED\n", failures); return 1; }
    std::printf("all checks passed\n");
    return 0;
}
