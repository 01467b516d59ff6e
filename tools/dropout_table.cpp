// Prints the table C_VALUES of tests/test_dropout_restate.py: the dropout generator of csrc/common.h evaluated by the C functions
// themselves on the host.  No device code and no GPU:
//   hipcc -O1 -o dropout_table tools/dropout_table.cpp && ./dropout_table
// pair_seed is a __device__ function of csrc/attention_common.h (a header full of device code); its single line is restated below,
// character for character, in terms of the header's rlt_mix32.
#define RLT_HOST_ONLY
#include "../ranked-list-truncation_amd/csrc/common.h"
#include <cmath>
#include <cstdio>
#include <cstring>

static uint32_t pair_seed(uint32_t seed, int pair) { return rlt_mix32(seed ^ ((uint32_t)pair * 0x9E3779B9U)); }

static void row(uint32_t seed, uint32_t r, uint32_t c, int pair, float p) {
    uint32_t pbits;
    std::memcpy(&pbits, &p, 4);
    const uint32_t thr = rlt_drop_threshold(p), ps = pair_seed(seed, pair);
    std::printf("    ((0x%08X, 0x%08X, 0x%08X, %d, 0x%08X), 0x%08X, 0x%08X, 0x%08X, %d, %d),\n", seed, r, c, pair, pbits,
                rlt_col_hash(seed, c), ps, thr, (int)rlt_keep(seed, r, c, thr), (int)rlt_keep(ps, r, c, thr));
}

int main() {
    const uint32_t top = 0xFFFFFFFFu;
    const float below_one = std::nextafterf(1.0f, 0.0f);
    const float corner_p[] = {0.0f, 0.5f, below_one};
    std::printf("# (seed, row, col, pair, p as float32 bits) -> col_hash(seed, col), pair_seed(seed, pair), drop_threshold(p), "
                "keep(seed, row, col), keep(pair_seed, row, col)\n");
    // the corners: p = 0, 0.5 and the float32 just below 1, at row / col = 0 and 0xFFFFFFFF, seed 0 and not
    const uint32_t rc[][2] = {{0u, 0u}, {0u, top}, {top, 0u}, {top, top}};
    for (int k = 0; k < 4; ++k)
        for (int j = 0; j < 3; ++j) {
            row(0u, rc[k][0], rc[k][1], k, corner_p[j]);
            row(12345u, rc[k][0], rc[k][1], 3 - k, corner_p[j]);
        }
    // a walk over seeds, indices, pairs and rates
    const float ps[] = {0.1f, 0.3f, 0.9f, std::nextafterf(0.0f, 1.0f), 1.0f - 1.0f / 4096.0f, 0.5f, 0.25f, std::nextafterf(0.5f, 1.0f)};
    const uint32_t seeds[] = {1u, 4321u, top, 0x80000000u, 0u, 777u};
    const uint32_t idx[] = {1u, 63u, 64u, 515u, 0x7FFFFFFFu, 0x80000000u, 2047u, 0u};
    const int pairs[] = {0, 1, 3, 4095, 0x7FFFFFFF};
    for (int i = 0; i < 16; ++i) row(seeds[i % 6], idx[(i * 3) % 8], idx[(i * 5 + 1) % 8], pairs[i % 5], ps[i % 8]);
    // the clamp: the float32 just below 1 gives 2^32 - 256 and does not reach it; only p >= 1 does (the entry points refuse p = 1)
    row(12345u, 5u, 7u, 1, 1.0f);
    row(4321u, top, 0u, 2, 2.0f);
    std::printf("# rlt_row_hash(12345, 999) = 0x%08X (tests/test_compare_restate.py has the same value)\n", rlt_row_hash(12345u, 999u));
    return 0;
}
