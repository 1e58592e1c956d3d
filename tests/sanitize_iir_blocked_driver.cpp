// Drives the pure-host functions that csrc/iir_plan.cpp has for recursive filtering parallel in time (grail_biquad_block_matrix, the
// set's matrix image, the grid and the scratch size) under AddressSanitizer and UBSan (tests/test_iir_blocked_sanitize.py
// builds and runs it): every array lives on the heap at exactly the size the call is entitled to, so that a read or write
// one element past it is caught, and the sizes are walked at the edges of 32 and 64 bits.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <limits>
#include <memory>
#include <vector>

#include "../include/grail_hip.h"
#include "../grail-rs_amd/csrc/iir_plan.h"

#define CHECK(cond)                                                                  \
    do {                                                                             \
        if (!(cond)) {                                                               \
            std::fprintf(stderr, "sanitize iir blocked driver: %s failed (line %d)\n", #cond, __LINE__); \
            return 1;                                                                \
        }                                                                            \
    } while (0)

int main()
{
    const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
    // the matrix of S sections into exactly [2 S][2 S] doubles from exactly 5 S: finite for a stable filter, and no state
    // reached from a later section
    for (uint32_t S = 1; S <= GRAIL_IIR_SECTIONS_MAX; ++S) {
        std::unique_ptr<double[]> coef(new double[5 * S]);
        for (uint32_t j = 0; j < S; ++j)
            CHECK(grail_iir_design(GRAIL_IIR_LOWPASS + (int)(j % 7), 48000, 100.0 + 700.0 * j, 0.7 + j, 3.0, coef.get() + 5 * j) == GRAIL_OK);
        std::unique_ptr<double[]> m(new double[4 * S * S]);
        for (uint32_t k = 0; k < 4 * S * S; ++k) m[k] = 77.0;
        CHECK(grail_biquad_block_matrix(coef.get(), S, m.get()) == GRAIL_OK);
        for (uint32_t i = 0; i < 2 * S; ++i)
            for (uint32_t c = 0; c < 2 * S; ++c) {
                const double t = m[i * 2 * S + c];
                CHECK(std::isfinite(t) && std::fabs(t) < 10.0 && (c <= 2 * (i / 2) + 1 || t == 0.0));
            }
        // the refusals write nothing
        for (uint32_t k = 0; k < 4 * S * S; ++k) m[k] = 77.0;
        CHECK(grail_biquad_block_matrix(nullptr, S, m.get()) == GRAIL_ERR_INVALID_ARG && grail_biquad_block_matrix(coef.get(), S, nullptr) == GRAIL_ERR_INVALID_ARG);
        coef[5 * S - 1] = nan;
        CHECK(grail_biquad_block_matrix(coef.get(), S, m.get()) == GRAIL_ERR_INVALID_ARG);
        coef[5 * S - 1] = 0.5, coef[0] = -inf;
        CHECK(grail_biquad_block_matrix(coef.get(), S, m.get()) == GRAIL_ERR_INVALID_ARG);
        for (uint32_t k = 0; k < 4 * S * S; ++k) CHECK(m[k] == 77.0);
    }
    {
        std::unique_ptr<double[]> coef(new double[5]), m(new double[4]);
        for (int k = 0; k < 5; ++k) coef[k] = 0.25;
        for (int k = 0; k < 4; ++k) m[k] = 77.0;
        for (uint32_t S : {0u, 9u, 0x80000000u, 0xFFFFFFFFu}) CHECK(grail_biquad_block_matrix(coef.get(), S, m.get()) == GRAIL_ERR_INVALID_ARG);
        for (int k = 0; k < 4; ++k) CHECK(m[k] == 77.0);
        // an unstable pole overflows in the matrix as it would in the row: said in the numbers, not refused
        coef[0] = 1.0, coef[1] = coef[2] = coef[4] = 0.0, coef[3] = -4.0;
        CHECK(grail_biquad_block_matrix(coef.get(), 1, m.get()) == GRAIL_OK && !std::isfinite(m[0]));
    }

    // a set's matrices: [F][16][16], filter f's own 2 S x 2 S in the corner, +0.0 elsewhere
    for (uint32_t F : {1u, 3u, 64u}) {
        std::unique_ptr<uint32_t[]> S(new uint32_t[F]);
        uint32_t total = 0;
        for (uint32_t f = 0; f < F; ++f) {
            S[f] = F == 1 ? 1u : (f % 3 == 0 ? 1u : f % 3 == 1 ? 7u : 8u);
            total += 5 * S[f];
        }
        std::unique_ptr<double[]> coef(new double[total]);
        for (uint32_t i = 0; i < total; ++i) coef[i] = ((double)(i % 17) - 8.25) / 64.0;
        std::vector<double> image, matrices;
        std::vector<uint32_t> sections;
        uint32_t bound = 0;
        grail::iir_set_image(coef.get(), S.get(), F, image, sections, &bound);
        grail::iir_block_image(image, sections, matrices);
        CHECK(matrices.size() == (size_t)F * grail::IIR_MATRIX_DOUBLES && grail::IIR_MATRIX_DOUBLES == 256);
        size_t from = 0;
        for (uint32_t f = 0; f < F; ++f) {
            std::unique_ptr<double[]> own(new double[4 * S[f] * S[f]]);
            CHECK(grail_biquad_block_matrix(coef.get() + from, S[f], own.get()) == GRAIL_OK);
            for (uint32_t i = 0; i < 16; ++i)
                for (uint32_t c = 0; c < 16; ++c) {
                    const double got = matrices[(size_t)f * 256 + i * 16 + c];
                    if (i < 2 * S[f] && c < 2 * S[f]) {
                        const double want = own[i * 2 * S[f] + c];
                        CHECK(got == want && std::signbit(got) == std::signbit(want));
                    } else {
                        CHECK(got == 0.0 && !std::signbit(got));
                    }
                }
            from += 5 * S[f];
        }
    }

    // the grid and the scratch at the edges: row_stride 0, 1, 1024, 2^32 - 1 with tail 0 and 2^32 - 1
    const uint64_t top = 0xFFFFFFFFull;
    struct Edge {
        uint64_t row_stride;
        uint32_t tail;
        uint64_t blocks, groups;
    };
    const Edge edges[] = {{0, 0, 0, 0},
                          {1, 0, 1, 1},
                          {1024, 0, 1, 1},
                          {top, 0, 1ull << 22, 1ull << 16},
                          {0, 0xFFFFFFFFu, 1ull << 22, 1ull << 16},
                          {1, 0xFFFFFFFFu, 1ull << 22, 1ull << 16},
                          {1024, 0xFFFFFFFFu, (1ull << 22) + 1, (1ull << 16) + 1},
                          {top, 0xFFFFFFFFu, 1ull << 23, 1ull << 17}};
    for (const Edge &e : edges) {
        const uint64_t blocks = grail::iir_block_grid_blocks(e.row_stride, e.tail);
        CHECK(blocks == e.blocks && grail::iir_block_groups(blocks) == e.groups);
        // every step of the longest row has a block, and no block is idle for all rows
        CHECK(blocks * grail::IIR_BLOCK >= e.row_stride + e.tail && (blocks == 0 || (blocks - 1) * grail::IIR_BLOCK < e.row_stride + e.tail));
        for (uint32_t bound : {1u, 2u, 4u, 8u})
            for (uint32_t n_rows : {0u, 1u, 64u, 0xFFFFFFFFu}) {
                const uint64_t doubles = grail::iir_block_scratch_doubles(n_rows, blocks, bound);
                CHECK(doubles == (uint64_t)n_rows * blocks * 2 * bound);        // (2^32 * 2^23 * 16 < 2^64: none of these saturates)
            }
    }
    // a stride past 32 bits counts as 2^32 - 1 samples (len is 32 bits wide); 1025 steps are two blocks, 65 blocks two groups
    CHECK(grail::iir_block_grid_blocks(1ull << 40, 0) == 1ull << 22 && grail::iir_block_grid_blocks(UINT64_MAX, 0xFFFFFFFFu) == 1ull << 23);
    CHECK(grail::iir_block_grid_blocks(1024, 1) == 2 && grail::iir_block_grid_blocks(1023, 1) == 1 && grail::iir_block_grid_blocks(0, 1) == 1);
    CHECK(grail::iir_block_groups(64) == 1 && grail::iir_block_groups(65) == 2 && grail::iir_block_groups(UINT64_MAX) == (1ull << 58));
    // ... and a product past 64 bits saturates
    CHECK(grail::iir_block_scratch_doubles(0xFFFFFFFFu, 1ull << 60, 8) == UINT64_MAX && grail::iir_block_scratch_doubles(0, 1ull << 59, 8) == 0);
    CHECK(grail::iir_block_scratch_doubles(2, 1ull << 58, 8) == 1ull << 63 && grail::iir_block_scratch_doubles(3, 1ull << 59, 8) == UINT64_MAX);
    std::printf("sanitize iir blocked driver: ok\n");
    return 0;
}
