// Drives the pure-host resampling functions of csrc/resample_plan.cpp under AddressSanitizer and UBSan
// (tests/test_resample_sanitize.py builds and runs it): every table lives on the heap at exactly up * taps entries, so
// that a read or write one element past it is caught.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <memory>

#include "../include/grail_hip.h"

#define CHECK(cond)                                                                  \
    do {                                                                             \
        if (!(cond)) {                                                               \
            std::fprintf(stderr, "sanitize resample driver: %s failed (line %d)\n", #cond, __LINE__); \
            return 1;                                                                \
        }                                                                            \
    } while (0)

int main()
{
    const uint32_t pairs[][2] = {{48000, 16000}, {48000, 8000}, {44100, 48000}, {48000, 44100}, {44100, 16000}, {48000, 96000},
                                 {48000, 22050}, {44100, 8000}, {48000, 11025}, {2, 3}, {3, 2}, {5, 7}, {682, 1}, {1, 682}};
    for (const auto &pair : pairs) {
        uint32_t U = 0, D = 0, P = 0;
        CHECK(grail_resample_ratio(pair[0], pair[1], &U, &D, &P) == GRAIL_OK);
        CHECK(U && D && P >= 2u * GRAIL_RESAMPLE_ZERO_CROSSINGS && P % 2 == 0 && U * P <= GRAIL_RESAMPLE_TABLE_MAX);
        CHECK((uint64_t)pair[0] * U == (uint64_t)pair[1] * D);
        const uint32_t cells = U * P;
        std::unique_ptr<int32_t[]> num(new int32_t[cells]);
        for (uint32_t i = 0; i < cells; ++i) num[i] = INT32_MIN;
        // one entry short: refused before anything is written
        CHECK(grail_resample_coefficients(pair[0], pair[1], num.get(), cells - 1) == GRAIL_ERR_INVALID_ARG);
        CHECK(grail_resample_coefficients(pair[0], pair[1], nullptr, cells) == GRAIL_ERR_INVALID_ARG);
        for (uint32_t i = 0; i < cells; ++i) CHECK(num[i] == INT32_MIN);
        CHECK(grail_resample_coefficients(pair[0], pair[1], num.get(), cells) == GRAIL_OK);
        // N(j) sits at num[p * P + k] with j = (k - P/2) U + p: bounds, and N(j) = N(-j) wherever -j is in the table
        const int64_t half = (int64_t)(P / 2) * U;
        const auto N = [&](int64_t j) {
            const int64_t at = j + half;
            return num[(size_t)(at % U) * P + (size_t)(at / U)];
        };
        int64_t sum = 0;
        for (int64_t j = -half; j < half; ++j) {
            CHECK(N(j) > -(1 << 26) && N(j) < (1 << 26));
            if (j > -half) CHECK(N(j) == N(-j));
            sum += N(j);
        }
        CHECK(N(0) > 0 && sum > 0);
        uint64_t n_out = 0;
        for (uint64_t n : {(uint64_t)0, (uint64_t)1, (uint64_t)D, (uint64_t)0xFFFFFFFFull, (uint64_t)1 << 40}) {
            CHECK(grail_resample_len(n, pair[0], pair[1], &n_out) == GRAIL_OK);
            CHECK(n_out * D >= n * U && (n_out == 0 || (n_out - 1) * D < n * U));
        }
    }
    const uint32_t refused[][2] = {{48000, 48000}, {0, 48000}, {48000, 0}, {0, 0}, {48000, 44101}, {11025, 96000}, {96000, 11025},
                                   {0xFFFFFFFFu, 0xFFFFFFFEu}, {683, 1}, {1, 683}};
    for (const auto &pair : refused) {
        uint32_t U = 7, D = 7, P = 7;
        int32_t one = 77;
        uint64_t n_out = 77;
        CHECK(grail_resample_ratio(pair[0], pair[1], &U, &D, &P) == GRAIL_ERR_INVALID_ARG && U == 7 && D == 7 && P == 7);
        CHECK(grail_resample_coefficients(pair[0], pair[1], &one, 0xFFFFFFFFu) == GRAIL_ERR_INVALID_ARG && one == 77);
        CHECK(grail_resample_len(1000, pair[0], pair[1], &n_out) == GRAIL_ERR_INVALID_ARG && n_out == 77);
    }
    uint64_t n_out = 77;
    CHECK(grail_resample_len(UINT64_MAX, 16000, 48000, &n_out) == GRAIL_ERR_INVALID_ARG && n_out == 77);
    CHECK(grail_resample_len(UINT64_MAX, 48000, 16000, &n_out) == GRAIL_OK && n_out == UINT64_MAX / 3);
    CHECK(grail_resample_len(1, 48000, 16000, nullptr) == GRAIL_ERR_INVALID_ARG);
    CHECK(grail_resample_ratio(48000, 16000, nullptr, nullptr, nullptr) == GRAIL_OK);
    std::printf("sanitize resample driver: ok\n");
    return 0;
}
