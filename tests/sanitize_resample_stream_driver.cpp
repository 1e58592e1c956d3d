// Drives the pure-host side of resample streams (csrc/resample_plan.cpp: grail_resample_stream_len, the ring's capacity, the
// checks of next and finish) under AddressSanitizer and UBSan (tests/test_resample_stream_sanitize.py builds and runs it): the
// lengths against the closed form in 128 bits and against the incremental form the device keeps; the device addresses are
// numbers nobody may look behind.
#include <cstdint>
#include <cstdio>
#include <initializer_list>

#include "../include/grail_hip.h"
#include "../grail-rs_amd/csrc/resample_plan.h"

#define CHECK(cond)                                                                  \
    do {                                                                             \
        if (!(cond)) {                                                               \
            std::fprintf(stderr, "sanitize resample stream driver: %s failed (line %d)\n", #cond, __LINE__); \
            return 1;                                                                \
        }                                                                            \
    } while (0)

typedef unsigned __int128 u128;

static u128 known(uint64_t N, uint32_t U, uint32_t D, uint32_t P)
{
    const uint64_t h = P / 2;
    return N <= h ? 0 : ((u128)(N - h) * U + (D - 1)) / D;
}

int main()
{
    const uint32_t pairs[][2] = {{2, 3}, {3, 2}, {48000, 16000}, {48000, 96000}, {44100, 48000}, {48000, 44100},
                                 {44100, 16000}, {48000, 11025}, {50, 3}, {48000, 2000}, {8000, 96000}, {96000, 8000}};
    for (const auto &pr : pairs) {
        uint32_t U = 0, D = 0, P = 0;
        CHECK(grail_resample_ratio(pr[0], pr[1], &U, &D, &P) == GRAIL_OK);
        const uint64_t h = P / 2;
        for (uint64_t N : {(uint64_t)0, (uint64_t)1, h - 1, h, h + 1, (uint64_t)P, (uint64_t)1 << 40, ((uint64_t)1 << 62) - 1}) {
            uint64_t got = 77, whole = 77;
            for (uint64_t n : {(uint64_t)0, (uint64_t)1, h, h + 1, (uint64_t)480, (uint64_t)4800}) {
                CHECK(grail_resample_stream_len(N, n, pr[0], pr[1], 0, &got) == GRAIL_OK);
                CHECK((u128)got == known(N + n, U, D, P) - known(N, U, D, P) && (u128)got <= grail::resample_stream_most(n, U, D));
            }
            CHECK(grail_resample_stream_len(N, 0, pr[0], pr[1], 1, &got) == GRAIL_OK);
            CHECK((u128)got == grail::resample_stream_most(N, U, D) - known(N, U, D, P) && got <= grail::resample_stream_tail(U, D, P));
            CHECK((N == 0) == (got == 0));
            if (N < ((uint64_t)1 << 50)) CHECK(grail_resample_len(N, pr[0], pr[1], &whole) == GRAIL_OK && known(N, U, D, P) + got == (u128)whole);
        }
        // the incremental form: i = floor(M D / U), p = M D mod U, never a product of N, from N near 2^62 on
        uint64_t N = ((uint64_t)1 << 62) - 200000;
        const u128 M0 = known(N, U, D, P);
        uint64_t i = (uint64_t)(M0 * D / U);
        uint32_t p = (uint32_t)(M0 * D % U);
        for (uint32_t n : {0u, 1u, 480u, 4800u, 7u, 0u, 44100u}) {
            uint64_t got = 77;
            CHECK(grail_resample_stream_len(N, n, pr[0], pr[1], 0, &got) == GRAIL_OK);
            const int64_t T = (int64_t)(N + n) - 1 - (int64_t)h;
            const uint64_t c = T < (int64_t)i ? 0 : ((uint64_t)(T - (int64_t)i + 1) * U - p + (D - 1)) / D;
            CHECK(c == got && (T < (int64_t)i || (uint64_t)(T - (int64_t)i + 1) * U < ((uint64_t)1 << 44)));
            const uint64_t a = p + c * D;
            i += a / U, p = (uint32_t)(a % U), N += n;
        }
        // the ring: P - 1 rounded up to a power of two
        const uint32_t cap = grail::resample_stream_ring_capacity(P);
        CHECK(cap >= P - 1 && (cap & (cap - 1)) == 0 && cap / 2 < P - 1 && cap <= 32768);
    }
    CHECK(grail::resample_stream_ring_capacity(48) == 64 && grail::resample_stream_ring_capacity(64) == 64);
    CHECK(grail::resample_stream_ring_capacity(66) == 128 && grail::resample_stream_ring_capacity(32768) == 32768);

    uint64_t n_out = 77;
    CHECK(grail_resample_stream_len(5, 1, 0, 8000, 0, &n_out) == GRAIL_ERR_INVALID_ARG && grail_resample_stream_len(5, 1, 8000, 8000, 0, &n_out) == GRAIL_ERR_INVALID_ARG);
    CHECK(grail_resample_stream_len(5, 1, 11025, 96000, 0, &n_out) == GRAIL_ERR_INVALID_ARG && grail_resample_stream_len(5, 1, 48000, 16000, 0, nullptr) == GRAIL_ERR_INVALID_ARG);
    CHECK(grail_resample_stream_len(5, 1, 48000, 16000, 1, &n_out) == GRAIL_ERR_INVALID_ARG);            // finish feeds nothing
    CHECK(grail_resample_stream_len(UINT64_MAX, 1, 48000, 16000, 0, &n_out) == GRAIL_ERR_INVALID_ARG);
    CHECK(grail_resample_stream_len(0, UINT64_MAX, 8000, 96000, 0, &n_out) == GRAIL_ERR_INVALID_ARG && n_out == 77);
    CHECK(grail_resample_stream_len(UINT64_MAX, 0, 8000, 96000, 1, &n_out) == GRAIL_OK && n_out == 288);
    CHECK(grail_resample_stream_len(0, UINT64_MAX, 96000, 8000, 0, &n_out) == GRAIL_OK && n_out == (UINT64_MAX - 288 + 11) / 12);

    // next: addresses are compared, never looked behind; 48 000 -> 16 000 is 1 / 3, 8 000 -> 96 000 is 12 / 1
    const void *a = (const void *)(uintptr_t)0x10000000, *b = (const void *)(uintptr_t)0x20000000, *ln = (const void *)(uintptr_t)0x30000000;
    uint64_t chunks = 77;
    CHECK(grail::resample_stream_next_error(a, 4800, ln, 8, b, 1600, 1, 3, &chunks) == nullptr && chunks == 2);
    CHECK(grail::resample_stream_next_error(a, 4800, ln, 8, b, 1599, 1, 3, &chunks) != nullptr && chunks == 0);
    CHECK(grail::resample_stream_next_error(a, 4801, ln, 8, b, 1600, 1, 3, &chunks) != nullptr);
    CHECK(grail::resample_stream_next_error(a, 4801, ln, 8, b, 1601, 1, 3, &chunks) == nullptr && chunks == 2);
    CHECK(grail::resample_stream_next_error(a, 480, ln, 8, b, 5760, 12, 1, &chunks) == nullptr && chunks == 6);
    CHECK(grail::resample_stream_next_error(a, 480, ln, 8, b, 5759, 12, 1, &chunks) != nullptr);
    CHECK(grail::resample_stream_next_error(a, 441, ln, 8, b, 480, 160, 147, &chunks) == nullptr && chunks == 1);
    CHECK(grail::resample_stream_next_error(a, 442, ln, 8, b, 481, 160, 147, &chunks) != nullptr);
    CHECK(grail::resample_stream_next_error(nullptr, 0, ln, 8, nullptr, 0, 1, 3, &chunks) == nullptr && chunks == 0);
    CHECK(grail::resample_stream_next_error(a, 64, nullptr, 8, b, 64, 1, 3, &chunks) != nullptr);
    CHECK(grail::resample_stream_next_error(nullptr, 64, ln, 8, b, 64, 1, 3, &chunks) != nullptr && grail::resample_stream_next_error(a, 64, ln, 8, nullptr, 64, 1, 3, &chunks) != nullptr);
    CHECK(grail::resample_stream_next_error(nullptr, 0, nullptr, 8, nullptr, 0, 1, 3, &chunks) != nullptr);
    // overlapping ranges: out inside in, out's end inside in, in inside out; next to one another is fine
    const void *in_end = (const void *)((uintptr_t)a + 8u * 64u * 4u), *before = (const void *)((uintptr_t)a - 8u * 64u * 4u);
    CHECK(grail::resample_stream_next_error(a, 64, ln, 8, in_end, 64, 1, 3, &chunks) == nullptr && grail::resample_stream_next_error(a, 64, ln, 8, before, 64, 1, 3, &chunks) == nullptr);
    CHECK(grail::resample_stream_next_error(a, 64, ln, 8, a, 64, 1, 3, &chunks) != nullptr);
    CHECK(grail::resample_stream_next_error(a, 64, ln, 8, (const void *)((uintptr_t)in_end - 4u), 64, 1, 3, &chunks) != nullptr);
    CHECK(grail::resample_stream_next_error(a, 64, ln, 8, (const void *)((uintptr_t)before + 4u), 64, 1, 3, &chunks) != nullptr);
    // spans, rows of 2^32 outputs and chunk counts that do not fit
    CHECK(grail::resample_stream_next_error(a, (uint64_t)1 << 58, ln, 8, (const void *)((uintptr_t)1 << 63), (uint64_t)1 << 58, 1, 3, &chunks) != nullptr);
    CHECK(grail::resample_stream_next_error(a, (uint64_t)1 << 29, ln, 1, (const void *)((uintptr_t)1 << 50), (uint64_t)1 << 33, 12, 1, &chunks) != nullptr);
    CHECK(grail::resample_stream_next_error(a, ((uint64_t)1 << 28), ln, 1, (const void *)((uintptr_t)1 << 50), (uint64_t)12 << 28, 12, 1, &chunks) == nullptr &&
          chunks == ((uint64_t)12 << 28) / 1024);
    CHECK(grail::resample_stream_next_error(a, 0xFFFFFFFFull, ln, 1024, (const void *)((uintptr_t)1 << 50), 0xFFFFFFFFull, 2, 3, &chunks) != nullptr);
    CHECK(grail::resample_stream_next_error(a, (uint64_t)1 << 40, ln, 3, (const void *)((uintptr_t)1 << 60), (uint64_t)1 << 40, 1, 3, &chunks) == nullptr &&
          chunks == ((0xFFFFFFFFull + 2) / 3 + 1023) / 1024);                          // (a call feeds a row fewer than 2^32 samples)
    CHECK(grail::resample_stream_next_error(a, UINT64_MAX, ln, 1, b, UINT64_MAX, 12, 1, &chunks) != nullptr);      // (12 * 2^64: no wrap)

    // finish: room for ceil(h U / D) outputs
    CHECK(grail::resample_stream_tail(1, 3, 144) == 24 && grail::resample_stream_tail(12, 1, 48) == 288 && grail::resample_stream_tail(160, 147, 48) == 27);
    CHECK(grail::resample_stream_finish_error(b, 24, 8, 1, 3, 144, &chunks) == nullptr && chunks == 1);
    CHECK(grail::resample_stream_finish_error(b, 23, 8, 1, 3, 144, &chunks) != nullptr && grail::resample_stream_finish_error(nullptr, 24, 8, 1, 3, 144, &chunks) != nullptr);
    CHECK(grail::resample_stream_finish_error(b, 288, 0x7FFFFFFFu, 12, 1, 48, &chunks) == nullptr && chunks == 1);
    CHECK(grail::resample_stream_finish_error(b, (uint64_t)1 << 58, 8, 1, 3, 144, &chunks) != nullptr);
    std::printf("sanitize resample stream driver: ok\n");
    return 0;
}
