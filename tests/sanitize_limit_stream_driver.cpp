// Drives the pure-host side of limit streams (csrc/limit_plan.cpp: E(N) and grail_limit_stream_len, the ring's capacity, the
// checks of open, next and finish, the chunk count) under AddressSanitizer and UBSan (tests/test_limit_stream_sanitize.py
// builds and runs it): the lengths at the edges of 64 bits, the capacities of every look-ahead, every check; the device
// addresses are numbers nobody may look behind.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <initializer_list>
#include <limits>

#include "../include/grail_hip.h"
#include "../grail-rs_amd/csrc/limit_plan.h"

#define CHECK(cond)                                                                  \
    do {                                                                             \
        if (!(cond)) {                                                               \
            std::fprintf(stderr, "sanitize limit stream driver: %s failed (line %d)\n", #cond, __LINE__); \
            return 1;                                                                \
        }                                                                            \
    } while (0)

int main()
{
    // the lengths: E(N) = max(0, N - LAMBDA), a call writes E(N + n) - E(N), finish min(N, LAMBDA)
    for (uint32_t ell = 0; ell <= GRAIL_LIMIT_LOOKAHEAD_LOG2_MAX; ++ell) {
        const uint64_t lam = GRAIL_LIMIT_STREAM_DELAY(ell);
        CHECK(lam == ((uint64_t)1 << ell) + 10 && grail::limit_stream_delay(ell) == lam);
        for (uint64_t N : {(uint64_t)0, (uint64_t)1, lam - 1, lam, lam + 1, (uint64_t)1 << 40, UINT64_MAX - 4800, UINT64_MAX}) {
            const uint64_t known = N > lam ? N - lam : 0;
            CHECK(grail::limit_stream_known(N, ell) == known);
            uint64_t got = 77;
            for (uint64_t n : {(uint64_t)0, (uint64_t)1, lam, lam + 1, (uint64_t)480, (uint64_t)4800}) {
                if (N > UINT64_MAX - n) {
                    CHECK(grail_limit_stream_len(N, n, ell, 0, &got) == GRAIL_ERR_INVALID_ARG);
                    continue;
                }
                CHECK(grail_limit_stream_len(N, n, ell, 0, &got) == GRAIL_OK);
                CHECK(got == (N + n > lam ? N + n - lam : 0) - known && got <= n);
            }
            CHECK(grail_limit_stream_len(N, 0, ell, 1, &got) == GRAIL_OK && got == (N < lam ? N : lam) && known + got == N);
        }
        // the ring: 3 L + 19 rounded up to a power of two, at most 16 KB a row
        const uint32_t cap = grail::limit_stream_ring_capacity(ell), need = 3u * (1u << ell) + 19u;
        CHECK(cap >= need && (cap & (cap - 1)) == 0 && cap / 2 < need && cap % 4 == 0 && cap * 4u <= 16384u);
    }
    CHECK(grail::limit_stream_ring_capacity(0) == 32 && grail::limit_stream_ring_capacity(8) == 1024);
    CHECK(grail::limit_stream_ring_capacity(10) == 4096);
    uint64_t n_out = 77;
    CHECK(grail_limit_stream_len(5, 1, 11, 0, &n_out) == GRAIL_ERR_INVALID_ARG && grail_limit_stream_len(5, 1, 0xFFFFFFFFu, 0, &n_out) == GRAIL_ERR_INVALID_ARG);
    CHECK(grail_limit_stream_len(5, 1, 8, 0, nullptr) == GRAIL_ERR_INVALID_ARG);
    CHECK(grail_limit_stream_len(5, 1, 8, 1, &n_out) == GRAIL_ERR_INVALID_ARG);                     // finish feeds nothing
    CHECK(grail_limit_stream_len(UINT64_MAX, 1, 8, 0, &n_out) == GRAIL_ERR_INVALID_ARG);
    CHECK(grail_limit_stream_len((uint64_t)1 << 63, (uint64_t)1 << 63, 8, 0, &n_out) == GRAIL_ERR_INVALID_ARG && n_out == 77);
    CHECK(grail_limit_stream_len(0, UINT64_MAX, 10, 0, &n_out) == GRAIL_OK && n_out == UINT64_MAX - 1034);
    CHECK(grail_limit_stream_len(UINT64_MAX - 1, 1, 0, 0, &n_out) == GRAIL_OK && n_out == 1);
    CHECK(grail_limit_stream_len(UINT64_MAX, 0, 10, 1, &n_out) == GRAIL_OK && n_out == 1034);

    // open: what grail_limit_async refuses, and no rows
    const float inf = std::numeric_limits<float>::infinity(), nan = std::nanf("");
    CHECK(grail::limit_stream_open_error(4, 1, 0.5f, 8) == nullptr && grail::limit_stream_open_error(4, 2, 1e-45f, 0) == nullptr);
    CHECK(grail::limit_stream_open_error(4, 4, 3.4028234663852886e38f, 10) == nullptr);
    CHECK(grail::limit_stream_open_error(4, 1, 0.5f, 11) != nullptr && grail::limit_stream_open_error(4, 1, 0.5f, 0xFFFFFFFFu) != nullptr);
    CHECK(grail::limit_stream_open_error(4, 0, 0.5f, 8) != nullptr && grail::limit_stream_open_error(4, 3, 0.5f, 8) != nullptr);
    CHECK(grail::limit_stream_open_error(4, 8, 0.5f, 8) != nullptr && grail::limit_stream_open_error(0, 1, 0.5f, 8) != nullptr);
    CHECK(grail::limit_stream_open_error(4, 1, 0.0f, 8) != nullptr && grail::limit_stream_open_error(4, 1, -0.5f, 8) != nullptr);
    CHECK(grail::limit_stream_open_error(4, 1, nan, 8) != nullptr && grail::limit_stream_open_error(4, 1, inf, 8) != nullptr);
    CHECK(grail::limit_stream_open_error(4, 1, -inf, 8) != nullptr);

    // next: addresses are compared, never looked behind
    const void *a = (const void *)(uintptr_t)0x10000000, *b = (const void *)(uintptr_t)0x20000000, *ln = (const void *)(uintptr_t)0x30000000;
    uint64_t chunks = 77;
    CHECK(grail::limit_stream_next_error(a, 4800, ln, 8, 2, b, 4800, &chunks) == nullptr && chunks == 2);
    CHECK(grail::limit_stream_next_error(a, 4096, ln, 8, 1, b, 4100, &chunks) == nullptr && chunks == 1);
    CHECK(grail::limit_stream_next_error(a, 4097, ln, 8, 1, b, 4100, &chunks) == nullptr && chunks == 2);
    CHECK(grail::limit_stream_next_error(a, 4800, ln, 8, 2, b, 4799, &chunks) != nullptr && chunks == 0);
    CHECK(grail::limit_stream_next_error(nullptr, 0, ln, 8, 2, nullptr, 0, &chunks) == nullptr && chunks == 0);
    CHECK(grail::limit_stream_next_error(a, 64, nullptr, 8, 2, b, 64, &chunks) != nullptr);
    CHECK(grail::limit_stream_next_error(nullptr, 64, ln, 8, 2, b, 64, &chunks) != nullptr && grail::limit_stream_next_error(a, 64, ln, 8, 2, nullptr, 64, &chunks) != nullptr);
    CHECK(grail::limit_stream_next_error(nullptr, 0, nullptr, 8, 2, nullptr, 0, &chunks) != nullptr);
    // overlapping ranges: out inside in, out's end inside in, in inside out; next to one another is fine
    const void *in_end = (const void *)((uintptr_t)a + 8u * 64u * 4u), *before = (const void *)((uintptr_t)a - 8u * 64u * 4u);
    CHECK(grail::limit_stream_next_error(a, 64, ln, 8, 1, in_end, 64, &chunks) == nullptr && grail::limit_stream_next_error(a, 64, ln, 8, 1, before, 64, &chunks) == nullptr);
    CHECK(grail::limit_stream_next_error(a, 64, ln, 8, 1, a, 64, &chunks) != nullptr);
    CHECK(grail::limit_stream_next_error(a, 64, ln, 8, 1, (const void *)((uintptr_t)in_end - 4u), 64, &chunks) != nullptr);
    CHECK(grail::limit_stream_next_error(a, 64, ln, 8, 1, (const void *)((uintptr_t)before + 4u), 64, &chunks) != nullptr);
    // spans and chunk counts that do not fit; a call feeds a row fewer than 2^32 samples, so a group has at most 2^20 chunks
    CHECK(grail::limit_stream_next_error(a, (uint64_t)1 << 58, ln, 8, 1, (const void *)((uintptr_t)1 << 63), (uint64_t)1 << 58, &chunks) != nullptr);
    CHECK(grail::limit_stream_next_error(a, (uint64_t)1 << 40, ln, 3, 1, (const void *)((uintptr_t)1 << 60), (uint64_t)1 << 40, &chunks) == nullptr &&
          chunks == (0xFFFFFFFFull + 4095) / 4096);
    CHECK(grail::limit_stream_next_error(a, (uint64_t)1 << 33, ln, 4096, 1, (const void *)((uintptr_t)1 << 60), (uint64_t)1 << 33, &chunks) != nullptr);
    CHECK(grail::limit_stream_next_error(a, (uint64_t)1 << 33, ln, 4096, 4, (const void *)((uintptr_t)1 << 60), (uint64_t)1 << 33, &chunks) == nullptr);
    CHECK(grail::limit_stream_next_error(a, UINT64_MAX, ln, 1, 1, b, UINT64_MAX, &chunks) != nullptr);

    // finish: room for LAMBDA outputs a row
    CHECK(grail::limit_stream_finish_error(b, 266, 8, 2, 8, &chunks) == nullptr && chunks == 1);
    CHECK(grail::limit_stream_finish_error(b, 265, 8, 2, 8, &chunks) != nullptr && chunks == 0);
    CHECK(grail::limit_stream_finish_error(nullptr, 266, 8, 2, 8, &chunks) != nullptr);
    CHECK(grail::limit_stream_finish_error(b, 11, 1, 1, 0, &chunks) == nullptr && grail::limit_stream_finish_error(b, 10, 1, 1, 0, &chunks) != nullptr);
    CHECK(grail::limit_stream_finish_error(b, 1034, 0x7FFFFFFFu, 1, 10, &chunks) == nullptr && chunks == 1);
    CHECK(grail::limit_stream_finish_error(b, 1034, 0xFFFFFFFFu, 1, 10, &chunks) != nullptr);
    CHECK(grail::limit_stream_finish_error(b, (uint64_t)1 << 58, 8, 1, 8, &chunks) != nullptr);
    std::printf("sanitize limit stream driver: ok\n");
    return 0;
}
