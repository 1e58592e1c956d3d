// Drives the pure-host side of filter streams (csrc/fir_plan.cpp: grail_filter_stream_len, the ring's capacity, the checks of
// open, next and finish) under AddressSanitizer and UBSan (tests/test_fir_stream_sanitize.py builds and runs it): the host
// arrays live on the heap at exactly the size the call is entitled to, so that a read one element past them is caught, and
// the device addresses are numbers nobody may look behind.
#include <cstdint>
#include <cstdio>
#include <memory>

#include "../include/grail_hip.h"
#include "../grail-rs_amd/csrc/fir_plan.h"

#define CHECK(cond)                                                                  \
    do {                                                                             \
        if (!(cond)) {                                                               \
            std::fprintf(stderr, "sanitize fir stream driver: %s failed (line %d)\n", #cond, __LINE__); \
            return 1;                                                                \
        }                                                                            \
    } while (0)

static uint64_t known(uint64_t N, uint32_t o) { return N > o ? N - o : 0; }

int main()
{
    // lengths: a call writes E(N + n) - E(N), finish N + K - 1 - o - E(N) (0 for N = 0); together the one-shot length
    const uint32_t Ks[] = {1, 2, 8, 9, 4096};
    for (uint32_t K : Ks) {
        for (uint32_t o : {0u, (K - 1u) / 2u, K - 1u}) {
            for (uint64_t N : {(uint64_t)0, (uint64_t)1, (uint64_t)(o ? o - 1 : 0), (uint64_t)o, (uint64_t)o + 1, (uint64_t)1 << 40}) {
                uint64_t got = 77, whole = 77;
                for (uint64_t n : {(uint64_t)0, (uint64_t)1, (uint64_t)o, (uint64_t)K, (uint64_t)4800}) {
                    CHECK(grail_filter_stream_len(N, n, K, o, 0, &got) == GRAIL_OK && got == known(N + n, o) - known(N, o) && got <= n);
                }
                CHECK(grail_filter_stream_len(N, 0, K, o, 1, &got) == GRAIL_OK && grail_fir_len(N, K, o, &whole) == GRAIL_OK);
                CHECK(known(N, o) + got == whole && got <= K - 1);
            }
        }
    }
    uint64_t n_out = 77;
    CHECK(grail_filter_stream_len(5, 1, 0, 0, 0, &n_out) == GRAIL_ERR_INVALID_ARG && grail_filter_stream_len(5, 1, 4097, 0, 0, &n_out) == GRAIL_ERR_INVALID_ARG);
    CHECK(grail_filter_stream_len(5, 1, 9, 9, 0, &n_out) == GRAIL_ERR_INVALID_ARG && grail_filter_stream_len(5, 1, 9, 4, 0, nullptr) == GRAIL_ERR_INVALID_ARG);
    CHECK(grail_filter_stream_len(5, 1, 9, 4, 1, &n_out) == GRAIL_ERR_INVALID_ARG);                  // finish feeds nothing
    CHECK(grail_filter_stream_len(UINT64_MAX, 1, 1, 0, 0, &n_out) == GRAIL_ERR_INVALID_ARG);
    CHECK(grail_filter_stream_len(UINT64_MAX - 4094, 0, 4096, 0, 0, &n_out) == GRAIL_ERR_INVALID_ARG && n_out == 77);
    CHECK(grail_filter_stream_len(UINT64_MAX - 4095, 0, 4096, 0, 1, &n_out) == GRAIL_OK && n_out == 4095);

    // the ring: the longest K - 1 rounded up to a power of two, at least 1, at most 4096 samples
    const uint32_t caps[][2] = {{1, 1}, {2, 1}, {3, 2}, {8, 8}, {9, 8}, {10, 16}, {255, 256}, {257, 256}, {258, 512}, {4096, 4096}};
    for (const auto &c : caps) CHECK(grail::fir_stream_ring_capacity(c[0]) == c[1]);

    // open: the rows' filters, an array of exactly n_rows indices
    {
        std::unique_ptr<uint32_t[]> which(new uint32_t[5]{0, 3, 1, 2, 3});
        CHECK(grail::fir_stream_open_error(which.get(), 5, 4) == nullptr && grail::fir_stream_open_error(nullptr, 5, 4) == nullptr);
        CHECK(grail::fir_stream_open_error(which.get(), 5, 3) != nullptr && grail::fir_stream_open_error(which.get(), 1, 1) == nullptr);
        CHECK(grail::fir_stream_open_error(which.get(), 0, 4) != nullptr && grail::fir_stream_open_error(nullptr, 0, 4) != nullptr);
        which[4] = 0xFFFFFFFFu;
        CHECK(grail::fir_stream_open_error(which.get(), 5, 64) != nullptr && grail::fir_stream_open_error(which.get(), 4, 64) == nullptr);
    }

    // next: addresses are compared, never looked behind
    const void *a = (const void *)(uintptr_t)0x10000000, *b = (const void *)(uintptr_t)0x20000000, *ln = (const void *)(uintptr_t)0x30000000;
    uint64_t chunks = 77;
    CHECK(grail::fir_stream_next_error(a, 4800, ln, 8, b, 4800, &chunks) == nullptr && chunks == 3);
    CHECK(grail::fir_stream_next_error(a, 2048, ln, 8, b, 4096, &chunks) == nullptr && chunks == 1);
    CHECK(grail::fir_stream_next_error(a, 2049, ln, 8, b, 4096, &chunks) == nullptr && chunks == 2);
    CHECK(grail::fir_stream_next_error(nullptr, 0, ln, 8, nullptr, 0, &chunks) == nullptr && chunks == 0);
    CHECK(grail::fir_stream_next_error(a, 64, ln, 8, b, 63, &chunks) != nullptr && grail::fir_stream_next_error(a, 64, nullptr, 8, b, 64, &chunks) != nullptr);
    CHECK(grail::fir_stream_next_error(nullptr, 64, ln, 8, b, 64, &chunks) != nullptr && grail::fir_stream_next_error(a, 64, ln, 8, nullptr, 64, &chunks) != nullptr);
    CHECK(grail::fir_stream_next_error(nullptr, 0, nullptr, 8, nullptr, 0, &chunks) != nullptr);
    // overlapping ranges: out inside in, out's end inside in, in inside out; next to one another is fine
    const void *in_end = (const void *)((uintptr_t)a + 8u * 64u * 4u), *before = (const void *)((uintptr_t)a - 8u * 64u * 4u);
    CHECK(grail::fir_stream_next_error(a, 64, ln, 8, in_end, 64, &chunks) == nullptr && grail::fir_stream_next_error(a, 64, ln, 8, before, 64, &chunks) == nullptr);
    CHECK(grail::fir_stream_next_error(a, 64, ln, 8, a, 64, &chunks) != nullptr);
    CHECK(grail::fir_stream_next_error(a, 64, ln, 8, (const void *)((uintptr_t)in_end - 4u), 64, &chunks) != nullptr);
    CHECK(grail::fir_stream_next_error(a, 64, ln, 8, (const void *)((uintptr_t)before + 4u), 64, &chunks) != nullptr);
    CHECK(grail::fir_stream_next_error(a, 64, ln, 8, (const void *)((uintptr_t)a - 4u), 1024, &chunks) != nullptr);
    // spans and chunk counts that do not fit
    CHECK(grail::fir_stream_next_error(a, (uint64_t)1 << 58, ln, 8, (const void *)((uintptr_t)1 << 63), (uint64_t)1 << 58, &chunks) != nullptr);
    CHECK(grail::fir_stream_next_error(a, 0xFFFFFFFFull, ln, 1024, (const void *)((uintptr_t)1 << 50), 0xFFFFFFFFull, &chunks) != nullptr);
    CHECK(grail::fir_stream_next_error(a, 0xFFFFFFFFull, ln, 1023, (const void *)((uintptr_t)1 << 50), 0xFFFFFFFFull, &chunks) == nullptr &&
          chunks == 2097152);
    CHECK(grail::fir_stream_next_error(a, (uint64_t)1 << 40, ln, 1023, (const void *)((uintptr_t)1 << 60), (uint64_t)1 << 40, &chunks) == nullptr &&
          chunks == 2097152);                                                         // (a call feeds a row fewer than 2^32 samples)

    // finish: room for the set's longest K - 1
    CHECK(grail::fir_stream_finish_error(b, 254, 8, 255, &chunks) == nullptr && chunks == 1);
    CHECK(grail::fir_stream_finish_error(b, 253, 8, 255, &chunks) != nullptr && grail::fir_stream_finish_error(nullptr, 254, 8, 255, &chunks) != nullptr);
    CHECK(grail::fir_stream_finish_error(nullptr, 0, 8, 1, &chunks) == nullptr && chunks == 0);
    CHECK(grail::fir_stream_finish_error(b, 4095, 8, 4096, &chunks) == nullptr && chunks == 2);
    CHECK(grail::fir_stream_finish_error(b, 2048, 8, 2049, &chunks) == nullptr && chunks == 1);
    CHECK(grail::fir_stream_finish_error(b, 4095, 0x7FFFFFFFu, 4096, &chunks) != nullptr);
    CHECK(grail::fir_stream_finish_error(b, (uint64_t)1 << 58, 8, 255, &chunks) != nullptr);
    std::printf("sanitize fir stream driver: ok\n");
    return 0;
}
