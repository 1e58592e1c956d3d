// Drives the pure-host side of meter streams (csrc/meter_plan.cpp: the hop of a rate, grail_meter_stream_hops, the stride rule
// of a call's hop sums, the checks of open and next, the chunk count) under AddressSanitizer and UBSan
// (tests/test_meter_stream_sanitize.py builds and runs it): the counts at the edges of 64 bits, every check either side of its
// threshold; the device addresses are numbers nobody may look behind.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <initializer_list>

#include "../include/grail_hip.h"
#include "../grail-rs_amd/csrc/meter_plan.h"

#define CHECK(cond)                                                                  \
    do {                                                                             \
        if (!(cond)) {                                                               \
            std::fprintf(stderr, "sanitize meter stream driver: %s failed (line %d)\n", #cond, __LINE__); \
            return 1;                                                                \
        }                                                                            \
    } while (0)

static bool says(const char *got, const char *want) { return got && std::strstr(got, want) != nullptr; }

int main()
{
    // the hop of a rate, and the hops of a call: (fed + n) / H - fed / H
    CHECK(grail::meter_stream_hop(GRAIL_LOUDNESS_RATE_MIN - 1u) == 0 && grail::meter_stream_hop(GRAIL_LOUDNESS_RATE_MAX + 1u) == 0);
    CHECK(grail::meter_stream_hop(0) == 0 && grail::meter_stream_hop(UINT32_MAX) == 0);
    for (uint32_t rate : {GRAIL_LOUDNESS_RATE_MIN, 2569u, 8000u, 44100u, 48000u, GRAIL_LOUDNESS_RATE_MAX}) {
        const uint64_t H = rate / 10u;
        CHECK(grail::meter_stream_hop(rate) == H);
        for (uint64_t fed : {(uint64_t)0, (uint64_t)1, H - 1, H, H + 1, (uint64_t)UINT32_MAX, (uint64_t)1 << 32, ((uint64_t)1 << 63) - H,
                             (uint64_t)1 << 63, UINT64_MAX - 5 * H, UINT64_MAX - 1, UINT64_MAX}) {
            for (uint64_t n : {(uint64_t)0, (uint64_t)1, H - 1, H, 5 * H, (uint64_t)UINT32_MAX, UINT64_MAX}) {
                uint64_t got = 77;
                if (fed > UINT64_MAX - n) {
                    CHECK(grail_meter_stream_hops(fed, n, rate, &got) == GRAIL_ERR_INVALID_ARG && got == 77);
                    continue;
                }
                CHECK(grail_meter_stream_hops(fed, n, rate, &got) == GRAIL_OK);
                CHECK(got == (fed + n) / H - fed / H && got <= n / H + 1);
                CHECK(got == grail::meter_stream_hops(fed, n, (uint32_t)H));
            }
        }
        uint64_t got = 77;
        CHECK(grail_meter_stream_hops(0, 1, rate, nullptr) == GRAIL_ERR_INVALID_ARG);
        CHECK(grail_meter_stream_hops(0, 1, 0, &got) == GRAIL_ERR_INVALID_ARG && got == 77);
        // the stride rule: the most hops a row can complete in a call, from the last place inside a hop
        for (uint64_t stride : {(uint64_t)0, (uint64_t)1, H - 1, H, H + 1, 7 * H, (uint64_t)UINT32_MAX, (uint64_t)1 << 60, UINT64_MAX}) {
            const uint64_t want = stride / H + (stride % H ? 1 : 0);
            CHECK(grail::meter_stream_hops_stride(stride, (uint32_t)H) == want);
            if (stride && stride <= UINT32_MAX) CHECK(grail::meter_stream_hops(H - 1, stride, (uint32_t)H) == want);
        }
    }

    // open: the numbers, in the order they are said
    CHECK(says(grail::meter_stream_open_error(1, 2559, 10), "sample_rate"));
    CHECK(says(grail::meter_stream_open_error(0, 2559, 0), "sample_rate"));
    CHECK(says(grail::meter_stream_open_error(0, 48000, 0), "n_rows is 0"));
    CHECK(says(grail::meter_stream_open_error(1, 48000, 0), "max_hops is 0"));
    CHECK(says(grail::meter_stream_open_error(1, 48000, SIZE_MAX / 8u + 1u), "do not fit"));
    CHECK(grail::meter_stream_open_error(1, 48000, SIZE_MAX / 8u) == nullptr);
    CHECK(says(grail::meter_stream_open_error(UINT32_MAX, 48000, (SIZE_MAX / 8u) / UINT32_MAX + 1u), "do not fit"));
    CHECK(grail::meter_stream_open_error(UINT32_MAX, 48000, (SIZE_MAX / 8u) / UINT32_MAX) == nullptr);
    CHECK(says(grail::meter_stream_open_error(2, 48000, UINT64_MAX), "do not fit"));
    CHECK(grail::meter_stream_open_error(4096, 48000, 36000) == nullptr);

    // next: addresses are compared with NULL and never looked behind
    const void *in = (const void *)((uintptr_t)1 << 48), *len = (const void *)(uintptr_t)0x30000000, *out = (const void *)((uintptr_t)1 << 50);
    uint64_t chunks = 77;
    CHECK(says(grail::meter_stream_next_error(in, 64, nullptr, 1, nullptr, 0, 256, &chunks), "NULL buffer") && chunks == 0);
    CHECK(says(grail::meter_stream_next_error(nullptr, 64, len, 1, nullptr, 0, 256, &chunks), "NULL buffer"));
    CHECK(grail::meter_stream_next_error(nullptr, 0, len, 1, nullptr, 0, 256, &chunks) == nullptr && chunks == 0);
    CHECK(grail::meter_stream_next_error(in, 0, len, 1, out, 0, 256, &chunks) == nullptr && chunks == 0);
    CHECK(says(grail::meter_stream_next_error(in, ((uint64_t)1 << 60) + 1, len, 1, nullptr, 0, 256, &chunks), "2^60"));
    CHECK(says(grail::meter_stream_next_error(in, ((uint64_t)1 << 59) + 1, len, 2, nullptr, 0, 256, &chunks), "2^60"));
    CHECK(says(grail::meter_stream_next_error(in, UINT64_MAX, len, 1, nullptr, 0, 256, &chunks), "2^60"));
    CHECK(says(grail::meter_stream_next_error(in, 256, len, 1, out, 0, 256, &chunks), "hops_stride"));
    CHECK(says(grail::meter_stream_next_error(in, 257, len, 1, out, 1, 256, &chunks), "hops_stride"));
    CHECK(grail::meter_stream_next_error(in, 257, len, 1, out, 2, 256, &chunks) == nullptr && chunks == 1);
    CHECK(grail::meter_stream_next_error(in, 257, len, 1, nullptr, 0, 256, &chunks) == nullptr && chunks == 1);
    CHECK(says(grail::meter_stream_next_error(in, 64, len, 2, out, ((uint64_t)1 << 59) + 1, 256, &chunks), "2^60"));
    CHECK(grail::meter_stream_next_error(in, 4096, len, 3, out, 16, 256, &chunks) == nullptr && chunks == 1);
    CHECK(grail::meter_stream_next_error(in, 4097, len, 3, out, 17, 256, &chunks) == nullptr && chunks == 2);
    // a row is fed fewer than 2^32 samples a call: at most 2^20 chunks a row; 2^31 chunks in all are too many
    CHECK(grail::meter_stream_next_error(in, (uint64_t)1 << 40, len, 2047, nullptr, 0, 256, &chunks) == nullptr && chunks == (uint64_t)1 << 20);
    CHECK(says(grail::meter_stream_next_error(in, (uint64_t)1 << 40, len, 2048, nullptr, 0, 256, &chunks), "2^31 chunks"));
    CHECK(grail::meter_stream_next_error(in, 4096, len, 0x7FFFFFFFu, nullptr, 0, 256, &chunks) == nullptr && chunks == 1);
    CHECK(says(grail::meter_stream_next_error(in, 4097, len, 0x7FFFFFFFu, nullptr, 0, 256, &chunks), "2^31 chunks"));

    std::printf("sanitize meter stream driver: ok\n");
    return 0;
}
