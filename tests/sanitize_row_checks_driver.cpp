// Drives the row-pair check (csrc/row_checks.h: the buffers, the 2^60 span, the overlap of the two address ranges, the 32 bits
// of an output length) along the edges of each rule under AddressSanitizer and UBSan (tests/test_row_checks_sanitize.py builds
// and runs it).  Every address is a number nobody may look behind.  grail_limit_async, grail_resample_async and
// grail_fir_async (csrc/transforms.cpp) reach this arithmetic only through the loaded library; here it runs observed.  Then
// the same for where the checks of the calls on streams (csrc/transform_streams.cpp) end alike: a call's chunks and their count.
#include <cstdint>
#include <cstdio>
#include <initializer_list>

#include "../grail-rs_amd/csrc/row_checks.h"

using namespace grail;

#define CHECK(cond)                                                                  \
    do {                                                                             \
        if (!(cond)) {                                                               \
            std::fprintf(stderr, "sanitize row checks driver: %s failed (line %d)\n", #cond, __LINE__); \
            return 1;                                                                \
        }                                                                            \
    } while (0)

static const char *const OVER = "overlaps (why)";
static const OutRule ALWAYS = OutRule::always, STRIDED = OutRule::when_out_stride;

static const void *at(uint64_t address) { return (const void *)(uintptr_t)address; }

// a pair with every buffer there: `in` and `out` by address
static const char *pair(uint64_t in, uint64_t in_stride, uint32_t n_rows, uint64_t out, uint64_t out_stride, OutRule need_out = ALWAYS,
                        OutRule overlap = ALWAYS, uint64_t longest = 0)
{
    return row_pair_error({at(in), in_stride, at(0x30000000), n_rows, at(out), out_stride}, need_out, overlap, OVER, longest);
}

int main()
{
    const uint64_t A = 0x10000000, LEN = 0x30000000, FAR = 1ull << 63, P32 = 1ull << 32, P60 = 1ull << 60;

    // no rows: nothing is checked, whatever else is wrong
    for (OutRule rule : {ALWAYS, STRIDED})
        CHECK(row_pair_error({nullptr, 1ull << 61, nullptr, 0, nullptr, 1ull << 61}, rule, rule, OVER, ~0ull) == nullptr);

    // the buffers: len always; in and out once the rows have samples; out under the second rule only where something is written
    for (OutRule rule : {ALWAYS, STRIDED}) {
        CHECK(row_pair_error({at(A), 64, nullptr, 1, at(FAR), 64}, rule, rule, OVER, 0) == ROWS_NULL);
        CHECK(row_pair_error({nullptr, 0, nullptr, 1, nullptr, 0}, rule, rule, OVER, 0) == ROWS_NULL);
        CHECK(row_pair_error({nullptr, 0, at(LEN), 1, nullptr, 0}, rule, rule, OVER, 0) == nullptr);
        CHECK(row_pair_error({nullptr, 0, at(LEN), 2, nullptr, 64}, rule, rule, OVER, 0) == nullptr);
        CHECK(row_pair_error({nullptr, 1, at(LEN), 1, at(FAR), 1}, rule, rule, OVER, 0) == ROWS_NULL);
        CHECK(row_pair_error({at(A), 1, at(LEN), 1, nullptr, 1}, rule, rule, OVER, 0) == ROWS_NULL);
        CHECK(row_pair_error({at(A), 1, at(LEN), 1, at(FAR), 1}, rule, rule, OVER, 0) == nullptr);
    }
    // out_stride == 0 under both rules: "the lengths and counts only" wants no out and compares none
    CHECK(row_pair_error({at(A), 64, at(LEN), 2, nullptr, 0}, ALWAYS, ALWAYS, OVER, 0) == ROWS_NULL);
    CHECK(row_pair_error({at(A), 64, at(LEN), 2, nullptr, 0}, ALWAYS, STRIDED, OVER, 0) == ROWS_NULL);
    CHECK(row_pair_error({at(A), 64, at(LEN), 2, nullptr, 0}, STRIDED, STRIDED, OVER, 0) == nullptr);
    CHECK(row_pair_error({at(A), 64, at(LEN), 2, nullptr, 0}, STRIDED, ALWAYS, OVER, 0) == nullptr);
    CHECK(pair(A, 64, 2, A + 4, 0, STRIDED, STRIDED) == nullptr && pair(A, 64, 2, FAR, 0, ALWAYS, ALWAYS) == nullptr);
    CHECK(pair(A, 64, 2, A + 4, 1, STRIDED, STRIDED) == OVER);

    // the span: n_rows rows of at most 2^60 / n_rows samples, on either side; every stride below is fine
    CHECK(rows_span_fits(~0ull, 0) && rows_span_fits(P60, 1) && !rows_span_fits(P60 + 1, 1) && rows_span_fits(0, 0xFFFFFFFFu));
    const uint32_t ns[] = {1u, 2u, 0xFFFFFFFFu};
    const uint64_t most[] = {P60, 1ull << 59, 1ull << 28};              // 2^60 / n_rows; (2^28 + 1) * (2^32 - 1) > 2^60
    for (int i = 0; i < 3; ++i) {
        const uint32_t n = ns[i];
        CHECK(most[i] == P60 / n && rows_span_fits(most[i], n) && !rows_span_fits(most[i] + 1, n));
        const uint64_t strides[] = {0, 1, P32 - 1, P32, most[i], most[i] + 1};
        for (uint64_t s_in : strides) {
            for (uint64_t s_out : strides) {
                // (in ends below 2^62 + 4096, out begins at 2^63 and ends below 2^63 + 2^62: apart wherever the spans fit)
                const char *want = s_in == 0 ? nullptr : (s_in > most[i] || s_out > most[i]) ? ROWS_SPAN : nullptr;
                CHECK(pair(4096, s_in, n, FAR, s_out) == want);
                CHECK(pair(4096, s_in, n, FAR, s_out, STRIDED, STRIDED, ~0ull) == (want || s_in == 0 || s_out <= 0xFFFFFFFFull ? want : ROWS_TOO_LONG));
            }
        }
    }
    // ... and it is said before the overlap, the NULL buffer before both
    CHECK(pair(A, P60 + 1, 1, A, P60 + 1) == ROWS_SPAN && pair(A, 64, 0xFFFFFFFFu, A, 1ull << 29) == ROWS_SPAN);
    CHECK(row_pair_error({at(A), P60 + 1, at(LEN), 1, nullptr, P60 + 1}, ALWAYS, ALWAYS, OVER, 0) == ROWS_NULL);

    // the overlap: out abutting in on either side is fine, one sample inside it is not
    const uint64_t in_bytes = 8u * 64u * 4u;
    CHECK(pair(A, 64, 8, A + in_bytes, 64) == nullptr && pair(A, 64, 8, A - in_bytes, 64) == nullptr);
    CHECK(pair(A, 64, 8, A + in_bytes - 4, 64) == OVER && pair(A, 64, 8, A - in_bytes + 4, 64) == OVER);
    CHECK(pair(A, 64, 8, A, 64) == OVER && pair(A, 64, 8, A - 4, 1024) == OVER && pair(A, 1024, 8, A + 4, 64) == OVER);
    CHECK(pair(A, 64, 8, A - 2 * in_bytes, 128) == nullptr && pair(A, 64, 8, A - 2 * in_bytes + 4, 128) == OVER);
    CHECK(pair(A, 64, 8, A + in_bytes, 128) == nullptr && pair(A, 64, 8, A + in_bytes - 4, 128) == OVER);
    CHECK(pair(A, 1, 1, A + 4, 1) == nullptr && pair(A, 1, 1, A - 4, 1) == nullptr && pair(A, 1, 1, A, 1) == OVER);
    // ... with the rows' count and stride at their widest: 2^32 - 1 rows of 2^28, 4 * (2^60 - 2^28) bytes
    const uint64_t wide = 4ull * 0xFFFFFFFFull * (1ull << 28);
    CHECK(pair(4096, 1ull << 28, 0xFFFFFFFFu, 4096 + wide, 1ull << 28) == nullptr);
    CHECK(pair(4096, 1ull << 28, 0xFFFFFFFFu, 4096 + wide - 4, 1ull << 28) == OVER);
    CHECK(pair(4096 + wide, 1ull << 28, 0xFFFFFFFFu, 4096, 1ull << 28) == nullptr);
    CHECK(pair(4096 + wide, 1ull << 28, 0xFFFFFFFFu, 4100, 1ull << 28) == OVER);
    // ... and address sums near 2^64: in = [2^63, 2^63 + 2^62), out behind it ends at 2^64 - 4
    const uint64_t top = FAR + (1ull << 62);
    CHECK(pair(FAR, P60, 1, top, P60 - 1) == nullptr && top + 4 * (P60 - 1) == ~0ull - 3);
    CHECK(pair(FAR, P60, 1, top - 4, P60 - 1) == OVER && pair(top, P60 - 1, 1, FAR, P60) == nullptr && pair(top, P60 - 1, 1, FAR + 4, P60) == OVER);
    CHECK(pair(~0ull - 7, 1, 1, ~0ull - 11, 1) == nullptr && pair(~0ull - 7, 1, 1, ~0ull - 7, 1) == OVER);
    // (a range that would end at or past 2^64 does not exist on any machine; the sum wraps as unsigned sums do, and what is
    // answered is not promised: the call is made for the sanitizers' sake)
    (void)pair(~0ull - 3, 1, 1, A, 1);
    (void)pair(A, 1, 1, FAR + (1ull << 62), P60);

    // the output length: the longest a row can have, cut at out_stride, stays below 2^32; said last
    CHECK(pair(4096, P32, 1, FAR, P32, STRIDED, STRIDED, P32 - 1) == nullptr && pair(4096, P32, 1, FAR, P32 - 1, STRIDED, STRIDED, P32) == nullptr);
    CHECK(pair(4096, P32, 1, FAR, P32, STRIDED, STRIDED, P32) == ROWS_TOO_LONG && pair(4096, 1, 2, FAR, ~0ull >> 5, STRIDED, STRIDED, ~0ull) == ROWS_TOO_LONG);
    CHECK(pair(4096, P32, 1, FAR, P32, STRIDED, STRIDED, 0) == nullptr && pair(4096, 64, 2, FAR, 0, STRIDED, STRIDED, ~0ull) == nullptr);
    CHECK(pair(4096, P32, 1, 4096, P32, STRIDED, STRIDED, P32) == OVER && pair(4096, P32, 1, FAR, P60 + 1, STRIDED, STRIDED, P32) == ROWS_SPAN);

    // ---- the calls on streams
    // the chunks of a row: longest at 0, 1, chunk, chunk + 1, 2^32 - 1, and cut there
    const uint32_t CH = 2048;
    CHECK(stream_chunks(0, CH) == 0 && stream_chunks(1, CH) == 1 && stream_chunks(CH, CH) == 1 && stream_chunks(CH + 1, CH) == 2);
    CHECK(stream_chunks(P32 - 1, CH) == 1u << 21 && stream_chunks(P32, CH) == 1u << 21 && stream_chunks(~0ull, CH) == 1u << 21);
    CHECK(stream_chunks(P32 - 1, 1) == P32 - 1 && stream_chunks(~0ull, 1) == P32 - 1 && stream_chunks(P32 - 1, 0xFFFFFFFFu) == 1);
    // a feeding call: the pair's refusals first, no chunks of strides of 0, else the chunks of the longest output
    const uint64_t longests[] = {1, CH, CH + 1, P32 - 1};
    const uint64_t counts[] = {1, 1, 2, 1u << 21};
    for (int i = 0; i < 4; ++i) {
        uint64_t chunks = 77;
        CHECK(stream_next_error({at(A), longests[i], at(LEN), 3, at(FAR), longests[i]}, longests[i], 3, CH, &chunks) == nullptr);
        CHECK(chunks == counts[i]);
    }
    uint64_t chunks = 77;
    CHECK(stream_next_error({nullptr, 0, at(LEN), 3, nullptr, 0}, 0, 3, CH, &chunks) == nullptr && chunks == 77);
    CHECK(stream_next_error({nullptr, 0, nullptr, 3, nullptr, 0}, 0, 3, CH, &chunks) == ROWS_NULL && chunks == 77);
    CHECK(stream_next_error({at(A), 64, at(LEN), 3, nullptr, 64}, 64, 3, CH, &chunks) == ROWS_NULL);
    CHECK(stream_next_error({at(A), P60, at(LEN), 3, at(FAR), P60}, P32 - 1, 3, CH, &chunks) == ROWS_SPAN);
    CHECK(stream_next_error({at(A), 64, at(LEN), 3, at(A + 4), 64}, 64, 3, CH, &chunks) != nullptr && chunks == 77);
    CHECK(stream_next_error({at(A), 1, at(LEN), 1, at(FAR), P32}, P32, 1, CH, &chunks) == ROWS_TOO_LONG && chunks == 77);
    // ... units x chunks at 2^31 - 1 and at 2^31, by the chunks and by the units
    const uint32_t P31 = 1u << 31;
    CHECK(stream_next_error({at(A), P31 - 1, at(LEN), 1, at(FAR), P31 - 1}, P31 - 1, 1, 1, &chunks) == nullptr && chunks == P31 - 1);
    CHECK(stream_next_error({at(A), P31, at(LEN), 1, at(FAR), P31}, P31, 1, 1, &chunks) == STREAM_CHUNKS && chunks == P31);
    CHECK(stream_next_error({at(A), 1, at(LEN), P31 - 1, at(FAR), 1}, 1, P31 - 1, CH, &chunks) == nullptr && chunks == 1);
    CHECK(stream_next_error({at(A), 1, at(LEN), P31, at(FAR), 1}, 1, P31, CH, &chunks) == STREAM_CHUNKS);
    CHECK(stream_next_error({at(A), CH + 1, at(LEN), P31, at(FAR), CH + 1}, CH + 1, P31 / 2 - 1, CH, &chunks) == nullptr && chunks == 2);
    CHECK(stream_next_error({at(A), CH + 1, at(LEN), P31, at(FAR), CH + 1}, CH + 1, P31 / 2, CH, &chunks) == STREAM_CHUNKS);
    // a finishing call: no tail, nothing looked at; else out, its span, the chunks of the tail
    chunks = 77;
    CHECK(stream_finish_error(nullptr, P60 + 1, 0xFFFFFFFFu, 0, 0xFFFFFFFFu, CH, &chunks) == nullptr && chunks == 77);
    CHECK(stream_finish_error(nullptr, 64, 3, 1, 3, CH, &chunks) == ROWS_NULL && chunks == 77);
    CHECK(stream_finish_error(at(FAR), P60 / 3 + 1, 3, 1, 3, CH, &chunks) == ROWS_SPAN && chunks == 77);
    CHECK(stream_finish_error(at(FAR), P60 / 3, 3, 1, 3, CH, &chunks) == nullptr && chunks == 1);
    CHECK(stream_finish_error(at(FAR), 4096, 3, CH, 3, CH, &chunks) == nullptr && chunks == 1);
    CHECK(stream_finish_error(at(FAR), 4096, 3, CH + 1, 3, CH, &chunks) == nullptr && chunks == 2);
    CHECK(stream_finish_error(at(FAR), P32, 3, P32 - 1, 3, CH, &chunks) == nullptr && chunks == 1u << 21);
    CHECK(stream_finish_error(at(FAR), 64, P31 - 1, 1, P31 - 1, CH, &chunks) == nullptr && chunks == 1);
    CHECK(stream_finish_error(at(FAR), 64, P31, 1, P31, CH, &chunks) == STREAM_CHUNKS);
    CHECK(stream_finish_error(at(FAR), P32, 1, P31 - 1, 1, 1, &chunks) == nullptr && stream_finish_error(at(FAR), P32, 1, P31, 1, 1, &chunks) == STREAM_CHUNKS);
    std::printf("sanitize row checks driver: ok\n");
    return 0;
}
