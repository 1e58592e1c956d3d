// row_checks.h — what the calls that read rows and write rows (transforms.cpp; for transform_streams.cpp the stream checks of
// fir_plan.cpp, resample_plan.cpp and limit_plan.cpp) check of the pair alike, written once: the buffers are there, neither
// side spans more than 2^60 samples, the two do not overlap, and no row's output length outgrows 32 bits.  Below that, where
// the checks of the three kinds of stream end alike: the chunks of a call and their count.  Pure host code, no HIP type: it
// builds with g++, and tests/test_row_checks_sanitize.py walks its edges under AddressSanitizer and UBSan.  The convention is
// fir_plan.h's: NULL means fine, else what is wrong, and the entry point puts its own name in front.
#pragma once

#include <cstdint>

namespace grail {

// n_rows rows of `in_stride` samples read at `in` (their lengths at `len`), n_rows rows of `out_stride` written at `out`.
// Addresses are compared, never looked behind.
struct RowPair {
    const void *in;
    uint64_t in_stride;
    const void *len;
    uint32_t n_rows;
    const void *out;
    uint64_t out_stride;
};

// Where the calls differ on purpose.  The limiter and a stream call always write (their out_stride is at least the input's);
// the resampler and the FIR call take out_stride == 0 as "the lengths and counts only", and then want no `out` and compare none.
enum class OutRule { always, when_out_stride };

constexpr const char *ROWS_NULL = "NULL buffer";
constexpr const char *ROWS_SPAN = "the rows span more than 2^60 samples";
constexpr const char *ROWS_TOO_LONG = "a row could hold 2^32 output samples or more (out_len is 32 bits wide)";

// n_rows rows at this stride stay within 2^60 samples (so their bytes, and the products below, within 2^62)
inline bool rows_span_fits(uint64_t stride, uint32_t n_rows) { return n_rows == 0 || stride <= (1ull << 60) / n_rows; }

// [in, in + n_rows * in_stride) and [out, out + n_rows * out_stride) in float32 share a byte (both spans fit)
inline bool rows_overlap(const RowPair &p)
{
    const uintptr_t in0 = (uintptr_t)p.in, in1 = in0 + (uintptr_t)(p.n_rows * p.in_stride * 4u);
    const uintptr_t out0 = (uintptr_t)p.out, out1 = out0 + (uintptr_t)(p.n_rows * p.out_stride * 4u);
    return in0 < out1 && out0 < in1;
}

// The checks in the order every call says them.  No rows: nothing to check.  Rows of no samples: only `len` is needed.
// need_out: `out` must be there; overlap: the two are compared, and `overlap_message` is what the call says then (its
// parenthesis names what would go wrong).  longest_out: the most output samples a row can have (0: no longer than its input,
// which holds fewer than 2^32); the output is cut at out_stride.
inline const char *row_pair_error(const RowPair &p, OutRule need_out, OutRule overlap, const char *overlap_message, uint64_t longest_out)
{
    if (p.n_rows == 0) return nullptr;
    const bool writes = p.out_stride != 0;
    if (!p.len || (p.in_stride && (!p.in || ((need_out == OutRule::always || writes) && !p.out)))) return ROWS_NULL;
    if (p.in_stride == 0) return nullptr;
    if (!rows_span_fits(p.in_stride, p.n_rows) || !rows_span_fits(p.out_stride, p.n_rows)) return ROWS_SPAN;
    if ((overlap == OutRule::always || writes) && rows_overlap(p)) return overlap_message;
    if ((longest_out < p.out_stride ? longest_out : p.out_stride) > 0xFFFFFFFFull) return ROWS_TOO_LONG;
    return nullptr;
}

// ---- calls on streams: each kind says its own first check (its out_stride against what the call may write), then one of these

constexpr const char *STREAM_CHUNKS = "more than 2^31 chunks";

// the chunks of `chunk` outputs of a row of at most `longest` of them (fewer than 2^32: the lengths are 32 bits wide)
inline uint64_t stream_chunks(uint64_t longest, uint32_t chunk)
{
    const uint64_t most = longest < 0xFFFFFFFFull ? longest : 0xFFFFFFFFull;
    return (most + chunk - 1u) / chunk;
}

// A feeding call: the pair (a stream has rows, and always writes), whose rows give at most `longest` outputs, then the chunks
// of the call's grid, `units` (rows, or groups of rows) times *chunks of them.  Strides of 0 feed nothing: no chunks.
inline const char *stream_next_error(const RowPair &p, uint64_t longest, uint32_t units, uint32_t chunk, uint64_t *chunks)
{
    if (const char *why = row_pair_error(p, OutRule::always, OutRule::always,
                                         "out_dev overlaps in_dev (a chunk reads what another would have written)", longest))
        return why;
    if (p.in_stride == 0) return nullptr;
    *chunks = stream_chunks(longest, chunk);
    return (uint64_t)units * *chunks > 0x7FFFFFFFull ? STREAM_CHUNKS : nullptr;
}

// A finishing call, which writes up to `tail` outputs a row (the caller has held out_stride against it).  No tail (a filter
// stream whose filters have one tap each): nothing is written, and `out` is not looked at.
inline const char *stream_finish_error(const void *out, uint64_t out_stride, uint32_t n_rows, uint64_t tail, uint32_t units,
                                       uint32_t chunk, uint64_t *chunks)
{
    if (tail == 0) return nullptr;
    if (!out) return ROWS_NULL;
    if (!rows_span_fits(out_stride, n_rows)) return ROWS_SPAN;
    *chunks = stream_chunks(tail, chunk);
    return (uint64_t)units * *chunks > 0x7FFFFFFFull ? STREAM_CHUNKS : nullptr;
}

}  // namespace grail
