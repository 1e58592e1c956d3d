// resample_plan.h — what the pure-host side of sample-rate conversion (resample_plan.cpp) shares with transforms.cpp and
// transform_streams.cpp: the ring and the checks of the calls on resample streams (grail_resample_stream_*).  No HIP type: it
// builds with g++ (tests/test_resample_stream_sanitize.py).  The convention is fir_plan.h's: NULL means fine, else what is wrong.
#pragma once

#include <cstdint>

#include "../../include/grail_hip.h"

namespace grail {

// The outputs of one workgroup of the stream kernel: the one-shot kernel's chunk (DESIGN.md §4.16 has the figures that
// decided it).  Not part of the contract: no number depends on it.
constexpr uint32_t RESAMPLE_STREAM_CHUNK = GRAIL_RESAMPLE_CHUNK;

// The samples of a row's ring: taps - 1 rounded up to a power of two (taps is even and at least 48: at least 64, at most
// 32 768, 128 KB).  fir_stream_ring_capacity stops at 4096, the longest FIR filter, so it does not fit as it is.
uint32_t resample_stream_ring_capacity(uint32_t taps);
// the most a call that feeds `n` samples can write, ceil(n U / D), and the most a finishing call can, ceil((taps / 2) U / D)
unsigned __int128 resample_stream_most(uint64_t n, uint32_t U, uint32_t D);
uint64_t resample_stream_tail(uint32_t U, uint32_t D, uint32_t taps);
// NULL when a call of grail_resample_stream_next_async may be queued, *chunks = the chunks of RESAMPLE_STREAM_CHUNK outputs a
// row can have (0: no samples at all), else what is wrong with its arguments (addresses are compared, never looked behind)
const char *resample_stream_next_error(const void *in, uint64_t in_stride, const void *in_len, uint32_t n_rows, const void *out,
                                       uint64_t out_stride, uint32_t U, uint32_t D, uint64_t *chunks);
// ... and of grail_resample_stream_finish_async
const char *resample_stream_finish_error(const void *out, uint64_t out_stride, uint32_t n_rows, uint32_t U, uint32_t D, uint32_t taps,
                                         uint64_t *chunks);

}  // namespace grail
