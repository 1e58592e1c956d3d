// meter_plan.h — what the pure-host side of meter streams (meter_plan.cpp) shares with transform_streams.cpp.  No HIP type: it
// builds with g++ (tests/test_meter_stream_sanitize.py), as limit_plan.h does.
#pragma once

#include <cstddef>
#include <cstdint>

namespace grail {

// H = sample_rate / 10, the samples of a hop; 0 for a rate outside GRAIL_LOUDNESS_RATE_MIN .. _MAX
uint32_t meter_stream_hop(uint32_t sample_rate);
// The hops a row completes when it is fed n samples after fed_before (fed_before + n fits 64 bits, hop > 0)
uint64_t meter_stream_hops(uint64_t fed_before, uint64_t n, uint32_t hop);
// The least hops_stride of a feeding call: (in_stride + H - 1) / H, the most hops a row can complete in it
uint64_t meter_stream_hops_stride(uint64_t in_stride, uint32_t hop);
// NULL when grail_meter_stream_open takes (n_rows, sample_rate, max_hops), else what is wrong with them
const char *meter_stream_open_error(uint32_t n_rows, uint32_t sample_rate, uint64_t max_hops);
// NULL when a call of grail_meter_stream_next_async may be queued, *chunks = the chunks of METER_STREAM_CHUNK output times a
// row can have (0: no samples at all), else what is wrong with its arguments (addresses are compared, never looked behind)
const char *meter_stream_next_error(const void *in, uint64_t in_stride, const void *in_len, uint32_t n_rows, const void *hop_sumsq,
                                    uint64_t hops_stride, uint32_t hop, uint64_t *chunks);

}  // namespace grail
