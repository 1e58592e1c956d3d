// limit_plan.h — what the pure-host side of limit streams (limit_plan.cpp) shares with transform_streams.cpp.  No HIP type: it
// builds with g++ (tests/test_limit_stream_sanitize.py), as fir_plan.h and resample_plan.h do.
#pragma once

#include <cstdint>

namespace grail {

// The delay of a limit stream with a look-ahead of 2^ell samples, ell <= 10: Lambda = 2^ell + 10
uint32_t limit_stream_delay(uint32_t ell);
// E(N) = max(0, N - Lambda): the outputs that are final after N samples
uint64_t limit_stream_known(uint64_t fed, uint32_t ell);
// The samples of a row's ring: 3 * 2^ell + 19 rounded up to a power of two, 32 at ell = 0 and 4096 (16 KB) at ell = 10
uint32_t limit_stream_ring_capacity(uint32_t ell);
// NULL when grail_limit_stream_open takes (n_rows, group, ceiling, ell), else what is wrong with them
const char *limit_stream_open_error(uint32_t n_rows, uint32_t group, float ceiling, uint32_t ell);
// NULL when a call of grail_limit_stream_next_async may be queued, *chunks = the chunks of GRAIL_LIMIT_CHUNK outputs a group
// can have (0: no samples at all), else what is wrong with its arguments (addresses are compared, never looked behind)
const char *limit_stream_next_error(const void *in, uint64_t in_stride, const void *in_len, uint32_t n_rows, uint32_t group,
                                    const void *out, uint64_t out_stride, uint64_t *chunks);
// ... and of grail_limit_stream_finish_async, for a stream whose look-ahead is 2^ell
const char *limit_stream_finish_error(const void *out, uint64_t out_stride, uint32_t n_rows, uint32_t group, uint32_t ell,
                                      uint64_t *chunks);

}  // namespace grail
