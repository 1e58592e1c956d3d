// fir_plan.h — what the pure-host side of FIR filtering (fir_plan.cpp) shares with transforms.cpp and transform_streams.cpp,
// and the two functions it shares with the resampler's table (resample_plan.cpp).  No HIP type: it builds with g++
// (tests/test_fir_sanitize.py).
#pragma once

#include <cstdint>
#include <vector>

namespace grail {

// resample_plan.cpp: I0 by its power series; sin(pi a) / (pi a), 1 at 0
double bessel_i0(double y);
double sinc_pi(double a);

// one filter of a set as the kernels read it: FIR_DESC_WORDS words of the set's descriptor array
constexpr uint32_t FIR_DESC_WORDS = 4;      // {first tap in the image, padded taps (a multiple of 8), taps, origin}

// NULL when (taps, n_taps, origin, n_filters) is a set grail_fir_create takes, else what is wrong with it
const char *fir_set_error(const float *taps, const uint32_t *n_taps, const uint32_t *origin, uint32_t n_filters);
// the device image of a checked set: every filter's taps as binary64, padded with +0.0 to a multiple of 8, one after
// another; desc[FIR_DESC_WORDS * f ..]: filter f; *tail_max = the largest n_taps - 1 - origin (how far a row rings out)
void fir_set_image(const float *taps, const uint32_t *n_taps, const uint32_t *origin, uint32_t n_filters,
                   std::vector<double> &image, std::vector<uint32_t> &desc, uint32_t *tail_max);

// Streams (grail_filter_stream_*).  The samples of a row's ring: the set's longest n_taps - 1 rounded up to a power of two,
// at least 1 and at most 4096 (16 KB)
uint32_t fir_stream_ring_capacity(uint32_t longest_taps);
// NULL when filter (host [n_rows], or NULL = filter 0) binds n_rows >= 1 rows to filters of a set of n_filters
const char *fir_stream_open_error(const uint32_t *filter, uint32_t n_rows, uint32_t n_filters);
// NULL when a call of grail_filter_stream_next_async may be queued, *chunks = the chunks of GRAIL_FIR_CHUNK outputs a row
// can have (0: no samples at all), else what is wrong with its arguments (addresses are compared, never looked behind)
const char *fir_stream_next_error(const void *in, uint64_t in_stride, const void *in_len, uint32_t n_rows, const void *out,
                                  uint64_t out_stride, uint64_t *chunks);
// ... and of grail_filter_stream_finish_async, for a set whose longest filter has longest_taps taps
const char *fir_stream_finish_error(const void *out, uint64_t out_stride, uint32_t n_rows, uint32_t longest_taps, uint64_t *chunks);

}  // namespace grail
