// iir_plan.h — what the pure-host side of recursive filtering (iir_plan.cpp) shares with transforms.cpp, transform_streams.cpp
// and iir_kernels.hip.  No HIP type: it builds with g++ (tests/test_iir_sanitize.py).
#pragma once

#include <cstdint>
#include <vector>

namespace grail {

// one filter of a set as the kernels read it: IIR_IMAGE_DOUBLES doubles of the set's image, section j at 5 j (b0 b1 b2 a1 a2),
// the sections past the filter's own +0.0 (they are computed by no lane that keeps their result: iir_kernels.hip)
constexpr uint32_t IIR_SECTIONS = 8;        // == GRAIL_IIR_SECTIONS_MAX
constexpr uint32_t IIR_IMAGE_DOUBLES = 5 * IIR_SECTIONS;
// a stream's state words a row for a section bound: N with the end's bit, then s1, s2 of each section
constexpr uint32_t iir_stream_state_words(uint32_t bound) { return 1u + 2u * bound; }

// NULL when (coef, n_sections, n_filters) is a set grail_iir_create takes, else what is wrong with it
const char *iir_set_error(const double *coef, const uint32_t *n_sections, uint32_t n_filters);
// the device image of a checked set: image[IIR_IMAGE_DOUBLES * f ..]: filter f; sections[f]: its S; *bound: the set's
// largest S rounded up to 1, 2, 4 or 8 (the kernel instantiation that serves the set)
void iir_set_image(const double *coef, const uint32_t *n_sections, uint32_t n_filters, std::vector<double> &image,
                   std::vector<uint32_t> &sections, uint32_t *bound);
// n_out of a row of n samples: 0 for n = 0, else min(n + tail, out_stride)
uint64_t iir_len(uint64_t n, uint32_t tail, uint64_t out_stride);

// Streams (grail_iir_stream_*).  NULL when filter (host [n_rows], or NULL = filter 0) binds n_rows >= 1 rows to filters of
// a set of n_filters
const char *iir_stream_open_error(const uint32_t *filter, uint32_t n_rows, uint32_t n_filters);
// NULL when a call of grail_iir_stream_next_async may be queued, else what is wrong with its arguments (addresses are
// compared, never looked behind)
const char *iir_stream_next_error(const void *in, uint64_t in_stride, const void *in_len, uint32_t n_rows, const void *out,
                                  uint64_t out_stride);
// ... and of grail_iir_stream_finish_async, for a stream whose rows ring out over `tail` outputs
const char *iir_stream_finish_error(const void *out, uint64_t out_stride, uint32_t n_rows, uint32_t tail);

}  // namespace grail
