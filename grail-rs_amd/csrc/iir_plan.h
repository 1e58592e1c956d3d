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

// The form parallel in time (grail_biquad_blocked_async, biquad_block_kernels.hip).  A row's steps are cut into
// blocks of IIR_BLOCK; IIR_BLOCK_LANES consecutive blocks of one row make a workgroup of one wave.
constexpr uint32_t IIR_BLOCK = 1024;        // == GRAIL_BIQUAD_BLOCK
constexpr uint32_t IIR_BLOCK_LANES = 64;
constexpr uint32_t IIR_MATRIX_STATES = 2 * IIR_SECTIONS;
constexpr uint32_t IIR_MATRIX_DOUBLES = IIR_MATRIX_STATES * IIR_MATRIX_STATES;     // one filter of a set's matrix image
// T of one checked filter of S sections (coef [5 S]): matrix[i * pitch + c] = state i (s1[0] s2[0] s1[1] ...) after IIR_BLOCK
// steps of the recurrence on +0.0 from the state that is 1.0 in place c, for i, c < 2 S; nothing else of matrix is written
void iir_block_matrix(const double *coef, uint32_t n_sections, double *matrix, uint32_t pitch);
// the matrices of a set as the propagate kernel reads them: [n_filters][16][16], +0.0 past a filter's own 2 S
void iir_block_image(const std::vector<double> &image, const std::vector<uint32_t> &sections, std::vector<double> &matrices);
// G: the blocks a row of the call can have, ceil((min(row_stride, 2^32 - 1) + tail) / IIR_BLOCK); the grid's workgroups a row,
// ceil(G / 64); the doubles of scratch, n_rows * G * 2 * bound (UINT64_MAX where that is past 64 bits)
uint64_t iir_block_grid_blocks(uint64_t row_stride, uint32_t tail);
uint64_t iir_block_groups(uint64_t grid_blocks);
uint64_t iir_block_scratch_doubles(uint32_t n_rows, uint64_t grid_blocks, uint32_t bound);

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
