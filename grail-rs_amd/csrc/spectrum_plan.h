// spectrum_plan.h — what the pure-host side of short-time spectra (spectrum_plan.cpp) shares with transforms.cpp and
// spectrum_kernels.hip: a set's facts, its checks and image, the checks and the grid of grail_spectrum_async.  No HIP type: it
// builds with g++ (tests/test_spectrum_sanitize.py).
#pragma once

#include <cstdint>
#include <vector>

namespace grail {

constexpr uint32_t SPECTRUM_LOG2_MIN = 6, SPECTRUM_LOG2_MAX = 12;      // == GRAIL_SPECTRUM_LOG2_MIN / _MAX
constexpr uint32_t SPECTRUM_CHUNK_FRAMES = 8;  // == GRAIL_SPECTRUM_CHUNK_FRAMES (not part of the contract: no number depends on it)
// one band of a set as the kernels read it: SPECTRUM_BAND_WORDS words of the set's descriptor array
constexpr uint32_t SPECTRUM_BAND_WORDS = 4;    // {first bin, count, first weight in the weights' array, 0}

// what a call reads of its set on the host
struct SpectrumFacts {
    uint32_t log2n = 0;     // p: N = 2^p
    uint32_t n_window = 0;  // W
    uint32_t hop = 0;       // H
    uint32_t pad = 0;
    uint32_t n_bands = 0;   // B
};

// NULL when the arguments are a set grail_spectrum_create takes, else what is wrong with them
const char *spectrum_set_error(uint32_t log2n, const float *window, uint32_t n_window, uint32_t hop, uint32_t pad, uint32_t n_bands,
                               const uint32_t *band_first, const uint32_t *band_count, const float *band_weights);
// the device image of a checked set: twiddles: T as N/2 pairs (re, im); desc[SPECTRUM_BAND_WORDS * b ..]: band b; weights: the
// bands' weights one after another (one +0.0f, never read, where there are none: no buffer of no bytes)
void spectrum_set_image(uint32_t log2n, uint32_t n_bands, const uint32_t *band_first, const uint32_t *band_count,
                        const float *band_weights, std::vector<double> &twiddles, std::vector<uint32_t> &desc,
                        std::vector<float> &weights);

// the frames a row of this stride can have (a row holds fewer than 2^32 samples: len is 32 bits wide), and the workgroups a
// row: chunks of SPECTRUM_CHUNK_FRAMES frames
uint64_t spectrum_frames_max(uint64_t row_stride, uint32_t hop);
uint64_t spectrum_grid_chunks(uint64_t row_stride, uint32_t hop);
// NULL when a call of grail_spectrum_async may be queued, else what is wrong with its arguments (addresses are compared,
// never looked behind).  set NULL: the call has no context and could not look its set up; what needs the set's facts is
// then not checked (the call ends at the device).
const char *spectrum_call_error(const SpectrumFacts *set, const void *rows, uint64_t row_stride, const void *len, uint32_t n_rows,
                                const void *power, const void *bands, uint64_t frames_stride);

}  // namespace grail
