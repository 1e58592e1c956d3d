// fir_plan.h — what the pure-host side of FIR filtering (fir_plan.cpp) shares with levels.cpp, and the two functions it
// shares with the resampler's table (resample_plan.cpp).  No HIP type: it builds with g++ (tests/test_fir_sanitize.py).
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

}  // namespace grail
