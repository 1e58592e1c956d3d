// fir_plan.cpp — the host side of FIR filtering that needs no device: grail_fir_len, grail_filter_stream_len and the checks of
// the calls on filter streams (tests/test_fir_stream_sanitize.py; where they end as every stream's do: row_checks.h),
// grail_fir_design (a Kaiser-windowed
// band-pass with the resampler's sinc and I0), the checks of a filter set and the padded image of one as the kernels read
// it.  The contract is include/grail_hip.h, "levels, continued: FIR filtering".  No HIP call, so it builds with g++ under
// AddressSanitizer and UBSan (tests/test_fir_sanitize.py), as resample_plan.cpp does.  DESIGN.md §4.14.
#include <cmath>
#include <cstdint>

#include "../../include/grail_hip.h"
#include "fir_plan.h"
#include "row_checks.h"

namespace {

constexpr double FIR_BETA = 8.0;

bool filter_ok(uint32_t n_taps, uint32_t origin) { return n_taps >= 1 && n_taps <= GRAIL_FIR_TAPS_MAX && origin <= n_taps - 1; }

}  // namespace

namespace grail {

const char *fir_set_error(const float *taps, const uint32_t *n_taps, const uint32_t *origin, uint32_t n_filters)
{
    if (!taps || !n_taps || !origin) return "NULL argument";
    if (n_filters < 1 || n_filters > GRAIL_FIR_FILTERS_MAX) return "n_filters is outside 1 .. 64";
    size_t at = 0;
    for (uint32_t f = 0; f < n_filters; ++f) {
        if (!filter_ok(n_taps[f], origin[f])) return "a filter's n_taps is outside 1 .. 4096 or its origin above n_taps - 1";
        for (uint32_t k = 0; k < n_taps[f]; ++k)
            if (!std::isfinite(taps[at + k])) return "a tap is not finite";
        at += n_taps[f];
    }
    return nullptr;
}

void fir_set_image(const float *taps, const uint32_t *n_taps, const uint32_t *origin, uint32_t n_filters,
                   std::vector<double> &image, std::vector<uint32_t> &desc, uint32_t *tail_max)
{
    size_t padded_total = 0;
    for (uint32_t f = 0; f < n_filters; ++f) padded_total += (n_taps[f] + 7u) & ~7u;
    // The padding is +0.0, and a tap of +0.0 changes no bit of the fold: acc is never -0.0 (it starts at +0.0;
    // +0.0 + -0.0 = +0.0 and x + (-x) = +0.0 in round-to-nearest, so no step can make it -0.0), a padded product is
    // +0.0 or -0.0 (the samples it meets are finite: non-finite ones were zeroed), and acc + (+-0.0) = acc for every
    // acc but -0.0.  tests/test_fir_host.py holds the argument against the model.
    image.assign(padded_total, 0.0);
    desc.assign((size_t)n_filters * FIR_DESC_WORDS, 0u);
    size_t from = 0, to = 0;
    uint32_t tail = 0;
    for (uint32_t f = 0; f < n_filters; ++f) {
        const uint32_t K = n_taps[f], padded = (K + 7u) & ~7u;
        for (uint32_t k = 0; k < K; ++k) image[to + k] = (double)taps[from + k];
        uint32_t *d = &desc[(size_t)f * FIR_DESC_WORDS];
        d[0] = (uint32_t)to, d[1] = padded, d[2] = K, d[3] = origin[f];       // (to <= 64 * 4096)
        tail = K - 1u - origin[f] > tail ? K - 1u - origin[f] : tail;
        from += K;
        to += padded;
    }
    *tail_max = tail;
}

uint32_t fir_stream_ring_capacity(uint32_t longest_taps)
{
    uint32_t cap = 1;
    while (cap < longest_taps - 1u && cap < GRAIL_FIR_TAPS_MAX) cap <<= 1;     // (longest_taps >= 1)
    return cap;
}

const char *fir_stream_open_error(const uint32_t *filter, uint32_t n_rows, uint32_t n_filters)
{
    if (n_rows == 0) return "n_rows is 0";
    if (filter)
        for (uint32_t u = 0; u < n_rows; ++u)
            if (filter[u] >= n_filters) return "a row's filter index is outside the set";
    return nullptr;
}

// (a stream has rows: fir_stream_open_error; a call feeds a row fewer than 2^32 samples: in_len is 32 bits wide)
const char *fir_stream_next_error(const void *in, uint64_t in_stride, const void *in_len, uint32_t n_rows, const void *out,
                                  uint64_t out_stride, uint64_t *chunks)
{
    *chunks = 0;
    if (out_stride < in_stride) return "out_stride < in_stride (a stream never cuts outputs short)";
    const uint64_t longest = in_stride < 0xFFFFFFFFull ? in_stride : 0xFFFFFFFFull;
    return stream_next_error({in, in_stride, in_len, n_rows, out, out_stride}, longest, n_rows, GRAIL_FIR_CHUNK, chunks);
}

const char *fir_stream_finish_error(const void *out, uint64_t out_stride, uint32_t n_rows, uint32_t longest_taps, uint64_t *chunks)
{
    *chunks = 0;
    const uint32_t tail = longest_taps - 1u;
    if (out_stride < tail) return "out_stride is below the set's longest n_taps - 1";
    return stream_finish_error(out, out_stride, n_rows, tail, n_rows, GRAIL_FIR_CHUNK, chunks);
}

}  // namespace grail

extern "C" {

int grail_fir_len(uint64_t n, uint32_t n_taps, uint32_t origin, uint64_t *n_out)
{
    if (!n_out || !filter_ok(n_taps, origin)) return GRAIL_ERR_INVALID_ARG;
    const uint64_t tail = n_taps - 1u - origin;
    if (n > UINT64_MAX - tail) return GRAIL_ERR_INVALID_ARG;
    *n_out = n == 0 ? 0 : n + tail;
    return GRAIL_OK;
}

int grail_filter_stream_len(uint64_t fed_before, uint64_t n, uint32_t n_taps, uint32_t origin, int finishing, uint64_t *n_out)
{
    if (!n_out || !filter_ok(n_taps, origin)) return GRAIL_ERR_INVALID_ARG;
    const uint64_t tail = n_taps - 1u - origin;
    if ((finishing && n) || fed_before > UINT64_MAX - n || fed_before + n > UINT64_MAX - tail) return GRAIL_ERR_INVALID_ARG;
    const uint64_t known = fed_before > origin ? fed_before - origin : 0;       // E(N) = max(0, N - o)
    if (finishing) {
        *n_out = fed_before == 0 ? 0 : fed_before + tail - known;
    } else {
        const uint64_t to = fed_before + n;
        *n_out = (to > origin ? to - origin : 0) - known;
    }
    return GRAIL_OK;
}

int grail_fir_design(uint32_t sample_rate, double lo_hz, double hi_hz, uint32_t n_taps, float *taps)
{
    if (!taps || sample_rate == 0 || n_taps < 3 || n_taps > GRAIL_FIR_TAPS_MAX || n_taps % 2 == 0) return GRAIL_ERR_INVALID_ARG;
    // (written so that a NaN fails)
    if (!(lo_hz >= 0.0 && lo_hz < hi_hz && hi_hz <= (double)sample_rate / 2.0)) return GRAIL_ERR_INVALID_ARG;
    const double c = (double)((n_taps - 1u) / 2u), W = c + 1.0, i0_beta = grail::bessel_i0(FIR_BETA);
    const double f_l = lo_hz / (double)sample_rate, f_h = hi_hz / (double)sample_rate;
    for (uint32_t k = 0; k < n_taps; ++k) {
        const double x = (double)k - c;
        const double r = x / W;
        const double window = grail::bessel_i0(FIR_BETA * std::sqrt(1.0 - r * r)) / i0_beta;
        const double band = 2.0 * f_h * grail::sinc_pi(2.0 * f_h * x) - 2.0 * f_l * grail::sinc_pi(2.0 * f_l * x);
        taps[k] = (float)(window * band);
    }
    return GRAIL_OK;
}

}  // extern "C"
