// iir_plan.cpp — the host side of recursive filtering that needs no device: grail_iir_design (one biquad by the bilinear
// transform, the K-weighting's form), grail_iir_stream_len, the checks of a filter set and of the calls on IIR streams (their
// common end: row_checks.h), the image of a set as the kernels read it, the length rule, and of the form parallel in time (grail_biquad_blocked_async,
// §4.22) the block transition matrix (grail_biquad_block_matrix), the grid and the scratch size.  The contract is
// include/grail_hip.h, "levels, continued: recursive filtering".  No HIP call, so it builds with g++ under AddressSanitizer
// and UBSan (tests/test_iir_sanitize.py), as fir_plan.cpp does.  DESIGN.md §4.19, §4.20.
#include <cmath>
#include <cstdint>

#include "../../include/grail_hip.h"
#include "iir_plan.h"
#include "row_checks.h"

// the block matrix below is the recurrence itself: every operation rounded by itself under either compiler, whatever its flags
#if defined(__clang__)
#pragma clang fp contract(off)
#elif defined(__GNUC__)
#pragma GCC optimize("fp-contract=off")
#endif

namespace grail {

static_assert(IIR_SECTIONS == GRAIL_IIR_SECTIONS_MAX, "the image's pitch is the header's bound");
static_assert(IIR_BLOCK == GRAIL_BIQUAD_BLOCK, "the block is the header's");

const char *iir_set_error(const double *coef, const uint32_t *n_sections, uint32_t n_filters)
{
    if (!coef || !n_sections) return "NULL argument";
    if (n_filters < 1 || n_filters > GRAIL_IIR_FILTERS_MAX) return "n_filters is outside 1 .. 64";
    size_t at = 0;
    for (uint32_t f = 0; f < n_filters; ++f) {
        if (n_sections[f] < 1 || n_sections[f] > GRAIL_IIR_SECTIONS_MAX) return "a filter's n_sections is outside 1 .. 8";
        for (uint32_t k = 0; k < 5u * n_sections[f]; ++k)
            if (!std::isfinite(coef[at + k])) return "a coefficient is not finite";
        at += 5u * n_sections[f];
    }
    return nullptr;
}

void iir_set_image(const double *coef, const uint32_t *n_sections, uint32_t n_filters, std::vector<double> &image,
                   std::vector<uint32_t> &sections, uint32_t *bound)
{
    image.assign((size_t)n_filters * IIR_IMAGE_DOUBLES, 0.0);
    sections.assign(n_sections, n_sections + n_filters);
    size_t from = 0;
    uint32_t most = 1;
    for (uint32_t f = 0; f < n_filters; ++f) {
        const uint32_t k = 5u * n_sections[f];
        for (uint32_t i = 0; i < k; ++i) image[(size_t)f * IIR_IMAGE_DOUBLES + i] = coef[from + i];
        from += k;
        most = n_sections[f] > most ? n_sections[f] : most;
    }
    uint32_t b = 1;
    while (b < most) b <<= 1;
    *bound = b;
}

uint64_t iir_len(uint64_t n, uint32_t tail, uint64_t out_stride)
{
    if (n == 0) return 0;
    const uint64_t whole = n > UINT64_MAX - tail ? UINT64_MAX : n + tail;
    return whole < out_stride ? whole : out_stride;
}

void iir_block_matrix(const double *coef, uint32_t n_sections, double *matrix, uint32_t pitch)
{
    for (uint32_t c = 0; c < 2u * n_sections; ++c) {
        double s1[IIR_SECTIONS] = {}, s2[IIR_SECTIONS] = {};
        if (c & 1u)
            s2[c / 2u] = 1.0;
        else
            s1[c / 2u] = 1.0;
        for (uint32_t t = 0; t < IIR_BLOCK; ++t) {
            double v = 0.0;
            for (uint32_t j = 0; j < n_sections; ++j) {
                const double *k = coef + 5u * j;
                const double y = k[0] * v + s1[j];
                s1[j] = (k[1] * v - k[3] * y) + s2[j];
                s2[j] = k[2] * v - k[4] * y;
                v = y;
            }
        }
        for (uint32_t j = 0; j < n_sections; ++j) {
            matrix[(size_t)(2u * j) * pitch + c] = s1[j];
            matrix[(size_t)(2u * j + 1u) * pitch + c] = s2[j];
        }
    }
}

void iir_block_image(const std::vector<double> &image, const std::vector<uint32_t> &sections, std::vector<double> &matrices)
{
    matrices.assign(sections.size() * (size_t)IIR_MATRIX_DOUBLES, 0.0);
    for (size_t f = 0; f < sections.size(); ++f)
        iir_block_matrix(image.data() + f * IIR_IMAGE_DOUBLES, sections[f], matrices.data() + f * IIR_MATRIX_DOUBLES, IIR_MATRIX_STATES);
}

uint64_t iir_block_grid_blocks(uint64_t row_stride, uint32_t tail)
{
    // (a row holds fewer than 2^32 samples: len is 32 bits wide)
    const uint64_t most = (row_stride < 0xFFFFFFFFull ? row_stride : 0xFFFFFFFFull) + tail;
    return most / IIR_BLOCK + (most % IIR_BLOCK != 0u);
}

uint64_t iir_block_groups(uint64_t grid_blocks) { return grid_blocks / IIR_BLOCK_LANES + (grid_blocks % IIR_BLOCK_LANES != 0u); }

uint64_t iir_block_scratch_doubles(uint32_t n_rows, uint64_t grid_blocks, uint32_t bound)
{
    const uint64_t per_block = 2u * bound;
    if (grid_blocks > UINT64_MAX / per_block) return UINT64_MAX;
    const uint64_t a_row = grid_blocks * per_block;
    return n_rows && a_row > UINT64_MAX / n_rows ? UINT64_MAX : a_row * n_rows;
}

const char *iir_stream_open_error(const uint32_t *filter, uint32_t n_rows, uint32_t n_filters)
{
    if (n_rows == 0) return "n_rows is 0";
    if (filter)
        for (uint32_t u = 0; u < n_rows; ++u)
            if (filter[u] >= n_filters) return "a row's filter index is outside the set";
    return nullptr;
}

// (a stream has rows: iir_stream_open_error; a call feeds a row fewer than 2^32 samples: in_len is 32 bits wide)
const char *iir_stream_next_error(const void *in, uint64_t in_stride, const void *in_len, uint32_t n_rows, const void *out,
                                  uint64_t out_stride)
{
    if (out_stride < in_stride) return "out_stride < in_stride (a stream never cuts outputs short)";
    return row_pair_error({in, in_stride, in_len, n_rows, out, out_stride}, OutRule::always, OutRule::always,
                          "out_dev overlaps in_dev (a wave reads ahead of another's stores)", 0);
}

const char *iir_stream_finish_error(const void *out, uint64_t out_stride, uint32_t n_rows, uint32_t tail)
{
    if (out_stride < tail) return "out_stride is below the stream's tail";
    if (tail == 0) return nullptr;
    if (!out) return ROWS_NULL;
    if (!rows_span_fits(out_stride, n_rows)) return ROWS_SPAN;
    return nullptr;
}

}  // namespace grail

extern "C" {

int grail_iir_stream_len(uint64_t fed_before, uint64_t n, uint32_t tail, int finishing, uint64_t *n_out)
{
    if (!n_out || (finishing && n) || fed_before > (1ull << 63) - 1u || n > (1ull << 63) - 1u - fed_before)
        return GRAIL_ERR_INVALID_ARG;
    *n_out = finishing ? (fed_before ? tail : 0u) : n;
    return GRAIL_OK;
}

int grail_biquad_block_matrix(const double *coef, uint32_t n_sections, double *matrix)
{
    if (!coef || !matrix || n_sections < 1 || n_sections > GRAIL_IIR_SECTIONS_MAX) return GRAIL_ERR_INVALID_ARG;
    for (uint32_t k = 0; k < 5u * n_sections; ++k)
        if (!std::isfinite(coef[k])) return GRAIL_ERR_INVALID_ARG;
    grail::iir_block_matrix(coef, n_sections, matrix, 2u * n_sections);
    return GRAIL_OK;
}

int grail_iir_design(int kind, uint32_t sample_rate, double f0_hz, double q, double gain_db, double coef[5])
{
    if (!coef || sample_rate == 0 || kind < GRAIL_IIR_LOWPASS || kind > GRAIL_IIR_HIGHSHELF) return GRAIL_ERR_INVALID_ARG;
    // (written so that a NaN fails)
    if (!(f0_hz > 0.0 && f0_hz < (double)sample_rate / 2.0) || !(q > 0.0 && std::isfinite(q)) || !std::isfinite(gain_db))
        return GRAIL_ERR_INVALID_ARG;
    const double pi = 3.141592653589793;
    const double K = std::tan(pi * f0_hz / (double)sample_rate), KQ = K / q, KK = K * K;
    const double D = (1.0 + KQ) + KK;
    double b0, b1, b2, a1 = 2.0 * (KK - 1.0) / D, a2 = ((1.0 - KQ) + KK) / D;
    switch (kind) {
    case GRAIL_IIR_LOWPASS:
        b0 = KK / D, b1 = 2.0 * KK / D, b2 = KK / D;
        break;
    case GRAIL_IIR_HIGHPASS:
        b0 = 1.0 / D, b1 = -2.0 / D, b2 = 1.0 / D;
        break;
    case GRAIL_IIR_BANDPASS:
        b0 = KQ / D, b1 = 0.0, b2 = -KQ / D;
        break;
    case GRAIL_IIR_NOTCH:
        b0 = (1.0 + KK) / D, b1 = 2.0 * (KK - 1.0) / D, b2 = (1.0 + KK) / D;
        break;
    case GRAIL_IIR_HIGHSHELF: {
        const double V = std::pow(10.0, gain_db / 20.0), W = std::sqrt(V);
        b0 = ((V + W * KQ) + KK) / D, b1 = 2.0 * (KK - V) / D, b2 = ((V - W * KQ) + KK) / D;
        break;
    }
    case GRAIL_IIR_LOWSHELF: {
        const double V = std::pow(10.0, gain_db / 20.0), W = std::sqrt(V);
        b0 = ((1.0 + W * KQ) + V * KK) / D, b1 = 2.0 * (V * KK - 1.0) / D, b2 = ((1.0 - W * KQ) + V * KK) / D;
        break;
    }
    default:        // GRAIL_IIR_PEAK
        if (gain_db >= 0.0) {
            const double V = std::pow(10.0, gain_db / 20.0);
            b0 = ((1.0 + V * KQ) + KK) / D, b1 = 2.0 * (KK - 1.0) / D, b2 = ((1.0 - V * KQ) + KK) / D;
        } else {
            const double V = std::pow(10.0, -gain_db / 20.0), E = (1.0 + V * KQ) + KK;
            b0 = D / E, b1 = 2.0 * (KK - 1.0) / E, b2 = ((1.0 - KQ) + KK) / E;
            a1 = 2.0 * (KK - 1.0) / E, a2 = ((1.0 - V * KQ) + KK) / E;
        }
        break;
    }
    // (f0 next to half the rate, or a huge gain, can overflow: such a section would be refused by grail_iir_create)
    if (!std::isfinite(b0) || !std::isfinite(b1) || !std::isfinite(b2) || !std::isfinite(a1) || !std::isfinite(a2))
        return GRAIL_ERR_INVALID_ARG;
    coef[0] = b0, coef[1] = b1, coef[2] = b2, coef[3] = a1, coef[4] = a2;
    return GRAIL_OK;
}

}  // extern "C"
