// spectrum_plan.cpp — the host side of short-time spectra that needs no device: grail_spectrum_twiddles (the table the
// transform reads), grail_spectrum_frames, grail_spectrum_window (periodic Hann and Hamming, a rectangle), grail_mel_design (HTK
// mel triangles), the checks of a set and its image as the kernels read it, the checks and the grid of grail_spectrum_async.
// The contract is include/grail_spectrum.h, "levels, continued: short-time spectra".  No HIP call, so it builds with g++ under
// AddressSanitizer and UBSan (tests/test_spectrum_sanitize.py), as dyn_plan.cpp does.  DESIGN.md §4.25.
#include <cmath>
#include <cstdint>
#include <cstring>

#include "../../include/grail_hip.h"
#include "row_checks.h"
#include "spectrum_plan.h"

// the designers' arithmetic is the contract's: every operation rounded by itself under either compiler, whatever its flags
#if defined(__clang__)
#pragma clang fp contract(off)
#elif defined(__GNUC__)
#pragma GCC optimize("fp-contract=off")
#endif

namespace grail {

static_assert(SPECTRUM_LOG2_MIN == GRAIL_SPECTRUM_LOG2_MIN && SPECTRUM_LOG2_MAX == GRAIL_SPECTRUM_LOG2_MAX, "the sizes are the header's");
static_assert(SPECTRUM_CHUNK_FRAMES == GRAIL_SPECTRUM_CHUNK_FRAMES, "the chunk is the header's");

namespace {

constexpr double TWO_PI = 2.0 * 3.14159265358979323846;     // (exact: a power of two times the binary64 nearest to pi)

bool log2n_ok(uint32_t log2n) { return log2n >= SPECTRUM_LOG2_MIN && log2n <= SPECTRUM_LOG2_MAX; }

// T of the header's TWIDDLES: a quarter from the C library, the rest by sign and mirror
void twiddles(uint32_t log2n, double *re_im)
{
    const uint32_t N = 1u << log2n, Q = N / 4u;
    for (uint32_t j = 0; j <= Q; ++j) {
        double c, s;
        if (j == 0) {
            c = 1.0, s = 0.0;
        } else if (j == Q) {
            c = 0.0, s = 1.0;
        } else {
            const double x = (TWO_PI * (double)j) / (double)N;
            c = std::cos(x), s = std::sin(x);
        }
        re_im[2u * j] = c, re_im[2u * j + 1u] = 0.0 - s;
        if (j >= 1 && j < Q) re_im[2u * (N / 2u - j)] = 0.0 - c, re_im[2u * (N / 2u - j) + 1u] = 0.0 - s;
    }
}

double mel_of(double f) { return 2595.0 * std::log10(1.0 + f / 700.0); }
double hz_of(double m) { return 700.0 * (std::pow(10.0, m / 2595.0) - 1.0); }

// the weight of the triangle (l, c, r) at f, as the header's MEL rounds it
float mel_weight(double f, double l, double c, double r)
{
    const double up = (f - l) / (c - l), down = (r - f) / (r - c);
    const double least = up < down ? up : down;
    return (float)(least > 0.0 ? least : 0.0);
}

// a numbers of `each` words each stay within 2^60 words
bool span_fits(uint64_t a, uint64_t each) { return a == 0 || each <= (1ull << 60) / a; }

// [a, a + a_words) and [b, b + b_words) in 4-byte words share a byte (both spans fit 2^60 words)
bool words_overlap(const void *a, uint64_t a_words, const void *b, uint64_t b_words)
{
    const uintptr_t a0 = (uintptr_t)a, a1 = a0 + (uintptr_t)(a_words * 4u);
    const uintptr_t b0 = (uintptr_t)b, b1 = b0 + (uintptr_t)(b_words * 4u);
    return a0 < b1 && b0 < a1;
}

}  // namespace

const char *spectrum_set_error(uint32_t log2n, const float *window, uint32_t n_window, uint32_t hop, uint32_t pad, uint32_t n_bands,
                               const uint32_t *band_first, const uint32_t *band_count, const float *band_weights)
{
    if (!window) return "NULL argument";
    if (!log2n_ok(log2n)) return "log2n is outside 6 .. 12";
    const uint32_t N = 1u << log2n;
    if (n_window < 1 || n_window > N) return "n_window is outside 1 .. N";
    if (hop == 0) return "hop is 0";
    if (pad >= n_window) return "pad is not below n_window";
    if (n_bands > GRAIL_SPECTRUM_BANDS_MAX) return "n_bands is above 256";
    for (uint32_t j = 0; j < n_window; ++j)
        if (!std::isfinite(window[j])) return "a window number is not finite";
    if (n_bands == 0) return nullptr;
    if (!band_first || !band_count) return "bands without band_first or band_count";
    uint64_t total = 0;
    for (uint32_t b = 0; b < n_bands; ++b) {
        if ((uint64_t)band_first[b] + band_count[b] > N / 2u + 1u) return "a band leaves the bins 0 .. N/2";
        total += band_count[b];
    }
    if (total > GRAIL_SPECTRUM_WEIGHTS_MAX) return "the bands hold more than 65 536 weights";
    if (total && !band_weights) return "weights without band_weights";
    for (uint64_t k = 0; k < total; ++k)
        if (!std::isfinite(band_weights[k])) return "a weight is not finite";
    return nullptr;
}

void spectrum_set_image(uint32_t log2n, uint32_t n_bands, const uint32_t *band_first, const uint32_t *band_count,
                        const float *band_weights, std::vector<double> &tw, std::vector<uint32_t> &desc, std::vector<float> &weights)
{
    tw.assign((size_t)1u << log2n, 0.0);        // (N/2 pairs)
    twiddles(log2n, tw.data());
    desc.assign((size_t)(n_bands ? n_bands : 1u) * SPECTRUM_BAND_WORDS, 0u);
    uint32_t at = 0;
    for (uint32_t b = 0; b < n_bands; ++b) {
        uint32_t *d = &desc[(size_t)b * SPECTRUM_BAND_WORDS];
        d[0] = band_first[b], d[1] = band_count[b], d[2] = at;       // (at <= 65 536)
        at += band_count[b];
    }
    weights.assign(at ? at : 1u, 0.0f);
    if (at) std::memcpy(weights.data(), band_weights, (size_t)at * sizeof(float));
}

uint64_t spectrum_frames_max(uint64_t row_stride, uint32_t hop)
{
    const uint64_t most = row_stride < 0xFFFFFFFFull ? row_stride : 0xFFFFFFFFull;
    return (most + hop - 1u) / hop;             // (hop >= 1: the set's check)
}

uint64_t spectrum_grid_chunks(uint64_t row_stride, uint32_t hop)
{
    return (spectrum_frames_max(row_stride, hop) + SPECTRUM_CHUNK_FRAMES - 1u) / SPECTRUM_CHUNK_FRAMES;
}

const char *spectrum_call_error(const SpectrumFacts *set, const void *rows, uint64_t row_stride, const void *len, uint32_t n_rows,
                                const void *power, const void *bands, uint64_t frames_stride)
{
    if (!power && !bands) return "power_dev and bands_dev are both NULL";
    if (set && bands && set->n_bands == 0) return "bands_dev with a set of no bands";
    // (ceil(row_stride / H) without the sum that could wrap)
    if (set && frames_stride < row_stride / set->hop + (row_stride % set->hop ? 1u : 0u)) return "frames_stride < ceil(row_stride / hop)";
    if (n_rows == 0) return nullptr;
    if (!len || (row_stride && !rows)) return ROWS_NULL;
    if (row_stride == 0) return nullptr;
    if (!rows_span_fits(row_stride, n_rows)) return ROWS_SPAN;
    if (!set) return nullptr;
    const uint64_t bins = ((uint64_t)1u << set->log2n) / 2u + 1u;
    // the numbers of one output: n_rows * frames_stride frames of `each` numbers
    if (!span_fits(n_rows, frames_stride)) return "the outputs span more than 2^60 numbers";
    const uint64_t frames = (uint64_t)n_rows * frames_stride;
    if ((power && !span_fits(frames, bins)) || (bands && !span_fits(frames, set->n_bands))) return "the outputs span more than 2^60 numbers";
    if (power && words_overlap(rows, (uint64_t)n_rows * row_stride, power, frames * bins)) return "power_dev overlaps rows_dev";
    if (bands && words_overlap(rows, (uint64_t)n_rows * row_stride, bands, frames * set->n_bands)) return "bands_dev overlaps rows_dev";
    if ((uint64_t)n_rows * spectrum_grid_chunks(row_stride, set->hop) > 0x7FFFFFFFull) return "more than 2^31 - 1 workgroups";
    return nullptr;
}

}  // namespace grail

extern "C" {

int grail_spectrum_twiddles(uint32_t log2n, double *re_im)
{
    if (!re_im || !grail::log2n_ok(log2n)) return GRAIL_ERR_INVALID_ARG;
    grail::twiddles(log2n, re_im);
    return GRAIL_OK;
}

int grail_spectrum_frames(uint64_t n, uint32_t hop, uint64_t *n_frames)
{
    if (!n_frames || hop == 0) return GRAIL_ERR_INVALID_ARG;
    *n_frames = n / hop + (n % hop ? 1u : 0u);
    return GRAIL_OK;
}

int grail_spectrum_window(int kind, uint32_t n_window, float *w)
{
    if (!w || n_window < 1 || n_window > (1u << GRAIL_SPECTRUM_LOG2_MAX)) return GRAIL_ERR_INVALID_ARG;
    if (kind != GRAIL_SPECTRUM_RECT && kind != GRAIL_SPECTRUM_HANN && kind != GRAIL_SPECTRUM_HAMMING) return GRAIL_ERR_INVALID_ARG;
    const double a = kind == GRAIL_SPECTRUM_HANN ? 0.5 : 0.54;
    for (uint32_t j = 0; j < n_window; ++j)
        w[j] = kind == GRAIL_SPECTRUM_RECT ? 1.0f : (float)(a - (1.0 - a) * std::cos((grail::TWO_PI * (double)j) / (double)n_window));
    return GRAIL_OK;
}

int grail_mel_design(uint32_t sample_rate, uint32_t log2n, uint32_t n_bands, double lo_hz, double hi_hz, uint32_t *first,
                     uint32_t *count, float *weights, uint32_t cap, uint32_t *n_weights)
{
    if (!first || !count || !n_weights || (cap && !weights)) return GRAIL_ERR_INVALID_ARG;
    if (sample_rate == 0 || !grail::log2n_ok(log2n) || n_bands < 1 || n_bands > GRAIL_SPECTRUM_BANDS_MAX) return GRAIL_ERR_INVALID_ARG;
    // (written so that a NaN fails)
    if (!(lo_hz >= 0.0 && lo_hz < hi_hz && hi_hz <= (double)sample_rate / 2.0)) return GRAIL_ERR_INVALID_ARG;
    const uint32_t N = 1u << log2n, B = n_bands;
    double p[GRAIL_SPECTRUM_BANDS_MAX + 2];
    const double m_lo = grail::mel_of(lo_hz), m_hi = grail::mel_of(hi_hz);
    for (uint32_t i = 0; i < B + 2u; ++i) {
        p[i] = grail::hz_of(m_lo + ((m_hi - m_lo) * (double)i) / (double)(B + 1u));
        if (i && !(p[i] > p[i - 1u])) return GRAIL_ERR_INVALID_ARG;
    }
    // a pass to count, a pass to write: a table that does not fit leaves the caller's arrays as they were
    uint32_t lo[GRAIL_SPECTRUM_BANDS_MAX], n[GRAIL_SPECTRUM_BANDS_MAX];
    uint64_t total = 0;
    for (uint32_t b = 0; b < B; ++b) {
        lo[b] = n[b] = 0;
        for (uint32_t k = 0; k <= N / 2u; ++k) {
            const double f = ((double)k * (double)sample_rate) / (double)N;
            if (!(grail::mel_weight(f, p[b], p[b + 1u], p[b + 2u]) > 0.0f)) continue;
            if (n[b] == 0) lo[b] = k;
            n[b] = k - lo[b] + 1u;              // (the bins above 0 are the ones inside (l, r): no gap between them)
        }
        total += n[b];
    }
    *n_weights = (uint32_t)total;               // (at most 256 * 2049)
    if (total > cap) return GRAIL_ERR_BUFFER_TOO_SMALL;
    size_t at = 0;
    for (uint32_t b = 0; b < B; ++b) {
        first[b] = lo[b], count[b] = n[b];
        for (uint32_t k = 0; k < n[b]; ++k) {
            const double f = ((double)(lo[b] + k) * (double)sample_rate) / (double)N;
            weights[at++] = grail::mel_weight(f, p[b], p[b + 1u], p[b + 2u]);
        }
    }
    return GRAIL_OK;
}

}  // extern "C"
