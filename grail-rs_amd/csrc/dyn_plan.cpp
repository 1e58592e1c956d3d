// dyn_plan.cpp — the host side of dynamics that needs no device: grail_dyn_design (the soft-knee compressor and its mirror,
// the expander, as a table of gains), grail_dyn_ballistics, lev[k] and the lookup's index arithmetic, the checks of a curve set,
// of grail_dyn_async and of the calls on dynamics streams (their common end: row_checks.h), and the image of a set as the
// kernel reads it.  The contract is include/grail_hip.h, "levels, continued: dynamics".  No HIP call, so it builds with g++
// under AddressSanitizer and UBSan (tests/test_dyn_sanitize.py), as iir_plan.cpp does.  DESIGN.md §4.23.
#include <cmath>
#include <cstdint>
#include <cstring>

#include "../../include/grail_hip.h"
#include "dyn_plan.h"
#include "row_checks.h"

// the lookup and the image's differences are the contract's arithmetic: every operation rounded by itself under either
// compiler, whatever its flags
#if defined(__clang__)
#pragma clang fp contract(off)
#elif defined(__GNUC__)
#pragma GCC optimize("fp-contract=off")
#endif

namespace grail {

static_assert(DYN_POINTS == GRAIL_DYN_POINTS && DYN_STEPS == GRAIL_DYN_STEPS_PER_OCTAVE, "the table is the header's");
static_assert(DYN_LOG2_LO == GRAIL_DYN_LOG2_LO && DYN_LOG2_HI == GRAIL_DYN_LOG2_HI, "the table's range is the header's");
static_assert((DYN_LOG2_HI - DYN_LOG2_LO) * (int32_t)DYN_STEPS + 1 == (int32_t)DYN_POINTS, "a point a step, both ends in");

double dyn_level(uint32_t k)
{
    return std::ldexp(1.0 + (double)(k % DYN_STEPS) / (double)DYN_STEPS, DYN_LOG2_LO + (int)(k / DYN_STEPS));
}

void dyn_index(double e, uint32_t *k, double *f, bool *inside)
{
    const double lo = std::ldexp(1.0, DYN_LOG2_LO), hi = std::ldexp(1.0, DYN_LOG2_HI);
    uint64_t bits;
    std::memcpy(&bits, &e, sizeof bits);
    *inside = e >= lo && e < hi;
    // (inside, the sign is clear and the exponent field lies in 991 .. 1030: the difference is 0 .. 639)
    const uint32_t raw = (uint32_t)(bits >> 48) - DYN_KEY_LO;
    *k = e < lo ? 0u : (*inside ? raw : DYN_POINTS - 1u);
    // m's low 48 bits as the top of a mantissa under the exponent of 1.0: 1 + f, and the subtraction is exact
    const uint64_t one_f = 0x3FF0000000000000ull | ((bits & 0xFFFFFFFFFFFFull) << 4);
    double of;
    std::memcpy(&of, &one_f, sizeof of);
    *f = *inside ? of - 1.0 : 0.0;
}

double dyn_lookup(const double *gain, double e)
{
    uint32_t k;
    double f;
    bool inside;
    dyn_index(e, &k, &f, &inside);
    if (!inside) return gain[k];
    return gain[k] + f * (gain[k + 1u] - gain[k]);
}

const char *dyn_set_error(const double *gain, const double *alpha, const uint32_t *detector, uint32_t n_curves)
{
    if (!gain || !alpha || !detector) return "NULL argument";
    if (n_curves < 1 || n_curves > GRAIL_DYN_CURVES_MAX) return "n_curves is outside 1 .. 16";
    for (uint32_t c = 0; c < n_curves; ++c) {
        if (detector[c] != GRAIL_DYN_PEAK && detector[c] != GRAIL_DYN_SQUARE) return "a detector is neither PEAK nor SQUARE";
        // (written so that a NaN fails)
        for (uint32_t i = 0; i < 2; ++i)
            if (!(alpha[2u * c + i] >= 0.0 && alpha[2u * c + i] < 1.0)) return "an alpha is outside [0, 1)";
        for (uint32_t k = 0; k < DYN_POINTS; ++k) {
            const double g = gain[(size_t)c * DYN_POINTS + k];
            if (!std::isfinite(g)) return "a gain is not finite";
            if (!(g >= 0.0)) return "a gain is negative";
        }
    }
    return nullptr;
}

void dyn_set_image(const double *gain, uint32_t n_curves, std::vector<double> &image)
{
    image.assign((size_t)n_curves * DYN_IMAGE_DOUBLES, 0.0);
    for (uint32_t c = 0; c < n_curves; ++c) {
        const double *g = gain + (size_t)c * DYN_POINTS;
        double *at = image.data() + (size_t)c * DYN_IMAGE_DOUBLES;
        for (uint32_t k = 0; k < DYN_POINTS; ++k) {
            at[2u * k] = g[k];
            at[2u * k + 1u] = k + 1u < DYN_POINTS ? g[k + 1u] - g[k] : 0.0;
        }
    }
}

namespace {

// [a, a + a_samples) and [b, b + b_samples) in float32 share a byte (both spans fit 2^60 samples)
bool spans_overlap(const void *a, uint64_t a_samples, const void *b, uint64_t b_samples)
{
    const uintptr_t a0 = (uintptr_t)a, a1 = a0 + (uintptr_t)(a_samples * 4u);
    const uintptr_t b0 = (uintptr_t)b, b1 = b0 + (uintptr_t)(b_samples * 4u);
    return a0 < b1 && b0 < a1;
}

// what a keyed call checks of its keys once the pair of rows is fine: n_keys rows of key_stride at key, against the
// n_rows rows of out_stride written at out
const char *key_error(const void *key, uint64_t key_stride, uint32_t n_keys, const void *key_row, uint32_t n_rows, const void *out,
                      uint64_t out_stride)
{
    if (n_keys == 0) return "key_dev with n_keys = 0";
    if (!key_row && n_keys < n_rows) return "key_row_dev is NULL and n_keys < n_rows";
    if (!rows_span_fits(key_stride, n_keys)) return ROWS_SPAN;
    if (out && out_stride && key_stride && spans_overlap(key, (uint64_t)n_keys * key_stride, out, (uint64_t)n_rows * out_stride))
        return "out_dev overlaps key_dev (a wave reads ahead of another's stores)";
    return nullptr;
}

}  // namespace

const char *dyn_call_error(const void *rows, uint64_t row_stride, const void *len, uint32_t n_rows, const void *key,
                           uint64_t key_stride, uint32_t n_keys, const void *key_row, const void *out, uint64_t out_stride)
{
    // (a row holds fewer than 2^32 samples, for len is 32 bits wide; strides that allow more all the same are refused)
    if (const char *why = row_pair_error({rows, row_stride, len, n_rows, out, out_stride}, OutRule::when_out_stride,
                                         OutRule::when_out_stride, "out_dev overlaps rows_dev (a wave reads ahead of another's stores)",
                                         row_stride))
        return why;
    if (n_rows == 0 || !key) return nullptr;
    return key_error(key, key_stride, n_keys, key_row, n_rows, row_stride ? out : nullptr, out_stride);
}

const char *dyn_stream_open_error(const uint32_t *curve, uint32_t n_rows, uint32_t n_curves, uint32_t n_keys, const uint32_t *key_row)
{
    if (n_rows == 0) return "n_rows is 0";
    if (curve)
        for (uint32_t u = 0; u < n_rows; ++u)
            if (curve[u] >= n_curves) return "a row's curve index is outside the set";
    if (n_keys == 0) return nullptr;
    if (!key_row) return n_keys < n_rows ? "key_row is NULL and n_keys < n_rows" : nullptr;
    for (uint32_t u = 0; u < n_rows; ++u)
        if (key_row[u] >= n_keys) return "a row's key index is outside n_keys";
    return nullptr;
}

// (a stream has rows: dyn_stream_open_error; a call feeds a row fewer than 2^32 samples: in_len is 32 bits wide)
const char *dyn_stream_next_error(const void *in, uint64_t in_stride, const void *in_len, uint32_t n_rows, bool keyed,
                                  uint32_t n_keys, const void *key, uint64_t key_stride, const void *out, uint64_t out_stride)
{
    if (out_stride < in_stride) return "out_stride < in_stride (a stream never cuts outputs short)";
    if (keyed && in_stride && !key) return "a keyed stream needs key_dev";
    if (!keyed && key) return "a self-keyed stream takes no key_dev";
    if (keyed && key_stride < in_stride) return "key_stride < in_stride (the key advances with the row it drives)";
    if (const char *why = row_pair_error({in, in_stride, in_len, n_rows, out, out_stride}, OutRule::always, OutRule::always,
                                         "out_dev overlaps in_dev (a wave reads ahead of another's stores)", 0))
        return why;
    if (!keyed || in_stride == 0) return nullptr;
    // (the rows' key indices were checked at open, so key_row is not asked about here)
    return key_error(key, key_stride, n_keys, key, n_rows, out, out_stride);
}

}  // namespace grail

extern "C" {

int grail_dyn_design(int kind, int detector, double threshold_db, double ratio, double knee_db, double range_db, double makeup_db,
                     double *gain)
{
    if (!gain || (kind != GRAIL_DYN_COMPRESS && kind != GRAIL_DYN_EXPAND) || (detector != GRAIL_DYN_PEAK && detector != GRAIL_DYN_SQUARE))
        return GRAIL_ERR_INVALID_ARG;
    // (written so that a NaN fails)
    if (!std::isfinite(threshold_db) || !std::isfinite(makeup_db) || !(ratio >= 1.0 && std::isfinite(ratio)) ||
        !(knee_db >= 0.0 && std::isfinite(knee_db)) || !(range_db >= 0.0 && std::isfinite(range_db)))
        return GRAIL_ERR_INVALID_ARG;
    const double T = threshold_db, R = ratio, W = knee_db, h = W / 2.0;
    double table[grail::DYN_POINTS];
    for (uint32_t k = 0; k < grail::DYN_POINTS; ++k) {
        const double l = std::log10(grail::dyn_level(k));
        const double x = detector == GRAIL_DYN_PEAK ? 20.0 * l : 10.0 * l;
        const double d = x - T;
        double r;
        if (kind == GRAIL_DYN_COMPRESS) {
            if (d <= -h) {
                r = 0.0;
            } else if (d >= h) {
                r = (T + d / R) - x;
            } else {
                const double q = d + h;
                r = ((1.0 / R - 1.0) * (q * q)) / (2.0 * W);
            }
        } else {
            if (d >= h) {
                r = 0.0;
            } else if (d <= -h) {
                r = (T + d * R) - x;
            } else {
                const double q = d - h;
                r = ((1.0 - R) * (q * q)) / (2.0 * W);
            }
            if (r < -range_db) r = -range_db;
        }
        table[k] = std::pow(10.0, (r + makeup_db) / 20.0);
        if (!std::isfinite(table[k])) return GRAIL_ERR_INVALID_ARG;
    }
    std::memcpy(gain, table, sizeof table);
    return GRAIL_OK;
}

int grail_dyn_ballistics(uint32_t sample_rate, double attack_ms, double release_ms, double alpha[2])
{
    if (!alpha || sample_rate == 0) return GRAIL_ERR_INVALID_ARG;
    const double ms[2] = {attack_ms, release_ms};
    double got[2];
    for (int i = 0; i < 2; ++i) {
        if (!(ms[i] >= 0.0 && std::isfinite(ms[i]))) return GRAIL_ERR_INVALID_ARG;
        got[i] = ms[i] == 0.0 ? 0.0 : std::exp(-1000.0 / (ms[i] * (double)sample_rate));
        if (!(got[i] < 1.0)) return GRAIL_ERR_INVALID_ARG;
    }
    alpha[0] = got[0], alpha[1] = got[1];
    return GRAIL_OK;
}

}  // extern "C"
