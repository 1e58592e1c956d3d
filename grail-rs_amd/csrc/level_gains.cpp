// level_gains.cpp — the host side of levels that needs no device: grail_level_gains (a row's numbers and a target level
// per item -> the item's gain), grail_active_level (a row's level over its active frames) and the host side of the
// K-weighted loudness: grail_kweighting, grail_gated_mean_square, grail_loudness_lufs, grail_loudness_level, grail_loudness_window_max,
// grail_loudness_range; and of the
// true peak: grail_true_peak_coefficients, grail_true_peak_db, grail_true_peak_limit_gains, grail_limit_ceiling.  No HIP call, so it builds
// with g++ under AddressSanitizer and UBSan (tests/test_levels_host.py, tests/test_loudness_host.py,
// tests/test_true_peak_host.py), as mix_plan.cpp does.  DESIGN.md §4.9, §4.10, §4.11.
#include <algorithm>
#include <cmath>
#include <vector>

#include "../../include/grail_hip.h"
#include "true_peak_taps.h"

extern "C" {

int grail_level_gains(int mode, const double *sumsq, const float *peak, const uint32_t *nonfinite,
                      const uint32_t *row_len, const double *active_level, uint32_t n_rows,
                      const uint32_t *item_rows, const float *item_level_db, uint32_t n_items, float *item_gains,
                      uint32_t *n_unleveled)
{
    if (mode != GRAIL_LEVEL_PEAK && mode != GRAIL_LEVEL_RMS && mode != GRAIL_LEVEL_ACTIVE && mode != GRAIL_LEVEL_LOUDNESS)
        return GRAIL_ERR_INVALID_ARG;
    if (n_items && (!item_rows || !item_level_db || !item_gains)) return GRAIL_ERR_INVALID_ARG;
    if (n_items && mode == GRAIL_LEVEL_PEAK && !peak) return GRAIL_ERR_INVALID_ARG;
    if (n_items && mode == GRAIL_LEVEL_RMS && (!sumsq || !row_len)) return GRAIL_ERR_INVALID_ARG;
    if (n_items && (mode == GRAIL_LEVEL_ACTIVE || mode == GRAIL_LEVEL_LOUDNESS) && !active_level) return GRAIL_ERR_INVALID_ARG;
    for (uint32_t i = 0; i < n_items; ++i)
        if (item_rows[i] >= n_rows) return GRAIL_ERR_INVALID_ARG;          // (before the first gain is written)
    uint32_t unleveled = 0;
    for (uint32_t i = 0; i < n_items; ++i) {
        const uint32_t r = item_rows[i];
        double level = 0.0;
        if (mode == GRAIL_LEVEL_PEAK) level = (double)peak[r];
        else if (mode == GRAIL_LEVEL_RMS) level = row_len[r] ? std::sqrt(sumsq[r] / (double)row_len[r]) : 0.0;
        else level = active_level[r];
        // a level that is 0 (an empty or silent row) or no number, or a row holding a non-finite sample: left out
        if (!(level > 0.0) || !std::isfinite(level) || (nonfinite && nonfinite[r])) {
            item_gains[i] = 0.0f;
            ++unleveled;
            continue;
        }
        item_gains[i] = (float)(std::pow(10.0, (double)item_level_db[i] / 20.0) / level);
    }
    if (n_unleveled) *n_unleveled = unleveled;
    return GRAIL_OK;
}

double grail_active_level(const double *frame_sumsq, uint32_t row_len, uint32_t frame, float floor_db)
{
    if (!frame_sumsq || row_len == 0 || frame == 0) return 0.0;
    const uint32_t frames = row_len / frame + (row_len % frame != 0);
    const auto count = [&](uint32_t f) { return (double)(f + 1 < frames ? frame : row_len - f * frame); };
    double loudest = 0.0;
    for (uint32_t f = 0; f < frames; ++f) {
        const double ms = frame_sumsq[f] / count(f);
        if (ms > loudest) loudest = ms;
    }
    if (!(loudest > 0.0)) return 0.0;
    const double threshold = loudest * std::pow(10.0, -(double)floor_db / 10.0);
    double sum = 0.0, samples = 0.0;
    for (uint32_t f = 0; f < frames; ++f) {
        if (frame_sumsq[f] / count(f) >= threshold) {
            sum = sum + frame_sumsq[f];
            samples = samples + count(f);
        }
    }
    return samples > 0.0 ? std::sqrt(sum / samples) : 0.0;
}

int grail_kweighting(uint32_t sample_rate, double coef[10])
{
    if (!coef || sample_rate < GRAIL_LOUDNESS_RATE_MIN || sample_rate > GRAIL_LOUDNESS_RATE_MAX) return GRAIL_ERR_INVALID_ARG;
    const double pi = 3.141592653589793, rate = (double)sample_rate;
    {       // the shelf
        const double K = std::tan(pi * 1681.974450955533 / rate), Q = 0.7071752369554196;
        const double Vh = std::pow(10.0, 3.999843853973347 / 20.0), Vb = std::pow(Vh, 0.4996667741545416);
        const double a0 = 1.0 + K / Q + K * K;
        coef[0] = (Vh + Vb * K / Q + K * K) / a0;
        coef[1] = 2.0 * (K * K - Vh) / a0;
        coef[2] = (Vh - Vb * K / Q + K * K) / a0;
        coef[3] = 2.0 * (K * K - 1.0) / a0;
        coef[4] = (1.0 - K / Q + K * K) / a0;
    }
    {       // the high-pass
        const double K = std::tan(pi * 38.13547087602444 / rate), Q = 0.5003270373238773;
        const double a0 = 1.0 + K / Q + K * K;
        coef[5] = 1.0;
        coef[6] = -2.0;
        coef[7] = 1.0;
        coef[8] = 2.0 * (K * K - 1.0) / a0;
        coef[9] = (1.0 - K / Q + K * K) / a0;
    }
    return GRAIL_OK;
}

double grail_gated_mean_square(const double *hop_sumsq, uint32_t n_hops, uint32_t hop)
{
    if (!hop_sumsq || hop == 0 || n_hops < 4) return 0.0;
    const uint32_t blocks = n_hops - 3u;
    const double per = 4.0 * (double)hop;
    const auto block = [&](uint32_t j) {
        return (((hop_sumsq[j] + hop_sumsq[j + 1]) + hop_sumsq[j + 2]) + hop_sumsq[j + 3]) / per;
    };
    double sum = 0.0;
    uint32_t count = 0;
    for (uint32_t j = 0; j < blocks; ++j) {
        const double z = block(j);
        if (z > GRAIL_LOUDNESS_ABS_GATE) {
            sum = sum + z;
            ++count;
        }
    }
    if (count == 0) return 0.0;
    const double r = 0.1 * (sum / (double)count);
    sum = 0.0;
    count = 0;
    for (uint32_t j = 0; j < blocks; ++j) {
        const double z = block(j);
        if (z > GRAIL_LOUDNESS_ABS_GATE && z > r) {
            sum = sum + z;
            ++count;
        }
    }
    return count ? sum / (double)count : 0.0;
}

double grail_loudness_lufs(double gated_ms)
{
    if (!(gated_ms > 0.0)) return gated_ms == 0.0 ? -HUGE_VAL : gated_ms;      // (a NaN or a negative stays what it is)
    return -0.691 + 10.0 * std::log10(gated_ms);
}

double grail_loudness_level(double gated_ms) { return std::sqrt(gated_ms * GRAIL_LOUDNESS_LEVEL_SCALE); }

namespace {

// the mean square of the window of `window` hops that starts at hop j: a left fold from h[j]
double window_block(const double *h, uint32_t j, uint32_t window, double per)
{
    double sum = h[j];
    for (uint32_t i = 1; i < window; ++i) sum = sum + h[j + i];
    return sum / per;
}

}  // namespace

double grail_loudness_window_max(const double *hop_sumsq, uint32_t n_hops, uint32_t hop, uint32_t window_hops)
{
    if (!hop_sumsq || hop == 0 || window_hops == 0 || n_hops < window_hops) return 0.0;
    const double per = (double)window_hops * (double)hop;
    double largest = 0.0;
    for (uint32_t j = 0; j <= n_hops - window_hops; ++j) {
        const double z = window_block(hop_sumsq, j, window_hops, per);
        if (z > largest) largest = z;
    }
    return largest;
}

double grail_loudness_range(const double *hop_sumsq, uint32_t n_hops, uint32_t hop)
{
    const uint32_t window = 30;
    if (!hop_sumsq || hop == 0 || n_hops < window) return 0.0;
    const uint32_t blocks = n_hops - window + 1u;
    const double per = (double)window * (double)hop;
    std::vector<double> kept;
    kept.reserve(blocks);
    double sum = 0.0;
    for (uint32_t j = 0; j < blocks; ++j) {
        const double z = window_block(hop_sumsq, j, window, per);
        if (z > GRAIL_LOUDNESS_ABS_GATE) {
            sum = sum + z;
            kept.push_back(z);
        }
    }
    if (kept.empty()) return 0.0;
    const double r = 0.01 * (sum / (double)kept.size());
    size_t n = 0;
    for (const double z : kept)
        if (z > r) kept[n++] = z;
    if (n == 0) return 0.0;         // (cannot happen for numbers: the largest block is above a hundredth of the mean)
    kept.resize(n);
    std::sort(kept.begin(), kept.end());
    const double lo = kept[(size_t)(((uint64_t)(n - 1) * 10u + 50u) / 100u)];
    const double hi = kept[(size_t)(((uint64_t)(n - 1) * 95u + 50u) / 100u)];
    return 10.0 * std::log10(hi / lo);
}

int grail_true_peak_coefficients(double coef[GRAIL_TRUE_PEAK_PHASES * GRAIL_TRUE_PEAK_TAPS])
{
    if (!coef) return GRAIL_ERR_INVALID_ARG;
    for (int p = 0; p < GRAIL_TRUE_PEAK_PHASES; ++p)
        for (int k = 0; k < GRAIL_TRUE_PEAK_TAPS; ++k) coef[p * GRAIL_TRUE_PEAK_TAPS + k] = grail::true_peak_tap(p, k);
    return GRAIL_OK;
}

double grail_true_peak_db(double true_peak)
{
    if (true_peak == 0.0) return -HUGE_VAL;
    if (!(true_peak > 0.0)) return std::nan("");        // (no true peak is negative; a NaN stays one)
    return 20.0 * std::log10(true_peak);
}

float grail_limit_ceiling(float ceiling_db) { return (float)std::pow(10.0, (double)ceiling_db / 20.0); }

int grail_true_peak_limit_gains(const double *true_peak, uint32_t n_rows, const uint32_t *item_rows, uint32_t n_items,
                                float ceiling_db, float *item_gains, uint32_t *n_limited)
{
    if (!std::isfinite(ceiling_db)) return GRAIL_ERR_INVALID_ARG;
    if (n_items && (!true_peak || !item_rows || !item_gains)) return GRAIL_ERR_INVALID_ARG;
    for (uint32_t i = 0; i < n_items; ++i)
        if (item_rows[i] >= n_rows) return GRAIL_ERR_INVALID_ARG;          // (before the first gain is written)
    const double c = std::pow(10.0, (double)ceiling_db / 20.0);
    uint32_t limited = 0;
    for (uint32_t i = 0; i < n_items; ++i) {
        const double tp = true_peak[item_rows[i]];
        const float g = item_gains[i];
        if (!(tp > 0.0) || !((double)std::fabs(g) * tp > c)) continue;
        float q = (float)(c / tp);
        if ((double)q * tp > c) q = std::nextafterf(q, 0.0f);      // rounded up past the ceiling: one step back is under it
        item_gains[i] = std::signbit(g) ? -q : q;
        ++limited;
    }
    if (n_limited) *n_limited = limited;
    return GRAIL_OK;
}

}  // extern "C"
