// level_gains.cpp — the host side of levels that needs no device: grail_level_gains (a row's numbers and a target level
// per item -> the item's gain) and grail_active_level (a row's level over its active frames).  No HIP call, so it builds
// with g++ under AddressSanitizer and UBSan (tests/test_levels_host.py), as mix_plan.cpp does.  DESIGN.md §4.9.
#include <cmath>

#include "../../include/grail_hip.h"

extern "C" {

int grail_level_gains(int mode, const double *sumsq, const float *peak, const uint32_t *nonfinite,
                      const uint32_t *row_len, const double *active_level, uint32_t n_rows,
                      const uint32_t *item_rows, const float *item_level_db, uint32_t n_items, float *item_gains,
                      uint32_t *n_unleveled)
{
    if (mode != GRAIL_LEVEL_PEAK && mode != GRAIL_LEVEL_RMS && mode != GRAIL_LEVEL_ACTIVE) return GRAIL_ERR_INVALID_ARG;
    if (n_items && (!item_rows || !item_level_db || !item_gains)) return GRAIL_ERR_INVALID_ARG;
    if (n_items && mode == GRAIL_LEVEL_PEAK && !peak) return GRAIL_ERR_INVALID_ARG;
    if (n_items && mode == GRAIL_LEVEL_RMS && (!sumsq || !row_len)) return GRAIL_ERR_INVALID_ARG;
    if (n_items && mode == GRAIL_LEVEL_ACTIVE && !active_level) return GRAIL_ERR_INVALID_ARG;
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

}  // extern "C"
