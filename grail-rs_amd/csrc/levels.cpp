// levels.cpp — rendered rows measured on the device: grail_levels_async, grail_frame_levels_async, grail_loudness_async,
// grail_loudness_segmented_async and grail_true_peak_async, grail_limit_async (checks, the scratch, the launches) and what grail_batch_mix_leveled and its
// _limited form (mix.cpp) need per block.  The kernels are level_kernels.hip, loudness_kernels.hip, loudness_segment_kernels.hip, true_peak_kernels.hip
// and limiter_kernels.hip, the gains are level_gains.cpp (pure host).  DESIGN.md §4.9, §4.10, §4.11, §4.12.
#include "api_internal.hpp"

using namespace grail;
using namespace grail::host;

// Per context (grail_ctx::level_state), grown and never shrunk, freed by grail_destroy: the per-frame numbers that a
// totals call folds (16 B per frame of 4096 samples: 0.1 % of the rows), one block's totals for the leveled mix, and the
// hop sums of a loudness call that does not ask for them (8 B per hop of 100 ms), and the chunk maxima and counts that a
// true-peak call folds (12 B per chunk of 4096 output times) with one block's true peaks for the limited mix, and the
// chunk numbers that a limiter call folds (16 B per group and chunk of 4096 samples), and the hops' non-finite counts that a
// segmented loudness call folds (4 B per hop).
struct LevelState {
    double *d_fsum = nullptr;
    float *d_fpeak = nullptr;
    uint32_t *d_fbad = nullptr;
    size_t cap_fsum = 0, cap_fpeak = 0, cap_fbad = 0;
    double *d_sumsq = nullptr;
    float *d_peak = nullptr;
    uint32_t *d_bad = nullptr;
    size_t cap_sumsq = 0, cap_peak = 0, cap_bad = 0;
    double *d_hops = nullptr;
    size_t cap_hops = 0;
    double *d_cmax = nullptr;
    uint32_t *d_cbad = nullptr;
    size_t cap_cmax = 0, cap_cbad = 0;
    double *d_tp = nullptr;
    size_t cap_tp = 0;
    unsigned char *d_lstat = nullptr;
    size_t cap_lstat = 0;
    uint32_t *d_hbad = nullptr;
    size_t cap_hbad = 0;
};

namespace grail {
namespace host {

void levels_release(grail_ctx *ctx)
{
    LevelState *st = (LevelState *)ctx->level_state;
    if (!st) return;
    for (void *p : {(void *)st->d_fsum, (void *)st->d_fpeak, (void *)st->d_fbad, (void *)st->d_sumsq, (void *)st->d_peak,
                    (void *)st->d_bad, (void *)st->d_hops, (void *)st->d_cmax, (void *)st->d_cbad, (void *)st->d_tp, (void *)st->d_lstat,
                    (void *)st->d_hbad})
        if (p) (void)hipFree(p);
    delete st;
    ctx->level_state = nullptr;
}

}  // namespace host
}  // namespace grail

namespace {

template <typename T>
int reserve(grail_ctx *ctx, T **p, size_t *cap, size_t n)
{
    n = std::max<size_t>(n, 1);
    if (*cap >= n) return GRAIL_OK;
    if (*p) {
        HIP_TRY(hipStreamSynchronize(ctx->stream));    // (a queued measurement may still use the old buffer)
        HIP_TRY(hipFree(*p));
        *p = nullptr;
        *cap = 0;
    }
    HIP_TRY(hipMalloc((void **)p, n * sizeof(T)));
    *cap = n;
    return GRAIL_OK;
}

// a context, or why there is none: the device entry points say GRAIL_ERR_NO_DEVICE on a machine without a GPU
int bind_device(grail_ctx *ctx, const char *who)
{
    if (ctx) return bind(ctx);
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n < 1)
        return fail(GRAIL_ERR_NO_DEVICE, std::string(who) + ": no usable HIP device (there is no CPU fallback)");
    return fail(GRAIL_ERR_INVALID_ARG, std::string(who) + ": ctx is NULL");
}

LevelState *state(grail_ctx *ctx)
{
    if (!ctx->level_state) ctx->level_state = new (std::nothrow) LevelState();
    return (LevelState *)ctx->level_state;
}

uint64_t ceil_div(uint64_t a, uint64_t b) { return a / b + (a % b != 0); }

// the rows' totals with frames of GRAIL_LEVEL_FRAME through the context's frame scratch (which then holds the frames'
// numbers at stride ceil(row_stride / GRAIL_LEVEL_FRAME) until the context's next measurement)
int totals(grail_ctx *ctx, const char *who, const float *rows_dev, uint64_t row_stride, const uint32_t *len_dev,
           uint32_t n_rows, double *sumsq_dev, float *peak_dev, uint32_t *nonfinite_dev)
{
    LevelState *st = state(ctx);
    if (!st) return fail(GRAIL_ERR_OUT_OF_MEMORY, "level state");
    const uint64_t frames = ceil_div(row_stride, GRAIL_LEVEL_FRAME);
    if (frames == 0) {          // rows of no samples: +0.0, +0.0f, 0
        const hipError_t e = launch_level_totals(len_dev, 0, n_rows, GRAIL_LEVEL_FRAME, nullptr, nullptr, nullptr, 0,
                                                 sumsq_dev, peak_dev, nonfinite_dev, ctx->stream);
        if (e != hipSuccess) return hip_fail(e, "level totals kernel launch");
        return GRAIL_OK;
    }
    if (frames > 0xFFFFFFFFull || (uint64_t)n_rows * frames > (1ull << 32))
        return fail(GRAIL_ERR_INVALID_ARG, std::string(who) + ": more than 2^32 frames");
    const size_t cells = (size_t)n_rows * (size_t)frames;
    int rc;
    if ((rc = reserve(ctx, &st->d_fsum, &st->cap_fsum, cells))) return rc;
    if ((rc = reserve(ctx, &st->d_fpeak, &st->cap_fpeak, cells))) return rc;
    if ((rc = reserve(ctx, &st->d_fbad, &st->cap_fbad, cells))) return rc;
    hipError_t e = launch_level_frames(rows_dev, row_stride, len_dev, n_rows, GRAIL_LEVEL_FRAME, (uint32_t)frames, st->d_fsum,
                                       st->d_fpeak, st->d_fbad, frames, ctx->stream);
    if (e != hipSuccess) return hip_fail(e, "level frames kernel launch");
    e = launch_level_totals(len_dev, row_stride, n_rows, GRAIL_LEVEL_FRAME, st->d_fsum, st->d_fpeak, st->d_fbad, frames,
                            sumsq_dev, peak_dev, nonfinite_dev, ctx->stream);
    if (e != hipSuccess) return hip_fail(e, "level totals kernel launch");
    return GRAIL_OK;
}

// hop sums, gated mean squares and non-finite counts (any output may be NULL; hops_dev NULL = the context's scratch);
// segmented: every hop from a zero state GRAIL_LOUDNESS_WARMUP_HOPS hops before it, one lane per hop
int loudness(grail_ctx *ctx, const char *who, bool segmented, const float *rows_dev, uint64_t row_stride,
             const uint32_t *len_dev, uint32_t n_rows, uint32_t sample_rate, const double *coef, double *gated_dev,
             double *hops_dev, uint64_t hops_stride, uint32_t *nonfinite_dev)
{
    double own[10];
    if (!coef) {
        if (grail_kweighting(sample_rate, own)) return fail(GRAIL_ERR_INVALID_ARG, std::string(who) + ": sample rate out of range");
        coef = own;
    }
    const uint32_t hop = sample_rate / 10u;
    if (!hops_dev) {
        LevelState *st = state(ctx);
        if (!st) return fail(GRAIL_ERR_OUT_OF_MEMORY, "level state");
        hops_stride = row_stride / hop;
        if (hops_stride && (uint64_t)n_rows > (1ull << 40) / hops_stride)
            return fail(GRAIL_ERR_INVALID_ARG, std::string(who) + ": more than 2^40 hops");
        int rc;
        if ((rc = reserve(ctx, &st->d_hops, &st->cap_hops, (size_t)n_rows * (size_t)hops_stride))) return rc;
        hops_dev = st->d_hops;
    }
    hipError_t e;
    if (segmented) {
        const uint64_t lanes = loudness_segment_lanes(row_stride, hop), waves = loudness_segment_waves(row_stride, hop);
        // (the one refusal the serial call does not have: the launch is one grid of a wave per 64 hops of a row)
        if (waves > LOUD_SEGMENT_WAVES_MAX || (uint64_t)n_rows * waves > LOUD_SEGMENT_WAVES_MAX)
            return fail(GRAIL_ERR_INVALID_ARG, std::string(who) + ": more than 2^26 - 1 waves of 64 hops (n_rows * ceil(ceil(row_stride / H) / 64))");
        uint32_t *hop_bad = nullptr;
        if (nonfinite_dev) {
            LevelState *st = state(ctx);
            if (!st) return fail(GRAIL_ERR_OUT_OF_MEMORY, "level state");
            int rc;
            if ((rc = reserve(ctx, &st->d_hbad, &st->cap_hbad, (size_t)n_rows * (size_t)lanes))) return rc;
            hop_bad = st->d_hbad;
        }
        e = launch_loudness_segments(rows_dev, row_stride, len_dev, n_rows, hop, coef, hops_dev, hops_stride, hop_bad,
                                     nonfinite_dev, ctx->stream);
        if (e != hipSuccess) return hip_fail(e, "loudness segments kernel launch");
    } else {
        e = launch_loudness_hops(rows_dev, row_stride, len_dev, n_rows, hop, coef, hops_dev, hops_stride, nonfinite_dev,
                                 ctx->stream);
        if (e != hipSuccess) return hip_fail(e, "loudness hops kernel launch");
    }
    if (gated_dev) {
        e = launch_loudness_gate(len_dev, row_stride, n_rows, hop, hops_dev, hops_stride, gated_dev, ctx->stream);
        if (e != hipSuccess) return hip_fail(e, "loudness gate kernel launch");
    }
    return GRAIL_OK;
}

// the checks of grail_loudness_async and grail_loudness_segmented_async, which differ in nothing but the kernel
int loudness_call(grail_ctx *ctx, const char *who, bool segmented, const float *rows_dev, uint64_t row_stride,
                  const uint32_t *len_dev, uint32_t n_rows, uint32_t sample_rate, const double *coef, double *gated_ms_dev,
                  double *hop_sumsq_dev, uint64_t hops_stride, uint32_t *nonfinite_dev)
{
    int rc = bind_device(ctx, who);
    if (rc) return rc;
    if (sample_rate < GRAIL_LOUDNESS_RATE_MIN || sample_rate > GRAIL_LOUDNESS_RATE_MAX)
        return fail(GRAIL_ERR_INVALID_ARG, std::string(who) + ": sample_rate is outside 2 560 .. 1 048 576");
    if (hop_sumsq_dev && hops_stride < row_stride / (sample_rate / 10u))
        return fail(GRAIL_ERR_INVALID_ARG, std::string(who) + ": hops_stride < row_stride / (sample_rate / 10)");
    if (n_rows == 0) return GRAIL_OK;
    if (!len_dev || (row_stride && !rows_dev)) return fail(GRAIL_ERR_INVALID_ARG, std::string(who) + ": NULL buffer");
    if (!gated_ms_dev && !hop_sumsq_dev && !nonfinite_dev) return GRAIL_OK;
    return loudness(ctx, who, segmented, rows_dev, row_stride, len_dev, n_rows, sample_rate, coef, gated_ms_dev, hop_sumsq_dev,
                    hops_stride, nonfinite_dev);
}

// true peaks and non-finite counts (either output may be NULL) through the context's chunk scratch
int true_peak(grail_ctx *ctx, const char *who, const float *rows_dev, uint64_t row_stride, const uint32_t *len_dev,
              uint32_t n_rows, double *true_peak_dev, uint32_t *nonfinite_dev)
{
    LevelState *st = state(ctx);
    if (!st) return fail(GRAIL_ERR_OUT_OF_MEMORY, "level state");
    const uint64_t chunks = true_peak_grid_chunks(row_stride);
    if (chunks > 0xFFFFFFFFull || (uint64_t)n_rows * chunks > (1ull << 32))
        return fail(GRAIL_ERR_INVALID_ARG, std::string(who) + ": more than 2^32 chunks");
    if (chunks) {               // (rows of no samples: +0.0, 0 from the totals alone)
        const size_t cells = (size_t)n_rows * (size_t)chunks;
        int rc;
        if ((rc = reserve(ctx, &st->d_cmax, &st->cap_cmax, cells))) return rc;
        if ((rc = reserve(ctx, &st->d_cbad, &st->cap_cbad, cells))) return rc;
        const hipError_t e = launch_true_peak_frames(rows_dev, row_stride, len_dev, n_rows, (uint32_t)chunks, st->d_cmax,
                                                     st->d_cbad, ctx->stream);
        if (e != hipSuccess) return hip_fail(e, "true peak frames kernel launch");
    }
    const hipError_t e = launch_true_peak_totals(len_dev, row_stride, n_rows, st->d_cmax, st->d_cbad, (uint32_t)chunks,
                                                 true_peak_dev, nonfinite_dev, ctx->stream);
    if (e != hipSuccess) return hip_fail(e, "true peak totals kernel launch");
    return GRAIL_OK;
}

// grail_batch_mix_leveled_limited's part of a block, first half: the rows' true peaks queued behind the level's kernels
// and their copy to tp[n_rows] on the host, complete once the caller has waited for the stream (8 bytes a row more)
int queue_block_true_peaks(grail_ctx *ctx, LevelState *st, const float *rows_dev, uint64_t row_stride,
                           const uint32_t *len_dev, uint32_t n_rows, double *tp)
{
    int rc;
    if ((rc = reserve(ctx, &st->d_tp, &st->cap_tp, n_rows))) return rc;
    if ((rc = true_peak(ctx, "grail_batch_mix_leveled_limited", rows_dev, row_stride, len_dev, n_rows, st->d_tp, nullptr)))
        return rc;
    HIP_TRY(hipMemcpyAsync(tp, st->d_tp, (size_t)n_rows * 8, hipMemcpyDeviceToHost, ctx->stream));
    return GRAIL_OK;
}

// ... second half: the ceiling applied to the gains that grail_level_gains gave; *n_limited is added to
int limit_block_gains(const double *tp, uint32_t n_rows, const uint32_t *item_rows, uint32_t n_items, float ceiling_db,
                      float *gains, uint32_t *n_limited)
{
    uint32_t limited = 0;
    const int rc = grail_true_peak_limit_gains(tp, n_rows, item_rows, n_items, ceiling_db, gains, &limited);
    if (rc) return fail(rc, "grail_batch_mix_leveled_limited: grail_true_peak_limit_gains refused the block");
    *n_limited += limited;
    return GRAIL_OK;
}

}  // namespace

namespace grail {
namespace host {

uint32_t level_table_rate(const grail_ctx *ctx)
{
    uint32_t rate = 0;
    for (const grail_voice &v : ctx->voices) {
        const float r = v.sample_rate;
        if (!(r >= (float)GRAIL_LOUDNESS_RATE_MIN) || !(r <= (float)GRAIL_LOUDNESS_RATE_MAX)) return 0;
        const uint32_t whole = (uint32_t)r;
        if ((float)whole != r || (rate && whole != rate)) return 0;
        rate = whole;
    }
    return rate;
}

int level_block_gains(grail_ctx *ctx, int mode, uint32_t sample_rate, const float *rows_dev, uint64_t row_stride,
                      const uint32_t *len_dev, const uint32_t *row_len, uint32_t n_rows, const uint32_t *item_rows,
                      const float *item_level_db, uint32_t n_items, float *gains, uint32_t *n_unleveled,
                      const float *ceiling_db, uint32_t *n_limited)
{
    LevelState *st = state(ctx);
    if (!st) return fail(GRAIL_ERR_OUT_OF_MEMORY, "level state");
    if (n_rows == 0 || n_items == 0) return GRAIL_OK;
    int rc;
    std::vector<double> tp(ceiling_db ? n_rows : 0);      // with a ceiling: the rows' true peaks, brought back in the same wait
    if ((rc = reserve(ctx, &st->d_sumsq, &st->cap_sumsq, n_rows))) return rc;
    if ((rc = reserve(ctx, &st->d_peak, &st->cap_peak, n_rows))) return rc;
    if ((rc = reserve(ctx, &st->d_bad, &st->cap_bad, n_rows))) return rc;
    if (mode == GRAIL_LEVEL_LOUDNESS) {     // the gated mean squares in place of the totals: 12 bytes a row come back
        if ((rc = loudness(ctx, "grail_batch_mix_leveled", false, rows_dev, row_stride, len_dev, n_rows, sample_rate, nullptr,
                           st->d_sumsq, nullptr, 0, st->d_bad)))
            return rc;
        if (ceiling_db && (rc = queue_block_true_peaks(ctx, st, rows_dev, row_stride, len_dev, n_rows, tp.data()))) return rc;
        std::vector<double> gated(n_rows), level(n_rows);
        std::vector<uint32_t> bad(n_rows);
        HIP_TRY(hipMemcpyAsync(gated.data(), st->d_sumsq, (size_t)n_rows * 8, hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(hipMemcpyAsync(bad.data(), st->d_bad, (size_t)n_rows * 4, hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(hipStreamSynchronize(ctx->stream));
        for (uint32_t r = 0; r < n_rows; ++r) level[r] = grail_loudness_level(gated[r]);
        uint32_t unleveled = 0;
        rc = grail_level_gains(mode, nullptr, nullptr, bad.data(), row_len, level.data(), n_rows, item_rows, item_level_db,
                               n_items, gains, &unleveled);
        if (rc) return fail(rc, "grail_batch_mix_leveled: grail_level_gains refused the block");
        *n_unleveled += unleveled;
        return ceiling_db ? limit_block_gains(tp.data(), n_rows, item_rows, n_items, *ceiling_db, gains, n_limited) : GRAIL_OK;
    }
    if ((rc = totals(ctx, "grail_batch_mix_leveled", rows_dev, row_stride, len_dev, n_rows, st->d_sumsq, st->d_peak, st->d_bad)))
        return rc;
    if (ceiling_db && (rc = queue_block_true_peaks(ctx, st, rows_dev, row_stride, len_dev, n_rows, tp.data()))) return rc;
    std::vector<double> sumsq(n_rows), active;
    std::vector<float> peak(n_rows);
    std::vector<uint32_t> bad(n_rows);
    if (mode == GRAIL_LEVEL_RMS)
        HIP_TRY(hipMemcpyAsync(sumsq.data(), st->d_sumsq, (size_t)n_rows * 8, hipMemcpyDeviceToHost, ctx->stream));
    if (mode == GRAIL_LEVEL_PEAK)
        HIP_TRY(hipMemcpyAsync(peak.data(), st->d_peak, (size_t)n_rows * 4, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipMemcpyAsync(bad.data(), st->d_bad, (size_t)n_rows * 4, hipMemcpyDeviceToHost, ctx->stream));
    std::vector<double> frames;
    const uint64_t fs = ceil_div(row_stride, GRAIL_LEVEL_FRAME);
    if (mode == GRAIL_LEVEL_ACTIVE && fs) {
        frames.resize((size_t)n_rows * fs);
        HIP_TRY(hipMemcpyAsync(frames.data(), st->d_fsum, frames.size() * 8, hipMemcpyDeviceToHost, ctx->stream));
    }
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    if (mode == GRAIL_LEVEL_ACTIVE) {
        active.assign(n_rows, 0.0);
        // (frames past a row's last were never written: grail_active_level reads ceil(len / frame) of them)
        for (uint32_t r = 0; r < n_rows && fs; ++r)
            active[r] = grail_active_level(frames.data() + (size_t)r * fs, row_len[r], GRAIL_LEVEL_FRAME,
                                           GRAIL_LEVEL_ACTIVE_FLOOR_DB);
    }
    uint32_t unleveled = 0;
    rc = grail_level_gains(mode, sumsq.data(), peak.data(), bad.data(), row_len, active.data(), n_rows, item_rows,
                           item_level_db, n_items, gains, &unleveled);
    if (rc) return fail(rc, "grail_batch_mix_leveled: grail_level_gains refused the block");
    *n_unleveled += unleveled;
    return ceiling_db ? limit_block_gains(tp.data(), n_rows, item_rows, n_items, *ceiling_db, gains, n_limited) : GRAIL_OK;
}

}  // namespace host
}  // namespace grail

extern "C" {

int grail_levels_async(grail_ctx *ctx, const float *rows_dev, uint64_t row_stride, const uint32_t *len_dev,
                       uint32_t n_rows, double *sumsq_dev, float *peak_dev, uint32_t *nonfinite_dev)
{
    int rc = bind_device(ctx, "grail_levels_async");
    if (rc) return rc;
    if (n_rows == 0) return GRAIL_OK;
    if (!len_dev || (row_stride && !rows_dev)) return fail(GRAIL_ERR_INVALID_ARG, "grail_levels_async: NULL buffer");
    if (!sumsq_dev && !peak_dev && !nonfinite_dev) return GRAIL_OK;
    return totals(ctx, "grail_levels_async", rows_dev, row_stride, len_dev, n_rows, sumsq_dev, peak_dev, nonfinite_dev);
}

int grail_true_peak_async(grail_ctx *ctx, const float *rows_dev, uint64_t row_stride, const uint32_t *len_dev,
                          uint32_t n_rows, double *true_peak_dev, uint32_t *nonfinite_dev)
{
    int rc = bind_device(ctx, "grail_true_peak_async");
    if (rc) return rc;
    if (n_rows == 0) return GRAIL_OK;
    if (!len_dev || (row_stride && !rows_dev)) return fail(GRAIL_ERR_INVALID_ARG, "grail_true_peak_async: NULL buffer");
    if (!true_peak_dev && !nonfinite_dev) return GRAIL_OK;
    return true_peak(ctx, "grail_true_peak_async", rows_dev, row_stride, len_dev, n_rows, true_peak_dev, nonfinite_dev);
}

int grail_limit_async(grail_ctx *ctx, const float *rows_dev, uint64_t row_stride, const uint32_t *len_dev, uint32_t n_rows,
                      uint32_t group, float ceiling, uint32_t lookahead_log2, float *out_dev, uint64_t out_stride,
                      float *min_gain_dev, uint32_t *n_limited_dev, uint32_t *nonfinite_dev)
{
    // (what is wrong with the arguments is said before what is wrong with the machine)
    if (lookahead_log2 > GRAIL_LIMIT_LOOKAHEAD_LOG2_MAX)
        return fail(GRAIL_ERR_INVALID_ARG, "grail_limit_async: lookahead_log2 is above 10");
    if (group == 0 || n_rows % group != 0)
        return fail(GRAIL_ERR_INVALID_ARG, "grail_limit_async: n_rows is no multiple of group");
    if (!(ceiling > 0.0f) || !(ceiling <= 3.4028234663852886e38f))
        return fail(GRAIL_ERR_INVALID_ARG, "grail_limit_async: the ceiling is not a finite number above 0");
    if (out_stride < row_stride) return fail(GRAIL_ERR_INVALID_ARG, "grail_limit_async: out_stride < row_stride");
    if (n_rows && (!len_dev || (row_stride && (!rows_dev || !out_dev))))
        return fail(GRAIL_ERR_INVALID_ARG, "grail_limit_async: NULL buffer");
    if (n_rows && row_stride) {
        if (row_stride > (1ull << 60) / n_rows || out_stride > (1ull << 60) / n_rows)
            return fail(GRAIL_ERR_INVALID_ARG, "grail_limit_async: the rows span more than 2^60 samples");
        const uintptr_t in0 = (uintptr_t)rows_dev, in1 = in0 + (uintptr_t)(n_rows * row_stride * 4u);
        const uintptr_t out0 = (uintptr_t)out_dev, out1 = out0 + (uintptr_t)(n_rows * out_stride * 4u);
        if (in0 < out1 && out0 < in1)
            return fail(GRAIL_ERR_INVALID_ARG, "grail_limit_async: out_dev overlaps rows_dev (the look-ahead reads ahead of the stores)");
    }
    int rc = bind_device(ctx, "grail_limit_async");
    if (rc) return rc;
    if (n_rows == 0) return GRAIL_OK;
    LevelState *st = state(ctx);
    if (!st) return fail(GRAIL_ERR_OUT_OF_MEMORY, "level state");
    const uint32_t n_groups = n_rows / group;
    const uint64_t chunks = limit_grid_chunks(row_stride);
    if ((uint64_t)n_groups * chunks > 0x7FFFFFFFull) return fail(GRAIL_ERR_INVALID_ARG, "grail_limit_async: more than 2^31 chunks");
    if (chunks) {               // (rows of no samples: 1.0f, 0, 0 from the totals alone)
        if ((rc = reserve(ctx, &st->d_lstat, &st->cap_lstat, (size_t)n_groups * (size_t)chunks * limit_chunk_bytes()))) return rc;
        const hipError_t e = launch_limit_frames(rows_dev, row_stride, len_dev, n_groups, group, ceiling, lookahead_log2,
                                                 (uint32_t)chunks, out_dev, out_stride, st->d_lstat, ctx->stream);
        if (e != hipSuccess) return hip_fail(e, "limiter frames kernel launch");
    }
    if (!min_gain_dev && !n_limited_dev && !nonfinite_dev) return GRAIL_OK;
    const hipError_t e = launch_limit_totals(len_dev, row_stride, n_groups, group, lookahead_log2, st->d_lstat, (uint32_t)chunks,
                                             min_gain_dev, n_limited_dev, nonfinite_dev, ctx->stream);
    if (e != hipSuccess) return hip_fail(e, "limiter totals kernel launch");
    return GRAIL_OK;
}

int grail_loudness_async(grail_ctx *ctx, const float *rows_dev, uint64_t row_stride, const uint32_t *len_dev,
                         uint32_t n_rows, uint32_t sample_rate, const double *coef, double *gated_ms_dev,
                         double *hop_sumsq_dev, uint64_t hops_stride, uint32_t *nonfinite_dev)
{
    return loudness_call(ctx, "grail_loudness_async", false, rows_dev, row_stride, len_dev, n_rows, sample_rate, coef,
                         gated_ms_dev, hop_sumsq_dev, hops_stride, nonfinite_dev);
}

int grail_loudness_segmented_async(grail_ctx *ctx, const float *rows_dev, uint64_t row_stride, const uint32_t *len_dev,
                                   uint32_t n_rows, uint32_t sample_rate, const double *coef, double *gated_ms_dev,
                                   double *hop_sumsq_dev, uint64_t hops_stride, uint32_t *nonfinite_dev)
{
    return loudness_call(ctx, "grail_loudness_segmented_async", true, rows_dev, row_stride, len_dev, n_rows, sample_rate, coef,
                         gated_ms_dev, hop_sumsq_dev, hops_stride, nonfinite_dev);
}

int grail_frame_levels_async(grail_ctx *ctx, const float *rows_dev, uint64_t row_stride, const uint32_t *len_dev,
                             uint32_t n_rows, uint32_t frame, double *frame_sumsq_dev, float *frame_peak_dev,
                             uint64_t frames_stride)
{
    int rc = bind_device(ctx, "grail_frame_levels_async");
    if (rc) return rc;
    if (frame < GRAIL_LEVEL_FRAME_MIN || frame > GRAIL_LEVEL_FRAME_MAX)
        return fail(GRAIL_ERR_INVALID_ARG, "grail_frame_levels_async: frame is outside 256 .. 1 048 576");
    const uint64_t frames = ceil_div(row_stride, frame);
    if (frames_stride < frames)
        return fail(GRAIL_ERR_INVALID_ARG, "grail_frame_levels_async: frames_stride < ceil(row_stride / frame)");
    if (n_rows == 0 || frames == 0) return GRAIL_OK;
    if (!len_dev || !rows_dev) return fail(GRAIL_ERR_INVALID_ARG, "grail_frame_levels_async: NULL buffer");
    if (!frame_sumsq_dev && !frame_peak_dev) return GRAIL_OK;
    if (frames > 0xFFFFFFFFull || (uint64_t)n_rows * frames > (1ull << 32))
        return fail(GRAIL_ERR_INVALID_ARG, "grail_frame_levels_async: more than 2^32 frames");
    const hipError_t e = launch_level_frames(rows_dev, row_stride, len_dev, n_rows, frame, (uint32_t)frames, frame_sumsq_dev,
                                             frame_peak_dev, nullptr, frames_stride, ctx->stream);
    if (e != hipSuccess) return hip_fail(e, "level frames kernel launch");
    return GRAIL_OK;
}

}  // extern "C"
