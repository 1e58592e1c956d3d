// levels.cpp — rendered rows measured on the device: grail_levels_async, grail_frame_levels_async, grail_loudness_async,
// grail_loudness_segmented_async and grail_true_peak_async (checks, the scratch, the launches) and what
// grail_batch_mix_leveled and its _limited form (mix.cpp) need per block.  The kernels are level_kernels.hip,
// loudness_kernels.hip, loudness_segment_kernels.hip and true_peak_kernels.hip, the gains are level_gains.cpp (pure host).
// DESIGN.md §4.9, §4.10, §4.11.  The calls that write rows are transforms.cpp.
#include "api_internal.hpp"

using namespace grail;
using namespace grail::host;

// Per context (grail_ctx::level_state), kept from call to call and only ever grown (DeviceBuffer::reserve, to the exact
// size), freed by grail_destroy: the per-frame numbers that a totals call folds (16 B per frame of 4096 samples: 0.1 % of
// the rows), one block's totals for the leveled mix, the hop sums of a loudness call that does not ask for them (8 B per
// hop of 100 ms), the chunk maxima and counts that a true-peak call folds (12 B per chunk of 4096 output times) with one
// block's true peaks for the limited mix, the hops' non-finite counts that a segmented loudness call folds (4 B per hop).
struct LevelState : CtxPart {
    DeviceBuffer<double> d_fsum;            // frames: sums of squares,
    DeviceBuffer<float> d_fpeak;            // ... peaks
    DeviceBuffer<uint32_t> d_fbad;          // ... and non-finite counts
    DeviceBuffer<double> d_sumsq;           // a block's rows: the same three (loudness mode: gated mean squares in d_sumsq)
    DeviceBuffer<float> d_peak;
    DeviceBuffer<uint32_t> d_bad;
    DeviceBuffer<double> d_hops;            // hop sums
    DeviceBuffer<double> d_cmax;            // true-peak chunks: maxima
    DeviceBuffer<uint32_t> d_cbad;          // ... and non-finite counts
    DeviceBuffer<double> d_tp;              // a block's true peaks
    DeviceBuffer<uint32_t> d_hbad;          // segmented loudness: non-finite counts per hop
};

namespace {

// rows on the device as every measurement takes them: n rows at `stride`, row r of len[r] samples
struct Rows {
    const float *dev;
    uint64_t stride;
    const uint32_t *len;
    uint32_t n;
};

// what the measurement calls check alike, in this order: no rows is success, a missing buffer the caller's error, no
// output asked for success again; *measure says whether anything is left to do
int check_rows(const char *who, const Rows &r, bool any_output, bool *measure)
{
    *measure = false;
    if (r.n == 0) return GRAIL_OK;
    if (!r.len || (r.stride && !r.dev)) return fail(GRAIL_ERR_INVALID_ARG, std::string(who) + ": NULL buffer");
    *measure = any_output;
    return GRAIL_OK;
}

// the context's state, made at first use
int state(grail_ctx *ctx, LevelState **st)
{
    if (!ctx->level_state) ctx->level_state.reset(new (std::nothrow) LevelState());
    *st = static_cast<LevelState *>(ctx->level_state.get());
    return *st ? GRAIL_OK : fail(GRAIL_ERR_OUT_OF_MEMORY, "level state");
}

uint64_t ceil_div(uint64_t a, uint64_t b) { return a / b + (a % b != 0); }

// the rows' totals with frames of GRAIL_LEVEL_FRAME through the context's frame scratch (which then holds the frames'
// numbers at stride ceil(row_stride / GRAIL_LEVEL_FRAME) until the context's next measurement)
int totals(grail_ctx *ctx, const char *who, const Rows &r, double *sumsq_dev, float *peak_dev, uint32_t *nonfinite_dev)
{
    LevelState *st;
    int rc = state(ctx, &st);
    if (rc) return rc;
    const uint64_t frames = ceil_div(r.stride, GRAIL_LEVEL_FRAME);
    if (frames == 0) {          // rows of no samples: +0.0, +0.0f, 0
        const hipError_t e = launch_level_totals(r.len, 0, r.n, GRAIL_LEVEL_FRAME, nullptr, nullptr, nullptr, 0, sumsq_dev,
                                                 peak_dev, nonfinite_dev, ctx->stream);
        if (e != hipSuccess) return hip_fail(e, "level totals kernel launch");
        return GRAIL_OK;
    }
    if (frames > 0xFFFFFFFFull || (uint64_t)r.n * frames > (1ull << 32))
        return fail(GRAIL_ERR_INVALID_ARG, std::string(who) + ": more than 2^32 frames");
    const size_t cells = (size_t)r.n * (size_t)frames;
    if ((rc = st->d_fsum.reserve(ctx->stream, cells))) return rc;
    if ((rc = st->d_fpeak.reserve(ctx->stream, cells))) return rc;
    if ((rc = st->d_fbad.reserve(ctx->stream, cells))) return rc;
    hipError_t e = launch_level_frames(r.dev, r.stride, r.len, r.n, GRAIL_LEVEL_FRAME, (uint32_t)frames, st->d_fsum.get(),
                                       st->d_fpeak.get(), st->d_fbad.get(), frames, ctx->stream);
    if (e != hipSuccess) return hip_fail(e, "level frames kernel launch");
    e = launch_level_totals(r.len, r.stride, r.n, GRAIL_LEVEL_FRAME, st->d_fsum.get(), st->d_fpeak.get(), st->d_fbad.get(),
                            frames, sumsq_dev, peak_dev, nonfinite_dev, ctx->stream);
    if (e != hipSuccess) return hip_fail(e, "level totals kernel launch");
    return GRAIL_OK;
}

// hop sums, gated mean squares and non-finite counts (any output may be NULL; hops_dev NULL = the context's scratch);
// segmented: every hop from a zero state GRAIL_LOUDNESS_WARMUP_HOPS hops before it, one lane per hop
int loudness(grail_ctx *ctx, const char *who, bool segmented, const Rows &r, uint32_t sample_rate, const double *coef,
             double *gated_dev, double *hops_dev, uint64_t hops_stride, uint32_t *nonfinite_dev)
{
    double own[10];
    if (!coef) {
        if (grail_kweighting(sample_rate, own)) return fail(GRAIL_ERR_INVALID_ARG, std::string(who) + ": sample rate out of range");
        coef = own;
    }
    const uint32_t hop = sample_rate / 10u;
    int rc;
    if (!hops_dev) {
        LevelState *st;
        if ((rc = state(ctx, &st))) return rc;
        hops_stride = r.stride / hop;
        if (hops_stride && (uint64_t)r.n > (1ull << 40) / hops_stride)
            return fail(GRAIL_ERR_INVALID_ARG, std::string(who) + ": more than 2^40 hops");
        if ((rc = st->d_hops.reserve(ctx->stream, (size_t)r.n * (size_t)hops_stride))) return rc;
        hops_dev = st->d_hops.get();
    }
    hipError_t e;
    if (segmented) {
        const uint64_t lanes = loudness_segment_lanes(r.stride, hop), waves = loudness_segment_waves(r.stride, hop);
        // (the one refusal the serial call does not have: the launch is one grid of a wave per 64 hops of a row)
        if (waves > LOUD_SEGMENT_WAVES_MAX || (uint64_t)r.n * waves > LOUD_SEGMENT_WAVES_MAX)
            return fail(GRAIL_ERR_INVALID_ARG, std::string(who) + ": more than 2^26 - 1 waves of 64 hops (n_rows * ceil(ceil(row_stride / H) / 64))");
        uint32_t *hop_bad = nullptr;
        if (nonfinite_dev) {
            LevelState *st;
            if ((rc = state(ctx, &st))) return rc;
            if ((rc = st->d_hbad.reserve(ctx->stream, (size_t)r.n * (size_t)lanes))) return rc;
            hop_bad = st->d_hbad.get();
        }
        e = launch_loudness_segments(r.dev, r.stride, r.len, r.n, hop, coef, hops_dev, hops_stride, hop_bad, nonfinite_dev,
                                     ctx->stream);
        if (e != hipSuccess) return hip_fail(e, "loudness segments kernel launch");
    } else {
        e = launch_loudness_hops(r.dev, r.stride, r.len, r.n, hop, coef, hops_dev, hops_stride, nonfinite_dev, ctx->stream);
        if (e != hipSuccess) return hip_fail(e, "loudness hops kernel launch");
    }
    if (gated_dev) {
        e = launch_loudness_gate(r.len, r.stride, r.n, hop, hops_dev, hops_stride, gated_dev, ctx->stream);
        if (e != hipSuccess) return hip_fail(e, "loudness gate kernel launch");
    }
    return GRAIL_OK;
}

// the checks of grail_loudness_async and grail_loudness_segmented_async, which differ in nothing but the kernel
int loudness_call(grail_ctx *ctx, const char *who, bool segmented, const Rows &r, uint32_t sample_rate, const double *coef,
                  double *gated_ms_dev, double *hop_sumsq_dev, uint64_t hops_stride, uint32_t *nonfinite_dev)
{
    int rc = bind_device(ctx, who);
    if (rc) return rc;
    if (sample_rate < GRAIL_LOUDNESS_RATE_MIN || sample_rate > GRAIL_LOUDNESS_RATE_MAX)
        return fail(GRAIL_ERR_INVALID_ARG, std::string(who) + ": sample_rate is outside 2 560 .. 1 048 576");
    if (hop_sumsq_dev && hops_stride < r.stride / (sample_rate / 10u))
        return fail(GRAIL_ERR_INVALID_ARG, std::string(who) + ": hops_stride < row_stride / (sample_rate / 10)");
    bool measure;
    if ((rc = check_rows(who, r, gated_ms_dev || hop_sumsq_dev || nonfinite_dev, &measure)) || !measure) return rc;
    return loudness(ctx, who, segmented, r, sample_rate, coef, gated_ms_dev, hop_sumsq_dev, hops_stride, nonfinite_dev);
}

// true peaks and non-finite counts (either output may be NULL) through the context's chunk scratch
int true_peak(grail_ctx *ctx, const char *who, const Rows &r, double *true_peak_dev, uint32_t *nonfinite_dev)
{
    LevelState *st;
    int rc = state(ctx, &st);
    if (rc) return rc;
    const uint64_t chunks = true_peak_grid_chunks(r.stride);
    if (chunks > 0xFFFFFFFFull || (uint64_t)r.n * chunks > (1ull << 32))
        return fail(GRAIL_ERR_INVALID_ARG, std::string(who) + ": more than 2^32 chunks");
    if (chunks) {               // (rows of no samples: +0.0, 0 from the totals alone)
        const size_t cells = (size_t)r.n * (size_t)chunks;
        if ((rc = st->d_cmax.reserve(ctx->stream, cells))) return rc;
        if ((rc = st->d_cbad.reserve(ctx->stream, cells))) return rc;
        const hipError_t e = launch_true_peak_frames(r.dev, r.stride, r.len, r.n, (uint32_t)chunks, st->d_cmax.get(),
                                                     st->d_cbad.get(), ctx->stream);
        if (e != hipSuccess) return hip_fail(e, "true peak frames kernel launch");
    }
    const hipError_t e = launch_true_peak_totals(r.len, r.stride, r.n, st->d_cmax.get(), st->d_cbad.get(), (uint32_t)chunks,
                                                 true_peak_dev, nonfinite_dev, ctx->stream);
    if (e != hipSuccess) return hip_fail(e, "true peak totals kernel launch");
    return GRAIL_OK;
}

// grail_batch_mix_leveled_limited's part of a block, first half: the rows' true peaks queued behind the level's kernels
// and their copy to tp[r.n] on the host, complete once the caller has waited for the stream (8 bytes a row more)
int queue_block_true_peaks(grail_ctx *ctx, LevelState *st, const Rows &r, double *tp)
{
    int rc;
    if ((rc = st->d_tp.reserve(ctx->stream, r.n))) return rc;
    if ((rc = true_peak(ctx, "grail_batch_mix_leveled_limited", r, st->d_tp.get(), nullptr))) return rc;
    HIP_TRY(hipMemcpyAsync(tp, st->d_tp.get(), (size_t)r.n * 8, hipMemcpyDeviceToHost, ctx->stream));
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
    LevelState *st;
    int rc = state(ctx, &st);
    if (rc) return rc;
    if (n_rows == 0 || n_items == 0) return GRAIL_OK;
    const Rows r{rows_dev, row_stride, len_dev, n_rows};
    const bool loud = mode == GRAIL_LEVEL_LOUDNESS;
    if ((rc = st->d_sumsq.reserve(ctx->stream, n_rows))) return rc;
    if ((rc = st->d_peak.reserve(ctx->stream, n_rows))) return rc;
    if ((rc = st->d_bad.reserve(ctx->stream, n_rows))) return rc;
    // the measurement: the gated mean squares in place of the sums of squares, or the totals
    const char *who = "grail_batch_mix_leveled";
    rc = loud ? loudness(ctx, who, false, r, sample_rate, nullptr, st->d_sumsq.get(), nullptr, 0, st->d_bad.get())
              : totals(ctx, who, r, st->d_sumsq.get(), st->d_peak.get(), st->d_bad.get());
    if (rc) return rc;
    std::vector<double> tp(ceiling_db ? n_rows : 0);      // with a ceiling: the rows' true peaks, brought back in the same wait
    if (ceiling_db && (rc = queue_block_true_peaks(ctx, st, r, tp.data()))) return rc;
    // what the mode reads comes back (12 bytes a row; active level: the frames' sums too), with one wait
    std::vector<double> sumsq(n_rows), level, frames;
    std::vector<float> peak(n_rows);
    std::vector<uint32_t> bad(n_rows);
    if (loud || mode == GRAIL_LEVEL_RMS)
        HIP_TRY(hipMemcpyAsync(sumsq.data(), st->d_sumsq.get(), (size_t)n_rows * 8, hipMemcpyDeviceToHost, ctx->stream));
    if (mode == GRAIL_LEVEL_PEAK)
        HIP_TRY(hipMemcpyAsync(peak.data(), st->d_peak.get(), (size_t)n_rows * 4, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipMemcpyAsync(bad.data(), st->d_bad.get(), (size_t)n_rows * 4, hipMemcpyDeviceToHost, ctx->stream));
    const uint64_t fs = ceil_div(row_stride, GRAIL_LEVEL_FRAME);
    if (mode == GRAIL_LEVEL_ACTIVE && fs) {
        frames.resize((size_t)n_rows * fs);
        HIP_TRY(hipMemcpyAsync(frames.data(), st->d_fsum.get(), frames.size() * 8, hipMemcpyDeviceToHost, ctx->stream));
    }
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    // the per-row level of the two modes that have one (the other two go by the sums and peaks themselves)
    if (loud) {
        level.resize(n_rows);
        for (uint32_t i = 0; i < n_rows; ++i) level[i] = grail_loudness_level(sumsq[i]);
    } else if (mode == GRAIL_LEVEL_ACTIVE) {
        level.assign(n_rows, 0.0);
        // (frames past a row's last were never written: grail_active_level reads ceil(len / frame) of them)
        for (uint32_t i = 0; i < n_rows && fs; ++i)
            level[i] = grail_active_level(frames.data() + (size_t)i * fs, row_len[i], GRAIL_LEVEL_FRAME,
                                          GRAIL_LEVEL_ACTIVE_FLOOR_DB);
    }
    uint32_t unleveled = 0;
    rc = grail_level_gains(mode, loud ? nullptr : sumsq.data(), loud ? nullptr : peak.data(), bad.data(), row_len, level.data(),
                           n_rows, item_rows, item_level_db, n_items, gains, &unleveled);
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
    const Rows r{rows_dev, row_stride, len_dev, n_rows};
    int rc = bind_device(ctx, "grail_levels_async");
    if (rc) return rc;
    bool measure;
    if ((rc = check_rows("grail_levels_async", r, sumsq_dev || peak_dev || nonfinite_dev, &measure)) || !measure) return rc;
    return totals(ctx, "grail_levels_async", r, sumsq_dev, peak_dev, nonfinite_dev);
}

int grail_true_peak_async(grail_ctx *ctx, const float *rows_dev, uint64_t row_stride, const uint32_t *len_dev,
                          uint32_t n_rows, double *true_peak_dev, uint32_t *nonfinite_dev)
{
    const Rows r{rows_dev, row_stride, len_dev, n_rows};
    int rc = bind_device(ctx, "grail_true_peak_async");
    if (rc) return rc;
    bool measure;
    if ((rc = check_rows("grail_true_peak_async", r, true_peak_dev || nonfinite_dev, &measure)) || !measure) return rc;
    return true_peak(ctx, "grail_true_peak_async", r, true_peak_dev, nonfinite_dev);
}

int grail_loudness_async(grail_ctx *ctx, const float *rows_dev, uint64_t row_stride, const uint32_t *len_dev,
                         uint32_t n_rows, uint32_t sample_rate, const double *coef, double *gated_ms_dev,
                         double *hop_sumsq_dev, uint64_t hops_stride, uint32_t *nonfinite_dev)
{
    return loudness_call(ctx, "grail_loudness_async", false, {rows_dev, row_stride, len_dev, n_rows}, sample_rate, coef,
                         gated_ms_dev, hop_sumsq_dev, hops_stride, nonfinite_dev);
}

int grail_loudness_segmented_async(grail_ctx *ctx, const float *rows_dev, uint64_t row_stride, const uint32_t *len_dev,
                                   uint32_t n_rows, uint32_t sample_rate, const double *coef, double *gated_ms_dev,
                                   double *hop_sumsq_dev, uint64_t hops_stride, uint32_t *nonfinite_dev)
{
    return loudness_call(ctx, "grail_loudness_segmented_async", true, {rows_dev, row_stride, len_dev, n_rows}, sample_rate,
                         coef, gated_ms_dev, hop_sumsq_dev, hops_stride, nonfinite_dev);
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
