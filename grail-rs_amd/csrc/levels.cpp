// levels.cpp — rendered rows measured on the device: grail_levels_async, grail_frame_levels_async, grail_loudness_async,
// grail_loudness_segmented_async and grail_true_peak_async, grail_limit_async, grail_resample_async, grail_fir_create / _free /
// _async, grail_filter_stream_open / _next_async / _finish_async / _close (checks, the scratch, the launches) and what
// grail_batch_mix_leveled and its _limited form (mix.cpp) need per block.  The kernels are level_kernels.hip, loudness_kernels.hip,
// loudness_segment_kernels.hip, true_peak_kernels.hip, limiter_kernels.hip, resample_kernels.hip and fir_kernels.hip, the gains are level_gains.cpp,
// the resampler's ratio and table resample_plan.cpp and a filter set's checks and image fir_plan.cpp (pure host).
// DESIGN.md §4.9, §4.10, §4.11, §4.12, §4.13, §4.14, §4.15.
#include "api_internal.hpp"

using namespace grail;
using namespace grail::host;

// Per context (grail_ctx::level_state), kept from call to call and only ever grown (DeviceBuffer::reserve, to the exact
// size), freed by grail_destroy: the per-frame numbers that a totals call folds (16 B per frame of 4096 samples: 0.1 % of
// the rows), one block's totals for the leveled mix, the hop sums of a loudness call that does not ask for them (8 B per
// hop of 100 ms), the chunk maxima and counts that a true-peak call folds (12 B per chunk of 4096 output times) with one
// block's true peaks for the limited mix, the chunk numbers that a limiter call folds (16 B per group and chunk of 4096
// samples), the hops' non-finite counts that a segmented loudness call folds (4 B per hop), the chunks' non-finite counts
// that a resampling call folds (4 B per chunk of 1024 outputs), the resampler's tables of the last few pairs of rates,
// the same counts of a filtering call (4 B per chunk of 2048 outputs), the filter sets the caller has created and the
// filter streams open on them (each with its rows' state: a ring of samples and one word per row).
struct ResampleTable {
    uint32_t up = 0, down = 0;              // 0: the slot holds no table
    uint64_t used = 0;                      // the call that last asked for it (the oldest is evicted)
    std::vector<int32_t> host;              // (kept while the upload may be in flight)
    DeviceBuffer<int32_t> dev;              // [up][taps]
};

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
    DeviceBuffer<unsigned char> d_lstat;    // limiter chunks
    DeviceBuffer<uint32_t> d_hbad;          // segmented loudness: non-finite counts per hop
    DeviceBuffer<uint32_t> d_rbad;          // resampler chunks: non-finite counts
    ResampleTable tables[4];
    uint64_t table_calls = 0;
    DeviceBuffer<uint32_t> d_firbad;        // FIR chunks: non-finite counts
    std::vector<std::unique_ptr<grail_fir>> firs;   // the filter sets alive
    std::vector<std::unique_ptr<grail_filter_stream>> fir_streams;   // ... and the filter streams open on them
};

namespace {

// rows on the device as every measurement takes them: n rows at `stride`, row r of len[r] samples
struct Rows {
    const float *dev;
    uint64_t stride;
    const uint32_t *len;
    uint32_t n;
};

// a context, or why there is none: the device entry points say GRAIL_ERR_NO_DEVICE on a machine without a GPU
int bind_device(grail_ctx *ctx, const char *who)
{
    if (ctx) return bind(ctx);
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n < 1)
        return fail(GRAIL_ERR_NO_DEVICE, std::string(who) + ": no usable HIP device (there is no CPU fallback)");
    return fail(GRAIL_ERR_INVALID_ARG, std::string(who) + ": ctx is NULL");
}

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

LevelState *state(grail_ctx *ctx)
{
    if (!ctx->level_state) ctx->level_state.reset(new (std::nothrow) LevelState());
    return static_cast<LevelState *>(ctx->level_state.get());
}

uint64_t ceil_div(uint64_t a, uint64_t b) { return a / b + (a % b != 0); }

// the rows' totals with frames of GRAIL_LEVEL_FRAME through the context's frame scratch (which then holds the frames'
// numbers at stride ceil(row_stride / GRAIL_LEVEL_FRAME) until the context's next measurement)
int totals(grail_ctx *ctx, const char *who, const Rows &r, double *sumsq_dev, float *peak_dev, uint32_t *nonfinite_dev)
{
    LevelState *st = state(ctx);
    if (!st) return fail(GRAIL_ERR_OUT_OF_MEMORY, "level state");
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
    int rc;
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
        LevelState *st = state(ctx);
        if (!st) return fail(GRAIL_ERR_OUT_OF_MEMORY, "level state");
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
            LevelState *st = state(ctx);
            if (!st) return fail(GRAIL_ERR_OUT_OF_MEMORY, "level state");
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
    LevelState *st = state(ctx);
    if (!st) return fail(GRAIL_ERR_OUT_OF_MEMORY, "level state");
    const uint64_t chunks = true_peak_grid_chunks(r.stride);
    if (chunks > 0xFFFFFFFFull || (uint64_t)r.n * chunks > (1ull << 32))
        return fail(GRAIL_ERR_INVALID_ARG, std::string(who) + ": more than 2^32 chunks");
    if (chunks) {               // (rows of no samples: +0.0, 0 from the totals alone)
        const size_t cells = (size_t)r.n * (size_t)chunks;
        int rc;
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

// the table of a pair of rates on the device: uploaded once per (U, D), the last four kept, the oldest evicted once
// everything queued on the stream is through (a kernel still queued may be reading it)
int resample_table(grail_ctx *ctx, LevelState *st, uint32_t rate_in, uint32_t rate_out, uint32_t U, uint32_t D, uint32_t P,
                   const int32_t **table)
{
    ResampleTable *slot = &st->tables[0];
    ++st->table_calls;
    for (ResampleTable &t : st->tables) {
        if (t.dev.get() && t.up == U && t.down == D) {
            t.used = st->table_calls;
            *table = t.dev.get();
            return GRAIL_OK;
        }
        if (t.used < slot->used) slot = &t;
    }
    if (slot->dev.get()) HIP_TRY(hipStreamSynchronize(ctx->stream));
    slot->dev.reset();
    slot->up = slot->down = 0;              // (a failure below leaves the slot empty, not half-written under its old name)
    slot->host.assign((size_t)U * P, 0);
    if (grail_resample_coefficients(rate_in, rate_out, slot->host.data(), U * P))
        return fail(GRAIL_ERR_INVALID_ARG, "grail_resample_async: no table for this pair of rates");
    HIP_TRY(upload(slot->dev, slot->host.data(), slot->host.size(), ctx->stream));
    slot->up = U, slot->down = D, slot->used = st->table_calls;
    *table = slot->dev.get();
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
    const Rows r{rows_dev, row_stride, len_dev, n_rows};
    const bool loud = mode == GRAIL_LEVEL_LOUDNESS;
    int rc;
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
        if ((rc = st->d_lstat.reserve(ctx->stream, (size_t)n_groups * (size_t)chunks * limit_chunk_bytes()))) return rc;
        const hipError_t e = launch_limit_frames(rows_dev, row_stride, len_dev, n_groups, group, ceiling, lookahead_log2,
                                                 (uint32_t)chunks, out_dev, out_stride, st->d_lstat.get(), ctx->stream);
        if (e != hipSuccess) return hip_fail(e, "limiter frames kernel launch");
    }
    if (!min_gain_dev && !n_limited_dev && !nonfinite_dev) return GRAIL_OK;
    const hipError_t e = launch_limit_totals(len_dev, row_stride, n_groups, group, lookahead_log2, st->d_lstat.get(),
                                             (uint32_t)chunks, min_gain_dev, n_limited_dev, nonfinite_dev, ctx->stream);
    if (e != hipSuccess) return hip_fail(e, "limiter totals kernel launch");
    return GRAIL_OK;
}

int grail_resample_async(grail_ctx *ctx, const float *rows_dev, uint64_t row_stride, const uint32_t *len_dev, uint32_t n_rows,
                         uint32_t rate_in, uint32_t rate_out, float *out_dev, uint64_t out_stride, uint32_t *out_len_dev,
                         uint32_t *nonfinite_dev)
{
    // (what is wrong with the arguments is said before what is wrong with the machine)
    uint32_t U, D, P;
    if (grail_resample_ratio(rate_in, rate_out, &U, &D, &P))
        return fail(GRAIL_ERR_INVALID_ARG, "grail_resample_async: the rates are equal, 0, or need more than 32 768 table entries");
    if (n_rows && (!len_dev || (row_stride && (!rows_dev || (out_stride && !out_dev)))))
        return fail(GRAIL_ERR_INVALID_ARG, "grail_resample_async: NULL buffer");
    if (n_rows && row_stride) {
        if (row_stride > (1ull << 60) / n_rows || out_stride > (1ull << 60) / n_rows)
            return fail(GRAIL_ERR_INVALID_ARG, "grail_resample_async: the rows span more than 2^60 samples");
        const uintptr_t in0 = (uintptr_t)rows_dev, in1 = in0 + (uintptr_t)(n_rows * row_stride * 4u);
        const uintptr_t out0 = (uintptr_t)out_dev, out1 = out0 + (uintptr_t)(n_rows * out_stride * 4u);
        if (out_stride && in0 < out1 && out0 < in1)
            return fail(GRAIL_ERR_INVALID_ARG, "grail_resample_async: out_dev overlaps rows_dev (a chunk reads what another would have written)");
        // (a row holds fewer than 2^32 samples: len is 32 bits wide)
        const uint64_t longest = (std::min<uint64_t>(row_stride, 0xFFFFFFFFull) * U + (D - 1u)) / D;
        if (std::min(longest, out_stride) > 0xFFFFFFFFull)
            return fail(GRAIL_ERR_INVALID_ARG, "grail_resample_async: a row could hold 2^32 output samples or more (out_len is 32 bits wide)");
    }
    int rc = bind_device(ctx, "grail_resample_async");
    if (rc) return rc;
    if (n_rows == 0) return GRAIL_OK;
    LevelState *st = state(ctx);
    if (!st) return fail(GRAIL_ERR_OUT_OF_MEMORY, "level state");
    const uint64_t chunks = resample_grid_chunks(row_stride, out_stride, U, D);
    if ((uint64_t)n_rows * chunks > 0x7FFFFFFFull) return fail(GRAIL_ERR_INVALID_ARG, "grail_resample_async: more than 2^31 chunks");
    if (chunks) {               // (rows of no samples: 0, 0 from the totals alone)
        const int32_t *table = nullptr;
        if ((rc = resample_table(ctx, st, rate_in, rate_out, U, D, P, &table))) return rc;
        if ((rc = st->d_rbad.reserve(ctx->stream, (size_t)n_rows * (size_t)chunks))) return rc;
        const hipError_t e = launch_resample(rows_dev, row_stride, len_dev, n_rows, U, D, P, table, (uint32_t)chunks, out_dev,
                                             out_stride, st->d_rbad.get(), ctx->stream);
        if (e != hipSuccess) return hip_fail(e, "resample kernel launch");
    }
    if (!out_len_dev && !nonfinite_dev) return GRAIL_OK;
    const hipError_t e = launch_resample_totals(len_dev, row_stride, n_rows, U, D, out_stride, st->d_rbad.get(), (uint32_t)chunks,
                                                out_len_dev, nonfinite_dev, ctx->stream);
    if (e != hipSuccess) return hip_fail(e, "resample totals kernel launch");
    return GRAIL_OK;
}

int grail_fir_create(grail_ctx *ctx, const float *taps, const uint32_t *n_taps, const uint32_t *origin, uint32_t n_filters,
                     grail_fir **out)
{
    // (what is wrong with the arguments is said before what is wrong with the machine)
    if (!out) return fail(GRAIL_ERR_INVALID_ARG, "grail_fir_create: NULL argument");
    if (const char *why = fir_set_error(taps, n_taps, origin, n_filters))
        return fail(GRAIL_ERR_INVALID_ARG, std::string("grail_fir_create: ") + why);
    int rc = bind_device(ctx, "grail_fir_create");
    if (rc) return rc;
    LevelState *st = state(ctx);
    if (!st) return fail(GRAIL_ERR_OUT_OF_MEMORY, "level state");
    std::unique_ptr<grail_fir> set(new (std::nothrow) grail_fir());
    if (!set) return fail(GRAIL_ERR_OUT_OF_MEMORY, "filter set");
    set->n_filters = n_filters;
    for (uint32_t f = 0; f < n_filters; ++f) set->taps_max = std::max(set->taps_max, n_taps[f]);
    fir_set_image(taps, n_taps, origin, n_filters, set->image, set->desc, &set->tail_max);
    HIP_TRY(upload(set->d_taps, set->image.data(), set->image.size(), ctx->stream));
    HIP_TRY(upload(set->d_desc, set->desc.data(), set->desc.size(), ctx->stream));
    *out = set.get();
    st->firs.push_back(std::move(set));
    return GRAIL_OK;
}

int grail_fir_free(grail_ctx *ctx, grail_fir *set)
{
    if (!set) return GRAIL_OK;
    if (!ctx) return fail(GRAIL_ERR_INVALID_ARG, "grail_fir_free: ctx is NULL");
    LevelState *st = static_cast<LevelState *>(ctx->level_state.get());
    if (st) {
        for (auto it = st->firs.begin(); it != st->firs.end(); ++it) {
            if (it->get() != set) continue;
            for (const auto &fs : st->fir_streams)
                if (fs->set == set) return fail(GRAIL_ERR_INVALID_ARG, "grail_fir_free: the set still has open filter streams");
            // (a kernel or the upload still queued may be reading it)
            int rc = bind(ctx);
            if (rc) return rc;
            HIP_TRY(hipStreamSynchronize(ctx->stream));
            st->firs.erase(it);
            return GRAIL_OK;
        }
    }
    return fail(GRAIL_ERR_INVALID_ARG, "grail_fir_free: not a filter set of this context");
}

int grail_fir_async(grail_ctx *ctx, const grail_fir *set, const float *rows_dev, uint64_t row_stride, const uint32_t *len_dev,
                    uint32_t n_rows, const uint32_t *filter_dev, float *out_dev, uint64_t out_stride, uint32_t *out_len_dev,
                    uint32_t *nonfinite_dev)
{
    // (what is wrong with the arguments is said before what is wrong with the machine)
    if (!set) return fail(GRAIL_ERR_INVALID_ARG, "grail_fir_async: set is NULL");
    if (ctx) {          // (sets are looked up, not looked into: a stale pointer is refused, not read)
        const LevelState *own = static_cast<const LevelState *>(ctx->level_state.get());
        bool found = false;
        if (own)
            for (const auto &s : own->firs) found = found || s.get() == set;
        if (!found) return fail(GRAIL_ERR_INVALID_ARG, "grail_fir_async: not a filter set of this context");
    }
    if (n_rows && (!len_dev || (row_stride && (!rows_dev || (out_stride && !out_dev)))))
        return fail(GRAIL_ERR_INVALID_ARG, "grail_fir_async: NULL buffer");
    // (without a context the set was not looked up and is not looked into: the checks below run with a tail of 0, and the
    // call ends at bind_device)
    const uint32_t tail_max = ctx ? set->tail_max : 0u;
    uint64_t chunks = 0;
    if (n_rows && row_stride) {
        if (row_stride > (1ull << 60) / n_rows || out_stride > (1ull << 60) / n_rows)
            return fail(GRAIL_ERR_INVALID_ARG, "grail_fir_async: the rows span more than 2^60 samples");
        const uintptr_t in0 = (uintptr_t)rows_dev, in1 = in0 + (uintptr_t)(n_rows * row_stride * 4u);
        const uintptr_t out0 = (uintptr_t)out_dev, out1 = out0 + (uintptr_t)(n_rows * out_stride * 4u);
        if (out_stride && in0 < out1 && out0 < in1)
            return fail(GRAIL_ERR_INVALID_ARG, "grail_fir_async: out_dev overlaps rows_dev (a chunk reads what another would have written)");
        // (a row holds fewer than 2^32 samples: len is 32 bits wide)
        const uint64_t longest = std::min<uint64_t>(row_stride, 0xFFFFFFFFull) + tail_max;
        if (std::min(longest, out_stride) > 0xFFFFFFFFull)
            return fail(GRAIL_ERR_INVALID_ARG, "grail_fir_async: a row could hold 2^32 output samples or more (out_len is 32 bits wide)");
        chunks = fir_grid_chunks(row_stride, out_stride, tail_max);
        if ((uint64_t)n_rows * chunks > 0x7FFFFFFFull) return fail(GRAIL_ERR_INVALID_ARG, "grail_fir_async: more than 2^31 chunks");
    }
    int rc = bind_device(ctx, "grail_fir_async");
    if (rc) return rc;
    if (n_rows == 0) return GRAIL_OK;
    LevelState *st = state(ctx);
    if (!st) return fail(GRAIL_ERR_OUT_OF_MEMORY, "level state");
    if (chunks) {               // (rows of no samples: 0, 0 from the totals alone)
        if ((rc = st->d_firbad.reserve(ctx->stream, (size_t)n_rows * (size_t)chunks))) return rc;
        const hipError_t e = launch_fir(rows_dev, row_stride, len_dev, n_rows, filter_dev, set->d_taps.get(), set->d_desc.get(),
                                        set->n_filters, (uint32_t)chunks, out_dev, out_stride, st->d_firbad.get(), ctx->stream);
        if (e != hipSuccess) return hip_fail(e, "fir kernel launch");
    }
    if (!out_len_dev && !nonfinite_dev) return GRAIL_OK;
    const hipError_t e = launch_fir_totals(len_dev, row_stride, n_rows, filter_dev, set->d_desc.get(), set->n_filters, out_stride,
                                           st->d_firbad.get(), (uint32_t)chunks, out_len_dev, nonfinite_dev, ctx->stream);
    if (e != hipSuccess) return hip_fail(e, "fir totals kernel launch");
    return GRAIL_OK;
}

namespace {

// streams are looked up, not looked into: a stale pointer or another context's is refused, not read
grail_filter_stream *find_fir_stream(grail_ctx *ctx, const grail_filter_stream *fs)
{
    const LevelState *own = static_cast<const LevelState *>(ctx->level_state.get());
    if (own)
        for (const auto &s : own->fir_streams)
            if (s.get() == fs) return s.get();
    return nullptr;
}

// the two kernels of a call on a stream: the outputs (chunks = 0: there are none to write), then the state
int fir_stream_call(grail_ctx *ctx, grail_filter_stream *fs, const float *in_dev, uint64_t in_stride,
                    const uint32_t *in_len_dev, const uint8_t *mark_dev, bool finishing, uint64_t chunks, float *out_dev,
                    uint64_t out_stride, uint32_t *out_len_dev, uint32_t *nonfinite_dev)
{
    LevelState *st = state(ctx);
    if (!st) return fail(GRAIL_ERR_OUT_OF_MEMORY, "level state");
    const grail_fir *set = fs->set;
    if (chunks) {
        int rc;
        if ((rc = st->d_firbad.reserve(ctx->stream, (size_t)fs->n_rows * (size_t)chunks))) return rc;
        const hipError_t e = launch_fir_stream(in_dev, in_stride, in_len_dev, fs->n_rows, fs->d_filter.get(), set->d_taps.get(),
                                               set->d_desc.get(), set->n_filters, fs->d_state.get(), fs->d_ring.get(), fs->ring_cap,
                                               mark_dev, finishing, (uint32_t)chunks, out_dev, out_stride, st->d_firbad.get(),
                                               ctx->stream);
        if (e != hipSuccess) return hip_fail(e, "fir stream kernel launch");
    }
    const hipError_t e = launch_fir_stream_advance(in_dev, in_stride, in_len_dev, fs->n_rows, fs->d_filter.get(), set->d_desc.get(),
                                                   set->n_filters, fs->d_state.get(), fs->d_ring.get(), fs->ring_cap, mark_dev, finishing,
                                                   st->d_firbad.get(), (uint32_t)chunks, out_len_dev, nonfinite_dev, ctx->stream);
    if (e != hipSuccess) return hip_fail(e, "fir stream advance kernel launch");
    return GRAIL_OK;
}

}  // namespace

int grail_filter_stream_open(grail_ctx *ctx, const grail_fir *set, uint32_t n_rows, const uint32_t *filter, grail_filter_stream **out)
{
    // (what is wrong with the arguments is said before what is wrong with the machine; no context exists without a device)
    if (!ctx || !out) return fail(GRAIL_ERR_INVALID_ARG, "grail_filter_stream_open: NULL argument");
    bool found = false;
    if (const LevelState *own = static_cast<const LevelState *>(ctx->level_state.get()))
        for (const auto &s : own->firs) found = found || s.get() == set;
    if (!found) return fail(GRAIL_ERR_INVALID_ARG, "grail_filter_stream_open: not a filter set of this context");
    if (const char *why = fir_stream_open_error(filter, n_rows, set->n_filters))
        return fail(GRAIL_ERR_INVALID_ARG, std::string("grail_filter_stream_open: ") + why);
    int rc = bind(ctx);
    if (rc) return rc;
    LevelState *st = state(ctx);
    std::unique_ptr<grail_filter_stream> fs(new (std::nothrow) grail_filter_stream());
    if (!fs) return fail(GRAIL_ERR_OUT_OF_MEMORY, "filter stream");
    fs->set = set;
    fs->n_rows = n_rows;
    fs->ring_cap = fir_stream_ring_capacity(set->taps_max);
    fs->filter.assign(n_rows, 0u);
    if (filter) std::copy(filter, filter + n_rows, fs->filter.begin());
    HIP_TRY(upload(fs->d_filter, fs->filter.data(), n_rows, ctx->stream));
    HIP_TRY(fs->d_state.alloc(n_rows));
    HIP_TRY(fs->d_ring.alloc((size_t)n_rows * fs->ring_cap));
    HIP_TRY(fs->d_mark.alloc(n_rows));
    // no sample fed, no row ended; the ring is never read before it is written, zeroed all the same
    HIP_TRY(hipMemsetAsync(fs->d_state.get(), 0, (size_t)n_rows * sizeof(uint64_t), ctx->stream));
    HIP_TRY(hipMemsetAsync(fs->d_ring.get(), 0, (size_t)n_rows * fs->ring_cap * sizeof(float), ctx->stream));
    *out = fs.get();
    st->fir_streams.push_back(std::move(fs));
    return GRAIL_OK;
}

int grail_filter_stream_close(grail_ctx *ctx, grail_filter_stream *fs)
{
    if (!fs) return GRAIL_OK;
    if (!ctx) return fail(GRAIL_ERR_INVALID_ARG, "grail_filter_stream_close: ctx is NULL");
    LevelState *st = static_cast<LevelState *>(ctx->level_state.get());
    if (st) {
        for (auto it = st->fir_streams.begin(); it != st->fir_streams.end(); ++it) {
            if (it->get() != fs) continue;
            // (a kernel or an upload still queued may be using its state)
            int rc = bind(ctx);
            if (rc) return rc;
            HIP_TRY(hipStreamSynchronize(ctx->stream));
            st->fir_streams.erase(it);
            return GRAIL_OK;
        }
    }
    return fail(GRAIL_ERR_INVALID_ARG, "grail_filter_stream_close: not an open filter stream of this context");
}

int grail_filter_stream_next_async(grail_ctx *ctx, grail_filter_stream *fs, const float *in_dev, uint64_t in_stride,
                                   const uint32_t *in_len_dev, float *out_dev, uint64_t out_stride, uint32_t *out_len_dev,
                                   uint32_t *nonfinite_dev)
{
    // (what is wrong with the arguments is said before what is wrong with the machine)
    if (!fs) return fail(GRAIL_ERR_INVALID_ARG, "grail_filter_stream_next_async: the stream is NULL");
    if (ctx && !find_fir_stream(ctx, fs))
        return fail(GRAIL_ERR_INVALID_ARG, "grail_filter_stream_next_async: not an open filter stream of this context");
    // (without a context the stream was not looked up and is not looked into: the checks run for one row, and the call ends
    // at bind_device)
    uint64_t chunks = 0;
    if (const char *why = fir_stream_next_error(in_dev, in_stride, in_len_dev, ctx ? fs->n_rows : 1u, out_dev, out_stride, &chunks))
        return fail(GRAIL_ERR_INVALID_ARG, std::string("grail_filter_stream_next_async: ") + why);
    int rc = bind_device(ctx, "grail_filter_stream_next_async");
    if (rc) return rc;
    return fir_stream_call(ctx, fs, in_dev, in_stride, in_len_dev, nullptr, false, chunks, out_dev,
                           out_stride, out_len_dev, nonfinite_dev);
}

int grail_filter_stream_finish_async(grail_ctx *ctx, grail_filter_stream *fs, const uint8_t *which, float *out_dev,
                                     uint64_t out_stride, uint32_t *out_len_dev)
{
    if (!fs) return fail(GRAIL_ERR_INVALID_ARG, "grail_filter_stream_finish_async: the stream is NULL");
    if (ctx && !find_fir_stream(ctx, fs))
        return fail(GRAIL_ERR_INVALID_ARG, "grail_filter_stream_finish_async: not an open filter stream of this context");
    // (without a context: the checks of a set of one tap, and the call ends at bind_device)
    uint64_t chunks = 0;
    if (const char *why = fir_stream_finish_error(out_dev, out_stride, ctx ? fs->n_rows : 1u, ctx ? fs->set->taps_max : 1u, &chunks))
        return fail(GRAIL_ERR_INVALID_ARG, std::string("grail_filter_stream_finish_async: ") + why);
    int rc = bind_device(ctx, "grail_filter_stream_finish_async");
    if (rc) return rc;
    const uint8_t *mark_dev = nullptr;
    if (which) {
        // (the upload of the call before may still be reading the host copy)
        if (fs->ev_mark.get())
            HIP_TRY(hipEventSynchronize(fs->ev_mark));
        else
            HIP_TRY(fs->ev_mark.create());
        fs->mark.assign(which, which + fs->n_rows);
        HIP_TRY(hipMemcpyAsync(fs->d_mark.get(), fs->mark.data(), fs->n_rows, hipMemcpyHostToDevice, ctx->stream));
        HIP_TRY(hipEventRecord(fs->ev_mark, ctx->stream));
        mark_dev = fs->d_mark.get();
    }
    return fir_stream_call(ctx, fs, nullptr, 0, nullptr, mark_dev, true, chunks, out_dev, out_stride,
                           out_len_dev, nullptr);
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
