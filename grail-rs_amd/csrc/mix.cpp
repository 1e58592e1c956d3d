// mix.cpp — rendered rows -> tracks on the device: grail_mix_async (checks, the plan's upload, one launch), grail_batch_mix
// (a batch rendered in blocks of rows into scratch, each block mixed before the next one renders) and
// grail_pcm16_frames_async.  The plan is mix_plan.cpp (pure host), the kernels are mix_kernels.hip.  DESIGN.md §4.8.
#include "api_internal.hpp"
#include "mix_plan.h"

using namespace grail;
using namespace grail::host;

// Per context (grail_ctx::mix_state): the plan of the last mix and the device buffers it went to, and grail_batch_mix's
// scratch (one block of rows and their lengths) — kept from call to call and only ever grown (DeviceBuffer::reserve), so
// that a mix in steady state allocates nothing on the device (allocating and freeing a 25 GB block costs a third of a
// render, and varies from call to call).  The plan's buffers grow by a quarter more than asked for, so that slowly growing
// plans do not reallocate every call; the block's to the exact size.  The host vectors of the plan are rebuilt only once
// the upload from them has completed.
struct MixState : CtxPart {
    mix::Plan plan;
    DeviceBuffer<mix::MixItem> d_items;
    DeviceBuffer<uint32_t> d_tile_start, d_tile_items;
    DeviceBuffer<float> d_rows;       // grail_batch_mix: rows of one block
    DeviceBuffer<uint32_t> d_len;     // ... and their lengths
    Event uploaded;
    bool pending = false;
};

namespace {

// the context's, made at first use (nullptr: no host memory)
MixState *state(grail_ctx *ctx)
{
    if (!ctx->mix_state) ctx->mix_state.reset(new (std::nothrow) MixState());
    return static_cast<MixState *>(ctx->mix_state.get());
}

size_t quarter_more(size_t n) { return n + n / 4; }

// grail_mix_async after bind(): the checks, the plan, its upload, the launch
int mix_rows(grail_ctx *ctx, const char *who, const float *rows_dev, uint64_t row_stride, const uint32_t *row_len,
             uint32_t n_rows, const uint32_t *item_rows, const uint32_t *item_tracks, const uint64_t *item_offsets,
             const float *item_gains, uint32_t n_items, float *tracks_dev, uint64_t track_stride, uint32_t n_tracks,
             uint64_t track_len, uint32_t flags)
{
    if (flags & ~GRAIL_MIX_ACCUMULATE) return fail(GRAIL_ERR_INVALID_ARG, std::string(who) + ": unknown flags");
    if (n_items && !rows_dev) return fail(GRAIL_ERR_INVALID_ARG, std::string(who) + ": rows_dev is NULL");
    if (n_tracks && !tracks_dev) return fail(GRAIL_ERR_INVALID_ARG, std::string(who) + ": tracks_dev is NULL");
    MixState *st = state(ctx);
    if (!st) return fail(GRAIL_ERR_OUT_OF_MEMORY, "mix state");
    if (!st->uploaded) HIP_TRY(st->uploaded.create());
    if (st->pending) {
        HIP_TRY(hipEventSynchronize(st->uploaded));
        st->pending = false;
    }
    std::string why;
    const int rc = mix::build_plan(row_len, n_rows, row_stride, item_rows, item_tracks, item_offsets, item_gains, n_items,
                                   n_tracks, track_len, track_stride, (uint32_t)ctx->cus, st->plan, &why);
    if (rc) return fail(rc, std::string(who) + ": " + why);
    const mix::Plan &p = st->plan;
    const uint64_t wgs = (uint64_t)n_tracks * p.wgs_per_track;
    if (wgs == 0) return GRAIL_OK;
    int r;
    if ((r = st->d_items.reserve(ctx->stream, p.items.size(), quarter_more(p.items.size())))) return r;
    if ((r = st->d_tile_start.reserve(ctx->stream, p.tile_start.size(), quarter_more(p.tile_start.size())))) return r;
    if ((r = st->d_tile_items.reserve(ctx->stream, p.tile_items.size(), quarter_more(p.tile_items.size())))) return r;
    if (!p.items.empty())
        HIP_TRY(hipMemcpyAsync(st->d_items.get(), p.items.data(), p.items.size() * sizeof(mix::MixItem), hipMemcpyHostToDevice,
                               ctx->stream));
    HIP_TRY(hipMemcpyAsync(st->d_tile_start.get(), p.tile_start.data(), p.tile_start.size() * sizeof(uint32_t),
                           hipMemcpyHostToDevice, ctx->stream));
    if (!p.tile_items.empty())
        HIP_TRY(hipMemcpyAsync(st->d_tile_items.get(), p.tile_items.data(), p.tile_items.size() * sizeof(uint32_t),
                               hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(hipEventRecord(st->uploaded, ctx->stream));
    st->pending = true;
    MixArgs a{};
    a.rows = rows_dev;
    a.items = st->d_items.get();
    a.tile_start = st->d_tile_start.get();
    a.tile_items = st->d_tile_items.get();
    a.tracks = tracks_dev;
    a.track_stride = track_stride;
    a.track_len = track_len;
    a.wg_samples = p.wg_samples;
    a.wgs_per_track = (uint32_t)p.wgs_per_track;
    a.wgs_per_tile = (uint32_t)(p.tile_samples / p.wg_samples);
    a.tiles_per_track = (uint32_t)p.tiles_per_track;
    a.n_workgroups = (uint32_t)wgs;
    a.samples_per_lane = p.samples_per_lane;
    a.accumulate = flags & GRAIL_MIX_ACCUMULATE;
    const hipError_t e = launch_mix(a, ctx->stream);
    if (e != hipSuccess) return hip_fail(e, "mix kernel launch");
    return GRAIL_OK;
}

// grail_batch_mix after bind(), and grail_batch_mix_leveled: with item_level_db the gains are not given but derived per
// block, between its rendering and its mix, from the block's measured rows (levels.cpp: one small copy and one wait per
// block); they are returned through gains_out / n_unleveled once everything has succeeded.  With ceiling_db
// (grail_batch_mix_leveled_limited) each block's true peaks are measured too and cap its gains; n_limited as n_unleveled.
int batch_mix(grail_ctx *ctx, const char *who, const grail_batch *batch, const uint32_t *item_rows,
              const uint32_t *item_tracks, const uint64_t *item_offsets, const float *item_gains,
              const float *item_level_db, int mode, uint32_t n_items, float *tracks_dev, uint64_t track_stride,
              uint32_t n_tracks, uint64_t track_len, uint32_t *out_len, float *gains_out, uint32_t *n_unleveled,
              const float *ceiling_db, uint32_t *n_limited, uint32_t flags)
{
    int rc;
    if ((rc = check_ready(ctx, batch))) return rc;
    const bool leveled = item_level_db != nullptr;
    uint32_t level_rate = 0;
    if (leveled && mode == GRAIL_LEVEL_LOUDNESS && !(level_rate = level_table_rate(ctx)))
        return fail(GRAIL_ERR_INVALID_ARG, std::string(who) + ": GRAIL_LEVEL_LOUDNESS needs voices of one whole-numbered "
                                                              "sample rate within 2 560 .. 1 048 576");
    std::vector<float> level_gains(leveled ? n_items : 0);
    uint32_t unleveled = 0, limited = 0;
    const uint32_t n = batch->n_utt;
    // the items' checks before anything is rendered (the plan repeats them per block, with the rows' lengths)
    if (n_items && (!item_rows || !item_offsets)) return fail(GRAIL_ERR_INVALID_ARG, std::string(who) + ": item_rows or item_offsets is NULL");
    if (n_tracks && !tracks_dev) return fail(GRAIL_ERR_INVALID_ARG, std::string(who) + ": tracks_dev is NULL");
    if (track_len > track_stride) return fail(GRAIL_ERR_INVALID_ARG, std::string(who) + ": track_len > track_stride");
    if (flags & ~GRAIL_MIX_ACCUMULATE) return fail(GRAIL_ERR_INVALID_ARG, std::string(who) + ": unknown flags");
    for (uint32_t i = 0; i < n_items; ++i) {
        if (item_rows[i] >= n) return fail(GRAIL_ERR_INVALID_ARG, std::string(who) + ": an item's row is >= the batch size");
        if ((item_tracks ? item_tracks[i] : 0u) >= n_tracks)
            return fail(GRAIL_ERR_INVALID_ARG, std::string(who) + ": an item's track is >= n_tracks");
    }
    if (n == 0) {           // nothing to render: the tracks as an empty mix leaves them (+0.0, or untouched)
        rc = mix_rows(ctx, who, nullptr, 0, nullptr, 0, nullptr, nullptr, nullptr, nullptr, 0, tracks_dev,
                      track_stride, n_tracks, track_len, flags);
        const int sync_rc = grail_sync(ctx);
        if (!rc && !sync_rc && leveled && n_unleveled) *n_unleveled = 0;
        if (!rc && !sync_rc && ceiling_db && n_limited) *n_limited = 0;
        return rc ? rc : sync_rc;
    }
    std::vector<uint32_t> lens(n);
    if ((rc = grail_batch_lengths(ctx, batch, 0xFFFFFFFFu, lens.data()))) return rc;
    const uint64_t longest = *std::max_element(lens.begin(), lens.end());
    const uint64_t stride = std::max<uint64_t>(64, (longest + 63) / 64 * 64);
    MixState *st = state(ctx);
    if (!st) return fail(GRAIL_ERR_OUT_OF_MEMORY, "mix state");
    // the block rule of the header: 2 x 256 x CUs rows, as many as half of the free HBM holds (the context's scratch from an
    // earlier call counts as free: it is this call's to reuse)
    uint64_t block = 2ull * 256ull * (uint64_t)std::max(ctx->cus, 1);
    size_t free_bytes = 0, total_bytes = 0;
    HIP_TRY(hipMemGetInfo(&free_bytes, &total_bytes));
    const uint64_t fit = (uint64_t)((free_bytes + st->d_rows.capacity() * sizeof(float)) / 2) / (stride * sizeof(float));
    if (fit == 0) return fail(GRAIL_ERR_OUT_OF_MEMORY, std::string(who) + ": not one row fits in half of the free HBM");
    block = std::min(block, fit);
    const bool one_piece = n <= block;
    const uint64_t rows_alloc = one_piece ? n : block;
    const uint64_t n_blocks = one_piece ? 1 : (n + block - 1) / block;
    // the items of each block, in the order given (the plan orders them by row; blocks follow each other in row order)
    std::vector<std::vector<uint32_t>> of_block(n_blocks);
    if (!one_piece)
        for (uint32_t i = 0; i < n_items; ++i) of_block[item_rows[i] / block].push_back(i);
    if ((rc = st->d_rows.reserve(ctx->stream, rows_alloc * stride))) return rc;
    if ((rc = st->d_len.reserve(ctx->stream, rows_alloc))) return rc;
    float *const d_rows = st->d_rows.get();
    uint32_t *const d_len = st->d_len.get();
    std::vector<uint32_t> sub_rows, sub_tracks;
    std::vector<uint64_t> sub_offs;
    std::vector<float> sub_gains, sub_levels;
    for (uint64_t b = 0; !rc && b < n_blocks; ++b) {
        const uint32_t first = (uint32_t)(b * block), count = (uint32_t)std::min<uint64_t>(block, n - first);
        const uint32_t fl = b ? flags | GRAIL_MIX_ACCUMULATE : flags;
        if (one_piece) {
            rc = synthesize_rows(ctx, batch, d_rows, nullptr, stride, d_len);      // = grail_batch_synthesize_async
            if (!rc && leveled) {
                rc = level_block_gains(ctx, mode, level_rate, d_rows, stride, d_len, lens.data(), n, item_rows, item_level_db,
                                       n_items, level_gains.data(), &unleveled, ceiling_db, &limited);
                item_gains = level_gains.data();
            }
            if (!rc)
                rc = mix_rows(ctx, who, d_rows, stride, lens.data(), n, item_rows, item_tracks, item_offsets,
                              item_gains, n_items, tracks_dev, track_stride, n_tracks, track_len, fl);
            break;
        }
        if (b && of_block[b].empty()) continue;      // no item reads these rows: not rendered at all
        rc = synthesize_rows(ctx, batch, d_rows, nullptr, stride, d_len, first, count, (uint32_t)block);
        if (rc) break;
        sub_rows.clear();
        sub_tracks.clear();
        sub_offs.clear();
        sub_gains.clear();
        sub_levels.clear();
        for (const uint32_t i : of_block[b]) {
            sub_rows.push_back(item_rows[i] - first);
            if (item_tracks) sub_tracks.push_back(item_tracks[i]);
            sub_offs.push_back(item_offsets[i]);
            if (item_gains) sub_gains.push_back(item_gains[i]);
            if (leveled) sub_levels.push_back(item_level_db[i]);
        }
        if (leveled) {
            sub_gains.assign(sub_rows.size(), 0.0f);
            rc = level_block_gains(ctx, mode, level_rate, d_rows, stride, d_len, lens.data() + first, count, sub_rows.data(),
                                   sub_levels.data(), (uint32_t)sub_rows.size(), sub_gains.data(), &unleveled, ceiling_db,
                                   &limited);
            if (rc) break;
            for (size_t k = 0; k < of_block[b].size(); ++k) level_gains[of_block[b][k]] = sub_gains[k];
        }
        rc = mix_rows(ctx, who, d_rows, stride, lens.data() + first, count, sub_rows.data(),
                      item_tracks ? sub_tracks.data() : nullptr, sub_offs.data(),
                      item_gains || leveled ? sub_gains.data() : nullptr,
                      (uint32_t)sub_rows.size(), tracks_dev, track_stride, n_tracks, track_len, fl);
    }
    const int sync_rc = grail_sync(ctx);      // (every block queued; a cut row cannot happen: the stride holds the longest)
    if (rc) return rc;
    if (sync_rc) return sync_rc;
    if (out_len) std::memcpy(out_len, lens.data(), (size_t)n * sizeof(uint32_t));
    if (leveled && gains_out && n_items) std::memcpy(gains_out, level_gains.data(), (size_t)n_items * sizeof(float));
    if (leveled && n_unleveled) *n_unleveled = unleveled;
    if (ceiling_db && n_limited) *n_limited = limited;
    return GRAIL_OK;
}

// grail_batch_mix_leveled and grail_batch_mix_leveled_limited (ceiling_db: NULL = no ceiling)
int mix_leveled(const char *who, grail_ctx *ctx, const grail_batch *batch, const uint32_t *item_rows,
                const uint32_t *item_tracks, const uint64_t *item_offsets, const float *item_level_db, int mode,
                uint32_t n_items, float *tracks_dev, uint64_t track_stride, uint32_t n_tracks, uint64_t track_len,
                uint32_t *out_len, float *item_gains_out, uint32_t *n_unleveled, const float *ceiling_db,
                uint32_t *n_limited, uint32_t flags)
{
    if (!ctx) {                 // (no context can exist without a device: say which of the two it is)
        int n = 0;
        if (hipGetDeviceCount(&n) != hipSuccess || n < 1)
            return fail(GRAIL_ERR_NO_DEVICE, std::string(who) + ": no usable HIP device (there is no CPU fallback)");
    }
    int rc = bind(ctx);
    if (rc) return rc;
    if (mode != GRAIL_LEVEL_PEAK && mode != GRAIL_LEVEL_RMS && mode != GRAIL_LEVEL_ACTIVE && mode != GRAIL_LEVEL_LOUDNESS)
        return fail(GRAIL_ERR_INVALID_ARG, std::string(who) + ": unknown mode");
    if (ceiling_db && !std::isfinite(*ceiling_db)) return fail(GRAIL_ERR_INVALID_ARG, std::string(who) + ": ceiling_db is not finite");
    static const float none = 0.0f;
    if (n_items && !item_level_db) return fail(GRAIL_ERR_INVALID_ARG, std::string(who) + ": item_level_db is NULL");
    return batch_mix(ctx, who, batch, item_rows, item_tracks, item_offsets, nullptr, item_level_db ? item_level_db : &none,
                     mode, n_items, tracks_dev, track_stride, n_tracks, track_len, out_len, item_gains_out, n_unleveled,
                     ceiling_db, n_limited, flags);
}

}  // namespace

extern "C" {

int grail_mix_async(grail_ctx *ctx, const float *rows_dev, uint64_t row_stride, const uint32_t *row_len,
                    uint32_t n_rows, const uint32_t *item_rows, const uint32_t *item_tracks,
                    const uint64_t *item_offsets, const float *item_gains, uint32_t n_items,
                    float *tracks_dev, uint64_t track_stride, uint32_t n_tracks, uint64_t track_len,
                    uint32_t flags)
{
    int rc = bind(ctx);
    if (rc) return rc;
    return mix_rows(ctx, "grail_mix_async", rows_dev, row_stride, row_len, n_rows, item_rows, item_tracks, item_offsets,
                    item_gains, n_items, tracks_dev, track_stride, n_tracks, track_len, flags);
}

int grail_batch_mix(grail_ctx *ctx, const grail_batch *batch, const uint32_t *item_rows,
                    const uint32_t *item_tracks, const uint64_t *item_offsets, const float *item_gains,
                    uint32_t n_items, float *tracks_dev, uint64_t track_stride, uint32_t n_tracks,
                    uint64_t track_len, uint32_t *out_len, uint32_t flags)
{
    int rc = bind(ctx);
    if (rc) return rc;
    return batch_mix(ctx, "grail_batch_mix", batch, item_rows, item_tracks, item_offsets, item_gains, nullptr, 0, n_items,
                     tracks_dev, track_stride, n_tracks, track_len, out_len, nullptr, nullptr, nullptr, nullptr, flags);
}

int grail_batch_mix_leveled(grail_ctx *ctx, const grail_batch *batch, const uint32_t *item_rows,
                            const uint32_t *item_tracks, const uint64_t *item_offsets, const float *item_level_db,
                            int mode, uint32_t n_items, float *tracks_dev, uint64_t track_stride, uint32_t n_tracks,
                            uint64_t track_len, uint32_t *out_len, float *item_gains_out, uint32_t *n_unleveled,
                            uint32_t flags)
{
    return mix_leveled("grail_batch_mix_leveled", ctx, batch, item_rows, item_tracks, item_offsets, item_level_db, mode,
                       n_items, tracks_dev, track_stride, n_tracks, track_len, out_len, item_gains_out, n_unleveled, nullptr,
                       nullptr, flags);
}

int grail_batch_mix_leveled_limited(grail_ctx *ctx, const grail_batch *batch, const uint32_t *item_rows,
                                    const uint32_t *item_tracks, const uint64_t *item_offsets, const float *item_level_db,
                                    int mode, uint32_t n_items, float *tracks_dev, uint64_t track_stride,
                                    uint32_t n_tracks, uint64_t track_len, uint32_t *out_len, float *item_gains_out,
                                    uint32_t *n_unleveled, float ceiling_db, uint32_t *n_limited, uint32_t flags)
{
    return mix_leveled("grail_batch_mix_leveled_limited", ctx, batch, item_rows, item_tracks, item_offsets, item_level_db,
                       mode, n_items, tracks_dev, track_stride, n_tracks, track_len, out_len, item_gains_out, n_unleveled,
                       &ceiling_db, n_limited, flags);
}

int grail_pcm16_frames_async(grail_ctx *ctx, const float *tracks_dev, uint64_t track_stride,
                             uint32_t n_tracks, uint64_t n_frames, int16_t *frames_dev)
{
    int rc = bind(ctx);
    if (rc) return rc;
    if (n_frames == 0) return GRAIL_OK;
    if (n_tracks == 0) return fail(GRAIL_ERR_INVALID_ARG, "grail_pcm16_frames_async: no tracks");
    if (!tracks_dev || !frames_dev) return fail(GRAIL_ERR_INVALID_ARG, "grail_pcm16_frames_async: NULL buffer");
    if (n_frames > track_stride) return fail(GRAIL_ERR_INVALID_ARG, "grail_pcm16_frames_async: n_frames > track_stride");
    if (n_frames > UINT64_MAX / n_tracks) return fail(GRAIL_ERR_INVALID_ARG, "grail_pcm16_frames_async: too many frames");
    const hipError_t e = launch_pcm16_frames(tracks_dev, track_stride, n_tracks, n_frames, frames_dev, ctx->stream);
    if (e != hipSuccess) return hip_fail(e, "pcm16 frames kernel launch");
    return GRAIL_OK;
}

}  // extern "C"
