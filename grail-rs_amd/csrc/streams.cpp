// streams.cpp — resumable streams (the per-utterance state stays in HBM between pulls) and live streams (segments
// appended while samples are pulled: the lazy source of examples/interactive.rs:31-38).
#include "api_internal.hpp"

using namespace grail;
using namespace grail::host;

extern "C" {

int grail_stream_open(grail_ctx *ctx, const grail_batch *batch, grail_stream **out)
{
    int rc = bind(ctx);
    if (rc) return rc;
    if (!out) return fail(GRAIL_ERR_INVALID_ARG, "out is NULL");
    *out = nullptr;
    if ((rc = check_ready(ctx, batch))) return rc;
    grail_stream *s = new (std::nothrow) grail_stream();
    if (!s) return fail(GRAIL_ERR_OUT_OF_MEMORY, "host allocation failed");
    s->batch = batch;
    s->half_capable = batch_half_capable(ctx, batch);
    s->any_blend = batch->any_blend;
    s->live4 = batch_live4_any_blend(ctx, batch);      // (the lean resumable kernels exist for every blend length)
    s->voices_epoch = ctx->voices_epoch;
    s->L = ctx->opt.lanes_option ? ctx->opt.lanes_option : auto_lanes_per_utt(batch->n_utt, ctx_simds(ctx));
    if (s->live4 && !ctx->opt.lanes_option && ctx->opt.pipeline_option &&
        (int64_t)(((uint64_t)batch->n_utt + 15) / 16) <= pipe4_groups(ctx)) {
        s->L = 4;                            // the pipelined workgroups of four formants (stream_next), 16 utterances each
    } else if (s->live4) {
        if (s->L == 8) s->live4 = false;     // eight lanes per utterance need eight formants to lay out
        else if (!ctx->opt.lanes_option)         // same rule over four formants: the widest one-wave-per-SIMD mapping
            s->L = ((uint64_t)batch->n_utt * 4 + 63) / 64 <= ctx_simds(ctx) ? 4 : ((uint64_t)batch->n_utt * 2 + 63) / 64 <= ctx_simds(ctx) ? 2 : 1;
    }
    s->lanes = state_lanes(batch->n_utt, s->L);
    const hipError_t e = s->d_state.alloc((size_t)state_words(s->L) * s->lanes);
    if (e != hipSuccess) {
        delete s;
        return hip_fail(e, "stream state allocation");
    }
    *out = s;
    return GRAIL_OK;
}

// the statistics of a pull: one launch of the stream's mapping
static void record_pull(LaunchStats &st, const SynthArgs &a, int lanes)
{
    st.last_kernel = last_kernel_name();
    st.last_formants = a.live4 ? 4 : 8;
    st.last_lanes = lanes;
    st.last_pipe = a.pipe ? 1 : 0;
    st.last_fast = (int)a.fast;
    st.last_blocks = 1;
    // (last_split and last_packed stay what the last one-shot launch left: "last_launch_chunks" / "_packed" tell of those)
}

static int stream_next(grail_ctx *ctx, grail_stream *stream, uint32_t max_samples, float *out_dev,
                       int16_t *out_pcm16_dev, uint64_t out_stride, uint32_t *out_len_dev)
{
    int rc = bind(ctx);
    if (rc) return rc;
    if (!stream) return fail(GRAIL_ERR_INVALID_ARG, "stream is NULL");
    const grail_batch *batch = stream->batch;
    if ((rc = check_ready(ctx, batch))) return rc;
    if (max_samples > out_stride) return fail(GRAIL_ERR_INVALID_ARG, "max_samples exceeds out_stride");
    if (batch->n_utt == 0) return GRAIL_OK;
    if (!out_dev && !out_pcm16_dev && max_samples) return fail(GRAIL_ERR_INVALID_ARG, "out_dev is NULL");
    SynthArgs a{};
    batch_args(ctx, batch, 0u, a);
    a.ring_cap = stream->ring_cap;
    a.seg_counts = stream->d_counts.get();
    a.seg_open = stream->d_open.get();
    a.seg_consumed = stream->d_consumed.get();
    a.perm = batch->d_perm.get();
    a.out = out_dev;
    a.out_pcm16 = out_pcm16_dev;
    a.out_len = out_len_dev;
    a.out_stride = out_stride;
    a.cap = max_samples;
    a.n_utt = batch->n_utt;
    if (stream->voices_epoch != ctx->voices_epoch)
        return fail(GRAIL_ERR_INVALID_ARG, "the voice table changed since the stream was opened");
    a.half_capable = stream->half_capable ? 1u : 0u;
    a.any_blend = stream->any_blend ? 1u : 0u;
    a.live4 = stream->live4 ? 1u : 0u;
    // (may change between calls: both flavours share the state layout)
    // (sharper voices: the second tier has one-lane kernels only — streams on a wider mapping run the exact kernels)
    const int tier = fast_tier(ctx, batch);
    a.fast = tier == 1 ? 1u : (tier == 2 && stream->L == 1) ? 2u : 0u;
    // A few hundred to a few thousand streams leave most SIMDs idle on the lane kernels: they take the pipelined
    // workgroups (four waves share 16 / 8 utterances; synth_kernel<..., PIPE>) wherever a one-shot batch of this size
    // would — same state block as the lane kernels of the stream's mapping, exact arithmetic (a tolerance request is
    // served by them too: their bits are the reference's, and at these sizes they are the faster kernels)
    const uint64_t cus = (uint64_t)ctx->cus;
    if (ctx->opt.pipeline_option && !ctx->opt.lanes_option) {
        if (stream->live4 && stream->L == 4 && (int64_t)(((uint64_t)batch->n_utt + 15) / 16) <= pipe4_groups(ctx))
            a.pipe = ctx->opt.pipe_round32 && ((uint64_t)batch->n_utt + 15) / 16 <= cus ? 2u : 1u;
        else if (!stream->live4 && stream->L == 8 && (int64_t)(((uint64_t)batch->n_utt + 7) / 8) <= pipe8_groups(ctx))
            a.pipe = ctx->opt.pipe_round32 && ((uint64_t)batch->n_utt + 7) / 8 <= cus ? 2u : 1u;
        if (a.pipe) a.fast = 0u;
    }
    a.state = stream->d_state.get();
    a.state_stride = stream->lanes;
    a.resume = stream->started ? 1u : 0u;
    HIP_TRY(hipEventRecord(ctx->ev_start, ctx->stream));
    hipError_t e = launch_synth(a, stream->L, ctx->stream);
    if (e != hipSuccess) return hip_fail(e, "synth kernel launch");
    record_pull(ctx->stats, a, stream->L);
    HIP_TRY(hipEventRecord(ctx->ev_stop, ctx->stream));
    ctx->have_timing = true;
    stream->started = true;
    return GRAIL_OK;
}

int grail_stream_next_async(grail_ctx *ctx, grail_stream *stream, uint32_t max_samples,
                            float *out_dev, uint64_t out_stride, uint32_t *out_len_dev)
{
    return stream_next(ctx, stream, max_samples, out_dev, nullptr, out_stride, out_len_dev);
}

int grail_stream_next_pcm16_async(grail_ctx *ctx, grail_stream *stream, uint32_t max_samples,
                                  int16_t *out_dev, uint64_t out_stride, uint32_t *out_len_dev)
{
    return stream_next(ctx, stream, max_samples, nullptr, out_dev, out_stride, out_len_dev);
}

int grail_stream_close(grail_ctx *ctx, grail_stream *stream)
{
    if (!stream) return GRAIL_OK;
    int rc = bind(ctx);
    if (rc) return rc;
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    delete stream;          // (its buffers and events go with it, and the batch a live stream owns)
    return GRAIL_OK;
}

// ---- live streams: the lazy source of examples/interactive.rs:31-38 -------------------------------------------------
int grail_stream_open_live(grail_ctx *ctx, uint32_t n_utt, const uint32_t *voice_ids, const uint32_t *jitter_seeds,
                           uint32_t ring_segments, int caller_built_elems, grail_stream **out)
{
    int rc = bind(ctx);
    if (rc) return rc;
    if (!out) return fail(GRAIL_ERR_INVALID_ARG, "out is NULL");
    *out = nullptr;
    if (n_utt == 0) return fail(GRAIL_ERR_INVALID_ARG, "a live stream needs at least one utterance");
    if (ring_segments == 0) ring_segments = 64;
    if (ring_segments < 4 || (ring_segments & (ring_segments - 1)) != 0 || ring_segments > 65536)
        return fail(GRAIL_ERR_INVALID_ARG, "ring_segments must be a power of two, 4 .. 65536 (0: 64)");
    if ((uint64_t)n_utt * ring_segments > 0x7FFFFFFFull) return fail(GRAIL_ERR_INVALID_ARG, "n_utt x ring_segments exceeds 2^31");
    if (ctx->voices.empty() || !ctx->d_voices.get()) return fail(GRAIL_ERR_NO_VOICES, "call grail_set_voices first");
    grail_batch *b = new (std::nothrow) grail_batch();
    grail_stream *s = new (std::nothrow) grail_stream();
    if (!b || !s) {
        delete b;
        delete s;
        return fail(GRAIL_ERR_OUT_OF_MEMORY, "host allocation failed");
    }
    s->own.reset(b);
    s->batch = b;
    s->ring_cap = ring_segments;
    b->phoneme_mode = !caller_built_elems;
    b->any_blend = true;          // what will be appended is not known: the general instantiations
    b->plain = false;
    b->n_utt = n_utt;
    name_voices(*b, voice_ids, n_utt);
    const size_t ring_rows = (size_t)n_utt * ring_segments;      // (>= 4)
    hipError_t e = b->d_segs.alloc(ring_rows);
    if (e == hipSuccess) e = hipMemsetAsync(b->d_segs.get(), 0, ring_rows * sizeof(DevSeg), ctx->stream);
    if (e == hipSuccess && caller_built_elems) {
        e = b->d_elems.alloc(ring_rows * ELEM_FLOATS);
        if (e == hipSuccess) e = hipMemsetAsync(b->d_elems.get(), 0, ring_rows * ELEM_FLOATS * sizeof(float), ctx->stream);
    }
    for (DeviceBuffer<uint32_t> *p : {&s->d_counts, &s->d_consumed}) {
        if (e == hipSuccess) e = p->alloc(n_utt);
        if (e == hipSuccess) e = hipMemsetAsync(p->get(), 0, (size_t)n_utt * 4, ctx->stream);
    }
    if (e == hipSuccess) e = s->d_open.alloc(n_utt);
    if (e == hipSuccess) e = hipMemsetD32Async((hipDeviceptr_t)s->d_open.get(), 1, n_utt, ctx->stream);
    if (e == hipSuccess && voice_ids) e = upload(b->d_voice_ids, voice_ids, n_utt, ctx->stream);
    if (e == hipSuccess && jitter_seeds) e = upload(b->d_seeds, jitter_seeds, n_utt, ctx->stream);
    s->half_capable = batch_half_capable(ctx, b);
    s->any_blend = true;
    s->live4 = false;
    s->voices_epoch = ctx->voices_epoch;
    s->L = ctx->opt.lanes_option ? ctx->opt.lanes_option : auto_lanes_per_utt(n_utt, ctx_simds(ctx));
    s->lanes = state_lanes(n_utt, s->L);
    if (e == hipSuccess) e = s->d_state.alloc((size_t)state_words(s->L) * s->lanes);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);      // voice_ids / jitter_seeds are the caller's
    if (e != hipSuccess) {
        const int st = hip_fail(e, "live stream allocation");
        const std::string keep = last_error();
        grail_stream_close(ctx, s);
        last_error() = keep;
        return st;
    }
    s->appended.assign(n_utt, 0u);
    s->consumed.assign(n_utt, 0u);
    s->open.assign(n_utt, 1);
    if (caller_built_elems) {
        s->last_elem.resize(n_utt);
        s->last_has.assign(n_utt, 0);
    }
    *out = s;
    return GRAIL_OK;
}

// common part of the two append calls: room in the rings, upload, scatter on the device
static int live_append(grail_ctx *ctx, grail_stream *s, const std::vector<DevSeg> &segs, const float *elems,
                       const uint32_t *seg_offsets)
{
    const uint32_t n_utt = s->own->n_utt, cap = s->ring_cap;
    const uint32_t n_new = seg_offsets[n_utt];
    if (n_new == 0) return GRAIL_OK;
    // The Sequencer holds on to its current and next segment (and their elems in the ring are re-read when a call
    // resumes): a ring keeps the last two segments pulled besides everything pending.
    uint32_t full_at = 0;
    auto fits = [&]() {
        for (uint32_t u = 0; u < n_utt; ++u) {
            const uint32_t add = seg_offsets[u + 1] - seg_offsets[u];
            if (add && (uint64_t)s->appended[u] - s->consumed[u] + add + 2u > cap) {
                full_at = u;
                return false;
            }
        }
        return true;
    };
    if (!fits()) {
        // what the host knows of the Sequencers' progress is a lower bound: ask the device
        HIP_TRY(hipMemcpyAsync(s->consumed.data(), s->d_consumed.get(), (size_t)n_utt * 4, hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(hipStreamSynchronize(ctx->stream));
        if (!fits()) {
            char msg[200];
            std::snprintf(msg, sizeof msg, "the segment ring of utterance %u of the live stream is full (%u pending of %u): pull "
                          "samples first (or open the stream with a larger ring_segments); nothing was appended",
                          full_at, s->appended[full_at] - s->consumed[full_at], cap);
            return fail(GRAIL_ERR_BUFFER_TOO_SMALL, msg);
        }
    }
    for (uint32_t u = 0; u < n_utt; ++u)
        if (seg_offsets[u + 1] > seg_offsets[u] && !s->open[u])
            return fail(GRAIL_ERR_INVALID_ARG, "an utterance of the live stream has been finished: nothing can be appended to it");
    // the staging on the device: at least doubled when it grows (the first reserve that frees has waited for the stream,
    // the next finds it idle)
    const size_t cap_new = std::max<size_t>(std::max<size_t>(n_new, 2 * s->d_new.capacity()), 64);
    int rc;
    if ((rc = s->d_new.reserve(ctx->stream, n_new, cap_new))) return rc;
    if (elems && (rc = s->d_new_elems.reserve(ctx->stream, (size_t)n_new * ELEM_FLOATS, cap_new * ELEM_FLOATS))) return rc;
    if ((rc = s->d_new_offs.reserve(ctx->stream, (size_t)n_utt + 1))) return rc;
    hipError_t e = hipSuccess;
    // The caller's (and this function's) buffers go through a pinned buffer of the stream's own, so that the call can return
    // with its copies queued: with tens of thousands of live streams fed a phoneme at a time a synchronisation per append
    // — behind every kernel queued so far — was the pace of the whole session.
    const size_t b_segs = (size_t)n_new * sizeof(DevSeg), b_offs = ((size_t)n_utt + 1) * 4;
    const size_t b_elems = elems ? (size_t)n_new * ELEM_FLOATS * sizeof(float) : 0;
    const int slot = s->stage_next;
    if (s->stage_busy[slot]) {
        HIP_TRY(hipEventSynchronize(s->ev_stage[slot]));          // the append before last has left this buffer
        s->stage_busy[slot] = false;
    }
    if (s->h_stage[slot].capacity() < b_segs + b_offs + b_elems) {
        e = s->h_stage[slot].alloc(2 * (b_segs + b_offs + b_elems));
        if (e != hipSuccess) return hip_fail(e, "grail_stream_append pinned staging");
    }
    if (!s->ev_stage[slot]) HIP_TRY(s->ev_stage[slot].create());
    char *h = static_cast<char *>(s->h_stage[slot].get());
    std::memcpy(h, segs.data(), b_segs);
    std::memcpy(h + b_segs, seg_offsets, b_offs);
    if (elems) std::memcpy(h + b_segs + b_offs, elems, b_elems);
    e = hipMemcpyAsync(s->d_new.get(), h, b_segs, hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(s->d_new_offs.get(), h + b_segs, b_offs, hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess && elems)
        e = hipMemcpyAsync(s->d_new_elems.get(), h + b_segs + b_offs, b_elems, hipMemcpyHostToDevice, ctx->stream);
    // (stream order: behind every kernel that still reads the rings, ahead of every kernel that will)
    if (e == hipSuccess)
        e = launch_ring_append(s->own->d_segs.get(), s->own->d_elems.get(), s->d_counts.get(), cap, s->d_new.get(),
                               elems ? s->d_new_elems.get() : nullptr, s->d_new_offs.get(), n_utt, ctx->stream);
    if (e == hipSuccess) e = hipEventRecord(s->ev_stage[slot], ctx->stream);
    if (e != hipSuccess) {
        // some of the copies may be queued and still reading the pinned buffer, which the next append would overwrite (the
        // slot is not marked busy and stage_next does not move): wait for them before handing the failure back.  Whether
        // the scatter ran is unknown; `appended` is left alone, so the host's view stays a lower bound and the stream is
        // best closed by the caller.
        (void)hipStreamSynchronize(ctx->stream);
        return hip_fail(e, "grail_stream_append");
    }
    s->stage_busy[slot] = true;
    s->stage_next = slot ^ 1;
    for (uint32_t u = 0; u < n_utt; ++u) s->appended[u] += seg_offsets[u + 1] - seg_offsets[u];
    return GRAIL_OK;
}

static int live_check(grail_ctx *ctx, grail_stream *stream, const uint32_t *seg_offsets, bool elems)
{
    if (!stream || !stream->own) return fail(GRAIL_ERR_INVALID_ARG, "not a live stream (grail_stream_open_live)");
    if (stream->own->phoneme_mode == elems)
        return fail(GRAIL_ERR_INVALID_ARG, elems ? "the live stream takes PhonemeElems (grail_stream_append)"
                                                 : "the live stream takes SequenceElems (grail_stream_append_elems)");
    if (stream->voices_epoch != ctx->voices_epoch)
        return fail(GRAIL_ERR_INVALID_ARG, "the voice table changed since the stream was opened");
    uint32_t n = 0;
    return check_offsets(seg_offsets, stream->own->n_utt, &n);
}

int grail_stream_append(grail_ctx *ctx, grail_stream *stream, const grail_phoneme_elem *segs, const uint32_t *seg_offsets)
{
    int rc = bind(ctx);
    if (rc) return rc;
    if ((rc = live_check(ctx, stream, seg_offsets, false))) return rc;
    const uint32_t n_new = seg_offsets[stream->own->n_utt];
    if (n_new && !segs) return fail(GRAIL_ERR_INVALID_ARG, "segs is NULL");
    std::vector<DevSeg> ds(n_new);
    for (uint32_t i = 0; i < n_new; ++i) {
        if (segs[i].phoneme < 0 || segs[i].phoneme >= GRAIL_PH_COUNT)
            return fail(GRAIL_ERR_INVALID_ARG, "phoneme discriminant out of range");
        std::memcpy(&ds[i], &segs[i], sizeof(DevSeg));
    }
    return live_append(ctx, stream, ds, nullptr, seg_offsets);
}

int grail_stream_append_elems(grail_ctx *ctx, grail_stream *stream, const grail_sequence_elem *segs,
                              const uint32_t *seg_offsets)
{
    int rc = bind(ctx);
    if (rc) return rc;
    if ((rc = live_check(ctx, stream, seg_offsets, true))) return rc;
    const uint32_t n_utt = stream->own->n_utt, n_new = seg_offsets[n_utt];
    if (n_new && !segs) return fail(GRAIL_ERR_INVALID_ARG, "segs is NULL");
    std::vector<DevSeg> ds(n_new);
    std::vector<float> elems((size_t)(n_new ? n_new : 1) * ELEM_FLOATS);
    for (uint32_t i = 0; i < n_new; ++i) {
        ds[i].elem = segs[i].has_elem ? 0 : -1;        // (the device writes the ring row)
        ds[i].length = segs[i].length;
        ds[i].blend_length = segs[i].blend_length;
        ds[i].frequency = segs[i].elem.frequency;
        std::memcpy(&elems[(size_t)i * ELEM_FLOATS], &segs[i].elem, sizeof(grail_synthesis_elem));
    }
    // the sharpness fast arithmetic is served up to: every two consecutive elems of an utterance, the seam to what was
    // appended before included (grail_batch_upload_elems does the same over a closed list)
    double sharp = stream->own->elems_sharpness;
    std::vector<grail_synthesis_elem> last = stream->last_elem;
    std::vector<uint8_t> has = stream->last_has;
    for (uint32_t u = 0; u < n_utt; ++u)
        for (uint32_t i = seg_offsets[u]; i < seg_offsets[u + 1]; ++i) {
            if (segs[i].has_elem) {
                grail_synthesis_elem pair[2] = {segs[i].elem, segs[i].elem};
                size_t n_pair = 1;
                if (has[u]) pair[n_pair++] = last[u];
                sharp = std::fmax(sharp, elems_sharpness(pair, n_pair));
                last[u] = segs[i].elem;
            }
            has[u] = segs[i].has_elem ? 1 : 0;
        }
    rc = live_append(ctx, stream, ds, elems.data(), seg_offsets);
    if (rc) return rc;
    stream->own->elems_sharpness = sharp;
    stream->last_elem.swap(last);
    stream->last_has.swap(has);
    return GRAIL_OK;
}

int grail_stream_finish(grail_ctx *ctx, grail_stream *stream, const uint8_t *which)
{
    int rc = bind(ctx);
    if (rc) return rc;
    if (!stream || !stream->own) return fail(GRAIL_ERR_INVALID_ARG, "not a live stream (grail_stream_open_live)");
    const uint32_t n_utt = stream->own->n_utt;
    std::vector<uint32_t> open(n_utt);
    for (uint32_t u = 0; u < n_utt; ++u) {
        if (!which || which[u]) stream->open[u] = 0;
        open[u] = stream->open[u];
    }
    HIP_TRY(hipMemcpyAsync(stream->d_open.get(), open.data(), (size_t)n_utt * 4, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return GRAIL_OK;
}

int grail_stream_pending(grail_ctx *ctx, grail_stream *stream, uint32_t *pending)
{
    int rc = bind(ctx);
    if (rc) return rc;
    if (!stream || !stream->own) return fail(GRAIL_ERR_INVALID_ARG, "not a live stream (grail_stream_open_live)");
    if (!pending) return fail(GRAIL_ERR_INVALID_ARG, "pending is NULL");
    const uint32_t n_utt = stream->own->n_utt;
    HIP_TRY(hipMemcpyAsync(stream->consumed.data(), stream->d_consumed.get(), (size_t)n_utt * 4, hipMemcpyDeviceToHost,
                           ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    for (uint32_t u = 0; u < n_utt; ++u) pending[u] = stream->appended[u] - stream->consumed[u];
    return GRAIL_OK;
}

}  // extern "C"
