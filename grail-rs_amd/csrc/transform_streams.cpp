// transform_streams.cpp — finished rows filtered, resampled and limited chunk by chunk: grail_filter_stream_open / _next_async /
// _finish_async / _close (fir_kernels.hip), grail_resample_stream_* (resample_kernels.hip, §4.16) and
// grail_limit_stream_* (limiter_kernels.hip, §4.17), and metered chunk by chunk: grail_meter_stream_* (meter_stream_kernels.hip,
// §4.18), and filtered recursively chunk by chunk: grail_iir_stream_* (iir_kernels.hip, §4.20; checks iir_plan.cpp; one launch
// a call, no ring), and compressed chunk by chunk: grail_dyn_stream_* (dyn_kernels.hip, §4.23; checks dyn_plan.cpp; one launch a call,
// no ring, no finish).  A kind's own are its argument checks (fir_plan.cpp, resample_plan.cpp, limit_plan.cpp, meter_plan.cpp; their common
// end row_checks.h), what it keeps beside the rings, and its launches (two; the meter's three), which take one struct of arguments
// filled once a call (kernels.h).  What the kinds do alike stands once, first: telling a stream of the context's, its device
// state, a finishing call's marks, its close, and what a call's arguments take from the stream (on_stream).
#include "transform_state.h"

using namespace grail;
using namespace grail::host;

namespace {

int refuse(const char *who, const std::string &why) { return fail(GRAIL_ERR_INVALID_ARG, std::string(who) + ": " + why); }

// The first two refusals of a call `who` on a stream of the context's `list`, which the refusals call a `noun` stream.  Without a
// context the stream is not looked up, and the caller does not look into it: its checks run with stand-in numbers, and the call
// ends at bind_device.
template <typename T>
int known(grail_ctx *ctx, Owned<T> TransformState::*list, const T *s, const char *who, const char *noun)
{
    if (!s) return refuse(who, "the stream is NULL");
    if (ctx && !own(ctx, list, s)) return refuse(who, std::string("not an open ") + noun + " stream of this context");
    return GRAIL_OK;
}

template <typename T>
int stream_close(grail_ctx *ctx, Owned<T> TransformState::*list, T *s, const char *who, const char *noun)
{
    if (!s) return GRAIL_OK;
    if (!ctx) return refuse(who, "ctx is NULL");
    if (!own(ctx, list, s)) return refuse(who, std::string("not an open ") + noun + " stream of this context");
    // (a kernel or an upload still queued may be using its state, or what the kind keeps beside it)
    int rc = bind(ctx);
    if (rc) return rc;
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    (peek(ctx)->*list).remove(s);
    return GRAIL_OK;
}

// The device state of a stream just opened (n_rows, units and ring_cap are set), `words` state words a unit: no sample fed,
// nothing ended.  The rings are zeroed all the same: a kernel reads a ring before it was written at most where the index
// arithmetic discards what was read.
int alloc_state(grail_ctx *ctx, ChunkedStream &s, size_t words)
{
    HIP_TRY(s.d_state.alloc(s.units * words));
    HIP_TRY(s.d_ring.alloc((size_t)s.n_rows * s.ring_cap));
    HIP_TRY(s.d_mark.alloc(s.units));
    HIP_TRY(hipMemsetAsync(s.d_state.get(), 0, s.units * words * sizeof(uint64_t), ctx->stream));
    HIP_TRY(hipMemsetAsync(s.d_ring.get(), 0, (size_t)s.n_rows * s.ring_cap * sizeof(float), ctx->stream));
    return GRAIL_OK;
}

// A finishing call's marks, one byte a unit, on their way to the device: *mark_dev is where the kernels read them, NULL
// (every unit) where the caller gave none.  The upload reads the stream's host copy when the queue gets to it, so the copy is
// rewritten only behind the event of the upload before.
int marks(grail_ctx *ctx, ChunkedStream &s, const uint8_t *which, const uint8_t **mark_dev)
{
    *mark_dev = nullptr;
    if (!which) return GRAIL_OK;
    if (s.ev_mark.get())
        HIP_TRY(hipEventSynchronize(s.ev_mark));
    else
        HIP_TRY(s.ev_mark.create());
    s.mark.assign(which, which + s.units);
    HIP_TRY(hipMemcpyAsync(s.d_mark.get(), s.mark.data(), s.units, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(hipEventRecord(s.ev_mark, ctx->stream));
    *mark_dev = s.d_mark.get();
    return GRAIL_OK;
}

// What a kind's arguments take from the call's samples and from the stream itself: its state, its ring, the marks.
void on_stream(RowCallArgs &a, const ChunkedStream &s, const float *in_dev, uint64_t in_stride, const uint32_t *in_len_dev,
               const uint8_t *mark_dev, bool finishing)
{
    a.rows = in_dev, a.row_stride = in_stride, a.len = in_len_dev;
    a.state = s.d_state.get(), a.ring = s.d_ring.get(), a.ring_cap = s.ring_cap, a.mark = mark_dev, a.finishing = finishing;
}

// The two kernels of a call on a stream: the outputs (chunks = 0: there are none to write), then the state.  One function a
// kind, for their launches take what the kind keeps.
int fir_stream_call(grail_ctx *ctx, grail_filter_stream *fs, const float *in_dev, uint64_t in_stride,
                    const uint32_t *in_len_dev, const uint8_t *mark_dev, bool finishing, uint64_t chunks, float *out_dev,
                    uint64_t out_stride, uint32_t *out_len_dev, uint32_t *nonfinite_dev)
{
    TransformState *st;
    int rc = state(ctx, &st);
    if (rc) return rc;
    if (chunks && (rc = st->d_firbad.reserve(ctx->stream, (size_t)fs->units * (size_t)chunks))) return rc;
    const grail_fir *set = fs->set;
    FirArgs a = {};
    on_stream(a, *fs, in_dev, in_stride, in_len_dev, mark_dev, finishing);
    a.n_rows = fs->n_rows, a.filter = fs->filter.dev.get(), a.taps = set->d_taps.get(), a.desc = set->d_desc.get();
    a.n_filters = set->n_filters, a.grid_chunks = (uint32_t)chunks, a.out = out_dev, a.out_stride = out_stride;
    a.cbad = st->d_firbad.get(), a.out_len = out_len_dev, a.nonfinite = nonfinite_dev;
    if (chunks) {
        const hipError_t e = launch_fir_stream(a, ctx->stream);
        if (e != hipSuccess) return hip_fail(e, "fir stream kernel launch");
    }
    const hipError_t e = launch_fir_stream_advance(a, ctx->stream);
    if (e != hipSuccess) return hip_fail(e, "fir stream advance kernel launch");
    return GRAIL_OK;
}

int resample_stream_call(grail_ctx *ctx, grail_resample_stream *rs, const float *in_dev, uint64_t in_stride,
                         const uint32_t *in_len_dev, const uint8_t *mark_dev, bool finishing, uint64_t chunks, float *out_dev,
                         uint64_t out_stride, uint32_t *out_len_dev, uint32_t *nonfinite_dev)
{
    TransformState *st;
    int rc = state(ctx, &st);
    if (rc) return rc;
    if (chunks && (rc = st->d_rbad.reserve(ctx->stream, (size_t)rs->units * (size_t)chunks))) return rc;
    ResampleArgs a = {};
    on_stream(a, *rs, in_dev, in_stride, in_len_dev, mark_dev, finishing);
    a.n_rows = rs->n_rows, a.up = rs->up, a.down = rs->down, a.taps = rs->taps, a.table = rs->d_table.get();
    a.grid_chunks = (uint32_t)chunks, a.out = out_dev, a.out_stride = out_stride;
    a.cbad = st->d_rbad.get(), a.out_len = out_len_dev, a.nonfinite = nonfinite_dev;
    if (chunks) {
        const hipError_t e = launch_resample_stream(a, ctx->stream);
        if (e != hipSuccess) return hip_fail(e, "resample stream kernel launch");
    }
    const hipError_t e = launch_resample_stream_advance(a, ctx->stream);
    if (e != hipSuccess) return hip_fail(e, "resample stream advance kernel launch");
    return GRAIL_OK;
}

int limit_stream_call(grail_ctx *ctx, grail_limit_stream *ls, const float *in_dev, uint64_t in_stride, const uint32_t *in_len_dev,
                      const uint8_t *mark_dev, bool finishing, uint64_t chunks, float *out_dev, uint64_t out_stride,
                      uint32_t *out_len_dev, float *min_gain_dev, uint32_t *n_limited_dev, uint32_t *nonfinite_dev)
{
    TransformState *st;
    int rc = state(ctx, &st);
    if (rc) return rc;
    if (chunks && (rc = st->d_lstat.reserve(ctx->stream, (size_t)ls->units * (size_t)chunks * limit_chunk_bytes()))) return rc;
    LimitArgs a = {};
    on_stream(a, *ls, in_dev, in_stride, in_len_dev, mark_dev, finishing);
    a.n_groups = ls->units, a.group = ls->group, a.ceiling = ls->ceiling, a.ell = ls->ell;
    a.grid_chunks = (uint32_t)chunks, a.out = out_dev, a.out_stride = out_stride, a.cstat = st->d_lstat.get();
    a.out_len = out_len_dev, a.min_gain = min_gain_dev, a.n_limited = n_limited_dev, a.nonfinite = nonfinite_dev;
    if (chunks) {
        const hipError_t e = launch_limit_stream(a, ctx->stream);
        if (e != hipSuccess) return hip_fail(e, "limit stream kernel launch");
    }
    const hipError_t e = launch_limit_stream_advance(a, ctx->stream);
    if (e != hipSuccess) return hip_fail(e, "limit stream advance kernel launch");
    return GRAIL_OK;
}

// A meter stream's call is three kernels: the hops (a feeding call with samples only), the call's true peak, the state.
int meter_stream_call(grail_ctx *ctx, grail_meter_stream *ms, const float *in_dev, uint64_t in_stride, const uint32_t *in_len_dev,
                      const uint8_t *mark_dev, bool finishing, uint64_t chunks, double *hop_sumsq_dev, uint64_t hops_stride,
                      uint32_t *n_hops_dev, double *true_peak_dev, uint32_t *nonfinite_dev)
{
    TransformState *st;
    int rc = state(ctx, &st);
    if (rc) return rc;
    if (chunks && (rc = st->d_mpeak.reserve(ctx->stream, (size_t)ms->n_rows * (size_t)chunks))) return rc;
    if (chunks && (rc = st->d_mbad.reserve(ctx->stream, (size_t)ms->n_rows * (size_t)chunks))) return rc;
    MeterStreamArgs a = {};
    on_stream(a, *ms, in_dev, in_stride, in_len_dev, mark_dev, finishing);
    a.n_rows = ms->n_rows, a.hop = ms->hop, a.coef = ms->coef, a.ledger = ms->d_ledger.get(), a.max_hops = ms->max_hops;
    a.hops_out = hop_sumsq_dev, a.hops_stride = hops_stride, a.grid_chunks = (uint32_t)chunks;
    a.cmax = st->d_mpeak.get(), a.cbad = st->d_mbad.get(), a.n_hops = n_hops_dev, a.true_peak = true_peak_dev, a.nonfinite = nonfinite_dev;
    if (chunks) {
        if (!finishing) {
            const hipError_t e = launch_meter_stream_hops(a, ctx->stream);
            if (e != hipSuccess) return hip_fail(e, "meter stream hops kernel launch");
        }
        const hipError_t e = launch_meter_stream_peak(a, ctx->stream);
        if (e != hipSuccess) return hip_fail(e, "meter stream peak kernel launch");
    }
    const hipError_t e = launch_meter_stream_advance(a, ctx->stream);
    if (e != hipSuccess) return hip_fail(e, "meter stream advance kernel launch");
    return GRAIL_OK;
}

// An IIR stream's call is one kernel: grail_iir_async's, with the rows' state read at entry and written at exit.
int iir_stream_call(grail_ctx *ctx, grail_iir_stream *is, const float *in_dev, uint64_t in_stride, const uint32_t *in_len_dev,
                    const uint8_t *mark_dev, bool finishing, float *out_dev, uint64_t out_stride, uint32_t *out_len_dev,
                    uint32_t *nonfinite_dev)
{
    const grail_iir *set = is->set;
    IirArgs a = {};
    a.rows = in_dev, a.row_stride = in_stride, a.len = in_len_dev, a.n_rows = is->n_rows, a.filter = is->filter.dev.get();
    a.image = set->d_image.get(), a.sections = set->d_sections.get(), a.n_filters = set->n_filters, a.tail = is->tail;
    a.out = out_dev, a.out_stride = out_stride, a.out_len = out_len_dev, a.nonfinite = nonfinite_dev;
    a.state = is->d_state.get(), a.mark = mark_dev, a.finishing = finishing ? 1u : 0u;
    const hipError_t e = launch_iir(a, set->bound, ctx->stream);
    if (e != hipSuccess) return hip_fail(e, "iir stream kernel launch");
    return GRAIL_OK;
}

// A dynamics stream's call is one kernel too: grail_dyn_async's, with the rows' envelopes read at entry and written at exit.
int dyn_stream_call(grail_ctx *ctx, grail_dyn_stream *ds, const float *in_dev, uint64_t in_stride, const uint32_t *in_len_dev,
                    const float *key_dev, uint64_t key_stride, float *out_dev, uint64_t out_stride, uint32_t *out_len_dev,
                    uint32_t *nonfinite_dev, double *min_gain_dev)
{
    const grail_dyn *set = ds->set;
    DynArgs a = {};
    a.rows = in_dev, a.row_stride = in_stride, a.len = in_len_dev, a.n_rows = ds->n_rows, a.curve = ds->curve.dev.get();
    a.image = set->d_image.get(), a.alpha = set->d_alpha.get(), a.detector = set->d_detector.get(), a.n_curves = set->n_curves;
    if (ds->n_keys && in_stride)        // (a call of no samples reads no key and may come without one)
        a.key = key_dev, a.key_stride = key_stride, a.n_keys = ds->n_keys, a.key_row = ds->key_row.dev.get();
    a.out = out_dev, a.out_stride = out_stride, a.out_len = out_len_dev, a.nonfinite = nonfinite_dev, a.min_gain = min_gain_dev;
    a.state = ds->d_state.get();
    const hipError_t e = launch_dyn(a, ctx->stream);
    if (e != hipSuccess) return hip_fail(e, "dyn stream kernel launch");
    return GRAIL_OK;
}

}  // namespace

extern "C" {

// In every call below, what is wrong with the arguments is said before what is wrong with the machine (bind_device).  An open
// has no context without a device, so its "NULL argument" stands for both.

int grail_filter_stream_open(grail_ctx *ctx, const grail_fir *set, uint32_t n_rows, const uint32_t *filter, grail_filter_stream **out)
{
    if (!ctx || !out) return fail(GRAIL_ERR_INVALID_ARG, "grail_filter_stream_open: NULL argument");
    if (!own(ctx, &TransformState::firs, set)) return fail(GRAIL_ERR_INVALID_ARG, "grail_filter_stream_open: not a filter set of this context");
    if (const char *why = fir_stream_open_error(filter, n_rows, set->n_filters)) return refuse("grail_filter_stream_open", why);
    int rc = bind(ctx);
    if (rc) return rc;
    std::unique_ptr<grail_filter_stream> fs(new (std::nothrow) grail_filter_stream());
    if (!fs) return fail(GRAIL_ERR_OUT_OF_MEMORY, "filter stream");
    fs->set = set;
    fs->n_rows = fs->units = n_rows;
    fs->ring_cap = fir_stream_ring_capacity(set->taps_max);
    HIP_TRY(fs->filter.fill(filter, n_rows, false, ctx->stream));
    if ((rc = alloc_state(ctx, *fs, 1))) return rc;
    *out = peek(ctx)->fir_streams.add(std::move(fs));       // (the set was found: the state is there)
    return GRAIL_OK;
}

int grail_filter_stream_close(grail_ctx *ctx, grail_filter_stream *fs)
{
    return stream_close(ctx, &TransformState::fir_streams, fs, "grail_filter_stream_close", "filter");
}

int grail_filter_stream_next_async(grail_ctx *ctx, grail_filter_stream *fs, const float *in_dev, uint64_t in_stride,
                                   const uint32_t *in_len_dev, float *out_dev, uint64_t out_stride, uint32_t *out_len_dev,
                                   uint32_t *nonfinite_dev)
{
    const char *who = "grail_filter_stream_next_async";
    int rc = known(ctx, &TransformState::fir_streams, fs, who, "filter");
    if (rc) return rc;
    // (without a context: the checks of one row)
    uint64_t chunks = 0;
    if (const char *why = fir_stream_next_error(in_dev, in_stride, in_len_dev, ctx ? fs->n_rows : 1u, out_dev, out_stride, &chunks))
        return refuse(who, why);
    if ((rc = bind_device(ctx, who))) return rc;
    return fir_stream_call(ctx, fs, in_dev, in_stride, in_len_dev, nullptr, false, chunks, out_dev, out_stride, out_len_dev,
                           nonfinite_dev);
}

int grail_filter_stream_finish_async(grail_ctx *ctx, grail_filter_stream *fs, const uint8_t *which, float *out_dev,
                                     uint64_t out_stride, uint32_t *out_len_dev)
{
    const char *who = "grail_filter_stream_finish_async";
    int rc = known(ctx, &TransformState::fir_streams, fs, who, "filter");
    if (rc) return rc;
    // (without a context: the checks of one row and a set of one tap)
    uint64_t chunks = 0;
    if (const char *why = fir_stream_finish_error(out_dev, out_stride, ctx ? fs->n_rows : 1u, ctx ? fs->set->taps_max : 1u, &chunks))
        return refuse(who, why);
    if ((rc = bind_device(ctx, who))) return rc;
    const uint8_t *mark_dev;
    if ((rc = marks(ctx, *fs, which, &mark_dev))) return rc;
    return fir_stream_call(ctx, fs, nullptr, 0, nullptr, mark_dev, true, chunks, out_dev, out_stride, out_len_dev, nullptr);
}

int grail_resample_stream_open(grail_ctx *ctx, uint32_t rate_in, uint32_t rate_out, uint32_t n_rows, grail_resample_stream **out)
{
    if (!ctx || !out) return fail(GRAIL_ERR_INVALID_ARG, "grail_resample_stream_open: NULL argument");
    uint32_t U, D, P;
    if (grail_resample_ratio(rate_in, rate_out, &U, &D, &P))
        return fail(GRAIL_ERR_INVALID_ARG, "grail_resample_stream_open: the rates are equal, 0, or need more than 32 768 table entries");
    if (n_rows == 0) return fail(GRAIL_ERR_INVALID_ARG, "grail_resample_stream_open: n_rows is 0");
    int rc = bind(ctx);
    if (rc) return rc;
    TransformState *st;
    if ((rc = state(ctx, &st))) return rc;
    std::unique_ptr<grail_resample_stream> rs(new (std::nothrow) grail_resample_stream());
    if (!rs) return fail(GRAIL_ERR_OUT_OF_MEMORY, "resample stream");
    rs->up = U, rs->down = D, rs->taps = P;
    rs->n_rows = rs->units = n_rows;
    rs->ring_cap = resample_stream_ring_capacity(P);
    rs->table.assign((size_t)U * P, 0);
    if (grail_resample_coefficients(rate_in, rate_out, rs->table.data(), U * P))
        return fail(GRAIL_ERR_INVALID_ARG, "grail_resample_stream_open: no table for this pair of rates");
    HIP_TRY(upload(rs->d_table, rs->table.data(), rs->table.size(), ctx->stream));
    if ((rc = alloc_state(ctx, *rs, RESAMPLE_STREAM_STATE_WORDS))) return rc;       // (the next output is output 0)
    *out = st->resample_streams.add(std::move(rs));
    return GRAIL_OK;
}

int grail_resample_stream_close(grail_ctx *ctx, grail_resample_stream *rs)
{
    return stream_close(ctx, &TransformState::resample_streams, rs, "grail_resample_stream_close", "resample");
}

int grail_resample_stream_next_async(grail_ctx *ctx, grail_resample_stream *rs, const float *in_dev, uint64_t in_stride,
                                     const uint32_t *in_len_dev, float *out_dev, uint64_t out_stride, uint32_t *out_len_dev,
                                     uint32_t *nonfinite_dev)
{
    const char *who = "grail_resample_stream_next_async";
    int rc = known(ctx, &TransformState::resample_streams, rs, who, "resample");
    if (rc) return rc;
    // (without a context: the checks of one row at a ratio of 1 / 1)
    uint64_t chunks = 0;
    if (const char *why = resample_stream_next_error(in_dev, in_stride, in_len_dev, ctx ? rs->n_rows : 1u, out_dev, out_stride,
                                                     ctx ? rs->up : 1u, ctx ? rs->down : 1u, &chunks))
        return refuse(who, why);
    if ((rc = bind_device(ctx, who))) return rc;
    return resample_stream_call(ctx, rs, in_dev, in_stride, in_len_dev, nullptr, false, chunks, out_dev, out_stride, out_len_dev,
                                nonfinite_dev);
}

int grail_resample_stream_finish_async(grail_ctx *ctx, grail_resample_stream *rs, const uint8_t *which, float *out_dev,
                                       uint64_t out_stride, uint32_t *out_len_dev)
{
    const char *who = "grail_resample_stream_finish_async";
    int rc = known(ctx, &TransformState::resample_streams, rs, who, "resample");
    if (rc) return rc;
    // (without a context: the checks of one row at a ratio of 1 / 1 with two taps, a tail of one output)
    uint64_t chunks = 0;
    if (const char *why = resample_stream_finish_error(out_dev, out_stride, ctx ? rs->n_rows : 1u, ctx ? rs->up : 1u,
                                                       ctx ? rs->down : 1u, ctx ? rs->taps : 2u, &chunks))
        return refuse(who, why);
    if ((rc = bind_device(ctx, who))) return rc;
    const uint8_t *mark_dev;
    if ((rc = marks(ctx, *rs, which, &mark_dev))) return rc;
    return resample_stream_call(ctx, rs, nullptr, 0, nullptr, mark_dev, true, chunks, out_dev, out_stride, out_len_dev, nullptr);
}

int grail_limit_stream_open(grail_ctx *ctx, uint32_t n_rows, uint32_t group, float ceiling, uint32_t lookahead_log2,
                            grail_limit_stream **out)
{
    // (this one says what is wrong with its numbers first)
    if (const char *why = limit_stream_open_error(n_rows, group, ceiling, lookahead_log2)) return refuse("grail_limit_stream_open", why);
    if (!ctx || !out) return fail(GRAIL_ERR_INVALID_ARG, "grail_limit_stream_open: NULL argument");
    int rc = bind(ctx);
    if (rc) return rc;
    TransformState *st;
    if ((rc = state(ctx, &st))) return rc;
    std::unique_ptr<grail_limit_stream> ls(new (std::nothrow) grail_limit_stream());
    if (!ls) return fail(GRAIL_ERR_OUT_OF_MEMORY, "limit stream");
    ls->n_rows = n_rows, ls->group = group, ls->units = n_rows / group;
    ls->ceiling = ceiling, ls->ell = lookahead_log2;
    ls->ring_cap = limit_stream_ring_capacity(lookahead_log2);
    if ((rc = alloc_state(ctx, *ls, 1))) return rc;
    *out = st->limit_streams.add(std::move(ls));
    return GRAIL_OK;
}

int grail_limit_stream_close(grail_ctx *ctx, grail_limit_stream *ls)
{
    return stream_close(ctx, &TransformState::limit_streams, ls, "grail_limit_stream_close", "limit");
}

int grail_limit_stream_next_async(grail_ctx *ctx, grail_limit_stream *ls, const float *in_dev, uint64_t in_stride,
                                  const uint32_t *in_len_dev, float *out_dev, uint64_t out_stride, uint32_t *out_len_dev,
                                  float *min_gain_dev, uint32_t *n_limited_dev, uint32_t *nonfinite_dev)
{
    const char *who = "grail_limit_stream_next_async";
    int rc = known(ctx, &TransformState::limit_streams, ls, who, "limit");
    if (rc) return rc;
    // (without a context: the checks of one row alone)
    uint64_t chunks = 0;
    if (const char *why = limit_stream_next_error(in_dev, in_stride, in_len_dev, ctx ? ls->n_rows : 1u, ctx ? ls->group : 1u, out_dev,
                                                  out_stride, &chunks))
        return refuse(who, why);
    if ((rc = bind_device(ctx, who))) return rc;
    return limit_stream_call(ctx, ls, in_dev, in_stride, in_len_dev, nullptr, false, chunks, out_dev, out_stride, out_len_dev,
                             min_gain_dev, n_limited_dev, nonfinite_dev);
}

int grail_limit_stream_finish_async(grail_ctx *ctx, grail_limit_stream *ls, const uint8_t *which, float *out_dev,
                                    uint64_t out_stride, uint32_t *out_len_dev, float *min_gain_dev, uint32_t *n_limited_dev)
{
    const char *who = "grail_limit_stream_finish_async";
    int rc = known(ctx, &TransformState::limit_streams, ls, who, "limit");
    if (rc) return rc;
    // (without a context: the checks of one row alone at a look-ahead of one sample)
    uint64_t chunks = 0;
    if (const char *why = limit_stream_finish_error(out_dev, out_stride, ctx ? ls->n_rows : 1u, ctx ? ls->group : 1u,
                                                    ctx ? ls->ell : 0u, &chunks))
        return refuse(who, why);
    if ((rc = bind_device(ctx, who))) return rc;
    const uint8_t *mark_dev;
    if ((rc = marks(ctx, *ls, which, &mark_dev))) return rc;
    return limit_stream_call(ctx, ls, nullptr, 0, nullptr, mark_dev, true, chunks, out_dev, out_stride, out_len_dev, min_gain_dev,
                             n_limited_dev, nullptr);
}

int grail_meter_stream_open(grail_ctx *ctx, uint32_t n_rows, uint32_t sample_rate, const double *coef, uint64_t max_hops,
                            grail_meter_stream **out)
{
    // (as the limit stream's: what is wrong with the numbers first)
    if (const char *why = meter_stream_open_error(n_rows, sample_rate, max_hops)) return refuse("grail_meter_stream_open", why);
    if (!ctx || !out) return fail(GRAIL_ERR_INVALID_ARG, "grail_meter_stream_open: NULL argument");
    int rc = bind(ctx);
    if (rc) return rc;
    TransformState *st;
    if ((rc = state(ctx, &st))) return rc;
    std::unique_ptr<grail_meter_stream> ms(new (std::nothrow) grail_meter_stream());
    if (!ms) return fail(GRAIL_ERR_OUT_OF_MEMORY, "meter stream");
    ms->n_rows = ms->units = n_rows;
    ms->sample_rate = sample_rate, ms->hop = meter_stream_hop(sample_rate), ms->max_hops = max_hops;
    ms->ring_cap = METER_STREAM_RING;
    if (coef)
        std::copy(coef, coef + 10, ms->coef);
    else if (grail_kweighting(sample_rate, ms->coef))
        return fail(GRAIL_ERR_INVALID_ARG, "grail_meter_stream_open: no K-weighting for this rate");
    HIP_TRY(ms->d_ledger.alloc((size_t)n_rows * (size_t)max_hops));
    HIP_TRY(hipMemsetAsync(ms->d_ledger.get(), 0, (size_t)n_rows * (size_t)max_hops * sizeof(double), ctx->stream));
    if ((rc = alloc_state(ctx, *ms, METER_STREAM_STATE_WORDS))) return rc;       // (no sample fed, every double +0.0)
    *out = st->meter_streams.add(std::move(ms));
    return GRAIL_OK;
}

int grail_meter_stream_close(grail_ctx *ctx, grail_meter_stream *ms)
{
    return stream_close(ctx, &TransformState::meter_streams, ms, "grail_meter_stream_close", "meter");
}

int grail_meter_stream_next_async(grail_ctx *ctx, grail_meter_stream *ms, const float *in_dev, uint64_t in_stride,
                                  const uint32_t *in_len_dev, double *hop_sumsq_dev, uint64_t hops_stride, uint32_t *n_hops_dev,
                                  double *true_peak_dev, uint32_t *nonfinite_dev)
{
    const char *who = "grail_meter_stream_next_async";
    int rc = known(ctx, &TransformState::meter_streams, ms, who, "meter");
    if (rc) return rc;
    // (without a context: the checks of one row at the smallest hop)
    uint64_t chunks = 0;
    if (const char *why = meter_stream_next_error(in_dev, in_stride, in_len_dev, ctx ? ms->n_rows : 1u, hop_sumsq_dev, hops_stride,
                                                  ctx ? ms->hop : GRAIL_LOUDNESS_RATE_MIN / 10u, &chunks))
        return refuse(who, why);
    if ((rc = bind_device(ctx, who))) return rc;
    return meter_stream_call(ctx, ms, in_dev, in_stride, in_len_dev, nullptr, false, chunks, hop_sumsq_dev, hops_stride, n_hops_dev,
                             true_peak_dev, nonfinite_dev);
}

int grail_meter_stream_read_async(grail_ctx *ctx, grail_meter_stream *ms, double *integrated_ms_dev, double *momentary_ms_dev,
                                  double *short_term_ms_dev, double *true_peak_dev, uint64_t *hops_dev)
{
    const char *who = "grail_meter_stream_read_async";
    int rc = known(ctx, &TransformState::meter_streams, ms, who, "meter");
    if (rc) return rc;
    if ((rc = bind_device(ctx, who))) return rc;
    const hipError_t e = launch_meter_stream_read(ms->d_state.get(), ms->n_rows, ms->hop, ms->d_ledger.get(), ms->max_hops,
                                                  integrated_ms_dev, momentary_ms_dev, short_term_ms_dev, true_peak_dev, hops_dev,
                                                  ctx->stream);
    if (e != hipSuccess) return hip_fail(e, "meter stream read kernel launch");
    return GRAIL_OK;
}

int grail_meter_stream_ledger(grail_ctx *ctx, grail_meter_stream *ms, const double **hops_dev, uint64_t *stride)
{
    const char *who = "grail_meter_stream_ledger";
    int rc = known(ctx, &TransformState::meter_streams, ms, who, "meter");
    if (rc) return rc;
    if (!hops_dev || !stride) return refuse(who, "NULL argument");
    if ((rc = bind_device(ctx, who))) return rc;
    *hops_dev = ms->d_ledger.get();
    *stride = ms->max_hops;
    return GRAIL_OK;
}

int grail_meter_stream_finish_async(grail_ctx *ctx, grail_meter_stream *ms, const uint8_t *which, double *true_peak_dev)
{
    const char *who = "grail_meter_stream_finish_async";
    int rc = known(ctx, &TransformState::meter_streams, ms, who, "meter");
    if (rc) return rc;
    if ((rc = bind_device(ctx, who))) return rc;
    const uint8_t *mark_dev;
    if ((rc = marks(ctx, *ms, which, &mark_dev))) return rc;
    // (one chunk a row: the eleven outputs after its last sample)
    return meter_stream_call(ctx, ms, nullptr, 0, nullptr, mark_dev, true, 1, nullptr, 0, nullptr, true_peak_dev, nullptr);
}

int grail_iir_stream_open(grail_ctx *ctx, const grail_iir *set, uint32_t n_rows, const uint32_t *filter, uint32_t tail,
                          grail_iir_stream **out)
{
    if (!ctx || !out) return fail(GRAIL_ERR_INVALID_ARG, "grail_iir_stream_open: NULL argument");
    if (!own(ctx, &TransformState::iirs, set)) return fail(GRAIL_ERR_INVALID_ARG, "grail_iir_stream_open: not a filter set of this context");
    if (const char *why = iir_stream_open_error(filter, n_rows, set->n_filters)) return refuse("grail_iir_stream_open", why);
    int rc = bind(ctx);
    if (rc) return rc;
    std::unique_ptr<grail_iir_stream> is(new (std::nothrow) grail_iir_stream());
    if (!is) return fail(GRAIL_ERR_OUT_OF_MEMORY, "IIR stream");
    is->set = set;
    is->tail = tail;
    is->n_rows = is->units = n_rows;
    is->ring_cap = 0;                                       // (no ring: the filter's memory is its state)
    HIP_TRY(is->filter.fill(filter, n_rows, false, ctx->stream));
    if ((rc = alloc_state(ctx, *is, iir_stream_state_words(set->bound)))) return rc;       // (nothing fed, every state +0.0)
    *out = peek(ctx)->iir_streams.add(std::move(is));       // (the set was found: the state is there)
    return GRAIL_OK;
}

int grail_iir_stream_close(grail_ctx *ctx, grail_iir_stream *is)
{
    return stream_close(ctx, &TransformState::iir_streams, is, "grail_iir_stream_close", "IIR");
}

int grail_iir_stream_next_async(grail_ctx *ctx, grail_iir_stream *is, const float *in_dev, uint64_t in_stride,
                                const uint32_t *in_len_dev, float *out_dev, uint64_t out_stride, uint32_t *out_len_dev,
                                uint32_t *nonfinite_dev)
{
    const char *who = "grail_iir_stream_next_async";
    int rc = known(ctx, &TransformState::iir_streams, is, who, "IIR");
    if (rc) return rc;
    // (without a context: the checks of one row)
    if (const char *why = iir_stream_next_error(in_dev, in_stride, in_len_dev, ctx ? is->n_rows : 1u, out_dev, out_stride))
        return refuse(who, why);
    if ((rc = bind_device(ctx, who))) return rc;
    return iir_stream_call(ctx, is, in_dev, in_stride, in_len_dev, nullptr, false, out_dev, out_stride, out_len_dev, nonfinite_dev);
}

int grail_iir_stream_finish_async(grail_ctx *ctx, grail_iir_stream *is, const uint8_t *which, float *out_dev, uint64_t out_stride,
                                  uint32_t *out_len_dev)
{
    const char *who = "grail_iir_stream_finish_async";
    int rc = known(ctx, &TransformState::iir_streams, is, who, "IIR");
    if (rc) return rc;
    // (without a context: the checks of one row with a tail of one output)
    if (const char *why = iir_stream_finish_error(out_dev, out_stride, ctx ? is->n_rows : 1u, ctx ? is->tail : 1u)) return refuse(who, why);
    if ((rc = bind_device(ctx, who))) return rc;
    const uint8_t *mark_dev;
    if ((rc = marks(ctx, *is, which, &mark_dev))) return rc;
    return iir_stream_call(ctx, is, nullptr, 0, nullptr, mark_dev, true, out_dev, out_stride, out_len_dev, nullptr);
}

int grail_dyn_stream_open(grail_ctx *ctx, const grail_dyn *set, uint32_t n_rows, const uint32_t *curve, uint32_t n_keys,
                          const uint32_t *key_row, grail_dyn_stream **out)
{
    if (!ctx || !out) return fail(GRAIL_ERR_INVALID_ARG, "grail_dyn_stream_open: NULL argument");
    if (!own(ctx, &TransformState::dyns, set)) return fail(GRAIL_ERR_INVALID_ARG, "grail_dyn_stream_open: not a curve set of this context");
    if (const char *why = dyn_stream_open_error(curve, n_rows, set->n_curves, n_keys, key_row)) return refuse("grail_dyn_stream_open", why);
    int rc = bind(ctx);
    if (rc) return rc;
    std::unique_ptr<grail_dyn_stream> ds(new (std::nothrow) grail_dyn_stream());
    if (!ds) return fail(GRAIL_ERR_OUT_OF_MEMORY, "dynamics stream");
    ds->set = set;
    ds->n_keys = n_keys;
    ds->n_rows = ds->units = n_rows;
    ds->ring_cap = 0;                                       // (no ring: the envelope is the row's memory)
    HIP_TRY(ds->curve.fill(curve, n_rows, false, ctx->stream));
    if (n_keys) HIP_TRY(ds->key_row.fill(key_row, n_rows, true, ctx->stream));
    if ((rc = alloc_state(ctx, *ds, DYN_STREAM_STATE_WORDS))) return rc;       // (nothing fed, e = +0.0)
    *out = peek(ctx)->dyn_streams.add(std::move(ds));       // (the set was found: the state is there)
    return GRAIL_OK;
}

int grail_dyn_stream_close(grail_ctx *ctx, grail_dyn_stream *ds)
{
    return stream_close(ctx, &TransformState::dyn_streams, ds, "grail_dyn_stream_close", "dynamics");
}

int grail_dyn_stream_next_async(grail_ctx *ctx, grail_dyn_stream *ds, const float *in_dev, uint64_t in_stride,
                                const uint32_t *in_len_dev, const float *key_dev, uint64_t key_stride, float *out_dev,
                                uint64_t out_stride, uint32_t *out_len_dev, uint32_t *nonfinite_dev, double *min_gain_dev)
{
    const char *who = "grail_dyn_stream_next_async";
    int rc = known(ctx, &TransformState::dyn_streams, ds, who, "dynamics");
    if (rc) return rc;
    // (without a context: the checks of one row, keyed by one key if a key comes with the call)
    if (const char *why = dyn_stream_next_error(in_dev, in_stride, in_len_dev, ctx ? ds->n_rows : 1u, ctx ? ds->n_keys != 0u : key_dev != nullptr,
                                                ctx ? ds->n_keys : 1u, key_dev, key_stride, out_dev, out_stride))
        return refuse(who, why);
    if ((rc = bind_device(ctx, who))) return rc;
    return dyn_stream_call(ctx, ds, in_dev, in_stride, in_len_dev, key_dev, key_stride, out_dev, out_stride, out_len_dev, nonfinite_dev,
                           min_gain_dev);
}

}  // extern "C"
