// transforms.cpp — the calls that read finished rows and write rows: grail_limit_async (limiter_kernels.hip),
// grail_resample_async (resample_kernels.hip, the ratio and table resample_plan.cpp, §4.13), grail_fir_create / _free / _async
// (fir_kernels.hip, a set's checks and image fir_plan.cpp, §4.14) and grail_filter_stream_open / _next_async / _finish_async /
// _close (§4.15), grail_resample_stream_open / _next_async / _finish_async / _close (§4.16) and grail_limit_stream_open /
// _next_async / _finish_async / _close (limit_plan.cpp, §4.17): their checks, their scratch, their launches.  What they check of a pair of rows is row_checks.h.
#include "api_internal.hpp"
#include "row_checks.h"

using namespace grail;
using namespace grail::host;

namespace {

// What a context owns by handle and the caller names by pointer.  A pointer from outside is looked up, never looked into: a
// stale one, or another context's, is not found.
template <typename T>
class Owned {
public:
    T *find(const T *p) const
    {
        for (const auto &q : items_)
            if (q.get() == p) return q.get();
        return nullptr;
    }
    T *add(std::unique_ptr<T> p) { return items_.emplace_back(std::move(p)).get(); }
    // (the caller has waited for whatever may still use it)
    void remove(const T *p)
    {
        items_.erase(std::remove_if(items_.begin(), items_.end(), [p](const auto &q) { return q.get() == p; }), items_.end());
    }
    template <typename Pred>
    bool any(Pred pred) const { return std::any_of(items_.begin(), items_.end(), [&](const auto &q) { return pred(*q); }); }

private:
    std::vector<std::unique_ptr<T>> items_;
};

struct ResampleTable {
    uint32_t up = 0, down = 0;              // 0: the slot holds no table
    uint64_t used = 0;                      // the call that last asked for it (the oldest is evicted)
    std::vector<int32_t> host;              // (kept while the upload may be in flight)
    DeviceBuffer<int32_t> dev;              // [up][taps]
};

// Per context (grail_ctx::transform_state), kept from call to call and only ever grown (DeviceBuffer::reserve, to the exact
// size), freed by grail_destroy: the chunk numbers that a limiter call folds (16 B per group and chunk of 4096 samples), the
// chunks' non-finite counts that a resampling call folds (4 B per chunk of 1024 outputs), the resampler's tables of the
// last few pairs of rates, the same counts of a filtering call (4 B per chunk of 2048 outputs), the filter sets the caller
// has created and the filter streams open on them (each with its rows' state: a ring of samples and one word per row).
struct TransformState : CtxPart {
    DeviceBuffer<unsigned char> d_lstat;    // limiter chunks
    DeviceBuffer<uint32_t> d_rbad;          // resampler chunks: non-finite counts
    ResampleTable tables[4];
    uint64_t table_calls = 0;
    DeviceBuffer<uint32_t> d_firbad;        // FIR chunks: non-finite counts
    Owned<grail_fir> firs;                  // the filter sets alive
    Owned<grail_filter_stream> fir_streams; // ... and, after them (they die first), the filter streams open on them
    Owned<grail_resample_stream> resample_streams;  // the resample streams open (each with its own copy of its pair's table)
    Owned<grail_limit_stream> limit_streams;        // the limit streams open (their chunks' numbers go to d_lstat)
};

// what the context has, made by nobody: NULL before the first call that needed it
TransformState *peek(grail_ctx *ctx) { return static_cast<TransformState *>(ctx->transform_state.get()); }

// ... and made at first use (the refusal's words are from when levels.cpp kept this state)
int state(grail_ctx *ctx, TransformState **st)
{
    if (!ctx->transform_state) ctx->transform_state.reset(new (std::nothrow) TransformState());
    return (*st = peek(ctx)) ? GRAIL_OK : fail(GRAIL_ERR_OUT_OF_MEMORY, "level state");
}

// the caller's pointer as one of ctx's own, or NULL
grail_fir *own_set(grail_ctx *ctx, const grail_fir *set) { return peek(ctx) ? peek(ctx)->firs.find(set) : nullptr; }
grail_filter_stream *own_stream(grail_ctx *ctx, const grail_filter_stream *fs)
{
    return peek(ctx) ? peek(ctx)->fir_streams.find(fs) : nullptr;
}

grail_resample_stream *own_resample_stream(grail_ctx *ctx, const grail_resample_stream *rs)
{
    return peek(ctx) ? peek(ctx)->resample_streams.find(rs) : nullptr;
}

grail_limit_stream *own_limit_stream(grail_ctx *ctx, const grail_limit_stream *ls)
{
    return peek(ctx) ? peek(ctx)->limit_streams.find(ls) : nullptr;
}

// the table of a pair of rates on the device: uploaded once per (U, D), the last four kept, the oldest evicted once
// everything queued on the stream is through (a kernel still queued may be reading it)
int resample_table(grail_ctx *ctx, TransformState *st, uint32_t rate_in, uint32_t rate_out, uint32_t U, uint32_t D, uint32_t P,
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

// the two kernels of a call on a stream: the outputs (chunks = 0: there are none to write), then the state
int fir_stream_call(grail_ctx *ctx, grail_filter_stream *fs, const float *in_dev, uint64_t in_stride,
                    const uint32_t *in_len_dev, const uint8_t *mark_dev, bool finishing, uint64_t chunks, float *out_dev,
                    uint64_t out_stride, uint32_t *out_len_dev, uint32_t *nonfinite_dev)
{
    TransformState *st;
    int rc = state(ctx, &st);
    if (rc) return rc;
    const grail_fir *set = fs->set;
    if (chunks) {
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

// ... and of a call on a resample stream
int resample_stream_call(grail_ctx *ctx, grail_resample_stream *rs, const float *in_dev, uint64_t in_stride,
                         const uint32_t *in_len_dev, const uint8_t *mark_dev, bool finishing, uint64_t chunks, float *out_dev,
                         uint64_t out_stride, uint32_t *out_len_dev, uint32_t *nonfinite_dev)
{
    TransformState *st;
    int rc = state(ctx, &st);
    if (rc) return rc;
    if (chunks) {
        if ((rc = st->d_rbad.reserve(ctx->stream, (size_t)rs->n_rows * (size_t)chunks))) return rc;
        const hipError_t e = launch_resample_stream(in_dev, in_stride, in_len_dev, rs->n_rows, rs->up, rs->down, rs->taps,
                                                    rs->d_table.get(), rs->d_state.get(), rs->d_ring.get(), rs->ring_cap, mark_dev,
                                                    finishing, (uint32_t)chunks, out_dev, out_stride, st->d_rbad.get(), ctx->stream);
        if (e != hipSuccess) return hip_fail(e, "resample stream kernel launch");
    }
    const hipError_t e = launch_resample_stream_advance(in_dev, in_stride, in_len_dev, rs->n_rows, rs->up, rs->down, rs->taps,
                                                        rs->d_state.get(), rs->d_ring.get(), rs->ring_cap, mark_dev, finishing,
                                                        st->d_rbad.get(), (uint32_t)chunks, out_len_dev, nonfinite_dev, ctx->stream);
    if (e != hipSuccess) return hip_fail(e, "resample stream advance kernel launch");
    return GRAIL_OK;
}

// ... and of a call on a limit stream
int limit_stream_call(grail_ctx *ctx, grail_limit_stream *ls, const float *in_dev, uint64_t in_stride, const uint32_t *in_len_dev,
                      const uint8_t *mark_dev, bool finishing, uint64_t chunks, float *out_dev, uint64_t out_stride,
                      uint32_t *out_len_dev, float *min_gain_dev, uint32_t *n_limited_dev, uint32_t *nonfinite_dev)
{
    TransformState *st;
    int rc = state(ctx, &st);
    if (rc) return rc;
    const uint32_t n_groups = ls->n_rows / ls->group;
    if (chunks) {
        if ((rc = st->d_lstat.reserve(ctx->stream, (size_t)n_groups * (size_t)chunks * limit_chunk_bytes()))) return rc;
        const hipError_t e = launch_limit_stream(in_dev, in_stride, in_len_dev, n_groups, ls->group, ls->ceiling, ls->ell,
                                                 ls->d_state.get(), ls->d_ring.get(), ls->ring_cap, mark_dev, finishing,
                                                 (uint32_t)chunks, out_dev, out_stride, st->d_lstat.get(), ctx->stream);
        if (e != hipSuccess) return hip_fail(e, "limit stream kernel launch");
    }
    const hipError_t e = launch_limit_stream_advance(in_dev, in_stride, in_len_dev, n_groups, ls->group, ls->ell, ls->d_state.get(),
                                                     ls->d_ring.get(), ls->ring_cap, mark_dev, finishing, st->d_lstat.get(),
                                                     (uint32_t)chunks, out_len_dev, min_gain_dev, n_limited_dev, nonfinite_dev,
                                                     ctx->stream);
    if (e != hipSuccess) return hip_fail(e, "limit stream advance kernel launch");
    return GRAIL_OK;
}

}  // namespace

extern "C" {

// In every call below, what is wrong with the arguments is said before what is wrong with the machine (bind_device).

int grail_limit_async(grail_ctx *ctx, const float *rows_dev, uint64_t row_stride, const uint32_t *len_dev, uint32_t n_rows,
                      uint32_t group, float ceiling, uint32_t lookahead_log2, float *out_dev, uint64_t out_stride,
                      float *min_gain_dev, uint32_t *n_limited_dev, uint32_t *nonfinite_dev)
{
    if (lookahead_log2 > GRAIL_LIMIT_LOOKAHEAD_LOG2_MAX)
        return fail(GRAIL_ERR_INVALID_ARG, "grail_limit_async: lookahead_log2 is above 10");
    if (group == 0 || n_rows % group != 0)
        return fail(GRAIL_ERR_INVALID_ARG, "grail_limit_async: n_rows is no multiple of group");
    if (!(ceiling > 0.0f) || !(ceiling <= 3.4028234663852886e38f))
        return fail(GRAIL_ERR_INVALID_ARG, "grail_limit_async: the ceiling is not a finite number above 0");
    if (out_stride < row_stride) return fail(GRAIL_ERR_INVALID_ARG, "grail_limit_async: out_stride < row_stride");
    if (const char *why = row_pair_error({rows_dev, row_stride, len_dev, n_rows, out_dev, out_stride}, OutRule::always, OutRule::always,
                                         "out_dev overlaps rows_dev (the look-ahead reads ahead of the stores)", 0))
        return fail(GRAIL_ERR_INVALID_ARG, std::string("grail_limit_async: ") + why);
    int rc = bind_device(ctx, "grail_limit_async");
    if (rc) return rc;
    if (n_rows == 0) return GRAIL_OK;
    TransformState *st;
    if ((rc = state(ctx, &st))) return rc;
    const uint32_t n_groups = n_rows / group;
    const uint64_t chunks = limit_grid_chunks(row_stride);
    // (the one argument check that comes after the device)
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
    uint32_t U, D, P;
    if (grail_resample_ratio(rate_in, rate_out, &U, &D, &P))
        return fail(GRAIL_ERR_INVALID_ARG, "grail_resample_async: the rates are equal, 0, or need more than 32 768 table entries");
    // (a row holds fewer than 2^32 samples: len is 32 bits wide)
    const uint64_t longest = (std::min<uint64_t>(row_stride, 0xFFFFFFFFull) * U + (D - 1u)) / D;
    if (const char *why = row_pair_error({rows_dev, row_stride, len_dev, n_rows, out_dev, out_stride}, OutRule::when_out_stride,
                                         OutRule::when_out_stride, "out_dev overlaps rows_dev (a chunk reads what another would have written)",
                                         longest))
        return fail(GRAIL_ERR_INVALID_ARG, std::string("grail_resample_async: ") + why);
    int rc = bind_device(ctx, "grail_resample_async");
    if (rc) return rc;
    if (n_rows == 0) return GRAIL_OK;
    TransformState *st;
    if ((rc = state(ctx, &st))) return rc;
    const uint64_t chunks = resample_grid_chunks(row_stride, out_stride, U, D);
    // (the one argument check that comes after the device)
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
    if (!out) return fail(GRAIL_ERR_INVALID_ARG, "grail_fir_create: NULL argument");
    if (const char *why = fir_set_error(taps, n_taps, origin, n_filters))
        return fail(GRAIL_ERR_INVALID_ARG, std::string("grail_fir_create: ") + why);
    int rc = bind_device(ctx, "grail_fir_create");
    if (rc) return rc;
    TransformState *st;
    if ((rc = state(ctx, &st))) return rc;
    std::unique_ptr<grail_fir> set(new (std::nothrow) grail_fir());
    if (!set) return fail(GRAIL_ERR_OUT_OF_MEMORY, "filter set");
    set->n_filters = n_filters;
    for (uint32_t f = 0; f < n_filters; ++f) set->taps_max = std::max(set->taps_max, n_taps[f]);
    fir_set_image(taps, n_taps, origin, n_filters, set->image, set->desc, &set->tail_max);
    HIP_TRY(upload(set->d_taps, set->image.data(), set->image.size(), ctx->stream));
    HIP_TRY(upload(set->d_desc, set->desc.data(), set->desc.size(), ctx->stream));
    *out = st->firs.add(std::move(set));
    return GRAIL_OK;
}

int grail_fir_free(grail_ctx *ctx, grail_fir *set)
{
    if (!set) return GRAIL_OK;
    if (!ctx) return fail(GRAIL_ERR_INVALID_ARG, "grail_fir_free: ctx is NULL");
    if (!own_set(ctx, set)) return fail(GRAIL_ERR_INVALID_ARG, "grail_fir_free: not a filter set of this context");
    TransformState *st = peek(ctx);
    if (st->fir_streams.any([set](const grail_filter_stream &fs) { return fs.set == set; }))
        return fail(GRAIL_ERR_INVALID_ARG, "grail_fir_free: the set still has open filter streams");
    // (a kernel or the upload still queued may be reading it)
    int rc = bind(ctx);
    if (rc) return rc;
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    st->firs.remove(set);
    return GRAIL_OK;
}

int grail_fir_async(grail_ctx *ctx, const grail_fir *set, const float *rows_dev, uint64_t row_stride, const uint32_t *len_dev,
                    uint32_t n_rows, const uint32_t *filter_dev, float *out_dev, uint64_t out_stride, uint32_t *out_len_dev,
                    uint32_t *nonfinite_dev)
{
    if (!set) return fail(GRAIL_ERR_INVALID_ARG, "grail_fir_async: set is NULL");
    if (ctx && !own_set(ctx, set)) return fail(GRAIL_ERR_INVALID_ARG, "grail_fir_async: not a filter set of this context");
    // (without a context the set was not looked up and is not looked into: the checks run with a tail of 0, and the call
    // ends at bind_device)
    const uint32_t tail_max = ctx ? set->tail_max : 0u;
    // (a row holds fewer than 2^32 samples: len is 32 bits wide)
    const uint64_t longest = std::min<uint64_t>(row_stride, 0xFFFFFFFFull) + tail_max;
    if (const char *why = row_pair_error({rows_dev, row_stride, len_dev, n_rows, out_dev, out_stride}, OutRule::when_out_stride,
                                         OutRule::when_out_stride, "out_dev overlaps rows_dev (a chunk reads what another would have written)",
                                         longest))
        return fail(GRAIL_ERR_INVALID_ARG, std::string("grail_fir_async: ") + why);
    const uint64_t chunks = n_rows && row_stride ? fir_grid_chunks(row_stride, out_stride, tail_max) : 0;
    if ((uint64_t)n_rows * chunks > 0x7FFFFFFFull) return fail(GRAIL_ERR_INVALID_ARG, "grail_fir_async: more than 2^31 chunks");
    int rc = bind_device(ctx, "grail_fir_async");
    if (rc) return rc;
    if (n_rows == 0) return GRAIL_OK;
    TransformState *st;
    if ((rc = state(ctx, &st))) return rc;
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

int grail_filter_stream_open(grail_ctx *ctx, const grail_fir *set, uint32_t n_rows, const uint32_t *filter, grail_filter_stream **out)
{
    // (no context exists without a device)
    if (!ctx || !out) return fail(GRAIL_ERR_INVALID_ARG, "grail_filter_stream_open: NULL argument");
    if (!own_set(ctx, set)) return fail(GRAIL_ERR_INVALID_ARG, "grail_filter_stream_open: not a filter set of this context");
    if (const char *why = fir_stream_open_error(filter, n_rows, set->n_filters))
        return fail(GRAIL_ERR_INVALID_ARG, std::string("grail_filter_stream_open: ") + why);
    int rc = bind(ctx);
    if (rc) return rc;
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
    *out = peek(ctx)->fir_streams.add(std::move(fs));       // (the set was found: the state is there)
    return GRAIL_OK;
}

int grail_filter_stream_close(grail_ctx *ctx, grail_filter_stream *fs)
{
    if (!fs) return GRAIL_OK;
    if (!ctx) return fail(GRAIL_ERR_INVALID_ARG, "grail_filter_stream_close: ctx is NULL");
    if (!own_stream(ctx, fs)) return fail(GRAIL_ERR_INVALID_ARG, "grail_filter_stream_close: not an open filter stream of this context");
    // (a kernel or an upload still queued may be using its state)
    int rc = bind(ctx);
    if (rc) return rc;
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    peek(ctx)->fir_streams.remove(fs);
    return GRAIL_OK;
}

int grail_filter_stream_next_async(grail_ctx *ctx, grail_filter_stream *fs, const float *in_dev, uint64_t in_stride,
                                   const uint32_t *in_len_dev, float *out_dev, uint64_t out_stride, uint32_t *out_len_dev,
                                   uint32_t *nonfinite_dev)
{
    if (!fs) return fail(GRAIL_ERR_INVALID_ARG, "grail_filter_stream_next_async: the stream is NULL");
    if (ctx && !own_stream(ctx, fs))
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
    if (ctx && !own_stream(ctx, fs))
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

int grail_resample_stream_open(grail_ctx *ctx, uint32_t rate_in, uint32_t rate_out, uint32_t n_rows, grail_resample_stream **out)
{
    // (no context exists without a device)
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
    rs->n_rows = n_rows;
    rs->ring_cap = resample_stream_ring_capacity(P);
    rs->table.assign((size_t)U * P, 0);
    if (grail_resample_coefficients(rate_in, rate_out, rs->table.data(), U * P))
        return fail(GRAIL_ERR_INVALID_ARG, "grail_resample_stream_open: no table for this pair of rates");
    HIP_TRY(upload(rs->d_table, rs->table.data(), rs->table.size(), ctx->stream));
    HIP_TRY(rs->d_state.alloc((size_t)n_rows * RESAMPLE_STREAM_STATE_WORDS));
    HIP_TRY(rs->d_ring.alloc((size_t)n_rows * rs->ring_cap));
    HIP_TRY(rs->d_mark.alloc(n_rows));
    // no sample fed, no row ended, the next output is output 0; the ring is never read before it is written, zeroed all the same
    HIP_TRY(hipMemsetAsync(rs->d_state.get(), 0, (size_t)n_rows * RESAMPLE_STREAM_STATE_WORDS * sizeof(uint64_t), ctx->stream));
    HIP_TRY(hipMemsetAsync(rs->d_ring.get(), 0, (size_t)n_rows * rs->ring_cap * sizeof(float), ctx->stream));
    *out = st->resample_streams.add(std::move(rs));
    return GRAIL_OK;
}

int grail_resample_stream_close(grail_ctx *ctx, grail_resample_stream *rs)
{
    if (!rs) return GRAIL_OK;
    if (!ctx) return fail(GRAIL_ERR_INVALID_ARG, "grail_resample_stream_close: ctx is NULL");
    if (!own_resample_stream(ctx, rs))
        return fail(GRAIL_ERR_INVALID_ARG, "grail_resample_stream_close: not an open resample stream of this context");
    // (a kernel or an upload still queued may be using its state or its table)
    int rc = bind(ctx);
    if (rc) return rc;
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    peek(ctx)->resample_streams.remove(rs);
    return GRAIL_OK;
}

int grail_resample_stream_next_async(grail_ctx *ctx, grail_resample_stream *rs, const float *in_dev, uint64_t in_stride,
                                     const uint32_t *in_len_dev, float *out_dev, uint64_t out_stride, uint32_t *out_len_dev,
                                     uint32_t *nonfinite_dev)
{
    if (!rs) return fail(GRAIL_ERR_INVALID_ARG, "grail_resample_stream_next_async: the stream is NULL");
    if (ctx && !own_resample_stream(ctx, rs))
        return fail(GRAIL_ERR_INVALID_ARG, "grail_resample_stream_next_async: not an open resample stream of this context");
    // (without a context the stream was not looked up and is not looked into: the checks run for one row at a ratio of 1 / 1,
    // and the call ends at bind_device)
    uint64_t chunks = 0;
    if (const char *why = resample_stream_next_error(in_dev, in_stride, in_len_dev, ctx ? rs->n_rows : 1u, out_dev, out_stride,
                                                     ctx ? rs->up : 1u, ctx ? rs->down : 1u, &chunks))
        return fail(GRAIL_ERR_INVALID_ARG, std::string("grail_resample_stream_next_async: ") + why);
    int rc = bind_device(ctx, "grail_resample_stream_next_async");
    if (rc) return rc;
    return resample_stream_call(ctx, rs, in_dev, in_stride, in_len_dev, nullptr, false, chunks, out_dev, out_stride, out_len_dev,
                                nonfinite_dev);
}

int grail_resample_stream_finish_async(grail_ctx *ctx, grail_resample_stream *rs, const uint8_t *which, float *out_dev,
                                       uint64_t out_stride, uint32_t *out_len_dev)
{
    if (!rs) return fail(GRAIL_ERR_INVALID_ARG, "grail_resample_stream_finish_async: the stream is NULL");
    if (ctx && !own_resample_stream(ctx, rs))
        return fail(GRAIL_ERR_INVALID_ARG, "grail_resample_stream_finish_async: not an open resample stream of this context");
    // (without a context: the checks of a ratio of 1 / 1 with two taps, a tail of one output, and the call ends at bind_device)
    uint64_t chunks = 0;
    if (const char *why = resample_stream_finish_error(out_dev, out_stride, ctx ? rs->n_rows : 1u, ctx ? rs->up : 1u,
                                                       ctx ? rs->down : 1u, ctx ? rs->taps : 2u, &chunks))
        return fail(GRAIL_ERR_INVALID_ARG, std::string("grail_resample_stream_finish_async: ") + why);
    int rc = bind_device(ctx, "grail_resample_stream_finish_async");
    if (rc) return rc;
    const uint8_t *mark_dev = nullptr;
    if (which) {
        // (the upload of the call before may still be reading the host copy)
        if (rs->ev_mark.get())
            HIP_TRY(hipEventSynchronize(rs->ev_mark));
        else
            HIP_TRY(rs->ev_mark.create());
        rs->mark.assign(which, which + rs->n_rows);
        HIP_TRY(hipMemcpyAsync(rs->d_mark.get(), rs->mark.data(), rs->n_rows, hipMemcpyHostToDevice, ctx->stream));
        HIP_TRY(hipEventRecord(rs->ev_mark, ctx->stream));
        mark_dev = rs->d_mark.get();
    }
    return resample_stream_call(ctx, rs, nullptr, 0, nullptr, mark_dev, true, chunks, out_dev, out_stride, out_len_dev, nullptr);
}

int grail_limit_stream_open(grail_ctx *ctx, uint32_t n_rows, uint32_t group, float ceiling, uint32_t lookahead_log2,
                            grail_limit_stream **out)
{
    if (const char *why = limit_stream_open_error(n_rows, group, ceiling, lookahead_log2))
        return fail(GRAIL_ERR_INVALID_ARG, std::string("grail_limit_stream_open: ") + why);
    // (no context exists without a device)
    if (!ctx || !out) return fail(GRAIL_ERR_INVALID_ARG, "grail_limit_stream_open: NULL argument");
    int rc = bind(ctx);
    if (rc) return rc;
    TransformState *st;
    if ((rc = state(ctx, &st))) return rc;
    std::unique_ptr<grail_limit_stream> ls(new (std::nothrow) grail_limit_stream());
    if (!ls) return fail(GRAIL_ERR_OUT_OF_MEMORY, "limit stream");
    ls->n_rows = n_rows, ls->group = group;
    ls->ceiling = ceiling, ls->ell = lookahead_log2;
    ls->ring_cap = limit_stream_ring_capacity(lookahead_log2);
    const size_t n_groups = n_rows / group;
    HIP_TRY(ls->d_state.alloc(n_groups));
    HIP_TRY(ls->d_ring.alloc((size_t)n_rows * ls->ring_cap));
    HIP_TRY(ls->d_mark.alloc(n_groups));
    // no sample fed, no group ended; the rings are read before they are written only where the index arithmetic discards
    // what was read: zeroed all the same
    HIP_TRY(hipMemsetAsync(ls->d_state.get(), 0, n_groups * sizeof(uint64_t), ctx->stream));
    HIP_TRY(hipMemsetAsync(ls->d_ring.get(), 0, (size_t)n_rows * ls->ring_cap * sizeof(float), ctx->stream));
    *out = st->limit_streams.add(std::move(ls));
    return GRAIL_OK;
}

int grail_limit_stream_close(grail_ctx *ctx, grail_limit_stream *ls)
{
    if (!ls) return GRAIL_OK;
    if (!ctx) return fail(GRAIL_ERR_INVALID_ARG, "grail_limit_stream_close: ctx is NULL");
    if (!own_limit_stream(ctx, ls)) return fail(GRAIL_ERR_INVALID_ARG, "grail_limit_stream_close: not an open limit stream of this context");
    // (a kernel or an upload still queued may be using its state)
    int rc = bind(ctx);
    if (rc) return rc;
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    peek(ctx)->limit_streams.remove(ls);
    return GRAIL_OK;
}

int grail_limit_stream_next_async(grail_ctx *ctx, grail_limit_stream *ls, const float *in_dev, uint64_t in_stride,
                                  const uint32_t *in_len_dev, float *out_dev, uint64_t out_stride, uint32_t *out_len_dev,
                                  float *min_gain_dev, uint32_t *n_limited_dev, uint32_t *nonfinite_dev)
{
    if (!ls) return fail(GRAIL_ERR_INVALID_ARG, "grail_limit_stream_next_async: the stream is NULL");
    if (ctx && !own_limit_stream(ctx, ls))
        return fail(GRAIL_ERR_INVALID_ARG, "grail_limit_stream_next_async: not an open limit stream of this context");
    // (without a context the stream was not looked up and is not looked into: the checks run for one row alone, and the call
    // ends at bind_device)
    uint64_t chunks = 0;
    if (const char *why = limit_stream_next_error(in_dev, in_stride, in_len_dev, ctx ? ls->n_rows : 1u, ctx ? ls->group : 1u, out_dev,
                                                  out_stride, &chunks))
        return fail(GRAIL_ERR_INVALID_ARG, std::string("grail_limit_stream_next_async: ") + why);
    int rc = bind_device(ctx, "grail_limit_stream_next_async");
    if (rc) return rc;
    return limit_stream_call(ctx, ls, in_dev, in_stride, in_len_dev, nullptr, false, chunks, out_dev, out_stride, out_len_dev,
                             min_gain_dev, n_limited_dev, nonfinite_dev);
}

int grail_limit_stream_finish_async(grail_ctx *ctx, grail_limit_stream *ls, const uint8_t *which, float *out_dev,
                                    uint64_t out_stride, uint32_t *out_len_dev, float *min_gain_dev, uint32_t *n_limited_dev)
{
    if (!ls) return fail(GRAIL_ERR_INVALID_ARG, "grail_limit_stream_finish_async: the stream is NULL");
    if (ctx && !own_limit_stream(ctx, ls))
        return fail(GRAIL_ERR_INVALID_ARG, "grail_limit_stream_finish_async: not an open limit stream of this context");
    // (without a context: the checks of one row alone at a look-ahead of one sample, and the call ends at bind_device)
    uint64_t chunks = 0;
    if (const char *why = limit_stream_finish_error(out_dev, out_stride, ctx ? ls->n_rows : 1u, ctx ? ls->group : 1u,
                                                    ctx ? ls->ell : 0u, &chunks))
        return fail(GRAIL_ERR_INVALID_ARG, std::string("grail_limit_stream_finish_async: ") + why);
    int rc = bind_device(ctx, "grail_limit_stream_finish_async");
    if (rc) return rc;
    const uint8_t *mark_dev = nullptr;
    if (which) {
        // (the upload of the call before may still be reading the host copy)
        if (ls->ev_mark.get())
            HIP_TRY(hipEventSynchronize(ls->ev_mark));
        else
            HIP_TRY(ls->ev_mark.create());
        const uint32_t n_groups = ls->n_rows / ls->group;
        ls->mark.assign(which, which + n_groups);
        HIP_TRY(hipMemcpyAsync(ls->d_mark.get(), ls->mark.data(), n_groups, hipMemcpyHostToDevice, ctx->stream));
        HIP_TRY(hipEventRecord(ls->ev_mark, ctx->stream));
        mark_dev = ls->d_mark.get();
    }
    return limit_stream_call(ctx, ls, nullptr, 0, nullptr, mark_dev, true, chunks, out_dev, out_stride, out_len_dev, min_gain_dev,
                             n_limited_dev, nullptr);
}

}  // extern "C"
