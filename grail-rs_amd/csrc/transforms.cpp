// transforms.cpp — the calls that read finished rows and write rows, at once: grail_limit_async (limiter_kernels.hip, DESIGN.md
// §4.12), grail_resample_async (resample_kernels.hip, the ratio and table resample_plan.cpp, §4.13) and grail_fir_create /
// _free / _async (fir_kernels.hip, a set's checks and image fir_plan.cpp, §4.14) and grail_iir_create / _free / _async
// (iir_kernels.hip, a set's checks and image iir_plan.cpp, §4.19) and grail_biquad_blocked_async (biquad_block_kernels.hip, its
// matrices, grid and scratch size iir_plan.cpp, §4.22) and grail_dyn_create / _free / _async (dyn_kernels.hip, a set's checks and
// image dyn_plan.cpp, §4.23) and grail_track_dyn_async (track_env_kernels.hip, §4.24) and grail_spectrum_create / _free / _async
// (spectrum_kernels.hip, a set's checks and image and the call's checks spectrum_plan.cpp, §4.25): their checks, their scratch,
// their launches.
// What they check of a pair of rows is row_checks.h.  The same chunk by chunk, on streams, is transform_streams.cpp; what a
// context keeps for both is transform_state.h.
#include "row_checks.h"
#include "transform_state.h"

using namespace grail;
using namespace grail::host;

namespace {

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

// grail_fir_free, grail_iir_free and grail_dyn_free: a set of the context's `sets` is released unless one of its `streams` is
// still open on it.  The refusals of the call `who` speak of a `set_noun` set and of `stream_noun` streams.
template <typename Set, typename Stream>
int set_free(grail_ctx *ctx, Owned<Set> TransformState::*sets, Owned<Stream> TransformState::*streams, Set *set, const char *who,
             const char *set_noun, const char *stream_noun)
{
    if (!set) return GRAIL_OK;
    if (!ctx) return fail(GRAIL_ERR_INVALID_ARG, std::string(who) + ": ctx is NULL");
    if (!own(ctx, sets, set)) return fail(GRAIL_ERR_INVALID_ARG, std::string(who) + ": not a " + set_noun + " set of this context");
    TransformState *st = peek(ctx);
    if ((st->*streams).any([set](const Stream &s) { return s.set == set; }))
        return fail(GRAIL_ERR_INVALID_ARG, std::string(who) + ": the set still has open " + stream_noun + " streams");
    // (a kernel or the upload still queued may be reading it)
    int rc = bind(ctx);
    if (rc) return rc;
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    (st->*sets).remove(set);
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
    if (chunks && (rc = st->d_lstat.reserve(ctx->stream, (size_t)n_groups * (size_t)chunks * limit_chunk_bytes()))) return rc;
    LimitArgs a = {};
    a.rows = rows_dev, a.row_stride = row_stride, a.len = len_dev, a.n_groups = n_groups, a.group = group;
    a.ceiling = ceiling, a.ell = lookahead_log2, a.grid_chunks = (uint32_t)chunks, a.out = out_dev, a.out_stride = out_stride;
    a.cstat = st->d_lstat.get(), a.min_gain = min_gain_dev, a.n_limited = n_limited_dev, a.nonfinite = nonfinite_dev;
    if (chunks) {               // (rows of no samples: 1.0f, 0, 0 from the totals alone)
        const hipError_t e = launch_limit_frames(a, ctx->stream);
        if (e != hipSuccess) return hip_fail(e, "limiter frames kernel launch");
    }
    if (!min_gain_dev && !n_limited_dev && !nonfinite_dev) return GRAIL_OK;
    const hipError_t e = launch_limit_totals(a, ctx->stream);
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
    ResampleArgs a = {};
    a.rows = rows_dev, a.row_stride = row_stride, a.len = len_dev, a.n_rows = n_rows, a.up = U, a.down = D, a.taps = P;
    a.grid_chunks = (uint32_t)chunks, a.out = out_dev, a.out_stride = out_stride, a.out_len = out_len_dev, a.nonfinite = nonfinite_dev;
    if (chunks) {               // (rows of no samples: 0, 0 from the totals alone)
        if ((rc = resample_table(ctx, st, rate_in, rate_out, U, D, P, &a.table))) return rc;
        if ((rc = st->d_rbad.reserve(ctx->stream, (size_t)n_rows * (size_t)chunks))) return rc;
    }
    a.cbad = st->d_rbad.get();
    if (chunks) {
        const hipError_t e = launch_resample(a, ctx->stream);
        if (e != hipSuccess) return hip_fail(e, "resample kernel launch");
    }
    if (!out_len_dev && !nonfinite_dev) return GRAIL_OK;
    const hipError_t e = launch_resample_totals(a, ctx->stream);
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
    return set_free(ctx, &TransformState::firs, &TransformState::fir_streams, set, "grail_fir_free", "filter", "filter");
}

int grail_fir_async(grail_ctx *ctx, const grail_fir *set, const float *rows_dev, uint64_t row_stride, const uint32_t *len_dev,
                    uint32_t n_rows, const uint32_t *filter_dev, float *out_dev, uint64_t out_stride, uint32_t *out_len_dev,
                    uint32_t *nonfinite_dev)
{
    if (!set) return fail(GRAIL_ERR_INVALID_ARG, "grail_fir_async: set is NULL");
    if (ctx && !own(ctx, &TransformState::firs, set)) return fail(GRAIL_ERR_INVALID_ARG, "grail_fir_async: not a filter set of this context");
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
    if (chunks && (rc = st->d_firbad.reserve(ctx->stream, (size_t)n_rows * (size_t)chunks))) return rc;
    FirArgs a = {};
    a.rows = rows_dev, a.row_stride = row_stride, a.len = len_dev, a.n_rows = n_rows, a.filter = filter_dev;
    a.taps = set->d_taps.get(), a.desc = set->d_desc.get(), a.n_filters = set->n_filters, a.grid_chunks = (uint32_t)chunks;
    a.out = out_dev, a.out_stride = out_stride, a.cbad = st->d_firbad.get(), a.out_len = out_len_dev, a.nonfinite = nonfinite_dev;
    if (chunks) {               // (rows of no samples: 0, 0 from the totals alone)
        const hipError_t e = launch_fir(a, ctx->stream);
        if (e != hipSuccess) return hip_fail(e, "fir kernel launch");
    }
    if (!out_len_dev && !nonfinite_dev) return GRAIL_OK;
    const hipError_t e = launch_fir_totals(a, ctx->stream);
    if (e != hipSuccess) return hip_fail(e, "fir totals kernel launch");
    return GRAIL_OK;
}

int grail_iir_create(grail_ctx *ctx, const double *coef, const uint32_t *n_sections, uint32_t n_filters, grail_iir **out)
{
    if (!out) return fail(GRAIL_ERR_INVALID_ARG, "grail_iir_create: NULL argument");
    if (const char *why = iir_set_error(coef, n_sections, n_filters))
        return fail(GRAIL_ERR_INVALID_ARG, std::string("grail_iir_create: ") + why);
    int rc = bind_device(ctx, "grail_iir_create");
    if (rc) return rc;
    TransformState *st;
    if ((rc = state(ctx, &st))) return rc;
    std::unique_ptr<grail_iir> set(new (std::nothrow) grail_iir());
    if (!set) return fail(GRAIL_ERR_OUT_OF_MEMORY, "recursive filter set");
    set->n_filters = n_filters;
    iir_set_image(coef, n_sections, n_filters, set->image, set->sections, &set->bound);
    HIP_TRY(upload(set->d_image, set->image.data(), set->image.size(), ctx->stream));
    HIP_TRY(upload(set->d_sections, set->sections.data(), set->sections.size(), ctx->stream));
    *out = st->iirs.add(std::move(set));
    return GRAIL_OK;
}

int grail_iir_free(grail_ctx *ctx, grail_iir *set)
{
    return set_free(ctx, &TransformState::iirs, &TransformState::iir_streams, set, "grail_iir_free", "filter", "IIR");
}

int grail_iir_async(grail_ctx *ctx, const grail_iir *set, const float *rows_dev, uint64_t row_stride, const uint32_t *len_dev,
                    uint32_t n_rows, const uint32_t *filter_dev, uint32_t tail, float *out_dev, uint64_t out_stride,
                    uint32_t *out_len_dev, uint32_t *nonfinite_dev)
{
    if (!set) return fail(GRAIL_ERR_INVALID_ARG, "grail_iir_async: set is NULL");
    // (without a context the set was not looked up and is not looked into: the call ends at bind_device)
    if (ctx && !own(ctx, &TransformState::iirs, set)) return fail(GRAIL_ERR_INVALID_ARG, "grail_iir_async: not a filter set of this context");
    // (a row holds fewer than 2^32 samples: len is 32 bits wide)
    const uint64_t longest = std::min<uint64_t>(row_stride, 0xFFFFFFFFull) + tail;
    if (const char *why = row_pair_error({rows_dev, row_stride, len_dev, n_rows, out_dev, out_stride}, OutRule::when_out_stride,
                                         OutRule::when_out_stride, "out_dev overlaps rows_dev (a wave reads ahead of another's stores)",
                                         longest))
        return fail(GRAIL_ERR_INVALID_ARG, std::string("grail_iir_async: ") + why);
    int rc = bind_device(ctx, "grail_iir_async");
    if (rc) return rc;
    if (n_rows == 0) return GRAIL_OK;
    if (row_stride == 0 && !out_len_dev && !nonfinite_dev) return GRAIL_OK;     // (rows of no samples, and nobody asks)
    IirArgs a = {};
    a.rows = rows_dev, a.row_stride = row_stride, a.len = len_dev, a.n_rows = n_rows, a.filter = filter_dev;
    a.image = set->d_image.get(), a.sections = set->d_sections.get(), a.n_filters = set->n_filters, a.tail = tail;
    a.out = out_dev, a.out_stride = out_stride, a.out_len = out_len_dev, a.nonfinite = nonfinite_dev;
    const hipError_t e = launch_iir(a, set->bound, ctx->stream);
    if (e != hipSuccess) return hip_fail(e, "iir kernel launch");
    return GRAIL_OK;
}

int grail_dyn_create(grail_ctx *ctx, const double *gain, const double *alpha, const uint32_t *detector, uint32_t n_curves,
                     grail_dyn **out)
{
    if (!out) return fail(GRAIL_ERR_INVALID_ARG, "grail_dyn_create: NULL argument");
    if (const char *why = dyn_set_error(gain, alpha, detector, n_curves))
        return fail(GRAIL_ERR_INVALID_ARG, std::string("grail_dyn_create: ") + why);
    int rc = bind_device(ctx, "grail_dyn_create");
    if (rc) return rc;
    TransformState *st;
    if ((rc = state(ctx, &st))) return rc;
    std::unique_ptr<grail_dyn> set(new (std::nothrow) grail_dyn());
    if (!set) return fail(GRAIL_ERR_OUT_OF_MEMORY, "curve set");
    set->n_curves = n_curves;
    dyn_set_image(gain, n_curves, set->image);
    set->alpha.assign(alpha, alpha + 2u * n_curves);
    set->detector.assign(detector, detector + n_curves);
    HIP_TRY(upload(set->d_image, set->image.data(), set->image.size(), ctx->stream));
    HIP_TRY(upload(set->d_alpha, set->alpha.data(), set->alpha.size(), ctx->stream));
    HIP_TRY(upload(set->d_detector, set->detector.data(), set->detector.size(), ctx->stream));
    *out = st->dyns.add(std::move(set));
    return GRAIL_OK;
}

int grail_dyn_free(grail_ctx *ctx, grail_dyn *set)
{
    return set_free(ctx, &TransformState::dyns, &TransformState::dyn_streams, set, "grail_dyn_free", "curve", "dynamics");
}

int grail_dyn_async(grail_ctx *ctx, const grail_dyn *set, const float *rows_dev, uint64_t row_stride, const uint32_t *len_dev,
                    uint32_t n_rows, const uint32_t *curve_dev, const float *key_dev, uint64_t key_stride, const uint32_t *key_len_dev,
                    uint32_t n_keys, const uint32_t *key_row_dev, float *out_dev, uint64_t out_stride, uint32_t *out_len_dev,
                    uint32_t *nonfinite_dev, double *min_gain_dev)
{
    if (!set) return fail(GRAIL_ERR_INVALID_ARG, "grail_dyn_async: set is NULL");
    // (without a context the set was not looked up and is not looked into: the call ends at bind_device)
    if (ctx && !own(ctx, &TransformState::dyns, set)) return fail(GRAIL_ERR_INVALID_ARG, "grail_dyn_async: not a curve set of this context");
    if (const char *why = dyn_call_error(rows_dev, row_stride, len_dev, n_rows, key_dev, key_stride, n_keys, key_row_dev, out_dev, out_stride))
        return fail(GRAIL_ERR_INVALID_ARG, std::string("grail_dyn_async: ") + why);
    int rc = bind_device(ctx, "grail_dyn_async");
    if (rc) return rc;
    if (n_rows == 0) return GRAIL_OK;
    if (row_stride == 0 && !out_len_dev && !nonfinite_dev && !min_gain_dev) return GRAIL_OK;    // (rows of no samples, and nobody asks)
    DynArgs a = {};
    a.rows = rows_dev, a.row_stride = row_stride, a.len = len_dev, a.n_rows = n_rows, a.curve = curve_dev;
    a.image = set->d_image.get(), a.alpha = set->d_alpha.get(), a.detector = set->d_detector.get(), a.n_curves = set->n_curves;
    a.key = key_dev, a.key_stride = key_stride, a.key_len = key_len_dev, a.n_keys = n_keys, a.key_row = key_row_dev;
    a.out = out_dev, a.out_stride = out_stride, a.out_len = out_len_dev, a.nonfinite = nonfinite_dev, a.min_gain = min_gain_dev;
    const hipError_t e = launch_dyn(a, ctx->stream);
    if (e != hipSuccess) return hip_fail(e, "dyn kernel launch");
    return GRAIL_OK;
}

int grail_track_dyn_async(grail_ctx *ctx, const grail_dyn *set, const float *rows_dev, uint64_t row_stride, const uint32_t *len_dev,
                          uint32_t n_rows, const uint32_t *curve_dev, const float *key_dev, uint64_t key_stride,
                          const uint32_t *key_len_dev, uint32_t n_keys, const uint32_t *key_row_dev, float *out_dev, uint64_t out_stride,
                          uint32_t *out_len_dev, uint32_t *nonfinite_dev, double *min_gain_dev)
{
    if (!set) return fail(GRAIL_ERR_INVALID_ARG, "grail_track_dyn_async: set is NULL");
    // (without a context the set was not looked up and is not looked into: the call ends at bind_device)
    if (ctx && !own(ctx, &TransformState::dyns, set))
        return fail(GRAIL_ERR_INVALID_ARG, "grail_track_dyn_async: not a curve set of this context");
    if (const char *why = dyn_call_error(rows_dev, row_stride, len_dev, n_rows, key_dev, key_stride, n_keys, key_row_dev, out_dev, out_stride))
        return fail(GRAIL_ERR_INVALID_ARG, std::string("grail_track_dyn_async: ") + why);
    // (a workgroup a row)
    if (n_rows > 0x7FFFFFFFull) return fail(GRAIL_ERR_INVALID_ARG, "grail_track_dyn_async: more than 2^31 workgroups");
    int rc = bind_device(ctx, "grail_track_dyn_async");
    if (rc) return rc;
    if (n_rows == 0) return GRAIL_OK;
    if (row_stride == 0 && !out_len_dev && !nonfinite_dev && !min_gain_dev) return GRAIL_OK;    // (rows of no samples, and nobody asks)
    DynArgs a = {};
    a.rows = rows_dev, a.row_stride = row_stride, a.len = len_dev, a.n_rows = n_rows, a.curve = curve_dev;
    a.image = set->d_image.get(), a.alpha = set->d_alpha.get(), a.detector = set->d_detector.get(), a.n_curves = set->n_curves;
    a.key = key_dev, a.key_stride = key_stride, a.key_len = key_len_dev, a.n_keys = n_keys, a.key_row = key_row_dev;
    a.out = out_dev, a.out_stride = out_stride, a.out_len = out_len_dev, a.nonfinite = nonfinite_dev, a.min_gain = min_gain_dev;
    const hipError_t e = launch_track_dyn(a, ctx->stream);
    if (e != hipSuccess) return hip_fail(e, "track dyn kernel launch");
    return GRAIL_OK;
}

int grail_spectrum_create(grail_ctx *ctx, uint32_t log2n, const float *window, uint32_t n_window, uint32_t hop, uint32_t pad,
                          uint32_t n_bands, const uint32_t *band_first, const uint32_t *band_count, const float *band_weights,
                          grail_spectrum **out)
{
    if (!out) return fail(GRAIL_ERR_INVALID_ARG, "grail_spectrum_create: NULL argument");
    if (const char *why = spectrum_set_error(log2n, window, n_window, hop, pad, n_bands, band_first, band_count, band_weights))
        return fail(GRAIL_ERR_INVALID_ARG, std::string("grail_spectrum_create: ") + why);
    int rc = bind_device(ctx, "grail_spectrum_create");
    if (rc) return rc;
    TransformState *st;
    if ((rc = state(ctx, &st))) return rc;
    std::unique_ptr<grail_spectrum> set(new (std::nothrow) grail_spectrum());
    if (!set) return fail(GRAIL_ERR_OUT_OF_MEMORY, "spectrum set");
    set->facts.log2n = log2n, set->facts.n_window = n_window, set->facts.hop = hop, set->facts.pad = pad, set->facts.n_bands = n_bands;
    set->window.assign(window, window + n_window);
    spectrum_set_image(log2n, n_bands, band_first, band_count, band_weights, set->twiddles, set->desc, set->weights);
    HIP_TRY(upload(set->d_window, set->window.data(), set->window.size(), ctx->stream));
    HIP_TRY(upload(set->d_twiddles, set->twiddles.data(), set->twiddles.size(), ctx->stream));
    HIP_TRY(upload(set->d_desc, set->desc.data(), set->desc.size(), ctx->stream));
    HIP_TRY(upload(set->d_weights, set->weights.data(), set->weights.size(), ctx->stream));
    *out = st->spectra.add(std::move(set));
    return GRAIL_OK;
}

// (set_free without its streams: no stream is ever open on a spectrum set)
int grail_spectrum_free(grail_ctx *ctx, grail_spectrum *set)
{
    if (!set) return GRAIL_OK;
    if (!ctx) return fail(GRAIL_ERR_INVALID_ARG, "grail_spectrum_free: ctx is NULL");
    if (!own(ctx, &TransformState::spectra, set)) return fail(GRAIL_ERR_INVALID_ARG, "grail_spectrum_free: not a spectrum set of this context");
    // (a kernel or the upload still queued may be reading it)
    int rc = bind(ctx);
    if (rc) return rc;
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    peek(ctx)->spectra.remove(set);
    return GRAIL_OK;
}

int grail_spectrum_async(grail_ctx *ctx, const grail_spectrum *set, const float *rows_dev, uint64_t row_stride, const uint32_t *len_dev,
                         uint32_t n_rows, float *power_dev, float *bands_dev, uint64_t frames_stride, uint32_t *n_frames_dev,
                         uint32_t *nonfinite_dev)
{
    if (!set) return fail(GRAIL_ERR_INVALID_ARG, "grail_spectrum_async: set is NULL");
    if (ctx && !own(ctx, &TransformState::spectra, set))
        return fail(GRAIL_ERR_INVALID_ARG, "grail_spectrum_async: not a spectrum set of this context");
    // (without a context the set was not looked up and is not looked into: the checks that need its facts are left out, and
    // the call ends at bind_device)
    if (const char *why = spectrum_call_error(ctx ? &set->facts : nullptr, rows_dev, row_stride, len_dev, n_rows, power_dev, bands_dev,
                                              frames_stride))
        return fail(GRAIL_ERR_INVALID_ARG, std::string("grail_spectrum_async: ") + why);
    int rc = bind_device(ctx, "grail_spectrum_async");
    if (rc) return rc;
    if (n_rows == 0) return GRAIL_OK;
    if (row_stride == 0 && !n_frames_dev && !nonfinite_dev) return GRAIL_OK;    // (rows of no samples, and nobody asks)
    TransformState *st;
    if ((rc = state(ctx, &st))) return rc;
    const SpectrumFacts &f = set->facts;
    const uint64_t chunks = spectrum_grid_chunks(row_stride, f.hop);
    if (chunks && nonfinite_dev && (rc = st->d_specbad.reserve(ctx->stream, (size_t)n_rows * (size_t)chunks))) return rc;
    SpectrumArgs a = {};
    a.rows = rows_dev, a.row_stride = row_stride, a.len = len_dev, a.n_rows = n_rows;
    a.log2n = f.log2n, a.n_window = f.n_window, a.hop = f.hop, a.pad = f.pad, a.n_bands = f.n_bands;
    a.window = set->d_window.get(), a.twiddles = set->d_twiddles.get(), a.band_desc = set->d_desc.get();
    a.band_weights = set->d_weights.get(), a.power = power_dev, a.bands = bands_dev, a.frames_stride = frames_stride;
    a.grid_chunks = (uint32_t)chunks, a.cbad = chunks && nonfinite_dev ? st->d_specbad.get() : nullptr;
    a.n_frames = n_frames_dev, a.nonfinite = nonfinite_dev;
    if (chunks) {               // (rows of no samples: 0, 0 from the totals alone)
        const hipError_t e = launch_spectrum(a, ctx->stream);
        if (e != hipSuccess) return hip_fail(e, "spectrum kernel launch");
    }
    if (!n_frames_dev && !nonfinite_dev) return GRAIL_OK;
    const hipError_t e = launch_spectrum_totals(a, ctx->stream);
    if (e != hipSuccess) return hip_fail(e, "spectrum totals kernel launch");
    return GRAIL_OK;
}

int grail_biquad_blocked_async(grail_ctx *ctx, const grail_iir *set, const float *rows_dev, uint64_t row_stride, const uint32_t *len_dev,
                            uint32_t n_rows, const uint32_t *filter_dev, uint32_t tail, float *out_dev, uint64_t out_stride,
                            uint32_t *out_len_dev, uint32_t *nonfinite_dev)
{
    if (!set) return fail(GRAIL_ERR_INVALID_ARG, "grail_biquad_blocked_async: set is NULL");
    // (without a context the set was not looked up and is not looked into: the call ends at bind_device)
    grail_iir *mine = ctx ? own(ctx, &TransformState::iirs, set) : nullptr;
    if (ctx && !mine) return fail(GRAIL_ERR_INVALID_ARG, "grail_biquad_blocked_async: not a filter set of this context");
    // (a row holds fewer than 2^32 samples: len is 32 bits wide)
    const uint64_t longest = std::min<uint64_t>(row_stride, 0xFFFFFFFFull) + tail;
    if (const char *why = row_pair_error({rows_dev, row_stride, len_dev, n_rows, out_dev, out_stride}, OutRule::when_out_stride,
                                         OutRule::when_out_stride, "out_dev overlaps rows_dev (a wave reads ahead of another's stores)",
                                         longest))
        return fail(GRAIL_ERR_INVALID_ARG, std::string("grail_biquad_blocked_async: ") + why);
    const uint64_t blocks = n_rows && row_stride ? iir_block_grid_blocks(row_stride, tail) : 0;
    const uint64_t groups = iir_block_groups(blocks);
    if ((uint64_t)n_rows * groups > 0x7FFFFFFFull)
        return fail(GRAIL_ERR_INVALID_ARG, "grail_biquad_blocked_async: more than 2^31 workgroups");
    int rc = bind_device(ctx, "grail_biquad_blocked_async");
    if (rc) return rc;
    if (n_rows == 0) return GRAIL_OK;
    if (row_stride == 0 && !out_len_dev && !nonfinite_dev) return GRAIL_OK;     // (rows of no samples, and nobody asks)
    TransformState *st;
    if ((rc = state(ctx, &st))) return rc;
    BiquadBlockArgs a = {};
    a.rows = rows_dev, a.row_stride = row_stride, a.len = len_dev, a.n_rows = n_rows, a.filter = filter_dev;
    a.image = mine->d_image.get(), a.sections = mine->d_sections.get(), a.n_filters = mine->n_filters, a.tail = tail;
    a.out = out_dev, a.out_stride = out_stride, a.grid_blocks = (uint32_t)blocks, a.groups = (uint32_t)groups;
    if (blocks) {               // (rows of no samples: 0, 0 from the totals alone)
        if (!mine->d_block.get()) {
            iir_block_image(mine->image, mine->sections, mine->block_image);
            const hipError_t up = upload(mine->d_block, mine->block_image.data(), mine->block_image.size(), ctx->stream);
            if (up != hipSuccess) {     // (a later call starts over, not from an image that was never copied)
                mine->d_block.reset();
                return hip_fail(up, "block matrices upload");
            }
        }
        const uint64_t doubles = iir_block_scratch_doubles(n_rows, blocks, mine->bound);
        if (doubles > SIZE_MAX / sizeof(double)) return fail(GRAIL_ERR_OUT_OF_MEMORY, "grail_biquad_blocked_async: block states");
        if ((rc = st->d_iirblock.reserve(ctx->stream, (size_t)doubles))) return rc;
        if ((rc = st->d_iirbad.reserve(ctx->stream, (size_t)n_rows * (size_t)groups))) return rc;
        a.matrices = mine->d_block.get(), a.state = st->d_iirblock.get(), a.cbad = st->d_iirbad.get();
        hipError_t e = launch_biquad_block_rest(a, mine->bound, ctx->stream);
        if (e != hipSuccess) return hip_fail(e, "biquad block rest kernel launch");
        if ((e = launch_biquad_block_propagate(a, mine->bound, ctx->stream)) != hipSuccess)
            return hip_fail(e, "biquad block propagate kernel launch");
        if ((e = launch_biquad_block_output(a, mine->bound, ctx->stream)) != hipSuccess)
            return hip_fail(e, "biquad block output kernel launch");
    }
    if (!out_len_dev && !nonfinite_dev) return GRAIL_OK;
    const hipError_t e = launch_biquad_block_totals(a, out_len_dev, nonfinite_dev, ctx->stream);
    if (e != hipSuccess) return hip_fail(e, "biquad block totals kernel launch");
    return GRAIL_OK;
}

}  // extern "C"
