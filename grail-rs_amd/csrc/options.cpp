// options.cpp — the options of a context (include/grail_hip.h, "Options": the contract) as one table: a row per name
// with how a value is checked and where it lives.  grail_set_option and grail_get_option look the name up here.  Pure
// host code, like the launch planner (the debug_prof_<k> counters of -DGRAIL_FAST_PROF builds apart).
#include "api_internal.hpp"

using namespace grail;
using namespace grail::host;

namespace {

enum Access { RW, RO, WO };           // RO: a row without a setter; WO: settable, not readable
enum Kind {
    ANY,                              // any int64
    FLAG,                             // normalised to 0 / 1
    RANGE,                            // lo .. hi
    AT_LEAST,                         // lo ..
    LANES                             // 0, 1, 2, 4 or 8
};

struct Check {
    Kind kind = ANY;
    int64_t lo = 0, hi = 0;
    const char *error = nullptr;      // what a refused value is told
};
const Check flag = {FLAG, 0, 0, nullptr};
Check range(int64_t lo, int64_t hi, const char *error) { return {RANGE, lo, hi, error}; }
Check at_least(int64_t lo, const char *error) { return {AT_LEAST, lo, 0, error}; }

// a field of grail_ctx::opt, or accessors for what is computed or kept elsewhere
struct Where {
    int64_t Options::*field = nullptr;
    int64_t (*get)(const grail_ctx *) = nullptr;
    void (*set)(grail_ctx *, int64_t) = nullptr;
    Where(int64_t Options::*f) : field(f) {}
    Where(int64_t (*g)(const grail_ctx *), void (*s)(grail_ctx *, int64_t) = nullptr) : get(g), set(s) {}
};

struct Row {
    const char *name;
    Access access;
    Where where;
    Check check;
};

// (a read accessor from an expression over ctx)
#define GETTER(expr) {[](const grail_ctx *ctx) -> int64_t { return (int64_t)(expr); }}

const Row TABLE[] = {
    {"arithmetic", RW, &Options::fast_option, range(0, 2, "arithmetic must be 0 (exact), 1 (fast) or 2 (fast, exact coefficients)")},
    {"fast_sharpness_limit", RW, &Options::fast_limit, at_least(0, "negative limit")},
    {"fast_exact_coefficients", RW, &Options::mid_option, flag},
    {"fast_sharpness_limit_exact_coefficients", RW, &Options::mid_limit, at_least(0, "negative limit")},
    {"lanes_per_utterance", RW, &Options::lanes_option, {LANES, 0, 0, "lanes_per_utterance must be 0, 1, 2, 4 or 8"}},
    {"skip_silent_formants", RW, &Options::skip_silent_option, flag},
    {"small_batch_pipeline", RW, &Options::pipeline_option, flag},
    {"pipeline_round32", RW, &Options::pipe_round32,       // tuning (A/B)
     range(0, 2, "pipeline_round32 must be 0 (never), 1 (aligned batches) or 2 (any batch)")},
    {"pipeline_spread", RW, &Options::pipe_spread, flag},
    {"pipeline4_max_groups", RW, &Options::pipe4_max_groups, {}},   // tuning: four-formant batches, 16 utterances per workgroup
    {"pipeline8_max_groups", RW, &Options::pipe8_max_groups, {}},   // tuning: 0 keeps eight-formant batches off the pipeline
    {"time_parallel_scan", RW, &Options::scan_option, flag},
    // (read as set (-1: 34 / 6 per compute unit), so that get / set restores exactly)
    {"time_parallel_scan_max_utterances", RW, &Options::scan_max_utts, at_least(-1, "negative limit")},
    {"time_parallel_scan_split_max_utterances", RW, &Options::scan_split_max, at_least(-1, "negative limit")},
    {"time_split", RW, &Options::split_option, flag},
    {"time_split_min_utterances", RW, &Options::split_min_utts, at_least(-1, "negative limit")},   // -1: the cost model decides
    {"time_split_chunks", RW, &Options::split_chunks, range(0, SPLIT_MAX_CHUNKS, "time_split_chunks must be 0 (auto) .. 64")},
    {"time_split_span_samples", RW, &Options::split_span, range(0, 0x7fffffff, "time_split_span_samples out of range")},
    {"time_split_ff_cost_permille", RW, &Options::split_ff_permille, range(0, 1000, "time_split_ff_cost_permille must be 0 .. 1000")},
    {"composite_launches", RW, &Options::composite_option, flag},
    {"row_groups", RW, &Options::row_groups_option, range(0, 2, "row_groups must be 0 (off), 1 (by cost) or 2 (always)")},
    {"ragged_plan", RW, &Options::ragged_option, flag},
    {"two_waves_per_simd", RW, &Options::two_waves_option, flag},
    {"packed_launch_order", RW, &Options::packed_option, flag},
    {"sort_by_length", RW, &Options::sort_option, flag},           // applies to batches uploaded afterwards
    // plan for so many compute units; 0, set or read: the device's own count is in force
    {"assume_compute_units", RW,
     {[](const grail_ctx *ctx) -> int64_t { return ctx->cus == ctx->device_cus ? 0 : ctx->cus; },
      [](grail_ctx *ctx, int64_t value) { ctx->cus = value ? (int)value : ctx->device_cus; }},
     range(0, 4096, "assume_compute_units must be 0 (the device's) .. 4096")},
#ifdef GRAIL_SCAN_DEBUG
    {"scan_debug", WO, &Options::scan_debug, {}},                  // development builds only: see scan_kernels.hip
#endif
    {"compute_units", RO, GETTER(ctx->cus), {}},                   // what the launch policy plans for
    // the tier "arithmetic" = 1 gets for the voice table as a whole: 1 interpolating, 2 exact coefficients, 0 exact kernels
    {"fast_arithmetic_served", RO, GETTER(fast_tier_for(ctx, nullptr, 1)), {}},
    {"last_launch_fast", RO, GETTER(ctx->stats.last_fast), {}},
    {"last_launch_blocks", RO, GETTER(ctx->stats.last_blocks), {}},
    {"last_launch_formants", RO, GETTER(ctx->stats.last_formants), {}},   // 4 or 8 laid out over the lanes
    {"last_launch_lanes", RO, GETTER(ctx->stats.last_lanes), {}},
    {"last_launch_pipelined", RO, GETTER(ctx->stats.last_pipe), {}},
    {"last_launch_chunks", RO, GETTER(ctx->stats.last_split), {}},
    {"last_launch_packed", RO, GETTER(ctx->stats.last_packed), {}},
    {"slow_division_wave_steps", RO, GETTER(ctx->stats.slow_steps), {}},
    {"fast_wave_tiles", RO, GETTER(ctx->stats.fast_tiles), {}},           // wave-tiles rendered in fast arithmetic
    {"general_wave_steps", RO, GETTER(ctx->stats.general_steps), {}},     // wave-steps through the general step
};

#undef GETTER

const Row *find(const char *name)
{
    for (const Row &r : TABLE)
        if (std::strcmp(name, r.name) == 0) return &r;
    return nullptr;
}

}  // namespace

extern "C" {

int grail_set_option(grail_ctx *ctx, const char *name, int64_t value)
{
    if (!ctx || !name) return fail(GRAIL_ERR_INVALID_ARG, "NULL argument");
    ++ctx->options_epoch;             // (before the checks: a refused value and an unknown name count too)
    const Row *r = find(name);
    if (!r || r->access == RO) return fail(GRAIL_ERR_INVALID_ARG, std::string("unknown option ") + name);
    const Check &c = r->check;
    bool ok = true;
    switch (c.kind) {
    case ANY: break;
    case FLAG: value = value ? 1 : 0; break;
    case RANGE: ok = value >= c.lo && value <= c.hi; break;
    case AT_LEAST: ok = value >= c.lo; break;
    case LANES: ok = value == 0 || value == 1 || value == 2 || value == 4 || value == 8; break;
    }
    if (!ok) return fail(GRAIL_ERR_INVALID_ARG, c.error);
    if (r->where.set) r->where.set(ctx, value);
    else ctx->opt.*r->where.field = value;
    return GRAIL_OK;
}

int grail_get_option(grail_ctx *ctx, const char *name, int64_t *value)
{
    if (!ctx || !name || !value) return fail(GRAIL_ERR_INVALID_ARG, "NULL argument");
#ifdef GRAIL_FAST_PROF
    if (std::strncmp(name, "debug_prof_", 11) == 0) {          // debug builds: counter k of the tolerance-mode tile loop
        const int k = std::atoi(name + 11);
        if (k < 0 || k >= 32) return fail(GRAIL_ERR_INVALID_ARG, "debug_prof_<k>: k in 0 .. 31");
        unsigned long long v = 0;
        HIP_TRY(hipStreamSynchronize(ctx->stream));
        HIP_TRY(hipMemcpy(&v, reinterpret_cast<unsigned long long *>(ctx->d_truncated.get() + 8) + k, sizeof v, hipMemcpyDeviceToHost));
        *value = (int64_t)v;
        return GRAIL_OK;
    }
#endif
    const Row *r = find(name);
    if (!r || r->access == WO) return fail(GRAIL_ERR_INVALID_ARG, std::string("unknown option ") + name);
    *value = r->where.get ? r->where.get(ctx) : ctx->opt.*r->where.field;
    return GRAIL_OK;
}

}  // extern "C"
