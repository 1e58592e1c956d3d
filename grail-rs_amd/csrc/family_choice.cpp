// family_choice.cpp — which kernel family a block of rows may take and takes: what a batch qualifies for (four-formant
// kernels, the half-live loops), the exact family, the time-split and scan candidates of fast arithmetic, the choice among
// them.  Prices are family_cost.cpp's.  Pure host arithmetic over PlanEnv and BatchFacts.
#include "api_internal.hpp"

using namespace grail;
using namespace grail::host;

namespace grail {
namespace host {

int auto_lanes_per_utt(uint32_t n_utt, uint64_t simds)
{
    // Measured (profiles/r01_lanes_sweep.txt): a wave alone on its SIMD renders 2 s of audio
    // in 92 / 60 / 42 / 38 ms for L = 1 / 2 / 4 / 8, and a second wave on the same SIMD costs
    // more than it brings (the packed-f32 stream of one wave already keeps the VALU ~80 %
    // busy).  So: the widest mapping that still fits one wave per SIMD (4 per compute unit: 1024 on a
    // whole MI355X).
    for (int L = 8; L > 1; L /= 2)
        if (((uint64_t)n_utt * L + 63) / 64 <= simds) return L;
    return 1;
}

// A phoneme batch is judged by the voices IT names (batch->used_voices), not by the whole table: a preset with eight
// live formants somewhere in the table does not take the four-formant kernels away from batches that never use it.
// (A context without per-voice records — grail_plan_blocks — goes by the table-wide flag.)
template <typename Pred>
static bool used_voices_all(const PlanEnv *ctx, const BatchFacts *batch, bool table_wide, Pred pred)
{
    if (ctx->facts.voice_info.empty() || batch->used_voices.empty()) return table_wide;
    for (const uint32_t v : batch->used_voices)
        if (v >= ctx->facts.voice_info.size() || !pred(ctx->facts.voice_info[v])) return false;
    return true;
}
bool batch_half_capable(const PlanEnv *ctx, const BatchFacts *batch)
{
    // (caller-built elems: judged at upload over the batch's distinct elems, against the voice table of that moment)
    if (!batch->phoneme_mode)
        return ctx->opt.skip_silent_option && batch->elems_live4_ok && batch->elems_warmup_epoch == ctx->voices_epoch;
    return ctx->opt.skip_silent_option &&
           used_voices_all(ctx, batch, ctx->facts.voices_upper_silent, [](const VoiceInfo &v) { return v.upper_silent; });
}

// formants 5-8 left out altogether: the table qualifies (live4_ok); every segment is at least
// two samples long, so the Sequencer clock never goes negative and alpha stays in [0,1]; and
// every pitch stays >= 2^-20 under the pitch jitter, so the polyBLEP quotient and with it the
// saw every formant is fed from stay finite (a dead formant fed +-inf would emit NaN)
bool batch_live4_any_blend(const PlanEnv *ctx, const BatchFacts *batch)
{
    return batch_half_capable(ctx, batch) &&
           (!batch->phoneme_mode ||
            used_voices_all(ctx, batch, ctx->facts.voices_live4_ok, [](const VoiceInfo &v) { return v.live4_ok; })) &&
           batch->plain && lean_window(batch->min_length, batch->min_pitch, ctx->facts);
}
// ... and (the lane kernels' four-formant instantiations) every blend length a power of two
bool batch_live4(const PlanEnv *ctx, const BatchFacts *batch)
{
    return batch_live4_any_blend(ctx, batch) && !batch->any_blend;
}

// What choose_family works out once per call and its parts read.
struct Choice {
    const PlanEnv *ctx;
    const BatchFacts *batch;
    uint64_t out_stride;
    uint32_t fam;                 // rows of the block
    uint64_t simds, cus;
    int lanes_option;             // the option, or the call's pin_lanes (as if the option named it)
    bool rows_differ;
    bool l4ab;                    // batch_live4_any_blend
    bool want_pipe4, want_pipe8;  // the block is small enough for pipelined workgroups (four / eight formants) ...
    uint32_t pipe4_kind, pipe8_kind;   // ... with rounds of 16 samples (1) or 32 (2)
};

static Choice choice_of(const PlanEnv *ctx, const BatchFacts *batch, uint64_t out_stride, uint32_t fam, int pin_lanes)
{
    Choice c;
    c.ctx = ctx;
    c.batch = batch;
    c.out_stride = out_stride;
    c.fam = fam;
    c.simds = ctx_simds(ctx);
    c.cus = (uint64_t)ctx->cus;
    c.lanes_option = pin_lanes ? pin_lanes : ctx->opt.lanes_option;
    c.l4ab = batch_live4_any_blend(ctx, batch);
    // small batches leave SIMDs idle: four-wave workgroups (one wave renders 16 utterances, one carries
    // the per-utterance chain, two prepare the filter coefficients), up to two per CU (tools/pipe4_range.py:
    // 11.5 ms up to 4 096 utterances, 15.7 up to 8 192 where the lane kernels take 18.0; three per CU lose)
    c.want_pipe4 = c.l4ab && !c.lanes_option && ctx->opt.pipeline_option &&
                   (int64_t)(((uint64_t)fam + 15) / 16) <= pipe4_groups(ctx);
    c.want_pipe8 = !c.l4ab && !c.lanes_option && ctx->opt.pipeline_option &&
                   (int64_t)(((uint64_t)fam + 7) / 8) <= pipe8_groups(ctx);
    // one workgroup per CU suffices: rounds of 32 samples instead of 16 (pipe = 2) — for batches whose rows are aligned.
    // Rows that differ in length (the upload kept their summary) have their events at times of their own, and a tile with an
    // event is rendered in whole rounds where nobody has one (synth_kernel.h pipe_rounds): rounds of 16 fit between two events
    // far more often than rounds of 32 (256 speech-like utterances 18.8 ms against 20.0, with phonemes of 16 - 64 ms 10.0 / 11.2,
    // 4 - 16 ms 4.6 / 5.3; profiles/r05_mixed_runs.txt)
    c.rows_differ = rows_differ(batch);
    const bool round32 = ctx->opt.pipe_round32 == 2 || (ctx->opt.pipe_round32 == 1 && !c.rows_differ);      // (2: tests, A/B)
    c.pipe4_kind = round32 && ((uint64_t)fam + 15) / 16 <= c.cus ? 2u : 1u;
    c.pipe8_kind = round32 && ((uint64_t)fam + 7) / 8 <= c.cus ? 2u : 1u;
    return c;
}

// The family of the lane kernels and pipelined workgroups: the widest mapping that still gives every SIMD at most one wave.
// What exact arithmetic takes; in fast arithmetic (f.fast != 0) the candidate the scan and time-split kernels are weighed
// against.
static Family lane_family(const Choice &c, bool exact_only)
{
    const PlanEnv *ctx = c.ctx;
    const BatchFacts *batch = c.batch;
    Family f;
    // (the lane kernels and the pipelined workgroups have four-formant instantiations for every blend length; the lean
    // stream kernels for power-of-two blend lengths only: batch_live4)
    f.live4 = c.l4ab ? 1u : 0u;
    // fast arithmetic is served up to a sharpness of the resonances (elems_sharpness); beyond it the exact kernels run
    // ... in the tier the sharpness allows: 1 = coefficients interpolated, 2 = the reference's own coefficients (MID)
    f.fast = exact_only ? 0u : (uint32_t)fast_tier(ctx, batch);
    // (MID kernels exist one-shot with one lane per utterance, and time-split: a pinned wider mapping gets the exact kernels)
    if (f.fast == 2u && c.lanes_option > 1) f.fast = 0u;
    int L = c.lanes_option ? c.lanes_option : auto_lanes_per_utt(c.fam, c.simds);
    if (f.fast == 2u) L = 1;          // (before the four-formant layout is decided: eight lanes would give it up)
    if (c.want_pipe4 && !f.fast) {
        f.pipe = c.pipe4_kind;
        L = 4;
    } else if (c.want_pipe8 && !f.fast) {
        f.pipe = c.pipe8_kind;                            // eight formants: 8 utterances per workgroup
        L = 8;
    }
    // eight lanes per utterance need eight formants to lay out; for batches that small the
    // 8-lane kernel is also the fastest (18.2 against 18.8 ms: half the rows to flush per wave)
    if (f.live4 && !f.pipe && L == 8) f.live4 = 0u;
    if (f.live4 && !f.pipe && !c.lanes_option) {
        // same rule as auto_lanes_per_utt — the widest mapping with one wave per SIMD — over 4 formants
        L = ((uint64_t)c.fam * 4 + 63) / 64 <= c.simds ? 4 : ((uint64_t)c.fam * 2 + 63) / 64 <= c.simds ? 2 : 1;
    }
    // voices whose upper formants are never audible but that do not qualify for the 4-formant
    // kernels: one lane per utterance runs the half-live loop and ties two lanes per utterance,
    // whose second lane would only hold silent formants
    if (!c.lanes_option && !f.live4 && L == 2 && batch_half_capable(ctx, batch)) L = 1;
    f.L = L;
    f.half = !f.fast && !f.live4 && !f.pipe && L == 1 && batch_half_capable(ctx, batch);
    return f;
}

// Rows that differ in length (whole batch, launched longest first, the upload's length bounds on the device): a
// chunk's wave whose utterances all end before the chunk begins is gone at once (synth_kernel.h, SPLIT), so the
// grid may hold more (wave, chunk) pairs than the device has SIMDs (a speech-like corpus keeps a third of them: the
// grid's chunks are shortest at the far end, where only the longest rows still are)
static uint64_t active_pairs(const BatchFacts *batch, const uint32_t *bounds, const int k)
{
    uint64_t pairs = 0;
    for (size_t g = 0; g < batch->granule_samples.size(); g += 8) {      // 64 launch slots: the first is the longest
        const double len = (double)batch->granule_samples[g] * 1.02 + 64.0;
        int c = 1;
        while (c < k && (double)bounds[c] < len) ++c;
        pairs += (uint64_t)c;
    }
    return pairs;
}

// fast arithmetic, mid-size batches: one lane per utterance would leave most of the machine idle, so the time
// axis of every utterance is cut into chunks with a lane each (synth_kernel<..., SPLIT>): as many chunks as
// fill the machine, laid out over the batch's longest utterance so that all lanes finish together.
// The lane family with its grid, or (split_k == 0) the lane family as it is: the batch takes no time-split kernel.
static Family split_candidate(const Choice &c, const Family &lane, double span)
{
    const PlanEnv *ctx = c.ctx;
    const BatchFacts *batch = c.batch;
    const uint64_t out_stride = c.out_stride;
    const uint32_t fam = c.fam;
    Family split = lane;
    // (which voices / elems qualify: voice_warmup.  A phoneme batch is covered by its voice table; caller-built elems
    // by the warm-up computed over them at upload, against the voice table of that moment)
    const bool split_ok = batch->phoneme_mode ? used_voices_all(ctx, batch, ctx->facts.voices_split_ok,
                                                                [](const VoiceInfo &v) { return v.split_ok; })
                                              : (batch->elems_warmup != 0u && batch->elems_warmup_epoch == ctx->voices_epoch);
    // (the grid is laid out for the longest warm-up of the TABLE, not of the voices the batch names: for a pinned grid an
    // utterance's samples may not depend on what else is in the batch; each lane still warms up for its own voice's length)
    const uint32_t warmup = batch->phoneme_mode ? ctx->facts.max_warmup : batch->elems_warmup;
    if (!(ctx->opt.split_option && !c.lanes_option && split_ok && batch->plain &&
          out_stride <= 0xFFFFFFFFull && (ctx->opt.split_chunks >= 2 || ctx->opt.split_chunks == 0)))
        return split;
    const double sp = ctx->opt.split_span ? std::fmin((double)ctx->opt.split_span, (double)out_stride) : span;
    // as many chunks as give every SIMD one wave: ceil(fam / 64) waves per chunk index (5 000 utterances are 79 waves
    // per chunk: 12 chunks, not 65 536 / 5 000 = 13, which would be 1 027 waves and a second round for three of them)
    int K = ctx->opt.split_chunks ? (int)ctx->opt.split_chunks
                              : (int)std::min<uint64_t>(c.simds / (((uint64_t)fam + 63u) / 64u), SPLIT_MAX_CHUNKS);
    const bool by_length = !ctx->opt.split_chunks && !ctx->opt.split_span && c.rows_differ && fam == batch->n_utt &&
                           batch->len_bound_known && batch->len_bound_epoch == ctx->voices_epoch;
    K = (int)std::fmin((double)K, sp / 512.0);
    // (a fast-forwarded sample costs the same whatever is rendered afterwards; a rendered sample of eight live
    // formants costs 1.5 x one of four; 0.8 from a sweep, profiles/r03_small_batch.txt)
    const double ff_cost = 1e-3 * (double)ctx->opt.split_ff_permille * (c.l4ab ? 1.0 : 0.8) * (lane.fast == 2u ? 0.6 : 1.0);
    // the largest K <= K whose chunks fit (a chunk must render at least a tile): fitting is monotone in K
    if (K >= 2 && !split_grid((uint32_t)sp, warmup, K, ff_cost, split.split_bounds)) {
        int lo = 1, hi = K;                  // lo fits (or is 1), hi does not
        while (hi - lo > 1) {
            const int mid = (lo + hi) / 2;
            if (split_grid((uint32_t)sp, warmup, mid, ff_cost, split.split_bounds)) lo = mid;
            else hi = mid;
        }
        K = lo;
        if (K >= 2) (void)split_grid((uint32_t)sp, warmup, K, ff_cost, split.split_bounds);
    }
    if (K >= 2 && K <= 4 && by_length) {
        // (Batches of 16 384 utterances and more, whose grids are coarse — 4 chunks, 2 — and leave SIMDs without a wave:
        // up to 2 K - 1 chunks while the active pairs fit the device.  The count is an estimate from the upload's summary
        // — measured 6 % above what the kernel finds — and finer grids of smaller batches gain nothing: a chunk's lane
        // fast-forwards through everything before it, and on a speech-like corpus that costs more per sample than the
        // grid is laid out for: 4 096 utterances 15.4 ms on 16 chunks, 14.9 on 24, 19.6 on 34.)
        const int most = 2 * K - 1;
        for (int k = K + 1; k <= most && (double)k <= sp / 512.0; ++k) {
            uint32_t wider[SPLIT_MAX_CHUNKS + 1] = {};
            if (!split_grid((uint32_t)sp, warmup, k, ff_cost, wider) || active_pairs(batch, wider, k) * 16 > c.simds * 17) break;
            K = k;
            std::memcpy(split.split_bounds, wider, sizeof wider);
        }
    }
    if (K >= 2) {
        split.split_k = K;
        split.split_active = by_length ? (uint32_t)active_pairs(batch, split.split_bounds, K) : 0u;
        split.split_bounds[K] = (uint32_t)out_stride;
        split.live4 = c.l4ab ? 1u : 0u;
        split.pipe = 0u;
        split.L = 1;
    }
    return split;
}

// fast arithmetic, few utterances: one workgroup per utterance with the time axis across the lanes and the
// filter recurrences solved by parallel scans (scan_kernels.hip).  Needs every parameter inside the safe window
// (no IEEE fallback).  The lane family as a scan launch, or (scan == false) as it is.
static Family scan_candidate(const Choice &c, const Family &lane)
{
    const PlanEnv *ctx = c.ctx;
    const BatchFacts *batch = c.batch;
    Family scan = lane;
    // (rows that differ in length, option "ragged_plan": up to 64 workgroups per compute unit — there the cost model decides,
    // by the rows: 10 000 speech-like utterances 15.3 ms against 19.1 time-split, with phonemes of 16 - 64 ms 7.0 / 13.5)
    const int64_t scan_limit = ctx->opt.scan_max_utts < 0 && ctx->opt.ragged_option && c.rows_differ && c.fam == batch->n_utt
                                   ? 64 * (int64_t)ctx->cus : scan_max_utts(ctx);
    if (lane.fast == 1u && ctx->opt.scan_option && !c.lanes_option && (int64_t)c.fam * (c.l4ab ? 4 : 7) <= 4 * scan_limit &&
        used_voices_all(ctx, batch, ctx->facts.voices_scan_ok, [](const VoiceInfo &v) { return v.scan_ok; }) &&
        (batch->phoneme_mode || (batch->elems_scan_ok && batch->elems_warmup_epoch == ctx->voices_epoch)) &&
        batch->plain && lean_window(batch->min_length, batch->min_pitch, ctx->facts)) {
        scan.scan = true;
        scan.live4 = c.l4ab ? 1u : 0u;                        // (the scan kernel takes any blend length)
        // three-stage workgroups for few utterances (tools/scan_split_crossover.py: up to ~1500 with four
        // live formants, half that with eight, where the filter wave is the slower stage either way)
        scan.scan_pipe = (int64_t)c.fam * (scan.live4 ? 1 : 2) <= scan_split_max(ctx) ? 1u : 0u;
        scan.pipe = 0u;
    }
    return scan;
}

// Which of the three: a pinned grid or an explicit "time_split_min_utterances" decide as they always did; otherwise
// the cost model does (2 s utterances: the scan kernel up to ~1 500 of them, the time-split kernels up to half the
// machine's lanes, the lane kernels beyond; shorter utterances move the first crossover up — a chunk's warm-up
// does not shrink with the utterance).  Returns one of its three arguments.
static const Family &cheapest_family(const Choice &c, const Family &lane, const Family &split, const Family &scan, double span)
{
    const PlanEnv *ctx = c.ctx;
    const BatchFacts *batch = c.batch;
    const uint32_t fam = c.fam;
    bool take_split = false, take_scan = false;
    if (split.split_k && ctx->opt.split_chunks >= 2) {
        take_split = true;
    } else if (ctx->opt.split_min_utts >= 0) {
        take_split = split.split_k && (int64_t)fam * 6 >= ctx->opt.split_min_utts * (c.l4ab ? 6 : 5);
        take_scan = !take_split && scan.scan;
    } else {
        double c_lane = family_cost(ctx, lane, fam, span);
        double c_split = split.split_k ? family_cost(ctx, split, fam, span) : INFINITY;
        double c_scan = scan.scan ? family_cost(ctx, scan, fam, span) : INFINITY;
        if (ctx->opt.ragged_option && c.rows_differ && fam == batch->n_utt) {
            // Rows that differ in length (the whole batch, its summary from the upload; part of option "ragged_plan"): the three
            // families part ways.  The
            // scan kernel gives every utterance a workgroup of its own — what a compute unit works off is the SUM of its
            // utterances' lengths, whatever their spread, and an event costs a workgroup next to nothing (lanes are time) —
            // while a time-split lane fast-forwards through the events of 64 utterances and waits for the longest of them:
            // 4 096 speech-like utterances 6.7 ms on the scan kernel, 15.5 time-split (aligned: 6.4 against 3.3); with
            // phonemes of 16 - 64 ms 3.2 against 11.2.  Priced by the rows: mean length for the scan kernel (at least one
            // workgroup's way through the longest row), lengths and events (ragged_cost) for the other two.
            double mean = 0.0;
            for (const float g : batch->granule_samples) mean += (double)g;
            mean /= (double)batch->granule_samples.size();
            if (scan.scan) c_scan = std::fmax(family_cost(ctx, scan, fam, std::fmin(mean + 64.0, span)), family_cost(ctx, scan, 1u, span));
            if (split.split_k) c_split = ragged_cost(ctx, batch, split, 0u, fam, span);
            c_lane = ragged_cost(ctx, batch, lane, 0u, fam, span);
        }
        take_split = c_split <= c_scan && c_split < c_lane;
        take_scan = !take_split && c_scan < c_lane;
    }
    return take_split ? split : take_scan ? scan : lane;
}

// The second tier costs 0.8 of the exact one-lane kernel (0.64 - 0.8 time-split): where the exact kernels have a
// wider mapping to fill the machine with — mid-size batches of voices that do not qualify for time-splitting —
// they are the faster way to the same tolerance (their bits satisfy it trivially).
static void mid_against_exact(const Choice &c, Family &f, double span)
{
    const Family exact = lane_family(c, true);
    if (family_cost(c.ctx, exact, c.fam, span) <= family_cost(c.ctx, f, c.fam, span)) f = exact;
}

// fast arithmetic asked for, but the batch takes neither the scan kernel nor the time-split kernels (caller-built
// elems, a voice outside their windows, an option switched off) and is small enough for the pipelined exact
// workgroups: those are faster than the fast lane kernels there (8.1 - 11.5 against 12.4 ms), and exact bits
// satisfy the tolerance trivially
static void pipelined_fallback(const Choice &c, Family &f)
{
    if (c.want_pipe4 || c.want_pipe8) {
        f.fast = 0u;
        f.live4 = c.l4ab ? 1u : 0u;
        f.pipe = c.want_pipe4 ? c.pipe4_kind : c.pipe8_kind;
        f.L = c.want_pipe4 ? 4 : 8;
    }
}

// The family a block of `fam` rows of this batch takes.  Exact arithmetic: the widest mapping that still gives every
// SIMD at most one wave (pipelined workgroups, then 8 / 4 / 2 / 1 lanes per utterance).  Fast arithmetic: the cheapest
// of the scan kernel, the time-split kernels and the fast lane kernels by the cost model (which follows the
// utterances' length: a time-split pays a warm-up per chunk, the scan kernel the latency of one utterance's chain),
// unless an option pins the choice.
void choose_family(const PlanEnv *ctx, const BatchFacts *batch, uint64_t out_stride, uint32_t fam, Family &f,
                   bool exact_only, int pin_lanes)
{
    const Choice c = choice_of(ctx, batch, out_stride, fam, pin_lanes);
    const Family lane = lane_family(c, exact_only);
    f = lane;
    if (!f.fast) return;
    const double span = batch_span(ctx, batch, out_stride);
    const Family split = split_candidate(c, lane, span), scan = scan_candidate(c, lane);
    f = cheapest_family(c, lane, split, scan, span);
    if (f.fast == 2u && !c.lanes_option && ctx->opt.split_chunks < 2) {
        mid_against_exact(c, f, span);
        return;
    }
    if (!f.split_k && !f.scan) pipelined_fallback(c, f);
}

}  // namespace host
}  // namespace grail
