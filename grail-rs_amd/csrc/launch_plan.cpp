// launch_plan.cpp — how a batch is cut into blocks with a kernel family each (family_choice.cpp chooses them,
// family_cost.cpp prices them), and the two entry points that preview a plan.
// Pure host arithmetic over what a context plans with (PlanEnv) and a batch's summary (BatchFacts); no HIP call, no type
// that owns device memory: grail_plan_blocks runs it without a device.
#include "api_internal.hpp"

using namespace grail;
using namespace grail::host;

namespace grail {
namespace host {

// Cut `rows` rows into blocks, each rendered by the family that suits ITS size, so that the time of a batch is not a
// step function of its size: a family fills the machine with a fixed number of rows (one wave per SIMD), one row more
// costs a whole further round of it — 65 537 utterances took two rounds of the one-lane kernel (81 ms) where one
// round and a pipelined workgroup launch (40.6 + 6.5 ms) do.  Candidates: the whole of it in one launch; or a full
// block of one of the families' capacities (as many rounds as fit for the one-lane kernels) followed by the best
// plan for the rest.  Exact arithmetic is mapping-invariant, so the cut never changes a bit; in fast arithmetic a row's
// samples follow the family of ITS block (include/grail_hip.h, "Determinism contract").
struct Planner {
    const PlanEnv *ctx;
    const BatchFacts *batch;
    uint64_t out_stride;
    double span;
    bool exact_only;                           // (the plan a fast request is weighed against: ragged_plan)
    static constexpr double LAUNCH_MS = 0.05;  // what a further launch costs by itself (measured: 0.02 - 0.06 ms)
    // (choose_family lays out time-split grids by bisection: every size is looked at once)
    std::map<uint32_t, std::pair<Family, double>> families;
    std::map<uint32_t, std::pair<double, std::vector<Block>>> plans;

    const std::pair<Family, double> &family(uint32_t rows)
    {
        auto it = families.find(rows);
        if (it != families.end()) return it->second;
        std::pair<Family, double> e;
        choose_family(ctx, batch, out_stride, rows, e.first, exact_only);
        e.second = family_cost(ctx, e.first, rows, span);
        return families.emplace(rows, e).first->second;
    }
    const std::pair<double, std::vector<Block>> &plan(uint32_t rows, int depth)
    {
        auto it = plans.find(rows);
        if (it != plans.end()) return it->second;
        const std::pair<Family, double> &whole = family(rows);
        double best = whole.second;
        std::vector<Block> best_plan{Block{rows, whole.first}};
        if (depth < 4) {
            const uint64_t lanes = ctx_lanes(ctx), cus = (uint64_t)ctx->cus;
            // the capacities at which some family is exactly full (largest first: of two plans of equal cost the
            // one with the larger head wins)
            const uint64_t caps[] = {lanes, lanes / 2, lanes / 4, lanes / 8, 32 * cus, 16 * cus, 8 * cus};
            uint64_t seen = 0;
            for (const uint64_t c : caps) {
                if (c == 0 || c >= rows || c == seen) continue;
                seen = c;
                const uint32_t m = c == lanes ? (uint32_t)(rows / c) : 1u;
                const uint32_t head = (uint32_t)(m * c);
                const std::pair<Family, double> &fc = family(head);
                if (fc.second + LAUNCH_MS >= best) continue;
                const std::pair<double, std::vector<Block>> &rest = plan(rows - head, depth + 1);
                if (fc.second + LAUNCH_MS + rest.first < best) {
                    best = fc.second + LAUNCH_MS + rest.first;
                    best_plan.assign(1, Block{head, fc.first});
                    best_plan.insert(best_plan.end(), rest.second.begin(), rest.second.end());
                }
            }
        }
        return plans.emplace(rows, std::make_pair(best, best_plan)).first->second;
    }
};

double plan_blocks(const PlanEnv *ctx, const BatchFacts *batch, uint64_t out_stride, uint32_t rows, double span,
                   std::vector<Block> &out, bool exact_only)
{
    Planner p{ctx, batch, out_stride, span, exact_only, {}, {}};
    const std::pair<double, std::vector<Block>> &best = p.plan(rows, 0);
    out = best.second;
    if (out.size() > 1) {
        // launch order: the block that is cheapest PER ROW first (in practice: the largest).  Two reasons.  Length-
        // sorted (ragged) batches hand out their slots longest first and a block lasts as long as its longest
        // utterance: with lengths falling by g per slot, moving a block of r rows and per-sample cost c behind one of
        // r', c' saves g (c r' - c' r) — the long utterances belong where a ROW costs least.  And a small block leaves
        // most of the machine idle for milliseconds: the large kernel behind it then starts on lowered clocks and
        // loses 2.5 - 3 ms (65 537 utterances: 50.3 ms with the single utterance first, profiles/r04_tail.txt).
        std::stable_sort(out.begin(), out.end(), [&](const Block &x, const Block &y) {
            return family_cost(ctx, x.f, x.rows, span) * (double)y.rows < family_cost(ctx, y.f, y.rows, span) * (double)x.rows;
        });
    }
    return best.first;
}

void ragged_plan(const PlanEnv *ctx, const BatchFacts *batch, uint64_t out_stride, uint32_t rows, std::vector<Block> &plan)
{
    if (!ctx->opt.ragged_option || batch->granule_samples.empty() || rows != batch->n_utt || plan.empty()) return;
    if (plan.size() == 1 && plan[0].f.scan) return;   // (a few utterances in fast arithmetic: the scan kernel's)
    const double span = batch_span(ctx, batch, out_stride);
    auto cost_of = [&](const std::vector<Block> &blocks) {
        double c = 0.0;
        uint32_t slot0 = 0;
        for (const Block &b : blocks) {
            c += ragged_cost(ctx, batch, b.f, slot0, b.rows, span) + Planner::LAUNCH_MS;
            slot0 += b.rows;
        }
        return c;
    };
    // GRAIL_PLAN_DEBUG=1: the candidates and their prices on stderr (development aid; read once)
    static const bool debug = [] { const char *e = getenv("GRAIL_PLAN_DEBUG"); return e && *e && *e != '0'; }();
    // (a candidate has to be worth the change: in tolerance arithmetic a row's bits follow its family, and grail_plan_blocks
    // predicts the cut by size; exact bits follow nothing, and one launch in packed order beats the same mapping cut in two)
    const double worth = ctx->opt.fast_option ? 0.95 : 0.98;
    double best = worth * cost_of(plan);
    if (debug) std::fprintf(stderr, "[ragged_plan] %u rows: the cut by size (%zu block(s)) %.2f ms\n", rows, plan.size(), best / worth);
    if (ctx->opt.fast_option) {
        // fast arithmetic asked for: the cut exact arithmetic would get stands too (small batches: the pipelined
        // workgroups) — events this dense cost the fast kernels more than they save, and exact bits satisfy the tolerance
        // trivially.  Phonemes of 16 - 64 ms, 65 536 utterances: 32 ms exact against 57 fast.
        std::vector<Block> exact;
        plan_blocks(ctx, batch, out_stride, rows, span, exact, true);
        const double c = cost_of(exact);
        if (c < best) {
            best = c;
            plan = exact;
        }
    }
    // ... the ONE launch the batch as a whole would get (choose_family weighs scan, time-split and lane kernels by the rows
    // when it is asked about the whole batch; the cut above was made block by block, by the aligned model: 6 000 speech-like
    // utterances as 4 096 + 1 904 time-split rows took 26.9 ms, the scan kernel takes 10.9)
    if (ctx->opt.fast_option) {       // (exact arithmetic: that launch is one of the lane mappings below)
        Family whole;
        choose_family(ctx, batch, out_stride, rows, whole, false);
        const double c = ragged_cost(ctx, batch, whole, 0, rows, span) + Planner::LAUNCH_MS;
        if (c < best) {
            best = c;
            plan.assign(1, Block{rows, whole});
        }
    }
    // ... and ONE launch of each lane mapping in as many rounds as it takes
    for (int exact_only = 0; exact_only <= (ctx->opt.fast_option ? 1 : 0); ++exact_only)
        for (int L = 1; L <= 8; L *= 2) {
            Family f;
            choose_family(ctx, batch, out_stride, rows, f, exact_only != 0, L);
            if (f.scan || f.pipe || f.split_k) continue;
            const double c = ragged_cost(ctx, batch, f, 0, rows, span) + Planner::LAUNCH_MS;
            if (debug)
                std::fprintf(stderr, "[ragged_plan]   one launch on %d lane(s)%s%s: %.2f ms\n", f.L, f.fast ? " fast" : " exact",
                             family_cohabits(ctx, f, rows) ? ", two waves per SIMD" : "", c);
            if (c < best) {
                best = c;
                plan.assign(1, Block{rows, f});
            }
        }
}

}  // namespace host
}  // namespace grail

extern "C" {

// grail_plan_blocks / grail_plan_ragged_blocks: row_samples == nullptr is the aligned batch
static int plan_preview(uint32_t compute_units, int arithmetic, int live_formants, uint32_t warmup, uint32_t rows,
                        uint32_t span_samples, const uint32_t *row_samples, const uint32_t *row_segments,
                        const uint32_t *row_kinks, grail_plan_block *blocks, uint32_t cap, uint32_t *n_blocks)
{
    if (!n_blocks) return fail(GRAIL_ERR_INVALID_ARG, "n_blocks is NULL");
    *n_blocks = 0;
    if (compute_units == 0 || compute_units > 4096) return fail(GRAIL_ERR_INVALID_ARG, "compute_units must be 1 .. 4096");
    if (live_formants != 4 && live_formants != 8) return fail(GRAIL_ERR_INVALID_ARG, "live_formants must be 4 or 8");
    if (arithmetic != 0 && arithmetic != 1 && arithmetic != 2) return fail(GRAIL_ERR_INVALID_ARG, "arithmetic must be 0, 1 or 2");
    if (rows == 0) return GRAIL_OK;
    // a context and a batch as choose_family sees them: default options, a voice table that qualifies for every
    // family (four or eight live formants), a plain phoneme batch with power-of-two blend lengths
    PlanEnv ctx;
    ctx.cus = (int)compute_units;
    ctx.opt.fast_option = arithmetic;
    VoiceFacts &facts = ctx.facts;
    facts.voices_sharpness = 0.0;
    facts.voices_upper_silent = facts.voices_live4_ok = live_formants == 4;
    facts.voices_scan_ok = true;
    facts.voices_split_ok = warmup != 0u;
    facts.max_warmup = warmup;
    facts.max_rate = 1.0f;                // max_seconds below is in samples
    facts.max_dt = 1.0f;
    BatchFacts batch;
    batch.n_utt = rows;
    batch.phoneme_mode = true;
    batch.plain = true;
    batch.max_seconds = (float)span_samples;
    batch.min_length = 1e9f;
    batch.min_pitch = 0.25f;
    if (row_samples) {
        batch.len_bound_known = true;        // (what upload_len_bound keeps)
        // (what upload_length_order keeps of a length-sorted batch)
        const size_t n_gran = ((size_t)rows + 7) / 8;
        batch.granule_samples.assign(n_gran, 0.0f);
        batch.granule_segs.assign(n_gran, 0u);
        batch.granule_kinks.assign(n_gran, 0u);
        for (uint32_t s = 0; s < rows; ++s) {
            batch.granule_samples[s / 8] = std::fmax(batch.granule_samples[s / 8], (float)row_samples[s]);
            batch.granule_segs[s / 8] += row_segments ? row_segments[s] : 0u;
            batch.granule_kinks[s / 8] += row_kinks ? row_kinks[s] : 0u;
        }
    }
    const uint64_t stride = ((uint64_t)span_samples + 64u + 63u) / 64u * 64u;
    std::vector<Block> plan;
    plan_blocks(&ctx, &batch, stride, rows, batch_span(&ctx, &batch, stride), plan);
    ragged_plan(&ctx, &batch, stride, rows, plan);
    *n_blocks = (uint32_t)plan.size();
    uint32_t slot0 = 0;
    for (uint32_t i = 0; i < plan.size(); ++i) {
        const Family &f = plan[i].f;
        if (i < cap && blocks) {
            blocks[i].rows = plan[i].rows;
            blocks[i].lanes_per_utterance = f.scan ? 0u : (uint32_t)f.L;
            blocks[i].pipelined = f.scan ? 0u : f.pipe;
            blocks[i].chunks = (uint32_t)f.split_k;
            blocks[i].scan = f.scan ? (f.scan_pipe ? 2u : 1u) : 0u;
            blocks[i].fast = f.fast;
            blocks[i].formants = f.live4 ? 4u : 8u;
            blocks[i].model_ms = (float)ragged_cost(&ctx, &batch, f, slot0, plan[i].rows, batch_span(&ctx, &batch, stride));
        }
        slot0 += plan[i].rows;
    }
    return GRAIL_OK;
}

int grail_plan_blocks(uint32_t compute_units, int arithmetic, int live_formants, uint32_t warmup, uint32_t rows,
                      uint32_t span_samples, grail_plan_block *blocks, uint32_t cap, uint32_t *n_blocks)
{
    return plan_preview(compute_units, arithmetic, live_formants, warmup, rows, span_samples, nullptr, nullptr, nullptr,
                        blocks, cap, n_blocks);
}

int grail_plan_ragged_blocks(uint32_t compute_units, int arithmetic, int live_formants, uint32_t warmup, uint32_t rows,
                             const uint32_t *row_samples, const uint32_t *row_segments, const uint32_t *row_kinks,
                             grail_plan_block *blocks, uint32_t cap, uint32_t *n_blocks)
{
    if (n_blocks) *n_blocks = 0;
    if (rows && !row_samples) return fail(GRAIL_ERR_INVALID_ARG, "row_samples is NULL");
    uint32_t span = 0;
    for (uint32_t s = 0; s < rows; ++s) span = std::max(span, row_samples[s]);
    return plan_preview(compute_units, arithmetic, live_formants, warmup, rows, span, row_samples, row_segments, row_kinks,
                        blocks, cap, n_blocks);
}

}  // extern "C"
