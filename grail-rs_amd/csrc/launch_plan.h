// launch_plan.h — the launch policy's functions: which kernel family renders a block of rows (family_choice.cpp), what it
// costs (family_cost.cpp), the measured workgroup dispatcher and the packed order (dispatch_model.cpp), how a batch is cut
// into blocks (launch_plan.cpp).  Included by api_internal.hpp, below the types these read (PlanEnv, BatchFacts, Family,
// Block); pure host arithmetic, no HIP call.
#pragma once

namespace grail {
namespace host {

// the SIMDs and lanes the policy plans for: 4 SIMDs per compute unit, 64 lanes per wavefront.  Every family is laid out
// for ONE resident wave per SIMD (a second wave on a SIMD costs as much as it brings: profiles/r01_lanes_sweep.txt), so
// all capacities below are multiples of the compute-unit count hipGetDeviceProperties reports (a partitioned MI355X —
// CPX, 32 CUs — plans for 32, not 256); "assume_compute_units" overrides it for tests.
inline uint64_t ctx_simds(const PlanEnv *ctx) { return 4ull * (uint64_t)ctx->cus; }
inline uint64_t ctx_lanes(const PlanEnv *ctx) { return 256ull * (uint64_t)ctx->cus; }
inline int64_t pipe4_groups(const PlanEnv *ctx) { return ctx->opt.pipe4_max_groups < 0 ? 2 * (int64_t)ctx->cus : ctx->opt.pipe4_max_groups; }
inline int64_t pipe8_groups(const PlanEnv *ctx) { return ctx->opt.pipe8_max_groups < 0 ? 2 * (int64_t)ctx->cus : ctx->opt.pipe8_max_groups; }
inline int64_t scan_max_utts(const PlanEnv *ctx) { return ctx->opt.scan_max_utts < 0 ? 34 * (int64_t)ctx->cus : ctx->opt.scan_max_utts; }
inline int64_t scan_split_max(const PlanEnv *ctx) { return ctx->opt.scan_split_max < 0 ? 6 * (int64_t)ctx->cus : ctx->opt.scan_split_max; }

// ---- what several of the units (and grail_api.cpp, synthesize.cpp) compute alike
// rows that differ in length: the upload kept their summary, longest first
inline bool rows_differ(const BatchFacts *batch)
{
    return batch != nullptr && !batch->granule_samples.empty() &&
           batch->granule_samples.front() != batch->granule_samples.back();
}
// the lean families' window over a batch's (or a row's) shortest segment and lowest pitch: every segment at least two samples
// long, every pitch >= 2^-20 under the pitch jitter (batch_live4_any_blend says why)
inline bool lean_window(float min_length, float min_pitch, const VoiceFacts &facts)
{
    return min_length >= 2.0f * facts.max_dt &&
           min_pitch * window::MARGIN_DOWN - window::JITTER_MARGIN * facts.max_pitch_jitter >= window::X_LO;
}
// the granules [g0, g1) of launch slots [slot0, slot0 + rows) of a batch that has granules
struct GranuleRange {
    size_t g0, g1;
};
inline GranuleRange granule_range(const BatchFacts *batch, uint32_t slot0, uint32_t rows)
{
    const size_t n_gran = batch->granule_samples.size();
    return {std::min<size_t>(slot0 / 8, n_gran - 1), std::min<size_t>(((size_t)slot0 + rows + 7) / 8, n_gran)};
}
// granules (8 launch slots) that a wave of a lane kernel holds
inline size_t granules_per_wave(const Family &f) { return (size_t)(8 / f.L > 0 ? 8 / f.L : 1); }
// a lane kernel's workgroup: its waves and the rows it renders
struct WorkgroupShape {
    uint32_t waves, rows;
};
inline WorkgroupShape workgroup_shape(const Family &f)
{
    const uint32_t waves = f.L >= 4 ? 4u : 1u;
    return {waves, (64u / (uint32_t)f.L) * waves};
}
// rounds of a time-split launch (a wave holds 64 utterances at ONE chunk index: ceil(rows / 64) waves per chunk, whatever
// rows modulo 64 is; rows that differ in length: the (wave, chunk) pairs that have anything to render)
inline double split_rounds(const PlanEnv *ctx, const Family &f, uint32_t rows)
{
    return f.split_active ? std::ceil((double)f.split_active / (double)ctx_simds(ctx))
                          : std::ceil(std::ceil((double)rows / 64.0) * f.split_k / (double)ctx_simds(ctx));
}

// ---- family_choice.cpp
// lanes per utterance when the option is 0 (auto): the widest mapping that gives each of `simds` SIMDs at most one wave
int auto_lanes_per_utt(uint32_t n_utt, uint64_t simds);
bool batch_half_capable(const PlanEnv *ctx, const BatchFacts *batch);
bool batch_live4_any_blend(const PlanEnv *ctx, const BatchFacts *batch);
bool batch_live4(const PlanEnv *ctx, const BatchFacts *batch);
void choose_family(const PlanEnv *ctx, const BatchFacts *batch, uint64_t out_stride, uint32_t fam, Family &f,
                   bool exact_only = false, int pin_lanes = 0);

// ---- family_cost.cpp
double batch_span(const PlanEnv *ctx, const BatchFacts *batch, uint64_t out_stride);
double family_cost(const PlanEnv *ctx, const Family &f, uint32_t rows, double span);
// pipelined workgroups, rows that differ in length: utterances per workgroup of a launch of `rows` rows (0: every slot)
uint32_t pipe_fill_for(const PlanEnv *ctx, const BatchFacts *batch, const Family &f, uint32_t rows);
// a launch of `rows` rows with family f takes the instantiations built for two waves per SIMD (SynthArgs::cohabit)
bool family_cohabits(const PlanEnv *ctx, const Family &f, uint32_t rows);
// what the wave of granules [g, min(g + per_wave, g1)) costs a lane kernel: its longest row, its rows' events
double ragged_wave_cost(const BatchFacts *batch, const Family &f, size_t g, size_t per_wave, size_t g1, double span);
// ragged batches: what a block costs given the lengths and events of ITS rows
double ragged_cost(const PlanEnv *ctx, const BatchFacts *batch, const Family &f, uint32_t slot0, uint32_t rows, double span);

// ---- dispatch_model.cpp
// The launch order of the workgroups of such a block (one wave per SIMD, more workgroups than the device holds at once):
// true and order[position] = workgroup (in the plain, longest-first numbering) when the packed order is worth it by the
// dispatcher's model; *plain_ms / *packed_ms: the model's makespans.  rows_per_block: what a workgroup renders.
bool packed_launch_order(const PlanEnv *ctx, const BatchFacts *batch, const Family &f, uint32_t slot0, uint32_t rows, double span,
                         std::vector<uint32_t> *order, uint32_t *rows_per_block, double *plain_ms, double *packed_ms);

// ---- launch_plan.cpp
// ragged batches: the whole-batch plan weighed against one launch of each lane mapping with as many rounds as it takes
void ragged_plan(const PlanEnv *ctx, const BatchFacts *batch, uint64_t out_stride, uint32_t rows, std::vector<Block> &plan);
double plan_blocks(const PlanEnv *ctx, const BatchFacts *batch, uint64_t out_stride, uint32_t rows, double span,
                   std::vector<Block> &out, bool exact_only = false);

}  // namespace host
}  // namespace grail
