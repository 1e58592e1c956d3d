// family_cost.cpp — what a kernel family costs by the planner's model: a launch of aligned rows (family_cost), a block of
// rows that differ in length by ITS rows' lengths and events (ragged_cost), and what goes with the prices: which launches
// take two waves per SIMD, how thinly pipelined workgroups are filled.  Pure host arithmetic over PlanEnv and BatchFacts.
#include "api_internal.hpp"

#include <functional>
#include <queue>

using namespace grail;
using namespace grail::host;

namespace grail {
namespace host {

// the longest utterance of the batch in samples, as far as the host knows it (the f32 clock adds a few per segment)
double batch_span(const PlanEnv *ctx, const BatchFacts *batch, uint64_t out_stride)
{
    double span = std::ceil((double)batch->max_seconds * ctx->facts.max_rate) + 64.0;
    if (!(span >= 64.0)) span = 64.0;                         // NaN / negative lengths
    return std::fmin(span, (double)(out_stride ? out_stride : 1));
}

// Cost model of the planner, in milliseconds per SAMPLE OF THE LONGEST UTTERANCE for one round of a family (a round:
// as many rows as give every SIMD one wave).  Calibrated on 2 s utterances at 48 kHz, one MI355X
// (profiles/r03_small_batch.txt, profiles/r04_duration_sweep.txt); only the ratios matter.  Indexed [L = 1, 2, 4, 8].
constexpr double MID_MS_4 = 32.6, MID_MS_8 = 57.2;     // 65 536 x 2 s, the MID kernels (profiles/r04_middle_tier.txt)
static double lane_ms_per_sample(bool fast, bool live4, int L)
{
    static const double exact4[4] = {40.6, 26.9, 16.3, 18.2}, exact8[4] = {77.1, 43.5, 25.8, 15.7};
    static const double fast4[4] = {15.5, 13.6, 12.8, 12.1}, fast8[4] = {23.6, 16.4, 13.3, 12.0};
    const int i = L == 1 ? 0 : L == 2 ? 1 : L == 4 ? 2 : 3;
    return (fast ? (live4 ? fast4 : fast8) : (live4 ? exact4 : exact8))[i] / 96006.0;
}
// ... of the second tolerance tier (MID, one lane per utterance)
static double mid_ms_per_sample(bool live4) { return (live4 ? MID_MS_4 : MID_MS_8) / 96006.0; }

// Lane kernels that keep their state in 256 registers — tolerance mode on two (four live formants), four and eight lanes per
// utterance, exact on two (four live formants) and four — can share a SIMD with a second wave, and a launch of more waves
// than the device has SIMDs takes the instantiations built for that (tolerance mode: the lone wave leaves the VALU idle a
// quarter of the time; 65 536 aligned utterances on two lanes each 21.5 ms instead of 26.9, on four 38.6 instead of 51.0.
// Exact: 49.0 instead of 53.7 and 55.1 instead of 64.6; a speech-like corpus 58.1 instead of 67.0: profiles/r05_two_waves.txt).
// Launches that fit one wave per SIMD keep the one-wave instantiations — which cannot share a SIMD, so where the dispatcher
// puts their waves cannot matter.
bool family_cohabits(const PlanEnv *ctx, const Family &f, uint32_t rows)
{
    if (!ctx->opt.two_waves_option || f.scan || f.pipe || f.split_k || f.fast > 1u) return false;
    // (tolerance mode: 2 lanes with four formants laid out, 4 and 8 lanes; exact: 2 lanes with four formants, 4 lanes —
    // the instantiations that hold their state in 256 registers without a scratch segment)
    const bool built = f.fast ? (f.L == 4 || f.L == 8 || (f.L == 2 && f.live4)) : (f.L == 4 || (f.L == 2 && f.live4));
    return built && ((uint64_t)rows * (uint64_t)f.L + 63u) / 64u > ctx_simds(ctx);
}
// What two waves on a SIMD take together, over twice the lone wave's time.  Tolerance mode: 0.76 - 0.80 on aligned batches
// (the plain pairs of one wave fill three quarters of the issue slots), 0.50 - 0.68 where events are dense — a slow sample is
// latency (the elems' loads behind a segment advance, branches, end-point evaluations under one lane's predicate), which the
// other wave fills.  Exact: the lone wave issues at 94 % of the best rate this SIMD has shown, yet two
// resident waves take 0.85 - 0.91 of two in turn on aligned batches — tile heads, flushes and the general steps of the segment
// boundaries are latency too — and 0.70 on phonemes of 4 - 16 ms (profiles/r05_two_waves.txt).
// `density`: events per lane and sample, as in ragged_wave_ms.  Fitted with tools/ragged_fit.py (profiles/r05_ragged_fit.txt).
static double cohabit_gain(const Family &f, double density = 0.0)
{
    if (!f.fast) {
        // (two lanes: 0.905 aligned, 0.873 on the speech-like corpus, 0.85 with phonemes of 4 - 16 ms; four: 0.85 / 0.83 / 0.70)
        const double aligned = f.L == 2 ? 0.91 : 0.85, dense = f.L == 2 ? 0.86 : 0.70;
        return aligned - (aligned - dense) * std::fmin(1.0, density / (f.L == 2 ? 6.0e-4 : 3.0e-3));
    }
    const double aligned = f.L == 2 ? 0.80 : 0.76, dense = f.L == 2 ? 0.52 : f.L == 4 ? 0.65 : 0.68;
    return aligned - (aligned - dense) * std::fmin(1.0, density / 3.0e-4);
}

// Pipelined workgroups on rows that differ in length: a tile with an event of ONE of a workgroup's utterances costs the
// workgroup several calm tiles, so a small batch is spread thinly — as few utterances per workgroup as give every compute
// unit two workgroups — instead of filling 16 (8) slots of a few workgroups and leaving the other units idle: 256 speech-like
// utterances, one per workgroup, hold no event but their own (profiles/r05_mixed_runs.txt).
uint32_t pipe_fill_for(const PlanEnv *ctx, const BatchFacts *batch, const Family &f, uint32_t rows)
{
    if (!f.pipe || !ctx->opt.pipe_spread || !rows_differ(batch)) return 0u;
    const uint32_t slots = f.live4 ? 16u : 8u;
    // (two workgroups to a compute unit — what the rounds of 16 samples leave room for: they fill each other's stalls.
    // 4 096 speech-like utterances, eight to a workgroup: 16.8 ms; sixteen to a workgroup, one per unit: 19.4)
    const uint32_t units = 2u * (uint32_t)ctx->cus;
    const uint32_t fill = (rows + units - 1u) / units;
    return fill >= slots ? 0u : (fill < 1u ? 1u : fill);
}

// what launching `rows` rows with family f costs (model milliseconds)
double family_cost(const PlanEnv *ctx, const Family &f, uint32_t rows, double span)
{
    const double cus = (double)ctx->cus, lanes = (double)ctx_lanes(ctx);
    if (f.scan) {
        // one workgroup per utterance; g = workgroups per compute unit.  Three-stage flavour: the latency of one
        // utterance's chain up to ~2 per CU, then ~0.53 ms per workgroup and CU (2 s); two-stage: 0.41 (four live
        // formants) / 0.65 (eight)
        const double g = std::ceil((double)rows / cus);
        const double ms2s = f.scan_pipe ? (f.live4 ? std::fmax(1.14, 0.53 * g) : std::fmax(1.67, 0.75 * g))
                                        : (f.live4 ? 0.41 * g + 0.1 : 0.65 * g + 0.2);
        return ms2s * span / 96006.0;
    }
    if (f.split_k) {
        // every lane takes as long as the first chunk's, which renders split_bounds[1] samples and nothing else
        const double rounds = split_rounds(ctx, f, rows);
        // (+ 0.12 ms: what a launch of chunk lanes costs before any of them renders — short utterances see it)
        if (f.fast == 2u) return rounds * ((double)f.split_bounds[1] * mid_ms_per_sample(f.live4 != 0) + 0.12);
        return rounds * ((double)f.split_bounds[1] * (f.live4 ? 15.7 : 23.3) / 96006.0 + 0.12);
    }
    if (f.pipe) {
        const double groups = std::ceil((double)rows / (f.live4 ? 16.0 : 8.0));
        const double per_cu = std::ceil(groups / cus);
        // rounds of 32: one workgroup per CU; rounds of 16: two per CU are resident together, further ones queue
        // (rounds of 16 with one workgroup per CU: 7.9 ms for config 2 where rounds of 32 take 6.5)
        const double ms2s = f.pipe == 2 ? (f.live4 ? 6.5 : 7.3) * per_cu
                                        : per_cu <= 1.0 ? (f.live4 ? 7.9 : 8.8) : 11.2 * std::ceil(per_cu / 2.0);
        return ms2s * span / 96006.0;
    }
    const double rounds = std::ceil((double)rows * f.L / lanes);
    if (f.fast == 2u) return rounds * span * mid_ms_per_sample(f.live4 != 0);
    // (eight formants laid out, the upper four silent: the half-live loops of the one-lane kernel, 45.7 ms where all
    // eight live take 77.1)
    if (f.half) return rounds * span * 45.7 / 96006.0;
    if (family_cohabits(ctx, f, rows)) {
        // (pairs of waves: an odd wave-round at the end runs alone, at the lone wave's rate)
        const double pairs = std::floor(rounds / 2.0), rest = rounds - 2.0 * pairs;
        return (2.0 * pairs * cohabit_gain(f) + rest) * span * lane_ms_per_sample(f.fast != 0, f.live4 != 0, f.L);
    }
    return rounds * span * lane_ms_per_sample(f.fast != 0, f.live4 != 0, f.L);
}

// ---- Ragged batches ------------------------------------------------------------------------------------------------------
// The families above are laid out for ONE round: the widest lane mapping that gives every SIMD one wave, priced by the
// batch's longest utterance.  On a length-sorted batch whose utterances differ much in length that leaves most SIMDs idle
// most of the time — the one wave of a SIMD lasts as long as ITS longest row, the launch as long as the longest of all —
// where a wider mapping in several rounds keeps them busy: its waves are shorter, they start longest first, and a SIMD that
// finishes a short one takes the next.  And a wave holds fewer utterances, so fewer of its tiles hold some lane's event.
// (Speech-like corpus, 65 536 utterances of 0.5 - 3.8 s: exact 90.0 ms one lane per utterance, 71.7 two; eight formants
// 171.6 / 113.6; fast 87.7 / 73.6 and 145.7 / 88.8; 100 000: 125 -> 94 in ONE launch of the one-lane kernel.  profiles/r04_ragged_plan.txt.)
// Model: a wave costs its longest row's samples at the mapping's rate plus what its rows' events cost.  Exact: the tiles
// that hold some lane's segment boundary, tiles x (1 - exp(-boundaries per tile)), at 7 / 8 us per 32 samples (four / eight
// formants), and 1.5 / 3.7 us per boundary on one lane per utterance.  Fast: the aligned rate x m plus c per event (below).
// Waves are handed to the SIMDs in launch order as they fall free.  The exact constants were fitted on pinned-mapping
// measurements of the speech-like corpus at 65 536 utterances with phonemes of 40 - 160, 16 - 64 and 4 - 16 ms, L = 1 / 2 / 4,
// four and eight formants (within 10 %, three L = 1 cells of the densest corpus 20 - 28 % under) and checked at 16 384 ...
// 131 072 utterances: profiles/r04_ragged_plan.txt.
static double ragged_wave_ms(const Family &f, double samples, double segs, double kinks)
{
    const bool nfa4 = f.live4 != 0;
    const int li = f.L == 1 ? 0 : f.L == 2 ? 1 : f.L == 4 ? 2 : 3;
    if (!f.fast) {
        // (the half-live loops of the one-lane kernel, 45.7 ms per 2 s, showed on aligned batches only: not priced in)
        const double T = (f.L == 1 || (!nfa4 && f.L == 4)) ? 32.0 : 64.0;
        const double tiles = std::fmax(samples / T, 1.0);
        const double event_tiles = tiles * (1.0 - std::exp(-segs / tiles));
        // (round 5: the 2 / 4 / 8-lane kernels render the samples between the events of such a tile by the calm tile's loops —
        // synth_kernel.h MIXED_RUNS — and a tile with an event costs them 0.5 - 0.75 of what it did; the four-lane kernel with
        // eight formants, tiles of 32 in runs of 8, gains nothing: profiles/r05_mixed_runs.txt)
        const double runs = f.L == 1 ? 1.0 : f.L == 2 ? (nfa4 ? 0.74 : 0.60) : f.L == 4 ? (nfa4 ? 0.51 : 1.0) : 0.58;
        return samples * lane_ms_per_sample(false, nfa4, f.L) + event_tiles * (nfa4 ? 0.007 : 0.008) * (T / 32.0) * runs +
               (f.L == 1 ? segs * (nfa4 ? 0.0015 : 0.0037) : 0.0);
    }
    // Fast (round 5: sub-tiles that never span an event, one slow sample per event — synth_kernel.h fast_render_tile): a wave
    // costs its longest row at the mapping's aligned rate x m — while a lane's parameters move (blends of 30 - 80 ms) its
    // sub-tiles are 16 samples instead of 32, and the wave takes new slopes at the pace of its busiest lane — plus c
    // per event of its rows (boundaries and kinks of alpha: the slow sample, the lane's two end points, the shorter runs
    // around it).  Fitted on pinned-mapping measurements of the speech-like corpus with phonemes of 40 - 160, 16 - 64 and
    // 4 - 16 ms at 65 536 utterances, one and eight voices, L = 1 / 2 / 4 / 8: all 24 cells within 3.3 % (tools/ragged_fit.py,
    // profiles/r05_ragged_fit.txt).  m fades to 1 where events are rare (long segments have long blends: the bench corpora).
    static const double m4[4] = {1.16, 1.10, 1.06, 1.02}, c4[4] = {0.00475, 0.0050, 0.00675, 0.00925};
    static const double m8[4] = {1.08, 1.06, 1.04, 1.02}, c8[4] = {0.00775, 0.00675, 0.0070, 0.0095};
    const double events = segs + kinks;
    const double density = events / ((64.0 / (double)f.L) * std::fmax(samples, 1.0));        // per lane and sample
    const double m = 1.0 + ((nfa4 ? m4 : m8)[li] - 1.0) * std::fmin(1.0, density / 3.0e-4);
    const double rate = f.fast == 2u ? mid_ms_per_sample(nfa4) : lane_ms_per_sample(true, nfa4, f.L);
    return samples * rate * m + events * (nfa4 ? c4 : c8)[li];
}

// the rows of one wave, granules [g, min(g + per_wave, g1)): the longest row, the rows' segments and kinks
struct WaveRows {
    double samples = 0.0, segs = 0.0, kinks = 0.0;
};
static WaveRows wave_rows(const BatchFacts *batch, size_t g, size_t per_wave, size_t g1)
{
    WaveRows w;
    for (size_t k = g; k < std::min(g + per_wave, g1); ++k) {
        w.samples = std::fmax(w.samples, (double)batch->granule_samples[k]);
        w.segs += batch->granule_segs[k];
        w.kinks += batch->granule_kinks[k];
    }
    return w;
}
double ragged_wave_cost(const BatchFacts *batch, const Family &f, size_t g, size_t per_wave, size_t g1, double span)
{
    const WaveRows w = wave_rows(batch, g, per_wave, g1);
    return ragged_wave_ms(f, std::fmin(w.samples + 64.0, span), w.segs, w.kinks);
}
// the mean over granules [g0, g1) of their longest rows
static double mean_samples(const BatchFacts *batch, const GranuleRange &r)
{
    double mean = 0.0;
    for (size_t g = r.g0; g < r.g1; ++g) mean += (double)batch->granule_samples[g];
    return mean / (double)(r.g1 - r.g0);
}

// one workgroup per utterance: a compute unit works off the sum of its utterances' lengths (choose_family)
static double ragged_scan_cost(const PlanEnv *ctx, const BatchFacts *batch, const Family &f, const GranuleRange &r, uint32_t rows,
                               double span)
{
    return std::fmax(family_cost(ctx, f, rows, std::fmin(mean_samples(batch, r) + 64.0, span)),
                     family_cost(ctx, f, 1u, std::fmin(span, (double)batch->granule_samples[r.g0] + 64.0)));
}

// (families that render an utterance with many lanes: by the block's own longest row.  A pipelined workgroup renders its
// 16 / 8 utterances in rounds of 32 samples; a round that holds a segment boundary of one of them costs it ~11 us more (14
// before the runs between events):
// 256 utterances with phonemes of 4 - 16 ms take 5.7 ms where their 0.39 s alone would take 1.3)
static double ragged_pipe_cost(const PlanEnv *ctx, const BatchFacts *batch, const Family &f, const GranuleRange &r, uint32_t rows,
                               double span)
{
    const size_t g0 = r.g0, g1 = r.g1;
    double longest = std::fmin(span, std::fmax((double)batch->granule_samples[g0], 0.0) + 64.0);
    // (two workgroups per compute unit: the one with the shorter rows ends early and leaves the unit to the other —
    // 8 192 speech-like utterances take 19.6 ms where their longest row at the rate of two resident workgroups would
    // take 21.0; with phonemes of 16 - 64 ms 10.3, of 4 - 16 ms 4.6: profiles/r05_mixed_runs.txt)
    if (std::ceil((double)rows / (f.live4 ? 16.0 : 8.0)) > (double)ctx->cus)
        longest = 0.55 * longest + 0.45 * std::fmin(longest, mean_samples(batch, r) + 64.0);
    double c = family_cost(ctx, f, rows, longest);
    c *= 1.15;      // (ragged corpora measure 15 - 25 % over the aligned rate before any event: pitch contours, stops)
    double segs = batch->granule_segs[g0];
    if (f.live4 && g0 + 1 < g1) segs += batch->granule_segs[g0 + 1];
    // (spread thinly: a workgroup's tiles hold the events of `fill` utterances, not of 16 / 8)
    const uint32_t fill = pipe_fill_for(ctx, batch, f, rows);
    if (fill) segs *= (double)fill / (f.live4 ? 16.0 : 8.0);
    const double rounds = std::fmax(longest / 32.0, 1.0);
    const double groups = std::ceil((double)rows / (f.live4 ? 16.0 : 8.0));
    c += 0.011 * rounds * (1.0 - std::exp(-segs / rounds)) * std::ceil(groups / ((f.pipe == 2 ? 1.0 : 2.0) * (double)ctx->cus));
    return c;
}

// every wave holds 64 utterances at one chunk index: the events of a one-lane wave; the first chunk of the
// longest rows sets the time (x 1.2: fast-forward and restarts, from the same corpus)
static double ragged_split_cost(const PlanEnv *ctx, const BatchFacts *batch, const Family &f, const GranuleRange &r, uint32_t rows)
{
    const WaveRows w = wave_rows(batch, r.g0, 8, r.g1);
    const double len = std::fmax((double)batch->granule_samples[r.g0], 64.0), part = (double)f.split_bounds[1] / len;
    Family lane = f;
    lane.split_k = 0;
    lane.L = 1;
    return split_rounds(ctx, f, rows) * (1.2 * ragged_wave_ms(lane, (double)f.split_bounds[1], w.segs * part, w.kinks * part) + 0.12);
}

// Two waves per SIMD: while two are resident each advances at 1 / (2 gain) of the lone wave's pace (together
// 1 / gain: the 20 - 25 % the second wave adds); the one left behind by a shorter neighbour runs on alone at full
// pace.  Waves are handed out in launch order, two per SIMD at first, then to the SIMD that has a slot free first.
static double two_wave_cost(const PlanEnv *ctx, const BatchFacts *batch, const Family &f, const GranuleRange &r, double span)
{
    const size_t g0 = r.g0, g1 = r.g1, per_wave = granules_per_wave(f);
    const uint64_t simds = ctx_simds(ctx);
    struct Simd { double t, a, b; };              // time reached; work left (in lone-wave ms) in the two slots, a <= b; < 0: empty
    auto take = [](Simd &m, const double w) {     // a free slot of the SIMD takes a wave
        if (m.b < 0.0) m.b = w;
        else if (w <= m.b) m.a = w;
        else { m.a = m.b; m.b = w; }
    };
    double ev_sum = 0.0, lane_samples = 0.0;
    for (size_t g = g0; g < g1; ++g) {
        ev_sum += (double)batch->granule_segs[g] + (double)batch->granule_kinks[g];
        lane_samples += 8.0 * std::fmax((double)batch->granule_samples[g], 1.0);
    }
    const double pace2 = 1.0 / (2.0 * cohabit_gain(f, ev_sum / std::fmax(lane_samples, 1.0)));
    std::vector<Simd> sm(simds, Simd{0.0, -1.0, -1.0});
    auto next_done = [&](const Simd &m) {         // when the SIMD's next wave ends (it has at least one)
        return m.a < 0.0 ? m.t + m.b : m.t + m.a / pace2;
    };
    typedef std::pair<double, size_t> Ev;
    std::priority_queue<Ev, std::vector<Ev>, std::greater<Ev>> done_at;
    // (a launch of at most two rounds: the waves of the second take their slots in reverse order — synth_kernel.h FOLD —
    // so that the SIMD with the longest rows of the first round gets the shortest of the second)
    const size_t n_waves = (g1 - g0 + per_wave - 1) / per_wave;
    const bool fold = n_waves > simds && n_waves <= 2 * simds;
    size_t g = g0, filled = 0;
    for (; g < g1 && filled < 2 * simds; g += per_wave, ++filled)
        take(sm[filled % simds], ragged_wave_cost(batch, f, fold && filled >= simds ? g0 + (n_waves - 1 - (filled - simds)) * per_wave : g,
                                                  per_wave, g1, span));
    for (size_t i = 0; i < simds; ++i)
        if (sm[i].b >= 0.0) done_at.push(Ev(next_done(sm[i]), i));
    double makespan = 0.0;
    while (!done_at.empty()) {
        const Ev ev = done_at.top();
        done_at.pop();
        Simd &m = sm[ev.second];
        if (m.a < 0.0) {                          // the lone wave ends
            m.t += m.b;
            m.b = -1.0;
        } else {                                  // the shorter of two ends; the other has advanced as far
            m.t += m.a / pace2;
            m.b -= m.a;
            m.a = -1.0;
        }
        makespan = std::fmax(makespan, m.t);
        if (g < g1) {                             // the slot takes the next wave of the launch
            take(m, ragged_wave_cost(batch, f, g, per_wave, g1, span));
            g += per_wave;
        }
        if (m.b >= 0.0) done_at.push(Ev(next_done(m), ev.second));
    }
    // Against measurements of every pinned mapping on 40 000 ... 200 000 speech-like rows, one and eight voices
    // (profiles/r06_plan_debug.txt): the exact two-wave kernels run ahead of this simulation — two lanes 0.77 - 0.86 of
    // it (they got their runs between events after the wave prices were fitted), four lanes 0.86 - 0.95 — at every
    // size, and the tolerance-mode two-lane kernel falls behind it (1.13 - 1.20) once a launch holds more waves than
    // are resident at once.  With the one-wave-per-SIMD launches priced by the dispatcher's model (within 0.93 - 1.0
    // of their measurements), the two-wave prices are brought to the same scale here.
    const double waves = std::ceil((double)(g1 - g0) / (double)per_wave);
    const double scale = !f.fast ? (f.L == 2 ? 0.84 : 0.91) : (f.L == 2 && waves > 2.0 * (double)simds ? 1.15 : 1.0);
    return makespan * scale;
}

// one wave per SIMD: the workgroups of the launch through the dispatcher's model, in the plain (longest rows first) or
// in the packed order, whichever the launch will take (packed_launch_order: the same decision)
static double dispatched_cost(const PlanEnv *ctx, const BatchFacts *batch, const Family &f, uint32_t slot0, uint32_t rows, double span)
{
    double plain_ms = 0.0, packed_ms = 0.0;
    const bool packed = packed_launch_order(ctx, batch, f, slot0, rows, span, nullptr, nullptr, &plain_ms, &packed_ms);
    // (x 0.96: the wave prices of ragged_wave_ms through the dispatcher's model come out 0 - 7 % over the measurements,
    // uniformly over mappings, sizes and both arithmetics — profiles/r06_plan_debug.txt)
    return 0.96 * (packed ? packed_ms : plain_ms);
}

// what a block of rows [slot0, slot0 + rows) costs by the lengths and events of ITS rows: each family its own way; the lane
// kernels in waves of 64 / L consecutive slots, handed out in launch order to the SIMD that falls free first
double ragged_cost(const PlanEnv *ctx, const BatchFacts *batch, const Family &f, uint32_t slot0, uint32_t rows, double span)
{
    if (batch->granule_samples.empty() || rows == 0) return family_cost(ctx, f, rows, span);
    const GranuleRange r = granule_range(batch, slot0, rows);
    if (f.scan) return ragged_scan_cost(ctx, batch, f, r, rows, span);
    if (f.pipe) return ragged_pipe_cost(ctx, batch, f, r, rows, span);
    if (f.split_k) return ragged_split_cost(ctx, batch, f, r, rows);
    if (family_cohabits(ctx, f, rows)) return two_wave_cost(ctx, batch, f, r, span);
    return dispatched_cost(ctx, batch, f, slot0, rows, span);
}

}  // namespace host
}  // namespace grail
