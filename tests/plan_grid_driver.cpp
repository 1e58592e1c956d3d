// plan_grid_driver.cpp — the launch planner's answers over a grid of contexts and batches built directly (PlanEnv,
// BatchFacts), where tests/golden/plan_transcript.txt reaches it through grail_plan_blocks only: option branches,
// caller-built elems, per-voice records, the half-live and MID fall-backs, ragged_cost at a later slot, the packed order.
// Built by tests/test_plan_grid_host.py with g++ from the planner's units, voice_analysis.cpp and voice_host.cpp (none
// makes a HIP call); the three error helpers of grail_api.cpp are defined here.  Output: "== <group>" headers, below each
// the cells of the group, one line per family; prices as (float) in %a ("--doubles": the double itself).  The driver
// checks its own coverage (every option of the planner moves a line, every family kind occurs) and exits 1 if not.
#include <cstdarg>
#include <set>

#include "../grail-rs_amd/csrc/api_internal.hpp"

namespace grail {
namespace host {
static thread_local std::string g_err;
int fail(int status, const std::string &msg)
{
    g_err = msg;
    return status;
}
int hip_fail(hipError_t, const char *what) { return fail(GRAIL_ERR_HIP, what); }
std::string &last_error() { return g_err; }
}  // namespace host
}  // namespace grail

using namespace grail;
using namespace grail::host;

static bool g_doubles = false;
static int g_fails = 0;
#define CHECK(c) do { if (!(c)) { std::fprintf(stderr, "plan grid driver: not covered: %s\n", #c); ++g_fails; } } while (0)

static void put(std::string &s, const char *fmt, ...)
{
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    std::vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    s += buf;
}
static void put_ms(std::string &s, const char *name, double ms)
{
    if (g_doubles) put(s, " %s=%a", name, ms);
    else put(s, " %s=%a", name, (double)(float)ms);
}

// ---- the axes
constexpr uint64_t EPOCH = 7;
constexpr uint32_t SPAN = 96006, WARMUP = 3904;
static const int CUS[] = {256, 32, 20};
static const uint32_t ROWS[] = {1, 300, 1500, 4096, 20000, 70000};
enum Voices { LIVE4 = 0, UPPER_SILENT = 1, EIGHT_LIVE = 2 };
enum Mode { PHONEMES = 0, ELEMS = 1, ELEMS_STALE = 2 };
static const char *const MODE_NAME[] = {"phonemes", "elems", "elems_stale"};

struct OptCell {
    const char *name;             // "field=value"
    int64_t Options::*field;      // nullptr: the defaults
    int64_t value;
};
// every Options field the planner reads, off its default ("arithmetic", fast_option, is an axis of its own)
static const OptCell OPTS[] = {
    {"defaults", nullptr, 0},
    {"lanes_option=4", &Options::lanes_option, 4},
    {"lanes_option=8", &Options::lanes_option, 8},
    {"skip_silent_option=0", &Options::skip_silent_option, 0},
    {"pipeline_option=0", &Options::pipeline_option, 0},
    {"pipe_round32=0", &Options::pipe_round32, 0},
    {"pipe_round32=2", &Options::pipe_round32, 2},
    {"pipe_spread=0", &Options::pipe_spread, 0},
    {"pipe4_max_groups=8", &Options::pipe4_max_groups, 8},
    {"pipe8_max_groups=8", &Options::pipe8_max_groups, 8},
    {"scan_option=0", &Options::scan_option, 0},
    {"scan_max_utts=100", &Options::scan_max_utts, 100},
    {"scan_split_max=0", &Options::scan_split_max, 0},
    {"split_option=0", &Options::split_option, 0},
    {"split_chunks=8", &Options::split_chunks, 8},
    {"split_span=48000", &Options::split_span, 48000},
    {"split_ff_permille=400", &Options::split_ff_permille, 400},
    {"split_min_utts=2000", &Options::split_min_utts, 2000},
    {"ragged_option=0", &Options::ragged_option, 0},
    {"two_waves_option=0", &Options::two_waves_option, 0},
    {"packed_option=0", &Options::packed_option, 0},
};
constexpr size_t N_OPTS = sizeof OPTS / sizeof OPTS[0];

static uint32_t rng_state = 1u;
static uint32_t rnd()
{
    rng_state = rng_state * 1664525u + 1013904223u;
    return rng_state >> 8;
}

// a voice table of two: voice 0 as the axis says, voice 1 with eight live formants outside every window.  The batch names
// voice 0 only, so the table-wide flags (false) must not be what decides.
static PlanEnv make_env(int cus, int arith, Voices voices, const OptCell &o)
{
    PlanEnv env;
    env.cus = cus;
    env.voices_epoch = EPOCH;
    env.opt.fast_option = arith;
    if (o.field) env.opt.*o.field = o.value;
    VoiceInfo v0;
    v0.upper_silent = voices != EIGHT_LIVE;
    v0.live4_ok = voices == LIVE4;
    v0.scan_ok = v0.split_ok = true;
    v0.warmup = WARMUP;
    env.facts.voice_info = {v0, VoiceInfo()};
    env.facts.max_warmup = WARMUP;
    env.facts.max_rate = 1.0f;            // (max_seconds is in samples)
    env.facts.max_dt = 1.0f;
    // (arithmetic 2: too sharp for the interpolating tier, served by the MID tier)
    env.facts.voice_sharpness = {arith == 2 ? GRAIL_FAST_SHARPNESS_LIMIT + 4.0 : 24.0, INFINITY};
    env.facts.voices_sharpness = INFINITY;
    return env;
}

// what the upload keeps of `rows` rows of 0.5 - 3.8 s at 48 kHz with 8 - 32 segments each, longest first (made once per size)
static const BatchFacts &ragged_summary(uint32_t rows)
{
    static std::map<uint32_t, BatchFacts> made;
    auto it = made.find(rows);
    if (it != made.end()) return it->second;
    BatchFacts &b = made[rows];
    rng_state = 1u + rows;
    std::vector<uint32_t> len(rows), segs(rows), kinks(rows);
    for (uint32_t r = 0; r < rows; ++r) len[r] = 24000u + rnd() % 158000u;
    std::sort(len.begin(), len.end(), std::greater<uint32_t>());
    for (uint32_t r = 0; r < rows; ++r) {
        segs[r] = 8u + rnd() % 25u;
        kinks[r] = rnd() % (segs[r] + 1u);
    }
    const size_t n_gran = ((size_t)rows + 7) / 8;
    b.granule_samples.assign(n_gran, 0.0f);
    b.granule_segs.assign(n_gran, 0u);
    b.granule_kinks.assign(n_gran, 0u);
    for (uint32_t r = 0; r < rows; ++r) {
        b.granule_samples[r / 8] = std::fmax(b.granule_samples[r / 8], (float)len[r]);
        b.granule_segs[r / 8] += segs[r];
        b.granule_kinks[r / 8] += kinks[r];
    }
    b.max_seconds = (float)len[0];
    return b;
}

// a plain batch of `rows` rows: ragged as above, or all of SPAN samples (aligned)
static BatchFacts make_batch(uint32_t rows, bool ragged, Voices voices, Mode mode)
{
    BatchFacts b;
    if (ragged) {
        b = ragged_summary(rows);
        b.len_bound_known = true;
        b.len_bound_epoch = EPOCH;
    } else {
        b.max_seconds = (float)SPAN;
    }
    b.n_utt = rows;
    b.plain = true;
    b.min_length = 1e9f;
    b.min_pitch = 0.25f;
    b.used_voices = {0u};
    b.phoneme_mode = mode == PHONEMES;
    if (!b.phoneme_mode) {
        b.elems_sharpness = 24.0;
        b.elems_warmup = WARMUP;
        b.elems_warmup_epoch = mode == ELEMS ? EPOCH : EPOCH - 1;
        b.elems_live4_ok = voices == LIVE4;
        b.elems_scan_ok = true;
    }
    return b;
}

// ---- what has occurred (the coverage conditions)
static std::set<std::string> kinds;
static bool packed_true = false, packed_false_ragged = false, cohabits_exact = false, cohabits_fast = false;
static bool fast_came_back_pipelined = false, mid_came_back_exact = false;

static void note_kind(const Family &f)
{
    char k[96];
    if (f.scan) std::snprintf(k, sizeof k, "scan pipe=%u formants=%d", f.scan_pipe, f.live4 ? 4 : 8);
    else if (f.split_k) std::snprintf(k, sizeof k, "split fast=%u active=%d", f.fast, f.split_active ? 1 : 0);
    else if (f.pipe) std::snprintf(k, sizeof k, "pipe=%u L=%d", f.pipe, f.L);
    else if (f.half) std::snprintf(k, sizeof k, "half");
    else std::snprintf(k, sizeof k, "lane L=%d fast=%u live4=%u", f.L, f.fast, f.live4);
    kinds.insert(k);
}

static void put_family(std::string &s, const char *tag, const PlanEnv &env, const BatchFacts &b, uint32_t rows, double span,
                       const Family &f)
{
    note_kind(f);
    put(s, "  %s L=%d pipe=%u live4=%u half=%d fast=%u k=%d active=%u scan=%d scan_pipe=%u b=", tag, f.L, f.pipe, f.live4,
        (int)f.half, f.fast, f.split_k, f.split_active, (int)f.scan, f.scan_pipe);
    for (int k = 0; k <= f.split_k; ++k) put(s, k ? ",%u" : "%u", f.split_bounds[k]);
    const bool cohabits = family_cohabits(&env, f, rows);
    (f.fast ? cohabits_fast : cohabits_exact) |= cohabits;
    put(s, " cohabits=%d fill=%u", (int)cohabits, pipe_fill_for(&env, &b, f, rows));
    put_ms(s, "cost", family_cost(&env, f, rows, span));
    put_ms(s, "ragged0", ragged_cost(&env, &b, f, 0u, rows, span));
    const uint32_t later = rows / 2u / 8u * 8u;
    put_ms(s, "ragged_later", ragged_cost(&env, &b, f, later, rows - later, span));
    std::vector<uint32_t> order;
    uint32_t per_block = 0;
    double plain = 0.0, packed = 0.0;
    const bool is_packed = packed_launch_order(&env, &b, f, 0u, rows, span, &order, &per_block, &plain, &packed);
    uint32_t sum = 2166136261u;
    for (const uint32_t o : order) sum = (sum ^ o) * 16777619u;
    packed_true |= is_packed;
    packed_false_ragged |= !is_packed && !b.granule_samples.empty();
    put(s, " packed=%d per_block=%u n=%zu order=%08x", (int)is_packed, per_block, order.size(), sum);
    put_ms(s, "plain", plain);
    put_ms(s, "packed_ms", packed);
    s += "\n";
}

static std::string cell(const PlanEnv &env, const BatchFacts &b, uint32_t rows, bool ragged)
{
    std::string s;
    const uint64_t stride = ((uint64_t)b.max_seconds + 64u + 63u) / 64u * 64u;
    const double span = batch_span(&env, &b, stride);
    put(s, " cell %s rows=%u\n", ragged ? "ragged" : "aligned", rows);
    Family f;
    choose_family(&env, &b, stride, rows, f);
    put_family(s, "chosen", env, b, rows, span, f);
    if (env.opt.fast_option && !f.fast) {
        fast_came_back_pipelined |= f.pipe != 0u && fast_tier(&env, &b) != 0;
        mid_came_back_exact |= fast_tier(&env, &b) == 2;
    }
    choose_family(&env, &b, stride, rows, f, true);
    put_family(s, "exact_only", env, b, rows, span, f);
    for (int L = 1; L <= 8; L *= 2) {
        char tag[16];
        std::snprintf(tag, sizeof tag, "pin%d", L);
        choose_family(&env, &b, stride, rows, f, false, L);
        put_family(s, tag, env, b, rows, span, f);
    }
    std::vector<Block> plan;
    plan_blocks(&env, &b, stride, rows, span, plan);
    ragged_plan(&env, &b, stride, rows, plan);
    put(s, "  plan");
    uint32_t slot0 = 0;
    for (const Block &blk : plan) {
        const Family &g = blk.f;
        put(s, " [%u: L=%d pipe=%u live4=%u half=%d fast=%u k=%d active=%u scan=%d scan_pipe=%u", blk.rows, g.L, g.pipe, g.live4,
            (int)g.half, g.fast, g.split_k, g.split_active, (int)g.scan, g.scan_pipe);
        put_ms(s, "ms", ragged_cost(&env, &b, g, slot0, blk.rows, span));
        s += "]";
        slot0 += blk.rows;
    }
    s += "\n";
    return s;
}

// the 12 cells of a group: aligned and ragged rows of every block size
static std::string group(int cus, int arith, Voices voices, Mode mode, const OptCell &o)
{
    const PlanEnv env = make_env(cus, arith, voices, o);
    std::string s;
    for (const bool ragged : {false, true})
        for (const uint32_t rows : ROWS) s += cell(env, make_batch(rows, ragged, voices, mode), rows, ragged);
    return s;
}

int main(int argc, char **argv)
{
    g_doubles = argc > 1 && !std::strcmp(argv[1], "--doubles");
    bool moved[N_OPTS] = {};
    bool arithmetic_moved = false;
    std::string exact[3][3];
    for (size_t c = 0; c < 3; ++c)
        for (int arith = 0; arith <= 2; ++arith)
            for (const Voices voices : {LIVE4, UPPER_SILENT, EIGHT_LIVE}) {
                const int cus = CUS[c];
                std::string defaults;
                for (const Mode mode : {PHONEMES, ELEMS, ELEMS_STALE})
                    // (the option axis: phoneme batches on the whole device)
                    for (size_t o = 0; o < (mode == PHONEMES && cus == CUS[0] ? N_OPTS : 1u); ++o) {
                        const std::string text = group(cus, arith, voices, mode, OPTS[o]);
                        std::printf("== cus=%d arithmetic=%d voices=%d batch=%s %s cells=12\n%s", cus, arith, (int)voices,
                                    MODE_NAME[mode], OPTS[o].name, text.c_str());
                        if (mode == PHONEMES && o == 0) defaults = text;
                        else if (mode == PHONEMES) moved[o] |= text != defaults;
                    }
                if (arith == 0) exact[c][voices] = defaults;
                else arithmetic_moved |= defaults != exact[c][voices];
            }

    // ---- coverage: conditions, not measurements
    CHECK(arithmetic_moved);                                             // Options::fast_option
    for (size_t o = 1; o < N_OPTS; ++o)
        if (!moved[o]) {
            std::fprintf(stderr, "plan grid driver: not covered: %s moves no line\n", OPTS[o].name);
            ++g_fails;
        }
    static const char *const required[] = {
        "scan pipe=0 formants=4", "scan pipe=0 formants=8", "scan pipe=1 formants=4", "scan pipe=1 formants=8",
        "split fast=1 active=0", "split fast=1 active=1", "split fast=2 active=0", "split fast=2 active=1",
        "pipe=1 L=4", "pipe=2 L=4", "pipe=1 L=8", "pipe=2 L=8", "half",
        "lane L=1 fast=0 live4=0", "lane L=1 fast=0 live4=1", "lane L=1 fast=1 live4=0", "lane L=1 fast=1 live4=1",
        "lane L=2 fast=0 live4=0", "lane L=2 fast=0 live4=1", "lane L=2 fast=1 live4=0", "lane L=2 fast=1 live4=1",
        "lane L=1 fast=2 live4=0", "lane L=1 fast=2 live4=1", "lane L=8 fast=0 live4=0",
    };
    for (const char *k : required)
        if (!kinds.count(k)) {
            std::fprintf(stderr, "plan grid driver: not covered: family kind \"%s\"\n", k);
            ++g_fails;
        }
    CHECK(fast_came_back_pipelined);
    CHECK(mid_came_back_exact);
    CHECK(packed_true && packed_false_ragged);
    CHECK(cohabits_exact && cohabits_fast);
    std::printf("== coverage cells=0\n");
    for (const std::string &k : kinds) std::printf(" kind %s\n", k.c_str());
    std::printf(" %zu kinds, %zu option cells\n", kinds.size(), N_OPTS - 1);
    return g_fails ? 1 : 0;
}
