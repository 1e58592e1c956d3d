// grail_api.cpp — the C ABI (include/grail_hip.h) over the HIP kernels: contexts, voice tables, HBM-resident
// batches, synchronisation and the device utilities.  Host orchestration only (with options.cpp, voice_analysis.cpp,
// the launch planner (launch_plan.h), synthesize.cpp, streams.cpp, host_output.cpp, comm.cpp): no arithmetic of the hot
// path happens here and there is no CPU fallback: without a HIP device every compute call fails.
#include "api_internal.hpp"

using namespace grail;
using namespace grail::host;

static_assert(sizeof(grail_synthesis_elem) == 196, "SynthesisElem is 49 x f32");
static_assert(sizeof(grail_phoneme_elem) == sizeof(DevSeg), "PhonemeElem uploads as-is");
static_assert(offsetof(grail_phoneme_elem, phoneme) == offsetof(DevSeg, elem), "layout");
static_assert(offsetof(grail_phoneme_elem, frequency) == offsetof(DevSeg, frequency), "layout");
static_assert(sizeof(grail_voice) == 4 + 2 * 196 + 5 * 4, "Voice layout");
static_assert(GRAIL_UNIQUE_ID_BYTES == NCCL_UNIQUE_ID_BYTES, "unique id size");

namespace grail {
namespace host {

namespace {
thread_local std::string g_last_error;
// Voice-table epochs are drawn from ONE counter for the whole process: a batch (or a stream) remembers the epoch of the
// table something was computed against, and a batch may be rendered by another context than the one that uploaded it —
// two contexts that each installed one table must not both be "epoch 1".
std::atomic<uint64_t> g_epoch{0};
}

std::string &last_error() { return g_last_error; }

int fail(int status, const std::string &msg)
{
    g_last_error = msg;
    return status;
}

int hip_fail(hipError_t e, const char *what)
{
    if (e == hipErrorOutOfMemory)
        return fail(GRAIL_ERR_OUT_OF_MEMORY, std::string(what) + ": " + hipGetErrorString(e));
    if (e == hipErrorNoDevice || e == hipErrorInvalidDevice)
        return fail(GRAIL_ERR_NO_DEVICE, std::string(what) + ": " + hipGetErrorString(e));
    return fail(GRAIL_ERR_HIP, std::string(what) + ": " + hipGetErrorString(e));
}

int bind(grail_ctx *ctx)
{
    if (!ctx) return fail(GRAIL_ERR_INVALID_ARG, "ctx is NULL");
    HIP_TRY(hipSetDevice(ctx->device));
    return GRAIL_OK;
}

int bind_device(grail_ctx *ctx, const char *who)
{
    if (ctx) return bind(ctx);
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n < 1)
        return fail(GRAIL_ERR_NO_DEVICE, std::string(who) + ": no usable HIP device (there is no CPU fallback)");
    return fail(GRAIL_ERR_INVALID_ARG, std::string(who) + ": ctx is NULL");
}

// clk / 2^k is clk * 2^-k exactly; any other blend length needs the division code of the kernel
bool blend_is_pow2(float blend_length)
{
    uint32_t bits;
    std::memcpy(&bits, &blend_length, sizeof bits);
    const uint32_t e = (bits >> 23) & 0xFFu;
    return (bits & 0x7FFFFFu) == 0u && e >= 1u && e <= 253u;
}

int check_offsets(const uint32_t *seg_offsets, uint32_t n_utt, uint32_t *n_segs)
{
    if (!seg_offsets) return fail(GRAIL_ERR_INVALID_ARG, "seg_offsets is NULL");
    for (uint32_t u = 0; u < n_utt; ++u)
        if (seg_offsets[u + 1] < seg_offsets[u])
            return fail(GRAIL_ERR_INVALID_ARG, "seg_offsets must be non-decreasing");
    *n_segs = seg_offsets[n_utt];
    return GRAIL_OK;
}

// What the launch policy asks of an utterance's segments (the batch's fields of the same names are these over all rows)
struct RowStats {
    bool plain = true;          // every length / blend length / pitch finite, blend lengths > 0
    bool any_blend = false;     // some blend length is not +-2^k
    float min_length = INFINITY, min_pitch = INFINITY, seconds = 0.0f;
    uint32_t segs = 0, kinks = 0;   // segments; those whose alpha = min(clk / blend_length, 1) has a kink (blend_length < length)
    double bound_samples = 0.0;     // grail_length_bound of the row at the table's highest sample rate (INFINITY: none)
};

// What one segment can last at most, in samples.  Every advance adds the segment's length to the clock (:873 / :882), every
// sample takes dt off it in f32 (:861): a step lowers the clock by at least dt - ulp(length) / 2 (the clock is at most the
// length while the segment lasts), so the segment is over after length / (dt - ulp / 2) steps, + 1 for the step that finds
// the clock negative, + 1 for a segment that leaves it negative and still takes its sample.  At 192 kHz a segment of 16 s
// lasts up to 22 % longer than its nominal 3 072 000 samples (ulp(16) / 2 = 0.18 dt) — in the reference as here.
static double segment_bound(float length, double dt)
{
    if (!(length > 0.0f)) return 2.0;
    int e = 0;
    (void)std::frexp(length, &e);                       // length = m 2^e, m in [0.5, 1): ulp = 2^(e - 24)
    const double half_ulp = std::ldexp(1.0, e - 25);
    if (!(dt > 2.0 * half_ulp)) return INFINITY;        // (the clock may not move at all)
    return (double)length / (dt - half_ulp) + 2.0;
}

// An utterance's segments [i0, i1) (PhonemeElems, or the DevSegs of caller-built elems); pitch_of(frequency): the pitch the
// kernels will see.
// min_dt: the device's dt of the table's highest sample rate, as the kernels have it (an f32 reciprocal; 0: no table).
template <typename Seg, typename Pitch>
static RowStats row_stats(const Seg *segs, uint32_t i0, uint32_t i1, double min_dt, Pitch pitch_of)
{
    RowStats r;
    for (uint32_t i = i0; i < i1; ++i) {
        const float pitch = pitch_of(segs[i].frequency);
        r.plain = r.plain && std::isfinite(segs[i].length) && std::isfinite(segs[i].blend_length) &&
                  std::isfinite(segs[i].frequency) && segs[i].blend_length > 0.0f;
        r.any_blend = r.any_blend || !blend_is_pow2(segs[i].blend_length);
        if (segs[i].length < r.min_length) r.min_length = segs[i].length;
        if (pitch < r.min_pitch) r.min_pitch = pitch;
        r.seconds += segs[i].length;
        r.bound_samples += segment_bound(segs[i].length, min_dt);
        r.segs += 1u;
        r.kinks += segs[i].blend_length < segs[i].length ? 1u : 0u;
    }
    return r;
}

// the summary of no rows, and a row folded into it (a batch's, a row group's)
static void clear_summary(BatchFacts &t)
{
    t.plain = true;
    t.any_blend = false;
    t.min_length = INFINITY;
    t.min_pitch = INFINITY;
    t.max_seconds = 0.0f;
}
static void add_row(BatchFacts &t, const RowStats &r)
{
    t.plain = t.plain && r.plain;
    t.any_blend = t.any_blend || r.any_blend;
    if (r.min_length < t.min_length) t.min_length = r.min_length;
    if (r.min_pitch < t.min_pitch) t.min_pitch = r.min_pitch;
    if (r.seconds > t.max_seconds) t.max_seconds = r.seconds;
}

// (every utterance, then the batch: what the launch policy asks of the segments)
template <typename Seg, typename Pitch>
static std::vector<RowStats> batch_stats(const grail_ctx *ctx, grail_batch *b, const Seg *segs, const uint32_t *seg_offsets,
                                         uint32_t n_utt, Pitch pitch_of)
{
    const double min_dt = ctx->facts.max_rate > 0.0f ? (double)(1.0f / ctx->facts.max_rate) : 0.0;
    std::vector<RowStats> rows(n_utt);
    clear_summary(*b);
    for (uint32_t u = 0; u < n_utt; ++u) {
        rows[u] = row_stats(segs, seg_offsets[u], seg_offsets[u + 1], min_dt, pitch_of);
        add_row(*b, rows[u]);
    }
    return rows;
}

// An upper bound of every utterance's length in samples, on the device (time-split kernels: a chunk's lane whose utterance
// ends before the chunk begins has nothing to render and says so at once — batches whose rows differ in length then take
// more, shorter chunks; family_choice.cpp): grail_length_bound at the table's highest sample rate, + a tile.
int upload_len_bound(grail_ctx *ctx, grail_batch *b, const std::vector<RowStats> &rows, uint32_t n_utt)
{
    if (!b->plain || n_utt == 0 || ctx->voices.empty()) return GRAIL_OK;
    std::vector<uint32_t> bound(n_utt);
    for (uint32_t u = 0; u < n_utt; ++u) {
        const double samples = rows[u].bound_samples + 64.0;
        bound[u] = samples < 4.0e9 ? (uint32_t)samples : 0xFFFFFFFFu;
    }
    HIP_TRY(upload(b->d_len_bound, bound.data(), n_utt, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    b->len_bound_epoch = ctx->voices_epoch;
    b->len_bound_known = true;
    return GRAIL_OK;
}

// Ragged batches: the lanes of a wave run in lockstep, so a wave lasts as long as its longest utterance.
// Launch slots are therefore filled in order of decreasing length (sum of the segment lengths, in seconds
// — close enough to the sample count for sorting): the utterances of a wave end together, and when the
// batch is larger than the machine the longest waves start first.  Results do not depend on the slot
// (batch invariance), rows stay where the caller put them.  Aligned batches (all sums equal) keep the
// identity assignment and pay nothing.
// Rows the lean kernel families cannot take (RowGroup) go last, whatever their length: the batch is then
// planned as two batches.  (Judged against the voice table of this moment: the bounds involve its sample rates and
// pitch jitter; a batch uploaded before any table, or rendered with another one, is planned as one.)
int upload_length_order(grail_ctx *ctx, grail_batch *b, const std::vector<RowStats> &rows, uint32_t n_utt)
{
    if (n_utt < 2 || !ctx->opt.sort_option) return GRAIL_OK;
    std::vector<uint8_t> outlier(n_utt, 0);
    uint32_t n_out = 0;
    if (!ctx->voices.empty()) {
        for (uint32_t u = 0; u < n_utt; ++u) {
            const RowStats &r = rows[u];
            const bool lean = r.plain && lean_window(r.min_length, r.min_pitch, ctx->facts);
            outlier[u] = lean ? 0 : 1;
            n_out += outlier[u];
        }
        if (n_out == n_utt) n_out = 0;                  // nothing to separate them from
    }
    float lo = rows[0].seconds, hi = rows[0].seconds;
    for (uint32_t u = 1; u < n_utt; ++u) {
        lo = std::fmin(lo, rows[u].seconds);
        hi = std::fmax(hi, rows[u].seconds);
    }
    const bool ragged = hi - lo > 0.002f;           // (aligned, or NaN lengths: nothing to gain from sorting)
    if (!ragged && n_out == 0) return GRAIL_OK;
    std::vector<uint32_t> perm(n_utt);
    for (uint32_t u = 0; u < n_utt; ++u) perm[u] = u;
    auto key = [&](uint32_t u) { return std::isfinite(rows[u].seconds) ? rows[u].seconds : 0.0f; };   // (a strict weak order)
    std::stable_sort(perm.begin(), perm.end(), [&](uint32_t a, uint32_t c) {
        if (n_out && outlier[a] != outlier[c]) return outlier[a] < outlier[c];
        return ragged && key(a) > key(c);
    });
    HIP_TRY(upload(b->d_perm, perm.data(), n_utt, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    if (n_out) {
        // two row groups: the batch's facts, each with the summary of its own rows
        b->groups.resize(2);
        for (int g = 0; g < 2; ++g) {
            RowGroup &v = b->groups[g];
            static_cast<BatchFacts &>(v) = *b;
            v.slot0 = g ? n_utt - n_out : 0u;
            v.n_utt = g ? n_out : n_utt - n_out;
            clear_summary(v);
        }
        for (uint32_t u = 0; u < n_utt; ++u) add_row(b->groups[outlier[u]], rows[u]);
        b->groups_epoch = ctx->voices_epoch;
    }
    // What ragged_plan() and ragged_cost() weigh the lane mappings with: per 8 launch slots the longest row and the rows'
    // segment and kink counts — of the whole batch in launch order, and, where a few rows the lean kernel families cannot take
    // were put last, of the OTHER rows by themselves too: the first row group is the corpus, and one zero-length
    // segment among 65 536 speech-like utterances must not cost the rest their plan.  (A group is planned by its rows' lengths
    // only if they differ THEMSELVES: an aligned batch with a few odd rows is ragged only through those, and its first group
    // keeps the aligned plan — the model prices every lane's events as its own, which an aligned group's are not.)
    auto summarise = [&](BatchFacts &t, const uint32_t n_rows) {
        const size_t n_gran = ((size_t)n_rows + 7) / 8;
        t.granule_samples.assign(n_gran, 0.0f);
        t.granule_segs.assign(n_gran, 0u);
        t.granule_kinks.assign(n_gran, 0u);
        for (uint32_t s = 0; s < n_rows; ++s) {
            const RowStats &r = rows[perm[s]];
            const float samples = key(perm[s]) * ctx->facts.max_rate;
            if (samples > t.granule_samples[s / 8]) t.granule_samples[s / 8] = samples;
            t.granule_segs[s / 8] += r.segs;
            t.granule_kinks[s / 8] += r.kinks;
        }
    };
    if (ragged && n_out) {
        float llo = INFINITY, lhi = -INFINITY;
        for (uint32_t u = 0; u < n_utt; ++u)
            if (!outlier[u]) {
                llo = std::fmin(llo, rows[u].seconds);
                lhi = std::fmax(lhi, rows[u].seconds);
            }
        if (lhi - llo > 0.002f) {
            summarise(b->groups[0], n_utt - n_out);
            summarise(*b, n_utt);
        }
    } else if (ragged) {
        summarise(*b, n_utt);
    }
    b->perm_host.swap(perm);
    return GRAIL_OK;
}

// the voices a batch names: used_voices and max_voice_id (no ids: voice 0 for all)
void name_voices(BatchFacts &b, const uint32_t *voice_ids, uint32_t n_utt)
{
    b.max_voice_id = 0;
    b.used_voices.assign(1, 0u);
    if (!voice_ids || !n_utt) return;
    b.used_voices.assign(voice_ids, voice_ids + n_utt);
    std::sort(b.used_voices.begin(), b.used_voices.end());
    b.used_voices.erase(std::unique(b.used_voices.begin(), b.used_voices.end()), b.used_voices.end());
    b.max_voice_id = b.used_voices.back();
}

int upload_common(grail_ctx *ctx, grail_batch *b, const uint32_t *seg_offsets,
                  const uint32_t *voice_ids, const uint32_t *jitter_seeds, uint32_t n_utt)
{
    HIP_TRY(upload(b->d_offsets, seg_offsets, (size_t)n_utt + 1, ctx->stream));
    name_voices(*b, voice_ids, n_utt);
    if (voice_ids) HIP_TRY(upload(b->d_voice_ids, voice_ids, n_utt, ctx->stream));
    if (jitter_seeds) HIP_TRY(upload(b->d_seeds, jitter_seeds, n_utt, ctx->stream));
    b->n_utt = n_utt;
    // host buffers may be freed by the caller right after we return
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return GRAIL_OK;
}

int install_voices(grail_ctx *ctx, const grail_voice *voices, uint32_t n_voices)
{
    if (!voices || n_voices == 0) return fail(GRAIL_ERR_INVALID_ARG, "no voices given");
    std::vector<DevVoice> dv(n_voices);
    std::vector<float> elems((size_t)n_voices * NUM_VOICED * ELEM_FLOATS);
    for (uint32_t v = 0; v < n_voices; ++v) {
        dv[v].sample_rate = voices[v].sample_rate;
        dv[v].jitter_frequency = voices[v].jitter_frequency;
        dv[v].jitter_delta_frequency = voices[v].jitter_delta_frequency;
        dv[v].jitter_delta_formant_frequency = voices[v].jitter_delta_formant_frequency;
        dv[v].jitter_delta_amplitude = voices[v].jitter_delta_amplitude;
        dv[v].elem_base = v * NUM_VOICED;
        dv[v].warmup = voice_warmup(voices[v]);
        dv[v].pad = 0;
        std::memcpy(&elems[(size_t)v * NUM_VOICED * ELEM_FLOATS], voices[v].phonemes,
                    sizeof(grail_synthesis_elem) * NUM_VOICED);
    }
    HIP_TRY(hipStreamSynchronize(ctx->stream));  // kernels may still read the old table
    ctx->voices.clear();                          // a failure below leaves "no voice table set"
    // on the context's own (non-blocking) stream: ordered with the kernels that read the table
    HIP_TRY(upload(ctx->d_voices, dv.data(), dv.size(), ctx->stream));
    HIP_TRY(upload(ctx->d_voice_elems, elems.data(), elems.size(), ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));   // dv / elems are locals
    // what the table qualifies for, voice by voice and folded over the table; assigned whole, so that no fact of the
    // table before survives
    VoiceFacts facts;
    facts.voices_upper_silent = facts.voices_live4_ok = facts.voices_scan_ok = facts.voices_split_ok = true;
    facts.voices_sharpness = 0.0;
    facts.voice_info.resize(n_voices);
    facts.voice_sharpness.resize(n_voices);
    for (uint32_t v = 0; v < n_voices; ++v) {
        VoiceInfo &vi = facts.voice_info[v];
        vi.upper_silent = true;
        for (int p = 0; p < NUM_VOICED; ++p)
            for (int i = NF / 2; i < NF; ++i) {
                uint32_t bits;
                std::memcpy(&bits, &voices[v].phonemes[p].formant_amp[i], sizeof bits);
                vi.upper_silent = vi.upper_silent && bits == 0u;
            }
        vi.live4_ok = live4_ok(voices[v]);
        vi.scan_ok = scan_voice_ok(voices[v]);
        vi.warmup = dv[v].warmup;
        vi.split_ok = dv[v].warmup != 0u && voices[v].sample_rate > 0.0f && std::isfinite(voices[v].sample_rate);
        facts.voices_upper_silent = facts.voices_upper_silent && vi.upper_silent;
        facts.voices_live4_ok = facts.voices_live4_ok && vi.live4_ok;
        facts.voices_scan_ok = facts.voices_scan_ok && vi.scan_ok;
        facts.voices_split_ok = facts.voices_split_ok && vi.split_ok;
        if (vi.warmup > facts.max_warmup) facts.max_warmup = vi.warmup;
        if (voices[v].sample_rate > facts.max_rate) facts.max_rate = voices[v].sample_rate;
        const float dt = 1.0f / voices[v].sample_rate;
        if (!(dt <= facts.max_dt)) facts.max_dt = dt;       // NaN-proof max
        const float pj = std::fabs(voices[v].jitter_delta_frequency);
        if (!(pj <= facts.max_pitch_jitter)) facts.max_pitch_jitter = pj;
        facts.voice_sharpness[v] = elems_sharpness(voices[v].phonemes, NUM_VOICED);
        facts.voices_sharpness = std::fmax(facts.voices_sharpness, facts.voice_sharpness[v]);
    }
    ctx->voices.assign(voices, voices + n_voices);
    ctx->voices_epoch = ++g_epoch;
    ctx->facts = std::move(facts);
    return GRAIL_OK;
}

int check_ready(grail_ctx *ctx, const grail_batch *batch)
{
    if (!batch) return fail(GRAIL_ERR_INVALID_ARG, "batch is NULL");
    if (ctx->voices.empty() || !ctx->d_voices.get() || !ctx->d_voice_elems.get())   // also after a failed upload
        return fail(GRAIL_ERR_NO_VOICES, "call grail_set_voices first");
    if (batch->max_voice_id >= ctx->voices.size())
        return fail(GRAIL_ERR_INVALID_ARG, "a voice id exceeds the voice table");
    return GRAIL_OK;
}

}  // namespace host
}  // namespace grail

extern "C" {

int grail_abi_version(void) { return GRAIL_ABI_VERSION; }

const char *grail_status_string(int status)
{
    switch (status) {
    case GRAIL_OK: return "ok";
    case GRAIL_ERR_INVALID_ARG: return "invalid argument";
    case GRAIL_ERR_NO_DEVICE: return "no usable HIP device (there is no CPU fallback)";
    case GRAIL_ERR_HIP: return "HIP runtime error";
    case GRAIL_ERR_BUFFER_TOO_SMALL: return "an utterance did not end within out_stride samples";
    case GRAIL_ERR_OUT_OF_MEMORY: return "out of device memory";
    case GRAIL_ERR_RCCL: return "RCCL error";
    case GRAIL_ERR_NO_VOICES: return "no voice table set";
    default: return "unknown status";
    }
}

const char *grail_last_error(void) { return g_last_error.c_str(); }

int grail_device_count(int *count)
{
    if (!count) return fail(GRAIL_ERR_INVALID_ARG, "count is NULL");
    *count = 0;
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess) return hip_fail(e, "hipGetDeviceCount");
    *count = n;
    return GRAIL_OK;
}

int grail_device_pci_bus_id(grail_ctx *ctx, char *out, size_t cap)
{
    if (!ctx || !out || cap < 16) return fail(GRAIL_ERR_INVALID_ARG, "grail_device_pci_bus_id: NULL argument or cap < 16");
    out[0] = 0;
    HIP_TRY(hipDeviceGetPCIBusId(out, (int)cap, ctx->device));
    return GRAIL_OK;
}

int grail_create(int device, grail_ctx **out)
{
    if (!out) return fail(GRAIL_ERR_INVALID_ARG, "out is NULL");
    *out = nullptr;
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n <= 0)
        return fail(GRAIL_ERR_NO_DEVICE,
                    std::string("no HIP device: ") + (e != hipSuccess ? hipGetErrorString(e) : "count 0"));
    if (device < 0 || device >= n) return fail(GRAIL_ERR_NO_DEVICE, "device index out of range");
    HIP_TRY(hipSetDevice(device));
    // the kernels in this library are gfx950 code objects only, and the launch policy is laid out for CDNA4's
    // 4 SIMDs x 64 lanes per compute unit: any other architecture is "no usable device"
    hipDeviceProp_t prop;
    HIP_TRY(hipGetDeviceProperties(&prop, device));
    if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return fail(GRAIL_ERR_NO_DEVICE, std::string("device ") + std::to_string(device) + " is " + prop.gcnArchName +
                                             ": this library holds gfx950 (MI355X) kernels only");
    if (prop.multiProcessorCount <= 0) return fail(GRAIL_ERR_NO_DEVICE, "the device reports no compute units");
    std::unique_ptr<grail_ctx> ctx(new (std::nothrow) grail_ctx());
    if (!ctx) return fail(GRAIL_ERR_OUT_OF_MEMORY, "host allocation failed");
    ctx->device = device;
    ctx->cus = ctx->device_cus = prop.multiProcessorCount;
    hipError_t err;
    if ((err = ctx->stream.create()) != hipSuccess ||
        (err = ctx->ev_start.create(true)) != hipSuccess ||
        (err = ctx->ev_stop.create(true)) != hipSuccess ||
        (err = ctx->d_truncated.alloc(TRUNCATED_WORDS)) != hipSuccess ||
        (err = hipMemsetAsync(ctx->d_truncated.get(), 0, TRUNCATED_WORDS * sizeof(uint32_t), ctx->stream)) != hipSuccess ||
        (err = hipStreamSynchronize(ctx->stream)) != hipSuccess)
        return hip_fail(err, "grail_create");       // (what exists so far goes with ctx)
    *out = ctx.release();
    return GRAIL_OK;
}

int grail_destroy(grail_ctx *ctx)
{
    if (!ctx) return GRAIL_OK;
    (void)hipSetDevice(ctx->device);
    if (ctx->stream) (void)hipStreamSynchronize(ctx->stream);
    comm_release(ctx);
    delete ctx;
    return GRAIL_OK;
}

int grail_set_voices(grail_ctx *ctx, const grail_voice *voices, uint32_t n_voices)
{
    int rc = bind(ctx);
    if (rc) return rc;
    return install_voices(ctx, voices, n_voices);
}

int grail_get_voices(grail_ctx *ctx, grail_voice *voices, uint32_t cap, uint32_t *n_voices)
{
    if (!ctx) return fail(GRAIL_ERR_INVALID_ARG, "ctx is NULL");
    if (n_voices) *n_voices = (uint32_t)ctx->voices.size();
    if (voices)
        for (uint32_t i = 0; i < cap && i < ctx->voices.size(); ++i) voices[i] = ctx->voices[i];
    return GRAIL_OK;
}

uint64_t grail_length_bound(const float *segment_lengths, uint32_t n_segments, float sample_rate)
{
    if (!(sample_rate > 0.0f) || (n_segments && !segment_lengths)) return UINT64_MAX;
    const double dt = (double)(1.0f / sample_rate);
    double samples = 0.0;
    for (uint32_t i = 0; i < n_segments; ++i) {
        if (!std::isfinite(segment_lengths[i])) return UINT64_MAX;
        samples += segment_bound(segment_lengths[i], dt);
    }
    return samples < 1.8e19 ? (uint64_t)samples : UINT64_MAX;
}

int grail_batch_upload(grail_ctx *ctx, const grail_phoneme_elem *segs, const uint32_t *seg_offsets,
                       const uint32_t *voice_ids, const uint32_t *jitter_seeds, uint32_t n_utt,
                       grail_batch **out)
{
    int rc = bind(ctx);
    if (rc) return rc;
    if (!out) return fail(GRAIL_ERR_INVALID_ARG, "out is NULL");
    *out = nullptr;
    uint32_t n_segs = 0;
    if ((rc = check_offsets(seg_offsets, n_utt, &n_segs))) return rc;
    if (n_segs && !segs) return fail(GRAIL_ERR_INVALID_ARG, "segs is NULL");
    for (uint32_t i = 0; i < n_segs; ++i)
        if (segs[i].phoneme < 0 || segs[i].phoneme >= GRAIL_PH_COUNT)
            return fail(GRAIL_ERR_INVALID_ARG, "phoneme discriminant out of range");
    std::unique_ptr<grail_batch> b(new (std::nothrow) grail_batch());
    if (!b) return fail(GRAIL_ERR_OUT_OF_MEMORY, "host allocation failed");
    b->phoneme_mode = true;
    b->n_segs = n_segs;
    const std::vector<RowStats> rows = batch_stats(ctx, b.get(), segs, seg_offsets, n_utt,
                                                   [](float f) { return std::fmin(f, 0.5f); });   // copy_with_frequency :445-450
    HIP_TRY(upload(b->d_segs, segs, n_segs, ctx->stream));
    if ((rc = upload_common(ctx, b.get(), seg_offsets, voice_ids, jitter_seeds, n_utt)) ||
        (rc = upload_len_bound(ctx, b.get(), rows, n_utt)) || (rc = upload_length_order(ctx, b.get(), rows, n_utt)))
        return rc;
    *out = b.release();
    return GRAIL_OK;
}

int grail_batch_upload_elems(grail_ctx *ctx, const grail_sequence_elem *segs,
                             const uint32_t *seg_offsets, const uint32_t *voice_ids,
                             const uint32_t *jitter_seeds, uint32_t n_utt, grail_batch **out)
{
    int rc = bind(ctx);
    if (rc) return rc;
    if (!out) return fail(GRAIL_ERR_INVALID_ARG, "out is NULL");
    *out = nullptr;
    uint32_t n_segs = 0;
    if ((rc = check_offsets(seg_offsets, n_utt, &n_segs))) return rc;
    if (n_segs && !segs) return fail(GRAIL_ERR_INVALID_ARG, "segs is NULL");
    // Split the SequenceElems into the 16-B segment records and the elem table.
    std::vector<DevSeg> ds(n_segs);
    std::vector<float> elems((size_t)(n_segs ? n_segs : 1) * ELEM_FLOATS);
    for (uint32_t i = 0; i < n_segs; ++i) {
        ds[i].elem = segs[i].has_elem ? (int32_t)i : -1;
        ds[i].length = segs[i].length;
        ds[i].blend_length = segs[i].blend_length;
        ds[i].frequency = segs[i].elem.frequency;
        std::memcpy(&elems[(size_t)i * ELEM_FLOATS], &segs[i].elem, sizeof(grail_synthesis_elem));
    }
    std::unique_ptr<grail_batch> b(new (std::nothrow) grail_batch());
    if (!b) return fail(GRAIL_ERR_OUT_OF_MEMORY, "host allocation failed");
    b->phoneme_mode = false;
    b->n_segs = n_segs;
    // (a caller-built elem keeps its frequency as it is: copy_with_frequency's min(f, 0.5) :445-450 belongs to the Selector)
    const std::vector<RowStats> rows = batch_stats(ctx, b.get(), ds.data(), seg_offsets, n_utt, [](float f) { return f; });
    // The elems of the batch, interned by their formant arrays (everything but the pitch, which none of the analyses
    // below looks at): a corpus names a few dozen distinct parameter sets in hundreds of thousands of segments.
    struct FormantsHash {
        size_t operator()(const float *p) const
        {
            uint64_t h = 0x9E3779B97F4A7C15ull, w;
            for (int i = 0; i < 24; ++i) {                   // 48 floats after the frequency
                std::memcpy(&w, p + 1 + 2 * i, sizeof w);
                h = (h ^ w) * 0xFF51AFD7ED558CCDull;
                h ^= h >> 29;
            }
            return (size_t)h;
        }
    };
    struct FormantsEq {
        bool operator()(const float *a, const float *c) const { return std::memcmp(a + 1, c + 1, 48 * sizeof(float)) == 0; }
    };
    std::unordered_map<const float *, uint32_t, FormantsHash, FormantsEq> ids;
    std::vector<grail_synthesis_elem> distinct;
    std::vector<uint32_t> id_of(n_segs, 0xFFFFFFFFu);
    for (uint32_t i = 0; i < n_segs; ++i) {
        if (!segs[i].has_elem) continue;
        const auto it = ids.emplace((const float *)&segs[i].elem, (uint32_t)distinct.size());
        if (it.second) distinct.push_back(segs[i].elem);
        id_of[i] = it.first->second;
    }
    // the sharpness of the batch (elems_sharpness): parameters only ever blend between the elems of two consecutive
    // segments of an utterance (Sequencer::next :897-921), so every such pair is judged like a voice of two phonemes
    // (once per distinct pair)
    std::unordered_map<uint64_t, double> pair_sharpness;
    for (uint32_t u = 0; u < n_utt; ++u)
        for (uint32_t i = seg_offsets[u]; i < seg_offsets[u + 1]; ++i) {
            if (!segs[i].has_elem) continue;
            const uint32_t a = id_of[i];
            const uint32_t c = (i + 1 < seg_offsets[u + 1] && segs[i + 1].has_elem) ? id_of[i + 1] : a;
            const uint64_t key = ((uint64_t)std::min(a, c) << 32) | std::max(a, c);
            auto it = pair_sharpness.find(key);
            if (it == pair_sharpness.end()) {
                const grail_synthesis_elem pair[2] = {distinct[a], distinct[c]};
                it = pair_sharpness.emplace(key, elems_sharpness(pair, a == c ? 1 : 2)).first;
            }
            b->elems_sharpness = std::fmax(b->elems_sharpness, it->second);
        }
    HIP_TRY(upload(b->d_segs, ds.data(), n_segs, ctx->stream));
    HIP_TRY(upload(b->d_elems, elems.data(), elems.size(), ctx->stream));
    if ((rc = upload_common(ctx, b.get(), seg_offsets, voice_ids, jitter_seeds, n_utt)) ||
        (rc = upload_len_bound(ctx, b.get(), rows, n_utt)) || (rc = upload_length_order(ctx, b.get(), rows, n_utt)))
        return rc;
    // the warm-up length of the time-split fast kernels for THESE elems (elems_warmup: the slowest filter over the distinct
    // elems of the batch, the formant-frequency jitter of the voices it names), valid for the voice table of this moment;
    // 0: the batch does not qualify and fast arithmetic renders it with the lane kernels
    if (!ctx->voices.empty() && b->max_voice_id < ctx->voices.size()) {
        double jd = 0.0;
        bool rates_ok = true;
        for (const uint32_t v : b->used_voices) {
            jd = std::fmax(jd, std::fabs((double)ctx->voices[v].jitter_delta_formant_frequency));
            rates_ok = rates_ok && ctx->voices[v].sample_rate > 0.0f && std::isfinite(ctx->voices[v].sample_rate);
        }
        // can formants 5-8 be left out (the four-formant kernels)?  As for a voice table (live4_ok): the scalars of the
        // voices named, and every distinct elem of the batch
        bool voices4 = true;
        for (const uint32_t v : b->used_voices) {
            grail_voice scalars = ctx->voices[v];
            for (int ph = 0; ph < NUM_VOICED; ++ph) grail_elem_silent(&scalars.phonemes[ph]);     // (only the scalars count here)
            voices4 = voices4 && live4_ok(scalars);
        }
        b->elems_live4_ok = voices4 && live4_elems_ok(distinct.data(), distinct.size(), (float)jd);
        b->elems_warmup = rates_ok ? elems_warmup(distinct.data(), distinct.size(), jd) : 0u;
        // ... and whether the scan kernel may take them (its window has no IEEE fallback; pitches as the Selector
        // would have left them: at most 1/2)
        float max_pitch = 0.0f;
        for (uint32_t i = 0; i < n_segs; ++i) max_pitch = std::fmax(max_pitch, segs[i].elem.frequency);
        b->elems_scan_ok = rates_ok && max_pitch <= 0.5f && scan_elems_ok(distinct.data(), distinct.size(), (float)jd);
        b->elems_warmup_epoch = ctx->voices_epoch;
        for (RowGroup &g : b->groups) {             // (the groups were made before these were known)
            g.elems_warmup = b->elems_warmup;
            g.elems_warmup_epoch = b->elems_warmup_epoch;
            g.elems_live4_ok = b->elems_live4_ok;
            g.elems_scan_ok = b->elems_scan_ok;
        }
    }
    *out = b.release();
    return GRAIL_OK;
}

int grail_batch_free(grail_ctx *ctx, grail_batch *batch)
{
    if (!batch) return GRAIL_OK;
    int rc = bind(ctx);
    if (rc) return rc;
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    delete batch;          // (its device arrays, packed tables and plans go with it)
    return GRAIL_OK;
}

uint32_t grail_batch_size(const grail_batch *batch) { return batch ? batch->n_utt : 0; }

int grail_batch_lengths(grail_ctx *ctx, const grail_batch *batch, uint32_t max_len,
                        uint32_t *out_len)
{
    int rc = bind(ctx);
    if (rc) return rc;
    if ((rc = check_ready(ctx, batch))) return rc;
    if (!out_len && batch->n_utt) return fail(GRAIL_ERR_INVALID_ARG, "out_len is NULL");
    if (batch->n_utt == 0) return GRAIL_OK;
    DeviceBuffer<uint32_t> d_len;
    HIP_TRY(d_len.alloc(batch->n_utt));
    LenArgs a{};
    a.segs = batch->d_segs.get();
    a.seg_offsets = batch->d_offsets.get();
    a.voice_ids = batch->d_voice_ids.get();
    a.voices = ctx->d_voices.get();
    a.out_len = d_len.get();
    a.n_utt = batch->n_utt;
    a.n_voices = (uint32_t)ctx->voices.size();
    a.max_len = max_len;
    HIP_TRY(launch_lengths(a, ctx->stream));
    HIP_TRY(hipMemcpyAsync(out_len, d_len.get(), (size_t)batch->n_utt * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return GRAIL_OK;
}

int grail_sync(grail_ctx *ctx)
{
    int rc = bind(ctx);
    if (rc) return rc;
    // flag read-back and reset travel on the stream the kernels run on (a non-blocking stream has
    // no implicit ordering with the null stream)
    uint32_t flags[4] = {0, 0, 0, 0};
    HIP_TRY(hipMemcpyAsync(flags, ctx->d_truncated.get(), sizeof flags, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    const uint32_t flag = flags[0];
    // the statistics counters are cumulative on the device (u32, wrapping): the host takes differences, so the usual
    // call costs one copy and one synchronisation; only a truncation flag has to be cleared
    ctx->stats.slow_steps += (uint32_t)(flags[1] - ctx->seen_counters[1]);
    ctx->stats.fast_tiles += (uint32_t)(flags[2] - ctx->seen_counters[2]);
    ctx->stats.general_steps += (uint32_t)(flags[3] - ctx->seen_counters[3]);
    for (int i = 1; i < 4; ++i) ctx->seen_counters[i] = flags[i];
    if (flag) {
        HIP_TRY(hipMemsetAsync(ctx->d_truncated.get(), 0, sizeof(uint32_t), ctx->stream));
        HIP_TRY(hipStreamSynchronize(ctx->stream));
    }
    if (flag) {
        return fail(GRAIL_ERR_BUFFER_TOO_SMALL,
                    "at least one utterance did not end within out_stride samples");
    }
    return GRAIL_OK;
}

const char *grail_last_kernel_name(grail_ctx *ctx) { return ctx ? ctx->stats.last_kernel.c_str() : "none"; }

int grail_last_kernel_ms(grail_ctx *ctx, float *ms)
{
    int rc = bind(ctx);
    if (rc) return rc;
    if (!ms) return fail(GRAIL_ERR_INVALID_ARG, "ms is NULL");
    if (!ctx->have_timing) return fail(GRAIL_ERR_INVALID_ARG, "no kernel has been launched");
    HIP_TRY(hipEventSynchronize(ctx->ev_stop));
    HIP_TRY(hipEventElapsedTime(ms, ctx->ev_start, ctx->ev_stop));
    return GRAIL_OK;
}

int grail_pcm16_async(grail_ctx *ctx, const float *in_dev, uint64_t in_stride,
                      const uint32_t *len_dev, uint32_t n_utt, uint32_t max_len, int16_t *out_dev,
                      uint64_t out_stride)
{
    int rc = bind(ctx);
    if (rc) return rc;
    if (n_utt && (!in_dev || !len_dev || !out_dev)) return fail(GRAIL_ERR_INVALID_ARG, "NULL buffer");
    hipError_t e = launch_pcm16(in_dev, in_stride, len_dev, n_utt, max_len, out_dev, out_stride,
                                ctx->stream);
    if (e != hipSuccess) return hip_fail(e, "pcm16 kernel launch");
    return GRAIL_OK;
}

int grail_batch_digest(grail_ctx *ctx, const float *in_dev, uint64_t in_stride,
                       const uint32_t *len_dev, uint32_t n_utt, uint64_t *sums, float *maxabs,
                       uint32_t *nonfinite)
{
    int rc = bind(ctx);
    if (rc) return rc;
    if (n_utt == 0) return GRAIL_OK;
    if (!in_dev || !len_dev || !sums || !maxabs || !nonfinite)
        return fail(GRAIL_ERR_INVALID_ARG, "NULL buffer");
    DeviceBuffer<unsigned long long> d_s;
    DeviceBuffer<float> d_m;
    DeviceBuffer<uint32_t> d_b;
    HIP_TRY(d_s.alloc(n_utt));
    HIP_TRY(d_m.alloc(n_utt));
    HIP_TRY(d_b.alloc(n_utt));
    HIP_TRY(launch_digest(in_dev, in_stride, len_dev, n_utt, d_s.get(), d_m.get(), d_b.get(), ctx->stream));
    HIP_TRY(hipMemcpyAsync(sums, d_s.get(), (size_t)n_utt * 8, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipMemcpyAsync(maxabs, d_m.get(), (size_t)n_utt * 4, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipMemcpyAsync(nonfinite, d_b.get(), (size_t)n_utt * 4, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return GRAIL_OK;
}

int grail_batch_compare(grail_ctx *ctx, const float *a_dev, const float *b_dev, uint64_t stride,
                        const uint32_t *len_a_dev, const uint32_t *len_b_dev, uint32_t n_utt, float *maxdiff,
                        double *sumsq, uint32_t *mismatches)
{
    int rc = bind(ctx);
    if (rc) return rc;
    if (n_utt == 0) return GRAIL_OK;
    if (!a_dev || !b_dev || !len_a_dev || !len_b_dev || !maxdiff || !sumsq || !mismatches)
        return fail(GRAIL_ERR_INVALID_ARG, "NULL buffer");
    DeviceBuffer<float> d_m;
    DeviceBuffer<double> d_q;
    DeviceBuffer<uint32_t> d_b;
    HIP_TRY(d_m.alloc(n_utt));
    HIP_TRY(d_q.alloc(n_utt));
    HIP_TRY(d_b.alloc(n_utt));
    HIP_TRY(launch_compare(a_dev, b_dev, stride, len_a_dev, len_b_dev, n_utt, d_m.get(), d_q.get(), d_b.get(), ctx->stream));
    HIP_TRY(hipMemcpyAsync(maxdiff, d_m.get(), (size_t)n_utt * 4, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipMemcpyAsync(sumsq, d_q.get(), (size_t)n_utt * 8, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipMemcpyAsync(mismatches, d_b.get(), (size_t)n_utt * 4, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return GRAIL_OK;
}

int grail_device_alloc(grail_ctx *ctx, size_t bytes, void **out)
{
    int rc = bind(ctx);
    if (rc) return rc;
    if (!out) return fail(GRAIL_ERR_INVALID_ARG, "out is NULL");
    *out = nullptr;
    HIP_TRY(hipMalloc(out, bytes ? bytes : 1));
    return GRAIL_OK;
}

int grail_device_free(grail_ctx *ctx, void *ptr)
{
    int rc = bind(ctx);
    if (rc) return rc;
    if (ptr) HIP_TRY(hipFree(ptr));
    return GRAIL_OK;
}

int grail_host_alloc(grail_ctx *ctx, size_t bytes, void **out)
{
    int rc = bind(ctx);
    if (rc) return rc;
    if (!out) return fail(GRAIL_ERR_INVALID_ARG, "out is NULL");
    *out = nullptr;
    HIP_TRY(hipHostMalloc(out, bytes ? bytes : 1, hipHostMallocDefault));
    return GRAIL_OK;
}

int grail_host_free(grail_ctx *ctx, void *ptr)
{
    int rc = bind(ctx);
    if (rc) return rc;
    if (ptr) HIP_TRY(hipHostFree(ptr));
    return GRAIL_OK;
}

int grail_memcpy_d2h(grail_ctx *ctx, void *dst_host, const void *src_dev, size_t bytes)
{
    int rc = bind(ctx);
    if (rc) return rc;
    HIP_TRY(hipMemcpyAsync(dst_host, src_dev, bytes, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return GRAIL_OK;
}

int grail_memcpy_h2d(grail_ctx *ctx, void *dst_dev, const void *src_host, size_t bytes)
{
    int rc = bind(ctx);
    if (rc) return rc;
    HIP_TRY(hipMemcpyAsync(dst_dev, src_host, bytes, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return GRAIL_OK;
}

int grail_memset_d(grail_ctx *ctx, void *dst_dev, int value, size_t bytes)
{
    int rc = bind(ctx);
    if (rc) return rc;
    HIP_TRY(hipMemsetAsync(dst_dev, value, bytes, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return GRAIL_OK;
}

}  // extern "C"
