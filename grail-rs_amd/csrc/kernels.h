// kernels.h — device-side data layout and launcher prototypes (internal).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace grail {

constexpr int NF = 8;            // NUM_FORMANTS, reference src/lib.rs:24
constexpr int ELEM_FLOATS = 49;  // SynthesisElem, reference src/lib.rs:316-337
constexpr int NUM_VOICED = 2;    // VoiceStorage {a, e}, reference src/lib.rs:653-659
constexpr int PH_FIRST_VOICED = 3;
constexpr int SPLIT_MAX_CHUNKS = 64;   // time-split fast kernels: chunks per utterance

// field offsets inside a 49-float SynthesisElem (declared order)
constexpr int F_FREQ = 1, F_BW = 9, F_SMOOTH = 17, F_BREATH = 25, F_TURB = 33, F_AMP = 41;

// One segment as the kernel reads it: 16 B, one dwordx4 load.
// Phoneme mode: bit-identical to grail_phoneme_elem (PhonemeElem, src/lib.rs:961-973),
//   `elem` holds the Phoneme discriminant and the Selector runs on the device.
// Elem mode: `elem` is the row of the batch's elem table, or -1 for None
//   (SequenceElem.elem, src/lib.rs:817), `frequency` repeats the elem's own.
struct DevSeg {
    int32_t elem;
    float length;
    float blend_length;
    float frequency;
};
static_assert(sizeof(DevSeg) == 16, "DevSeg must be one dwordx4");

// Per-voice scalars (Voice, src/lib.rs:696-717) + where its phoneme elems sit
// in the elem table. 32 B.
struct DevVoice {
    float sample_rate;
    float jitter_frequency;
    float jitter_delta_frequency;
    float jitter_delta_formant_frequency;
    float jitter_delta_amplitude;
    uint32_t elem_base;  // row of phonemes.a in the voice elem table
    uint32_t warmup;     // time-split fast kernels: samples after which a filter state started from zero has
                         // decayed below half an ulp of full scale (a multiple of 64; 0: the voice does not qualify)
    uint32_t pad;
};
static_assert(sizeof(DevVoice) == 32, "DevVoice layout");

struct SynthArgs {
    const DevSeg *segs;
    const uint32_t *seg_offsets;  // [n_utt + 1]
    const uint32_t *voice_ids;    // [n_utt] or nullptr (voice 0)
    const uint32_t *seeds;        // [n_utt] or nullptr (seed 0)
    const uint32_t *perm;         // [n_utt] or nullptr: launch slot -> utterance (ragged batches: sorted by
                                  // length on upload, so the lanes of a wave end together)
    const float *elems;           // phoneme mode: voice elem table; elem mode: batch elem table
    const DevVoice *voices;
    float *out;
    int16_t *out_pcm16;           // not nullptr: rows of i16 PCM instead (examples/cli.rs:49 fused
                                  // into the tile flush); `out` is then unused
    uint32_t *out_len;            // may be nullptr
    uint32_t *truncated;          // [0]: set to 1 when an utterance is cut at out_stride;
                                  // [1]: += wave-steps that ran the IEEE-division body
                                  // [2]: += wave-tiles rendered in fast arithmetic, [3]: += general wave-steps
    uint64_t out_stride;          // samples between rows
    uint64_t cap;                 // samples a row may receive in this launch (<= out_stride)
    uint32_t n_utt;
    uint32_t n_voices;
    uint32_t phoneme_mode;        // 1: run the Selector on the device
    uint32_t skip_silent;         // 1: skip the band-pass of formant vectors proven silent (same bits)
    uint32_t half_capable;        // host hint: every voice has amplitude 0 in formants 5-8 of every
                                  // phoneme (phoneme batches) / every elem of the batch has (caller-built elems,
                                  // with parameters that keep them at +0: live4_elems_ok), so the half-live loops can be used
    uint32_t live4;               // host-verified: formants 5-8 contribute exactly +0.0 for the whole
                                  // batch (see voice_analysis.cpp live4_ok); selects the NFA = 4 kernels
    uint32_t pipe;                // live4 batches small enough to leave SIMDs idle: the four-wave
                                  // pipelined workgroups (synth_kernel<..., PIPE>)
    uint32_t fast;                // tolerance-mode arithmetic in calm tiles (option "arithmetic" = 1): 1 = coefficients
                                  // interpolated, 2 = the reference's own coefficients at every sample (MID)
    uint32_t any_blend;           // host hint: some segment has a blend length that is not +-2^k
    uint32_t cohabit;             // lane kernels on 2 / 4 / 8 lanes per utterance: the instantiation built for two waves per
                                  // SIMD (launches of more waves than the device has SIMDs; family_cost.cpp family_cohabits)
    const uint32_t *len_bound;    // time-split kernels: per utterance an upper bound of its length in samples, or nullptr — a
                                  // chunk's lane whose utterance ends before the chunk begins renders nothing
    uint32_t pipe_fill;           // pipelined workgroups, one-shot: utterances per workgroup (0: all 16 / 8 slots) — a small batch
                                  // of rows that differ in length is spread thinly, so that a workgroup's tiles hold few events
    uint32_t fold_from;           // two waves per SIMD, at most two rounds of the device: workgroups from this index on take the
                                  // launch slots in reverse order (0: none) — see synth_kernel.h
    uint32_t *state;              // resumable synthesis: state[word][lane] or nullptr (one-shot)
    uint64_t state_stride;        // lanes of the launch (= state_lanes())
    uint32_t resume;              // 1: load the state first (not the first call of a stream)
    // live streams (grail_stream_open_live: the lazy source of examples/interactive.rs:31-38): the segments of
    // utterance u sit in a ring, segs[u * ring_cap + (i & (ring_cap - 1))] for its i-th segment ever appended;
    // seg_counts[u] of them have been appended so far, and while seg_open[u] != 0 more may follow: a Sequencer that
    // needs a segment which is not there yet PAUSES (src/lib.rs:866-888 pulls iter.next() on demand) instead of
    // ending the utterance.  seg_offsets is unused then.
    uint32_t ring_cap;            // 0: not a live stream
    const uint32_t *seg_counts;   // [n_utt]
    const uint32_t *seg_open;     // [n_utt]
    uint32_t *seg_consumed;       // [n_utt] out: segments the Sequencer has pulled so far
    // time-split fast kernels (synth_kernel<..., SPLIT>): chunk k of every utterance is the samples
    // [split_bounds[k], split_bounds[k + 1]) (multiples of 64; the last bound is `cap`), one lane each
    uint32_t split_chunks;        // K, 0: not a time-split launch
    uint32_t split_warmup;        // caller-built elems: the warm-up length of the batch (0: the lane's voice has it, DevVoice::warmup)
    uint32_t split_bounds[SPLIT_MAX_CHUNKS + 1];
};

struct LenArgs {
    const DevSeg *segs;
    const uint32_t *seg_offsets;
    const uint32_t *voice_ids;
    const DevVoice *voices;
    uint32_t *out_len;
    uint32_t n_utt;
    uint32_t n_voices;
    uint32_t max_len;
};

// Launches `yes` where `flag` holds and `no` otherwise, two instantiations of one kernel template (16-byte against 4-byte
// accesses, say): a launcher names its kernel's arguments once, whichever variant runs.
template <typename... Params, typename... Args>
void launch_either(bool flag, void (*yes)(Params...), void (*no)(Params...), dim3 grid, dim3 block, uint32_t lds, hipStream_t stream,
                   Args... args)
{
    hipLaunchKernelGGL(flag ? yes : no, grid, block, lds, stream, static_cast<Params>(args)...);
}

// the instantiation the calling thread's last launch_synth started, e.g. "synth_kernel<L=1,T=32,...>"
const char *last_kernel_name();
// lanes_per_utt in {1, 2, 4, 8}; returns hipSuccess or the launch error.
hipError_t launch_synth(const SynthArgs &args, int lanes_per_utt, hipStream_t stream);
hipError_t launch_lengths(const LenArgs &args, hipStream_t stream);
// live streams: utterance u's new segments new_segs[new_offsets[u] .. new_offsets[u + 1]) go to the next slots of its
// ring and counts[u] grows by their number; elem mode (new_elems != nullptr): new_elems[i] is new_segs[i]'s elem (49
// floats) and the segment's `elem` field is rewritten to the ring slot's row of ring_elems (or stays -1 for None)
hipError_t launch_ring_append(DevSeg *ring, float *ring_elems, uint32_t *counts, uint32_t ring_cap, const DevSeg *new_segs,
                              const float *new_elems, const uint32_t *new_offsets, uint32_t n_utt, hipStream_t stream);
// small batches, fast arithmetic: one workgroup per utterance, lanes = time, recurrences by parallel scan
// (scan_kernels.hip).  args.live4 selects two formant-pair waves instead of four.
hipError_t launch_scan(const SynthArgs &args, hipStream_t stream);
// f32 rows -> i16 PCM rows (examples/cli.rs:49); only the first len[u] (<= max_len) samples of row u
hipError_t launch_pcm16(const float *in, uint64_t in_stride, const uint32_t *len, uint32_t n_utt,
                        uint32_t max_len, int16_t *out, uint64_t out_stride, hipStream_t stream);
// per-row digest (bit-pattern sum mod 2^64, max |x|, count of NaN/Inf) of rendered rows
hipError_t launch_digest(const float *in, uint64_t in_stride, const uint32_t *len, uint32_t n_utt,
                         unsigned long long *sums, float *maxabs, uint32_t *nonfinite,
                         hipStream_t stream);
// per-row distance of two renderings: max |a-b|, sum of squared differences, structural mismatches
hipError_t launch_compare(const float *a, const float *b, uint64_t stride, const uint32_t *len_a,
                          const uint32_t *len_b, uint32_t n_utt, float *maxdiff, double *sumsq, uint32_t *bad,
                          hipStream_t stream);
// resumable synthesis: words per lane and lanes per launch of the state buffer
uint32_t state_words(int lanes_per_utt);
uint64_t state_lanes(uint32_t n_utt, int lanes_per_utt);

// mixing (mix_kernels.hip): one launch of a plan of mix_plan.cpp — a workgroup per (track, span), n_workgroups of them
namespace mix { struct MixItem; }
struct MixArgs {
    const float *rows;
    const mix::MixItem *items;
    const uint32_t *tile_start;
    const uint32_t *tile_items;
    float *tracks;
    uint64_t track_stride, track_len, wg_samples;
    uint32_t wgs_per_track, wgs_per_tile, tiles_per_track, n_workgroups;
    uint32_t samples_per_lane;   // 1 or 8
    uint32_t accumulate;         // GRAIL_MIX_ACCUMULATE
};
hipError_t launch_mix(const MixArgs &args, hipStream_t stream);
// tracks [n_tracks][track_stride] -> interleaved i16 frames[f * n_tracks + t] (examples/cli.rs:49)
hipError_t launch_pcm16_frames(const float *tracks, uint64_t track_stride, uint32_t n_tracks, uint64_t n_frames,
                               int16_t *frames, hipStream_t stream);

// levels (level_kernels.hip): one wave per (row, frame of `frame` samples), grid_frames = ceil(row_stride / frame) of them
// per row; per frame the binary64 sum of squares, the largest finite |x| and the count of non-finite samples, at
// [row * frames_stride + f] (any of the three may be NULL; frames past a row's last are left unwritten)
hipError_t launch_level_frames(const float *rows, uint64_t row_stride, const uint32_t *len, uint32_t n_rows,
                               uint32_t frame, uint32_t grid_frames, double *fsum, float *fpeak, uint32_t *fbad,
                               uint64_t frames_stride, hipStream_t stream);
// ... and a row's totals from them: the sums folded in ascending frame order (outputs may be NULL)
hipError_t launch_level_totals(const uint32_t *len, uint64_t row_stride, uint32_t n_rows, uint32_t frame,
                               const double *fsum, const float *fpeak, const uint32_t *fbad, uint64_t frames_stride,
                               double *sumsq, float *peak, uint32_t *nonfinite, hipStream_t stream);

// loudness (loudness_kernels.hip): one lane per row through the two K-weighting sections (coef: HOST [10]), the sum of
// z*z per hop of `hop` samples at hops[row * hops_stride + h] for the row's floor(n / hop) whole hops, and the count of
// non-finite samples (may be NULL); hops_stride >= row_stride / hop
hipError_t launch_loudness_hops(const float *rows, uint64_t row_stride, const uint32_t *len, uint32_t n_rows, uint32_t hop,
                                const double *coef, double *hops, uint64_t hops_stride, uint32_t *nonfinite,
                                hipStream_t stream);
// ... and a row's gated mean square from its hops, one lane per row
hipError_t launch_loudness_gate(const uint32_t *len, uint64_t row_stride, uint32_t n_rows, uint32_t hop, const double *hops,
                                uint64_t hops_stride, double *gated, hipStream_t stream);
// the segmented form (loudness_segment_kernels.hip): one lane per (row, hop), each hop filtered from a zero state
// GRAIL_LOUDNESS_WARMUP_HOPS hops before its first sample; the same hop layout as launch_loudness_hops, so that
// launch_loudness_gate follows unchanged.  hop_bad: DEVICE [n_rows][loudness_segment_lanes(row_stride, hop)], the hops'
// own non-finite counts (the lane after a row's last whole hop counts the row's tail), folded into nonfinite[n_rows] by
// one lane per row; both NULL where the counts are not asked for.  One launch of n_rows * loudness_segment_waves blocks of
// 64 lanes: a grid holds fewer than 2^32 threads, so more than LOUD_SEGMENT_WAVES_MAX of them is hipErrorInvalidValue.
constexpr uint64_t LOUD_SEGMENT_WAVES_MAX = (1ull << 26) - 1u;
uint64_t loudness_segment_lanes(uint64_t row_stride, uint32_t hop);
uint64_t loudness_segment_waves(uint64_t row_stride, uint32_t hop);
hipError_t launch_loudness_segments(const float *rows, uint64_t row_stride, const uint32_t *len, uint32_t n_rows, uint32_t hop,
                                    const double *coef, double *hops, uint64_t hops_stride, uint32_t *hop_bad,
                                    uint32_t *nonfinite, hipStream_t stream);

// true peak (true_peak_kernels.hip): one wave per (row, chunk of output times), grid_chunks =
// true_peak_grid_chunks(row_stride) of them per row; per chunk the largest |y| of the 4x oversampling filter and the
// count of non-finite samples at [row * grid_chunks + c] (chunks past a row's last are left unwritten)
uint64_t true_peak_grid_chunks(uint64_t row_stride);
hipError_t launch_true_peak_frames(const float *rows, uint64_t row_stride, const uint32_t *len, uint32_t n_rows,
                                   uint32_t grid_chunks, double *cmax, uint32_t *cbad, hipStream_t stream);
// ... and a row's true peak and count from them, one lane per row (outputs may be NULL)
hipError_t launch_true_peak_totals(const uint32_t *len, uint64_t row_stride, uint32_t n_rows, const double *cmax,
                                   const uint32_t *cbad, uint32_t grid_chunks, double *true_peak, uint32_t *nonfinite,
                                   hipStream_t stream);

// Row transforms (limiter, resampler, FIR, meter streams): one struct of arguments a kind, taken by every launcher of the kind,
// one-shot and on streams alike.  A launcher hands its kernel the fields that the kernel's parameters name
// (tests/test_launch_args_host.py holds them to it).  Every pointer is DEVICE unless it says HOST; every result may be NULL.
// Streams: rows (the limiter: groups of rows) fed call by call.  What every kind keeps, said once in row_kernel_common.h:
// the state word (the samples fed so far, bit 63 set once the row has ended), word 0 of a row's state, and a ring of ring_cap
// samples a row, ring_cap a power of two: sample t of a row at t mod ring_cap, +0.0 where it was not finite.  A call launches
// a chunk kernel that reads state and ring and writes out and the chunks' numbers (grid_chunks of them a row: enough for the
// most outputs a row can have in the call, *_plan.cpp), then an advance kernel, the only writer of state and ring.  A row
// that has ended and is fed is refused: 0xFFFFFFFF where its length would stand, 0 non-finite samples, nothing else.
struct RowCallArgs {
    const float *rows;      // [n_rows][row_stride]; row u holds min(len[u], row_stride) samples.  On a stream: the samples the
    uint64_t row_stride;    // call feeds (the kernels' in, in_stride, in_len)
    const uint32_t *len;    // [n_rows]
    uint64_t *state;        // from here on: a call on a stream (a one-shot call leaves the five zero).  [units][the kind's words],
                            // word 0 the state word; units: the rows, or the limiter's groups
    float *ring;            // [n_rows][ring_cap]
    uint32_t ring_cap;
    const uint8_t *mark;    // [units] or NULL (every unit): whom a finishing call ends
    bool finishing;         // rows and len are not read (no samples are fed), the marked units that have not ended write their
                            // tail and end; nonfinite is not written
};

// The two rules every launcher of these kinds follows.  A kernel's VEC instantiation (16-byte accesses) runs where the rows it
// touches start on 16 bytes and lie a multiple of 4 samples apart, else its 4-byte one: the same bits.
inline bool aligned16(const void *rows, uint64_t stride) { return (reinterpret_cast<uintptr_t>(rows) & 15u) == 0 && (stride & 3u) == 0; }
inline bool aligned16(const void *a, uint64_t a_stride, const void *b, uint64_t b_stride) { return aligned16(a, a_stride) && aligned16(b, b_stride); }
// A grid of `workgroups` is launched (true) unless there are none (*e = hipSuccess) or more than 2^31 - 1 (hipErrorInvalidValue).
inline bool grid_fits(uint64_t workgroups, hipError_t *e)
{
    *e = workgroups > 0x7FFFFFFFull ? hipErrorInvalidValue : hipSuccess;
    return workgroups != 0 && *e == hipSuccess;
}

// limiter (limiter_kernels.hip): one workgroup per (group of `group` consecutive rows, chunk of LIMIT_CHUNK samples; a stream:
// of the call's outputs).  state: [n_groups]; ring: [n_groups * group][at or above 3 * 2^ell + 19]; mark: [n_groups].  A group
// whose members differ in length (a stream: are fed different n, or that has ended and is fed) is refused: out_len 0xFFFFFFFF,
// min_gain NaN, n_limited 0xFFFFFFFF (a stream: 0), nonfinite 0, nothing else written.
constexpr uint32_t LIMIT_CHUNK = 4096;      // == GRAIL_LIMIT_CHUNK (not part of the contract: no number depends on it)
uint64_t limit_grid_chunks(uint64_t row_stride);
size_t limit_chunk_bytes();
struct LimitArgs : RowCallArgs {
    uint32_t n_groups, group;
    float ceiling;              // finite and > 0
    uint32_t ell;               // lookahead_log2, <= 10
    uint32_t grid_chunks;       // limit_grid_chunks(row_stride) a group; a stream's chunk kernel runs only when != 0
    float *out;                 // the limited rows (chunks past a group's last are left unwritten)
    uint64_t out_stride;
    void *cstat;                // the chunks' numbers, limit_chunk_bytes() each, at [group * grid_chunks + c]
    uint32_t *out_len, *n_limited, *nonfinite;  // [n_groups] each: a group's outputs of the call (streams only), its limited
    float *min_gain;                            // and its non-finite samples, its smallest gain
};
hipError_t launch_limit_frames(const LimitArgs &a, hipStream_t stream);
hipError_t launch_limit_totals(const LimitArgs &a, hipStream_t stream);             // one lane per group: the results from cstat
hipError_t launch_limit_stream(const LimitArgs &a, hipStream_t stream);
hipError_t launch_limit_stream_advance(const LimitArgs &a, hipStream_t stream);     // one wave per group: results, rings, state

// sample-rate conversion (resample_kernels.hip): one workgroup per (row, chunk of RESAMPLE_CHUNK outputs; a stream: of
// RESAMPLE_STREAM_CHUNK of the call's outputs), all rows on one pair of rates.  state: [n_rows][RESAMPLE_STREAM_STATE_WORDS] =
// {the state word, the input time floor(M D / U) of the row's next output M, the phase M D mod U}; ring: [n_rows][at or above P - 1].
constexpr uint32_t RESAMPLE_CHUNK = 1024;   // == GRAIL_RESAMPLE_CHUNK (not part of the contract: no number depends on it)
constexpr uint32_t RESAMPLE_STREAM_STATE_WORDS = 3;
uint64_t resample_grid_chunks(uint64_t row_stride, uint64_t out_stride, uint32_t U, uint32_t D);
struct ResampleArgs : RowCallArgs {
    uint32_t n_rows, up, down, taps;    // up, down, taps: grail_resample_ratio's U, D and P (the taps of one phase)
    const int32_t *table;       // [up][taps] numerators of 2^26 (grail_resample_coefficients)
    uint32_t grid_chunks;       // resample_grid_chunks(row_stride, out_stride, up, down) a row
    float *out;                 // the resampled rows (chunks past a row's last are left unwritten)
    uint64_t out_stride;
    uint32_t *cbad;             // the non-finite input samples a chunk owns, at [row * grid_chunks + c]
    uint32_t *out_len, *nonfinite;      // [n_rows]: min(ceil(n U / D), out_stride) (a stream: the call's outputs), and the count
};
hipError_t launch_resample(const ResampleArgs &a, hipStream_t stream);
hipError_t launch_resample_totals(const ResampleArgs &a, hipStream_t stream);           // one lane per row: the results from cbad
hipError_t launch_resample_stream(const ResampleArgs &a, hipStream_t stream);
hipError_t launch_resample_stream_advance(const ResampleArgs &a, hipStream_t stream);   // one wave per row: results, ring, state

// FIR filtering (fir_kernels.hip): one workgroup per (row, chunk of FIR_CHUNK outputs; a stream: of the call's outputs).  state:
// [n_rows], the state word; ring: [n_rows][at or above the set's longest n_taps - 1].  A row whose filter index is outside the
// set: 0xFFFFFFFF and 0, nothing of it written (a stream's indices were checked by the host).
constexpr uint32_t FIR_CHUNK = 2048;   // == GRAIL_FIR_CHUNK (not part of the contract: no number depends on it)
uint64_t fir_grid_chunks(uint64_t row_stride, uint64_t out_stride, uint32_t tail_max);
struct FirArgs : RowCallArgs {
    uint32_t n_rows;
    const uint32_t *filter;     // [n_rows] or NULL (filter 0 for every row)
    const double *taps;         // the set's image as binary64, every filter padded with +0.0 to a multiple of 8
    const uint32_t *desc;       // [n_filters][4] = {first tap, padded taps, taps, origin} (fir_plan.h)
    uint32_t n_filters;
    uint32_t grid_chunks;       // fir_grid_chunks(row_stride, out_stride, the set's longest tail) a row
    float *out;                 // the filtered rows (chunks past a row's last are left unwritten)
    uint64_t out_stride;
    uint32_t *cbad;             // the non-finite input samples a chunk owns, at [row * grid_chunks + c]
    uint32_t *out_len, *nonfinite;      // [n_rows]: min(n + K - 1 - o, out_stride) (a stream: the call's outputs), and the count
};
hipError_t launch_fir(const FirArgs &a, hipStream_t stream);
hipError_t launch_fir_totals(const FirArgs &a, hipStream_t stream);             // one lane per row: the results from cbad
hipError_t launch_fir_stream(const FirArgs &a, hipStream_t stream);
hipError_t launch_fir_stream_advance(const FirArgs &a, hipStream_t stream);     // one wave per row: results, ring, state

// meter streams (meter_stream_kernels.hip): rows metered call by call.  A call is three launches in this order: the hops (one
// lane per row; a feeding call only), the call's true peak (one wave per row and chunk of METER_STREAM_CHUNK output times), the
// advance (one wave per row: the call's results, the ring, N, the running peak, the hop count).  The first two read N and the
// hop count, only the third writes them.  state: [n_rows][METER_STREAM_STATE_WORDS] (word 0: the state word; 1 .. 5: s1 .. s4
// and acc as their bits; 6: the running true peak; 7: the hops completed); ring: [n_rows][METER_STREAM_RING].  A row that has
// ended and is fed, or that the call would carry past max_hops: 0xFFFFFFFF, NaN, 0, nothing else.
constexpr uint32_t METER_STREAM_STATE_WORDS = 8;
constexpr uint32_t METER_STREAM_RING = 16;
constexpr uint32_t METER_STREAM_CHUNK = 4096;
struct MeterStreamArgs : RowCallArgs {
    uint32_t n_rows, hop;
    const double *coef;         // HOST [10], the K-weighting
    double *ledger;             // [n_rows][max_hops]: every hop sum of a row so far
    uint64_t max_hops;
    double *hops_out;           // [n_rows][hops_stride] or NULL: the hop sums this call completes
    uint64_t hops_stride;
    uint32_t grid_chunks;       // chunks of output times a row
    double *cmax;               // a chunk's largest |y| and its non-finite count, each at [row * grid_chunks + c]
    uint32_t *cbad;
    uint32_t *n_hops, *nonfinite;       // [n_rows] each: the hops the call completed, its non-finite samples, its true peak
    double *true_peak;
};
hipError_t launch_meter_stream_hops(const MeterStreamArgs &a, hipStream_t stream);
hipError_t launch_meter_stream_peak(const MeterStreamArgs &a, hipStream_t stream);
hipError_t launch_meter_stream_advance(const MeterStreamArgs &a, hipStream_t stream);
// ... and what a meter shows of every row now, one lane per row (outputs may be NULL); changes nothing
hipError_t launch_meter_stream_read(const uint64_t *state, uint32_t n_rows, uint32_t hop, const double *ledger, uint64_t max_hops,
                                    double *integrated, double *momentary, double *short_term, double *true_peak, uint64_t *hops_out,
                                    hipStream_t stream);

// recursive filtering (iir_kernels.hip): one lane per row through the S sections of its filter, 64 rows to a wave, the
// filtered rows to out.  image: DEVICE [n_filters][40], section j of a filter at 5 j, +0.0 past its own; sections: DEVICE
// [n_filters], each filter's S; bound: 1, 2, 4 or 8, at or above every S of the set (iir_plan.h); filter: DEVICE [n_rows] or
// NULL (filter 0 for every row).  A row's n_out = min(n + tail, out_stride), 0 for n = 0; out_len, nonfinite: DEVICE
// [n_rows], may be NULL; a row whose filter index is outside the set: 0xFFFFFFFF and 0, nothing written.
// state != NULL: a call on a stream, the one kernel with the state read at entry and written at exit.  state: DEVICE
// [n_rows][1 + 2 * bound] = {the state word, then s1, s2 of each section as their bits}.  Feeding: n = min(len, row_stride) samples in, n out (tail is not read).  finishing: rows and len are not
// read, the rows with mark[u] != 0 (mark NULL: every row) that have not ended write tail outputs (none if fed nothing) and
// end; nonfinite is not written.  A row that has ended and is fed: 0xFFFFFFFF and 0, nothing else.
struct IirArgs {
    const float *rows;
    uint64_t row_stride;
    const uint32_t *len;
    uint32_t n_rows;
    const uint32_t *filter;
    const double *image;
    const uint32_t *sections;
    uint32_t n_filters;
    uint32_t tail;
    float *out;
    uint64_t out_stride;
    uint32_t *out_len;
    uint32_t *nonfinite;
    uint64_t *state;
    const uint8_t *mark;
    uint32_t finishing;
};
hipError_t launch_iir(const IirArgs &args, uint32_t bound, hipStream_t stream);

// recursive filtering parallel in time (biquad_block_kernels.hip; the contract is grail_hip.h's "recursive filtering, parallel
// in time"): a row's steps in blocks of IIR_BLOCK, one lane per (row, block), 64 consecutive blocks of a row
// to a workgroup of one wave, `groups` = iir_block_groups(grid_blocks) workgroups a row.  rows .. out_stride as in IirArgs;
// matrices: DEVICE [n_filters][16][16], iir_block_image's; state: DEVICE [n_rows][grid_blocks][2 * bound] doubles: slot k of a
// row holds z_k after the rest pass and e_{k+1} after the propagate; cbad: DEVICE [n_rows][groups], the non-finite samples
// the output pass's workgroups read.  Slots and counts past a row's own blocks are left as they were and read by nobody.
struct BiquadBlockArgs {
    const float *rows;
    uint64_t row_stride;
    const uint32_t *len;
    uint32_t n_rows;
    const uint32_t *filter;
    const double *image;
    const uint32_t *sections;
    const double *matrices;
    uint32_t n_filters;
    uint32_t tail;
    float *out;
    uint64_t out_stride;
    double *state;
    uint32_t *cbad;
    uint32_t grid_blocks;
    uint32_t groups;
};
// the rest pass (z_k of every block but a row's last), the propagate (one wave a row: the call's serial chain) and the output
// pass, in this order on one stream; n_rows * groups is at most 2^31 - 1
hipError_t launch_biquad_block_rest(const BiquadBlockArgs &args, uint32_t bound, hipStream_t stream);
hipError_t launch_biquad_block_propagate(const BiquadBlockArgs &args, uint32_t bound, hipStream_t stream);
hipError_t launch_biquad_block_output(const BiquadBlockArgs &args, uint32_t bound, hipStream_t stream);
// ... and a row's out_len and count from cbad, one lane per row (outputs may be NULL); a refused row: 0xFFFFFFFF and 0
hipError_t launch_biquad_block_totals(const BiquadBlockArgs &args, uint32_t *out_len, uint32_t *nonfinite, hipStream_t stream);

// dynamics (dyn_kernels.hip; the contract is grail_hip.h's "levels, continued: dynamics"): one lane per row
// through envelope, table and gain, 64 rows to a wave, the rows to out.  image: DEVICE [n_curves][641] pairs {G[k], G[k+1] -
// G[k]} (dyn_plan.h); alpha: DEVICE [n_curves][2]; detector: DEVICE [n_curves]; curve: DEVICE [n_rows] or NULL (curve 0).
// key != NULL: keyed, key [n_keys][key_stride] (n_keys >= 1), key_len: DEVICE [n_keys] or NULL (key_stride), key_row: DEVICE
// [n_rows] or NULL (row u to key u).  out_len, nonfinite, min_gain: DEVICE [n_rows], may be NULL; a row whose curve or key
// index is outside: 0xFFFFFFFF, 0 and NaN, nothing written.
// state != NULL: a call on a stream: state: DEVICE [n_rows][2] = {N, the bits of e}, read at entry and written at exit; n =
// min(len, row_stride) samples in, n out; a keyed row's key has the row's n samples (key_len is not read, key_row is the
// stream's and was checked when it was opened).
struct DynArgs {
    const float *rows;
    uint64_t row_stride;
    const uint32_t *len;
    uint32_t n_rows;
    const uint32_t *curve;
    const double *image;
    const double *alpha;
    const uint32_t *detector;
    uint32_t n_curves;
    const float *key;
    uint64_t key_stride;
    const uint32_t *key_len;
    uint32_t n_keys;
    const uint32_t *key_row;
    float *out;
    uint64_t out_stride;
    uint32_t *out_len;
    uint32_t *nonfinite;
    double *min_gain;
    uint64_t *state;
};
hipError_t launch_dyn(const DynArgs &args, hipStream_t stream);
// the same rows, the same bits, a workgroup a row (track_env_kernels.hip): for the few long tracks of a mix.
// state is not read (there is no stream form); more than 2^31 - 1 rows: hipErrorInvalidValue.
hipError_t launch_track_dyn(const DynArgs &args, hipStream_t stream);

// short-time spectra (spectrum_kernels.hip; the contract is grail_spectrum.h's "levels, continued: short-time spectra", DESIGN.md
// §4.25): one workgroup per (row, chunk of SPECTRUM_CHUNK_FRAMES frames), grid_chunks = spectrum_grid_chunks(row_stride, hop)
// of them a row (spectrum_plan.h).  log2n .. n_bands: the set's facts; window: DEVICE [n_window]; twiddles: DEVICE [N/2]
// pairs (re, im); band_desc: DEVICE [n_bands][4] = {first bin, count, first weight, 0}; band_weights: DEVICE, the bands'
// weights one after another.  power: [n_rows][frames_stride][N/2 + 1] or NULL; bands: [n_rows][frames_stride][n_bands] or NULL;
// frames past a row's last are left unwritten.  cbad: the non-finite samples a chunk owns (those of its frames' hops), at
// [row * grid_chunks + c], or NULL when nobody asks for the count (chunks past a row's last are left unwritten).
struct SpectrumArgs {
    const float *rows;
    uint64_t row_stride;
    const uint32_t *len;
    uint32_t n_rows;
    uint32_t log2n, n_window, hop, pad, n_bands;
    const float *window;
    const double *twiddles;
    const uint32_t *band_desc;
    const float *band_weights;
    float *power;
    float *bands;
    uint64_t frames_stride;
    uint32_t grid_chunks;
    uint32_t *cbad;
    uint32_t *n_frames;
    uint32_t *nonfinite;
};
// n_rows * grid_chunks is at most 2^31 - 1 (the host has checked)
hipError_t launch_spectrum(const SpectrumArgs &args, hipStream_t stream);
// ... and a row's n_frames and count from cbad, one lane per row (outputs may be NULL)
hipError_t launch_spectrum_totals(const SpectrumArgs &args, hipStream_t stream);

}  // namespace grail
