/*
 * grail_hip.h — C ABI of the MI355X-native (gfx950) batched implementation of
 * the grail-rs per-sample synthesis hot path.
 *
 * What it replaces.  grail-rs has no FFI layer; its boundary for this path is
 * the iterator-adapter API (reference = /root/reference):
 *
 *     phoneme_elems.into_iter()
 *         .select(voice)          // src/lib.rs:1013  Selector::next   :990
 *         .sequence(voice)        // src/lib.rs:941   Sequencer::next  :859
 *         .jitter(seed, voice)    // src/lib.rs:786   Jitter::next     :753
 *         .synthesize()           // src/lib.rs:587   Synthesize::next :497
 *         .collect::<Vec<f32>>()
 *
 * grail_synthesize_batch() is that expression evaluated for N independent
 * utterances at once on one GPU; every entry point below cites the reference
 * item it stands for.  INTEGRATION.md shows the Rust `extern "C"` block and
 * the IntoSynthesizeBatch trait shim a maintainer would add.
 *
 * Types are plain-old-data with the reference's declared field order; no
 * torch / HIP types appear in any signature (device memory is `void *`).
 *
 * Determinism contract: the samples of utterance u are a pure
 * function of (its segments, its voice, its jitter seed) — independent of the
 * batch size, its position in the batch, the lane mapping and the GPU count —
 * and are bit-identical to the reference's IEEE-754 binary32 arithmetic
 * (no FMA contraction, correctly rounded division, denormals kept).  That is the
 * default, "arithmetic" = 0.  With grail_set_option(ctx, "arithmetic", 1) the
 * samples are within GRAIL_FAST_TOLERANCE x max(1, the utterance's largest
 * |sample|) of those bits instead (lengths, segment boundaries, noise wraps and
 * saw edges still exactly the reference's).  Two tolerance tiers serve it, chosen from
 * the sharpness of the resonances of the voices a batch uses (grail_fast_sharpness):
 * up to GRAIL_FAST_SHARPNESS_LIMIT the filter coefficients are interpolated across
 * sub-tiles (2.6x the exact mode on the headline batch); sharper voices get the
 * reference's own band-pass coefficients at every sample and fast arithmetic for
 * the rest (1.25x - 1.55x; at most 17.3 * 2^-23 off on 1000 random voice tables of
 * any sharpness, profiles/r04_middle_tier.txt); beyond
 * GRAIL_FAST_SHARPNESS_LIMIT_EXACT_COEFFICIENTS, and wherever an exact kernel is the
 * faster way to render a block, the exact bits (they satisfy any tolerance).
 * Fast-mode samples are a pure function of (the utterance, the kernel family):
 * every lane decides from its own state, so they do not depend on the batch size,
 * the position in the batch or the other utterances of the batch AS LONG AS THE
 * KERNEL FAMILY IS THE SAME.  The family is what the host picks for the BLOCK of rows
 * an utterance is rendered in: a batch is cut into blocks by size (grail_plan_blocks
 * predicts the cut: whole rounds of the one-lane kernels, then the rest on whatever
 * suits its size) and each block takes the time-parallel scan kernel (few rows),
 * the time-split kernels (their chunk grid follows the block's size and the batch's
 * longest utterance; "time_split_chunks" / "time_split_span_samples" pin it) or the
 * lane kernels ("lanes_per_utterance" pins the mapping; a pinned option also keeps
 * the batch in ONE block).  The host-output calls render a batch in blocks of up to
 * 4096 rows (2 GB) and choose the family for that block size, the short last block
 * included: there the "batch size" is min(n_utt, 4096).
 * A caller that needs the reference's contract in fast mode too — an utterance's
 * samples a pure function of (segments, voice, seed), whatever batch it is part of —
 * pins ONE family: "lanes_per_utterance" = 1 renders every batch size with the fast
 * one-lane kernels (batch-invariant by construction; it gives up the time-split and
 * scan kernels' speed on batches that do not fill the machine).
 *
 * There is no CPU fallback: every compute entry point fails with
 * GRAIL_ERR_NO_DEVICE when no HIP device is usable, and grail_create() refuses a
 * device whose architecture is not gfx950 (the library holds gfx950 code objects
 * only).  The launch policy is derived from the device: every capacity is a multiple
 * of hipDeviceProp_t::multiProcessorCount (256 on a whole MI355X, 32 on a CPX
 * partition), every crossover follows the utterances' length
 * (profiles/r04_duration_sweep.txt).
 */
#ifndef GRAIL_HIP_H
#define GRAIL_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Bumped whenever an entry point, an option name or the meaning of an option changes; a binding compares it with
 * grail_abi_version() of the library it loaded BEFORE its first call (the Python and Rust bindings do).
 *   1: rounds 1-2.   2: round 3-4 — grail_device_pci_bus_id, grail_time_split_warmup / _grid, grail_fast_sharpness,
 *   grail_plan_blocks, grail_stream_open_live / _append / _append_elems / _finish / _pending; option "kernel_variant" removed, "scan_debug" in
 *   development builds only; "arithmetic" = 1 is served up to a sharpness of the voice table.
 *   3: round 5 — grail_length_bound; options "two_waves_per_simd", "pipeline_spread", "pipeline_round32" = 2; "ragged_plan" also weighs the scan and
 *   time-split kernels by the rows.
 *   4: round 6 — grail_node_* (one call, every GPU of the node); option "packed_launch_order".  Additions since, which
 *   change nothing that was there: grail_mix_async, grail_batch_mix, grail_mix_place_sequential,
 *   grail_pcm16_frames_async, grail_wav_write_i16_frames. */
#define GRAIL_ABI_VERSION 4
/* fast mode ("arithmetic" = 1): bound on |fast - exact| per sample, full scale = 1.0; k * 2^-23 */
#define GRAIL_FAST_TOLERANCE_ULPS 64
#define GRAIL_FAST_TOLERANCE (GRAIL_FAST_TOLERANCE_ULPS * 1.1920928955078125e-07f)
/* fast mode is served for voices whose grail_fast_sharpness() is at most this (predicted deviation, units of 2^-23) */
#define GRAIL_FAST_SHARPNESS_LIMIT 28.0
/* sharper voices get the second tolerance tier — the reference's own band-pass coefficients at every sample, fast
 * arithmetic elsewhere: at most 17.3 * 2^-23 from the reference on 1000 random voice tables of any sharpness on the
 * device, 16.3 in the CPU experiment over 3000 (profiles/r04_middle_tier.txt) — up to this sharpness; beyond it the exact
 * kernels */
#define GRAIL_FAST_SHARPNESS_LIMIT_EXACT_COEFFICIENTS 1024.0

/* src/lib.rs:24  NUM_FORMANTS, src/lib.rs:21 DEFAULT_SAMPLE_RATE */
#define GRAIL_NUM_FORMANTS 8
#define GRAIL_DEFAULT_SAMPLE_RATE 44100.0f

/* Phoneme: src/lib.rs:632-649 with make_phonemes!(A a test, E e test) :686-689.
 * Discriminants follow the declaration order of the Rust enum. */
typedef enum grail_phoneme {
    GRAIL_PH_SILENCE = 0, /* src/lib.rs:635 */
    GRAIL_PH_STOP    = 1, /* src/lib.rs:640 */
    GRAIL_PH_GLIDE   = 2, /* src/lib.rs:643 */
    GRAIL_PH_A       = 3,
    GRAIL_PH_E       = 4,
    GRAIL_PH_COUNT   = 5
} grail_phoneme;
/* number of VoiceStorage fields (src/lib.rs:653-659): a, e */
#define GRAIL_NUM_VOICED 2
#define GRAIL_PH_FIRST_VOICED GRAIL_PH_A

typedef enum grail_status {
    GRAIL_OK                   = 0,
    GRAIL_ERR_INVALID_ARG      = -1,
    GRAIL_ERR_NO_DEVICE        = -2, /* no usable HIP device: there is NO CPU fallback */
    GRAIL_ERR_HIP              = -3, /* a hip* call failed; see grail_last_error() */
    GRAIL_ERR_BUFFER_TOO_SMALL = -4, /* >=1 utterance did not end within out_stride samples */
    GRAIL_ERR_OUT_OF_MEMORY    = -5,
    GRAIL_ERR_RCCL             = -6,
    GRAIL_ERR_NO_VOICES        = -7  /* grail_set_voices() has not been called */
} grail_status;

/* SynthesisElem: src/lib.rs:316-337, 49 x f32 in declared order.
 * `Array` (src/lib.rs:88) is float[8]. */
typedef struct grail_synthesis_elem {
    float frequency;
    float formant_freq[GRAIL_NUM_FORMANTS];
    float formant_bw[GRAIL_NUM_FORMANTS];
    float formant_smooth[GRAIL_NUM_FORMANTS];
    float formant_breath[GRAIL_NUM_FORMANTS];
    float formant_turb[GRAIL_NUM_FORMANTS];
    float formant_amp[GRAIL_NUM_FORMANTS];
} grail_synthesis_elem;

/* Voice: src/lib.rs:696-717; `phonemes` is VoiceStorage {a, e} (src/lib.rs:653-659). */
typedef struct grail_voice {
    float                sample_rate;
    grail_synthesis_elem phonemes[GRAIL_NUM_VOICED];
    float                center_frequency;
    float                jitter_frequency;
    float                jitter_delta_frequency;
    float                jitter_delta_formant_frequency;
    float                jitter_delta_amplitude;
} grail_voice;

/* PhonemeElem: src/lib.rs:961-973 (the Selector's input item). */
typedef struct grail_phoneme_elem {
    int32_t phoneme;      /* grail_phoneme */
    float   length;       /* seconds */
    float   blend_length; /* seconds */
    float   frequency;    /* normalised to the sample rate */
} grail_phoneme_elem;

/* SequenceElem: src/lib.rs:814-824 (the Sequencer's input item);
 * Option<SynthesisElem> is (has_elem, elem). */
typedef struct grail_sequence_elem {
    int32_t              has_elem;
    grail_synthesis_elem elem;
    float                length;
    float                blend_length;
} grail_sequence_elem;

typedef struct grail_ctx   grail_ctx;   /* one per (process, GPU); owns a HIP stream */
typedef struct grail_batch grail_batch; /* inputs of one batch, resident in HBM */
typedef struct grail_stream grail_stream; /* resumable synthesis of one batch */
typedef struct grail_node  grail_node;  /* one process, several GPUs: a grail_ctx and a host thread per GPU */

/* flags of grail_synthesize_batch*() */
#define GRAIL_OUT_HOST   0u /* `out` is host memory (pageable or pinned) */
#define GRAIL_OUT_DEVICE 1u /* `out` is device memory of ctx's GPU; no copy is made */

/* ---- library ----------------------------------------------------------- */
int         grail_abi_version(void);
const char *grail_status_string(int status);
/* text of the last failure on this thread ("" if none) */
const char *grail_last_error(void);

/* ---- host-side parameter algebra (per voice / per phoneme, once) ------- */
/* SynthesisElem::silent()  src/lib.rs:367-377 */
void grail_elem_silent(grail_synthesis_elem *out);
/* SynthesisElem::new_phoneme(freq, bw, smooth, turb, breath, amp)  src/lib.rs:381-401
 * (== voices::MKPHON, src/voices/mod.rs:7-14); each argument is float[8]. */
void grail_elem_new_phoneme(grail_synthesis_elem *out, const float *formant_freq,
                            const float *formant_bw, const float *formant_smooth,
                            const float *formant_turb, const float *formant_breath,
                            const float *formant_amp);
/* SynthesisElem::new(sample_rate, frequency, freq, smooth, bw, breath, turb, amp)
 * src/lib.rs:343-364 — note the argument order differs from new_phoneme. */
void grail_elem_new(grail_synthesis_elem *out, float sample_rate, float frequency,
                    const float *formant_freq, const float *formant_smooth,
                    const float *formant_bw, const float *formant_breath,
                    const float *formant_turb, const float *formant_amp);
/* SynthesisElem::resample(old, new) in place  src/lib.rs:418-440 */
void grail_elem_resample(grail_synthesis_elem *elem, float old_sample_rate,
                         float new_sample_rate);
/* SynthesisElem::blend(self, other, alpha)  src/lib.rs:404-414 */
void grail_elem_blend(grail_synthesis_elem *out, const grail_synthesis_elem *self,
                      const grail_synthesis_elem *other, float alpha);
/* voices::generic()  src/voices/generic.rs:5-40 */
void grail_voice_generic(grail_voice *out);
/* generic() carried to another sample rate (the reference ships 44.1 kHz only):
 * every phoneme .resample(44100, rate) (src/lib.rs:418 through for_all :674),
 * sample_rate = rate, scalars 120/rate, 16/rate, 6/rate, 6/rate, 0.2
 * (cf. src/voices/generic.rs:34-38).  SURVEY.md §8d "48 kHz voice". */
void grail_voice_generic_at(grail_voice *out, float sample_rate);
/* VoiceStorage::get(phoneme)  src/lib.rs:664-671; returns 1 and fills *out for a
 * voiced phoneme, 0 for Silence/Stop/Glide (None). */
int grail_voice_get(const grail_voice *voice, int32_t phoneme, grail_synthesis_elem *out);

/* ---- context ----------------------------------------------------------- */
/* Binds to HIP device `device` (>= 0) and creates a stream.
 * GRAIL_ERR_NO_DEVICE when HIP reports no such device or its architecture is not gfx950. */
int grail_create(int device, grail_ctx **out);
int grail_destroy(grail_ctx *ctx);
int grail_device_count(int *count);
/* hipDeviceGetPCIBusId of ctx's GPU ("0000:05:00.0", NUL-terminated; cap >= 16).  Lets a launcher prove
 * that its ranks sit on distinct GPUs. */
int grail_device_pci_bus_id(grail_ctx *ctx, char *out, size_t cap);
/* Uploads the voice table (the `voice` argument of .select/.sequence/.jitter,
 * src/lib.rs:1013, 941, 786) to HBM.  Utterances refer to it by voice id. */
int grail_set_voices(grail_ctx *ctx, const grail_voice *voices, uint32_t n_voices);
int grail_get_voices(grail_ctx *ctx, grail_voice *voices, uint32_t cap, uint32_t *n_voices);
/* Options (grail_set_option / grail_get_option; int64 values).  What each one may change: "bits: fast" = the samples of a
 * tolerance-mode rendering, within GRAIL_FAST_TOLERANCE; every other option changes time only.  With "arithmetic" = 0 no
 * option ever changes a result bit.  What each is worth on an MI355X is measured in DESIGN.md section 4, not here.
 *   "arithmetic"            0 (default) exact: every sample the reference's binary32 bits.  1 fast: the tolerance mode —
 *                           |fast - reference| <= GRAIL_FAST_TOLERANCE per sample, identical lengths, the discontinuous
 *                           state (Sequencer clock, jitter phase, carrier phase, both LCGs) exact; served by the tier the
 *                           voices' sharpness allows (below).  2: the second tier whatever the voices.  THE option that
 *                           changes result bits.
 *   "fast_sharpness_limit"  (default GRAIL_FAST_SHARPNESS_LIMIT) first tier (filter coefficients interpolated) for batches
 *                           whose voices / elems have a grail_fast_sharpness() of at most this.  bits: fast.
 *   "fast_exact_coefficients" 1 (default) / 0: sharper batches, up to "fast_sharpness_limit_exact_coefficients" (default
 *                           GRAIL_FAST_SHARPNESS_LIMIT_EXACT_COEFFICIENTS), get the second tier (the reference's own band-pass
 *                           coefficients at every sample); 0 or beyond: the exact kernels.  bits: fast.
 *   "lanes_per_utterance"   0 (default) auto, or 1 / 2 / 4 / 8: wavefront lanes that share an utterance's formants; pins the
 *                           lane kernels (no pipelined workgroups, no composite cut).  bits: fast (the kernel family).
 *   "skip_silent_formants"  1 (default) / 0: formants that provably contribute exactly +0.0 (amplitude 0 in both elems of a
 *                           segment pair, band-pass state 0) are skipped, and not laid out at all where the voice table and
 *                           the batch guarantee it for formants 5-8; 0: all eight evaluated literally.
 *   "small_batch_pipeline"  1 (default) / 0: small exact blocks run four-wave pipelined workgroups; streams of that size too.
 *   "pipeline_round32"      1 (default) / 0 / 2: ... in rounds of 32 samples while one workgroup per compute unit suffices and
 *                           the rows are of one length / never / whatever the rows (rounds of 16 otherwise).
 *   "pipeline_spread"       1 (default) / 0: ... of rows that differ in length hold as few utterances each as give every compute
 *                           unit two workgroups (a tile with an event of one utterance costs the whole workgroup).
 *   "pipeline4_max_groups", "pipeline8_max_groups"  (default -1: two per compute unit) workgroups a block may need to take them.
 *   "time_parallel_scan"    1 (default) / 0: fast, first tier: few utterances run one workgroup each, lanes = time (parallel
 *                           scans).  "time_parallel_scan_max_utterances" (-1 auto): hard upper limit;
 *                           "time_parallel_scan_split_max_utterances" (-1 auto): up to here the three-stage flavour.  bits: fast.
 *   "time_split"            1 (default) / 0: fast, both tiers: up to half a device's lanes' worth of utterances are cut along
 *                           their time axis, one lane per chunk (filters warmed up from zero: grail_time_split_warmup).
 *                           "time_split_min_utterances" (-1 auto), "time_split_chunks" (0 auto, 2..64) and
 *                           "time_split_span_samples" (0: the longest utterance) pin the grid (grail_time_split_grid);
 *                           "time_split_ff_cost_permille" (default 165): a fast-forwarded sample against a rendered one.  bits: fast.
 *   "composite_launches"    1 (default) / 0: a batch is cut into blocks with a kernel family each (grail_plan_blocks); 0: one
 *                           launch per call.  bits: fast (a row follows its block's family).
 *   "row_groups"            1 (default) / 0 / 2: rows the lean kernel families cannot take (a segment shorter than two samples,
 *                           a non-finite length, blend length or pitch) are planned apart where cheaper / never / always.
 *   "ragged_plan"           1 (default) / 0: batches whose utterances differ in length are planned by the rows' lengths and
 *                           events (grail_plan_ragged_blocks): one launch of each lane mapping in several rounds, and in fast
 *                           arithmetic the scan and time-split kernels, are weighed against the cut by size; a fast request may
 *                           be served by an exact mapping where that is cheaper ("last_launch_fast").  bits: fast.
 *   "two_waves_per_simd"    1 (default) / 0: launches of the 2 / 4 / 8-lane kernels with more wavefronts than the device has
 *                           SIMDs take instantiations built for two wavefronts per SIMD (same operations, same bits).
 *   "packed_launch_order"   1 (default) / 0: a launch of more one-wave-per-SIMD workgroups than the device holds at once, of rows
 *                           that differ in length, takes its workgroups in a packed order (the SIMDs end together) instead of
 *                           longest first.
 *   "sort_by_length"        1 (default) / 0: batches uploaded afterwards fill the launch slots longest first (rows stay put).
 *   "assume_compute_units"  0 (default: the device's own) or a count to plan for: tests, callers that share a device.
 *   "scan_debug"            development builds only.
 * Read-only (grail_get_option): "compute_units"; "fast_arithmetic_served" (what "arithmetic" = 1 gets for the voice table as
 *   a whole: 1 / 2 / 0 exact kernels); of the last launch (its largest block): "last_launch_fast" (tier that ran, 0 exact),
 *   "last_launch_blocks", "last_launch_formants" (4 / 8), "last_launch_lanes", "last_launch_pipelined", "last_launch_chunks",
 *   "last_launch_packed" (blocks launched in packed order);
 *   statistics: "slow_division_wave_steps" (summed over the waves: the most steps any one lane of a wave took with a segment
 *   pair outside the window of the short division; 0: every division of every lane took it), "fast_wave_tiles" (tiles
 *   rendered without a slow sample), "general_wave_steps" (tolerance mode: slow samples; exact: general steps). */
int grail_set_option(grail_ctx *ctx, const char *name, int64_t value);
int grail_get_option(grail_ctx *ctx, const char *name, int64_t *value);
/* The planning behind "time_split", as pure host functions (no GPU, no context): what a caller needs to
 * predict or pin a fast-mode kernel family, and what the CPU tests check.
 * grail_time_split_warmup: the warm-up length of `voice` in samples, a multiple of 64 — after so many samples a
 *   filter state started from zero is within 2^-21 of the one Synthesize::next (src/lib.rs:530-575) would hold,
 *   from the slowest one-pole / band-pass decay over the voice's phonemes with a 5 % margin.  0: the voice does
 *   not qualify (a formant parameter outside (0, 0.5) / (0, 1), or more than 16384 samples).
 * grail_time_split_grid: bounds[0 .. chunks) of `chunks` chunks (2..64) over span_samples, multiples of 64 with
 *   bounds[0] = 0, spaced so that fast-forwarding (ff_cost_permille per sample, a rendered sample = 1000),
 *   warming up and rendering take every chunk's lane the same time.  GRAIL_ERR_INVALID_ARG when so many chunks
 *   do not fit (a chunk would render fewer than 64 samples). */
uint32_t grail_time_split_warmup(const grail_voice *voice);
/* An upper bound of an utterance's length in samples (pure host arithmetic): the lengths of its segments in seconds and the
 * sample rate of its voice.  Sequencer::next (src/lib.rs:859-888) adds every segment's length to an f32 clock and takes
 * 1 / sample_rate off it per sample, so a segment lasts length * sample_rate samples only up to the clock's rounding: a step
 * lowers it by at least dt - ulp(length) / 2, and the bound is the sum of length / (dt - ulp(length) / 2) + 2 over the
 * segments (a segment of 16 s at 192 kHz may last 22 % longer than its nominal length — in the reference too).  For sizing
 * out_stride without the device pre-pass (grail_batch_lengths gives the exact lengths); the time-split kernels use it to
 * skip the chunks an utterance does not reach.  UINT64_MAX: no bound (a length that is not finite, a clock that may not
 * move: dt <= ulp(length)). */
uint64_t grail_length_bound(const float *segment_lengths, uint32_t n_segments, float sample_rate);
/* The sharpness of a voice's resonances as the fast kernels see it: the predicted |fast - reference| in units of
 * 2^-23 of max(1, peak).  Per formant E_i = share_i * (0.0709 / bw_i) * (1 + (f_i / 0.075)^2) — share = the
 * formant's part of the phoneme's amplitudes, f and bw in cycles per sample, each the worst of the voice's
 * phonemes — and S = sqrt(sum_i E_i^2) (voices::generic(): 24, measured 13 - 20).  A rounding-level difference of a
 * filter coefficient (src/lib.rs:555-562) is amplified by the quality and the ring time of the band-pass, in the
 * reference's own arithmetic as well; the formula is a fit to measurements (profiles/r03_sharpness.txt).
 * The interpolating tier of fast arithmetic is served up to GRAIL_FAST_SHARPNESS_LIMIT; sharper voices (and
 * caller-built elems, judged the same way at upload: every two consecutive elems of an utterance like a voice of two
 * phonemes, the worst pair of the batch counts) get the tier that evaluates the reference's own coefficients, or the
 * exact kernels — read-only options "fast_arithmetic_served" / "last_launch_fast" tell.  A batch is judged by the
 * voices it names, not by the whole table.  +inf: a formant outside (0, 0.5) or a bandwidth <= 0. */
float grail_fast_sharpness(const grail_voice *voice);
int grail_time_split_grid(uint32_t span_samples, uint32_t warmup, uint32_t chunks, uint32_t ff_cost_permille,
                          uint32_t *bounds);
/* The launch plan, as a pure host function (no GPU, no context).  A kernel family fills the machine with a fixed
 * number of utterances (one wavefront per SIMD: 16 / 32 per compute unit for the pipelined workgroups, 256 / L for L
 * lanes per utterance), and one utterance more costs it a whole further round.  A batch is therefore cut into BLOCKS,
 * each rendered by the family that suits the block's size: whole rounds of the one-lane kernels first, the rest with
 * wider mappings (65537 utterances: 65536 on one lane each + 1 on a pipelined workgroup).  The
 * cut minimises a cost model calibrated on the device (profiles/r04_duration_sweep.txt) that follows the compute-unit
 * count and the utterances' length.  Exact arithmetic is mapping-invariant: the cut never changes a bit.  In fast
 * arithmetic a row's samples follow the family of ITS block, which this function predicts: rows keep batch order
 * (length-sorted batches: slot order), block i covers the next blocks[i].rows of them.
 *   compute_units: hipDeviceProp_t::multiProcessorCount (256 for a whole MI355X; option "compute_units" tells)
 *   arithmetic: 0 exact / 1 fast (voices the interpolating tier is served for) / 2 fast with the reference's own
 *     coefficients (sharper voices);  live_formants: 4 (formants 5-8 silent in every phoneme, as voices::generic()) or 8
 *   warmup: grail_time_split_warmup() of the voice table's slowest voice (0: no time-split kernels)
 *   rows, span_samples: the batch size and its longest utterance
 * *n_blocks receives the number of blocks even when it exceeds cap. */
typedef struct grail_plan_block {
    uint32_t rows;
    uint32_t lanes_per_utterance; /* lane kernels and pipelined workgroups: 1 / 2 / 4 / 8; scan kernel: 0 */
    uint32_t pipelined;           /* exact pipelined workgroups: 1 rounds of 16 samples, 2 rounds of 32; else 0 */
    uint32_t chunks;              /* time-split kernels: chunks per utterance; else 0 */
    uint32_t scan;                /* scan kernel: 1 two-stage, 2 three-stage workgroups; else 0 */
    uint32_t fast;                /* the block runs tolerance arithmetic */
    uint32_t formants;            /* formants laid out: 4 or 8 */
    float    model_ms;            /* the cost model's estimate for the block */
} grail_plan_block;
int grail_plan_blocks(uint32_t compute_units, int arithmetic, int live_formants, uint32_t warmup, uint32_t rows,
                      uint32_t span_samples, grail_plan_block *blocks, uint32_t cap, uint32_t *n_blocks);
/* ... of a batch whose utterances differ in length (option "ragged_plan"), rows in launch order = longest first:
 *   row_samples[rows]: the utterances' lengths in samples, descending
 *   row_segments[rows], row_kinks[rows]: their segments, and those among them with blend_length < length (the kink of
 *     alpha = min(clk / blend_length, 1), an event of its own in fast arithmetic); NULL: none
 * model_ms is then the estimate for the block's own rows. */
int grail_plan_ragged_blocks(uint32_t compute_units, int arithmetic, int live_formants, uint32_t warmup, uint32_t rows,
                             const uint32_t *row_samples, const uint32_t *row_segments, const uint32_t *row_kinks,
                             grail_plan_block *blocks, uint32_t cap, uint32_t *n_blocks);
/* The workgroup dispatcher as the library models it, and the packed launch order, as pure host functions (no GPU).  A launch
 * of workgroups that each hold their SIMDs alone (the one-wave-per-SIMD kernel families), n of them, more than the device
 * holds at once: workgroup b runs on XCC b mod 8; the k-th workgroup of an XCC goes to shader engine k mod 4 of it, whatever
 * the engines' load; it starts when that engine has room AND every earlier workgroup of the XCC has started (measured:
 * tools/dispatch_order.hip, profiles/r06_dispatch_order.txt — the model gives the makespan of recorded launches to the
 * microsecond).  waves_per_workgroup: 1 (a SIMD each: 32 per engine) or 4 (a compute unit each: 8 per engine);
 * compute_units that are not whole XCCs of 32: one pool.
 * grail_dispatch_model: the makespan of workgroups that take workgroup_ms[b], launched in `order` (order[position] =
 *   workgroup; NULL: 0, 1, 2 ...).
 * grail_packed_launch_order: the order option "packed_launch_order" launches them in — dealt to the pools by cost, each pool
 *   packed into its SIMDs (best-fit decreasing under the smallest capacity that fits), launched by planned start time — so
 *   that the SIMDs end together where "longest first" leaves them uneven (two or three workgroups per SIMD: up to 15 %). */
int grail_dispatch_model(uint32_t compute_units, uint32_t waves_per_workgroup, const double *workgroup_ms,
                         const uint32_t *order, uint32_t n, double *makespan_ms);
int grail_packed_launch_order(uint32_t compute_units, uint32_t waves_per_workgroup, const double *workgroup_ms, uint32_t n,
                              uint32_t *order);

/* ---- batches ----------------------------------------------------------- */
/* Uploads the inputs of n_utt utterances: utterance u is
 *   segs[seg_offsets[u] .. seg_offsets[u+1]).into_iter()
 *       .select(v).sequence(v).jitter(jitter_seeds[u], v).synthesize()
 * with v = voices[voice_ids[u]].  voice_ids == NULL means voice 0 for all,
 * jitter_seeds == NULL means seed 0 for all (examples/cli.rs:182). */
int grail_batch_upload(grail_ctx *ctx, const grail_phoneme_elem *segs,
                       const uint32_t *seg_offsets, const uint32_t *voice_ids,
                       const uint32_t *jitter_seeds, uint32_t n_utt, grail_batch **out);
/* Same, for callers that build SequenceElems themselves (skips the Selector):
 *   segs[..].into_iter().sequence(v).jitter(seed, v).synthesize() */
int grail_batch_upload_elems(grail_ctx *ctx, const grail_sequence_elem *segs,
                             const uint32_t *seg_offsets, const uint32_t *voice_ids,
                             const uint32_t *jitter_seeds, uint32_t n_utt,
                             grail_batch **out);
int grail_batch_free(grail_ctx *ctx, grail_batch *batch);
uint32_t grail_batch_size(const grail_batch *batch);

/* Sequencer clock pre-pass (src/lib.rs:861-888 only): the number of samples
 * each utterance yields, capped at max_len.  out_len is host memory [n_utt]. */
int grail_batch_lengths(grail_ctx *ctx, const grail_batch *batch, uint32_t max_len,
                        uint32_t *out_len);

/* Enqueue the fused Sequencer->Jitter->Synthesize kernel on ctx's stream.
 * out_dev: device memory, utterance u written at out_dev + u*out_stride,
 * samples past its end are left untouched.  out_len_dev: device memory [n_utt]
 * (samples written, <= out_stride) or NULL.  Returns without waiting.
 * Any out_stride >= the longest utterance works (grail_batch_lengths tells).  Rows that start 16-byte aligned — out_dev
 * from grail_device_alloc and out_stride a multiple of 4 samples — are written with 16-byte stores, and a multiple of 64
 * makes every 64-sample tile one aligned 256-byte run; an odd stride takes 4-byte stores in runs of 16 samples: + 2 - 4 %
 * (exact) / + 7 - 8 % (fast) on the headline batch (96006 instead of 96064 samples per row; with all eight formants
 * live on one lane the general flush: + 7 % / + 14 %). */
int grail_batch_synthesize_async(grail_ctx *ctx, const grail_batch *batch, float *out_dev,
                                 uint64_t out_stride, uint32_t *out_len_dev);
/* Wait for ctx's stream.  Returns GRAIL_ERR_BUFFER_TOO_SMALL if any utterance
 * of a kernel enqueued since the last sync was cut at out_stride. */
int grail_sync(grail_ctx *ctx);
/* HIP-event time (ms) of the most recent synthesis kernel on ctx's stream
 * (events recorded on the stream the kernel is launched on).  Syncs. */
int grail_last_kernel_ms(grail_ctx *ctx, float *ms);
/* Which kernel instantiation the most recent synthesis launch of ctx started, e.g.
 * "synth_kernel<L=1,T=32,W=1,1,NFA=4>" (profiling bookkeeping: counters measured on one
 * instantiation are never reported for another).  Owned by ctx; valid until its next launch. */
const char *grail_last_kernel_name(grail_ctx *ctx);

/* Resumable synthesis (the lazy-iterator use of the chain, examples/interactive.rs:31-48):
 * the per-utterance iterator state (Sequencer :839-854, Jitter :724-748, Synthesize :470-488)
 * lives in HBM between launches.  Each call renders the NEXT max_samples (<= out_stride)
 * samples of every utterance to out_dev + u*out_stride (from index 0) and the count to
 * out_len_dev[u] (0 once the utterance has ended).  Concatenating the chunks gives exactly the
 * one-shot result, whatever the chunk sizes ("arithmetic" = 0; in fast mode the chunks follow the
 * exact state to the bit — same lengths, same boundaries — and the samples agree with the one-shot
 * rendering within the fast-mode tolerance).  The batch must outlive the stream. */
int grail_stream_open(grail_ctx *ctx, const grail_batch *batch, grail_stream **out);
int grail_stream_next_async(grail_ctx *ctx, grail_stream *stream, uint32_t max_samples,
                            float *out_dev, uint64_t out_stride, uint32_t *out_len_dev);
/* The same chunk as i16 PCM (the WAV sink's conversion, examples/cli.rs:49, fused into the store):
 * what a sound-card callback wants.  f32 and i16 calls may be mixed on one stream. */
int grail_stream_next_pcm16_async(grail_ctx *ctx, grail_stream *stream, uint32_t max_samples,
                                  int16_t *out_dev, uint64_t out_stride, uint32_t *out_len_dev);
int grail_stream_close(grail_ctx *ctx, grail_stream *stream);
/* LIVE streams — the lazy source of examples/interactive.rs:31-48.  There ONE chain runs for the whole session and its
 * source never ends: text arrives while the audio callback is pulling samples, Sequencer::next fetches the next
 * SequenceElem only when a segment runs out (src/lib.rs:866-888), and carrier phase, noise seed, jitter and filter
 * state carry across everything that is ever said.  A live stream is that: it is opened EMPTY for n_utt utterances
 * (each one chain: voice_ids / jitter_seeds as in grail_batch_upload, NULL = voice 0 / seed 0), segments are appended
 * while it runs, and samples are pulled with grail_stream_next_async / _pcm16_async as from any stream.
 *   grail_stream_append: utterance u receives segs[seg_offsets[u] .. seg_offsets[u + 1]) behind what it already has
 *     (seg_offsets as in grail_batch_upload: n_utt + 1 non-decreasing entries; an empty range appends nothing).
 *   grail_stream_append_elems: the same for streams opened with caller_built_elems != 0 (SequenceElems, no Selector).
 *     Both return when the segments are queued on the context's stream, behind the launches before the call and ahead of
 *     those after it (the caller's arrays have been copied and may be reused at once); a failure of the queued work
 *     surfaces at the next grail_sync, like a kernel's.
 *   A Sequencer that needs a segment which has not been appended yet PAUSES: the call returns fewer than max_samples
 *     for that row (possibly 0) and the next call after an append carries on from exactly the same state — so the
 *     samples are those of the one-shot rendering of everything appended, bit for bit ("arithmetic" = 0), whatever
 *     the interleaving of appends and pulls.  (The reference starts by pulling TWO segments, :877-878: a fresh stream
 *     renders nothing until two are there or it is finished.)
 *   grail_stream_finish: the source of the utterances marked in `which` (n_utt bytes; NULL = all) has ended: what is
 *     pending is rendered, the last segment fades out (:906-912) and the row ends, as with a closed batch.
 *   grail_stream_pending: segments appended but not yet pulled by the Sequencer, per utterance (host memory [n_utt]);
 *     synchronises.  What an interactive front end needs to feed its chain just in time — the reference's source
 *     hands over ' ' (a Silence phoneme, src/lib.rs:1201 and the transcriber's no-rule case :1158-1163) whenever the
 *     Sequencer asks and no text is waiting.
 * Every ring holds ring_segments segments per utterance (a power of two, 4 .. 65536; 0 = 64): two the Sequencer is
 * working on and ring_segments - 2 pending; an append that does not fit fails with GRAIL_ERR_BUFFER_TOO_SMALL and
 * changes nothing.  Live streams run the general kernel instantiations (nothing is known about segments to come). */
int grail_stream_open_live(grail_ctx *ctx, uint32_t n_utt, const uint32_t *voice_ids, const uint32_t *jitter_seeds,
                           uint32_t ring_segments, int caller_built_elems, grail_stream **out);
int grail_stream_append(grail_ctx *ctx, grail_stream *stream, const grail_phoneme_elem *segs,
                        const uint32_t *seg_offsets);
int grail_stream_append_elems(grail_ctx *ctx, grail_stream *stream, const grail_sequence_elem *segs,
                              const uint32_t *seg_offsets);
int grail_stream_finish(grail_ctx *ctx, grail_stream *stream, const uint8_t *which);
int grail_stream_pending(grail_ctx *ctx, grail_stream *stream, uint32_t *pending);

/* One-call forms: upload, synthesize, copy back (GRAIL_OUT_HOST) or leave in
 * place (GRAIL_OUT_DEVICE), wait.  With GRAIL_OUT_HOST the rows are rendered in blocks of up to
 * 4096 utterances while the previous block travels over PCIe on a second stream, so the call
 * costs about max(kernel, copy) instead of their sum and needs two blocks of HBM, not the batch.  out_len is host memory [n_utt] or NULL.
 * GRAIL_OUT_HOST overwrites all n_utt*out_stride floats: each row is its
 * samples followed by zeros.  GRAIL_OUT_DEVICE leaves the tail untouched. */
int grail_synthesize_batch(grail_ctx *ctx, const grail_phoneme_elem *segs,
                           const uint32_t *seg_offsets, const uint32_t *voice_ids,
                           const uint32_t *jitter_seeds, uint32_t n_utt, float *out,
                           uint64_t out_stride, uint32_t *out_len, uint32_t flags);
int grail_synthesize_batch_elems(grail_ctx *ctx, const grail_sequence_elem *segs,
                                 const uint32_t *seg_offsets, const uint32_t *voice_ids,
                                 const uint32_t *jitter_seeds, uint32_t n_utt, float *out,
                                 uint64_t out_stride, uint32_t *out_len, uint32_t flags);

/* ---- text front half + PCM sink ------------------ */
/* TranscriptionRule  src/lib.rs:1030-1036; strings are Unicode scalar values (str::chars). */
typedef struct grail_rule {
    const uint32_t *string;
    uint32_t        string_len;
    const int32_t  *phonemes;   /* grail_phoneme */
    uint32_t        n_phonemes;
} grail_rule;
/* languages::generic()  src/languages/mod.rs:4-34; returns the rule count. */
uint32_t grail_language_generic(const grail_rule **rules, int *case_sensitive);
/* Transcriber::next until None  src/lib.rs:1116-1191.  leading_silence != 0 is
 * `.transcribe(language)` (buffer seeded with Silence, :1201); 0 starts with an empty buffer as
 * the reference's own unit tests do (:1212-1225).  *n_out is the full count even when > cap. */
int grail_transcribe(const uint32_t *text, uint32_t text_len, const grail_rule *rules,
                     uint32_t n_rules, int case_sensitive, int leading_silence,
                     int32_t *out_phonemes, uint32_t cap, uint32_t *n_out);
/* Intonator::next  src/lib.rs:1057-1075 (`.intonate(language, voice)` :1081). */
int grail_intonate(const grail_voice *voice, const int32_t *phonemes, uint32_t n,
                   grail_phoneme_elem *out);
/* text.chars().transcribe(languages::generic()).intonate(languages::generic(), voice)
 * — the front of examples/cli.rs:176-179.  out == NULL only counts. */
int grail_text_to_phoneme_elems(const grail_voice *voice, const char *text_utf8,
                                grail_phoneme_elem *out, uint32_t cap, uint32_t *n_out);
/* The whole chain of examples/cli.rs:175-184 for n texts: text i is spoken with
 * voices[voice_ids[i]] (NULL: voice 0) and jitter seed seeds[i] (NULL: 0, as the CLI). */
int grail_say_batch(grail_ctx *ctx, const char *const *texts_utf8, uint32_t n_texts,
                    const uint32_t *voice_ids, const uint32_t *jitter_seeds, float *out,
                    uint64_t out_stride, uint32_t *out_len, uint32_t flags);
/* `(x * i16::MAX as f32) as i16` of examples/cli.rs:49 on the device: rows of f32 -> rows of
 * i16, first len_dev[u] samples of each row; all pointers are device memory. Asynchronous.
 * max_len must be at least every len_dev[u] (the launch is sized from it: samples of a row at or past
 * max_len are not converted), and every len_dev[u] at most both strides.  Any alignment of the two
 * bases and any strides give the same samples; 16-byte aligned addresses take the vector path. */
int grail_pcm16_async(grail_ctx *ctx, const float *in_dev, uint64_t in_stride,
                      const uint32_t *len_dev, uint32_t n_utt, uint32_t max_len,
                      int16_t *out_dev, uint64_t out_stride);
/* grail_batch_synthesize_async() with the examples/cli.rs:49 conversion fused into the kernel's
 * store: rows of i16 PCM in device memory, out_stride in samples; 2 B instead of 4 B of HBM
 * written per sample and no f32 copy anywhere.  out_dev 8-byte aligned and out_stride % 4 == 0
 * give vector stores (any other stride: 2-byte stores in runs of 16 samples, + 2 % on the headline batch). */
int grail_batch_synthesize_pcm16_async(grail_ctx *ctx, const grail_batch *batch, int16_t *out_dev,
                                       uint64_t out_stride, uint32_t *out_len_dev);
/* grail_synthesize_batch() with the conversion fused the same way: rows of i16 PCM (half the
 * PCIe bytes of the f32 form).  Same flags and row semantics. */
int grail_synthesize_batch_pcm16(grail_ctx *ctx, const grail_phoneme_elem *segs,
                                 const uint32_t *seg_offsets, const uint32_t *voice_ids,
                                 const uint32_t *jitter_seeds, uint32_t n_utt, int16_t *out,
                                 uint64_t out_stride, uint32_t *out_len, uint32_t flags);
/* Per-row digest of rendered rows, computed on the device (comparing a 25 GB batch over PCIe is
 * pointless): sums[u] = sum of the samples' IEEE bit patterns mod 2^64, maxabs[u] = largest
 * finite |x| (0 where there is none), nonfinite[u] = count of NaN/Inf, over the first len_dev[u]
 * samples of row u.  Every len_dev[u] must be at most in_stride (the length is not clamped).
 * The sum sees any single changed sample, the sign of a zero included, but it is blind to a
 * permutation of the samples within a row: use grail_batch_compare beside it where the order matters.
 * in_dev/len_dev are device memory, the three results host memory [n_utt].  Synchronous. */
int grail_batch_digest(grail_ctx *ctx, const float *in_dev, uint64_t in_stride,
                       const uint32_t *len_dev, uint32_t n_utt, uint64_t *sums, float *maxabs,
                       uint32_t *nonfinite);
/* Per-row distance between two renderings of one batch, computed on the device (fast mode against
 * exact mode at full size), over the first len_a_dev[u] samples of row u.  d = |a - b| is computed in
 * binary32 (denormals kept).  Where d is finite it enters maxdiff[u] = max d and sumsq[u] = sum of
 * (double)d^2 (in no particular order).  Where d is not finite the sample enters neither, and it counts
 * in mismatches[u] unless both sides carry the same bits or both are NaN:
 *     (NaN, NaN) of any payloads, (+Inf, +Inf), (-Inf, -Inf)        0
 *     (+Inf, -Inf), (NaN, +-Inf), (NaN, finite), (finite, +-Inf)     1
 *     two finite samples whose difference overflows (3e38, -3e38)   1
 * mismatches[u] counts 1 more if len_a_dev[u] != len_b_dev[u] (the rows are still compared over
 * len_a_dev[u] samples).  -0.0 and +0.0 compare equal (d = 0): compare is blind to the sign of a zero,
 * which grail_batch_digest sees.  Every length must be at most stride (the lengths are not clamped).
 * a/b/len_* are device memory, the three results host memory [n_utt].  Synchronous. */
int grail_batch_compare(grail_ctx *ctx, const float *a_dev, const float *b_dev, uint64_t stride,
                        const uint32_t *len_a_dev, const uint32_t *len_b_dev, uint32_t n_utt,
                        float *maxdiff, double *sumsq, uint32_t *mismatches);
/* save_wav  examples/cli.rs:28-67: 44-byte RIFF header (PCM, mono, 16 bit) + samples. */
int grail_wav_write_i16(const char *path, const int16_t *pcm, uint32_t n, uint32_t sample_rate);

/* ---- mixing: rendered rows -> tracks, on the device ---------------------------------------------------------------
 * An ITEM i adds one rendered row, item_rows[i], using its first row_len[row] samples, scaled by item_gains[i], into
 * track item_tracks[i], starting at track sample item_offsets[i].  Samples at or past track_len are dropped; an item
 * that starts at or past track_len adds nothing.  For every track sample s of track t:
 *
 *     acc = +0.0f                         (GRAIL_MIX_ACCUMULATE: acc = the track's current value)
 *     for each item i covering (t, s), in ascending item_rows[i], ties in the order the items were given:
 *         acc = acc + gain_i * x           (binary32; the product rounded, then the sum rounded; never a fused multiply-add)
 *
 * Samples that no item covers are +0.0, or left untouched with GRAIL_MIX_ACCUMULATE.  Track memory between track_len
 * and track_stride is never written.  An uncovered lane skips the add rather than adding zero (adding +0.0 would turn
 * a -0.0 into +0.0).  The order is by row, not by item index: that lets grail_batch_mix render a batch in blocks of
 * rows and still produce the same bits.  No atomics: every sample is one left fold in a fixed order, so the result is
 * bit-identical across devices, block sizes and kernel tilings, and a three-line CPU loop reproduces it.
 * GRAIL_ERR_INVALID_ARG, tracks unwritten: an item's row >= n_rows, an item's track >= n_tracks, track_len >
 * track_stride, a row_len > row_stride, or a pointer the call needs is NULL (also: more than 4 194 304 tracks). */
#define GRAIL_MIX_ACCUMULATE 1u   /* add into the tracks' contents instead of starting from +0.0 */

/* rows_dev: device [n_rows][row_stride]; row_len: HOST [n_rows] (grail_batch_lengths / out_len);
 * items: HOST arrays [n_items], copied before the call returns; item_tracks NULL = track 0, item_gains NULL = 1.0f;
 * tracks_dev: device [n_tracks][track_stride], track_len <= track_stride.  Queued on ctx's stream behind earlier
 * work (a grail_batch_synthesize_async before it needs no sync).  Rows and tracks must not overlap.
 * The host side of a call is not free of waiting: it builds the plan into host memory of the context that the
 * previous mix of the context was uploaded from, and first waits until that upload has completed — which is queued
 * behind everything submitted before that previous mix.  So in render, mix, render, mix the second mix returns once
 * the first render has finished (the device never idles: the work queued after it is already there). */
int grail_mix_async(grail_ctx *ctx, const float *rows_dev, uint64_t row_stride, const uint32_t *row_len,
                    uint32_t n_rows, const uint32_t *item_rows, const uint32_t *item_tracks,
                    const uint64_t *item_offsets, const float *item_gains, uint32_t n_items,
                    float *tracks_dev, uint64_t track_stride, uint32_t n_tracks, uint64_t track_len,
                    uint32_t flags);

/* Render an uploaded batch and mix it, without ever holding all of its rows: contiguous row ranges are rendered
 * into scratch and mixed before the next range (same bits as rendering everything and calling grail_mix_async,
 * "arithmetic" = 0).  out_len: HOST [n_utt] or NULL.  Synchronous.
 * Block rule: 2 x 256 x CUs rows, CUs = what the planner plans for (the device's compute units, or option
 * "assume_compute_units"), fewer where half of the free HBM does not hold that many rows at the batch's stride (its
 * longest utterance rounded up to 64 samples).  A batch that fits in one block renders in one piece, exactly as
 * grail_batch_synthesize_async would; otherwise every block, the short last one included, is rendered with the kernel
 * family of a full block (as the host-output calls do), and blocks after the first are mixed with
 * GRAIL_MIX_ACCUMULATE, in block order; a block after the first that no item reads is not rendered.  The scratch (one
 * block of rows and their lengths) stays with the context for its next call, grown and never shrunk, until
 * grail_destroy: what an earlier call left counts as free HBM for the rule above.  In fast arithmetic ("arithmetic" = 1) the rows follow each block's kernel
 * family, as every fast-mode rendering does: within GRAIL_FAST_TOLERANCE of the exact rows, per row. */
int grail_batch_mix(grail_ctx *ctx, const grail_batch *batch, const uint32_t *item_rows,
                    const uint32_t *item_tracks, const uint64_t *item_offsets, const float *item_gains,
                    uint32_t n_items, float *tracks_dev, uint64_t track_stride, uint32_t n_tracks,
                    uint64_t track_len, uint32_t *out_len, uint32_t flags);

/* Pure host (no GPU): lay items end to end per track, in the accumulation order above.  Item i starts gaps[i]
 * samples after the end of the previous item on its track (the first at gaps[i]); a negative gap overlaps
 * (cross-fade); a start below 0 is GRAIL_ERR_INVALID_ARG.  gaps NULL = 0.  track_len: HOST [n_tracks], end of the
 * last item per track (the furthest end of any of its items, where a negative gap lets an item end before the one
 * before it; 0 for a track without items).  item_tracks NULL = track 0. */
int grail_mix_place_sequential(const uint32_t *row_len, uint32_t n_rows, const uint32_t *item_rows,
                               const uint32_t *item_tracks, const int64_t *gaps, uint32_t n_items,
                               uint32_t n_tracks, uint64_t *item_offsets, uint64_t *track_len);

/* Tracks -> interleaved i16 frames (frames_dev[f * n_tracks + t]) with the examples/cli.rs:49 conversion of
 * pcm16.h: what a multichannel WAV's data chunk and a sound card's callback hold.  n_frames <= track_stride.
 * Asynchronous. */
int grail_pcm16_frames_async(grail_ctx *ctx, const float *tracks_dev, uint64_t track_stride,
                             uint32_t n_tracks, uint64_t n_frames, int16_t *frames_dev);

/* save_wav for n_channels interleaved channels; n_channels = 1 is byte-identical to grail_wav_write_i16. */
int grail_wav_write_i16_frames(const char *path, const int16_t *frames, uint32_t n_frames,
                               uint32_t n_channels, uint32_t sample_rate);

/* ---- levels: how loud rendered rows are, measured on the device -----------------------------------------------------
 * For a row of n = len[u] samples and a frame length F (samples, 256 <= F <= 1 048 576):
 *   - Frame f holds the samples t in [f*F, min((f+1)*F, n)), t counted from the row's first sample.  A row has
 *     ceil(n / F) frames; an empty row has none.
 *   - A sample is FINITE when |x| <= FLT_MAX.  A sample that is not is counted and otherwise skipped.
 *   - PEAK of a frame: the largest |x| of its finite samples, +0.0 if there are none.
 *   - SUM OF SQUARES of a frame, binary64: 256 partial sums p[j], j = t mod 256; each starts at +0.0 and is the left
 *     fold, in ascending t, of p[j] + (double)x * (double)x over the frame's finite samples with that j (the product of
 *     two binary32 values is exact in binary64, so a fused multiply-add gives the same bits).  Then the halving tree
 *         for w = 128, 64, ..., 1:  p[j] = p[j] + p[j + w]  for j < w
 *     and the frame's value is p[0].
 *   - ROW TOTALS: peak = the largest frame peak; sumsq = the left fold from +0.0, in ascending f, of the frames' sums
 *     with F = GRAIL_LEVEL_FRAME; nonfinite = the count.
 * No float atomics anywhere: a row's numbers are a pure function of its samples and F, not of row_stride, the row's
 * index, the number of rows, the alignment of rows_dev, the device or the launch.  A len[u] above row_stride is read
 * as row_stride.  -0.0 and denormals are finite samples like any other. */
#define GRAIL_LEVEL_FRAME      4096u      /* the frame length of the row totals (and of GRAIL_LEVEL_ACTIVE in the leveled mix) */
#define GRAIL_LEVEL_FRAME_MIN  256u
#define GRAIL_LEVEL_FRAME_MAX  1048576u
#define GRAIL_LEVEL_PEAK       0          /* level = peak */
#define GRAIL_LEVEL_RMS        1          /* level = sqrt(sumsq / len) */
#define GRAIL_LEVEL_ACTIVE     2          /* level = grail_active_level of the row */
#define GRAIL_LEVEL_ACTIVE_FLOOR_DB 40.0f /* the floor grail_batch_mix_leveled uses in GRAIL_LEVEL_ACTIVE */

/* Row totals.  Queued on ctx's stream behind earlier work (a grail_batch_synthesize_async before it needs no sync);
 * rows_dev: device [n_rows][row_stride]; len_dev: device [n_rows], the out_len a rendering wrote; results are DEVICE
 * arrays [n_rows], any of them may be NULL.  16-byte loads where rows_dev is 16-byte aligned and row_stride a multiple
 * of 4, 4-byte loads otherwise: same bits.  The per-frame numbers go through scratch that stays with the context
 * (16 bytes per GRAIL_LEVEL_FRAME samples of n_rows x row_stride), grown and never shrunk, until grail_destroy.
 * Without a usable device: GRAIL_ERR_NO_DEVICE. */
int grail_levels_async(grail_ctx *ctx, const float *rows_dev, uint64_t row_stride, const uint32_t *len_dev,
                       uint32_t n_rows, double *sumsq_dev, float *peak_dev, uint32_t *nonfinite_dev);

/* Per frame of `frame` samples: DEVICE arrays [n_rows][frames_stride], either may be NULL; frames past a row's last
 * are left unwritten.  The lengths live on the device, so the bound the host can check is on row_stride:
 * frames_stride >= ceil(row_stride / frame), else GRAIL_ERR_INVALID_ARG (as for a frame outside 256 .. 1 048 576).
 * One wavefront folds one frame, so frames much longer than GRAIL_LEVEL_FRAME need many rows to fill the device. */
int grail_frame_levels_async(grail_ctx *ctx, const float *rows_dev, uint64_t row_stride, const uint32_t *len_dev,
                             uint32_t n_rows, uint32_t frame, double *frame_sumsq_dev, float *frame_peak_dev,
                             uint64_t frames_stride);

/* Pure host (no GPU): the gain that brings item i's row to item_level_db[i] decibels (0 dB = level 1.0),
 *     gain_i = (float)(pow(10.0, item_level_db[i] / 20.0) / level(row_i))     computed in binary64, rounded once.
 * mode: GRAIL_LEVEL_PEAK (needs peak), GRAIL_LEVEL_RMS (needs sumsq and row_len), GRAIL_LEVEL_ACTIVE (needs
 * active_level: one grail_active_level per row); the arrays a mode does not need may be NULL, as may nonfinite (no row
 * holds a non-finite sample) and n_unleveled.  A row whose level is 0 or that holds a non-finite sample gets gain 0 and
 * its ITEMS are counted in *n_unleveled: not an error, a batch may hold an empty utterance.
 * GRAIL_ERR_INVALID_ARG, outputs unwritten: an unknown mode, an item's row >= n_rows, a NULL array the mode needs. */
int grail_level_gains(int mode, const double *sumsq, const float *peak, const uint32_t *nonfinite,
                      const uint32_t *row_len, const double *active_level, uint32_t n_rows,
                      const uint32_t *item_rows, const float *item_level_db, uint32_t n_items, float *item_gains,
                      uint32_t *n_unleveled);

/* Pure host: the "active" level of one row from its frames' sums of squares [ceil(row_len / frame)] (speech has
 * pauses; the RMS of a whole row under-reads it).  A frame's mean square is its sum over its own sample count (the
 * last frame may be short); frames whose mean square is at least 10^(-floor_db / 10) of the loudest frame's are
 * active; returns sqrt(sum of their sums / sum of their sample counts), both folded in ascending frame order in
 * binary64.  0.0 for an empty or all-silent row. */
double grail_active_level(const double *frame_sumsq, uint32_t row_len, uint32_t frame, float floor_db);

/* grail_batch_mix with a level per item instead of a gain: same arguments, block rule, scratch and skipping of blocks
 * no item reads.  Per block: render, measure (grail_levels_async's kernels), copy the block's numbers to the host (at
 * most 16 bytes a row, or the frame sums in GRAIL_LEVEL_ACTIVE: frames of GRAIL_LEVEL_FRAME, floor
 * GRAIL_LEVEL_ACTIVE_FLOOR_DB), grail_level_gains, mix: one small copy and one wait per block more than
 * grail_batch_mix.  The tracks are the bits grail_batch_mix gives with the gains that were used.
 * item_gains_out: HOST [n_items] or NULL, those gains; n_unleveled: the items that got gain 0, or NULL; both are
 * written only when the call succeeds.  Invalid arguments follow the mixing section's rules. */
int grail_batch_mix_leveled(grail_ctx *ctx, const grail_batch *batch, const uint32_t *item_rows,
                            const uint32_t *item_tracks, const uint64_t *item_offsets, const float *item_level_db,
                            int mode, uint32_t n_items, float *tracks_dev, uint64_t track_stride, uint32_t n_tracks,
                            uint64_t track_len, uint32_t *out_len, float *item_gains_out, uint32_t *n_unleveled,
                            uint32_t flags);

/* ---- levels, continued: K-weighted gated loudness (ITU-R BS.1770-4 / EBU R 128) ----------------------------------------
 * All arithmetic is IEEE binary64, every operation rounded by itself (no fused multiply-add anywhere: unlike the square
 * of a binary32, z*z below is not exact), evaluated exactly in the order written.  As above, a row's numbers are a pure
 * function of its samples, the sample rate and the ten coefficients: not of row_stride, the row's index, the number of
 * rows, the alignment of rows_dev, the device or the launch.  No atomics.
 *   - THE FILTER AND THE HOPS.  coef[10] = b0 b1 b2 a1 a2 of the shelf, then d0 d1 d2 e1 e2 of the high-pass.  For a row
 *     of n = min(len[u], row_stride) samples, H = sample_rate / 10 (integer division: a hop of 100 ms), the state
 *     s1 = s2 = s3 = s4 = +0.0 at the row's first sample, and for t = 0 .. n-1 in ascending order:
 *         v  = (double)x[t]          (a sample that is not finite is counted and enters as +0.0)
 *         y  = b0*v + s1;   s1 = (b1*v - a1*y) + s2;   s2 = b2*v - a2*y        (transposed direct form II)
 *         z  = d0*y + s3;   s3 = (d1*y - e1*z) + s4;   s4 = d2*y - e2*z
 *         acc = acc + z*z            (acc = +0.0 at the first sample of every hop)
 *     Hop h holds the samples [h*H, (h+1)*H); its value is acc after its last sample.  A row has floor(n / H) hops; the
 *     samples after the last whole hop are filtered and belong to no hop.  Denormals are not flushed: after a row falls
 *     silent the filter's state decays through the binary64 denormal range.
 *   - THE GATE, in the linear domain (no logarithm on the device).  Blocks of four hops every hop: for j = 0 .. hops-4,
 *         z_j = (((h[j] + h[j+1]) + h[j+2]) + h[j+3]) / (4.0 * H).
 *     A = the blocks with z_j > GRAIL_LOUDNESS_ABS_GATE.  If A is empty the gated mean square is +0.0.  Otherwise
 *     r = 0.1 * (sum(A) / |A|), B = the blocks of A with z_j > r (never empty), and the GATED MEAN SQUARE is
 *     sum(B) / |B|; both sums are left folds from +0.0 in ascending j, the counts converted to double.  A row of fewer
 *     than four hops (shorter than 400 ms) has no block and reads +0.0.
 *   - loudness in LUFS = -0.691 + 10 log10(gated mean square); level = sqrt(gated mean square * GRAIL_LOUDNESS_LEVEL_SCALE),
 *     so that 20 log10(level) is the loudness in LUFS. */
#define GRAIL_LOUDNESS_ABS_GATE    1.1724653045822981e-07   /* 10^((-70 + 0.691) / 10): the mean square of -70 LUFS */
#define GRAIL_LOUDNESS_LEVEL_SCALE 0.8529037030705663       /* 10^(-0.691 / 10) */
#define GRAIL_LOUDNESS_RATE_MIN    2560u                    /* a hop then holds at least 256 samples */
#define GRAIL_LOUDNESS_RATE_MAX    1048576u
/* level = grail_loudness_level(gated mean square of the row); item_level_db is then a target in LUFS.  (3 stays an
 * unknown mode.) */
#define GRAIL_LEVEL_LOUDNESS       4

/* Pure host: the ten K-weighting coefficients for a sample rate, by the bilinear transform of the analogue prototypes
 * (BS.1770 prints them for 48 kHz only).  With K = tan(pi * f0 / rate), a0 = 1 + K/Q + K*K:
 *   shelf      f0 = 1681.974450955533 Hz, G = 3.999843853973347 dB, Q = 0.7071752369554196, Vh = 10^(G/20),
 *              Vb = Vh^0.4996667741545416: b = (Vh + Vb*K/Q + K*K)/a0, 2*(K*K - Vh)/a0, (Vh - Vb*K/Q + K*K)/a0;
 *   high-pass  f0 = 38.13547087602444 Hz, Q = 0.5003270373238773: b = 1, -2, 1;
 *   both       a1 = 2*(K*K - 1)/a0, a2 = (1 - K/Q + K*K)/a0.
 * GRAIL_ERR_INVALID_ARG, coef unwritten: a rate outside GRAIL_LOUDNESS_RATE_MIN .. GRAIL_LOUDNESS_RATE_MAX, coef NULL.
 * Below 3 364 Hz the shelf's corner lies above half the rate and the ten numbers are no K-weighting (the library renders
 * at 8 - 192 kHz).  The bits of tan and pow are the C library's: the device takes the ten doubles as an argument. */
int grail_kweighting(uint32_t sample_rate, double coef[10]);

/* Hop sums, gated mean squares and non-finite counts of rows, queued on ctx's stream like grail_levels_async.
 * coef: HOST [10], copied before the call returns; NULL = grail_kweighting(sample_rate).  gated_ms_dev: DEVICE double
 * [n_rows]; hop_sumsq_dev: DEVICE double [n_rows][hops_stride], hops past a row's last left unwritten, hops_stride >=
 * row_stride / H (else GRAIL_ERR_INVALID_ARG, as for a rate out of range); nonfinite_dev: DEVICE uint32 [n_rows]; any of
 * the three may be NULL.  The hop sums are what momentary (4 hops) and short-term (30 hops) loudness are built from.
 * Where hop_sumsq_dev is NULL the hops go through scratch that stays with the context (8 bytes per hop), grown and never
 * shrunk, until grail_destroy.  One lane filters one row from its first sample to its last (the recurrence is serial in
 * exact arithmetic), 64 rows to a wavefront: many rows fill the device, a lone long row is one lane's serial work
 * (measured on an MI355X: 10 000 000 samples in 746 ms, 75 ns a sample; 65 536 rows of 96 006 samples in 7.5 ms).
 * Without a usable device: GRAIL_ERR_NO_DEVICE. */
int grail_loudness_async(grail_ctx *ctx, const float *rows_dev, uint64_t row_stride, const uint32_t *len_dev,
                         uint32_t n_rows, uint32_t sample_rate, const double *coef, double *gated_ms_dev,
                         double *hop_sumsq_dev, uint64_t hops_stride, uint32_t *nonfinite_dev);

/* THE SEGMENTED FORM: the same measurement, parallel in time, for few long rows (a finished track).  The signature is
 * grail_loudness_async's and so is everything else: binary64, every operation rounded by itself, no fused multiply-add;
 * the ten coefficients; H = sample_rate / 10; n = min(len[u], row_stride); non-finite samples counted and entering as
 * +0.0; the gate; the outputs and which of them may be NULL; hops past a row's last left unwritten; the hops_stride rule,
 * the rate range, the scratch for hop_sumsq_dev == NULL (plus 4 bytes per hop for the counts); the error returns, and one
 * more: the call is one grid of a wavefront per 64 hops of a row, ceil(ceil(row_stride / H) / 64) per row, and more than
 * 2^26 - 1 of them in all is GRAIL_ERR_INVALID_ARG (a grid holds fewer than 2^32 lanes).  The one difference is where the
 * filter's state starts.  With P = GRAIL_LOUDNESS_WARMUP_HOPS:
 *   - Hop h of a row is the acc of the serial recurrence above, run with s1 = s2 = s3 = s4 = +0.0 at sample
 *     max(h, P) * H - P * H (that is (h - P) * H for h >= P and 0 for h < P) and over the samples from there to
 *     (h + 1) * H - 1 in ascending order, acc = +0.0 at sample h * H.
 *   - Hops 0 .. P are therefore grail_loudness_async's hops bit for bit, and a row of at most P + 1 hops reads exactly
 *     what grail_loudness_async reads: hops, gated mean square and count.
 *   - nonfinite[u] counts every non-finite sample among x[0 .. n) once: the warm-up of a later hop does not count it
 *     again, and the samples after the last whole hop, which belong to no hop, are counted as they are there.
 *   - A row's numbers remain a pure function of its samples, the rate and the coefficients: not of row_stride, the row's
 *     index, its neighbours, the alignment, the device, the launch or the number of segments in flight.  No atomics.
 *   - WHAT IT IS NOT: grail_loudness_async's bits from hop P + 1 on.  In exact arithmetic the two differ by the response
 *     to the state s = (s1, s2, s3, s4) that the serial call holds at the segment's first sample and this call replaces
 *     by zero.  Both sections have complex poles (Q > 1/2), of radius rho = sqrt(a2) for the shelf and r = sqrt(e2) for
 *     the high-pass, rho < r; the all-pole response of such a pair is g[k] = r^k sin((k+1) th) / sin(th), |g[k]| <=
 *     (k+1) r^k.  A section in transposed direct form II started from its state (p, q) with no input gives p g[k] +
 *     q g[k-1]; the high-pass answers the shelf's decaying output through d0 g[k] + d1 g[k-1] + d2 g[k-2], at most
 *     4 (k+1) r^(k-2).  Summing the convolution, k = P * H samples after the start and for every later sample of the hop
 *         |dz| <= D * (|s1| + |s2| + |s3| + |s4|),    D = (P*H + 1) * r^(P*H - 2) * (1 + 4 / (rho * (1 - rho / r)^2)).
 *     r^H is the decay of a time constant in seconds over 100 ms, so it does not depend on the rate: 3.97e-11 .. 3.99e-11
 *     from 8 to 192 kHz, and r^(P*H) = 6.3e-32.  D is 5.0e-27 at 8 kHz, 1.8e-25 at 44.1 kHz, 2.3e-25 at 48 kHz and
 *     1.2e-23 at 192 kHz (1.8e-21 at GRAIL_LOUDNESS_RATE_MAX): below 2^-60 of the state at every rate where the ten
 *     numbers are a K-weighting, while every operation that formed that state rounded it by up to 2^-53 of itself.  In
 *     the samples: the state is at most S * max|x|, with Y = (|b0| + |b1| + |b2|) / (1 - rho)^2, Z = 4 Y / (1 - r)^2 and
 *     S = (|b1| + 2 |b2|) + (|a1| + 2 |a2|) Y + 4 Y + (|e1| + 2 |e2|) Z, so |dz| <= D * S * max|x|.
 *     D is the truncation in EXACT arithmetic.  What remains between the two calls in binary64 is larger and is not
 *     truncation: the rounded recurrence has a dead band.  Two trajectories fed the same samples contract towards each
 *     other (by r per sample: 0.97 at 8 kHz, 0.995 at 48 kHz) only until they are a few units in the last place of the
 *     state apart; there each step's roundings move them as much as the contraction pulls, and they stay that far apart,
 *     so most hops differ in their last bits.  That floor is the same one the serial call has against its own exact
 *     value.  Measured between the numpy models of
 *     the two contracts over noise, a tone on DC, a square wave before silence and noise bursts (8 kHz, 30 hops): at most
 *     6.2e-15 of full scale in a hop's mean square (|d hop| / H) and 1.8e-15 LU, 4 - 22 of the 30 hops bit-equal; P = 2
 *     gave 2.7e-14 LU, P = 1 gave 5.2e-10 LU.  tests/test_loudness_segmented_host.py asserts 100 times the measured.
 *   - For caller-supplied coef the call is still this pure function, but nothing is promised about its distance from
 *     grail_loudness_async's numbers.
 * WHICH CALL FOR WHAT: grail_loudness_async for many short rows (one pass over each sample, one lane per row);
 * this one for few long rows (P + 1 passes over each sample, and as many lanes as the rows have hops).  Measured on an
 * MI355X: a lone row of 10 000 000 samples at 48 kHz 2.58 ms against 750 ms (290 x); 64 rows of 10 minutes 13.8 ms; but
 * 65 536 rows of 96 006 samples 78.8 ms against 7.6 ms: a row of 20 hops fills a third of its wavefront's lanes. */
#define GRAIL_LOUDNESS_WARMUP_HOPS 3u
int grail_loudness_segmented_async(grail_ctx *ctx, const float *rows_dev, uint64_t row_stride, const uint32_t *len_dev,
                                   uint32_t n_rows, uint32_t sample_rate, const double *coef, double *gated_ms_dev,
                                   double *hop_sumsq_dev, uint64_t hops_stride, uint32_t *nonfinite_dev);

/* Pure host: the gate above over a row's n_hops hop sums, hop = H in samples; +0.0 for NULL, hop 0 or n_hops < 4. */
double grail_gated_mean_square(const double *hop_sumsq, uint32_t n_hops, uint32_t hop);
/* Pure host: -0.691 + 10 log10(gated_ms), -HUGE_VAL for 0; and sqrt(gated_ms * GRAIL_LOUDNESS_LEVEL_SCALE). */
double grail_loudness_lufs(double gated_ms);
double grail_loudness_level(double gated_ms);
/* Pure host: what a meter reads from a row's hop sums besides the integrated loudness.  hop = H in samples.
 * grail_loudness_window_max: the largest, over j = 0 .. n_hops - window_hops, of
 *     (left fold from h[j] of h[j] .. h[j + window_hops - 1] in ascending order) / ((double)window_hops * (double)hop),
 * a mean square (grail_loudness_lufs gives its LUFS); +0.0 for NULL, hop 0, window_hops 0 or n_hops < window_hops.
 * window_hops 4 is the momentary loudness (for it the blocks are the gate's z_j bit for bit), 30 the short-term one. */
double grail_loudness_window_max(const double *hop_sumsq, uint32_t n_hops, uint32_t hop, uint32_t window_hops);
/* grail_loudness_range: the loudness range in LU after EBU Tech 3342.  s_j = the blocks of 30 hops as above, one every
 * hop, j = 0 .. n_hops - 30.  A = the blocks with s_j > GRAIL_LOUDNESS_ABS_GATE; if A is empty the result is +0.0.
 * r = 0.01 * (sum(A) / |A|), the sum a left fold from +0.0 in ascending j, the count converted to double: 20 LU below
 * the mean.  B = the blocks of A with s_j > r, sorted ascending (never empty).  lo = B[((|B| - 1) * 10 + 50) / 100] and
 * hi = B[((|B| - 1) * 95 + 50) / 100] in integer division (64-bit): Tech 3342's round((n - 1) p / 100 + 1), zero-based.
 * The result is 10.0 * log10(hi / lo); the bits of log10 are the C library's.  +0.0 for NULL, hop 0 or n_hops < 30. */
double grail_loudness_range(const double *hop_sumsq, uint32_t n_hops, uint32_t hop);
/* GRAIL_LEVEL_LOUDNESS in grail_level_gains: the per-row level is read from active_level, exactly as GRAIL_LEVEL_ACTIVE
 * reads it (one grail_loudness_level per row).  In grail_batch_mix_leveled: item_level_db[i] is the item's target in LUFS;
 * the sample rate is that of the context's voice table (voices that do not all have one whole-numbered rate within
 * GRAIL_LOUDNESS_RATE_MIN .. _MAX: GRAIL_ERR_INVALID_ARG, tracks and outputs unwritten); per block the rows go through
 * grail_loudness_async's kernels and 12 bytes a row are copied.  A row whose gated mean square is 0 gets gain 0 and is
 * counted in *n_unleveled: that includes every row shorter than 400 ms. */

/* ---- levels, continued: true peak (ITU-R BS.1770-4 Annex 2) ---------------------------------------------------------------
 * The sample peak of grail_levels_async under-reads what a converter reconstructs between the samples (by 3 dB for a
 * tone at a quarter of the rate, sampled 45 degrees off its crests).  The true peak is the largest magnitude of the row
 * oversampled four times by the Annex's 48-tap filter, taken as four phases of twelve taps, C[p][k] = N[p][k] / 8192:
 *     N[0] =   14,  90, -161, 272,  -487, 1125, 7964,  -838, 390, -218, 122,  -68
 *     N[1] = -239, 240, -424, 730, -1364, 3810, 6388, -1641, 832, -477, 271, -155
 *     N[2] = N[1] reversed,  N[3] = N[0] reversed
 * (the Annex's 48 coefficients as multiples of 2^-13; this table is the library's contract, at any sample rate: at 96 or
 * 192 kHz the filter only looks closer than the standard asks).  All arithmetic is IEEE binary64.  For a row of
 * n = min(len[u], row_stride) samples:
 *   - v[t] = (double)x[t] for 0 <= t < n and +0.0 for t < 0 and t >= n; memory between n and row_stride is never looked
 *     at, whatever it holds.  A sample that is not finite (|x| > FLT_MAX or NaN) is counted and enters as +0.0.
 *   - For every output time t = 0 .. n + 10 and phase p = 0 .. 3: acc = +0.0; for k = 0 .. 11 ascending
 *     acc = acc + C[p][k] * v[t - k]; y[p][t] = acc.  Every C[p][k] * v is exact in binary64 (a 13-bit numerator times a
 *     24-bit significand), so a fused multiply-add and a multiply followed by an add give the same bits.
 *   - The row's TRUE PEAK is the largest |y[p][t]| over all p and t, a double; +0.0 for an empty row.
 *     dBTP = 20 log10(true peak).
 * The eleven outputs after the row's last sample belong to the row: the filter rings on, and a mix places the row in front
 * of silence (a row [0, ..., 0, 1.0] reads 7964 / 8192 with them and 239 / 8192 without).  A maximum is associative and
 * commutative and no NaN is left to order, so the number is a pure function of the row's samples: not of row_stride, the
 * alignment of rows_dev, the row's index, the number of rows, the device or the launch.  No float atomics.
 * The Annex's phase 0 is no pass-through (its centre tap is 7964 / 8192 = 0.972), so a row's true peak can read up to
 * about 0.25 dB BELOW its sample peak; a caller who wants the larger of the two has grail_levels_async. */
#define GRAIL_TRUE_PEAK_PHASES 4
#define GRAIL_TRUE_PEAK_TAPS   12
/* Pure host: coef[p * 12 + k] = C[p][k].  GRAIL_ERR_INVALID_ARG for NULL. */
int grail_true_peak_coefficients(double coef[48]);

/* True peaks and non-finite counts of rows, queued on ctx's stream like grail_levels_async: rows_dev: device
 * [n_rows][row_stride] (rendered rows or finished tracks alike); len_dev: device [n_rows]; results are DEVICE arrays
 * [n_rows], either may be NULL.  16-byte loads where rows_dev is 16-byte aligned and row_stride a multiple of 4, 4-byte
 * loads otherwise: same bits.  The filter is FIR, so time is parallel: one wavefront takes a stretch of one row, and a
 * lone long row fills the device.  The stretches' maxima go through scratch that stays with the context (12 bytes per
 * 4096 samples of n_rows x row_stride), grown and never shrunk, until grail_destroy.
 * Without a usable device: GRAIL_ERR_NO_DEVICE. */
int grail_true_peak_async(grail_ctx *ctx, const float *rows_dev, uint64_t row_stride, const uint32_t *len_dev,
                          uint32_t n_rows, double *true_peak_dev, uint32_t *nonfinite_dev);

/* Pure host: 20 log10(true_peak), -HUGE_VAL for 0; NaN for a negative number (no true peak is one) and for NaN. */
double grail_true_peak_db(double true_peak);

/* Pure host: caps gains so that no item's row exceeds a ceiling.  c = pow(10.0, (double)ceiling_db / 20.0).  Item i with
 * row r and gain g = item_gains[i] (in and out) is limited when true_peak[r] > 0 and (double)fabsf(g) * true_peak[r] > c:
 * its new magnitude is q = (float)(c / true_peak[r]), rounded to nearest, and one float towards 0 from there if
 * (double)q * true_peak[r] > c, so that (double)q * true_peak[r] <= c holds exactly; the sign of g is kept.  *n_limited
 * (may be NULL) counts the items changed.  GRAIL_ERR_INVALID_ARG with nothing written: an item's row >= n_rows, a NULL
 * array with n_items > 0, a ceiling_db that is not finite. */
int grail_true_peak_limit_gains(const double *true_peak, uint32_t n_rows, const uint32_t *item_rows,
                                uint32_t n_items, float ceiling_db, float *item_gains, uint32_t *n_limited);

/* grail_batch_mix_leveled with a true-peak ceiling in dBTP: per block render, measure the level, measure the true peak
 * (grail_true_peak_async's kernels), copy 8 bytes a row more in the same wait, grail_level_gains,
 * grail_true_peak_limit_gains, mix.  The tracks are the bits grail_batch_mix gives with the gains that were used;
 * item_gains_out reports them, *n_limited (may be NULL) the items the ceiling changed; both as n_unleveled only when the
 * call succeeds.  The ceiling binds each ITEM: items that overlap on a track can still sum above it, and the mix rounds
 * each product once more; a caller measures the finished tracks with grail_true_peak_async.  A ceiling_db that is not
 * finite: GRAIL_ERR_INVALID_ARG.  (No new GRAIL_LEVEL_* mode: the ceiling works with every one of them.) */
int grail_batch_mix_leveled_limited(grail_ctx *ctx, const grail_batch *batch, const uint32_t *item_rows,
                                    const uint32_t *item_tracks, const uint64_t *item_offsets,
                                    const float *item_level_db, int mode, uint32_t n_items, float *tracks_dev,
                                    uint64_t track_stride, uint32_t n_tracks, uint64_t track_len, uint32_t *out_len,
                                    float *item_gains_out, uint32_t *n_unleveled, float ceiling_db,
                                    uint32_t *n_limited, uint32_t flags);

/* ---- levels, continued: limiter ----------------------------------------------------------------------------------------------
 * grail_batch_mix_leveled_limited caps each item by one gain: items that overlap on a track can still sum above the
 * ceiling, and one loud syllable pulls its whole utterance down.  The limiter is the stage after the mix: a gain curve
 * computed from a look-ahead window and applied sample by sample, so that a finished track keeps its loudness and
 * gives way only where it is too high.  c = ceiling (linear, a finite float > 0), L = 2^l = 2^lookahead_log2 samples of
 * look-ahead, l = 0 .. GRAIL_LIMIT_LOOKAHEAD_LOG2_MAX (a power of two, so that the smoothing divides exactly; 256 samples
 * are 5.3 ms at 48 kHz; l = 0 is a hard limiter).  Rows come in GROUPS of `group` consecutive rows that share one gain
 * curve (1: every row alone; 2: a linked stereo pair); n_rows is a multiple of group.  The members of a group must have
 * equal n = min(len, row_stride); a group whose members differ is REFUSED: its out rows are left unwritten and its
 * results read min_gain = NaN, n_limited = GRAIL_LIMIT_REFUSED, nonfinite = 0.  For a group of n samples, Q = 2^24:
 *   1. Detection, per member row: v[t] and the outputs y[p][u], u = 0 .. n + 10, are those of the true-peak section above
 *      (binary64, the same fold, a non-finite sample counted and entering as +0.0).  e[u] = max over p of |y[p][u]|;
 *      d[t] = max(|v[t]|, e[t], ..., e[t + 11]): the sample and every oversampled output it feeds.  The group's d[t] is
 *      the maximum over its members.
 *   2. The required gain as an integer: q[t] = Q if d[t] <= (double)c, else min(Q, floor((double)c * Q / d[t])), one
 *      correctly rounded binary64 division (c * Q is exact).  q[s] = Q for s < 0 and s >= n.
 *   3. Look-ahead: m[s] = min(q[s], ..., q[s + L - 1]) for s = -(L - 1) .. n - 1.
 *   4. Smoothing: S[t] = m[t - L + 1] + ... + m[t], an integer of at most 2^34, so every summation order gives it;
 *      g[t] = (float)((double)S[t] * 2^-(24 + l)): the product is exact, the conversion rounds once.
 *   5. Apply, per member row: z[t] = g[t] * x[t] in binary32, then clamped: z < -c gives -c, z > c gives c, anything else
 *      (-0.0 included) stays.  A non-finite x[t] writes +0.0.  out between n and out_stride is never written.
 * Nothing above depends on chunking, layout, alignment, the rows around or the launch: out and the results are a pure
 * function of the group's samples, c, l.  No float atomics.
 * GUARANTEED: every m[s] under S[t] has q[t] in its window, so g[t] <= q[t] / Q <= c / d[t], and after the clamp
 * |z[t]| <= c holds exactly.  A group whose d never exceeds c has g = 1.0f throughout: z equals x bit for bit.
 * NOT guaranteed: the true peak of z exactly under c, because g varies across the filter's twelve taps.  g moves by at
 * most 1 / L per sample, which gives the BOUND
 *     true peak(z) <= c + (11 / L) * TAP_SUM * max|x| + TAP_SUM * 2^-24 * c,   TAP_SUM = 16571 / 8192
 * (the largest sum of |C[p][k]| of a phase).  The bound is loose (DESIGN.md §4.12 has overshoots of the model: thousandths of
 * a dB at L >= 16).  Measure the result with grail_true_peak_async; for delivery ask for a hair less than the rule's
 * ceiling.  Attack and release are both L samples: there are no separate times. */
#define GRAIL_LIMIT_LOOKAHEAD_LOG2_MAX 10
#define GRAIL_LIMIT_REFUSED 0xFFFFFFFFu
/* The samples of one workgroup's stretch of a group.  Not part of the contract (no number depends on it): it is here so
 * that tests can aim at the seams. */
#define GRAIL_LIMIT_CHUNK 4096

/* Pure host: the one float that a ceiling in dBTP is: (float)pow(10.0, (double)ceiling_db / 20.0). */
float grail_limit_ceiling(float ceiling_db);

/* The limiter above, queued on ctx's stream like grail_true_peak_async: rows_dev: device [n_rows][row_stride] (finished
 * tracks or rendered rows alike); len_dev: device [n_rows]; out_dev: device [n_rows][out_stride], out_stride >=
 * row_stride.  Results are DEVICE arrays [n_rows / group], any may be NULL: min_gain (the smallest g of the group; 1.0f
 * for a group of no samples), n_limited (the samples t with S[t] < L * Q), nonfinite (summed over the members).
 * out_dev must not overlap rows_dev: the look-ahead reads ahead of what other workgroups write.  16-byte loads and stores
 * where both bases are 16-byte aligned and both strides multiples of 4, 4-byte ones otherwise: same bits.  One workgroup
 * takes a stretch of one group, so a lone long track fills the device.  Scratch stays with the context (16 bytes per
 * group and 4096 samples), grown and never shrunk, until grail_destroy.
 * GRAIL_ERR_INVALID_ARG, nothing queued: lookahead_log2 > 10; group 0 or no divisor of n_rows; a ceiling that is not a
 * finite number above 0; out_stride < row_stride; a NULL buffer with samples to read; overlapping ranges.  These come
 * first; without a usable device: GRAIL_ERR_NO_DEVICE. */
int grail_limit_async(grail_ctx *ctx, const float *rows_dev, uint64_t row_stride, const uint32_t *len_dev, uint32_t n_rows,
                      uint32_t group, float ceiling, uint32_t lookahead_log2, float *out_dev, uint64_t out_stride,
                      float *min_gain_dev, uint32_t *n_limited_dev, uint32_t *nonfinite_dev);

/* ---- levels, continued: sample-rate conversion ----------------------------------------------------------------------------------
 * A context's voice table has one rate, and rendering at a lower one is a different signal (formants above Nyquist are
 * dropped, the carrier's harmonics alias).  The resampler is the stage after the mix and the limiter: finished rows at
 * rate_in become the same audio at rate_out, by a rational-ratio polyphase FIR filter.  All arithmetic is IEEE binary64.
 * RATIO.  Rates are whole numbers, both > 0, rate_in != rate_out.  g = gcd(rate_in, rate_out), U = rate_out / g (up),
 * D = rate_in / g (down), Z = GRAIL_RESAMPLE_ZERO_CROSSINGS = 24 zero crossings per side at the lower of the two rates,
 * P = 2 * ceil(Z * max(U, D) / U) taps per output sample (even).  A pair is supported when U * P <=
 * GRAIL_RESAMPLE_TABLE_MAX = 32 768 table entries, otherwise GRAIL_ERR_INVALID_ARG: every pair among 8 000, 11 025,
 * 16 000, 22 050, 24 000, 44 100, 48 000, 96 000 fits (44 100 -> 16 000: U = 160, D = 441, P = 134, 21 440 entries;
 * 48 000 -> 11 025: U = 147, D = 640, P = 210, 30 870 entries) but 11 025 <-> 96 000 (61 440 and 61 446 entries: go
 * through 48 000).  Equal rates are refused: a caller who asked for no change must not get a low-pass.
 * TABLE.  A Kaiser-windowed sinc, beta = 8.0, cutoff f = 0.9 * min(1, U / D) cycles per input sample, half-width
 * W = P / 2 input samples, indexed by an integer j so that it is exactly even.  For j = -(P/2) U .. (P/2) U - 1, with
 * x = (double)|j| / (double)U:
 *     H(j) = f * sinc(f * x) * I0(beta * sqrt(1 - (x / W)^2)) / I0(beta)
 *     sinc(a) = sin(pi a) / (pi a), sinc(0) = 1
 *     I0 by its power series, the terms ((y / 2)^k / k!)^2 summed ascending until a term no longer changes the sum
 *     N(j) = llrint(H(j) * 2^26), ties to even;   C[p][k] = N((k - P/2) U + p) / 2^26,  p = 0 .. U - 1, k = 0 .. P - 1
 * |N| < 2^26 because |H| <= 0.9.  A 27-bit numerator times a 24-bit significand is exact in binary64, so a fused
 * multiply-add and a multiply followed by an add give the same bits (the argument of the true-peak section).  The bits
 * of N come from the C library's sin: the table as grail_resample_coefficients returns it is the contract, as with
 * grail_kweighting.
 * SAMPLES.  For a row of n = min(len[u], row_stride) samples:
 *   - v[t] = (double)x[t] for 0 <= t < n and +0.0 outside; a sample that is not finite (|x| > FLT_MAX or NaN) is counted
 *     once and enters as +0.0; memory between n and row_stride is never looked at, whatever it holds.
 *   - n_out = min(ceil(n U / D), out_stride), computed in 64 bits.
 *   - For output m = 0 .. n_out - 1: a = m D in 64 bits, p = a mod U, i0 = a div U; acc = +0.0; for k = 0 .. P - 1
 *     ascending acc = acc + C[p][k] * v[i0 + P/2 - k]; y[m] = (float)acc, one rounding.
 *   - Output m sits at input time m D / U exactly: zero delay, linear phase.
 *   - out between n_out and out_stride is never written.  out_len[u] = n_out; nonfinite[u] = the count over all n
 *     samples (also where out_stride cut the output short).
 * Nothing above depends on chunking, layout, alignment, the rows around or the launch: out and the results are a pure
 * function of the row's samples and the two rates.  No float atomics.
 * NOT promised: the output's peak can exceed the input's, because the filter overshoots: limit or measure after
 * resampling, not before.  The passband ends at about 0.79 of the lower Nyquist frequency; the stopband starts at the
 * lower Nyquist frequency, at about 80 dB.  There is no pass-through phase: no output is a copy of an input sample. */
#define GRAIL_RESAMPLE_ZERO_CROSSINGS 24
#define GRAIL_RESAMPLE_TABLE_MAX 32768
/* The outputs of one workgroup's stretch of a row.  Not part of the contract (no number depends on it): it is here so
 * that tests can aim at the seams. */
#define GRAIL_RESAMPLE_CHUNK 1024

/* Pure host: U, D and P of a pair of rates (any of the three may be NULL).  GRAIL_ERR_INVALID_ARG, nothing written: a
 * rate of 0, equal rates, U * P > GRAIL_RESAMPLE_TABLE_MAX. */
int grail_resample_ratio(uint32_t rate_in, uint32_t rate_out, uint32_t *up, uint32_t *down, uint32_t *taps);
/* Pure host: num[p * taps + k] = N((k - taps/2) U + p), up * taps numerators of 2^26.  GRAIL_ERR_INVALID_ARG, nothing
 * written: a pair grail_resample_ratio refuses, num NULL, cap < up * taps. */
int grail_resample_coefficients(uint32_t rate_in, uint32_t rate_out, int32_t *num, uint32_t cap);
/* Pure host: *n_out = ceil(n U / D), the length of a row of n samples resampled.  GRAIL_ERR_INVALID_ARG: a pair
 * grail_resample_ratio refuses, n_out NULL, a length that does not fit 64 bits. */
int grail_resample_len(uint64_t n, uint32_t rate_in, uint32_t rate_out, uint64_t *n_out);

/* The resampler above, queued on ctx's stream like grail_true_peak_async: rows_dev: device [n_rows][row_stride] (finished
 * tracks or rendered rows alike); len_dev: device [n_rows]; out_dev: device [n_rows][out_stride].  Results are DEVICE
 * arrays [n_rows], either may be NULL: out_len, nonfinite.  out_dev must not overlap rows_dev.  16-byte loads and stores
 * where both bases are 16-byte aligned and both strides multiples of 4, 4-byte ones otherwise: same bits.  One workgroup
 * takes GRAIL_RESAMPLE_CHUNK outputs of one row, so a lone long track fills the device.  The table of a pair of rates is
 * uploaded at its first use and the last four pairs' stay with the context, as does the scratch (4 bytes per row and 1024
 * outputs), grown and never shrunk, until grail_destroy.
 * GRAIL_ERR_INVALID_ARG, nothing queued: a pair grail_resample_ratio refuses; a NULL buffer with samples to read or
 * write; overlapping ranges; strides that allow a row of 2^32 outputs or more.  These come first; without a usable
 * device: GRAIL_ERR_NO_DEVICE.  n_rows = 0 is a success that queues nothing. */
int grail_resample_async(grail_ctx *ctx, const float *rows_dev, uint64_t row_stride, const uint32_t *len_dev, uint32_t n_rows,
                         uint32_t rate_in, uint32_t rate_out, float *out_dev, uint64_t out_stride,
                         uint32_t *out_len_dev, uint32_t *nonfinite_dev);

/* ---- levels, continued: FIR filtering --------------------------------------------------------------------------------------------
 * Every stage above shapes the sound in a fixed way; this one applies the filter the caller chose: a telephone band on
 * the tracks a lower rate produced, a high-pass under a voice, a de-emphasis curve, the first milliseconds of a room.  A
 * FIR filter, because time is parallel (a lone long track fills the device) and because the contract can be exact: a
 * binary32 tap times a binary32 sample has 48 significant bits and is exact in binary64, so a fused multiply-add and a
 * multiply followed by an add give the same bits (the argument of the true-peak section).  All arithmetic is IEEE binary64.
 * FILTER.  K taps h[0 .. K-1] in binary32 and an origin o: 1 <= K <= GRAIL_FIR_TAPS_MAX = 4096, 0 <= o <= K - 1, every
 * tap finite.  o is the tap that sits at time zero: o = 0 for a causal impulse response, o = (K - 1) / 2 for a
 * linear-phase design with zero delay.
 * SAMPLES.  For a row of n = min(len[u], row_stride) samples:
 *   - v[t] = (double)x[t] for 0 <= t < n and +0.0 outside; a sample that is not finite (|x| > FLT_MAX or NaN) is counted
 *     once and enters as +0.0; memory between n and row_stride is never looked at, whatever it holds.
 *   - n_out = 0 when n = 0, otherwise n_out = min(n + K - 1 - o, out_stride): the tail rings out.
 *   - For output m = 0 .. n_out - 1: acc = +0.0; for k = 0 .. K - 1 ascending acc = acc + (double)h[k] * v[m + o - k];
 *     y[m] = (float)acc, one rounding.  The result may be infinite and is not counted.
 *   - out between n_out and out_stride is never written.  out_len[u] = n_out; nonfinite[u] = the count over all n
 *     samples (also where out_stride cut the output short).
 * Nothing above depends on chunking, layout, alignment, the rows around or the launch: out and the results are a pure
 * function of the row's samples and its filter.  No float atomics.
 * h = [1.0] is NOT a copy: -0.0 and non-finite samples come back as +0.0 (acc starts at +0.0, and +0.0 + -0.0 = +0.0).
 * FILTER SETS.  A call filters rows with the filters of one set, chosen per row.  A set holds 1 <= F <=
 * GRAIL_FIR_FILTERS_MAX = 64 filters; filter_dev is a device array [n_rows] of indices into it, NULL means filter 0 for
 * every row.  A row whose index is >= F is refused the way the limiter refuses a ragged group: out_len[u] =
 * GRAIL_LIMIT_REFUSED = 0xFFFFFFFF, nonfinite[u] = 0, its out row unwritten.
 * DESIGN.  grail_fir_design makes a Kaiser-windowed band-pass of K taps, K odd, 3 <= K <= 4096, for 0 <= lo < hi <=
 * rate / 2.  With c = (K - 1) / 2, x = k - c, W = c + 1, beta = 8.0, f_l = lo / rate, f_h = hi / rate:
 *     h[k] = (float)( I0(beta * sqrt(1 - (x / W)^2)) / I0(beta) * (2 f_h sinc(2 f_h x) - 2 f_l sinc(2 f_l x)) )
 * sinc and I0 are the resampler's (above).  lo = 0 is a low-pass, hi = rate / 2 a high-pass; the origin to use is c.
 * The bits come from the C library's sin: the table as grail_fir_design returns it is the contract, as with
 * grail_kweighting.  With Kaiser's transition width df = (81.3 - 7.95) / (2.285 * 2 pi * (K - 1)) * rate the passband is
 * flat within 0.001 dB from lo + df to hi - df and the stopband at or below -80 dB outside lo - df .. hi + df.
 * NOT promised: the output's peak can exceed the input's: limit or measure after filtering, not before. */
#define GRAIL_FIR_TAPS_MAX 4096
#define GRAIL_FIR_FILTERS_MAX 64
/* The outputs of one workgroup's stretch of a row.  Not part of the contract (no number depends on it): it is here so
 * that tests can aim at the seams. */
#define GRAIL_FIR_CHUNK 2048
typedef struct grail_fir grail_fir; /* a set of filters, its taps resident in HBM */

/* Pure host: *n_out = 0 for n = 0, else n + n_taps - 1 - origin, the length of a row of n samples filtered.
 * GRAIL_ERR_INVALID_ARG, nothing written: n_taps outside 1 .. 4096, origin > n_taps - 1, n_out NULL, a length that does
 * not fit 64 bits. */
int grail_fir_len(uint64_t n, uint32_t n_taps, uint32_t origin, uint64_t *n_out);
/* Pure host: taps[0 .. n_taps - 1] of the band-pass lo_hz .. hi_hz at sample_rate (DESIGN above).
 * GRAIL_ERR_INVALID_ARG, nothing written: n_taps even or outside 3 .. 4096, sample_rate 0, not 0 <= lo_hz < hi_hz <=
 * sample_rate / 2, taps NULL. */
int grail_fir_design(uint32_t sample_rate, double lo_hz, double hi_hz, uint32_t n_taps, float *taps);

/* A set of n_filters filters on ctx's device: taps holds the filters' taps one after another (n_taps[0] of filter 0,
 * then n_taps[1] of filter 1, ...), n_taps and origin [n_filters].  The set keeps its own copy, as binary64, uploaded on
 * ctx's stream; the arrays may be reused at once.  GRAIL_ERR_INVALID_ARG, nothing created: a NULL argument, n_filters
 * outside 1 .. 64, an n_taps outside 1 .. 4096, an origin > n_taps - 1, a tap that is not finite.  These come first;
 * without a usable device: GRAIL_ERR_NO_DEVICE. */
int grail_fir_create(grail_ctx *ctx, const float *taps, const uint32_t *n_taps, const uint32_t *origin,
                     uint32_t n_filters, grail_fir **out);
/* Releases a set once everything queued on ctx's stream is through; sets still alive at grail_destroy go with the
 * context.  NULL is a no-op.  GRAIL_ERR_INVALID_ARG: a pointer that is not a live set of this context (another context's, or
 * one freed before: sets are looked up, not looked into). */
int grail_fir_free(grail_ctx *ctx, grail_fir *set);
/* The filter above, queued on ctx's stream like grail_resample_async: rows_dev: device [n_rows][row_stride] (finished
 * tracks or rendered rows alike); len_dev: device [n_rows]; filter_dev: device [n_rows] or NULL; out_dev: device
 * [n_rows][out_stride].  Results are DEVICE arrays [n_rows], either may be NULL: out_len, nonfinite.  out_dev must not
 * overlap rows_dev.  16-byte loads and stores where both bases are 16-byte aligned and both strides multiples of 4,
 * 4-byte ones otherwise: same bits.  One workgroup takes GRAIL_FIR_CHUNK outputs of one row, so a lone long track fills
 * the device.  The scratch (4 bytes per row and 2048 outputs) stays with the context, grown and never shrunk, until
 * grail_destroy.
 * GRAIL_ERR_INVALID_ARG, nothing queued: set NULL or of another context; a NULL buffer with samples to read or write;
 * overlapping ranges; strides that allow a row of 2^32 outputs or more; more than 2^31 chunks.  These come first;
 * without a usable device: GRAIL_ERR_NO_DEVICE.  n_rows = 0 is a success that queues nothing. */
int grail_fir_async(grail_ctx *ctx, const grail_fir *set, const float *rows_dev, uint64_t row_stride,
                    const uint32_t *len_dev, uint32_t n_rows, const uint32_t *filter_dev,
                    float *out_dev, uint64_t out_stride, uint32_t *out_len_dev, uint32_t *nonfinite_dev);

/* ---- levels, continued: FIR filtering of streams ---------------------------------------------------------------------------------
 * grail_fir_async takes finished rows.  A caller who pulls a live stream chunk by chunk (grail_stream_next_async) filters
 * chunk by chunk with a FILTER STREAM: n_rows independent rows, each bound to one filter (K taps, origin o) of a live set
 * when the stream is opened, their state resident in HBM between calls.
 * THE CONTRACT.  For any split of a row's samples into calls (calls of no samples included), the outputs of the `next`
 * calls put end to end, followed by the tail that `finish` writes, are bit for bit what grail_fir_async writes for the whole
 * row with an out_stride that cuts nothing; the sum of the calls' nonfinite counts is its count.  This is the promise
 * grail_stream_next_async makes for rendering.
 * STATE.  Per row: N, the samples fed so far (64 bits); whether the row has ended; the last K - 1 samples fed, in a ring of
 * the set's longest K - 1 samples rounded up to a power of two (at most 16 KB a row).
 * E(N) = max(0, N - o) outputs can be known after N samples (output m needs sample m + o).  A `next` call that feeds n
 * samples writes outputs E(N) .. E(N + n) - 1 (at most n of them; none while the row is short of its origin); `finish`
 * writes the tail E(N) .. N + K - 1 - o - 1, the samples to come being +0.0: K - 1 - o + min(N, o) outputs, at most K - 1,
 * none for a row that was fed nothing.
 * (The functions are named grail_filter_stream_*, not grail_fir_*: the latter are the calls on finished rows.) */
typedef struct grail_filter_stream grail_filter_stream;

/* Pure host: *n_out = the outputs a call writes for a row that was fed fed_before samples before it: finishing = 0: a
 * `next` call that feeds n samples; finishing != 0: `finish` (n must be 0).  GRAIL_ERR_INVALID_ARG, nothing written: as
 * grail_fir_len; finishing with n != 0. */
int grail_filter_stream_len(uint64_t fed_before, uint64_t n, uint32_t n_taps, uint32_t origin, int finishing, uint64_t *n_out);
/* A stream of n_rows rows on the filters of `set`: filter is a HOST array [n_rows] of indices into the set, NULL means
 * filter 0 for every row.  The state (a ring and one 64-bit word per row) belongs to the stream, which belongs to the
 * context.  GRAIL_ERR_INVALID_ARG, nothing created: ctx or out NULL; a set that is not a live set of this context;
 * n_rows = 0; an index >= the set's filter count (the array is on the host, so it is checked here: a stream has no refused
 * rows of this kind).  These come first; without a usable device: GRAIL_ERR_NO_DEVICE. */
int grail_filter_stream_open(grail_ctx *ctx, const grail_fir *set, uint32_t n_rows, const uint32_t *filter,
                             grail_filter_stream **out);
/* Feeds every row u its next n = min(in_len_dev[u], in_stride) samples from in_dev + u * in_stride and writes the
 * E(N + n) - E(N) outputs that became known to out_dev + u * out_stride, from index 0; queued on ctx's stream.  Results
 * are DEVICE arrays [n_rows], either may be NULL: out_len[u] = that count; nonfinite[u] = the samples among this call's n
 * that are not finite (a sample is counted in the call that fed it and never again; it enters as +0.0).  n = 0 is legal (a
 * paused row): nothing is written, out_len 0.  A row that has ended and is fed n > 0 is refused as grail_fir_async refuses a
 * row: out_len = GRAIL_LIMIT_REFUSED, nonfinite 0, nothing written, its state as it was.  out_dev past out_len is never
 * written.  in_dev may be reused by whatever is queued behind the call: the call copies what it keeps.  16-byte loads and
 * stores where both bases are 16-byte aligned and both strides multiples of 4, 4-byte ones otherwise: same bits.
 * GRAIL_ERR_INVALID_ARG, nothing queued: a stream that is not an open stream of this context (looked up, not looked
 * into); a NULL buffer with samples to read or write, in_len_dev NULL; out_stride < in_stride (a stream never cuts outputs
 * short); overlapping ranges; more than 2^31 chunks of GRAIL_FIR_CHUNK outputs.  These come first; without a usable
 * device: GRAIL_ERR_NO_DEVICE. */
int grail_filter_stream_next_async(grail_ctx *ctx, grail_filter_stream *fs, const float *in_dev, uint64_t in_stride,
                                   const uint32_t *in_len_dev, float *out_dev, uint64_t out_stride,
                                   uint32_t *out_len_dev, uint32_t *nonfinite_dev);
/* Rings out the rows marked in which (a HOST array [n_rows] of bytes, non-zero = marked; NULL = every row, as
 * grail_stream_finish): a marked row that has not ended writes its tail to out_dev + u * out_stride and ends.  out_len
 * (device [n_rows], may be NULL): the tail's length; 0, and nothing written, for unmarked rows and rows that had ended
 * before.  The array may be reused at once.  GRAIL_ERR_INVALID_ARG, nothing queued: a stream that is not an open stream of
 * this context; out_stride below the set's longest K - 1; out_dev NULL with a tail to write. */
int grail_filter_stream_finish_async(grail_ctx *ctx, grail_filter_stream *fs, const uint8_t *which, float *out_dev,
                                     uint64_t out_stride, uint32_t *out_len_dev);
/* Releases a stream once everything queued on ctx's stream is through; streams still open at grail_destroy go with the
 * context.  NULL is a no-op.  GRAIL_ERR_INVALID_ARG: not an open stream of this context.  While a set has open streams,
 * grail_fir_free of it returns GRAIL_ERR_INVALID_ARG and frees nothing. */
int grail_filter_stream_close(grail_ctx *ctx, grail_filter_stream *fs);

/* ---- levels, continued: sample-rate conversion of streams ------------------------------------------------------------------------
 * grail_resample_async takes finished rows.  A caller who pulls a live stream chunk by chunk and needs another rate (10 ms
 * chunks at 48 000 for a telephone path at 8 000) resamples chunk by chunk with a RESAMPLE STREAM: n_rows independent rows,
 * all on one pair of rates fixed when the stream is opened, their state resident in HBM between calls.  U, D, P and the
 * table C are those of the one-shot section for the pair; h = P / 2.
 * THE CONTRACT.  For any split of a row's samples into calls (calls of no samples included), the outputs of the `next`
 * calls put end to end, followed by the tail that `finish` writes, are bit for bit what grail_resample_async writes for the
 * whole row with an out_stride that cuts nothing; the sum of the calls' nonfinite counts is its count.
 * One-shot output m reads the samples i0 - h + 1 .. i0 + h with i0 = floor(m D / U), so after N samples the outputs known
 * are E(N) = 0 for N <= h, else ceil((N - h) U / D).
 * STATE.  Per row: N, the samples fed so far (64 bits); whether the row has ended; the last P - 1 samples fed, already +0.0
 * where they were not finite, in a ring of P - 1 samples rounded up to a power of two (at most 4 KB a row for the eight rates
 * listed above, 128 KB at the table limit).
 * A `next` call that feeds n samples writes outputs E(N) .. E(N + n) - 1 of the one-shot contract applied to everything fed
 * so far (at most ceil(n U / D) of them; none while the row is short of h + 1 samples); `finish` writes the tail E(N) ..
 * ceil(N U / D) - 1, the samples to come being +0.0: at most ceil(h U / D) outputs, none for a row that was fed nothing.
 * A stream never cuts outputs short: out_stride is at least the most a call can write. */
typedef struct grail_resample_stream grail_resample_stream;

/* Pure host, 128-bit inside: *n_out = the outputs a call writes for a row that was fed fed_before samples before it:
 * finishing = 0: a `next` call that feeds n samples; finishing != 0: `finish` (n must be 0).  GRAIL_ERR_INVALID_ARG,
 * nothing written: a pair grail_resample_ratio refuses; n_out NULL; finishing with n != 0; fed_before + n or the count
 * does not fit 64 bits. */
int grail_resample_stream_len(uint64_t fed_before, uint64_t n, uint32_t rate_in, uint32_t rate_out, int finishing,
                              uint64_t *n_out);
/* A stream of n_rows rows from rate_in to rate_out.  The state (a ring, N, and the next output's place per row) and a copy
 * of the pair's table belong to the stream, which belongs to the context: the stream does not depend on the four tables
 * grail_resample_async keeps.  GRAIL_ERR_INVALID_ARG, nothing created: ctx or out NULL; a pair grail_resample_ratio
 * refuses; n_rows = 0.  These come first; without a usable device: GRAIL_ERR_NO_DEVICE. */
int grail_resample_stream_open(grail_ctx *ctx, uint32_t rate_in, uint32_t rate_out, uint32_t n_rows,
                               grail_resample_stream **out);
/* Feeds every row u its next n = min(in_len_dev[u], in_stride) samples from in_dev + u * in_stride and writes the
 * E(N + n) - E(N) outputs that became known to out_dev + u * out_stride, from index 0; queued on ctx's stream.  Results
 * are DEVICE arrays [n_rows], either may be NULL: out_len[u] = that count; nonfinite[u] = the samples among this call's n
 * that are not finite (a sample is counted in the call that fed it and never again; it enters as +0.0).  n = 0 is legal (a
 * paused row): nothing is written, out_len 0.  A row that has ended and is fed n > 0 is refused: out_len =
 * GRAIL_LIMIT_REFUSED, nonfinite 0, nothing written, its state as it was.  out_dev past out_len is never written.  in_dev
 * may be reused by whatever is queued behind the call: the call copies what it keeps.  16-byte loads and stores where both
 * bases are 16-byte aligned and both strides multiples of 4, 4-byte ones otherwise: same bits.
 * GRAIL_ERR_INVALID_ARG, nothing queued: a stream that is not an open stream of this context (looked up, not looked
 * into); a NULL buffer with samples to read or write, in_len_dev NULL; out_stride < ceil(in_stride U / D) =
 * grail_resample_len(in_stride); overlapping ranges; an in_stride that allows 2^32 outputs or more in a call; more than 2^31
 * chunks of GRAIL_RESAMPLE_CHUNK outputs.  These come first; without a usable device: GRAIL_ERR_NO_DEVICE. */
int grail_resample_stream_next_async(grail_ctx *ctx, grail_resample_stream *rs, const float *in_dev, uint64_t in_stride,
                                     const uint32_t *in_len_dev, float *out_dev, uint64_t out_stride,
                                     uint32_t *out_len_dev, uint32_t *nonfinite_dev);
/* Flushes the rows marked in which (a HOST array [n_rows] of bytes, non-zero = marked; NULL = every row, as
 * grail_filter_stream_finish_async): a marked row that has not ended writes its tail to out_dev + u * out_stride and ends.
 * out_len (device [n_rows], may be NULL): the tail's length; 0, and nothing written, for unmarked rows and rows that had
 * ended before.  The array may be reused at once.  GRAIL_ERR_INVALID_ARG, nothing queued: a stream that is not an open
 * stream of this context; out_stride < ceil(h U / D); out_dev NULL. */
int grail_resample_stream_finish_async(grail_ctx *ctx, grail_resample_stream *rs, const uint8_t *which, float *out_dev,
                                       uint64_t out_stride, uint32_t *out_len_dev);
/* Releases a stream once everything queued on ctx's stream is through; streams still open at grail_destroy go with the
 * context.  NULL is a no-op.  GRAIL_ERR_INVALID_ARG: not an open stream of this context. */
int grail_resample_stream_close(grail_ctx *ctx, grail_resample_stream *rs);

/* ---- levels, continued: the limiter on streams -----------------------------------------------------------------------------------
 * grail_limit_async takes finished rows.  Live voices summed into a track overlap above the ceiling, and a band-pass
 * overshoots its input: a caller who pulls a live stream chunk by chunk limits chunk by chunk with a LIMIT STREAM: n_rows rows
 * in groups of `group` consecutive rows that share one gain curve, as in grail_limit_async; c = ceiling and l =
 * lookahead_log2 (L = 2^l) fixed when the stream is opened, its state resident in HBM between calls.
 * THE CONTRACT.  For any split of a group's samples into calls (calls of no samples included), the rows the `next` calls
 * write put end to end, followed by the tail that `finish` writes, are bit for bit what grail_limit_async writes for the whole
 * group with the same c, l and group and an out_stride that cuts nothing.  Over all calls and the finish the per-call results
 * combine to the one-shot call's: the minimum of the min_gain values is its min_gain, the sum of the n_limited values its
 * n_limited, the sum of the nonfinite values its nonfinite.  This holds because every step of the limiter's contract is FIR (a
 * 12-tap detector, a minimum over L, a sum of L integers): a prefix of the output is final after a prefix of the input.
 * With LAMBDA = L + 10 = GRAIL_LIMIT_STREAM_DELAY(l): z[t] needs q up to t + L - 1 and q[s] needs x up to s + 11, so after N
 * samples E(N) = max(0, N - LAMBDA) outputs are known, and output N - LAMBDA does change with the next sample.  A `next` call
 * that feeds n samples writes outputs E(N) .. E(N + n) - 1 (at most n of them; none while the group is short of LAMBDA + 1
 * samples); `finish` writes the tail E(N) .. N - 1: min(N, LAMBDA) outputs, none for a group that was fed nothing.  At
 * `finish` the one-shot rule for the row's end applies: q[s] = Q for s >= N, and the samples to come enter the detector as
 * +0.0.  Fed zeros are NOT the row's end to the detector: after the last sample the e's are not zero (the filter rings on
 * for eleven outputs), and a fed zero gets their q where the row's end gets Q.  The outputs below N cannot tell, though: such a
 * q sees only e's that q[N - 1] sees as well, so it is never below q[N - 1], and every window that reaches past the end
 * holds q[N - 1].  `finish` is the row's end without LAMBDA samples fed and counted, and it ends the group.
 * The output lags the input by LAMBDA samples: 266 samples (5.5 ms) at l = 8 and 48 kHz.
 * STATE.  Per group: N, the samples fed so far (64 bits); whether the group has ended.  Per row: the last 3 L + 19 samples
 * fed (the oldest sample the next output may still need is x[N - 3 L - 19]), already +0.0 where they were not finite, in a
 * ring rounded up to a power of two (at most 16 KB a row, at l = 10).
 * A stream never cuts outputs short: out_stride is at least the most a call can write. */
#define GRAIL_LIMIT_STREAM_DELAY(l) ((1u << (l)) + 10u)
typedef struct grail_limit_stream grail_limit_stream;

/* Pure host: *n_out = the outputs a call writes for a group that was fed fed_before samples before it: finishing = 0: a
 * `next` call that feeds n samples; finishing != 0: `finish` (n must be 0).  GRAIL_ERR_INVALID_ARG, nothing written:
 * lookahead_log2 > 10; n_out NULL; finishing with n != 0; fed_before + n does not fit 64 bits. */
int grail_limit_stream_len(uint64_t fed_before, uint64_t n, uint32_t lookahead_log2, int finishing, uint64_t *n_out);
/* A stream of n_rows rows in groups of `group`, held under `ceiling` with a look-ahead of 2^lookahead_log2 samples.  The
 * state (one 64-bit word per group, a ring per row) belongs to the stream, which belongs to the context.
 * GRAIL_ERR_INVALID_ARG, nothing created: what grail_limit_async refuses (lookahead_log2 > 10; group 0 or no divisor of
 * n_rows; a ceiling that is not a finite number above 0); n_rows = 0; ctx or out NULL.  These come first; without a usable
 * device: GRAIL_ERR_NO_DEVICE. */
int grail_limit_stream_open(grail_ctx *ctx, uint32_t n_rows, uint32_t group, float ceiling, uint32_t lookahead_log2,
                            grail_limit_stream **out);
/* Feeds every row u its next n = min(in_len_dev[u], in_stride) samples from in_dev + u * in_stride and writes the
 * E(N + n) - E(N) outputs that became known to out_dev + u * out_stride, from index 0; queued on ctx's stream.  in_len_dev:
 * device [n_rows].  Results are DEVICE arrays [n_rows / group], any may be NULL: out_len = that count; min_gain = the smallest
 * g among the outputs this call wrote, 1.0f if it wrote none; n_limited counts among the outputs this call wrote; nonfinite
 * counts among the samples this call fed, summed over the members (a sample is counted in the call that fed it and never
 * again; it enters as +0.0).  n = 0 is legal (a paused group): nothing is written, out_len 0.  A group whose members are fed
 * different n in one call is REFUSED for that call: out_len = GRAIL_LIMIT_REFUSED, min_gain = NaN, both counts 0, nothing
 * written, its state as it was; a correct call may follow it.  A group that has ended and is fed n > 0 is refused in the same
 * way.  out_dev past out_len is never written.  in_dev may be reused by whatever is queued behind the call: the call copies
 * what it keeps.  16-byte loads and stores where both bases are 16-byte aligned and both strides multiples of 4, 4-byte ones
 * otherwise: same bits.  Scratch stays with the context, as for grail_limit_async.
 * GRAIL_ERR_INVALID_ARG, nothing queued: a stream that is not an open stream of this context (looked up, not looked into);
 * a NULL buffer with samples to read or write, in_len_dev NULL; out_stride < in_stride (a stream never cuts outputs short);
 * overlapping ranges; more than 2^31 chunks of GRAIL_LIMIT_CHUNK outputs.  These come first; without a usable device:
 * GRAIL_ERR_NO_DEVICE. */
int grail_limit_stream_next_async(grail_ctx *ctx, grail_limit_stream *ls, const float *in_dev, uint64_t in_stride,
                                  const uint32_t *in_len_dev, float *out_dev, uint64_t out_stride, uint32_t *out_len_dev,
                                  float *min_gain_dev, uint32_t *n_limited_dev, uint32_t *nonfinite_dev);
/* Ends the groups marked in which (a HOST array [n_rows / group] of bytes, non-zero = marked; NULL = every group, as
 * grail_filter_stream_finish_async): every member of a marked group that has not ended writes its tail to out_dev + u *
 * out_stride, and the group ends.  Results are DEVICE arrays [n_rows / group], any may be NULL: out_len = the tail's length,
 * min_gain and n_limited among the tail's outputs; 0, 1.0f, 0 and nothing written for groups that are unmarked or had
 * ended before.  The array may be reused at once.  GRAIL_ERR_INVALID_ARG, nothing queued: a stream that is not an open
 * stream of this context; out_stride < GRAIL_LIMIT_STREAM_DELAY(l); out_dev NULL. */
int grail_limit_stream_finish_async(grail_ctx *ctx, grail_limit_stream *ls, const uint8_t *which, float *out_dev,
                                    uint64_t out_stride, uint32_t *out_len_dev, float *min_gain_dev, uint32_t *n_limited_dev);
/* Releases a stream once everything queued on ctx's stream is through; streams still open at grail_destroy go with the
 * context.  NULL is a no-op.  GRAIL_ERR_INVALID_ARG: not an open stream of this context. */
int grail_limit_stream_close(grail_ctx *ctx, grail_limit_stream *ls);

/* ---- levels, continued: the meters on streams ------------------------------------------------------------------------------------
 * grail_loudness_async and grail_true_peak_async take finished rows.  A caller who pulls a live stream chunk by chunk, and
 * filters, resamples and limits it chunk by chunk, meters it chunk by chunk with a METER STREAM: n_rows independent rows, the
 * sample rate, the ten K-weighting coefficients and a hop capacity fixed when the stream is opened, its state resident in HBM
 * between calls.  H = sample_rate / 10; rates are limited as for grail_loudness_async.
 * STATE.  Per row: N, the samples fed so far (64 bits, bit 63: the row has ended); s1 .. s4 and acc of the loudness
 * recurrence; the running true peak; the hops completed; the last 11 samples fed, already +0.0 where they were not finite, in
 * a ring of 16 floats; a ledger of the row's hop sums, double [max_hops], in HBM.  Every double crosses a call as its 64 bits:
 * nothing is recomputed, rounded or flushed on the way.
 * THE CONTRACT, for any split of a row's samples into calls, calls of no samples included:
 *   - The hop sums the `next` calls write, put end to end, are bit for bit the hop_sumsq grail_loudness_async writes for the
 *     whole row with the same coefficients and rate, and they are the ledger's first floor(N / H) entries.
 *   - The true_peak of a `next` call is the largest |y[p][t]| (the true-peak section's y) over the call's own output times
 *     t = N .. N + n - 1, +0.0 for n = 0; that of `finish` is the largest over the eleven outputs t = N .. N + 10, the samples
 *     to come being +0.0.  The maximum of all these values is grail_true_peak_async's number for the whole row, bit for bit
 *     (a row [0, ..., 0, 1.0] whose 1.0 is a call's last sample: the calls read at most 239 / 8192, `finish` 7964 / 8192).
 *   - The sum of the calls' nonfinite counts is either one-shot call's count: a sample is counted in the call that fed it and
 *     enters both meters as +0.0.
 *   - `read`, at any moment, gives for each row what the one-shot calls give for a row that holds exactly the N samples fed so
 *     far: integrated_ms, grail_loudness_async's gated mean square over the ledger's hops (+0.0 below four hops);
 *     momentary_ms = (((h[j] + h[j+1]) + h[j+2]) + h[j+3]) / (4.0 * H) at j = hops - 4, the gate's last z_j (+0.0 below four
 *     hops); short_term_ms = the left fold of the last 30 hops from the oldest, divided by (30.0 * H), the last block of
 *     grail_loudness_window_max(..., 30) (+0.0 below 30 hops); true_peak, the running maximum (before `finish` it lacks the
 *     eleven outputs after the row's last sample; after it, it is the one-shot number); hops, the count of hops completed.
 *   - REFUSED for that call, as in the other kinds: a row that has ended and is fed n > 0, and a row that the call would carry
 *     past max_hops completed hops: n_hops = GRAIL_LIMIT_REFUSED, true_peak = NaN, nonfinite = 0, nothing written, its state as
 *     it was; a correct call may follow.
 * One lane filters one row's chunk (the recurrence is serial), 64 rows to a wavefront; a wavefront whose rows all stand at the
 * same place in their hops and are fed the same n takes the one-shot kernel's walk, any other a walk with a test a sample:
 * same bits.  The true peak of a call is parallel in time.  Measured on an MI355X: 65 536 rows of 96 006 samples fed whole in
 * one call, the hops in 7.3 ms where grail_loudness_async's take 7.4 - 7.6 (10.8 against 11.3 ms right behind a call's
 * true peak, which takes 16 ms); 4 096 rows fed 480 samples: 0.07 ms a call, 0.03 ms a read. */
typedef struct grail_meter_stream grail_meter_stream;

/* Pure host: *n_hops = the hops a `next` call completes for a row that was fed fed_before samples before it and is fed n:
 * (fed_before + n) / H - fed_before / H.  GRAIL_ERR_INVALID_ARG, nothing written: a rate outside GRAIL_LOUDNESS_RATE_MIN ..
 * GRAIL_LOUDNESS_RATE_MAX; n_hops NULL; fed_before + n does not fit 64 bits. */
int grail_meter_stream_hops(uint64_t fed_before, uint64_t n, uint32_t sample_rate, uint64_t *n_hops);
/* A stream of n_rows rows metered at sample_rate.  coef: HOST [10], copied before the call returns; NULL =
 * grail_kweighting(sample_rate).  max_hops: the hops a row's ledger holds (8 bytes each); a row is never carried past it.  The
 * state belongs to the stream, which belongs to the context.  GRAIL_ERR_INVALID_ARG, nothing created: a rate out of range;
 * n_rows = 0; max_hops = 0, or n_rows x max_hops x 8 does not fit size_t; ctx or out NULL.  These come first; without a
 * usable device: GRAIL_ERR_NO_DEVICE.  GRAIL_ERR_OUT_OF_MEMORY: the device refuses the ledger. */
int grail_meter_stream_open(grail_ctx *ctx, uint32_t n_rows, uint32_t sample_rate, const double *coef, uint64_t max_hops,
                            grail_meter_stream **out);
/* Feeds every row u its next n = min(in_len_dev[u], in_stride) samples from in_dev + u * in_stride; queued on ctx's stream.
 * in_len_dev: device [n_rows].  hop_sumsq_dev: DEVICE double [n_rows][hops_stride], the hops the call completes from index 0,
 * entries past n_hops never written; hops_stride >= (in_stride + H - 1) / H, the most hops a call can complete.  n_hops_dev,
 * true_peak_dev (double), nonfinite_dev: DEVICE arrays [n_rows].  All four may be NULL; the ledger is kept either way.  n = 0
 * is legal (a paused row): 0, +0.0, 0.  in_dev may be reused by whatever is queued behind the call: the call copies what it
 * keeps.  16-byte loads where in_dev is 16-byte aligned and in_stride a multiple of 4, 4-byte loads otherwise: same bits.
 * The chunks' maxima go through scratch that stays with the context (12 bytes per 4096 samples of n_rows x in_stride).
 * GRAIL_ERR_INVALID_ARG, nothing queued: a stream that is not an open stream of this context (looked up, not looked into); a
 * NULL in_dev with samples to read, in_len_dev NULL; hop_sumsq_dev with a hops_stride below the rule; rows that span more
 * than 2^60 samples; more than 2^31 chunks of 4096 output times.  These come first; without a usable device:
 * GRAIL_ERR_NO_DEVICE. */
int grail_meter_stream_next_async(grail_ctx *ctx, grail_meter_stream *ms, const float *in_dev, uint64_t in_stride,
                                  const uint32_t *in_len_dev, double *hop_sumsq_dev, uint64_t hops_stride, uint32_t *n_hops_dev,
                                  double *true_peak_dev, uint32_t *nonfinite_dev);
/* What the meter shows of every row now (THE CONTRACT, `read`), queued on ctx's stream: DEVICE arrays [n_rows], four of
 * double and hops_dev of uint64, any may be NULL.  It changes no state.  GRAIL_ERR_INVALID_ARG: not an open stream of this
 * context. */
int grail_meter_stream_read_async(grail_ctx *ctx, grail_meter_stream *ms, double *integrated_ms_dev, double *momentary_ms_dev,
                                  double *short_term_ms_dev, double *true_peak_dev, uint64_t *hops_dev);
/* The ledger's device address: row u's hop sums are (*hops_dev)[u * *stride + h], h below the row's hops; *stride = max_hops.
 * It stays valid until the stream is closed; the stream's calls write it on ctx's stream.  A caller copies a track's hops from
 * it for grail_loudness_range and grail_loudness_window_max.  GRAIL_ERR_INVALID_ARG: not an open stream of this context; a
 * NULL argument. */
int grail_meter_stream_ledger(grail_ctx *ctx, grail_meter_stream *ms, const double **hops_dev, uint64_t *stride);
/* Ends the rows marked in which (a HOST array [n_rows] of bytes, non-zero = marked; NULL = every row; the array may be reused
 * at once): the true-peak filter rings out over the eleven outputs after the row's last sample.  true_peak_dev: DEVICE double
 * [n_rows], may be NULL: the largest of those eleven, +0.0 for rows that are unmarked or had ended before.  The running
 * peak takes it in.  GRAIL_ERR_INVALID_ARG, nothing queued: not an open stream of this context. */
int grail_meter_stream_finish_async(grail_ctx *ctx, grail_meter_stream *ms, const uint8_t *which, double *true_peak_dev);
/* Releases a stream once everything queued on ctx's stream is through; streams still open at grail_destroy go with the
 * context.  NULL is a no-op.  GRAIL_ERR_INVALID_ARG: not an open stream of this context. */
int grail_meter_stream_close(grail_ctx *ctx, grail_meter_stream *ms);

/* ---- levels, continued: recursive filtering --------------------------------------------------------------------------------------
 * What is done to a voice between render and mix is mostly recursive: a high-pass under it, a presence peak, a shelf, a
 * notch, de-emphasis, a DC blocker, a resonance that rings out.  A FIR of 4 096 taps approximates a 100 Hz high-pass badly
 * at thousands of operations a sample; a biquad costs nine.  This is the K-weighting recurrence of the loudness section with
 * the caller's coefficients, and it writes samples.
 * ARITHMETIC.  All of it IEEE binary64, every operation rounded by itself (no fused multiply-add anywhere), evaluated in
 * the order written; denormals are not flushed.  The numbers are a pure function of the row's samples, its filter and the
 * call's tail: not of row_stride, out_stride beyond where it cuts, the row's index, the rows around it, the other filters
 * of the set, alignment, the device or the launch.  No atomics.
 * FILTER.  S sections in series, 1 <= S <= GRAIL_IIR_SECTIONS_MAX = 8, each five binary64 numbers b0 b1 b2 a1 a2, all
 * finite.  Stability is not checked: a filter with poles outside the unit circle overflows, and says so in its output.
 * SET.  1 <= F <= GRAIL_IIR_FILTERS_MAX = 64 filters, each with its own S.
 * ROW.  For a row of n = min(len[u], row_stride) samples and the call's `tail`:
 *   - n_out = 0 when n = 0, otherwise min(n + tail, out_stride).
 *   - The 2 S states s1[j] = s2[j] = +0.0 at the row's first sample.  For t = 0 .. n_out - 1 in ascending order:
 *         v = (double)x[t] for t < n, +0.0 for t >= n   (a sample that is not finite is counted once and enters as +0.0)
 *         for j = 0 .. S - 1 ascending:
 *             y = b0*v + s1;   s1 = (b1*v - a1*y) + s2;   s2 = b2*v - a2*y;   v = y       (transposed direct form II)
 *         out[t] = (float)v                             (one rounding; nothing is rounded to binary32 between sections)
 *   - The result may be infinite or NaN and is not counted; where it is NaN, which NaN is not promised.  Everything else is
 *     bit-exact.  out between n_out and out_stride is never written.  out_len[u] = n_out; nonfinite[u] is the count over all
 *     n samples (also where out_stride cut the output short).  Memory between n and row_stride enters no result, whatever it holds.
 * PER-ROW FILTER.  filter_dev is a device array [n_rows] of indices into the set, NULL means filter 0 for every row, as in
 * grail_fir_async.  A row whose index is >= F is refused: out_len[u] = GRAIL_LIMIT_REFUSED, nonfinite[u] = 0, its out row
 * unwritten.
 * IDENTITY IS NOT A COPY.  b0 = 1 with b1 = b2 = a1 = a2 = 0 gives y = 1*v + s1 with s1 = +0.0 at first: a row's first
 * -0.0 comes back as +0.0, as with h = [1.0] in FIR filtering (later ones may or may not: 0*v - 0*y can leave -0.0 in the
 * state).  So a filter of S sections is never computed as eight sections padded with identities, and a
 * row's result depends neither on the other filters of the set nor on the rows that share its wavefront.
 * DESIGN.  grail_iir_design returns one section.  With pi = 3.141592653589793, K = tan(pi * f0 / rate), KQ = K / Q,
 * KK = K * K, D = (1 + KQ) + KK, and for the kinds with a gain G in dB: V = 10^(G / 20) = pow(10, G / 20), W = sqrt(V):
 *     every kind but a PEAK that cuts:   a1 = 2 * (KK - 1) / D,   a2 = ((1 - KQ) + KK) / D,   and b0 b1 b2 =
 *     GRAIL_IIR_LOWPASS     KK / D,                       2 * KK / D,             KK / D
 *     GRAIL_IIR_HIGHPASS    1 / D,                        -2 / D,                 1 / D
 *     GRAIL_IIR_BANDPASS    KQ / D,                       0,                      -KQ / D             (peak gain 1 at f0)
 *     GRAIL_IIR_NOTCH       (1 + KK) / D,                 2 * (KK - 1) / D,       (1 + KK) / D
 *     GRAIL_IIR_HIGHSHELF   ((V + W*KQ) + KK) / D,        2 * (KK - V) / D,       ((V - W*KQ) + KK) / D   (the K-weighting shelf's form)
 *     GRAIL_IIR_LOWSHELF    ((1 + W*KQ) + V*KK) / D,      2 * (V*KK - 1) / D,     ((1 - W*KQ) + V*KK) / D
 *     GRAIL_IIR_PEAK, G >= 0, V = 10^(G / 20):  ((1 + V*KQ) + KK) / D,   2 * (KK - 1) / D,   ((1 - V*KQ) + KK) / D
 *     GRAIL_IIR_PEAK, G < 0, V = 10^(-G / 20), E = (1 + V*KQ) + KK:  numerator and denominator change places,
 *         b = D / E,  2 * (KK - 1) / E,  ((1 - KQ) + KK) / E;   a1 = 2 * (KK - 1) / E,   a2 = ((1 - V*KQ) + KK) / E
 * G is read by the shelves and the peak only.  The bits of tan, pow and sqrt are the C library's: the table as
 * grail_iir_design returns it is the contract, as with grail_kweighting.  A Butterworth low-pass or high-pass of order 2m
 * is m sections of that kind at the same f0 with Q_k = 1 / (2 cos(pi (2k + 1) / (4m))), k = 0 .. m - 1.
 * A LONE LONG ROW is one lane's serial work, as in grail_loudness_async: many rows fill the device.  A form parallel in time
 * is another contract (its order of operations differs): grail_biquad_blocked_async, "recursive filtering, parallel in time" below.
 * WHICH CALL FOR WHAT: grail_iir_async for many rows (thousands of rendered utterances), grail_biquad_blocked_async for a few
 * long ones (the tracks of a mix).
 * NOT promised: the output's peak can exceed the input's: limit or measure after filtering, not before. */
#define GRAIL_IIR_SECTIONS_MAX 8
#define GRAIL_IIR_FILTERS_MAX 64
#define GRAIL_IIR_LOWPASS   0
#define GRAIL_IIR_HIGHPASS  1
#define GRAIL_IIR_BANDPASS  2
#define GRAIL_IIR_NOTCH     3
#define GRAIL_IIR_PEAK      4
#define GRAIL_IIR_LOWSHELF  5
#define GRAIL_IIR_HIGHSHELF 6
typedef struct grail_iir grail_iir; /* a set of recursive filters, its coefficients resident in HBM */

/* Pure host: coef[0 .. 4] = b0 b1 b2 a1 a2 of one section (DESIGN above).  GRAIL_ERR_INVALID_ARG, nothing written: an
 * unknown kind, sample_rate 0, f0_hz not inside (0, sample_rate / 2), q not a finite number above 0, a gain_db that is not
 * finite, coef NULL, a section whose five numbers are not all finite (f0 next to half the rate, a gain of thousands of dB). */
int grail_iir_design(int kind, uint32_t sample_rate, double f0_hz, double q, double gain_db, double coef[5]);

/* A set of n_filters filters on ctx's device: coef holds the sections of filter 0, then of filter 1, and so on, five
 * doubles each; n_sections [n_filters].  The set keeps its own copy, uploaded on ctx's stream; the arrays may be reused at
 * once.  GRAIL_ERR_INVALID_ARG, nothing created: a NULL argument, n_filters outside 1 .. 64, an n_sections outside 1 .. 8,
 * a coefficient that is not finite.  These come first; without a usable device: GRAIL_ERR_NO_DEVICE. */
int grail_iir_create(grail_ctx *ctx, const double *coef, const uint32_t *n_sections, uint32_t n_filters, grail_iir **out);
/* Releases a set once everything queued on ctx's stream is through; sets still alive at grail_destroy go with the
 * context.  NULL is a no-op.  GRAIL_ERR_INVALID_ARG: a pointer that is not a live set of this context (sets are looked up,
 * not looked into); a set that still has open streams. */
int grail_iir_free(grail_ctx *ctx, grail_iir *set);
/* The filter above, queued on ctx's stream like grail_fir_async: rows_dev: device [n_rows][row_stride]; len_dev: device
 * [n_rows]; filter_dev: device [n_rows] or NULL; out_dev: device [n_rows][out_stride] (out_stride = 0: the lengths and
 * counts only).  Results are DEVICE arrays [n_rows], either may be NULL: out_len, nonfinite.  out_dev must not overlap
 * rows_dev.  16-byte loads and stores where both bases are 16-byte aligned and both strides multiples of 4, 4-byte ones
 * otherwise: same bits.  One lane filters one row, 64 rows to a wavefront (A LONE LONG ROW above).
 * GRAIL_ERR_INVALID_ARG, nothing queued: set NULL or of another context; a NULL buffer with samples to read or write;
 * overlapping ranges; strides that allow a row of 2^32 outputs or more.  These come first; without a usable device:
 * GRAIL_ERR_NO_DEVICE.  n_rows = 0 is a success that queues nothing. */
int grail_iir_async(grail_ctx *ctx, const grail_iir *set, const float *rows_dev, uint64_t row_stride,
                    const uint32_t *len_dev, uint32_t n_rows, const uint32_t *filter_dev, uint32_t tail,
                    float *out_dev, uint64_t out_stride, uint32_t *out_len_dev, uint32_t *nonfinite_dev);

/* ---- levels, continued: recursive filtering, parallel in time ----------------------------------------------------------------------
 * grail_iir_async gives a row to one lane.  The few long tracks of a mix leave the device idle that way: grail_biquad_blocked_async
 * cuts a row's steps into blocks of B = GRAIL_BIQUAD_BLOCK = 1024 and gives every block a lane.  Warming a block up would not do:
 * a caller's notch at Q = 30 or a high-pass at 20 Hz does not decay in any fixed number of samples.  This form is exact in
 * exact arithmetic for any coefficients; in binary64 it is a contract of its own, because its order of operations differs.
 * A row's n, its steps (its outputs, and its samples where out_stride cut the outputs short), n_out, the non-finite count,
 * the refused rows, `tail` and the cut by out_stride are exactly grail_iir_async's.  The row's inputs are its samples as
 * binary64, +0.0 for those that are not finite and +0.0 past n.  The 2 S states of a filter are ordered s1[0], s2[0], s1[1],
 * s2[1], ...; "the recurrence" is the one above, operation for operation, every operation rounded by itself.
 *   1. MATRIX.  T[i][c] is state i after B steps of the recurrence on +0.0 input from the state that is 1.0 in place c and
 *      +0.0 elsewhere: a function of the filter only, returned by grail_biquad_block_matrix.
 *   2. REST PASS.  Block k covers the steps [k B, (k + 1) B) of the row.  For every block that is not the row's last, z_k is
 *      the state after the block's B inputs through the recurrence from the state that is +0.0 in every place.
 *   3. ENTRY STATES.  e_0 = +0.0 in every place.  For k >= 0 and m = 2 (i / 2) + 1:
 *          e_{k+1}[i] = (...((T[i][0]*e_k[0] + T[i][1]*e_k[1]) + T[i][2]*e_k[2]) ... + T[i][m]*e_k[m]) + z_k[i]
 *      over the states of i's own section and of the sections before it (the others cannot reach it), ascending, one
 *      product and one addition each, each rounded by itself, nothing fused; z_k[i] is added last.
 *   4. OUTPUT PASS.  Block k's outputs are the recurrence from the state e_k over the block's steps, with the one rounding to
 *      binary32 at the end.  No block is stepped past the row's last step.
 * SO: a row of at most B steps is bit for bit grail_iir_async's row, and so are the first B outputs of every row.  From
 * output B on the two calls differ by the rounding of (3): within 1e-9 of the row's peak before the rounding to binary32 for
 * the filters of DESIGN.md §4.22, where they differed by 2e-11 at most.  A row's result depends on its samples, its filter
 * and the call's tail: not on the other rows, the other filters of the set, alignment, the device or the launch.  No atomics.
 * WHICH CALL FOR WHAT: this one for a few long rows (it is the faster of the two while the rows are too few to fill the
 * device with one lane each), grail_iir_async for many rows: this call runs the recurrence twice and holds scratch of
 * 16 S' bytes a block (S' the set's largest S rounded up to 1, 2, 4 or 8).  Streams have no blocked form. */
#define GRAIL_BIQUAD_BLOCK 1024
/* grail_iir_async's arguments, checks and refusals, under its own name; further GRAIL_ERR_INVALID_ARG, nothing queued: strides,
 * tail and n_rows that ask for more than 2^31 workgroups (n_rows * ceil(ceil((row_stride + tail) / 1024) / 64)).
 * GRAIL_ERR_OUT_OF_MEMORY: the scratch could not be had.  The set's matrices are computed at its first blocked call and
 * kept with it.  Queues four kernels on ctx's stream. */
int grail_biquad_blocked_async(grail_ctx *ctx, const grail_iir *set, const float *rows_dev, uint64_t row_stride,
                            const uint32_t *len_dev, uint32_t n_rows, const uint32_t *filter_dev, uint32_t tail,
                            float *out_dev, uint64_t out_stride, uint32_t *out_len_dev, uint32_t *nonfinite_dev);
/* Pure host, like grail_iir_design: T of (1) for one filter of n_sections = S sections, coef [5 S]: matrix [2 S][2 S],
 * row-major.  GRAIL_ERR_INVALID_ARG, nothing written: a NULL pointer, S outside 1 .. 8, a coefficient that is not finite. */
int grail_biquad_block_matrix(const double *coef, uint32_t n_sections, double *matrix);

/* ---- levels, continued: recursive filtering of streams ---------------------------------------------------------------------------
 * grail_iir_async takes finished rows.  A caller who pulls a live stream chunk by chunk filters chunk by chunk with an IIR
 * STREAM: n_rows independent rows, each bound to one filter of a live set when the stream is opened, with one `tail` for
 * all, their state resident in HBM between calls.
 * THE CONTRACT.  For any split of a row's samples into calls (calls of no samples included), the outputs of the `next`
 * calls put end to end, followed by the tail that `finish` writes, are bit for bit what grail_iir_async writes for the whole
 * row with the same tail and an out_stride that cuts nothing; the sum of the calls' nonfinite counts is its count.
 * STATE.  Per row: N, the samples fed so far (64 bits); whether the row has ended; the 2 S doubles s1[j], s2[j] (room for
 * the set's largest S).  A `next` call that feeds n samples writes n outputs: there is no delay.  `finish` writes `tail`
 * outputs on +0.0 input (none for a row that was fed nothing) and ends the row. */
typedef struct grail_iir_stream grail_iir_stream;

/* Pure host: *n_out = the outputs a call writes for a row that was fed fed_before samples before it: finishing = 0: a
 * `next` call that feeds n samples (n of them); finishing != 0: `finish` (n must be 0): tail, or 0 when fed_before = 0.
 * GRAIL_ERR_INVALID_ARG, nothing written: n_out NULL; finishing with n != 0; fed_before + n above 2^63 - 1. */
int grail_iir_stream_len(uint64_t fed_before, uint64_t n, uint32_t tail, int finishing, uint64_t *n_out);
/* A stream of n_rows rows on the filters of `set`: filter is a HOST array [n_rows] of indices into the set, NULL means
 * filter 0 for every row.  GRAIL_ERR_INVALID_ARG, nothing created: ctx or out NULL; a set that is not a live set of this
 * context; n_rows = 0; an index >= the set's filter count (checked here: a stream has no refused rows of this kind).
 * These come first; without a usable device: GRAIL_ERR_NO_DEVICE. */
int grail_iir_stream_open(grail_ctx *ctx, const grail_iir *set, uint32_t n_rows, const uint32_t *filter, uint32_t tail,
                          grail_iir_stream **out);
/* Feeds every row u its next n = min(in_len_dev[u], in_stride) samples from in_dev + u * in_stride and writes their n
 * outputs to out_dev + u * out_stride, from index 0; queued on ctx's stream.  Results are DEVICE arrays [n_rows], either
 * may be NULL: out_len[u] = n; nonfinite[u] = the samples among this call's n that are not finite.  n = 0 is legal (a
 * paused row).  A row that has ended and is fed n > 0 is refused: out_len = GRAIL_LIMIT_REFUSED, nonfinite 0, nothing
 * written, its state as it was.  out_dev past out_len is never written.  GRAIL_ERR_INVALID_ARG, nothing queued: a stream
 * that is not an open stream of this context (looked up, not looked into); a NULL buffer with samples to read or write,
 * in_len_dev NULL; out_stride < in_stride; overlapping ranges.  These come first; without a usable device:
 * GRAIL_ERR_NO_DEVICE. */
int grail_iir_stream_next_async(grail_ctx *ctx, grail_iir_stream *is, const float *in_dev, uint64_t in_stride,
                                const uint32_t *in_len_dev, float *out_dev, uint64_t out_stride,
                                uint32_t *out_len_dev, uint32_t *nonfinite_dev);
/* Rings out the rows marked in which (a HOST array [n_rows] of bytes, non-zero = marked; NULL = every row): a marked row
 * that has not ended writes its tail to out_dev + u * out_stride and ends.  out_len (device [n_rows], may be NULL): the
 * tail's length; 0, and nothing written, for unmarked rows, rows that had ended before and rows that were fed nothing.
 * GRAIL_ERR_INVALID_ARG, nothing queued: a stream that is not an open stream of this context; out_stride below the
 * stream's tail; out_dev NULL with a tail to write. */
int grail_iir_stream_finish_async(grail_ctx *ctx, grail_iir_stream *is, const uint8_t *which, float *out_dev,
                                  uint64_t out_stride, uint32_t *out_len_dev);
/* Releases a stream once everything queued on ctx's stream is through; streams still open at grail_destroy go with the
 * context.  NULL is a no-op.  GRAIL_ERR_INVALID_ARG: not an open stream of this context.  While a set has open streams,
 * grail_iir_free of it returns GRAIL_ERR_INVALID_ARG and frees nothing. */
int grail_iir_stream_close(grail_ctx *ctx, grail_iir_stream *is);

/* ---- levels, continued: dynamics ---------------------------------------------------------------------------------------------------
 * Between the equaliser (grail_iir_async) and the limiter (grail_limit_async) a speech chain has a compressor: it evens out
 * an utterance's syllables, holds a bus together, pushes a bed down under a voice (ducking), closes a gate on the noise
 * between phrases.  All of them are one thing: an envelope follower with separate attack and release, and a gain read off
 * a static curve at the envelope's level.  The limiter keeps its hard guarantee; this is the soft stage in front of it.
 * ARITHMETIC.  All of it IEEE binary64, every operation rounded by itself (no fused multiply-add anywhere), evaluated in
 * the order written; denormals are not flushed.  The device evaluates no log, exp or pow: the curve is a TABLE made on the
 * host, the caller's own or grail_dyn_design's, indexed with the exponent and mantissa bits of the envelope and interpolated
 * linearly.  The numbers are a pure function of the row's samples, its key's samples, its curve, alphas and detector: not
 * of the strides beyond where they cut, the row's index, the rows around it, the other curves of the set, alignment, the
 * device or the launch.  No atomics.
 * CURVE.  LO = GRAIL_DYN_LOG2_LO = -32, HI = GRAIL_DYN_LOG2_HI = 8, 16 = GRAIL_DYN_STEPS_PER_OCTAVE steps an octave,
 * GRAIL_DYN_POINTS = (HI - LO) * 16 + 1 = 641 points.  A curve is G[641] finite doubles >= 0, the gain at the levels
 *     lev[k] = 2^(LO + k div 16) * (1 + (k mod 16) / 16),   k = 0 .. 640           (lev[0] = 2^-32, lev[640] = 2^8)
 * of the envelope e; with it two numbers alpha_attack, alpha_release in [0, 1) and a detector, GRAIL_DYN_PEAK (e follows
 * |w|, a level in dB is 20 log10 e) or GRAIL_DYN_SQUARE (e follows w*w, a level in dB is 10 log10 e).
 * LOOKUP  curve(e), for e finite and >= 0:
 *   - e < 2^LO: G[0].   e >= 2^HI: G[640].
 *   - otherwise, with E the biased exponent field of e and m its 52 mantissa bits:
 *         k = (E - (1023 + LO)) * 16 + (m >> 48);   f = (double)(m & (2^48 - 1)) * 2^-48   (exact);
 *         g = G[k] + f * (G[k+1] - G[k])            (one subtraction, one product, one addition, each rounded)
 * SET.  1 <= C <= GRAIL_DYN_CURVES_MAX = 16 curves, each with its own alphas and detector.
 * ROW.  For a row of n = min(len[u], row_stride) samples with curve c = curve_dev[u] (NULL: curve 0 for every row), from
 * e = +0.0, for t = 0 .. n - 1 in ascending order:
 *     1. v = (double)x[t]                 (a sample that is not finite is counted once in nonfinite[u], enters as +0.0, and
 *                                          its output is +0.0)
 *     2. the key:  self-keyed: w = v.   keyed: w = (double)key[kr][t] for t < min(key_len[kr], key_stride), +0.0 beyond
 *                                          (a key sample that is not finite enters as +0.0 and is not counted)
 *     3. a = |w|  (PEAK)   or   a = w * w  (SQUARE)
 *     4. alpha = (a > e) ? alpha_attack : alpha_release;      e = a + alpha * (e - a)
 *     5. g = curve(e);      out[t] = (float)(g * v)  for t < n_out = min(n, out_stride): the only rounding to binary32
 *     6. min_gain[u] = the smallest g over ALL t < n (also where out_stride cut the outputs; the first of equal ones), and
 *        1.0 for n = 0.  With make-up in the curve it can lie above 1.0.
 * out between n_out and out_stride is never written; memory between n and row_stride enters nothing.  out_len[u] = n_out.
 * g is finite and v enters finite, so no NaN is ever produced: every output bit is promised.
 * REFUSED ROWS.  A row whose curve index is >= C, or (keyed) whose key index is >= n_keys: out_len[u] = GRAIL_LIMIT_REFUSED,
 * nonfinite[u] = 0, min_gain[u] = NaN (the bits 0x7FF8000000000000), its out row unwritten.
 * KEYS.  key_dev: device [n_keys][key_stride] floats, NULL = self-keyed (then the key arguments are not read).  key_len_dev:
 * device [n_keys], NULL = key_stride for every key.  key_row_dev: device [n_rows], NULL = row u listens to key u (then
 * n_keys >= n_rows).  Ducking: the bed's rows keyed by the voice's track.  The poor man's stereo link: both channels keyed
 * by one row.  Keyed rows may not overlap out_dev (they may be rows_dev itself).
 * DESIGN.  grail_dyn_design fills G[k] for k = 0 .. 640.  With T = threshold_db, R = ratio, W = knee_db:
 *     x = 20 * log10(lev[k])  (PEAK)   or   10 * log10(lev[k])  (SQUARE);     d = x - T;     h = W / 2
 *     GRAIL_DYN_COMPRESS:   d <= -h:  r = 0.0
 *                           d >=  h:  r = (T + d / R) - x
 *                           else:     q = d + h;   r = ((1 / R - 1) * (q * q)) / (2 * W)
 *     GRAIL_DYN_EXPAND:     d >=  h:  r = 0.0
 *                           d <= -h:  r = (T + d * R) - x
 *                           else:     q = d - h;   r = ((1 - R) * (q * q)) / (2 * W)
 *                           then r = -range_db where r < -range_db        (the reduction is held at the range; a gate is
 *                                                                          a large R with the range it may close by)
 *     G[k] = pow(10, (r + makeup_db) / 20)
 * (r is y - x of the usual soft-knee curve y(x); range_db is read by EXPAND only.)  The bits of log10 and pow are the C
 * library's: the table as grail_dyn_design returns it is the contract, as with grail_iir_design.
 * BALLISTICS.  grail_dyn_ballistics: alpha = exp(-1000 / (ms * (double)rate)), and exactly 0.0 for a time of 0 (the envelope
 * is the detector's value at once); alpha[0] from attack_ms, alpha[1] from release_ms.  After `ms` the envelope has covered
 * 1 - 1/e of a step.
 * WHAT THE TABLE PROMISES: between two points the curve is the chord.  Against the ideal formula that is within 0.01 dB
 * on a segment that holds no corner of the curve and within 0.14 dB on the one segment that holds a hard corner (DESIGN.md
 * §4.23 derives and measures both).
 * A LONE LONG ROW is one lane's serial work here, as in grail_iir_async.  The branch on a > e makes the recurrence
 * non-linear, so the chain of step 4 stays serial whoever runs it; the rest of a sample's work no longer is: the next
 * section, grail_track_dyn_async, gives a row a workgroup and writes these very bits.  NOT here: look-ahead (the limiter
 * is the look-ahead stage), linked groups that take the maximum over members (a shared key row is what there is), smoothing
 * in the log domain. */
#define GRAIL_DYN_STEPS_PER_OCTAVE 16
#define GRAIL_DYN_LOG2_LO (-32)
#define GRAIL_DYN_LOG2_HI 8
#define GRAIL_DYN_POINTS 641
#define GRAIL_DYN_CURVES_MAX 16
#define GRAIL_DYN_PEAK     0
#define GRAIL_DYN_SQUARE   1
#define GRAIL_DYN_COMPRESS 0
#define GRAIL_DYN_EXPAND   1
typedef struct grail_dyn grail_dyn; /* a set of gain curves with their ballistics, resident in HBM */

/* Pure host: gain[0 .. 640] = G of DESIGN above.  GRAIL_ERR_INVALID_ARG, nothing written: an unknown kind or detector,
 * a threshold_db or makeup_db that is not finite, ratio < 1 or not finite, knee_db or range_db below 0 or not finite, gain
 * NULL, a table whose numbers are not all finite (a make-up of thousands of dB). */
int grail_dyn_design(int kind, int detector, double threshold_db, double ratio, double knee_db, double range_db,
                     double makeup_db, double *gain /* [GRAIL_DYN_POINTS] */);
/* Pure host: alpha[0], alpha[1] of BALLISTICS above.  GRAIL_ERR_INVALID_ARG, nothing written: sample_rate 0, a time that
 * is negative or not finite, alpha NULL, a time so long that its alpha rounds to 1.0. */
int grail_dyn_ballistics(uint32_t sample_rate, double attack_ms, double release_ms, double alpha[2]);

/* A set of n_curves curves on ctx's device: gain [n_curves][GRAIL_DYN_POINTS], alpha [n_curves][2] (attack, release),
 * detector [n_curves].  The set keeps its own copy, uploaded on ctx's stream; the arrays may be reused at once.
 * GRAIL_ERR_INVALID_ARG, nothing created: a NULL argument, n_curves outside 1 .. 16, a gain that is not finite or is
 * negative, an alpha outside [0, 1), an unknown detector.  These come first; without a usable device: GRAIL_ERR_NO_DEVICE. */
int grail_dyn_create(grail_ctx *ctx, const double *gain, const double *alpha, const uint32_t *detector, uint32_t n_curves,
                     grail_dyn **out);
/* Releases a set once everything queued on ctx's stream is through; sets still alive at grail_destroy go with the
 * context.  NULL is a no-op.  GRAIL_ERR_INVALID_ARG: a pointer that is not a live set of this context (sets are looked up,
 * not looked into); a set that still has open streams. */
int grail_dyn_free(grail_ctx *ctx, grail_dyn *set);
/* ROW above, queued on ctx's stream like grail_iir_async: rows_dev: device [n_rows][row_stride]; len_dev: device [n_rows];
 * curve_dev: device [n_rows] or NULL; the keys as in KEYS; out_dev: device [n_rows][out_stride] (out_stride = 0: the
 * results only).  Results are DEVICE arrays [n_rows], each may be NULL: out_len, nonfinite, min_gain.  out_dev must overlap
 * neither rows_dev nor the keyed rows.  16-byte loads and stores where every base is 16-byte aligned and every stride a
 * multiple of 4, 4-byte ones otherwise: same bits.  One lane takes one row, 64 rows to a wavefront.
 * GRAIL_ERR_INVALID_ARG, nothing queued: set NULL or of another context; a NULL buffer with samples to read or write;
 * key_dev with n_keys = 0, or with key_row_dev NULL and n_keys < n_rows; overlapping ranges; rows or keys that span more
 * than 2^60 samples; row_stride and out_stride that both allow a row of 2^32 samples or more.  These come first; without a
 * usable device: GRAIL_ERR_NO_DEVICE.  n_rows = 0 is a success that queues nothing. */
int grail_dyn_async(grail_ctx *ctx, const grail_dyn *set, const float *rows_dev, uint64_t row_stride,
                    const uint32_t *len_dev, uint32_t n_rows, const uint32_t *curve_dev, const float *key_dev,
                    uint64_t key_stride, const uint32_t *key_len_dev, uint32_t n_keys, const uint32_t *key_row_dev,
                    float *out_dev, uint64_t out_stride, uint32_t *out_len_dev, uint32_t *nonfinite_dev,
                    double *min_gain_dev);

/* ---- levels, continued: dynamics, a workgroup a row ------------------------------------------------------------------------------
 * The same call for the few long tracks of a finished mix.  grail_dyn_async gives a row to one lane, which is right for
 * thousands of utterances and leaves a lone track of minutes to one lane of one wavefront.  grail_track_dyn_async gives a row
 * a workgroup.  Of a sample's work only step 4 of ROW above, alpha = (a > e) ? alpha_attack : alpha_release and
 * e = a + alpha * (e - a), needs the sample before it: that chain stays serial, one lane's.  Steps 1 to 3 ahead of it and the
 * lookup, the product, the rounding to binary32 and the candidate for min_gain behind it are done for 1 024 samples at a
 * time by the workgroup's other lanes, a tile ahead of the chain and a tile behind it.
 * THE BITS are those of ROW above, whatever the number of rows: this is no contract of its own.  Every operation is ROW's,
 * in ROW's order, each rounded by itself; out, out_len, nonfinite and min_gain are bit for bit what grail_dyn_async writes
 * for the same arguments, min_gain the first in time of equal gains (the sign of a zero gain included), over all t < n.
 * Sets, keys, curves, refused rows, out_stride = 0, the 16-byte and 4-byte accesses: all as there.  No atomics.
 * WHICH CALL FOR WHAT.  Both calls write the same bits, so the choice is one of time alone, and the library does not
 * make it.  Measured on one MI355X (DESIGN.md §4.24, rows of 96 006 samples, call and sync): this call is the faster up to
 * 512 rows and beyond: 2.1 ms against 11.8 ms for 1 row, 2.9 ms against 13.6 ms for 512 rows; at 4 096 rows the two are level
 * (14.5 ms against 13.7 ms); at 65 536 rows grail_dyn_async is 14 times the faster (15.9 ms against 220 ms).  A lone row of
 * 10^7 samples takes 221 ms here, 22 ns a sample, against 1 233 ms there, and eight such rows 238 to 264 ms (a launch's time
 * moves by a fifth with where its workgroups land).  So: the tracks of a mix, up to a few hundred rows: this call.  The
 * utterances of a batch, thousands of rows: grail_dyn_async.
 * Arguments, checks and errors are grail_dyn_async's, in its order, with this call's name in grail_last_error; besides,
 * GRAIL_ERR_INVALID_ARG for more than 2^31 - 1 rows (a workgroup a row).  These come first; without a usable device:
 * GRAIL_ERR_NO_DEVICE.  n_rows = 0 is a success that queues nothing, and so is row_stride = 0 with no result asked for.
 * NOT here: a stream form (grail_dyn_stream_* carries e between calls), a choice between the two calls made by the library. */
int grail_track_dyn_async(grail_ctx *ctx, const grail_dyn *set, const float *rows_dev, uint64_t row_stride,
                          const uint32_t *len_dev, uint32_t n_rows, const uint32_t *curve_dev, const float *key_dev,
                          uint64_t key_stride, const uint32_t *key_len_dev, uint32_t n_keys, const uint32_t *key_row_dev,
                          float *out_dev, uint64_t out_stride, uint32_t *out_len_dev, uint32_t *nonfinite_dev,
                          double *min_gain_dev);

/* ---- levels, continued: dynamics of streams ---------------------------------------------------------------------------------------
 * A DYNAMICS STREAM: n_rows independent rows, each bound to one curve of a live set (and, keyed, to one key row) when the
 * stream is opened, their state resident in HBM between calls: N, the samples fed so far (64 bits), and e.
 * THE CONTRACT.  For any split of a row's samples into calls (calls of no samples included), the outputs of the `next`
 * calls put end to end are bit for bit what grail_dyn_async writes for the whole row; the sum of the calls' nonfinite
 * counts is its count; a call's min_gain is that call's own (1.0 for a call that fed the row nothing), and the smallest
 * over the calls that fed the row something is the whole row's.  A row rings out over nothing: there is no `finish`, and
 * a row never ends.
 * KEYS.  A keyed stream (n_keys >= 1 at open) reads the key of row u in a call at key_dev + key_row[u] * key_stride,
 * samples t < in_len[u]: the key advances with the row it drives. */
typedef struct grail_dyn_stream grail_dyn_stream;

/* A stream of n_rows rows on the curves of `set`: curve is a HOST array [n_rows] of indices into the set, NULL means
 * curve 0 for every row.  n_keys = 0: self-keyed (key_row is not read).  n_keys >= 1: key_row is a HOST array [n_rows] of
 * indices below n_keys, NULL means row u listens to key u (then n_keys >= n_rows).  GRAIL_ERR_INVALID_ARG, nothing
 * created: ctx or out NULL; a set that is not a live set of this context; n_rows = 0; a curve index >= the set's count; a
 * key index >= n_keys (checked here: a stream has no refused rows).  These come first; without a usable device:
 * GRAIL_ERR_NO_DEVICE. */
int grail_dyn_stream_open(grail_ctx *ctx, const grail_dyn *set, uint32_t n_rows, const uint32_t *curve, uint32_t n_keys,
                          const uint32_t *key_row, grail_dyn_stream **out);
/* Feeds every row u its next n = min(in_len_dev[u], in_stride) samples from in_dev + u * in_stride and writes their n
 * outputs to out_dev + u * out_stride, from index 0; queued on ctx's stream.  key_dev: device [n_keys][key_stride] for a
 * keyed stream, NULL for a self-keyed one.  Results are DEVICE arrays [n_rows], each may be NULL: out_len[u] = n;
 * nonfinite[u]; min_gain[u].  n = 0 is legal (a paused row).  out_dev past out_len is never written.
 * GRAIL_ERR_INVALID_ARG, nothing queued: a stream that is not an open stream of this context (looked up, not looked into);
 * a NULL buffer with samples to read or write, in_len_dev NULL; out_stride < in_stride; a keyed stream without key_dev, a
 * self-keyed one with it; key_stride < in_stride; overlapping ranges.  These come first; without a usable device:
 * GRAIL_ERR_NO_DEVICE. */
int grail_dyn_stream_next_async(grail_ctx *ctx, grail_dyn_stream *ds, const float *in_dev, uint64_t in_stride,
                                const uint32_t *in_len_dev, const float *key_dev, uint64_t key_stride, float *out_dev,
                                uint64_t out_stride, uint32_t *out_len_dev, uint32_t *nonfinite_dev, double *min_gain_dev);
/* Releases a stream once everything queued on ctx's stream is through; streams still open at grail_destroy go with the
 * context.  NULL is a no-op.  GRAIL_ERR_INVALID_ARG: not an open stream of this context.  While a set has open streams,
 * grail_dyn_free of it returns GRAIL_ERR_INVALID_ARG and frees nothing. */
int grail_dyn_stream_close(grail_ctx *ctx, grail_dyn_stream *ds);

/* ---- device memory plumbing ------------------------------------------- */
int grail_device_alloc(grail_ctx *ctx, size_t bytes, void **out);
int grail_device_free(grail_ctx *ctx, void *ptr);
/* Pinned (page-locked) host memory.  A GRAIL_OUT_HOST destination that lives in it receives the
 * device-to-host copies directly, at PCIe rate; a pageable destination is fed through pinned
 * staging buffers and copier threads (still overlapped with the kernels, a little slower). */
int grail_host_alloc(grail_ctx *ctx, size_t bytes, void **out);
int grail_host_free(grail_ctx *ctx, void *ptr);
int grail_memcpy_d2h(grail_ctx *ctx, void *dst_host, const void *src_dev, size_t bytes);
int grail_memcpy_h2d(grail_ctx *ctx, void *dst_dev, const void *src_host, size_t bytes);
int grail_memset_d(grail_ctx *ctx, void *dst_dev, int value, size_t bytes);

/* ---- multi-GPU: utterance sharding + voice-table broadcast ------------- */
/* Contiguous utterance range of `rank` out of `world`:
 * [rank*n/world, (rank+1)*n/world) in 64-bit arithmetic. */
void grail_shard_range(uint64_t n_utt, uint32_t rank, uint32_t world, uint64_t *begin,
                       uint64_t *end);
/* RCCL path (one process per GPU).  grail_comm_unique_id fills a 128-byte id
 * on rank 0 that the launcher hands to every rank out of band;
 * grail_comm_init joins the communicator; grail_broadcast_voices sends rank
 * `root`'s voice table (grail_set_voices) to every rank's HBM with one
 * ncclBroadcast on ctx's stream and installs it there. */
#define GRAIL_UNIQUE_ID_BYTES 128
int grail_comm_unique_id(uint8_t id[GRAIL_UNIQUE_ID_BYTES]);
int grail_comm_init(grail_ctx *ctx, const uint8_t id[GRAIL_UNIQUE_ID_BYTES], uint32_t rank,
                    uint32_t world);
int grail_broadcast_voices(grail_ctx *ctx, uint32_t n_voices, uint32_t root);
/* What RCCL itself reports for ctx's communicator: *ranks = ncclCommCount (0 when no communicator
 * has been formed), *rank = ncclCommUserRank.  Lets a launcher prove that N ranks really met. */
int grail_comm_info(grail_ctx *ctx, uint32_t *ranks, uint32_t *rank);
int grail_comm_destroy(grail_ctx *ctx);

/* ---- one call, the whole node (SURVEY.md §8e "one process, 8 devices") ---------------------------------------------
 * The reference host makes ONE call for its whole job (examples/cli.rs:175-184: one chain, collected) and the chain's
 * state is per utterance (src/lib.rs:470-488, 724-748, 839-854), so a batch shards over the GPUs of a node with no
 * exchange step.  A grail_node is that for a host that stays one process (a Rust binary, say): one grail_ctx and one
 * host thread per device; a call cuts the batch into the contiguous ranges of grail_shard_range, renders the shards
 * concurrently and lands every shard in its slice of ONE host buffer.  Utterance u's samples are the same bits as from
 * grail_synthesize_batch on a single context ("arithmetic" = 0; in fast arithmetic they follow the kernel family of the
 * shard's size, as with any batch size — pin "lanes_per_utterance" for batch-invariant fast bits).
 * A node is used from one thread at a time.  Failures: the first failing device's status and message
 * ("device[i] = d: ..."); GRAIL_ERR_BUFFER_TOO_SMALL when some shard reported it and none failed harder. */
/* devices[n_devices]: HIP device ordinals, one shard each (NULL: 0 .. n_devices - 1).  A device may be named more than
 * once (several contexts on it — what the tests on a one-GPU box do); RCCL then cannot form the communicator, see
 * grail_node_set_voices. */
int grail_node_create(const int *devices, uint32_t n_devices, grail_node **out);
int grail_node_destroy(grail_node *node);
uint32_t grail_node_size(const grail_node *node);
/* The context of device slot `index` (borrowed; owned by the node): per-device queries — grail_get_option,
 * grail_device_pci_bus_id, grail_comm_info, grail_get_voices — between node calls. */
int grail_node_context(grail_node *node, uint32_t index, grail_ctx **ctx);
/* Installs the voice table on every device: device slot 0 receives it (grail_set_voices) and ONE ncclBroadcast over
 * xGMI carries it to the HBM of the others, over a communicator formed inside the process (ncclCommInitAll over the
 * node's devices, on the first call) — the collective of §8e.  RCCL refuses a communicator that names a GPU twice: a
 * node created with duplicate devices fails here with GRAIL_ERR_RCCL unless option "node_voices_without_rccl" = 1 was
 * set, which installs the table with one grail_set_voices per context instead (for tests on a one-GPU box; never
 * chosen silently). */
int grail_node_set_voices(grail_node *node, const grail_voice *voices, uint32_t n_voices);
/* "node_voices_without_rccl" (0 default / 1) belongs to the node; every other name is grail_set_option on each of
 * its contexts.  grail_node_get_option: "node_devices", "node_voices_without_rccl", "node_rccl_ranks" (the smallest
 * ncclCommCount over the contexts, 0: no communicator); any other name is read from device slot 0. */
int grail_node_set_option(grail_node *node, const char *name, int64_t value);
int grail_node_get_option(grail_node *node, const char *name, int64_t *value);
/* The shard of device slot `index` out of n_devices, as a pure host function (no GPU): rows
 * [first_row, first_row + rows) = grail_shard_range(n_utt, index, n_devices), their segments
 * segs[first_seg .. first_seg + n_segs), and — rebased_offsets != NULL, cap >= rows + 1 — the rows' seg_offsets
 * relative to first_seg.  The node calls below hand exactly this view to grail_synthesize_batch*(): segs + first_seg,
 * rebased_offsets, voice_ids + first_row, jitter_seeds + first_row, out + first_row * out_stride, out_len + first_row. */
typedef struct grail_node_shard {
    uint64_t first_row;
    uint64_t rows;
    uint32_t first_seg;
    uint32_t n_segs;
} grail_node_shard;
int grail_node_shard_of(const uint32_t *seg_offsets, uint64_t n_utt, uint32_t index, uint32_t n_devices,
                        grail_node_shard *shard, uint32_t *rebased_offsets, uint64_t cap);
/* grail_synthesize_batch / _elems / _pcm16 / grail_say_batch over the node: same arguments and row semantics; `out`
 * and `out_len` are HOST memory (flags must not hold GRAIL_OUT_DEVICE: there is no one device to leave the rows on).
 * Every shard goes through its context's overlapped device-to-host pipeline into its slice of `out`; pinned memory
 * from grail_node_host_alloc receives the copies directly. */
int grail_node_synthesize_batch(grail_node *node, const grail_phoneme_elem *segs, const uint32_t *seg_offsets,
                                const uint32_t *voice_ids, const uint32_t *jitter_seeds, uint32_t n_utt, float *out,
                                uint64_t out_stride, uint32_t *out_len, uint32_t flags);
int grail_node_synthesize_batch_elems(grail_node *node, const grail_sequence_elem *segs, const uint32_t *seg_offsets,
                                      const uint32_t *voice_ids, const uint32_t *jitter_seeds, uint32_t n_utt,
                                      float *out, uint64_t out_stride, uint32_t *out_len, uint32_t flags);
int grail_node_synthesize_batch_pcm16(grail_node *node, const grail_phoneme_elem *segs, const uint32_t *seg_offsets,
                                      const uint32_t *voice_ids, const uint32_t *jitter_seeds, uint32_t n_utt,
                                      int16_t *out, uint64_t out_stride, uint32_t *out_len, uint32_t flags);
/* ... with the rows LEFT IN HBM (what a downstream GPU consumer wants, and what the headline metric measures): slot i's shard is
 * rendered into out_dev[i] — device memory of slot i's GPU holding its rows x out_stride floats (grail_device_alloc on
 * grail_node_context(node, i); rows from grail_node_shard_of), row r of the shard at out_dev[i] + r * out_stride; NULL for a slot
 * whose shard is empty.  out_len: host memory [n_utt] or NULL.  No copy is made; the call returns when every slot has finished. */
int grail_node_synthesize_batch_device(grail_node *node, const grail_phoneme_elem *segs, const uint32_t *seg_offsets,
                                       const uint32_t *voice_ids, const uint32_t *jitter_seeds, uint32_t n_utt,
                                       float *const *out_dev, uint64_t out_stride, uint32_t *out_len);
int grail_node_say_batch(grail_node *node, const char *const *texts_utf8, uint32_t n_texts, const uint32_t *voice_ids,
                         const uint32_t *jitter_seeds, float *out, uint64_t out_stride, uint32_t *out_len,
                         uint32_t flags);
/* grail_batch_lengths over the node (the Sequencer clock pre-pass, src/lib.rs:861-888): what a caller sizes out_stride
 * with.  out_len is host memory [n_utt]. */
int grail_node_lengths(grail_node *node, const grail_phoneme_elem *segs, const uint32_t *seg_offsets,
                       const uint32_t *voice_ids, uint32_t n_utt, uint32_t max_len, uint32_t *out_len);
/* Wall-clock milliseconds each device slot spent in the last node call (host memory [grail_node_size]; 0 for a slot
 * whose shard was empty): how evenly the shards loaded the node. */
int grail_node_last_shard_ms(grail_node *node, float *ms, uint32_t cap);
/* Pinned host memory every device of the node can copy into (hipHostMallocPortable). */
int grail_node_host_alloc(grail_node *node, size_t bytes, void **out);
int grail_node_host_free(grail_node *node, void *ptr);

#ifdef __cplusplus
}
#endif

/* ---- levels, continued: short-time spectra (STFT power and mel bands of rows): a header of its own, a part of this one --- */
#include "grail_spectrum.h"

#endif /* GRAIL_HIP_H */
