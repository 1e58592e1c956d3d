// api_internal.hpp — what the host translation units of the library share (internal; host code only: the kernel
// units include kernels.h, never this).  grail_api.cpp: contexts, batches, voices; options.cpp: the option table,
// grail_set_option / grail_get_option; voice_analysis.cpp: what a voice table qualifies for; family_choice.cpp,
// family_cost.cpp, dispatch_model.cpp, launch_plan.cpp: kernel families, cost model, dispatcher model, block planner
// (launch_plan.h); synthesize.cpp: launches; streams.cpp: resumable and live streams; mix.cpp: rows
// mixed into tracks; levels.cpp: rows measured (levels, loudness, true peak); transforms.cpp: rows limited, resampled and
// filtered (FIR, recursive) at once, transform_streams.cpp: the same as streams (both on transform_state.h); host_output.cpp: the one-call
// forms with a host destination; comm.cpp and node.cpp: RCCL, the contexts of a node.  Every HIP resource these units
// create has one owner type (below): Event, Stream, DeviceBuffer, PinnedBuffer.
#pragma once

#include <dlfcn.h>
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>

#include <algorithm>
#include <atomic>
#include <cmath>
#include <condition_variable>
#include <cstdio>
#include <deque>
#include <map>
#include <memory>
#include <mutex>
#include <thread>
#include <cstdlib>
#include <cstring>
#include <new>
#include <string>
#include <type_traits>
#include <unordered_map>
#include <utility>
#include <vector>

#include "../../include/grail_hip.h"
#include "division_window.h"
#include "dyn_plan.h"
#include "fir_plan.h"
#include "iir_plan.h"
#include "kernels.h"
#include "limit_plan.h"
#include "meter_plan.h"
#include "resample_plan.h"
#include "spectrum_plan.h"

// (the opaque types of the C ABI are global; everything else the units share lives in grail::host)

// words of the device block behind grail_ctx::d_truncated: the flag and three statistics counters; debug builds
// (-DGRAIL_FAST_PROF) keep 32 u64 profile counters behind word 8
#ifdef GRAIL_FAST_PROF
constexpr size_t TRUNCATED_WORDS = 8 + 64;
#else
constexpr size_t TRUNCATED_WORDS = 4;
#endif

// What grail_set_option writes (options.cpp holds the table of names and checks), with every default.  All int64, as
// the ABI passes them.
struct Options {
    int64_t fast_option = 0;          // "arithmetic": 0 exact (bit-identical), 1 fast (stated tolerance: the tier the voices'
                                      // sharpness allows), 2 fast with the reference's own coefficients (MID) whatever the voices
    int64_t fast_limit = (int64_t)GRAIL_FAST_SHARPNESS_LIMIT;   // "fast_sharpness_limit": fast kernels up to this
    int64_t mid_option = 1;           // "fast_exact_coefficients": sharper voices get the second tolerance tier (MID)
    int64_t mid_limit = (int64_t)GRAIL_FAST_SHARPNESS_LIMIT_EXACT_COEFFICIENTS;   // ... up to this sharpness
    int64_t lanes_option = 0;         // 0 = auto
    int64_t skip_silent_option = 1;   // skip band-pass filters of provably silent formants
    int64_t pipeline_option = 1;      // small qualifying batches: producer/consumer workgroups
    int64_t pipe_round32 = 1;         // ... with rounds of 32 samples while one workgroup per CU suffices (8.20 -> 7.86 ms for config 2)
    int64_t pipe_spread = 1;          // pipelined workgroups on rows that differ in length: few utterances per workgroup (pipe_fill_for)
    int64_t pipe4_max_groups = -1;    // four-formant pipelined workgroups (16 utterances each): up to so many (-1: two per CU)
    int64_t pipe8_max_groups = -1;    // eight-formant pipelined workgroups: up to so many (-1: two per CU)
    int64_t scan_option = 1;          // fast arithmetic: small batches go to the time-parallel scan kernel
    int64_t scan_max_utts = -1;       // ... up to this many utterances (x 4/7 with eight live formants; -1: 34 per CU = 8704)
    int64_t scan_split_max = -1;      // ... and up to this many with the carrier phase on a wave of its own (-1: 6 per CU = 1536)
    int64_t scan_debug = 0;           // development builds only (-DGRAIL_SCAN_DEBUG): see scan_kernels.hip
    int64_t split_option = 1;         // fast arithmetic: mid-size batches split every utterance's time axis over lanes
    int64_t split_chunks = 0;         // ... into this many chunks (0: as many as fill the machine)
    int64_t split_span = 0;           // ... laid out over this many samples (0: the batch's longest utterance)
    int64_t split_ff_permille = 165;  // ... cost of a fast-forwarded sample against a rendered one
    int64_t split_min_utts = -1;      // ... -1: the cost model picks between the scan kernel, the time-split kernels and the lane
                                      // kernels (family_cost; 2 s utterances: 1 024 of them 2.00 (scan) against 3.13 ms (split),
                                      // 1 536: 3.22 / 3.14, 2 048: 3.33 / 3.13, profiles/r03_small_batch.txt); >= 0: batches smaller
                                      // than this (x 5/6 with eight live formants) stay with the scan kernel, whatever their length
    int64_t composite_option = 1;     // a batch may be cut into blocks with a kernel family each (plan_blocks)
    int64_t row_groups_option = 1;    // rows the lean families cannot take are planned apart: 1 where the cost model says so, 2 always, 0 never
    int64_t ragged_option = 1;        // length-sorted batches: lane mappings weighed by the rows' lengths (ragged_plan)
    int64_t two_waves_option = 1;     // tolerance-mode lane kernels on 2 / 4 / 8 lanes: two waves per SIMD where a launch has more waves than SIMDs
    int64_t packed_option = 1;        // launches of more one-wave-per-SIMD workgroups than the device has room for: launch slots in packed order
    int64_t sort_option = 1;          // ragged batches: fill launch slots in order of decreasing length
};

// what a voice of the table qualifies for (a batch is judged by the voices IT names: used_voices)
struct VoiceInfo {
    bool upper_silent = false, live4_ok = false, scan_ok = false, split_ok = false;
    uint32_t warmup = 0;
};

// What install_voices derives from the voice table; the defaults are "no voice table set".  The table-wide flags are what
// a context without per-voice records (grail_plan_blocks) goes by.
struct VoiceFacts {
    std::vector<VoiceInfo> voice_info;
    bool voices_upper_silent = false; // every voice: formants 5-8 have amplitude +0 in every phoneme
    bool voices_live4_ok = false;     // ... and parameters that keep their output at exactly +0 (live4_ok)
    bool voices_scan_ok = false;      // every formant of every voice inside the safe window (scan_voice_ok)
    bool voices_split_ok = false;     // every voice has a warm-up length (voice_warmup): time-split fast kernels
    uint32_t max_warmup = 0;          // ... the longest of them
    float max_rate = 0.0f;            // highest sample rate of the table
    float max_dt = 0.0f;              // largest 1/sample_rate of the table
    float max_pitch_jitter = 0.0f;    // largest |jitter_delta_frequency| of the table
    double voices_sharpness = INFINITY;   // the largest predicted fast-mode deviation of the table, units of 2^-23
    std::vector<double> voice_sharpness;  // ... per voice (a batch is judged by the voices it uses)
};

// What the read-only options tell of the last synthesis launch (its largest block) and of the kernels synced so far
struct LaunchStats {
    std::string last_kernel = "none"; // instantiation of the last synthesis launch
    int last_formants = 8, last_lanes = 0, last_pipe = 0;
    int last_split = 0;               // chunks of the last launch (0: not time-split)
    int last_fast = 0;                // the last launch ran tolerance arithmetic in some block
    int last_blocks = 0;              // kernel launches the last synthesis call was cut into
    int last_packed = 0;              // ... blocks of it launched in packed order
    uint64_t slow_steps = 0;          // of the kernels synced so far
    uint64_t fast_tiles = 0, general_steps = 0;
};

namespace grail {
namespace host {

// errors: the status is returned, the message kept per thread for grail_last_error()
int fail(int status, const std::string &msg);
int hip_fail(hipError_t e, const char *what);
std::string &last_error();

#define HIP_TRY(expr)                                  \
    do {                                               \
        hipError_t e_ = (expr);                        \
        if (e_ != hipSuccess) return ::grail::host::hip_fail(e_, #expr); \
    } while (0)

// One HIP resource and its only owner: move-only, the destructor releases, an empty one holds nothing and releases
// nothing.  Contexts, batches, streams, the per-context parts of the units and the calls' temporaries hold their events,
// streams, device and pinned memory in the four types below and in nothing else, so `delete` is all their tear-down.
template <typename H, hipError_t (*Release)(H)>
class Handle {
public:
    Handle() = default;
    Handle(Handle &&o) noexcept : h_(std::exchange(o.h_, H{})) {}
    Handle &operator=(Handle &&o) noexcept
    {
        if (this != &o) {
            reset();
            h_ = std::exchange(o.h_, H{});
        }
        return *this;
    }
    ~Handle() { reset(); }
    H get() const { return h_; }
    void reset()
    {
        if (h_) (void)Release(h_);
        h_ = H{};
    }
    // what was held is released first, then make(&slot) fills the slot; a failure leaves it empty
    template <typename Make>
    hipError_t renew(Make make)
    {
        reset();
        const hipError_t e = make(&h_);
        if (e != hipSuccess) h_ = H{};
        return e;
    }

private:
    H h_{};
};

// created on demand (`if (!ev) ev.create()`); only the context's two timing events keep their time stamps
struct Event : Handle<hipEvent_t, hipEventDestroy> {
    hipError_t create(bool timing = false)
    {
        return renew([&](hipEvent_t *ev) { return timing ? hipEventCreate(ev) : hipEventCreateWithFlags(ev, hipEventDisableTiming); });
    }
    operator hipEvent_t() const { return get(); }
};

// a non-blocking stream.  Its holder declares it before whatever may be queued on it, so that it is destroyed last.
struct Stream : Handle<hipStream_t, hipStreamDestroy> {
    hipError_t create()
    {
        return renew([](hipStream_t *s) { return hipStreamCreateWithFlags(s, hipStreamNonBlocking); });
    }
    operator hipStream_t() const { return get(); }
};

// One hipMalloc allocation of `capacity()` elements.  `reserve` is the one growth rule of device memory: grown when too
// small, never shrunk.  The launch policy (launch_plan.h, voice_analysis.cpp) never sees a type that holds one: its
// inputs are PlanEnv and BatchFacts.
template <typename T>
class DeviceBuffer {
public:
    T *get() const { return static_cast<T *>(mem_.get()); }
    size_t capacity() const { return mem_.get() ? cap_ : 0; }
    void reset() { mem_.reset(); }
    // exactly max(n, 1) elements; what was held is released first
    hipError_t alloc(size_t n)
    {
        cap_ = std::max<size_t>(n, 1);
        return mem_.renew([&](void **p) { return hipMalloc(p, cap_ * sizeof(T)); });
    }
    // room for `need` elements: nothing to do when there is; else `want` (>= need) of them, once everything queued on
    // `stream` is through (a kernel or copy still queued may use the old buffer)
    int reserve(hipStream_t stream, size_t need, size_t want)
    {
        if (capacity() >= std::max<size_t>(need, 1)) return GRAIL_OK;
        if (get()) HIP_TRY(hipStreamSynchronize(stream));
        HIP_TRY(alloc(want));
        return GRAIL_OK;
    }
    int reserve(hipStream_t stream, size_t need) { return reserve(stream, need, need); }

private:
    Handle<void *, hipFree> mem_;
    size_t cap_ = 0;           // of what mem_ holds (a moved-from buffer keeps the number and holds nothing)
};

// max(count, 1) elements for dst, the first `count` of them copied from src (if any) on `stream`
template <typename Tp>
hipError_t upload(DeviceBuffer<Tp> &dst, const void *src, size_t count, hipStream_t stream)
{
    const hipError_t e = dst.alloc(count);
    if (e != hipSuccess || !src || !count) return e;
    return hipMemcpyAsync(dst.get(), src, count * sizeof(Tp), hipMemcpyHostToDevice, stream);
}

// What a stream bound to a set knows of each row: the row's filter, its curve or its key.  The host copy is kept while the
// upload may be in flight.  fill: the caller's n_rows indices; where it gave none, 0 for every row (own_row: u for row u).
struct RowIndex {
    std::vector<uint32_t> host;
    DeviceBuffer<uint32_t> dev;         // [n_rows]
    hipError_t fill(const uint32_t *given, uint32_t n_rows, bool own_row, hipStream_t stream)
    {
        host.resize(n_rows);
        for (uint32_t u = 0; u < n_rows; ++u) host[u] = given ? given[u] : (own_row ? u : 0u);
        return upload(dev, host.data(), n_rows, stream);
    }
};

// One hipHostMalloc allocation of `capacity()` bytes.  Grow-only users ask `capacity() < need` before they alloc.
class PinnedBuffer {
public:
    void *get() const { return mem_.get(); }
    size_t capacity() const { return mem_.get() ? cap_ : 0; }
    void reset() { mem_.reset(); }
    // exactly `bytes`; what was held is released first
    hipError_t alloc(size_t bytes)
    {
        cap_ = bytes;
        return mem_.renew([&](void **p) { return hipHostMalloc(p, bytes, hipHostMallocDefault); });
    }

private:
    Handle<void *, hipHostFree> mem_;
    size_t cap_ = 0;
};

// the kernel family of a launch, a block of rows with its family (family_choice.cpp chooses them)
struct Family {
    int L = 1;                 // lanes per utterance (lane kernels, pipelined workgroups)
    uint32_t pipe = 0;         // exact pipelined workgroups: 1 = rounds of 16 samples, 2 = rounds of 32
    uint32_t live4 = 0;        // formants 5-8 not laid out
    bool half = false;         // one lane per utterance, exact, eight formants laid out but 5-8 silent: the half-live loops
    uint32_t fast = 0;         // tolerance arithmetic
    int split_k = 0;           // time-split kernels: chunks per utterance (0: not time-split)
    uint32_t split_bounds[SPLIT_MAX_CHUNKS + 1] = {};
    uint32_t split_active = 0; // ... rows that differ in length: how many (wave, chunk) pairs have anything to render (0: all)
    bool scan = false;         // the time-parallel scan kernel
    uint32_t scan_pipe = 0;    // ... its three-stage flavour
};

struct Block {
    uint32_t rows;
    Family f;
};

// the launch plan of the last synthesis call of a batch or of one of its row groups, with what it was made for (plan_blocks
// lays out time-split grids by bisection: a fraction of a millisecond of host time, which a one-millisecond kernel should
// not pay at every launch); empty: none yet
struct PlanCache {
    uint64_t key[6] = {};
    std::vector<Block> plan;
};

}  // namespace host
}  // namespace grail

// What the launch policy reads of a context (grail_plan_blocks builds one without a device)
struct PlanEnv {
    int cus = 256;                    // compute units the launch policy plans for (hipDeviceProp_t::multiProcessorCount;
                                      // "assume_compute_units" overrides it): every capacity of the policy is a multiple
    Options opt;
    VoiceFacts facts;
    uint64_t voices_epoch = 0;        // set by every install_voices: unique in the process, not per context
};

// what a unit keeps per context: a type private to the unit, made at first use by the unit's one accessor, deleted with
// the context
struct CtxPart {
    virtual ~CtxPart() = default;
};

struct grail_ctx : PlanEnv {
    int device = 0;
    int device_cus = 256;             // what the device reported (cus: what is planned for)
    grail::host::Stream stream;       // (before everything that may be queued on it: destroyed last)
    grail::host::Event ev_start, ev_stop;
    bool have_timing = false;
    uint64_t options_epoch = 0;       // bumped by every grail_set_option (a batch caches its launch plan against both)
    std::vector<grail_voice> voices;  // host copy of the table
    grail::host::DeviceBuffer<grail::DevVoice> d_voices;
    grail::host::DeviceBuffer<float> d_voice_elems;   // [n_voices * NUM_VOICED][49]
    LaunchStats stats;
    grail::host::DeviceBuffer<uint32_t> d_truncated;  // [0] truncation flag, [1] slow-path wave-steps, [2] fast wave-tiles, [3] general wave-steps
    uint32_t seen_counters[4] = {0, 0, 0, 0};   // d_truncated[1..3] as last read: the device counters only ever grow
    ncclComm_t comm = nullptr;        // (destroyed through the dlopen table: comm_release)
    uint32_t comm_rank = 0, comm_world = 1;
    std::unique_ptr<CtxPart> host_pipe;     // HostPipe (host_output.cpp): streams, events and buffers of the host-output path
    std::unique_ptr<CtxPart> mix_state;     // MixState (mix.cpp): the last mix's plan and the device buffers it was uploaded to
    std::unique_ptr<CtxPart> level_state;   // LevelState (levels.cpp): the frame scratch of grail_levels_async, a block's numbers
    std::unique_ptr<CtxPart> transform_state;   // TransformState (transform_state.h): chunk scratch, resampler tables, filter sets and streams
};

struct grail_stream {
    const grail_batch *batch = nullptr;
    grail::host::DeviceBuffer<uint32_t> d_state;   // [state_words(L)][lanes]
    uint64_t lanes = 0;
    int L = 1;
    bool started = false;
    // the kernel flavour, fixed when the stream is opened (the state layout follows it)
    bool live4 = false, half_capable = false, any_blend = false;
    uint64_t voices_epoch = 0;
    // live streams (grail_stream_open_live): the stream owns its batch, whose segments sit in per-utterance rings
    std::unique_ptr<grail_batch> own;
    uint32_t ring_cap = 0;            // segments per utterance ring (a power of two); 0: not a live stream
    grail::host::DeviceBuffer<uint32_t> d_counts;     // [n_utt] segments appended so far
    grail::host::DeviceBuffer<uint32_t> d_open;       // [n_utt] 1 while the utterance's source may deliver more
    grail::host::DeviceBuffer<uint32_t> d_consumed;   // [n_utt] segments the Sequencer has pulled (written by the kernels)
    std::vector<uint32_t> appended;   // host copy of d_counts
    std::vector<uint32_t> consumed;   // what the host last read of d_consumed (a lower bound)
    std::vector<uint8_t> open;        // host copy of d_open
    std::vector<grail_synthesis_elem> last_elem;   // elem mode: the last elem appended per utterance (sharpness of the next pair)
    std::vector<uint8_t> last_has;
    // staging of an append (kept: an interactive front end appends a phoneme every half second for hours)
    grail::host::DeviceBuffer<grail::DevSeg> d_new;
    grail::host::DeviceBuffer<float> d_new_elems;
    grail::host::DeviceBuffer<uint32_t> d_new_offs;
    // ... on the host side two pinned buffers in turn, each with the event behind its last upload: an append returns as
    // soon as its copies and its scatter kernel are queued, and waits only for the append before last (not for every
    // kernel queued on the stream) before it writes into a buffer again
    grail::host::PinnedBuffer h_stage[2];
    grail::host::Event ev_stage[2];
    bool stage_busy[2] = {false, false};
    int stage_next = 0;
};

// A set of FIR filters (transforms.cpp; the image and its descriptors are fir_plan.cpp's): owned by the context's
// TransformState, released by grail_fir_free or with the context.
struct grail_fir {
    uint32_t n_filters = 0;
    uint32_t tail_max = 0;            // the largest n_taps - 1 - origin of the set: how far a row rings out
    std::vector<double> image;        // (host copies, kept while the upload may be in flight)
    std::vector<uint32_t> desc;
    grail::host::DeviceBuffer<double> d_taps;     // every filter's taps, binary64, padded to a multiple of 8
    grail::host::DeviceBuffer<uint32_t> d_desc;   // [n_filters][FIR_DESC_WORDS]
    uint32_t taps_max = 0;            // the longest n_taps of the set (a stream's ring holds taps_max - 1 samples a row)
};

// What the three kinds of chunked stream on finished rows hold alike (transform_streams.cpp): rows that each keep a ring of
// their last samples in device memory, and units (rows, or groups of rows) that each keep their state words there.  The kind's
// kernels read and write both.  Owned by the context's TransformState, released by the kind's close or with the context.
struct ChunkedStream {
    uint32_t n_rows = 0;
    uint32_t units = 0;               // whose the state words and the marks are: the rows, or a limit stream's n_rows / group groups
    uint32_t ring_cap = 0;            // samples of a row's ring (a power of two: the kind's *_stream_ring_capacity)
    grail::host::DeviceBuffer<uint64_t> d_state;    // [units][the kind's words]; word 0: samples fed, bit 63: the unit has ended
    grail::host::DeviceBuffer<float> d_ring;        // [n_rows][ring_cap]
    // a finishing call's marks: the host copy is written again only once the upload before has been through
    std::vector<uint8_t> mark;
    grail::host::DeviceBuffer<uint8_t> d_mark;      // [units]
    grail::host::Event ev_mark;       // behind the last upload of the marks (made at the first)
};

// A stream of rows filtered call by call (fir_kernels.hip): one state word a row.
struct grail_filter_stream : ChunkedStream {
    const grail_fir *set = nullptr;   // (a set with open streams is not freed); ring_cap is fir_stream_ring_capacity(set->taps_max)
    grail::host::RowIndex filter;     // the rows' filters
};

// A stream of rows resampled call by call (resample_kernels.hip), all on one pair of rates: three state words a row (samples
// fed, the next output's input time, its phase).  The table is the stream's own copy: the context's cache of four pairs may
// evict the pair while the stream is open.
struct grail_resample_stream : ChunkedStream {
    uint32_t up = 0, down = 0, taps = 0;    // ring_cap is resample_stream_ring_capacity(taps)
    std::vector<int32_t> table;       // (host copy, kept while the upload may be in flight)
    grail::host::DeviceBuffer<int32_t> d_table;     // [up][taps]
};

// A stream of groups of rows limited call by call (the stream kernels of limiter_kernels.hip), all under one ceiling with one
// look-ahead: one state word a group.
struct grail_limit_stream : ChunkedStream {
    uint32_t group = 1;
    float ceiling = 0.0f;
    uint32_t ell = 0;                 // lookahead_log2; ring_cap is limit_stream_ring_capacity(ell)
};

// A stream of rows metered call by call (meter_stream_kernels.hip), all at one rate with one set of K-weighting coefficients:
// METER_STREAM_STATE_WORDS state words a row (samples fed, s1 .. s4, acc, the running true peak, the hops completed), a ring of
// METER_STREAM_RING samples a row, and the ledger of the rows' hop sums, which the read kernel gates.
struct grail_meter_stream : ChunkedStream {
    uint32_t sample_rate = 0, hop = 0;      // hop = sample_rate / 10
    uint64_t max_hops = 0;                  // the ledger's capacity a row, fixed at open
    double coef[10] = {};
    grail::host::DeviceBuffer<double> d_ledger;     // [n_rows][max_hops]
};

// A set of recursive filters (transforms.cpp; the image is iir_plan.cpp's): owned by the context's TransformState, released by
// grail_iir_free or with the context.
struct grail_iir {
    uint32_t n_filters = 0;
    uint32_t bound = 1;               // the set's largest S rounded up to 1, 2, 4 or 8: the kernel instantiation that serves it
    std::vector<double> image;        // (host copies, kept while the upload may be in flight)
    std::vector<uint32_t> sections;
    grail::host::DeviceBuffer<double> d_image;        // [n_filters][IIR_IMAGE_DOUBLES]
    grail::host::DeviceBuffer<uint32_t> d_sections;   // [n_filters]
    // the filters' block matrices, made at the set's first grail_biquad_blocked_async (iir_block_image; empty before it)
    std::vector<double> block_image;
    grail::host::DeviceBuffer<double> d_block;        // [n_filters][16][16]
};

// A stream of rows filtered recursively call by call (iir_kernels.hip): iir_stream_state_words(set->bound) state words a row
// (samples fed, then s1, s2 of each section), no ring (ring_cap 0: a recursive filter's memory is its state).
struct grail_iir_stream : ChunkedStream {
    const grail_iir *set = nullptr;   // (a set with open streams is not freed)
    uint32_t tail = 0;                // the outputs a row rings out over at its finish
    grail::host::RowIndex filter;     // the rows' filters
};

// A set of gain curves with their ballistics (transforms.cpp; the image is dyn_plan.cpp's): owned by the context's TransformState,
// released by grail_dyn_free or with the context.
struct grail_dyn {
    uint32_t n_curves = 0;
    std::vector<double> image;        // (host copies, kept while the upload may be in flight)
    std::vector<double> alpha;
    std::vector<uint32_t> detector;
    grail::host::DeviceBuffer<double> d_image;        // [n_curves][DYN_IMAGE_DOUBLES]
    grail::host::DeviceBuffer<double> d_alpha;        // [n_curves][2]
    grail::host::DeviceBuffer<uint32_t> d_detector;   // [n_curves]
};

// A set for short-time spectra (transforms.cpp; the checks and the image are spectrum_plan.cpp's): owned by the context's
// TransformState, released by grail_spectrum_free or with the context.  No stream is ever open on one.
struct grail_spectrum {
    grail::SpectrumFacts facts;
    std::vector<float> window;        // (host copies, kept while the upload may be in flight)
    std::vector<double> twiddles;
    std::vector<uint32_t> desc;
    std::vector<float> weights;
    grail::host::DeviceBuffer<float> d_window;        // [n_window]
    grail::host::DeviceBuffer<double> d_twiddles;     // [N/2] pairs (re, im)
    grail::host::DeviceBuffer<uint32_t> d_desc;       // [max(n_bands, 1)][SPECTRUM_BAND_WORDS]
    grail::host::DeviceBuffer<float> d_weights;       // the bands' weights one after another
};

// A stream of rows compressed call by call (dyn_kernels.hip): DYN_STREAM_STATE_WORDS state words a row (samples fed, then the
// envelope's bits), no ring (ring_cap 0: the envelope is all a row remembers), no marks (a row never ends).
struct grail_dyn_stream : ChunkedStream {
    const grail_dyn *set = nullptr;   // (a set with open streams is not freed)
    uint32_t n_keys = 0;              // 0: self-keyed
    grail::host::RowIndex curve;      // the rows' curves
    grail::host::RowIndex key_row;    // ... and keys (a keyed stream's; empty otherwise)
};

// What the launch policy reads of a batch, or of a row group of one: host facts only (copyable; grail_plan_ragged_blocks
// builds one without a device)
struct BatchFacts {
    uint32_t n_utt = 0;
    uint32_t n_segs = 0;
    uint32_t max_voice_id = 0;
    bool phoneme_mode = true;
    bool any_blend = false;    // some segment's blend length is not +-2^k (selects the kernel)
    bool plain = false;        // every length / blend length / pitch finite, blend lengths > 0
    float max_seconds = 0.0f;  // longest utterance: sum of its segment lengths
    float min_length = 0.0f;   // shortest segment (plain batches)
    float min_pitch = 0.0f;    // lowest frequency.min(0.5) of any segment (plain batches)
    uint64_t len_bound_epoch = 0;      // the device holds an upper bound of every utterance's length (plain batches; time-split
                                       // kernels) for the voice table of this epoch (its highest sample rate); epochs are unique
                                       // in the process, so a context other than the uploader never matches
    bool len_bound_known = false;      // (the planner's question; grail_plan_ragged_blocks answers it without a device)
    double elems_sharpness = 0.0;   // elem mode: predicted fast-mode deviation of the caller's elems (elems_sharpness())
    uint32_t elems_warmup = 0;      // elem mode: warm-up length of the time-split kernels over the batch's distinct elems and the
                                    // jitter of the voices it names (elems_warmup()); 0: the batch does not qualify
    uint64_t elems_warmup_epoch = 0;   // ... computed against this voice table (voices_epoch)
    bool elems_live4_ok = false;    // elem mode: formants 5-8 of every elem (and the voices named) can be left out (live4_ok); same epoch
    bool elems_scan_ok = false;     // elem mode: every elem inside the scan kernel's window (scan_elems_ok), pitches <= 1/2; same epoch
    std::vector<uint32_t> used_voices;   // the distinct voice ids of the batch, ascending
    // Ragged (length-sorted) batches, per granule of 8 consecutive launch slots: the longest row in samples (at the
    // context's highest rate), the rows' segments and their kinks of alpha (blend_length < length) — what ragged_plan()
    // weighs the lane mappings with.  Empty for aligned batches.
    std::vector<float> granule_samples;
    std::vector<uint32_t> granule_segs, granule_kinks;
};

// Row groups (whole-batch launches of length-sorted batches).  A few rows that the lean kernel families cannot take —
// a segment shorter than two samples, a non-finite length or pitch — would cost the whole batch its four-formant
// kernels, pipelined workgroups and fast families, because those are gated on the batch's worst row.  Such rows are
// put LAST in the slot order and the batch is planned as two: groups[0] = the lean rows (launch slots [0, groups[0].n_utt)),
// groups[1] = the rest, each with the summary of its own rows (used_voices: the batch's — a superset of the group's) and a
// cached plan of its own.  The device arrays are the batch's.
struct RowGroup : BatchFacts {
    uint32_t slot0 = 0;               // its first launch slot
    mutable grail::host::PlanCache plan_cache;
};

// A block of a ragged batch in PACKED launch order (dispatch_model.cpp, "The workgroup dispatcher"): the slot -> utterance table
// of rows [slot0, slot0 + rows) with its workgroups re-ordered, on the device.  Kept by the batch and never reallocated while
// it lives (a kernel of another context may still be reading it), freed with it.
struct PackedPerm {
    uint32_t view = 0;                // whose block: 0 the batch as a whole, 1 + g its row group g
    uint32_t slot0 = 0, rows = 0, per_block = 0, cus = 0;
    uint32_t family = 0;              // L | fast << 8 | live4 << 16: what the workgroups' costs were priced for
    grail::host::DeviceBuffer<uint32_t> d_perm;   // [rows]; none: the plain order is as good (remembered, so that it is not packed again)
    double model_ms = 0.0, plain_ms = 0.0;
};

// The facts are those of all rows; the device arrays are owned (`delete batch` releases everything; an array that was never
// allocated reads nullptr: "no ids: voice 0 for all", "no perm").
struct grail_batch : BatchFacts {
    grail::host::DeviceBuffer<grail::DevSeg> d_segs;
    grail::host::DeviceBuffer<uint32_t> d_offsets, d_voice_ids, d_seeds;
    grail::host::DeviceBuffer<uint32_t> d_perm;       // ragged batches: launch slot -> utterance, longest first
    std::vector<uint32_t> perm_host;                  // ... its host copy (packed launch orders are cut from it)
    grail::host::DeviceBuffer<uint32_t> d_len_bound;  // per utterance: an upper bound of its length in samples (len_bound_epoch)
    grail::host::DeviceBuffer<float> d_elems;         // elem mode only
    std::vector<RowGroup> groups;                     // none or two; valid for the voice table they were judged against
    uint64_t groups_epoch = 0;
    // one batch may be rendered by several contexts, each on a thread of its own: `lock` guards what a launch writes
    mutable std::mutex lock;
    mutable grail::host::PlanCache plan_cache;        // of the batch as a whole
    mutable std::vector<PackedPerm> packed;           // blocks in packed launch order, made at their first launch
};
static_assert(!std::is_copy_constructible_v<grail_batch>, "a batch owns its device arrays: row groups are BatchFacts, not batches");

#include "launch_plan.h"

namespace grail {
namespace host {

int bind(grail_ctx *ctx);
// ... for the device entry points that say their own name (levels.cpp, transforms.cpp, transform_streams.cpp): without a context, why there is none,
// GRAIL_ERR_NO_DEVICE on a machine without a GPU
int bind_device(grail_ctx *ctx, const char *who);

// grail_api.cpp
void name_voices(BatchFacts &b, const uint32_t *voice_ids, uint32_t n_utt);
bool blend_is_pow2(float blend_length);
int check_offsets(const uint32_t *seg_offsets, uint32_t n_utt, uint32_t *n_segs);
int install_voices(grail_ctx *ctx, const grail_voice *voices, uint32_t n_voices);
int check_ready(grail_ctx *ctx, const grail_batch *batch);

// voice_analysis.cpp: what a voice qualifies for (four-formant kernels, scan kernel, time-split warm-up), the predicted
// deviation of fast arithmetic (sharpness), the tier a batch is served in, the chunk grid of a time-split launch
bool live4_ok(const grail_voice &v);
bool live4_elems_ok(const grail_synthesis_elem *elems, size_t n_elems, float jitter_delta_formant_frequency);
bool scan_voice_ok(const grail_voice &v);
bool scan_elems_ok(const grail_synthesis_elem *elems, size_t n_elems, float jitter_delta_formant_frequency);
uint32_t voice_warmup(const grail_voice &v);
uint32_t elems_warmup(const grail_synthesis_elem *elems, size_t n_elems, double jitter_delta_formant_frequency);
double elems_sharpness(const grail_synthesis_elem *elems, size_t n);
double batch_sharpness(const PlanEnv *ctx, const BatchFacts *batch);
int fast_tier_for(const PlanEnv *ctx, const BatchFacts *batch, int arithmetic);
int fast_tier(const PlanEnv *ctx, const BatchFacts *batch);
bool split_grid(uint32_t span, uint32_t warmup, int K, double r, uint32_t *b);

// synthesize.cpp: one launch per block; a batch's cached plan
// what every synthesis launch takes from (ctx, batch): the batch's arrays from utterance row0 on, the voice table, the flags
void batch_args(const grail_ctx *ctx, const grail_batch *batch, uint32_t row0, SynthArgs &a);
int synthesize_rows(grail_ctx *ctx, const grail_batch *batch, float *out_dev, int16_t *out_pcm16_dev, uint64_t out_stride,
                    uint32_t *out_len_dev, uint32_t first = 0, uint32_t count = 0, uint32_t family_rows = 0);

// comm.cpp: the one thing grail_destroy releases by name
void comm_release(grail_ctx *ctx);
// host_output.cpp: grail_batch_free for a call that made the batch itself; returns rc, and grail_last_error() stays rc's
int drop_batch(grail_ctx *ctx, grail_batch *batch, int rc);
// levels.cpp, for grail_batch_mix_leveled: the rows of one rendered block measured on ctx's stream and their numbers
// brought to the host (one wait), then the items' gains by grail_level_gains; gains[n_items], *n_unleveled is added to.
// sample_rate is read in GRAIL_LEVEL_LOUDNESS only (level_table_rate).  ceiling_db (NULL: none) is
// grail_batch_mix_leveled_limited's: the rows' true peaks are measured too and grail_true_peak_limit_gains caps the gains;
// *n_limited is added to.
int level_block_gains(grail_ctx *ctx, int mode, uint32_t sample_rate, const float *rows_dev, uint64_t row_stride,
                      const uint32_t *len_dev, const uint32_t *row_len, uint32_t n_rows, const uint32_t *item_rows,
                      const float *item_level_db, uint32_t n_items, float *gains, uint32_t *n_unleveled,
                      const float *ceiling_db, uint32_t *n_limited);
// the one whole-numbered sample rate of ctx's voice table within GRAIL_LOUDNESS_RATE_MIN .. _MAX, or 0 if it has none
uint32_t level_table_rate(const grail_ctx *ctx);
// host_output.cpp: texts -> PhonemeElems (grail_say_batch, grail_node_say_batch)
int say_segments(const std::vector<grail_voice> &voices, const char *const *texts_utf8, uint32_t n_texts,
                 const uint32_t *voice_ids, std::vector<grail_phoneme_elem> &segs, std::vector<uint32_t> &offs);
// comm.cpp: one communicator over the contexts of a node, formed inside the process (ncclCommInitAll)
int comm_init_all(grail_ctx *const *ctxs, const int *devices, uint32_t n);

}  // namespace host
}  // namespace grail
