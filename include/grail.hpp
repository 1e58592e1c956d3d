// grail.hpp — header-only C++ facade over the C ABI (grail_hip.h) that keeps the call shape of
// the grail-rs crate for this path:
//
//   Rust (reference examples/cli.rs:175-184)            C++ (this header)
//   text.chars().transcribe(lang).intonate(lang, v)  -> grail::phoneme_elems(v, text)
//       .select(v).sequence(v).jitter(seed, v)
//       .synthesize().collect::<Vec<f32>>()           -> gpu.synthesize({Utterance{...}})
//   voices::generic()                                 -> grail::voices::generic()
//   pulling the iterator a buffer at a time             -> grail::Stream(gpu, utterances, chunk).next(...)
//       (examples/interactive.rs:31-48)
//   a chain whose source delivers while it runs         -> grail::LiveStream(gpu, chunk).append(...) / .next()
//       (repeat_with(|| receiver.try_recv()...), interactive.rs:31)
//   the same one call over every GPU of the node        -> grail::Node({0, 1, ...}, voices).synthesize({...})
//
// No arithmetic lives here; everything forwards to libgrail_hip.so.
#pragma once

#include <algorithm>
#include <cstdint>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "grail_hip.h"

namespace grail {

using SynthesisElem = grail_synthesis_elem;  // src/lib.rs:316
using Voice = grail_voice;                   // src/lib.rs:696
using PhonemeElem = grail_phoneme_elem;      // src/lib.rs:961
using SequenceElem = grail_sequence_elem;    // src/lib.rs:814

enum class Phoneme : int32_t {               // src/lib.rs:632-649
    Silence = GRAIL_PH_SILENCE, Stop = GRAIL_PH_STOP, Glide = GRAIL_PH_GLIDE,
    A = GRAIL_PH_A, E = GRAIL_PH_E,
};

struct Error : std::runtime_error {
    int status;
    Error(int s, const std::string &what) : std::runtime_error(what), status(s) {}
};

inline void check(int status)
{
    if (status != GRAIL_OK) {
        const char *msg = grail_last_error();
        throw Error(status, (msg && *msg) ? msg : grail_status_string(status));
    }
}

namespace voices {
inline Voice generic() { Voice v; grail_voice_generic(&v); return v; }             // generic.rs:5
// predicted |fast - reference| of a voice, units of 2^-23 of max(1, peak); served up to GRAIL_FAST_SHARPNESS_LIMIT
inline float fast_sharpness(const Voice &voice) { return grail_fast_sharpness(&voice); }
inline Voice generic_at(float sample_rate) { Voice v; grail_voice_generic_at(&v, sample_rate); return v; }
}  // namespace voices

// text.chars().transcribe(languages::generic()).intonate(languages::generic(), voice)
inline std::vector<PhonemeElem> phoneme_elems(const Voice &voice, const std::string &text_utf8)
{
    uint32_t n = 0;
    check(grail_text_to_phoneme_elems(&voice, text_utf8.c_str(), nullptr, 0, &n));
    std::vector<PhonemeElem> out(n);
    if (n) check(grail_text_to_phoneme_elems(&voice, text_utf8.c_str(), out.data(), n, &n));
    return out;
}

struct Utterance {
    std::vector<PhonemeElem> phonemes;
    uint32_t voice = 0;
    uint32_t jitter_seed = 0;   // examples/cli.rs:182 uses 0
};

// Where an utterance goes in a mix (Gpu::mix): utterance `utterance` of the call, added into track `track` from track
// sample `offset` on, scaled by `gain`.  The C ABI takes the same as parallel arrays (grail_batch_mix).
struct Placement {
    uint32_t utterance = 0;
    uint32_t track = 0;
    uint64_t offset = 0;
    float gain = 1.0f;
};

// What Gpu::levels measures, one entry per row (grail_levels_async)
struct Levels {
    std::vector<double> sumsq;         // binary64 sum of squares of the finite samples
    std::vector<float> peak;           // largest finite |x|
    std::vector<uint32_t> nonfinite;   // NaN and Inf samples
};

// What Gpu::loudness measures, one entry per row (grail_loudness_async)
struct Loudness {
    std::vector<double> gated_ms;      // K-weighted gated mean square (BS.1770-4); 0 for a row shorter than 400 ms
    std::vector<uint32_t> nonfinite;   // NaN and Inf samples (they enter the filter as 0)
    double lufs(size_t row) const { return grail_loudness_lufs(gated_ms[row]); }
};

// What a meter reads from one row's hop sums (pure host): the largest mean square over windows of window_hops hops (4 =
// momentary, 30 = short-term; grail_loudness_lufs gives its LUFS), and the loudness range in LU (EBU Tech 3342)
inline double loudness_window_max(const std::vector<double> &hop_sumsq, uint32_t hop, uint32_t window_hops)
{
    return grail_loudness_window_max(hop_sumsq.data(), (uint32_t)hop_sumsq.size(), hop, window_hops);
}
inline double loudness_range(const std::vector<double> &hop_sumsq, uint32_t hop)
{
    return grail_loudness_range(hop_sumsq.data(), (uint32_t)hop_sumsq.size(), hop);
}

// What Gpu::track_loudness measures (grail_loudness_segmented_async): Loudness, and each row's hop sums (100 ms each)
struct TrackLoudness : Loudness {
    uint32_t hop = 0;                              // samples per hop: sample_rate / 10
    std::vector<std::vector<double>> hop_sumsq;    // per row, its floor(len / hop) hop sums
    double range(size_t row) const { return loudness_range(hop_sumsq[row], hop); }                       // LU
    double momentary_max(size_t row) const { return grail_loudness_lufs(loudness_window_max(hop_sumsq[row], hop, 4)); }
    double short_term_max(size_t row) const { return grail_loudness_lufs(loudness_window_max(hop_sumsq[row], hop, 30)); }
};

// What Gpu::true_peak measures, one entry per row (grail_true_peak_async)
struct TruePeak {
    std::vector<double> true_peak;     // largest |y| of the row oversampled four times (BS.1770-4 Annex 2); 0 for an empty row
    std::vector<uint32_t> nonfinite;   // NaN and Inf samples (they enter the filter as 0)
    double db(size_t row) const { return grail_true_peak_db(true_peak[row]); }
};

// What Gpu::limit gives: the limited rows, and one entry per group of rows (grail_limit_async)
struct Limited {
    std::vector<std::vector<float>> rows;   // as long as they came; the rows of a refused group come back empty
    std::vector<float> min_gain;            // the smallest gain of the group; NaN for a refused group
    std::vector<uint32_t> n_limited;        // samples whose gain is below 1; GRAIL_LIMIT_REFUSED for a refused group
    std::vector<uint32_t> nonfinite;        // NaN and Inf samples of the group's rows (they are written as 0)
    bool refused(size_t group) const { return n_limited[group] == GRAIL_LIMIT_REFUSED; }
};

// The float that a ceiling in dBTP is to Gpu::limit (grail_limit_ceiling)
inline float limit_ceiling(float ceiling_db) { return grail_limit_ceiling(ceiling_db); }

// One FIR filter: its taps and the tap that sits at time zero (0: causal; (K - 1) / 2: linear phase, zero delay)
struct Fir {
    std::vector<float> taps;
    uint32_t origin = 0;
};

// The Kaiser-windowed band-pass lo_hz .. hi_hz at sample_rate, n_taps odd (grail_fir_design; lo_hz = 0: a low-pass,
// hi_hz = sample_rate / 2: a high-pass), with the origin that gives it zero delay
inline Fir fir_design(uint32_t sample_rate, double lo_hz, double hi_hz, uint32_t n_taps = 255)
{
    Fir f;
    f.taps.resize(n_taps ? n_taps : 1);
    check(grail_fir_design(sample_rate, lo_hz, hi_hz, n_taps, f.taps.data()));
    f.origin = (n_taps - 1) / 2;
    return f;
}

// A set of filters on a Gpu's device (grail_fir_create), made by Gpu::fir_set: move-only, released with grail_fir_free.
// It must not outlive its Gpu.
class FirSet {
public:
    FirSet(grail_ctx *ctx, const std::vector<Fir> &filters) : ctx_(ctx)
    {
        std::vector<float> taps;
        std::vector<uint32_t> n_taps, origin;
        for (const Fir &f : filters) {
            taps.insert(taps.end(), f.taps.begin(), f.taps.end());
            n_taps.push_back((uint32_t)f.taps.size());
            origin.push_back(f.origin);
            tail_ = std::max<uint64_t>(tail_, f.taps.size() > f.origin ? f.taps.size() - 1 - f.origin : 0);
            longest_ = std::max<uint32_t>(longest_, (uint32_t)f.taps.size());
        }
        check(grail_fir_create(ctx, taps.data(), n_taps.data(), origin.data(), (uint32_t)filters.size(), &set_));
    }
    ~FirSet() { grail_fir_free(ctx_, set_); }
    FirSet(FirSet &&o) noexcept : ctx_(o.ctx_), set_(std::exchange(o.set_, nullptr)), tail_(o.tail_), longest_(o.longest_) {}
    FirSet &operator=(FirSet &&o) noexcept
    {
        if (this != &o) {
            grail_fir_free(ctx_, set_);
            ctx_ = o.ctx_, set_ = std::exchange(o.set_, nullptr), tail_ = o.tail_, longest_ = o.longest_;
        }
        return *this;
    }
    FirSet(const FirSet &) = delete;
    FirSet &operator=(const FirSet &) = delete;
    const grail_fir *get() const { return set_; }
    uint64_t tail() const { return tail_; }     // the longest n_taps - 1 - origin: how far a row rings out
    uint32_t longest() const { return longest_; }   // the most taps of a filter of the set

private:
    grail_ctx *ctx_ = nullptr;
    grail_fir *set_ = nullptr;
    uint64_t tail_ = 0;
    uint32_t longest_ = 1;
};

namespace detail {
// the stride that holds the longest of a call's chunks, a multiple of 64 (no chunks, a finishing call: 0)
inline uint64_t chunk_stride(const std::vector<std::vector<float>> *chunks)
{
    size_t longest = 0;
    if (chunks)
        for (const auto &c : *chunks) longest = c.size() > longest ? c.size() : longest;
    return (longest + 63) / 64 * 64;
}

// One call on a stream of n rows, there and back: the rows' chunks (NULL: a finishing call, nothing goes in) and their lengths
// to device buffers of `stride` samples a row, entry(in, stride, len, out, out_stride, out_len) for the entry point, which writes
// at most `room` samples a row and one length per `group` rows, and each row cut at its length (none for a length of 0, or of
// a unit that was refused).  Everything is freed before a failure is thrown.
template <typename Entry>
std::vector<std::vector<float>> stream_round_trip(grail_ctx *ctx, uint32_t n, uint32_t group, const std::vector<std::vector<float>> *chunks,
                                                  uint64_t stride, uint64_t room, Entry entry)
{
    const uint32_t units = n / group;
    const uint64_t out_stride = (room + 63) / 64 * 64;
    std::vector<std::vector<float>> out(n);
    std::vector<uint32_t> lens(n, 0u), out_lens(units, 0u);
    for (uint32_t i = 0; chunks && i < n; ++i) lens[i] = (uint32_t)(*chunks)[i].size();
    void *d_in = nullptr, *d_out = nullptr, *d_len = nullptr, *d_out_len = nullptr;
    int rc = grail_device_alloc(ctx, (size_t)n * stride * 4 + 4, &d_in);
    if (!rc) rc = grail_device_alloc(ctx, (size_t)n * out_stride * 4 + 4, &d_out);
    if (!rc) rc = grail_device_alloc(ctx, (size_t)n * 4, &d_len);
    if (!rc) rc = grail_device_alloc(ctx, (size_t)units * 4, &d_out_len);
    for (uint32_t i = 0; !rc && i < n; ++i)
        if (lens[i]) rc = grail_memcpy_h2d(ctx, (float *)d_in + (size_t)i * stride, (*chunks)[i].data(), (size_t)lens[i] * 4);
    if (!rc) rc = grail_memcpy_h2d(ctx, d_len, lens.data(), (size_t)n * 4);
    if (!rc) rc = entry((const float *)d_in, stride, (const uint32_t *)d_len, (float *)d_out, out_stride, (uint32_t *)d_out_len);
    if (!rc) rc = grail_memcpy_d2h(ctx, out_lens.data(), d_out_len, (size_t)units * 4);
    for (uint32_t i = 0; !rc && i < n; ++i) {
        const uint32_t len = out_lens[i / group];
        if (!len || len == GRAIL_LIMIT_REFUSED) continue;
        out[i].resize(len);
        rc = grail_memcpy_d2h(ctx, out[i].data(), (const float *)d_out + (size_t)i * out_stride, (size_t)len * 4);
    }
    for (void *p : {d_in, d_out, d_len, d_out_len})
        if (p) grail_device_free(ctx, p);
    check(rc);
    return out;
}
}  // namespace detail

// Rows filtered chunk by chunk on a Gpu's device (grail_filter_stream_open; the contract is the header's section "levels,
// continued: FIR filtering of streams"), made by Gpu::fir_stream: move-only, closed with grail_filter_stream_close.  The
// chunks' outputs put end to end, then the tails of finish(), are the bits Gpu::fir gives for the whole rows.  It must not
// outlive its FirSet, which cannot be freed before it.
class FirStream {
public:
    FirStream(grail_ctx *ctx, const FirSet &set, uint32_t n_rows, const std::vector<uint32_t> &which = {})
        : ctx_(ctx), n_rows_(n_rows), tail_(set.longest() - 1)
    {
        if (!which.empty() && which.size() != n_rows) throw Error(GRAIL_ERR_INVALID_ARG, "fir_stream: one filter index per row");
        check(grail_filter_stream_open(ctx, set.get(), n_rows, which.empty() ? nullptr : which.data(), &fs_));
    }
    ~FirStream() { grail_filter_stream_close(ctx_, fs_); }
    FirStream(FirStream &&o) noexcept : ctx_(o.ctx_), fs_(std::exchange(o.fs_, nullptr)), n_rows_(o.n_rows_), tail_(o.tail_) {}
    FirStream &operator=(FirStream &&o) noexcept
    {
        if (this != &o) {
            grail_filter_stream_close(ctx_, fs_);
            ctx_ = o.ctx_, fs_ = std::exchange(o.fs_, nullptr), n_rows_ = o.n_rows_, tail_ = o.tail_;
        }
        return *this;
    }
    FirStream(const FirStream &) = delete;
    FirStream &operator=(const FirStream &) = delete;
    uint32_t rows() const { return n_rows_; }
    uint32_t tail() const { return tail_; }      // the set's longest n_taps - 1: the room finish() needs per row

    // grail_filter_stream_next_async on device buffers (a chunk that grail_stream_next_async has just rendered, say): queued on
    // the context's stream, nothing leaves the device
    void next_async(const float *in_dev, uint64_t in_stride, const uint32_t *in_len_dev, float *out_dev, uint64_t out_stride,
                    uint32_t *out_len_dev, uint32_t *nonfinite_dev = nullptr)
    {
        check(grail_filter_stream_next_async(ctx_, fs_, in_dev, in_stride, in_len_dev, out_dev, out_stride, out_len_dev, nonfinite_dev));
    }

    // Row i is fed chunks[i] (an empty chunk: the row pauses); returns the outputs that became known, per row.  A row that
    // has ended and is fed comes back empty.
    std::vector<std::vector<float>> next(const std::vector<std::vector<float>> &chunks)
    {
        if (chunks.size() != n_rows_) throw Error(GRAIL_ERR_INVALID_ARG, "FirStream::next: one chunk per row");
        return call(&chunks, nullptr);
    }
    // The rows marked in which (empty: every row) end; returns their tails: what the filters still ring out.
    std::vector<std::vector<float>> finish(const std::vector<uint8_t> &which = {})
    {
        if (!which.empty() && which.size() != n_rows_) throw Error(GRAIL_ERR_INVALID_ARG, "FirStream::finish: one mark per row");
        return call(nullptr, which.empty() ? nullptr : which.data());
    }

private:
    std::vector<std::vector<float>> call(const std::vector<std::vector<float>> *chunks, const uint8_t *which)
    {
        const uint64_t stride = detail::chunk_stride(chunks);
        return detail::stream_round_trip(ctx_, n_rows_, 1, chunks, stride, std::max<uint64_t>(stride, tail_),
            [&](const float *in, uint64_t in_stride, const uint32_t *len, float *out, uint64_t out_stride, uint32_t *out_len) {
                return chunks ? grail_filter_stream_next_async(ctx_, fs_, in, in_stride, len, out, out_stride, out_len, nullptr)
                              : grail_filter_stream_finish_async(ctx_, fs_, which, out, out_stride, out_len);
            });
    }

    grail_ctx *ctx_ = nullptr;
    grail_filter_stream *fs_ = nullptr;
    uint32_t n_rows_ = 0, tail_ = 0;
};

// Rows resampled chunk by chunk on a Gpu's device (grail_resample_stream_open; the contract is the header's section "levels,
// continued: sample-rate conversion of streams"), made by Gpu::resample_stream: move-only, closed with
// grail_resample_stream_close.  The chunks' outputs put end to end, then the tails of finish(), are the bits Gpu::resample
// gives for the whole rows.  It must not outlive its Gpu.
class ResampleStream {
public:
    ResampleStream(grail_ctx *ctx, uint32_t rate_in, uint32_t rate_out, uint32_t n_rows)
        : ctx_(ctx), rate_in_(rate_in), rate_out_(rate_out), n_rows_(n_rows)
    {
        uint32_t up = 0, down = 0, taps = 0;
        check(grail_resample_ratio(rate_in, rate_out, &up, &down, &taps));
        tail_ = most(taps / 2);
        check(grail_resample_stream_open(ctx, rate_in, rate_out, n_rows, &rs_));
    }
    ~ResampleStream() { grail_resample_stream_close(ctx_, rs_); }
    ResampleStream(ResampleStream &&o) noexcept
        : ctx_(o.ctx_), rs_(std::exchange(o.rs_, nullptr)), rate_in_(o.rate_in_), rate_out_(o.rate_out_), n_rows_(o.n_rows_), tail_(o.tail_)
    {
    }
    ResampleStream &operator=(ResampleStream &&o) noexcept
    {
        if (this != &o) {
            grail_resample_stream_close(ctx_, rs_);
            ctx_ = o.ctx_, rs_ = std::exchange(o.rs_, nullptr), rate_in_ = o.rate_in_, rate_out_ = o.rate_out_;
            n_rows_ = o.n_rows_, tail_ = o.tail_;
        }
        return *this;
    }
    ResampleStream(const ResampleStream &) = delete;
    ResampleStream &operator=(const ResampleStream &) = delete;
    uint32_t rows() const { return n_rows_; }
    uint64_t tail() const { return tail_; }      // ceil(h up / down): the room finish() needs per row
    // ceil(n up / down): the room a call that feeds rows of stride n needs per row (grail_resample_len)
    uint64_t most(uint64_t n) const
    {
        uint64_t out = 0;
        check(grail_resample_len(n, rate_in_, rate_out_, &out));
        return out;
    }

    // grail_resample_stream_next_async on device buffers (a chunk that a live stream has just rendered or a filter stream has
    // just written, say): queued on the context's stream, nothing leaves the device
    void next_async(const float *in_dev, uint64_t in_stride, const uint32_t *in_len_dev, float *out_dev, uint64_t out_stride,
                    uint32_t *out_len_dev, uint32_t *nonfinite_dev = nullptr)
    {
        check(grail_resample_stream_next_async(ctx_, rs_, in_dev, in_stride, in_len_dev, out_dev, out_stride, out_len_dev, nonfinite_dev));
    }

    // Row i is fed chunks[i] (an empty chunk: the row pauses); returns the outputs that became known, per row.  A row that
    // has ended and is fed comes back empty.
    std::vector<std::vector<float>> next(const std::vector<std::vector<float>> &chunks)
    {
        if (chunks.size() != n_rows_) throw Error(GRAIL_ERR_INVALID_ARG, "ResampleStream::next: one chunk per row");
        return call(&chunks, nullptr);
    }
    // The rows marked in which (empty: every row) end; returns their tails: the outputs that still read samples fed.
    std::vector<std::vector<float>> finish(const std::vector<uint8_t> &which = {})
    {
        if (!which.empty() && which.size() != n_rows_) throw Error(GRAIL_ERR_INVALID_ARG, "ResampleStream::finish: one mark per row");
        return call(nullptr, which.empty() ? nullptr : which.data());
    }

private:
    std::vector<std::vector<float>> call(const std::vector<std::vector<float>> *chunks, const uint8_t *which)
    {
        const uint64_t stride = detail::chunk_stride(chunks);
        return detail::stream_round_trip(ctx_, n_rows_, 1, chunks, stride, std::max<uint64_t>(most(stride), tail_),
            [&](const float *in, uint64_t in_stride, const uint32_t *len, float *out, uint64_t out_stride, uint32_t *out_len) {
                return chunks ? grail_resample_stream_next_async(ctx_, rs_, in, in_stride, len, out, out_stride, out_len, nullptr)
                              : grail_resample_stream_finish_async(ctx_, rs_, which, out, out_stride, out_len);
            });
    }

    grail_ctx *ctx_ = nullptr;
    grail_resample_stream *rs_ = nullptr;
    uint32_t rate_in_ = 0, rate_out_ = 0, n_rows_ = 0;
    uint64_t tail_ = 0;
};

// Groups of rows limited chunk by chunk on a Gpu's device (grail_limit_stream_open; the contract is the header's section
// "levels, continued: the limiter on streams"), made by Gpu::limit_stream: move-only, closed with grail_limit_stream_close.
// The chunks' outputs put end to end, then the tails of finish(), are the bits Gpu::limit gives for the whole rows, delay()
// samples late.  It must not outlive its Gpu.
class LimitStream {
public:
    LimitStream(grail_ctx *ctx, uint32_t n_rows, uint32_t group, float ceiling, uint32_t lookahead_log2)
        : ctx_(ctx), n_rows_(n_rows), group_(group)
    {
        check(grail_limit_stream_open(ctx, n_rows, group, ceiling, lookahead_log2, &ls_));
        delay_ = GRAIL_LIMIT_STREAM_DELAY(lookahead_log2);
    }
    ~LimitStream() { grail_limit_stream_close(ctx_, ls_); }
    LimitStream(LimitStream &&o) noexcept
        : ctx_(o.ctx_), ls_(std::exchange(o.ls_, nullptr)), n_rows_(o.n_rows_), group_(o.group_), delay_(o.delay_)
    {
    }
    LimitStream &operator=(LimitStream &&o) noexcept
    {
        if (this != &o) {
            grail_limit_stream_close(ctx_, ls_);
            ctx_ = o.ctx_, ls_ = std::exchange(o.ls_, nullptr), n_rows_ = o.n_rows_, group_ = o.group_, delay_ = o.delay_;
        }
        return *this;
    }
    LimitStream(const LimitStream &) = delete;
    LimitStream &operator=(const LimitStream &) = delete;
    uint32_t rows() const { return n_rows_; }
    uint32_t groups() const { return n_rows_ / group_; }
    uint32_t delay() const { return delay_; }    // GRAIL_LIMIT_STREAM_DELAY: the output's lag, and the room finish() needs per row

    // grail_limit_stream_next_async on device buffers (a chunk that a live stream has just rendered or a filter stream has
    // just written, say): queued on the context's stream, nothing leaves the device.  The results are per group.
    void next_async(const float *in_dev, uint64_t in_stride, const uint32_t *in_len_dev, float *out_dev, uint64_t out_stride,
                    uint32_t *out_len_dev, float *min_gain_dev = nullptr, uint32_t *n_limited_dev = nullptr,
                    uint32_t *nonfinite_dev = nullptr)
    {
        check(grail_limit_stream_next_async(ctx_, ls_, in_dev, in_stride, in_len_dev, out_dev, out_stride, out_len_dev, min_gain_dev,
                                            n_limited_dev, nonfinite_dev));
    }
    // grail_limit_stream_finish_async on a device buffer (out_stride >= delay())
    void finish_async(float *out_dev, uint64_t out_stride, uint32_t *out_len_dev, const uint8_t *which = nullptr)
    {
        check(grail_limit_stream_finish_async(ctx_, ls_, which, out_dev, out_stride, out_len_dev, nullptr, nullptr));
    }

    // Row i is fed chunks[i] (empty chunks: the group pauses); returns the outputs that became known, per row.  The rows of
    // a group whose members are fed different lengths, or that has ended and is fed, come back empty.
    std::vector<std::vector<float>> next(const std::vector<std::vector<float>> &chunks)
    {
        if (chunks.size() != n_rows_) throw Error(GRAIL_ERR_INVALID_ARG, "LimitStream::next: one chunk per row");
        return call(&chunks, nullptr);
    }
    // The groups marked in which (empty: every group) end; returns their rows' tails: the last delay() outputs at most.
    std::vector<std::vector<float>> finish(const std::vector<uint8_t> &which = {})
    {
        if (!which.empty() && which.size() != groups()) throw Error(GRAIL_ERR_INVALID_ARG, "LimitStream::finish: one mark per group");
        return call(nullptr, which.empty() ? nullptr : which.data());
    }

private:
    // (one length per group)
    std::vector<std::vector<float>> call(const std::vector<std::vector<float>> *chunks, const uint8_t *which)
    {
        const uint64_t stride = detail::chunk_stride(chunks);
        return detail::stream_round_trip(ctx_, n_rows_, group_, chunks, stride, std::max<uint64_t>(stride, delay_),
            [&](const float *in, uint64_t in_stride, const uint32_t *len, float *out, uint64_t out_stride, uint32_t *out_len) {
                return chunks ? grail_limit_stream_next_async(ctx_, ls_, in, in_stride, len, out, out_stride, out_len, nullptr, nullptr, nullptr)
                              : grail_limit_stream_finish_async(ctx_, ls_, which, out, out_stride, out_len, nullptr, nullptr);
            });
    }

    grail_ctx *ctx_ = nullptr;
    grail_limit_stream *ls_ = nullptr;
    uint32_t n_rows_ = 0, group_ = 1, delay_ = 0;
};

namespace detail {
inline void flatten(const std::vector<Utterance> &utts, std::vector<PhonemeElem> &segs, std::vector<uint32_t> &offs,
                    std::vector<uint32_t> &vids, std::vector<uint32_t> &seeds)
{
    offs.assign(1, 0u);
    for (const Utterance &u : utts) {
        segs.insert(segs.end(), u.phonemes.begin(), u.phonemes.end());
        offs.push_back((uint32_t)segs.size());
        vids.push_back(u.voice);
        seeds.push_back(u.jitter_seed);
    }
}
}  // namespace detail

// One GPU and its voice table.
class Gpu {
public:
    Gpu(int device, const std::vector<Voice> &voices) : voices_(voices)
    {
        check(grail_create(device, &ctx_));
        const int rc = grail_set_voices(ctx_, voices_.data(), (uint32_t)voices_.size());
        if (rc != GRAIL_OK) {
            grail_destroy(ctx_);
            check(rc);
        }
    }
    ~Gpu() { grail_destroy(ctx_); }
    Gpu(const Gpu &) = delete;
    Gpu &operator=(const Gpu &) = delete;

    grail_ctx *ctx() const { return ctx_; }
    const std::vector<Voice> &voices() const { return voices_; }

    // Exact (default): every sample bit-identical to the reference arithmetic.  Fast: the stated-tolerance
    // mode (|fast - exact| <= GRAIL_FAST_TOLERANCE; clocks, phases, wraps and noise generators stay exact).
    enum class Arithmetic { Exact = 0, Fast = 1 };
    void set_arithmetic(Arithmetic a) const { check(grail_set_option(ctx_, "arithmetic", (int64_t)a)); }
    // Fast is served for voice tables up to a sharpness of their resonances (grail_fast_sharpness); sharper tables
    // are rendered by the exact kernels whatever set_arithmetic says.
    bool fast_arithmetic_served() const
    {
        int64_t v = 0;
        check(grail_get_option(ctx_, "fast_arithmetic_served", &v));
        return v != 0;
    }

    // utterances.map(|u| u.phonemes.select(v).sequence(v).jitter(seed, v).synthesize().collect())
    std::vector<std::vector<float>> synthesize(const std::vector<Utterance> &utts) const
    {
        std::vector<PhonemeElem> segs;
        std::vector<uint32_t> offs(1, 0u), vids, seeds;
        for (const Utterance &u : utts) {
            segs.insert(segs.end(), u.phonemes.begin(), u.phonemes.end());
            offs.push_back((uint32_t)segs.size());
            vids.push_back(u.voice);
            seeds.push_back(u.jitter_seed);
        }
        const uint32_t n = (uint32_t)utts.size();
        std::vector<uint32_t> lens(n ? n : 1);
        grail_batch *b = nullptr;
        check(grail_batch_upload(ctx_, segs.data(), offs.data(), vids.data(), seeds.data(), n, &b));
        const int rc = grail_batch_lengths(ctx_, b, 0xFFFFFFFFu, lens.data());
        grail_batch_free(ctx_, b);
        check(rc);
        uint64_t stride = 64;
        for (uint32_t i = 0; i < n; ++i) stride = lens[i] > stride ? lens[i] : stride;
        stride = (stride + 63) / 64 * 64;
        std::vector<float> flat((size_t)n * stride);
        check(grail_synthesize_batch(ctx_, segs.data(), offs.data(), vids.data(), seeds.data(), n,
                                     flat.data(), stride, lens.data(), GRAIL_OUT_HOST));
        std::vector<std::vector<float>> out(n);
        for (uint32_t i = 0; i < n; ++i)
            out[i].assign(flat.begin() + (size_t)i * stride, flat.begin() + (size_t)i * stride + lens[i]);
        return out;
    }

    // the whole chain of examples/cli.rs:175-184 for several texts, voice 0, seed 0
    std::vector<std::vector<float>> say(const std::vector<std::string> &texts) const
    {
        std::vector<Utterance> utts;
        for (const std::string &t : texts) utts.push_back(Utterance{phoneme_elems(voices_.at(0), t), 0, 0});
        return synthesize(utts);
    }

    // examples/cli.rs:49 on the device, then save_wav (cli.rs:28-67)
    void save_wav(const std::string &path, const std::vector<float> &pcm, uint32_t sample_rate) const
    {
        const uint32_t n = (uint32_t)pcm.size();
        void *d_in = nullptr, *d_out = nullptr, *d_len = nullptr;
        std::vector<int16_t> i16(n);
        int rc = grail_device_alloc(ctx_, (size_t)n * 4 + 4, &d_in);
        if (!rc) rc = grail_device_alloc(ctx_, (size_t)n * 2 + 16, &d_out);
        if (!rc) rc = grail_device_alloc(ctx_, 4, &d_len);
        if (!rc && n) rc = grail_memcpy_h2d(ctx_, d_in, pcm.data(), (size_t)n * 4);
        if (!rc) rc = grail_memcpy_h2d(ctx_, d_len, &n, 4);
        if (!rc) rc = grail_pcm16_async(ctx_, (const float *)d_in, n, (const uint32_t *)d_len, 1, n,
                                        (int16_t *)d_out, n);
        if (!rc) rc = grail_sync(ctx_);
        if (!rc && n) rc = grail_memcpy_d2h(ctx_, i16.data(), d_out, (size_t)n * 2);
        for (void *p : {d_in, d_out, d_len})
            if (p) grail_device_free(ctx_, p);
        check(rc);
        check(grail_wav_write_i16(path.c_str(), i16.data(), n, sample_rate));
    }

    // every utterance's length in samples (the Sequencer clock alone, src/lib.rs:861-888): what a timeline is laid out with
    std::vector<uint32_t> lengths(const std::vector<Utterance> &utts) const
    {
        std::vector<PhonemeElem> segs;
        std::vector<uint32_t> offs, vids, seeds;
        detail::flatten(utts, segs, offs, vids, seeds);
        const uint32_t n = (uint32_t)utts.size();
        std::vector<uint32_t> lens(n ? n : 1);
        grail_batch *b = nullptr;
        check(grail_batch_upload(ctx_, segs.data(), offs.data(), vids.data(), seeds.data(), n, &b));
        const int rc = grail_batch_lengths(ctx_, b, 0xFFFFFFFFu, lens.data());
        grail_batch_free(ctx_, b);
        check(rc);
        lens.resize(n);
        return lens;
    }

    // Renders the utterances and mixes them into n_tracks tracks of track_len samples on the device (grail_batch_mix: every
    // track sample is the left fold, in utterance order, of gain * sample over the placements that cover it; bit-identical
    // to that CPU loop over Gpu::synthesize's rows, Exact), then copies the tracks back.
    std::vector<std::vector<float>> mix(const std::vector<Utterance> &utts, const std::vector<Placement> &placements,
                                        uint32_t n_tracks, uint64_t track_len) const
    {
        std::vector<PhonemeElem> segs;
        std::vector<uint32_t> offs, vids, seeds, rows, tracks;
        std::vector<uint64_t> at;
        std::vector<float> gains;
        detail::flatten(utts, segs, offs, vids, seeds);
        for (const Placement &p : placements) {
            rows.push_back(p.utterance);
            tracks.push_back(p.track);
            at.push_back(p.offset);
            gains.push_back(p.gain);
        }
        const uint64_t stride = track_len ? (track_len + 63) / 64 * 64 : 64;
        grail_batch *b = nullptr;
        check(grail_batch_upload(ctx_, segs.data(), offs.data(), vids.data(), seeds.data(), (uint32_t)utts.size(), &b));
        void *d = nullptr;
        std::vector<float> flat((size_t)n_tracks * stride);
        int rc = grail_device_alloc(ctx_, flat.size() * sizeof(float) + 4, &d);
        if (!rc) rc = grail_batch_mix(ctx_, b, rows.data(), tracks.data(), at.data(), gains.data(), (uint32_t)rows.size(),
                                      (float *)d, stride, n_tracks, track_len, nullptr, 0u);
        if (!rc && !flat.empty()) rc = grail_memcpy_d2h(ctx_, flat.data(), d, flat.size() * sizeof(float));
        if (d) grail_device_free(ctx_, d);
        grail_batch_free(ctx_, b);
        check(rc);
        std::vector<std::vector<float>> out(n_tracks);
        for (uint32_t t = 0; t < n_tracks; ++t)
            out[t].assign(flat.begin() + (size_t)t * stride, flat.begin() + (size_t)t * stride + track_len);
        return out;
    }

    // Gpu::mix with a level instead of a gain: placement i's utterance is brought to level_db[i] decibels (0 dB = level
    // 1.0; mode GRAIL_LEVEL_RMS, GRAIL_LEVEL_PEAK or GRAIL_LEVEL_ACTIVE; with GRAIL_LEVEL_LOUDNESS level_db[i] is a target
    // in LUFS and an utterance shorter than 400 ms cannot be leveled) and Placement::gain is not read.  The rows are
    // measured on the device between rendering and mixing (grail_batch_mix_leveled).  gains_used, unleveled: the gains the
    // mix applied, and how many placements got gain 0 because their utterance is empty, silent or holds a non-finite sample.
    std::vector<std::vector<float>> mix_leveled(const std::vector<Utterance> &utts, const std::vector<Placement> &placements,
                                                const std::vector<float> &level_db, uint32_t n_tracks, uint64_t track_len,
                                                int mode = GRAIL_LEVEL_RMS, std::vector<float> *gains_used = nullptr,
                                                uint32_t *unleveled = nullptr) const
    {
        return mix_leveled_with(utts, placements, level_db, nullptr, n_tracks, track_len, mode, gains_used, unleveled, nullptr);
    }

    // Gpu::mix_leveled under a true-peak ceiling in dBTP (grail_batch_mix_leveled_limited): every utterance's true peak is
    // measured too and a gain that would bring it above the ceiling is cut back to it; limited: how many placements that
    // changed.  The ceiling binds each placement: placements that overlap on a track can still sum above it (Gpu::true_peak
    // of the finished tracks tells).
    std::vector<std::vector<float>> mix_leveled_limited(const std::vector<Utterance> &utts,
                                                        const std::vector<Placement> &placements,
                                                        const std::vector<float> &level_db, float ceiling_db,
                                                        uint32_t n_tracks, uint64_t track_len, int mode = GRAIL_LEVEL_RMS,
                                                        std::vector<float> *gains_used = nullptr,
                                                        uint32_t *unleveled = nullptr, uint32_t *limited = nullptr) const
    {
        return mix_leveled_with(utts, placements, level_db, &ceiling_db, n_tracks, track_len, mode, gains_used, unleveled,
                                limited);
    }

    // How loud rows of samples are, measured on the device (grail_levels_async; the contract is the header's section
    // "levels"): per row the binary64 sum of squares, the largest finite |x| and the count of non-finite samples.
    Levels levels(const std::vector<std::vector<float>> &rows) const
    {
        const uint32_t n = (uint32_t)rows.size();
        size_t longest = 0;
        for (const auto &r : rows) longest = r.size() > longest ? r.size() : longest;
        const uint64_t stride = longest ? (longest + 63) / 64 * 64 : 64;
        Levels out;
        out.sumsq.resize(n);
        out.peak.resize(n);
        out.nonfinite.resize(n);
        if (!n) return out;
        std::vector<uint32_t> lens(n);
        for (uint32_t i = 0; i < n; ++i) lens[i] = (uint32_t)rows[i].size();
        void *d_rows = nullptr, *d_len = nullptr, *d_sumsq = nullptr, *d_peak = nullptr, *d_bad = nullptr;
        int rc = grail_device_alloc(ctx_, (size_t)n * stride * 4, &d_rows);
        if (!rc) rc = grail_device_alloc(ctx_, (size_t)n * 4, &d_len);
        if (!rc) rc = grail_device_alloc(ctx_, (size_t)n * 8, &d_sumsq);
        if (!rc) rc = grail_device_alloc(ctx_, (size_t)n * 4, &d_peak);
        if (!rc) rc = grail_device_alloc(ctx_, (size_t)n * 4, &d_bad);
        for (uint32_t i = 0; !rc && i < n; ++i)
            if (lens[i]) rc = grail_memcpy_h2d(ctx_, (float *)d_rows + (size_t)i * stride, rows[i].data(), (size_t)lens[i] * 4);
        if (!rc) rc = grail_memcpy_h2d(ctx_, d_len, lens.data(), (size_t)n * 4);
        if (!rc) rc = grail_levels_async(ctx_, (const float *)d_rows, stride, (const uint32_t *)d_len, n, (double *)d_sumsq,
                                         (float *)d_peak, (uint32_t *)d_bad);
        if (!rc) rc = grail_memcpy_d2h(ctx_, out.sumsq.data(), d_sumsq, (size_t)n * 8);
        if (!rc) rc = grail_memcpy_d2h(ctx_, out.peak.data(), d_peak, (size_t)n * 4);
        if (!rc) rc = grail_memcpy_d2h(ctx_, out.nonfinite.data(), d_bad, (size_t)n * 4);
        for (void *p : {d_rows, d_len, d_sumsq, d_peak, d_bad})
            if (p) grail_device_free(ctx_, p);
        check(rc);
        return out;
    }

    // K-weighted gated loudness of rows of samples at sample_rate, measured on the device (grail_loudness_async; the
    // contract is the header's section "levels, continued").  One lane filters one row: many rows fill the device.
    Loudness loudness(const std::vector<std::vector<float>> &rows, uint32_t sample_rate) const
    {
        Loudness out;
        measure_loudness(rows, sample_rate, false, out, nullptr);
        return out;
    }

    // The same of few long rows (finished tracks), parallel in time (grail_loudness_segmented_async: every hop of 100 ms
    // filtered from a zero state three hops before it, one lane per hop), with the rows' hop sums: integrated loudness,
    // loudness range, largest momentary and short-term loudness all follow from them on the host.
    TrackLoudness track_loudness(const std::vector<std::vector<float>> &rows, uint32_t sample_rate) const
    {
        TrackLoudness out;
        out.hop = sample_rate / 10u;
        measure_loudness(rows, sample_rate, true, out, &out.hop_sumsq);
        return out;
    }

    // True peak of rows of samples (rendered rows or finished tracks), measured on the device (grail_true_peak_async; the
    // contract is the header's section "levels, continued: true peak").  Time is parallel: one long row fills the device.
    TruePeak true_peak(const std::vector<std::vector<float>> &rows) const
    {
        const uint32_t n = (uint32_t)rows.size();
        size_t longest = 0;
        for (const auto &r : rows) longest = r.size() > longest ? r.size() : longest;
        const uint64_t stride = longest ? (longest + 63) / 64 * 64 : 64;
        TruePeak out;
        out.true_peak.resize(n);
        out.nonfinite.resize(n);
        if (!n) return out;
        std::vector<uint32_t> lens(n);
        for (uint32_t i = 0; i < n; ++i) lens[i] = (uint32_t)rows[i].size();
        void *d_rows = nullptr, *d_len = nullptr, *d_tp = nullptr, *d_bad = nullptr;
        int rc = grail_device_alloc(ctx_, (size_t)n * stride * 4, &d_rows);
        if (!rc) rc = grail_device_alloc(ctx_, (size_t)n * 4, &d_len);
        if (!rc) rc = grail_device_alloc(ctx_, (size_t)n * 8, &d_tp);
        if (!rc) rc = grail_device_alloc(ctx_, (size_t)n * 4, &d_bad);
        for (uint32_t i = 0; !rc && i < n; ++i)
            if (lens[i]) rc = grail_memcpy_h2d(ctx_, (float *)d_rows + (size_t)i * stride, rows[i].data(), (size_t)lens[i] * 4);
        if (!rc) rc = grail_memcpy_h2d(ctx_, d_len, lens.data(), (size_t)n * 4);
        if (!rc) rc = grail_true_peak_async(ctx_, (const float *)d_rows, stride, (const uint32_t *)d_len, n, (double *)d_tp,
                                            (uint32_t *)d_bad);
        if (!rc) rc = grail_memcpy_d2h(ctx_, out.true_peak.data(), d_tp, (size_t)n * 8);
        if (!rc) rc = grail_memcpy_d2h(ctx_, out.nonfinite.data(), d_bad, (size_t)n * 4);
        for (void *p : {d_rows, d_len, d_tp, d_bad})
            if (p) grail_device_free(ctx_, p);
        check(rc);
        return out;
    }

    // The look-ahead limiter over rows of samples, `group` consecutive rows sharing one gain curve (finished tracks as one
    // linked group: group = rows.size()), on the device (grail_limit_async; the contract is the header's section "levels,
    // continued: limiter").  ceiling is linear (limit_ceiling), the look-ahead 2^lookahead_log2 samples.  |sample| <= ceiling
    // holds exactly afterwards; the true peak follows to within the header's bound: measure it with true_peak.
    Limited limit(const std::vector<std::vector<float>> &rows, float ceiling, uint32_t lookahead_log2, uint32_t group = 1) const
    {
        const uint32_t n = (uint32_t)rows.size();
        if (group == 0 || n % group) throw Error(GRAIL_ERR_INVALID_ARG, "limit: the number of rows is no multiple of group");
        const uint32_t n_groups = n / group;
        size_t longest = 0;
        for (const auto &r : rows) longest = r.size() > longest ? r.size() : longest;
        const uint64_t stride = longest ? (longest + 63) / 64 * 64 : 64;
        Limited out;
        out.rows.resize(n);
        out.min_gain.resize(n_groups);
        out.n_limited.resize(n_groups);
        out.nonfinite.resize(n_groups);
        if (!n) return out;
        std::vector<uint32_t> lens(n);
        for (uint32_t i = 0; i < n; ++i) lens[i] = (uint32_t)rows[i].size();
        void *d_rows = nullptr, *d_out = nullptr, *d_len = nullptr, *d_gain = nullptr, *d_lim = nullptr, *d_bad = nullptr;
        int rc = grail_device_alloc(ctx_, (size_t)n * stride * 4, &d_rows);
        if (!rc) rc = grail_device_alloc(ctx_, (size_t)n * stride * 4, &d_out);
        if (!rc) rc = grail_device_alloc(ctx_, (size_t)n * 4, &d_len);
        if (!rc) rc = grail_device_alloc(ctx_, (size_t)n_groups * 4, &d_gain);
        if (!rc) rc = grail_device_alloc(ctx_, (size_t)n_groups * 4, &d_lim);
        if (!rc) rc = grail_device_alloc(ctx_, (size_t)n_groups * 4, &d_bad);
        for (uint32_t i = 0; !rc && i < n; ++i)
            if (lens[i]) rc = grail_memcpy_h2d(ctx_, (float *)d_rows + (size_t)i * stride, rows[i].data(), (size_t)lens[i] * 4);
        if (!rc) rc = grail_memcpy_h2d(ctx_, d_len, lens.data(), (size_t)n * 4);
        if (!rc) rc = grail_limit_async(ctx_, (const float *)d_rows, stride, (const uint32_t *)d_len, n, group, ceiling,
                                        lookahead_log2, (float *)d_out, stride, (float *)d_gain, (uint32_t *)d_lim,
                                        (uint32_t *)d_bad);
        if (!rc) rc = grail_memcpy_d2h(ctx_, out.min_gain.data(), d_gain, (size_t)n_groups * 4);
        if (!rc) rc = grail_memcpy_d2h(ctx_, out.n_limited.data(), d_lim, (size_t)n_groups * 4);
        if (!rc) rc = grail_memcpy_d2h(ctx_, out.nonfinite.data(), d_bad, (size_t)n_groups * 4);
        for (uint32_t i = 0; !rc && i < n; ++i) {
            if (out.refused(i / group) || !lens[i]) continue;
            out.rows[i].resize(lens[i]);
            rc = grail_memcpy_d2h(ctx_, out.rows[i].data(), (const float *)d_out + (size_t)i * stride, (size_t)lens[i] * 4);
        }
        for (void *p : {d_rows, d_out, d_len, d_gain, d_lim, d_bad})
            if (p) grail_device_free(ctx_, p);
        check(rc);
        return out;
    }

    // Rows of samples at rate_in resampled to rate_out on the device (grail_resample_async; the contract is the header's
    // section "levels, continued: sample-rate conversion"): output m of a row sits at input time m * rate_in / rate_out, a
    // row of n samples gives ceil(n * rate_out / rate_in).  The filter overshoots: limit or measure after resampling.
    std::vector<std::vector<float>> resample(const std::vector<std::vector<float>> &rows, uint32_t rate_in, uint32_t rate_out) const
    {
        const uint32_t n = (uint32_t)rows.size();
        size_t longest = 0;
        for (const auto &r : rows) longest = r.size() > longest ? r.size() : longest;
        uint64_t longest_out = 0;
        check(grail_resample_len(longest, rate_in, rate_out, &longest_out));
        const uint64_t stride = longest ? (longest + 63) / 64 * 64 : 64, out_stride = longest_out ? (longest_out + 63) / 64 * 64 : 64;
        std::vector<std::vector<float>> out(n);
        if (!n) return out;
        std::vector<uint32_t> lens(n), out_lens(n);
        for (uint32_t i = 0; i < n; ++i) lens[i] = (uint32_t)rows[i].size();
        void *d_rows = nullptr, *d_out = nullptr, *d_len = nullptr, *d_out_len = nullptr;
        int rc = grail_device_alloc(ctx_, (size_t)n * stride * 4, &d_rows);
        if (!rc) rc = grail_device_alloc(ctx_, (size_t)n * out_stride * 4, &d_out);
        if (!rc) rc = grail_device_alloc(ctx_, (size_t)n * 4, &d_len);
        if (!rc) rc = grail_device_alloc(ctx_, (size_t)n * 4, &d_out_len);
        for (uint32_t i = 0; !rc && i < n; ++i)
            if (lens[i]) rc = grail_memcpy_h2d(ctx_, (float *)d_rows + (size_t)i * stride, rows[i].data(), (size_t)lens[i] * 4);
        if (!rc) rc = grail_memcpy_h2d(ctx_, d_len, lens.data(), (size_t)n * 4);
        if (!rc) rc = grail_resample_async(ctx_, (const float *)d_rows, stride, (const uint32_t *)d_len, n, rate_in, rate_out,
                                           (float *)d_out, out_stride, (uint32_t *)d_out_len, nullptr);
        if (!rc) rc = grail_memcpy_d2h(ctx_, out_lens.data(), d_out_len, (size_t)n * 4);
        for (uint32_t i = 0; !rc && i < n; ++i) {
            if (!out_lens[i]) continue;
            out[i].resize(out_lens[i]);
            rc = grail_memcpy_d2h(ctx_, out[i].data(), (const float *)d_out + (size_t)i * out_stride, (size_t)out_lens[i] * 4);
        }
        for (void *p : {d_rows, d_out, d_len, d_out_len})
            if (p) grail_device_free(ctx_, p);
        check(rc);
        return out;
    }

    // A set of filters for fir(), resident on this device
    FirSet fir_set(const std::vector<Fir> &filters) const { return FirSet(ctx_, filters); }
    // A stream of n_rows rows filtered chunk by chunk with filters of the set, row i with filter which[i] (which empty: filter
    // 0 for every row), their history resident on this device between calls
    FirStream fir_stream(const FirSet &set, uint32_t n_rows, const std::vector<uint32_t> &which = {}) const
    {
        return FirStream(ctx_, set, n_rows, which);
    }
    // n_rows rows resampled chunk by chunk from rate_in to rate_out, their state resident in HBM between the calls.
    ResampleStream resample_stream(uint32_t rate_in, uint32_t rate_out, uint32_t n_rows) const
    {
        return ResampleStream(ctx_, rate_in, rate_out, n_rows);
    }
    // n_rows rows in groups of `group` limited chunk by chunk under `ceiling` (linear) with a look-ahead of 2^lookahead_log2
    // samples, their look-ahead resident in HBM between the calls.
    LimitStream limit_stream(uint32_t n_rows, float ceiling, uint32_t lookahead_log2, uint32_t group = 1) const
    {
        return LimitStream(ctx_, n_rows, group, ceiling, lookahead_log2);
    }

    // Rows of samples filtered on the device (grail_fir_async; the contract is the header's section "levels, continued: FIR
    // filtering"), row i with filter which[i] of the set (which empty: filter 0 for every row).  ring_out: a row of n samples
    // gives n + K - 1 - origin, the filter's tail included; otherwise the rows come back as long as they came.  A row whose
    // index is outside the set comes back empty.  The output's peak can exceed the input's: limit or measure afterwards.
    std::vector<std::vector<float>> fir(const FirSet &set, const std::vector<std::vector<float>> &rows,
                                        const std::vector<uint32_t> &which = {}, bool ring_out = true) const
    {
        const uint32_t n = (uint32_t)rows.size();
        if (!which.empty() && which.size() != rows.size()) throw Error(GRAIL_ERR_INVALID_ARG, "fir: one filter index per row");
        size_t longest = 0;
        for (const auto &r : rows) longest = r.size() > longest ? r.size() : longest;
        const uint64_t longest_out = longest + (ring_out ? set.tail() : 0);
        const uint64_t stride = longest ? (longest + 63) / 64 * 64 : 64, out_stride = longest_out ? (longest_out + 63) / 64 * 64 : 64;
        std::vector<std::vector<float>> out(n);
        if (!n) return out;
        std::vector<uint32_t> lens(n), out_lens(n);
        for (uint32_t i = 0; i < n; ++i) lens[i] = (uint32_t)rows[i].size();
        void *d_rows = nullptr, *d_out = nullptr, *d_len = nullptr, *d_out_len = nullptr, *d_which = nullptr;
        int rc = grail_device_alloc(ctx_, (size_t)n * stride * 4, &d_rows);
        if (!rc) rc = grail_device_alloc(ctx_, (size_t)n * out_stride * 4, &d_out);
        if (!rc) rc = grail_device_alloc(ctx_, (size_t)n * 4, &d_len);
        if (!rc) rc = grail_device_alloc(ctx_, (size_t)n * 4, &d_out_len);
        if (!rc && !which.empty()) rc = grail_device_alloc(ctx_, (size_t)n * 4, &d_which);
        for (uint32_t i = 0; !rc && i < n; ++i)
            if (lens[i]) rc = grail_memcpy_h2d(ctx_, (float *)d_rows + (size_t)i * stride, rows[i].data(), (size_t)lens[i] * 4);
        if (!rc) rc = grail_memcpy_h2d(ctx_, d_len, lens.data(), (size_t)n * 4);
        if (!rc && d_which) rc = grail_memcpy_h2d(ctx_, d_which, which.data(), (size_t)n * 4);
        if (!rc) rc = grail_fir_async(ctx_, set.get(), (const float *)d_rows, stride, (const uint32_t *)d_len, n, (const uint32_t *)d_which,
                                      (float *)d_out, out_stride, (uint32_t *)d_out_len, nullptr);
        if (!rc) rc = grail_memcpy_d2h(ctx_, out_lens.data(), d_out_len, (size_t)n * 4);
        for (uint32_t i = 0; !rc && i < n; ++i) {
            if (!out_lens[i] || out_lens[i] == GRAIL_LIMIT_REFUSED) continue;
            const size_t keep = ring_out ? out_lens[i] : std::min<size_t>(out_lens[i], lens[i]);
            out[i].resize(keep);
            rc = grail_memcpy_d2h(ctx_, out[i].data(), (const float *)d_out + (size_t)i * out_stride, keep * 4);
        }
        for (void *p : {d_rows, d_out, d_len, d_out_len, d_which})
            if (p) grail_device_free(ctx_, p);
        check(rc);
        return out;
    }

    // Tracks of equal length as one multichannel WAV: interleaved i16 frames made on the device (grail_pcm16_frames_async,
    // the examples/cli.rs:49 conversion), then save_wav for as many channels (grail_wav_write_i16_frames).
    void save_wav_frames(const std::string &path, const std::vector<std::vector<float>> &tracks, uint32_t sample_rate) const
    {
        const uint32_t ch = (uint32_t)tracks.size();
        const uint64_t n = ch ? tracks[0].size() : 0;
        for (const auto &t : tracks)
            if (t.size() != n) throw Error(GRAIL_ERR_INVALID_ARG, "save_wav_frames: tracks of different lengths");
        void *d_in = nullptr, *d_out = nullptr;
        std::vector<int16_t> frames((size_t)n * ch);
        check(grail_device_alloc(ctx_, (size_t)n * ch * 4 + 4, &d_in));
        int rc = grail_device_alloc(ctx_, frames.size() * 2 + 4, &d_out);
        for (uint32_t t = 0; !rc && t < ch && n; ++t)
            rc = grail_memcpy_h2d(ctx_, (float *)d_in + (size_t)t * n, tracks[t].data(), (size_t)n * 4);
        if (!rc) rc = grail_pcm16_frames_async(ctx_, (const float *)d_in, n, ch, n, (int16_t *)d_out);
        if (!rc) rc = grail_sync(ctx_);
        if (!rc && !frames.empty()) rc = grail_memcpy_d2h(ctx_, frames.data(), d_out, frames.size() * 2);
        grail_device_free(ctx_, d_in);
        if (d_out) grail_device_free(ctx_, d_out);
        check(rc);
        check(grail_wav_write_i16_frames(path.c_str(), frames.data(), (uint32_t)n, ch, sample_rate));
    }

private:
    // loudness (hop_sumsq NULL: grail_loudness_async) and track_loudness (grail_loudness_segmented_async, with the hop sums)
    void measure_loudness(const std::vector<std::vector<float>> &rows, uint32_t sample_rate, bool segmented, Loudness &out,
                          std::vector<std::vector<double>> *hop_sumsq) const
    {
        const uint32_t n = (uint32_t)rows.size();
        size_t longest = 0;
        for (const auto &r : rows) longest = r.size() > longest ? r.size() : longest;
        const uint64_t stride = longest ? (longest + 63) / 64 * 64 : 64;
        const uint32_t hop = sample_rate / 10u;
        out.gated_ms.resize(n);
        out.nonfinite.resize(n);
        if (hop_sumsq) hop_sumsq->assign(n, {});
        if (!n) return;
        std::vector<uint32_t> lens(n);
        for (uint32_t i = 0; i < n; ++i) lens[i] = (uint32_t)rows[i].size();
        const uint64_t hs = hop_sumsq && hop ? stride / hop : 0;
        std::vector<double> hops((size_t)n * hs);
        void *d_rows = nullptr, *d_len = nullptr, *d_ms = nullptr, *d_bad = nullptr, *d_hops = nullptr;
        int rc = grail_device_alloc(ctx_, (size_t)n * stride * 4, &d_rows);
        if (!rc) rc = grail_device_alloc(ctx_, (size_t)n * 4, &d_len);
        if (!rc) rc = grail_device_alloc(ctx_, (size_t)n * 8, &d_ms);
        if (!rc) rc = grail_device_alloc(ctx_, (size_t)n * 4, &d_bad);
        if (!rc && hs) rc = grail_device_alloc(ctx_, hops.size() * 8, &d_hops);
        for (uint32_t i = 0; !rc && i < n; ++i)
            if (lens[i]) rc = grail_memcpy_h2d(ctx_, (float *)d_rows + (size_t)i * stride, rows[i].data(), (size_t)lens[i] * 4);
        if (!rc) rc = grail_memcpy_h2d(ctx_, d_len, lens.data(), (size_t)n * 4);
        if (!rc && !segmented)
            rc = grail_loudness_async(ctx_, (const float *)d_rows, stride, (const uint32_t *)d_len, n, sample_rate, nullptr,
                                      (double *)d_ms, (double *)d_hops, hs, (uint32_t *)d_bad);
        if (!rc && segmented)
            rc = grail_loudness_segmented_async(ctx_, (const float *)d_rows, stride, (const uint32_t *)d_len, n, sample_rate,
                                                nullptr, (double *)d_ms, (double *)d_hops, hs, (uint32_t *)d_bad);
        if (!rc && hs) rc = grail_memcpy_d2h(ctx_, hops.data(), d_hops, hops.size() * 8);
        if (!rc) rc = grail_memcpy_d2h(ctx_, out.gated_ms.data(), d_ms, (size_t)n * 8);
        if (!rc) rc = grail_memcpy_d2h(ctx_, out.nonfinite.data(), d_bad, (size_t)n * 4);
        for (void *p : {d_rows, d_len, d_ms, d_bad, d_hops})
            if (p) grail_device_free(ctx_, p);
        check(rc);
        for (uint32_t i = 0; i < n && hs; ++i)      // (hops past a row's last were never written)
            (*hop_sumsq)[i].assign(hops.begin() + (size_t)i * hs, hops.begin() + (size_t)i * hs + lens[i] / hop);
    }

    // mix_leveled (ceiling_db NULL) and mix_leveled_limited
    std::vector<std::vector<float>> mix_leveled_with(const std::vector<Utterance> &utts, const std::vector<Placement> &placements,
                                                     const std::vector<float> &level_db, const float *ceiling_db,
                                                     uint32_t n_tracks, uint64_t track_len, int mode,
                                                     std::vector<float> *gains_used, uint32_t *unleveled,
                                                     uint32_t *limited) const
    {
        if (level_db.size() != placements.size())
            throw Error(GRAIL_ERR_INVALID_ARG, "mix_leveled: one level per placement");
        std::vector<PhonemeElem> segs;
        std::vector<uint32_t> offs, vids, seeds, rows, tracks;
        std::vector<uint64_t> at;
        detail::flatten(utts, segs, offs, vids, seeds);
        for (const Placement &p : placements) {
            rows.push_back(p.utterance);
            tracks.push_back(p.track);
            at.push_back(p.offset);
        }
        const uint64_t stride = track_len ? (track_len + 63) / 64 * 64 : 64;
        grail_batch *b = nullptr;
        check(grail_batch_upload(ctx_, segs.data(), offs.data(), vids.data(), seeds.data(), (uint32_t)utts.size(), &b));
        void *d = nullptr;
        std::vector<float> flat((size_t)n_tracks * stride), gains(rows.size() ? rows.size() : 1);
        uint32_t left_out = 0, cut = 0;
        int rc = grail_device_alloc(ctx_, flat.size() * sizeof(float) + 4, &d);
        if (!rc && ceiling_db)
            rc = grail_batch_mix_leveled_limited(ctx_, b, rows.data(), tracks.data(), at.data(), level_db.data(), mode,
                                                 (uint32_t)rows.size(), (float *)d, stride, n_tracks, track_len, nullptr,
                                                 gains.data(), &left_out, *ceiling_db, &cut, 0u);
        else if (!rc)
            rc = grail_batch_mix_leveled(ctx_, b, rows.data(), tracks.data(), at.data(), level_db.data(), mode,
                                         (uint32_t)rows.size(), (float *)d, stride, n_tracks, track_len, nullptr,
                                         gains.data(), &left_out, 0u);
        if (!rc && !flat.empty()) rc = grail_memcpy_d2h(ctx_, flat.data(), d, flat.size() * sizeof(float));
        if (d) grail_device_free(ctx_, d);
        grail_batch_free(ctx_, b);
        check(rc);
        gains.resize(rows.size());
        if (gains_used) *gains_used = gains;
        if (unleveled) *unleveled = left_out;
        if (limited) *limited = cut;
        std::vector<std::vector<float>> out(n_tracks);
        for (uint32_t t = 0; t < n_tracks; ++t)
            out[t].assign(flat.begin() + (size_t)t * stride, flat.begin() + (size_t)t * stride + track_len);
        return out;
    }

    grail_ctx *ctx_ = nullptr;
    std::vector<Voice> voices_;
};

// Every GPU of the node behind the same call (grail_node_*): one context and one host thread per device, the voice table
// carried to the others' HBM by one ncclBroadcast, the batch cut into contiguous shards that render concurrently into
// slices of one host buffer.  Results are those of Gpu::synthesize, row for row, bit for bit (Exact).
class Node {
public:
    // voices_without_rccl: tests on a box whose `devices` name one GPU more than once (RCCL refuses such a communicator)
    Node(const std::vector<int> &devices, const std::vector<Voice> &voices, bool voices_without_rccl = false) : voices_(voices)
    {
        check(grail_node_create(devices.data(), (uint32_t)devices.size(), &node_));
        int rc = voices_without_rccl ? grail_node_set_option(node_, "node_voices_without_rccl", 1) : GRAIL_OK;
        if (!rc) rc = grail_node_set_voices(node_, voices_.data(), (uint32_t)voices_.size());
        if (rc != GRAIL_OK) {
            grail_node_destroy(node_);
            check(rc);
        }
    }
    ~Node() { grail_node_destroy(node_); }
    Node(const Node &) = delete;
    Node &operator=(const Node &) = delete;

    grail_node *node() const { return node_; }
    uint32_t size() const { return grail_node_size(node_); }
    const std::vector<Voice> &voices() const { return voices_; }
    void set_arithmetic(Gpu::Arithmetic a) const { check(grail_node_set_option(node_, "arithmetic", (int64_t)a)); }
    // ranks RCCL reports for the node's communicator (ncclCommCount; 0 under voices_without_rccl)
    uint32_t rccl_ranks() const
    {
        int64_t v = 0;
        check(grail_node_get_option(node_, "node_rccl_ranks", &v));
        return (uint32_t)v;
    }

    std::vector<std::vector<float>> synthesize(const std::vector<Utterance> &utts) const
    {
        std::vector<PhonemeElem> segs;
        std::vector<uint32_t> offs(1, 0u), vids, seeds;
        for (const Utterance &u : utts) {
            segs.insert(segs.end(), u.phonemes.begin(), u.phonemes.end());
            offs.push_back((uint32_t)segs.size());
            vids.push_back(u.voice);
            seeds.push_back(u.jitter_seed);
        }
        const uint32_t n = (uint32_t)utts.size();
        std::vector<uint32_t> lens(n ? n : 1);
        check(grail_node_lengths(node_, segs.data(), offs.data(), vids.data(), n, 0xFFFFFFFFu, lens.data()));
        uint64_t stride = 64;
        for (uint32_t i = 0; i < n; ++i) stride = lens[i] > stride ? lens[i] : stride;
        stride = (stride + 63) / 64 * 64;
        std::vector<float> flat((size_t)n * stride);
        check(grail_node_synthesize_batch(node_, segs.data(), offs.data(), vids.data(), seeds.data(), n, flat.data(),
                                          stride, lens.data(), GRAIL_OUT_HOST));
        std::vector<std::vector<float>> out(n);
        for (uint32_t i = 0; i < n; ++i)
            out[i].assign(flat.begin() + (size_t)i * stride, flat.begin() + (size_t)i * stride + lens[i]);
        return out;
    }

    std::vector<std::vector<float>> say(const std::vector<std::string> &texts) const
    {
        std::vector<Utterance> utts;
        for (const std::string &t : texts) utts.push_back(Utterance{phoneme_elems(voices_.at(0), t), 0, 0});
        return synthesize(utts);
    }

private:
    grail_node *node_ = nullptr;
    std::vector<Voice> voices_;
};

// The lazy use of the chain: the crate's iterator is pulled a buffer at a time
// (examples/interactive.rs:31-48).  Here every utterance of the batch yields its next `chunk`
// samples per call; the iterator state stays in HBM between calls (grail_stream_*), and the
// chunks concatenate to exactly what Gpu::synthesize returns.
class Stream {
public:
    Stream(const Gpu &gpu, const std::vector<Utterance> &utts, uint32_t chunk)
        : ctx_(gpu.ctx()), n_((uint32_t)utts.size()), chunk_(chunk), stride_(((uint64_t)chunk + 63) / 64 * 64)
    {
        std::vector<PhonemeElem> segs;
        std::vector<uint32_t> offs(1, 0u), vids, seeds;
        for (const Utterance &u : utts) {
            segs.insert(segs.end(), u.phonemes.begin(), u.phonemes.end());
            offs.push_back((uint32_t)segs.size());
            vids.push_back(u.voice);
            seeds.push_back(u.jitter_seed);
        }
        check(grail_batch_upload(ctx_, segs.data(), offs.data(), vids.data(), seeds.data(), n_, &batch_));
        int rc = grail_stream_open(ctx_, batch_, &stream_);
        if (!rc) rc = grail_device_alloc(ctx_, (size_t)(n_ ? n_ : 1) * stride_ * sizeof(float), &d_out_);
        if (!rc) rc = grail_device_alloc(ctx_, (size_t)(n_ ? n_ : 1) * sizeof(uint32_t), &d_len_);
        if (rc) {
            release();
            check(rc);
        }
        host_.resize((size_t)n_ * stride_);
        lens_.resize(n_);
    }
    ~Stream() { release(); }
    Stream(const Stream &) = delete;
    Stream &operator=(const Stream &) = delete;

    // Iterator::next, `chunk` samples at a time: false once every chain has returned None
    bool next(std::vector<std::vector<float>> &chunks)
    {
        chunks.assign(n_, {});
        if (n_ == 0 || chunk_ == 0) return false;
        check(grail_stream_next_async(ctx_, stream_, chunk_, (float *)d_out_, stride_, (uint32_t *)d_len_));
        check(grail_sync(ctx_));
        check(grail_memcpy_d2h(ctx_, lens_.data(), d_len_, (size_t)n_ * sizeof(uint32_t)));
        check(grail_memcpy_d2h(ctx_, host_.data(), d_out_, host_.size() * sizeof(float)));
        bool any = false;
        for (uint32_t u = 0; u < n_; ++u) {
            chunks[u].assign(host_.begin() + (size_t)u * stride_, host_.begin() + (size_t)u * stride_ + lens_[u]);
            any = any || lens_[u] != 0;
        }
        return any;
    }

private:
    void release()
    {
        if (stream_) grail_stream_close(ctx_, stream_);
        if (batch_) grail_batch_free(ctx_, batch_);
        if (d_out_) grail_device_free(ctx_, d_out_);
        if (d_len_) grail_device_free(ctx_, d_len_);
        stream_ = nullptr; batch_ = nullptr; d_out_ = nullptr; d_len_ = nullptr;
    }
    grail_ctx *ctx_;
    uint32_t n_, chunk_;
    uint64_t stride_;
    grail_batch *batch_ = nullptr;
    grail_stream *stream_ = nullptr;
    void *d_out_ = nullptr, *d_len_ = nullptr;
    std::vector<float> host_;
    std::vector<uint32_t> lens_;
};

// The live use of the chain (examples/interactive.rs:31-48): ONE chain runs for the whole session, its source delivers
// while the audio callback is pulling, and carrier phase, noise seed, jitter and filter state carry across everything that
// is ever said.  Segments are appended whenever they are known; next() yields the next `chunk` samples, or fewer when
// the Sequencer is waiting for a segment that has not been appended yet (src/lib.rs:866-888 pulls iter.next() on demand)
// — the front end then feeds it, a Silence when no text is waiting, exactly as the reference's source hands over ' '.
class LiveStream {
public:
    LiveStream(const Gpu &gpu, uint32_t chunk, uint32_t voice = 0, uint32_t jitter_seed = 0, uint32_t ring_segments = 0)
        : ctx_(gpu.ctx()), chunk_(chunk), stride_(((uint64_t)chunk + 63) / 64 * 64)
    {
        check(grail_stream_open_live(ctx_, 1, &voice, &jitter_seed, ring_segments, 0, &stream_));
        int rc = grail_device_alloc(ctx_, (size_t)stride_ * sizeof(float), &d_out_);
        if (!rc) rc = grail_device_alloc(ctx_, sizeof(uint32_t), &d_len_);
        if (rc) {
            release();
            check(rc);
        }
    }
    ~LiveStream() { release(); }
    LiveStream(const LiveStream &) = delete;
    LiveStream &operator=(const LiveStream &) = delete;

    // the source delivers: these segments follow what the chain already has
    void append(const std::vector<PhonemeElem> &segs)
    {
        const uint32_t offs[2] = {0u, (uint32_t)segs.size()};
        check(grail_stream_append(ctx_, stream_, segs.data(), offs));
    }
    // the source has ended: what is pending is spoken, the last segment fades out, next() then returns nothing
    void finish() { check(grail_stream_finish(ctx_, stream_, nullptr)); }
    // segments appended that the Sequencer has not pulled yet
    uint32_t pending()
    {
        uint32_t n = 0;
        check(grail_stream_pending(ctx_, stream_, &n));
        return n;
    }
    // Iterator::next, up to `chunk` samples: fewer when the Sequencer waits for the source (or the chain has ended)
    std::vector<float> next()
    {
        uint32_t n = 0;
        check(grail_stream_next_async(ctx_, stream_, chunk_, (float *)d_out_, stride_, (uint32_t *)d_len_));
        check(grail_sync(ctx_));
        check(grail_memcpy_d2h(ctx_, &n, d_len_, sizeof n));
        std::vector<float> out(n);
        if (n) check(grail_memcpy_d2h(ctx_, out.data(), d_out_, (size_t)n * sizeof(float)));
        return out;
    }
    // ... through a filter stream of one row before anything leaves the device: the chunk the chain rendered is fed to
    // `filter` where it lies, and what comes back is what the filter could write for it (fewer samples than were rendered
    // while the filter is short of its origin).  *rendered: the chain's own count, which says whether the Sequencer waits.
    std::vector<float> next(FirStream &filter, uint32_t *rendered)
    {
        if (filter.rows() != 1) throw Error(GRAIL_ERR_INVALID_ARG, "LiveStream::next: a filter stream of one row");
        if (!d_filtered_) check(grail_device_alloc(ctx_, (size_t)stride_ * sizeof(float), &d_filtered_));
        if (!d_filtered_len_) check(grail_device_alloc(ctx_, sizeof(uint32_t), &d_filtered_len_));
        uint32_t n = 0;
        check(grail_stream_next_async(ctx_, stream_, chunk_, (float *)d_out_, stride_, (uint32_t *)d_len_));
        filter.next_async((const float *)d_out_, stride_, (const uint32_t *)d_len_, (float *)d_filtered_, stride_,
                          (uint32_t *)d_filtered_len_);
        check(grail_memcpy_d2h(ctx_, rendered, d_len_, sizeof *rendered));
        check(grail_memcpy_d2h(ctx_, &n, d_filtered_len_, sizeof n));
        std::vector<float> out(n);
        if (n) check(grail_memcpy_d2h(ctx_, out.data(), d_filtered_, (size_t)n * sizeof(float)));
        return out;
    }
    // ... through a resample stream of one row, behind `filter` if that is not NULL (a filter stream of one row): the
    // three-stage live chain, every stage reading what the stage before wrote where it lies.  What comes back is what the
    // resampler could write for the chunk, at its output rate.
    std::vector<float> next(FirStream *filter, ResampleStream &resampler, uint32_t *rendered)
    {
        if ((filter && filter->rows() != 1) || resampler.rows() != 1)
            throw Error(GRAIL_ERR_INVALID_ARG, "LiveStream::next: streams of one row");
        if (filter && !d_filtered_) check(grail_device_alloc(ctx_, (size_t)stride_ * sizeof(float), &d_filtered_));
        if (filter && !d_filtered_len_) check(grail_device_alloc(ctx_, sizeof(uint32_t), &d_filtered_len_));
        const uint64_t room = (resampler.most(stride_) + 63) / 64 * 64;
        if (!d_resampled_) check(grail_device_alloc(ctx_, (size_t)room * sizeof(float), &d_resampled_));
        if (!d_resampled_len_) check(grail_device_alloc(ctx_, sizeof(uint32_t), &d_resampled_len_));
        uint32_t n = 0;
        check(grail_stream_next_async(ctx_, stream_, chunk_, (float *)d_out_, stride_, (uint32_t *)d_len_));
        if (filter)
            filter->next_async((const float *)d_out_, stride_, (const uint32_t *)d_len_, (float *)d_filtered_, stride_,
                               (uint32_t *)d_filtered_len_);
        resampler.next_async((const float *)(filter ? d_filtered_ : d_out_), stride_,
                             (const uint32_t *)(filter ? d_filtered_len_ : d_len_), (float *)d_resampled_, room,
                             (uint32_t *)d_resampled_len_);
        check(grail_memcpy_d2h(ctx_, rendered, d_len_, sizeof *rendered));
        check(grail_memcpy_d2h(ctx_, &n, d_resampled_len_, sizeof n));
        std::vector<float> out(n);
        if (n) check(grail_memcpy_d2h(ctx_, out.data(), d_resampled_, (size_t)n * sizeof(float)));
        return out;
    }
    // ... through a limit stream of one row, behind `filter` and ahead of `resampler` where those are not NULL: the one-shot
    // order (filter, limit, resample), every stage reading what the stage before wrote where it lies.
    std::vector<float> next(FirStream *filter, LimitStream &limiter, ResampleStream *resampler, uint32_t *rendered)
    {
        if ((filter && filter->rows() != 1) || limiter.rows() != 1 || (resampler && resampler->rows() != 1))
            throw Error(GRAIL_ERR_INVALID_ARG, "LiveStream::next: streams of one row");
        if (filter && !d_filtered_) check(grail_device_alloc(ctx_, (size_t)stride_ * sizeof(float), &d_filtered_));
        if (filter && !d_filtered_len_) check(grail_device_alloc(ctx_, sizeof(uint32_t), &d_filtered_len_));
        if (!d_limited_) check(grail_device_alloc(ctx_, (size_t)stride_ * sizeof(float), &d_limited_));
        if (!d_limited_len_) check(grail_device_alloc(ctx_, sizeof(uint32_t), &d_limited_len_));
        const uint64_t room = resampler ? (resampler->most(stride_) + 63) / 64 * 64 : 0;
        if (resampler && !d_resampled_) check(grail_device_alloc(ctx_, (size_t)room * sizeof(float), &d_resampled_));
        if (resampler && !d_resampled_len_) check(grail_device_alloc(ctx_, sizeof(uint32_t), &d_resampled_len_));
        uint32_t n = 0;
        check(grail_stream_next_async(ctx_, stream_, chunk_, (float *)d_out_, stride_, (uint32_t *)d_len_));
        if (filter)
            filter->next_async((const float *)d_out_, stride_, (const uint32_t *)d_len_, (float *)d_filtered_, stride_,
                               (uint32_t *)d_filtered_len_);
        limiter.next_async((const float *)(filter ? d_filtered_ : d_out_), stride_, (const uint32_t *)(filter ? d_filtered_len_ : d_len_),
                           (float *)d_limited_, stride_, (uint32_t *)d_limited_len_);
        if (resampler)
            resampler->next_async((const float *)d_limited_, stride_, (const uint32_t *)d_limited_len_, (float *)d_resampled_, room,
                                  (uint32_t *)d_resampled_len_);
        check(grail_memcpy_d2h(ctx_, rendered, d_len_, sizeof *rendered));
        check(grail_memcpy_d2h(ctx_, &n, resampler ? d_resampled_len_ : d_limited_len_, sizeof n));
        std::vector<float> out(n);
        if (n) check(grail_memcpy_d2h(ctx_, out.data(), resampler ? d_resampled_ : d_limited_, (size_t)n * sizeof(float)));
        return out;
    }
    uint32_t chunk() const { return chunk_; }

private:
    void release()
    {
        if (stream_) grail_stream_close(ctx_, stream_);
        for (void *p : {d_out_, d_len_, d_filtered_, d_filtered_len_, d_resampled_, d_resampled_len_, d_limited_, d_limited_len_})
            if (p) grail_device_free(ctx_, p);
        stream_ = nullptr; d_out_ = nullptr; d_len_ = nullptr; d_filtered_ = nullptr; d_filtered_len_ = nullptr;
        d_resampled_ = nullptr; d_resampled_len_ = nullptr; d_limited_ = nullptr; d_limited_len_ = nullptr;
    }
    grail_ctx *ctx_;
    uint32_t chunk_;
    uint64_t stride_;
    grail_stream *stream_ = nullptr;
    void *d_out_ = nullptr, *d_len_ = nullptr;
    void *d_filtered_ = nullptr, *d_filtered_len_ = nullptr;      // next(filter, ...): made at its first call
    void *d_resampled_ = nullptr, *d_resampled_len_ = nullptr;    // next(filter, resampler, ...): made at its first call
    void *d_limited_ = nullptr, *d_limited_len_ = nullptr;        // next(filter, limiter, resampler, ...): made at its first call
};

}  // namespace grail
