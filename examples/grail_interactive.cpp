// grail_interactive — the reference's examples/interactive.rs without the sound card.
//
// There ONE iterator chain runs for the whole session (interactive.rs:31-38): its source is
// `repeat_with(|| receiver.try_recv().unwrap_or(' '))`, so text arrives while the audio callback (:42-48) is pulling
// samples, a ' ' — which no rule matches: a Silence phoneme (src/lib.rs:1158-1163) — is handed over whenever the chain
// asks and nothing is waiting, and carrier phase, noise seed, jitter and filter state carry from one line into the next.
// Here the chain is a grail::LiveStream on the GPU: every line is transcribed as `line.trim().chars() + ' '`
// (interactive.rs:78-80; the leading Silence of `.transcribe()`, src/lib.rs:1201, once per session), its phonemes wait in
// a queue, and whenever the Sequencer asks for its next segment (LiveStream::next() comes back short) it is fed ONE
// phoneme: the next of the queue, or a Silence.  Audio is pulled `chunk` samples at a time, the role of the cpal
// callback, and written to stdout as raw little-endian f32.
//
// Without a sound card time is the audio itself: a line "@1.5 text" arrives once 1.5 s of audio have been rendered, a line
// without a stamp arrives at once.  After the last line has been spoken the session runs `tail` seconds longer (the
// reference never ends) and the source is closed.
//   usage: grail_interactive [--band LO HI [--taps K]] [--ceiling DB [--lookahead l]] [--rate R] [--eq KIND:F0:Q[:GAIN]]... [--meter] [chunk_samples] [tail_seconds]
//          < script > out.f32
// --band LO HI: every pulled chunk goes through a filter stream (the Kaiser-windowed band-pass LO .. HI Hz of
// grail_fir_design, K taps, 255 unless --taps says otherwise, at its zero-delay origin) before it leaves the device, and when
// the chain has ended the filter rings out: the output is what grail_fir_async gives for the whole session, K / 2 samples
// longer than the session.
// --ceiling DB: every pulled chunk, after --band if that is given, goes through a limit stream that holds it under DB dBTP
// with a look-ahead of 2^l samples (l = 8 unless --lookahead says otherwise) before it leaves the device; the output lags
// the chain by 2^l + 10 samples, which the limiter's tail delivers at the end.  The output is what grail_limit_async gives
// for the whole (filtered) session.
// --rate R: every pulled chunk, after --band and --ceiling if those are given, goes through a resample stream from the voice's rate to R Hz
// before it leaves the device.  When the chain has ended the tails are flushed in chain order: the filter's tail is fed to
// the limiter and what that gives to the resampler, then the limiter's own tail likewise, then the resampler's.  The output is what grail_resample_async gives for the whole (filtered)
// session.
// --eq KIND:F0:Q[:GAIN] (up to eight times; examples/eq_option.h): everything that leaves the chain above, chunk by chunk and
// the tails too, goes through an IIR stream (grail_iir_stream_*) of one recursive filter of as many biquad sections as there
// are --eq, designed at the rate that is written (grail_iir_design), before it is written; after the last of them the filter
// rings out for a tenth of a second.  The output is what grail_iir_async gives for the whole session's samples with that tail.
// --meter: everything that is written goes through a meter stream (grail_meter_stream_*) at the rate it is written at, chunk by
// chunk and the tails too; after the last of them the row is finished and stderr gets the report of grail_dialogue --report
// (integrated loudness, range, max momentary, max short-term, true peak), then the gated mean square and the true peak as
// their own bits (%a): what grail_loudness_async and grail_true_peak_async give for the finished track.
// Every phoneme fed is reported on stderr ("fed <phoneme> at <sample>"), so that a test can render the same list with
// the oracle in one piece and compare bit for bit.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <deque>
#include <iostream>
#include <memory>
#include <string>
#include <vector>

#include "eq_option.h"
#include "grail.hpp"

namespace {

struct Line {
    double at;          // seconds of audio after which the line arrives
    std::string text;
};

// line.trim().chars().chain(Some(' '))  interactive.rs:78-80, through `.transcribe(generic()).intonate(generic(), voice)`
std::vector<grail::PhonemeElem> speak(const grail::Voice &voice, const std::string &line, bool first)
{
    const grail_rule *rules = nullptr;
    int case_sensitive = 0;
    const uint32_t n_rules = grail_language_generic(&rules, &case_sensitive);
    std::string t = line;
    while (!t.empty() && (t.back() == ' ' || t.back() == '\t' || t.back() == '\r')) t.pop_back();
    size_t lead = 0;
    while (lead < t.size() && (t[lead] == ' ' || t[lead] == '\t')) ++lead;
    std::vector<uint32_t> cps;
    for (size_t i = lead; i < t.size(); ++i) cps.push_back((unsigned char)t[i]);      // (the generic language is ASCII)
    cps.push_back(' ');
    std::vector<int32_t> ph(4 * cps.size() + 8);
    uint32_t n = 0;
    grail::check(grail_transcribe(cps.data(), (uint32_t)cps.size(), rules, n_rules, case_sensitive, first ? 1 : 0, ph.data(),
                                  (uint32_t)ph.size(), &n));
    std::vector<grail::PhonemeElem> out(n);
    if (n) grail::check(grail_intonate(&voice, ph.data(), n, out.data()));
    return out;
}

// --eq: an IIR stream of one row on what leaves the chain, through the C ABI (grail_iir_create, grail_iir_stream_*): the
// filter's state stays on the device from one pull to the next.
class Eq {
public:
    Eq(grail_ctx *ctx, const std::vector<double> &coef, uint32_t tail) : ctx_(ctx), tail_(tail)
    {
        const uint32_t sections = (uint32_t)(coef.size() / 5);
        grail::check(grail_iir_create(ctx, coef.data(), &sections, 1, &set_));
        grail::check(grail_iir_stream_open(ctx, set_, 1, nullptr, tail, &stream_));
    }
    Eq(const Eq &) = delete;
    Eq &operator=(const Eq &) = delete;
    ~Eq()
    {
        grail_iir_stream_close(ctx_, stream_);      // (before its set: a set with open streams is not freed)
        grail_iir_free(ctx_, set_);
        for (void *p : {in_, out_, len_}) grail_device_free(ctx_, p);
    }
    // the samples that left the chain go back to the device and through the filter; as many come back
    std::vector<float> next(const std::vector<float> &part)
    {
        if (part.empty()) return {};
        room(part.size());
        const uint32_t n = (uint32_t)part.size();
        grail::check(grail_memcpy_h2d(ctx_, in_, part.data(), n * sizeof(float)));
        grail::check(grail_memcpy_h2d(ctx_, len_, &n, sizeof n));
        grail::check(grail_iir_stream_next_async(ctx_, stream_, (const float *)in_, cap_, (const uint32_t *)len_, (float *)out_, cap_,
                                                 nullptr, nullptr));
        std::vector<float> out(n);
        grail::check(grail_memcpy_d2h(ctx_, out.data(), out_, n * sizeof(float)));
        return out;
    }
    // the row ends: what the filter rings out on +0.0 input (nothing if it was fed nothing)
    std::vector<float> finish()
    {
        room(tail_ ? tail_ : 1u);
        uint32_t n = 0;
        grail::check(grail_iir_stream_finish_async(ctx_, stream_, nullptr, (float *)out_, cap_, (uint32_t *)len_));
        grail::check(grail_memcpy_d2h(ctx_, &n, len_, sizeof n));
        std::vector<float> out(n);
        if (n) grail::check(grail_memcpy_d2h(ctx_, out.data(), out_, n * sizeof(float)));
        return out;
    }

private:
    void room(size_t samples)
    {
        if (!len_) grail::check(grail_device_alloc(ctx_, sizeof(uint32_t), &len_));
        if (samples <= cap_) return;
        grail::check(grail_sync(ctx_));
        for (void **p : {&in_, &out_}) {
            grail_device_free(ctx_, *p);
            *p = nullptr;
        }
        cap_ = (samples + 63) / 64 * 64;
        grail::check(grail_device_alloc(ctx_, cap_ * sizeof(float), &in_));
        grail::check(grail_device_alloc(ctx_, cap_ * sizeof(float), &out_));
    }
    grail_ctx *ctx_;
    uint32_t tail_;
    grail_iir *set_ = nullptr;
    grail_iir_stream *stream_ = nullptr;
    void *in_ = nullptr, *out_ = nullptr, *len_ = nullptr;
    size_t cap_ = 0;
};

// --meter: a meter stream of one row on what leaves the chain, through the C ABI (grail_meter_stream_*).  The ledger holds an
// hour of hops; a session that outgrows it is refused from there on, and the report says so.
class Meter {
public:
    Meter(grail_ctx *ctx, uint32_t rate) : ctx_(ctx), rate_(rate)
    {
        grail::check(grail_meter_stream_open(ctx, 1, rate, nullptr, 36000, &ms_));
    }
    Meter(const Meter &) = delete;
    Meter &operator=(const Meter &) = delete;
    ~Meter()
    {
        grail_meter_stream_close(ctx_, ms_);
        for (void *p : {in_, len_, res_}) grail_device_free(ctx_, p);
    }
    // the samples just written go back to the device and through the meter where they lie
    void feed(const std::vector<float> &part)
    {
        if (part.empty()) return;
        if (part.size() > cap_) {
            grail::check(grail_sync(ctx_));
            grail_device_free(ctx_, in_);
            in_ = nullptr;
            cap_ = (part.size() + 63) / 64 * 64;
            grail::check(grail_device_alloc(ctx_, cap_ * sizeof(float), &in_));
        }
        if (!len_) grail::check(grail_device_alloc(ctx_, sizeof(uint32_t), &len_));
        if (!res_) grail::check(grail_device_alloc(ctx_, 5 * sizeof(double), &res_));
        const uint32_t n = (uint32_t)part.size();
        grail::check(grail_memcpy_h2d(ctx_, in_, part.data(), n * sizeof(float)));
        grail::check(grail_memcpy_h2d(ctx_, len_, &n, sizeof n));
        uint32_t n_hops = 0;
        grail::check(grail_meter_stream_next_async(ctx_, ms_, (const float *)in_, cap_, (const uint32_t *)len_, nullptr, 0,
                                                   (uint32_t *)res_, nullptr, nullptr));
        grail::check(grail_memcpy_d2h(ctx_, &n_hops, res_, sizeof n_hops));
        full_ = full_ || n_hops == GRAIL_LIMIT_REFUSED;
    }
    // the row ends; I, max M, max S, LRA and TP as grail_dialogue --report prints them, then the two numbers' own bits
    void report(uint32_t track)
    {
        if (!res_) grail::check(grail_device_alloc(ctx_, 5 * sizeof(double), &res_));
        double *r = (double *)res_;
        grail::check(grail_meter_stream_finish_async(ctx_, ms_, nullptr, nullptr));
        grail::check(grail_meter_stream_read_async(ctx_, ms_, r, r + 1, r + 2, r + 3, (uint64_t *)(r + 4)));
        double got[4];
        uint64_t hops = 0;
        grail::check(grail_memcpy_d2h(ctx_, got, r, sizeof got));
        grail::check(grail_memcpy_d2h(ctx_, &hops, r + 4, sizeof hops));
        const double *ledger = nullptr;
        uint64_t stride = 0;
        grail::check(grail_meter_stream_ledger(ctx_, ms_, &ledger, &stride));
        std::vector<double> h((size_t)hops);
        if (hops) grail::check(grail_memcpy_d2h(ctx_, h.data(), ledger, h.size() * sizeof(double)));
        const uint32_t H = rate_ / 10u;
        const double short_max = grail_loudness_lufs(grail_loudness_window_max(h.data(), (uint32_t)hops, H, 30));
        const auto field = [](bool has, double value, const char *unit) {
            char text[48];
            if (has && std::isfinite(value)) std::snprintf(text, sizeof text, "%.2f %s", value, unit);
            else std::snprintf(text, sizeof text, "-");
            return std::string(text);
        };
        std::fprintf(stderr, "Track %u: integrated %s, range %s, max momentary %s, max short-term %s, true peak %s\n", track,
                     field(got[0] > 0.0, grail_loudness_lufs(got[0]), "LUFS").c_str(),
                     field(hops >= 30 && short_max > -70.0, grail_loudness_range(h.data(), (uint32_t)hops, H), "LU").c_str(),
                     field(hops >= 4, grail_loudness_lufs(grail_loudness_window_max(h.data(), (uint32_t)hops, H, 4)), "LUFS").c_str(),
                     field(hops >= 30, short_max, "LUFS").c_str(), field(got[3] > 0.0, grail_true_peak_db(got[3]), "dBTP").c_str());
        std::fprintf(stderr, "Metered at %u Hz: %llu hops, gated mean square %a, true peak %a%s\n", rate_, (unsigned long long)hops,
                     got[0], got[3], full_ ? " (the ledger was full: the end of the session is not in these numbers)" : "");
    }

private:
    grail_ctx *ctx_;
    uint32_t rate_;
    grail_meter_stream *ms_ = nullptr;
    void *in_ = nullptr, *len_ = nullptr, *res_ = nullptr;
    size_t cap_ = 0;
    bool full_ = false;
};

}  // namespace

int main(int argc, char **argv)
{
    std::vector<const char *> plain;
    double lo = -1.0, hi = -1.0;
    long taps = 0, rate = 0, lookahead = -1;
    double ceiling_db = 0.0;
    bool usage = false, limit = false, meter = false;
    EqOption eq_option;
    for (int i = 1; i < argc; ++i) {
        const std::string a = argv[i];
        char *end = nullptr;
        if (a == "--band" && i + 2 < argc) {
            lo = std::strtod(argv[i + 1], &end);
            usage = usage || end == argv[i + 1] || *end;
            hi = std::strtod(argv[i + 2], &end);
            usage = usage || end == argv[i + 2] || *end;
            i += 2;
        } else if (a == "--taps" && i + 1 < argc) {
            taps = std::strtol(argv[i + 1], &end, 10);
            usage = usage || end == argv[i + 1] || *end || taps < 3 || taps > GRAIL_FIR_TAPS_MAX || taps % 2 == 0;
            i += 1;
        } else if (a == "--ceiling" && i + 1 < argc) {
            ceiling_db = std::strtod(argv[i + 1], &end);
            // (written so that a NaN fails; the ceiling must come out a finite float above 0)
            usage = usage || end == argv[i + 1] || *end || !(ceiling_db >= -300.0 && ceiling_db <= 300.0);
            limit = true;
            i += 1;
        } else if (a == "--lookahead" && i + 1 < argc) {
            lookahead = std::strtol(argv[i + 1], &end, 10);
            usage = usage || end == argv[i + 1] || *end || lookahead < 0 || lookahead > GRAIL_LIMIT_LOOKAHEAD_LOG2_MAX;
            i += 1;
        } else if (a == "--rate" && i + 1 < argc) {
            rate = std::strtol(argv[i + 1], &end, 10);
            // (the voice's own rate is refused with the others: equal rates are no conversion)
            usage = usage || end == argv[i + 1] || *end || rate < 1 || rate > 0xFFFFFFFFl ||
                    grail_resample_ratio((uint32_t)grail::voices::generic().sample_rate, (uint32_t)rate, nullptr, nullptr, nullptr) != GRAIL_OK;
            i += 1;
        } else if (a == "--eq") {
            eq_option.take(argc, argv, i);
        } else if (a == "--meter") {
            meter = true;
        } else if (a.rfind("--", 0) == 0) {
            usage = true;
        } else {
            plain.push_back(argv[i]);
        }
    }
    const bool band = hi >= 0.0;
    const uint32_t chunk = plain.size() > 0 ? (uint32_t)std::strtoul(plain[0], nullptr, 10) : 441;
    const double tail = plain.size() > 1 ? std::strtod(plain[1], nullptr) : 1.0;
    // (--eq runs at the rate that is written: the designer refuses what it cannot make there)
    const uint32_t out_rate = rate ? (uint32_t)rate : (uint32_t)grail::voices::generic().sample_rate;
    std::vector<double> eq_coef;
    usage = usage || eq_option.bad || !eq_option.design(out_rate, eq_coef);
    // (a chunk of 0 samples — or text strtoul makes 0 of — would never feed the stream)
    if (usage || plain.size() > 2 || chunk == 0 || !(tail >= 0.0) || (taps && !band) || (band && !(lo >= 0.0 && lo < hi)) ||
        (lookahead >= 0 && !limit)) {
        std::fprintf(stderr, "usage: grail_interactive [--band LO HI [--taps K]] [--ceiling DB [--lookahead l]] [--rate R] [--eq KIND:F0:Q[:GAIN]]... "
                             "[--meter] [samples per pull >= 1 (default 441)] [seconds of tail >= 0 (default 1)]\n");
        return 2;
    }
    try {
        const grail::Voice voice = grail::voices::generic();       // interactive.rs:33-36
        grail::Gpu gpu(0, {voice});
        // --band: one filter, one row; the stream is declared after its set, so it is closed first
        std::vector<grail::FirSet> sets;
        std::vector<grail::FirStream> filters;
        if (band) {
            sets.push_back(gpu.fir_set({grail::fir_design((uint32_t)voice.sample_rate, lo, hi, taps ? (uint32_t)taps : 255u)}));
            filters.push_back(gpu.fir_stream(sets[0], 1));
        }
        std::vector<grail::LimitStream> limiters;
        if (limit) limiters.push_back(gpu.limit_stream(1, grail_limit_ceiling((float)ceiling_db), lookahead < 0 ? 8u : (uint32_t)lookahead));
        std::vector<grail::ResampleStream> resamplers;
        if (rate) resamplers.push_back(gpu.resample_stream((uint32_t)voice.sample_rate, (uint32_t)rate, 1));
        // (declared after the other streams: closed before them)
        std::unique_ptr<Eq> equaliser;
        if (eq_option.given()) equaliser.reset(new Eq(gpu.ctx(), eq_coef, out_rate / 10u));
        std::unique_ptr<Meter> metered;
        if (meter) metered.reset(new Meter(gpu.ctx(), rate ? (uint32_t)rate : (uint32_t)voice.sample_rate));
        std::vector<Line> script;
        std::string raw;
        while (std::getline(std::cin, raw)) {                        // interactive.rs:77-81
            Line l{0.0, raw};
            if (!raw.empty() && raw[0] == '@') {
                char *end = nullptr;
                l.at = std::strtod(raw.c_str() + 1, &end);
                l.text = end ? std::string(end) : std::string();
            }
            script.push_back(l);
        }
        grail::LiveStream chain(gpu, chunk, 0, 0);                   // .jitter(0, ...) interactive.rs:37
        std::deque<grail::PhonemeElem> waiting;                      // what the transcriber has, the Sequencer has not
        const grail::PhonemeElem silence = speak(voice, "", false).at(0);   // ' ': no rule matches
        size_t next_line = 0, total = 0, fed = 0, written = 0;
        bool first = true, closed = false;
        double close_at = -1.0;
        const char *names[] = {"Silence", "Stop", "Glide", "A", "E"};
        // what leaves the chain: through --eq, to stdout, through --meter
        const auto emit = [&](std::vector<float> samples, bool through_eq = true) {
            if (equaliser && through_eq) samples = equaliser->next(samples);
            std::fwrite(samples.data(), sizeof(float), samples.size(), stdout);
            if (meter) metered->feed(samples);
            written += samples.size();
        };
        for (;;) {
            const double now = (double)total / voice.sample_rate;
            while (next_line < script.size() && script[next_line].at <= now) {      // the channel receives a line
                for (const grail::PhonemeElem &p : speak(voice, script[next_line].text, first)) waiting.push_back(p);
                first = false;
                ++next_line;
            }
            uint32_t rendered = 0;                                    // what the chain rendered in this pull
            std::vector<float> part;
            if (limit) {
                // ... filtered, limited and resampled where it lay
                part = chain.next(band ? &filters[0] : nullptr, limiters[0], rate ? &resamplers[0] : nullptr, &rendered);
            } else if (rate) {
                part = chain.next(band ? &filters[0] : nullptr, resamplers[0], &rendered);    // ... filtered and resampled where it lay
            } else if (band) {
                part = chain.next(filters[0], &rendered);            // ... filtered where it lay
            } else {
                part = chain.next();
                rendered = (uint32_t)part.size();
            }
            emit(part);
            total += rendered;
            if (rendered == chunk) continue;
            if (closed) {
                if (rendered == 0) break;                             // the chain has returned None
                continue;
            }
            // the Sequencer asks its source for the next segment
            if (next_line == script.size() && waiting.empty()) {
                if (close_at < 0.0) close_at = (double)total / voice.sample_rate + tail;
                if ((double)total / voice.sample_rate >= close_at) {
                    chain.finish();
                    closed = true;
                    continue;
                }
            }
            grail::PhonemeElem p = silence;
            if (!waiting.empty()) {
                p = waiting.front();
                waiting.pop_front();
            } else if (first) {
                // nothing has been said yet: the chain's very first pull is the leading Silence of .transcribe()
                first = false;
            }
            chain.append({p});
            std::fprintf(stderr, "fed %s at %zu\n", names[p.phoneme], total);
            ++fed;
        }
        if (band) {                                                   // the chain has ended: the filter rings out
            std::vector<float> rest = filters[0].finish().at(0);
            if (limit) rest = limiters[0].next({rest}).at(0);         // ... into the next stages of the chain
            if (rate) rest = resamplers[0].next({rest}).at(0);
            emit(rest);
            if (rate || limit)
                std::fprintf(stderr, "Filtered %g - %g Hz at %g Hz (%u taps)\n", lo, hi, (double)voice.sample_rate, filters[0].tail() + 1);
            else
                std::fprintf(stderr, "Filtered %g - %g Hz at %g Hz (%u taps): %zu samples written\n", lo, hi,
                             (double)voice.sample_rate, filters[0].tail() + 1, written);
        }
        if (limit) {                                                  // ... the limiter's own tail: what its look-ahead held back
            std::vector<float> rest = limiters[0].finish().at(0);
            if (rate) rest = resamplers[0].next({rest}).at(0);
            emit(rest);
            if (rate)
                std::fprintf(stderr, "Limited to %g dBTP, %u samples late\n", ceiling_db, limiters[0].delay());
            else
                std::fprintf(stderr, "Limited to %g dBTP, %u samples late: %zu samples written\n", ceiling_db, limiters[0].delay(),
                             written);
        }
        if (rate) {                                                   // ... and the resampler's own tail
            const std::vector<float> rest = resamplers[0].finish().at(0);
            emit(rest);
            std::fprintf(stderr, "Resampled %g -> %ld Hz: %zu samples written\n", (double)voice.sample_rate, rate, written);
        }
        if (equaliser) {                                              // ... and the equaliser's: a tenth of a second of ringing
            emit(equaliser->finish(), false);
            std::fprintf(stderr, "Equalised at %u Hz,%s: %zu samples written\n", out_rate, eq_option.text().c_str(), written);
        }
        if (meter) metered->report(1);
        std::fprintf(stderr, "session: %zu samples (%.2f s), %zu phonemes fed, %zu lines, buffers of %u\n", total,
                     total / voice.sample_rate, fed, script.size(), chunk);
    } catch (const grail::Error &e) {
        std::fprintf(stderr, "grail_interactive: %s (status %d)\n", e.what(), e.status);
        return 1;
    }
    return 0;
}
