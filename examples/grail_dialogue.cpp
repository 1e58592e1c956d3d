// grail_dialogue — two lines of text by two voices, laid one after the other on a timeline (grail_mix_place_sequential),
// the first voice panned left and the second right, mixed on an MI355X (grail::Gpu::mix) and written as a stereo WAV.
//   usage: grail_dialogue [-o out.wav] [--level DB | --lufs L] [--ceiling DBTP [--limit]] [--band LO HI [--taps K]] [--eq KIND:F0:Q[:GAIN]]... [--eq-blocked] [--compress T:R[:KNEE[:ATTACK_MS:RELEASE_MS]] [--makeup DB]] [--compress-tracks] [--rate R] [--report] "first line" "second line"
// --level DB brings both lines to that RMS level (decibels, 0 dB = an RMS of 1.0) before they are panned: the rows are
// measured on the device and the gains follow from their levels (grail::Gpu::mix_leveled).  --lufs L brings them to a
// K-weighted gated loudness of L LUFS instead (GRAIL_LEVEL_LOUDNESS; a line shorter than 400 ms cannot be leveled).
// --ceiling DBTP (with --level or --lufs) holds every placement under that true peak as well: the rows' true peaks are
// measured on the device and cap the gains (grail_batch_mix_leveled_limited), and the two finished tracks are measured
// the same way (grail::Gpu::true_peak); "--lufs -23 --ceiling -1" is the delivery rule of EBU R 128.
// --limit (with --ceiling) then passes the two finished tracks, as one linked pair, through the look-ahead limiter
// (grail::Gpu::limit) with the largest power of two of samples within 5 ms as look-ahead, and prints the tracks' true
// peaks before and after: what placements that overlap, or the mix's own rounding, left above the ceiling gives way there.
// --band LO HI passes the two mixed tracks, at the voices' rate, after the mix and before the limiter, through one band-pass
// of LO .. HI Hz (grail::fir_design, a Kaiser window of --taps K taps, K odd, 255 unless said; grail::Gpu::fir): "--band 300
// 3400 --rate 8000" is a telephone line.  The tracks keep their length (the filter has zero delay; its tail past the end is
// dropped).  A filter overshoots, so with --ceiling the line that states the tracks' true peaks is measured after it.
// --eq KIND:F0:Q[:GAIN] (up to eight times) passes the two mixed tracks, after --band and before the limiter, through one
// recursive filter of as many biquad sections as there are --eq (grail_iir_design at the voices' rate, grail_iir_async): KIND is
// lowpass, highpass, bandpass, notch, peak, lowshelf or highshelf, F0 in Hz, GAIN in dB for peak and the shelves:
// "--eq highpass:100:0.707 --eq peak:3000:1.5:4" is a high-pass under the voices and a presence peak.  The tracks keep their
// length (no tail).  A filter overshoots, so with --ceiling the tracks' true peaks are measured after it.
// --eq-blocked (with --eq) filters them with grail_biquad_blocked_async instead, the form parallel in time that is meant for a few
// long tracks: the same samples up to the 1024th, within a rounding of the 16-bit scale after it.  The line printed names the call.
// --compress T:R[:KNEE[:ATTACK_MS:RELEASE_MS]] passes the two mixed tracks, after --eq and before the limiter, through a soft-knee
// compressor on the peak detector (grail_dyn_design, grail_dyn_ballistics at the voices' rate, grail_dyn_async; each track follows
// itself): threshold T in dB, ratio R >= 1, a knee of KNEE dB (6 unless given), attack and release in milliseconds (5 and 120
// unless given).  --makeup DB (with --compress) is built into the curve.  Prints each track's largest gain reduction in dB.  The
// make-up can lift peaks, so with --ceiling the tracks' true peaks are measured after it.
// --compress-tracks (with --compress) compresses them with grail_track_dyn_async instead, a workgroup a track, the form that is
// meant for a few long tracks: the same samples, bit for bit.  The line printed names the call.
// --rate R resamples the two finished tracks, after the mix and the limiter, from the voices' 44 100 Hz to R Hz on the device
// (grail::Gpu::resample) and writes the WAV at R; the filter overshoots a little, so the line it prints has the tracks'
// true peaks at R.
// --report measures the two finished tracks, after the last stage that ran and at the rate of what is written, as a meter would (grail::Gpu::track_loudness,
// parallel in time, and grail::Gpu::true_peak) and prints one line per track: integrated loudness, loudness range, largest
// momentary and short-term loudness, true peak; "-" where a track is too short (or too quiet) for a number.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <utility>
#include <vector>

#include "eq_option.h"
#include "grail.hpp"

int main(int argc, char **argv)
{
    std::string out_path = "dialogue.wav";
    std::vector<std::string> lines;
    bool leveled = false, bad_level = false, lufs = false;
    bool capped = false, bad_ceiling = false, limit = false, report = false, bad_report = false;
    float level_db = 0.0f, ceiling_db = 0.0f;
    bool resampled = false, bad_rate = false;
    uint32_t rate = 0;
    bool band = false, bad_band = false, taps_given = false;
    double band_lo = 0.0, band_hi = 0.0;
    uint32_t band_taps = 255;
    EqOption eq_option;
    bool eq_blocked = false;
    bool compress = false, bad_compress = false, makeup_given = false, compress_by_track = false;
    double comp[5] = {0.0, 1.0, 6.0, 5.0, 120.0}, makeup_db = 0.0;        // T, R, knee, attack ms, release ms
    for (int i = 1; i < argc; ++i) {
        if ((!std::strcmp(argv[i], "-o") || !std::strcmp(argv[i], "--output")) && i + 1 < argc) out_path = argv[++i];
        else if ((!std::strcmp(argv[i], "--level") || !std::strcmp(argv[i], "--lufs")) && i + 1 < argc) {
            lufs = !std::strcmp(argv[i], "--lufs");
            char *rest = nullptr;
            level_db = std::strtof(argv[++i], &rest);
            leveled = true;
            bad_level = rest == argv[i] || *rest || !std::isfinite(level_db);
        } else if (!std::strcmp(argv[i], "--ceiling") && i + 1 < argc) {
            char *rest = nullptr;
            ceiling_db = std::strtof(argv[++i], &rest);
            capped = true;
            bad_ceiling = rest == argv[i] || *rest || !std::isfinite(ceiling_db);
        } else if (!std::strcmp(argv[i], "--rate") && i + 1 < argc) {
            char *rest = nullptr;
            const unsigned long long r = std::strtoull(argv[++i], &rest, 10);
            resampled = true;
            rate = (uint32_t)r;
            bad_rate = rest == argv[i] || *rest || argv[i][0] == '-' || r == 0 || r > 0xFFFFFFFFull;
        } else if (!std::strcmp(argv[i], "--band")) {
            band = true;
            bad_band = i + 2 >= argc;
            if (!bad_band) {
                char *rest_lo = nullptr, *rest_hi = nullptr;
                band_lo = std::strtod(argv[i + 1], &rest_lo);
                band_hi = std::strtod(argv[i + 2], &rest_hi);
                bad_band = rest_lo == argv[i + 1] || *rest_lo || rest_hi == argv[i + 2] || *rest_hi || !(band_lo >= 0.0 && band_lo < band_hi);
                i += 2;
            }
        } else if (!std::strcmp(argv[i], "--taps") && i + 1 < argc) {
            char *rest = nullptr;
            const unsigned long long k = std::strtoull(argv[++i], &rest, 10);
            taps_given = true;
            band_taps = (uint32_t)k;
            bad_band = bad_band || rest == argv[i] || *rest || argv[i][0] == '-' || k < 3 || k > GRAIL_FIR_TAPS_MAX || k % 2 == 0;
        } else if (!std::strcmp(argv[i], "--eq")) eq_option.take(argc, argv, i);      // (examples/eq_option.h)
        else if (!std::strcmp(argv[i], "--eq-blocked")) eq_blocked = true;
        else if (!std::strcmp(argv[i], "--compress-tracks")) compress_by_track = true;
        else if (!std::strcmp(argv[i], "--compress")) {
            bad_compress = bad_compress || compress || i + 1 >= argc;      // (named twice, or without a value)
            compress = true;
            if (i + 1 < argc) {     // two, three or five numbers between colons
                const char *at = argv[++i];
                int fields = 0;
                for (;; ++at) {
                    char *rest = nullptr;
                    const double v = std::strtod(at, &rest);
                    if (rest == at || fields == 5 || !std::isfinite(v)) { bad_compress = true; break; }
                    comp[fields++] = v;
                    at = rest;
                    if (*at != ':') break;
                }
                bad_compress = bad_compress || *at || (fields != 2 && fields != 3 && fields != 5);
            }
        } else if (!std::strcmp(argv[i], "--makeup") && i + 1 < argc) {
            char *rest = nullptr;
            makeup_db = std::strtod(argv[++i], &rest);
            bad_compress = bad_compress || makeup_given || rest == argv[i] || *rest || !std::isfinite(makeup_db);
            makeup_given = true;
        }
        else if (!std::strcmp(argv[i], "--limit")) limit = true;
        else if (!std::strcmp(argv[i], "--report")) {
            bad_report = report;        // (named twice)
            report = true;
        } else if (!std::strncmp(argv[i], "--report", 8)) bad_report = true;        // (it takes no value)
        else lines.push_back(argv[i]);
    }
    // (the voices are the generic ones, at 44 100 Hz: a band that ends above their Nyquist frequency is said here, and the
    // sections of --eq are designed: the designer refuses what it cannot make)
    std::vector<double> eq;         // five numbers a section
    const bool bad_eq = eq_option.bad || !eq_option.design(44100, eq) || (eq_blocked && eq.empty());
    bad_band = bad_band || (taps_given && !band) || (band && band_hi > 22050.0);
    // (the curve and the alphas of --compress are made here: the designer refuses what it cannot make)
    std::vector<double> comp_gain(GRAIL_DYN_POINTS);
    double comp_alpha[2] = {0.0, 0.0};
    bad_compress = bad_compress || (makeup_given && !compress) || (compress_by_track && !compress) ||
                   (compress && (grail_dyn_design(GRAIL_DYN_COMPRESS, GRAIL_DYN_PEAK, comp[0], comp[1], comp[2], 0.0, makeup_db, comp_gain.data()) ||
                                 grail_dyn_ballistics(44100, comp[3], comp[4], comp_alpha)));
    if (lines.size() != 2 || bad_level || bad_ceiling || bad_report || bad_rate || bad_band || bad_eq || bad_compress || (capped && !leveled) || (limit && !capped)) {
        std::fprintf(stderr, "usage: grail_dialogue [-o out.wav] [--level DB | --lufs L] [--ceiling DBTP [--limit]] [--band LO HI [--taps K]] "
                             "[--eq KIND:F0:Q[:GAIN]]... [--eq-blocked] [--compress T:R[:KNEE[:ATTACK_MS:RELEASE_MS]] [--makeup DB]] [--compress-tracks] [--rate R] [--report] \"first line\" \"second line\"\n       (--ceiling needs --level or --lufs, --limit "
                             "needs --ceiling, --band takes 0 <= LO < HI <= 22050 Hz, --taps an odd number from 3 to 4096 and needs "
                             "--band, --eq takes lowpass, highpass, bandpass, notch, peak, lowshelf or highshelf, 0 < F0 < 22050 Hz, Q > 0 and a "
                             "gain in dB, up to eight times, --eq-blocked needs --eq, --compress takes a threshold in dB, a ratio of 1 or more, a knee of 0 dB or more and "
                             "two times of 0 ms or more, once, --makeup and --compress-tracks need --compress, --rate takes a whole number of Hz, --report takes no value)\n");
        return 2;
    }
    try {
        const grail::Voice first = grail::voices::generic();        // 44.1 kHz, as the CLI
        grail::Voice second = first;
        second.center_frequency = first.center_frequency * 1.5f;    // a higher voice
        grail::Gpu gpu(0, {first, second});
        const std::vector<grail::Utterance> utts = {grail::Utterance{grail::phoneme_elems(first, lines[0]), 0, 0},
                                                    grail::Utterance{grail::phoneme_elems(second, lines[1]), 1, 0}};
        const std::vector<uint32_t> lens = gpu.lengths(utts);
        // one timeline: the second line starts 0.3 s after the first has ended
        const uint32_t rows[2] = {0, 1};
        const int64_t gaps[2] = {0, (int64_t)(first.sample_rate * 3.0f / 10.0f)};
        uint64_t at[2] = {0, 0}, end = 0;
        grail::check(grail_mix_place_sequential(lens.data(), 2, rows, nullptr, gaps, 2, 1, at, &end));
        // the first voice left, the second right
        const std::vector<grail::Placement> placements = {
            {0, 0, at[0], 0.8f}, {0, 1, at[0], 0.2f}, {1, 0, at[1], 0.2f}, {1, 1, at[1], 0.8f}};
        std::vector<std::vector<float>> tracks;
        // --band: one designed filter for both tracks, which keep their length
        const auto band_pass = [&]() {
            if (!band) return;
            const uint32_t at_rate = (uint32_t)first.sample_rate;
            const grail::FirSet set = gpu.fir_set({grail::fir_design(at_rate, band_lo, band_hi, band_taps)});
            tracks = gpu.fir(set, tracks, {}, false);
            std::printf("Filtered %g - %g Hz at %u Hz (%u taps)\n", band_lo, band_hi, at_rate, band_taps);
        };
        // --eq: one recursive filter of as many sections as were named, for both tracks, which keep their length (the C ABI on
        // the Gpu's context: the facade has no class for it yet)
        const auto equalise = [&]() {
            if (eq.empty()) return;
            grail_ctx *ctx = gpu.ctx();
            const uint32_t sections = (uint32_t)(eq.size() / 5), n = (uint32_t)tracks.size();
            const uint64_t stride = ((uint64_t)end + 63) / 64 * 64;
            grail_iir *set = nullptr;
            grail::check(grail_iir_create(ctx, eq.data(), &sections, 1, &set));
            void *d_rows = nullptr, *d_out = nullptr, *d_len = nullptr;
            int rc = grail_device_alloc(ctx, n * stride * 4, &d_rows);
            if (!rc) rc = grail_device_alloc(ctx, n * stride * 4, &d_out);
            if (!rc) rc = grail_device_alloc(ctx, n * 4, &d_len);
            std::vector<uint32_t> track_len;
            for (const std::vector<float> &t : tracks) track_len.push_back((uint32_t)t.size());
            for (uint32_t t = 0; t < n && !rc; ++t)
                rc = grail_memcpy_h2d(ctx, (float *)d_rows + t * stride, tracks[t].data(), tracks[t].size() * 4);
            if (!rc) rc = grail_memcpy_h2d(ctx, d_len, track_len.data(), n * 4);
            if (!rc) rc = (eq_blocked ? grail_biquad_blocked_async : grail_iir_async)(ctx, set, (const float *)d_rows, stride, (const uint32_t *)d_len, n, nullptr, 0, (float *)d_out, stride, nullptr, nullptr);
            for (uint32_t t = 0; t < n && !rc; ++t)
                rc = grail_memcpy_d2h(ctx, tracks[t].data(), (const float *)d_out + t * stride, tracks[t].size() * 4);
            for (void *p : {d_rows, d_out, d_len})
                if (p) grail_device_free(ctx, p);
            const int freed = grail_iir_free(ctx, set);
            grail::check(rc ? rc : freed);
            std::printf("Equalised (%s), %u section%s:", eq_blocked ? "grail_biquad_blocked_async" : "grail_iir_async", sections, sections == 1 ? "" : "s");
            std::printf("%s\n", eq_option.text().c_str());
        };
        // --compress: one curve for both tracks, each following itself; they keep their length (the C ABI, as --eq)
        const auto compress_tracks = [&]() {
            if (!compress) return;
            grail_ctx *ctx = gpu.ctx();
            const uint32_t n = (uint32_t)tracks.size(), detector = GRAIL_DYN_PEAK;
            const uint64_t stride = ((uint64_t)end + 63) / 64 * 64;
            grail_dyn *set = nullptr;
            grail::check(grail_dyn_create(ctx, comp_gain.data(), comp_alpha, &detector, 1, &set));
            void *d_rows = nullptr, *d_out = nullptr, *d_len = nullptr, *d_gain = nullptr;
            int rc = grail_device_alloc(ctx, n * stride * 4, &d_rows);
            if (!rc) rc = grail_device_alloc(ctx, n * stride * 4, &d_out);
            if (!rc) rc = grail_device_alloc(ctx, n * 4, &d_len);
            if (!rc) rc = grail_device_alloc(ctx, n * 8, &d_gain);
            std::vector<uint32_t> track_len;
            for (const std::vector<float> &t : tracks) track_len.push_back((uint32_t)t.size());
            for (uint32_t t = 0; t < n && !rc; ++t)
                rc = grail_memcpy_h2d(ctx, (float *)d_rows + t * stride, tracks[t].data(), tracks[t].size() * 4);
            if (!rc) rc = grail_memcpy_h2d(ctx, d_len, track_len.data(), n * 4);
            if (!rc) rc = (compress_by_track ? grail_track_dyn_async : grail_dyn_async)(ctx, set, (const float *)d_rows, stride, (const uint32_t *)d_len, n, nullptr, nullptr, 0, nullptr, 0, nullptr,
                                                                                      (float *)d_out, stride, nullptr, nullptr, (double *)d_gain);
            for (uint32_t t = 0; t < n && !rc; ++t)
                rc = grail_memcpy_d2h(ctx, tracks[t].data(), (const float *)d_out + t * stride, tracks[t].size() * 4);
            std::vector<double> min_gain(n, 1.0);
            if (!rc) rc = grail_memcpy_d2h(ctx, min_gain.data(), d_gain, n * 8);
            for (void *p : {d_rows, d_out, d_len, d_gain})
                if (p) grail_device_free(ctx, p);
            const int freed = grail_dyn_free(ctx, set);
            grail::check(rc ? rc : freed);
            std::printf("Compressed (%s) above %g dB at %g:1, knee %g dB, attack %g ms, release %g ms, make-up %g dB: largest gain reduction",
                        compress_by_track ? "grail_track_dyn_async" : "grail_dyn_async", comp[0], comp[1], comp[2], comp[3], comp[4], makeup_db);
            for (uint32_t t = 0; t < n; ++t)    // (the curve holds the make-up: the reduction is what lies under it)
                std::printf("%s %.2f dB", t ? " and" : "", makeup_db - 20.0 * std::log10(min_gain[t]));
            std::printf("\n");
        };
        if (leveled) {          // the same pan as a level: 0.8 and 0.2 of the line at level_db
            std::vector<float> levels, gains;
            for (const grail::Placement &p : placements) levels.push_back(level_db + 20.0f * std::log10(p.gain));
            uint32_t unleveled = 0, limited = 0;
            const int mode = lufs ? GRAIL_LEVEL_LOUDNESS : GRAIL_LEVEL_RMS;
            tracks = capped ? gpu.mix_leveled_limited(utts, placements, levels, ceiling_db, 2, end, mode, &gains, &unleveled, &limited)
                            : gpu.mix_leveled(utts, placements, levels, 2, end, mode, &gains, &unleveled);
            band_pass();
            equalise();
            compress_tracks();
            if (lufs)
                std::printf("Lines brought to %.1f LUFS: gains %.4g and %.4g%s\n", level_db, gains[0] / 0.8f, gains[3] / 0.8f,
                            unleveled ? " (a silent line or one shorter than 400 ms was left out)" : "");
            else
                std::printf("Lines brought to %.1f dB RMS: gains %.4g and %.4g%s\n", level_db, gains[0] / 0.8f,
                            gains[3] / 0.8f, unleveled ? " (a silent line was left out)" : "");
            if (capped) {
                const grail::TruePeak tp = gpu.true_peak(tracks);
                std::printf("Ceiling %.1f dBTP: %u of 4 placements limited; track true peaks %.6f and %.6f dBTP\n", ceiling_db,
                            limited, tp.db(0), tp.db(1));
                if (limit) {    // the finished tracks as one linked pair; the largest power of two within rate / 200
                    uint32_t lookahead_log2 = 0;
                    while (lookahead_log2 < GRAIL_LIMIT_LOOKAHEAD_LOG2_MAX && (2u << lookahead_log2) <= (uint32_t)first.sample_rate / 200u)
                        ++lookahead_log2;
                    grail::Limited held = gpu.limit(tracks, grail::limit_ceiling(ceiling_db), lookahead_log2, 2);
                    const grail::TruePeak after = gpu.true_peak(held.rows);
                    std::printf("Limiter, %u samples of look-ahead: %u samples limited, smallest gain %.6f; track true peaks %.6f and "
                                "%.6f dBTP before, %.6f and %.6f dBTP after\n", 1u << lookahead_log2, held.n_limited[0],
                                held.min_gain[0], tp.db(0), tp.db(1), after.db(0), after.db(1));
                    tracks = std::move(held.rows);
                }
            }
        } else {
            tracks = gpu.mix(utts, placements, 2, end);
            band_pass();
            equalise();
            compress_tracks();
        }
        uint32_t out_rate = (uint32_t)first.sample_rate;
        if (resampled && rate != out_rate) {    // (the voices' own rate: nothing to do, and the library refuses equal rates)
            tracks = gpu.resample(tracks, out_rate, rate);
            const grail::TruePeak tp = gpu.true_peak(tracks);
            std::printf("Resampled from %u to %u Hz: %zu samples a track; track true peaks %.6f and %.6f dBTP\n", out_rate, rate,
                        tracks[0].size(), tp.db(0), tp.db(1));
            out_rate = rate;
        }
        if (report) {           // the finished tracks as a meter reads them; "-" where there is no number
            const grail::TrackLoudness loud = gpu.track_loudness(tracks, out_rate);
            const grail::TruePeak peak = gpu.true_peak(tracks);
            const auto field = [](bool has, double value, const char *unit) {
                char text[48];
                if (has && std::isfinite(value)) std::snprintf(text, sizeof text, "%.2f %s", value, unit);
                else std::snprintf(text, sizeof text, "-");
                return std::string(text);
            };
            for (size_t t = 0; t < tracks.size(); ++t) {
                const size_t hops = loud.hop_sumsq[t].size();
                std::printf("Track %zu: integrated %s, range %s, max momentary %s, max short-term %s, true peak %s\n", t + 1,
                            field(loud.gated_ms[t] > 0.0, loud.lufs(t), "LUFS").c_str(),
                            field(hops >= 30 && loud.short_term_max(t) > -70.0, loud.range(t), "LU").c_str(),
                            field(hops >= 4, loud.momentary_max(t), "LUFS").c_str(),
                            field(hops >= 30, loud.short_term_max(t), "LUFS").c_str(),
                            field(peak.true_peak[t] > 0.0, peak.db(t), "dBTP").c_str());
            }
        }
        std::printf("%.2f seconds of stereo audio: \"%s\" (left), \"%s\" (right)\n", end / first.sample_rate,
                    lines[0].c_str(), lines[1].c_str());
        std::printf("Writing the dialogue to %s\n", out_path.c_str());
        gpu.save_wav_frames(out_path, tracks, out_rate);
    } catch (const grail::Error &e) {
        std::fprintf(stderr, "grail_dialogue: %s (status %d)\n", e.what(), e.status);
        return 1;
    }
    return 0;
}
