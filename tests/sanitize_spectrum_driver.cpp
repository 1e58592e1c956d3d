// Drives the pure-host side of short-time spectra (csrc/spectrum_plan.cpp: grail_spectrum_twiddles, grail_spectrum_frames,
// grail_spectrum_window, grail_mel_design, a set's checks and image, the checks and the grid of grail_spectrum_async) under
// AddressSanitizer and UBSan (tests/test_spectrum_sanitize.py builds and runs it): every array lives on the heap at exactly the
// size the call is entitled to, so that a read or write one element past it is caught; the designers at the smallest and the
// largest transform, bands at both edges of 0 .. N/2, and every refusal.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <memory>
#include <vector>

#include "../include/grail_hip.h"
#include "../grail-rs_amd/csrc/spectrum_plan.h"

#define CHECK(cond)                                                                  \
    do {                                                                             \
        if (!(cond)) {                                                               \
            std::fprintf(stderr, "sanitize spectrum driver: %s failed (line %d)\n", #cond, __LINE__); \
            return 1;                                                                \
        }                                                                            \
    } while (0)

using namespace grail;

static bool says(const char *why, const char *word) { return why && std::strstr(why, word); }

int main()
{
    const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
    const float nanf = std::numeric_limits<float>::quiet_NaN(), inff = std::numeric_limits<float>::infinity();

    // the designers at p = 6 and p = 12, into exactly what they may write
    for (uint32_t p : {6u, 12u}) {
        const uint32_t N = 1u << p;
        std::unique_ptr<double[]> tw(new double[N]);
        CHECK(grail_spectrum_twiddles(p, tw.get()) == GRAIL_OK);
        CHECK(tw[0] == 1.0 && tw[1] == 0.0 && tw[2u * (N / 4u)] == 0.0 && tw[2u * (N / 4u) + 1u] == -1.0);
        for (uint32_t j = 1; j < N / 4u; ++j) {
            CHECK(tw[2u * (N / 2u - j)] == -tw[2u * j] && tw[2u * (N / 2u - j) + 1u] == tw[2u * j + 1u]);
            CHECK(std::fabs(tw[2u * j] * tw[2u * j] + tw[2u * j + 1u] * tw[2u * j + 1u] - 1.0) < 1e-15);
        }
        for (int kind : {GRAIL_SPECTRUM_RECT, GRAIL_SPECTRUM_HANN, GRAIL_SPECTRUM_HAMMING})
            for (uint32_t W : {1u, N - 1u, N}) {
                std::unique_ptr<float[]> w(new float[W]);
                CHECK(grail_spectrum_window(kind, W, w.get()) == GRAIL_OK);
                for (uint32_t j = 0; j < W; ++j) CHECK(w[j] >= 0.0f && w[j] <= 1.0f);
            }
        for (uint32_t B : {1u, 40u, 256u}) {
            std::unique_ptr<uint32_t[]> first(new uint32_t[B]), count(new uint32_t[B]);
            uint32_t total = 0;
            const int sized = grail_mel_design(16000, p, B, 0.0, 8000.0, first.get(), count.get(), nullptr, 0, &total);
            CHECK(sized == (total ? GRAIL_ERR_BUFFER_TOO_SMALL : GRAIL_OK));
            CHECK(total > 0 && total <= B * (N / 2u + 1u));
            std::unique_ptr<float[]> wt(new float[total]);
            uint32_t again = 0;
            CHECK(grail_mel_design(16000, p, B, 0.0, 8000.0, first.get(), count.get(), wt.get(), total - 1u, &again) == GRAIL_ERR_BUFFER_TOO_SMALL);
            CHECK(grail_mel_design(16000, p, B, 0.0, 8000.0, first.get(), count.get(), wt.get(), total, &again) == GRAIL_OK && again == total);
            uint32_t sum = 0;
            for (uint32_t b = 0; b < B; ++b) {
                CHECK(first[b] + count[b] <= N / 2u + 1u);
                sum += count[b];
            }
            CHECK(sum == total);
            for (uint32_t k = 0; k < total; ++k) CHECK(wt[k] > 0.0f && wt[k] <= 1.0f);
            // ... and, where a set can hold them, what a set's checks and image make of them
            std::unique_ptr<float[]> win(new float[N]);
            CHECK(grail_spectrum_window(GRAIL_SPECTRUM_HANN, N, win.get()) == GRAIL_OK);
            const char *why = spectrum_set_error(p, win.get(), N, 1, N - 1u, B, first.get(), count.get(), wt.get());
            if (total > GRAIL_SPECTRUM_WEIGHTS_MAX) {
                CHECK(says(why, "more than 65 536"));
                continue;
            }
            CHECK(!why);
            std::vector<double> image;
            std::vector<uint32_t> desc;
            std::vector<float> weights;
            spectrum_set_image(p, B, first.get(), count.get(), wt.get(), image, desc, weights);
            CHECK(image.size() == N && desc.size() == (size_t)B * SPECTRUM_BAND_WORDS && weights.size() == total);
            CHECK(std::memcmp(image.data(), tw.get(), N * sizeof(double)) == 0);
            for (uint32_t b = 0; b < B; ++b) CHECK(desc[4u * b] == first[b] && desc[4u * b + 1u] == count[b] && desc[4u * b + 2u] + count[b] <= total);
        }
        // the edges of the band range: lo = 0 puts the first triangle's left foot on bin 0, which is then not above 0; hi =
        // rate / 2 puts the last one's right foot on bin N/2 or a rounding beside it
        std::unique_ptr<uint32_t[]> first(new uint32_t[2]), count(new uint32_t[2]);
        std::unique_ptr<float[]> wt(new float[2u * (N / 2u + 1u)]);
        uint32_t total = 0;
        CHECK(grail_mel_design(8000, p, 2, 0.0, 4000.0, first.get(), count.get(), wt.get(), 2u * (N / 2u + 1u), &total) == GRAIL_OK);
        CHECK(first[0] == 1 && first[1] + count[1] >= N / 2u && first[1] + count[1] <= N / 2u + 1u);
    }

    // bands at the edges of 0 .. N/2 by hand: the single bins 0 and N/2, the whole range, empty bands at either end
    {
        const uint32_t p = 6, N = 64, half = N / 2u;
        std::unique_ptr<float[]> win(new float[1]);
        win[0] = -3.5f;
        const uint32_t B = 5;
        std::unique_ptr<uint32_t[]> first(new uint32_t[B]{0, half, 0, 0, half + 1u}), count(new uint32_t[B]{1, 1, half + 1u, 0, 0});
        const uint32_t total = half + 3u;
        std::unique_ptr<float[]> wt(new float[total]);
        for (uint32_t k = 0; k < total; ++k) wt[k] = -1.0f + (float)k;
        CHECK(!spectrum_set_error(p, win.get(), 1, 1, 0, B, first.get(), count.get(), wt.get()));
        std::vector<double> image;
        std::vector<uint32_t> desc;
        std::vector<float> weights;
        spectrum_set_image(p, B, first.get(), count.get(), wt.get(), image, desc, weights);
        CHECK(weights.size() == total && desc[4u * 2u + 2u] == 2 && desc[4u * 4u + 2u] == total);
        // no bands: the arrays are not looked at, the image holds a word of padding each
        CHECK(!spectrum_set_error(p, win.get(), 1, 7, 0, 0, nullptr, nullptr, nullptr));
        spectrum_set_image(p, 0, nullptr, nullptr, nullptr, image, desc, weights);
        CHECK(image.size() == N && desc.size() == SPECTRUM_BAND_WORDS && weights.size() == 1);
        // empty bands only: no weight is read
        std::unique_ptr<uint32_t[]> zero(new uint32_t[2]{0, 0}), at(new uint32_t[2]{0, half + 1u});
        CHECK(!spectrum_set_error(p, win.get(), 1, 1, 0, 2, at.get(), zero.get(), nullptr));

        // every refusal of a set
        std::unique_ptr<float[]> w64(new float[64]);
        for (uint32_t j = 0; j < 64; ++j) w64[j] = 1.0f;
        CHECK(says(spectrum_set_error(p, nullptr, 64, 1, 0, 0, nullptr, nullptr, nullptr), "NULL"));
        CHECK(says(spectrum_set_error(5, w64.get(), 32, 1, 0, 0, nullptr, nullptr, nullptr), "log2n"));
        CHECK(says(spectrum_set_error(13, w64.get(), 64, 1, 0, 0, nullptr, nullptr, nullptr), "log2n"));
        CHECK(says(spectrum_set_error(0xFFFFFFFFu, w64.get(), 64, 1, 0, 0, nullptr, nullptr, nullptr), "log2n"));
        CHECK(says(spectrum_set_error(p, w64.get(), 0, 1, 0, 0, nullptr, nullptr, nullptr), "n_window"));
        CHECK(says(spectrum_set_error(p, w64.get(), 65, 1, 0, 0, nullptr, nullptr, nullptr), "n_window"));
        CHECK(says(spectrum_set_error(p, w64.get(), 64, 0, 0, 0, nullptr, nullptr, nullptr), "hop is 0"));
        CHECK(says(spectrum_set_error(p, w64.get(), 64, 1, 64, 0, nullptr, nullptr, nullptr), "pad"));
        CHECK(!spectrum_set_error(p, w64.get(), 64, 0xFFFFFFFFu, 63, 0, nullptr, nullptr, nullptr));
        CHECK(says(spectrum_set_error(p, w64.get(), 64, 1, 0, 257, first.get(), count.get(), wt.get()), "above 256"));
        w64[63] = inff;
        CHECK(says(spectrum_set_error(p, w64.get(), 64, 1, 0, 0, nullptr, nullptr, nullptr), "window number"));
        CHECK(!spectrum_set_error(p, w64.get(), 63, 1, 0, 0, nullptr, nullptr, nullptr));     // (past the window: not looked at)
        w64[63] = 1.0f, w64[0] = nanf;
        CHECK(says(spectrum_set_error(p, w64.get(), 64, 1, 0, 0, nullptr, nullptr, nullptr), "window number"));
        w64[0] = 1.0f;
        CHECK(says(spectrum_set_error(p, w64.get(), 64, 1, 0, B, nullptr, count.get(), wt.get()), "without band_first"));
        CHECK(says(spectrum_set_error(p, w64.get(), 64, 1, 0, B, first.get(), nullptr, wt.get()), "without band_first"));
        CHECK(says(spectrum_set_error(p, w64.get(), 64, 1, 0, B, first.get(), count.get(), nullptr), "without band_weights"));
        first[4] = half + 2u;
        CHECK(says(spectrum_set_error(p, w64.get(), 64, 1, 0, B, first.get(), count.get(), wt.get()), "leaves the bins"));
        first[4] = 0xFFFFFFFFu, count[4] = 2;
        CHECK(says(spectrum_set_error(p, w64.get(), 64, 1, 0, B, first.get(), count.get(), wt.get()), "leaves the bins"));
        first[4] = half + 1u, count[4] = 0, count[2] = half + 2u;
        CHECK(says(spectrum_set_error(p, w64.get(), 64, 1, 0, B, first.get(), count.get(), wt.get()), "leaves the bins"));
        count[2] = half + 1u, wt[total - 1u] = inff;
        CHECK(says(spectrum_set_error(p, w64.get(), 64, 1, 0, B, first.get(), count.get(), wt.get()), "weight is not finite"));
        wt[total - 1u] = 1.0f;
        CHECK(!spectrum_set_error(p, w64.get(), 64, 1, 0, B, first.get(), count.get(), wt.get()));
        // more than 65 536 weights: 33 bands of 2000 bins at p = 12; the weights are not reached
        std::unique_ptr<uint32_t[]> f33(new uint32_t[33]), c33(new uint32_t[33]);
        std::unique_ptr<float[]> w4096(new float[4096]);
        for (uint32_t j = 0; j < 4096; ++j) w4096[j] = 0.5f;
        for (uint32_t b = 0; b < 33; ++b) f33[b] = 49, c33[b] = 2000;
        CHECK(says(spectrum_set_error(12, w4096.get(), 4096, 1, 0, 33, f33.get(), c33.get(), wt.get()), "more than 65 536"));
    }

    // the designers' refusals write nothing
    {
        std::unique_ptr<double[]> tw(new double[1]);
        tw[0] = 77.0;
        CHECK(grail_spectrum_twiddles(5, tw.get()) == GRAIL_ERR_INVALID_ARG && grail_spectrum_twiddles(13, tw.get()) == GRAIL_ERR_INVALID_ARG);
        CHECK(grail_spectrum_twiddles(6, nullptr) == GRAIL_ERR_INVALID_ARG && tw[0] == 77.0);
        uint64_t frames = 77;
        CHECK(grail_spectrum_frames(1, 0, &frames) == GRAIL_ERR_INVALID_ARG && frames == 77 && grail_spectrum_frames(1, 1, nullptr) == GRAIL_ERR_INVALID_ARG);
        CHECK(grail_spectrum_frames(0, 5, &frames) == GRAIL_OK && frames == 0);
        CHECK(grail_spectrum_frames(UINT64_MAX, 1, &frames) == GRAIL_OK && frames == UINT64_MAX);
        CHECK(grail_spectrum_frames(UINT64_MAX, 0xFFFFFFFFu, &frames) == GRAIL_OK && frames == 0x100000001ull);
        CHECK(grail_spectrum_frames(UINT64_MAX - 1u, 0xFFFFFFFFu, &frames) == GRAIL_OK && frames == 0x100000001ull);
        CHECK(grail_spectrum_frames(11, 5, &frames) == GRAIL_OK && frames == 3 && grail_spectrum_frames(10, 5, &frames) == GRAIL_OK && frames == 2);
        std::unique_ptr<float[]> w(new float[1]);
        w[0] = 77.0f;
        CHECK(grail_spectrum_window(3, 1, w.get()) == GRAIL_ERR_INVALID_ARG && grail_spectrum_window(-1, 1, w.get()) == GRAIL_ERR_INVALID_ARG);
        CHECK(grail_spectrum_window(1, 0, w.get()) == GRAIL_ERR_INVALID_ARG && grail_spectrum_window(1, 4097, w.get()) == GRAIL_ERR_INVALID_ARG);
        CHECK(grail_spectrum_window(1, 1, nullptr) == GRAIL_ERR_INVALID_ARG && w[0] == 77.0f);
        std::unique_ptr<uint32_t[]> first(new uint32_t[1]{77}), count(new uint32_t[1]{77});
        std::unique_ptr<float[]> wt(new float[1]{77.0f});
        uint32_t total = 77;
        CHECK(grail_mel_design(0, 6, 1, 0.0, 100.0, first.get(), count.get(), wt.get(), 1, &total) == GRAIL_ERR_INVALID_ARG);
        CHECK(grail_mel_design(8000, 5, 1, 0.0, 100.0, first.get(), count.get(), wt.get(), 1, &total) == GRAIL_ERR_INVALID_ARG);
        CHECK(grail_mel_design(8000, 13, 1, 0.0, 100.0, first.get(), count.get(), wt.get(), 1, &total) == GRAIL_ERR_INVALID_ARG);
        CHECK(grail_mel_design(8000, 6, 0, 0.0, 100.0, first.get(), count.get(), wt.get(), 1, &total) == GRAIL_ERR_INVALID_ARG);
        CHECK(grail_mel_design(8000, 6, 257, 0.0, 100.0, first.get(), count.get(), wt.get(), 1, &total) == GRAIL_ERR_INVALID_ARG);
        for (double lo : {-1.0, nan, 100.0, 200.0, inf})
            CHECK(grail_mel_design(8000, 6, 1, lo, 100.0, first.get(), count.get(), wt.get(), 1, &total) == GRAIL_ERR_INVALID_ARG);
        for (double hi : {nan, inf, 4000.5})
            CHECK(grail_mel_design(8000, 6, 1, 0.0, hi, first.get(), count.get(), wt.get(), 1, &total) == GRAIL_ERR_INVALID_ARG);
        CHECK(grail_mel_design(8000, 6, 1, 1000.0, 1000.0 + 1e-13, first.get(), count.get(), wt.get(), 1, &total) == GRAIL_ERR_INVALID_ARG);
        CHECK(grail_mel_design(8000, 6, 1, 0.0, 100.0, nullptr, count.get(), wt.get(), 1, &total) == GRAIL_ERR_INVALID_ARG);
        CHECK(grail_mel_design(8000, 6, 1, 0.0, 100.0, first.get(), nullptr, wt.get(), 1, &total) == GRAIL_ERR_INVALID_ARG);
        CHECK(grail_mel_design(8000, 6, 1, 0.0, 100.0, first.get(), count.get(), nullptr, 1, &total) == GRAIL_ERR_INVALID_ARG);
        CHECK(grail_mel_design(8000, 6, 1, 0.0, 100.0, first.get(), count.get(), wt.get(), 1, nullptr) == GRAIL_ERR_INVALID_ARG);
        CHECK(first[0] == 77 && count[0] == 77 && wt[0] == 77.0f && total == 77);
        // a band that catches no bin: bins lie 125 Hz apart, the triangle between 0 and 100 Hz has its feet on none but bin 0's
        CHECK(grail_mel_design(8000, 6, 1, 0.0, 100.0, first.get(), count.get(), nullptr, 0, &total) == GRAIL_OK);
        CHECK(first[0] == 0 && count[0] == 0 && total == 0);
    }

    // the call: the grid, and every refusal.  Addresses are compared, never looked behind.
    {
        const char *rows = (const char *)0x10000000, *out = (const char *)0x20000000, *len = (const char *)0x40000000;
        SpectrumFacts set;
        set.log2n = 6, set.n_window = 64, set.hop = 16, set.pad = 0, set.n_bands = 3;
        SpectrumFacts bare = set;
        bare.n_bands = 0;
        CHECK(spectrum_frames_max(0, 16) == 0 && spectrum_frames_max(1, 16) == 1 && spectrum_frames_max(16, 16) == 1 && spectrum_frames_max(17, 16) == 2);
        CHECK(spectrum_frames_max(UINT64_MAX, 1) == 0xFFFFFFFFull && spectrum_frames_max(UINT64_MAX, 0xFFFFFFFFu) == 1);
        CHECK(spectrum_grid_chunks(0, 16) == 0 && spectrum_grid_chunks(128, 16) == 1 && spectrum_grid_chunks(129, 16) == 2);
        CHECK(spectrum_grid_chunks(UINT64_MAX, 1) == 0x20000000ull);
        CHECK(!spectrum_call_error(&set, rows, 64, len, 2, out, nullptr, 4));
        CHECK(!spectrum_call_error(&set, rows, 64, len, 2, nullptr, out, 4));
        CHECK(!spectrum_call_error(&set, rows, 64, len, 2, out, out + 0x1000000, 4));
        CHECK(!spectrum_call_error(&set, nullptr, 0, len, 2, out, nullptr, 0));           // rows of no samples
        CHECK(!spectrum_call_error(&set, nullptr, 0, nullptr, 0, out, nullptr, 0));       // no rows
        CHECK(!spectrum_call_error(nullptr, rows, 64, len, 2, out, nullptr, 0));          // no context: the set's facts are not read
        CHECK(says(spectrum_call_error(&set, rows, 64, len, 2, nullptr, nullptr, 4), "both NULL"));
        CHECK(says(spectrum_call_error(nullptr, rows, 64, len, 0, nullptr, nullptr, 4), "both NULL"));
        CHECK(says(spectrum_call_error(&bare, rows, 64, len, 2, out, out + 0x1000000, 4), "set of no bands"));
        CHECK(!spectrum_call_error(&bare, rows, 64, len, 2, out, nullptr, 4));
        CHECK(says(spectrum_call_error(&set, rows, 64, len, 2, out, nullptr, 3), "frames_stride"));
        CHECK(says(spectrum_call_error(&set, rows, 65, len, 2, out, nullptr, 4), "frames_stride"));
        CHECK(says(spectrum_call_error(&set, rows, 64, len, 0, out, nullptr, 3), "frames_stride"));   // (also without rows)
        CHECK(says(spectrum_call_error(&set, rows, UINT64_MAX, len, 1, out, nullptr, UINT64_MAX / 16u), "frames_stride"));
        CHECK(says(spectrum_call_error(&set, rows, 64, nullptr, 2, out, nullptr, 4), "NULL buffer"));
        CHECK(says(spectrum_call_error(&set, nullptr, 64, len, 2, out, nullptr, 4), "NULL buffer"));
        CHECK(says(spectrum_call_error(&set, rows, 1ull << 59, len, 4, out, nullptr, 1ull << 55), "2^60 samples"));
        CHECK(says(spectrum_call_error(&set, rows, 64, len, 4, out, nullptr, 1ull << 59), "2^60 numbers"));
        CHECK(says(spectrum_call_error(&set, rows, 64, len, 4, out, nullptr, 1ull << 54), "2^60 numbers"));      // (33 bins a frame)
        CHECK(says(spectrum_call_error(&set, rows, 64, len, 4, nullptr, out, 1ull << 57), "2^60 numbers"));      // (3 bands a frame)
        CHECK(!spectrum_call_error(&set, rows, 64, len, 4, nullptr, (const char *)(1ull << 62), 1ull << 56));
        // overlaps: the outputs' first and last word against the rows' last and first
        CHECK(says(spectrum_call_error(&set, rows, 64, len, 2, rows + 4 * 127, nullptr, 4), "power_dev overlaps"));
        CHECK(!spectrum_call_error(&set, rows, 64, len, 2, rows + 4 * 128, nullptr, 4));
        CHECK(says(spectrum_call_error(&set, rows, 64, len, 2, rows - 4 * (2 * 4 * 33) + 4, nullptr, 4), "power_dev overlaps"));
        CHECK(!spectrum_call_error(&set, rows, 64, len, 2, rows - 4 * (2 * 4 * 33), nullptr, 4));
        CHECK(says(spectrum_call_error(&set, rows, 64, len, 2, out, rows + 4 * 127, 4), "bands_dev overlaps"));
        CHECK(says(spectrum_call_error(&set, rows, 64, len, 2, out, rows - 4 * (2 * 4 * 3) + 4, 4), "bands_dev overlaps"));
        CHECK(!spectrum_call_error(&set, rows, 64, len, 2, out, rows - 4 * (2 * 4 * 3), 4));
        // the grid: 2^31 - 1 workgroups pass, one more does not
        SpectrumFacts fine = set;
        fine.hop = 1;
        CHECK(!spectrum_call_error(&fine, rows, 8, len, 0x7FFFFFFFu, (const char *)(1ull << 62), nullptr, 8));
        CHECK(says(spectrum_call_error(&fine, rows, 9, len, 0x7FFFFFFFu, (const char *)(1ull << 62), nullptr, 9), "2^31 - 1 workgroups"));
        CHECK(says(spectrum_call_error(&fine, rows, 8, len, 0x80000000u, (const char *)(1ull << 62), nullptr, 8), "2^31 - 1 workgroups"));
    }

    std::printf("sanitize spectrum driver: ok\n");
    return 0;
}
