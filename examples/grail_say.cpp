// grail_say — the shape of the reference's examples/cli.rs (text in, WAV out, timing line),
// with the synthesis on an MI355X through include/grail.hpp.   usage: grail_say [-o out.wav] [--mel out.f32] text...
// --mel FILE: after the WAV, the utterance's mel energies as raw binary32, frames x 80 bands: frames of 1 024 samples under a
// periodic Hann window every 256, the first centred on sample 0, HTK triangles from 0 Hz to half the rate
// (grail_spectrum_async through the C ABI: the facade has no class for it yet).  No logarithm is taken: that is the reader's.
#include <chrono>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "grail.hpp"

namespace {

constexpr uint32_t MEL_LOG2N = 10, MEL_HOP = 256, MEL_BANDS = 80;

// the frames x MEL_BANDS energies of one utterance, computed where a batch's rows would lie: on the device
std::vector<float> mel_energies(grail_ctx *ctx, const std::vector<float> &pcm, uint32_t rate, uint64_t *n_frames)
{
    const uint32_t N = 1u << MEL_LOG2N, n = (uint32_t)pcm.size();
    std::vector<float> window(N);
    grail::check(grail_spectrum_window(GRAIL_SPECTRUM_HANN, N, window.data()));
    std::vector<uint32_t> first(MEL_BANDS), count(MEL_BANDS);
    uint32_t total = 0;
    const int sized = grail_mel_design(rate, MEL_LOG2N, MEL_BANDS, 0.0, rate / 2.0, first.data(), count.data(), nullptr, 0, &total);
    if (sized != GRAIL_ERR_BUFFER_TOO_SMALL) grail::check(sized);
    std::vector<float> weights(total ? total : 1u);
    grail::check(grail_mel_design(rate, MEL_LOG2N, MEL_BANDS, 0.0, rate / 2.0, first.data(), count.data(), weights.data(), total, &total));
    grail::check(grail_spectrum_frames(n, MEL_HOP, n_frames));
    std::vector<float> bands((size_t)*n_frames * MEL_BANDS);
    grail_spectrum *set = nullptr;
    grail::check(grail_spectrum_create(ctx, MEL_LOG2N, window.data(), N, MEL_HOP, N / 2u, MEL_BANDS, first.data(), count.data(),
                                       weights.data(), &set));
    void *d_rows = nullptr, *d_len = nullptr, *d_bands = nullptr;
    int rc = grail_device_alloc(ctx, (size_t)(n ? n : 1u) * 4, &d_rows);
    if (!rc) rc = grail_device_alloc(ctx, 4, &d_len);
    if (!rc) rc = grail_device_alloc(ctx, bands.size() * 4 + 4, &d_bands);
    if (!rc && n) rc = grail_memcpy_h2d(ctx, d_rows, pcm.data(), (size_t)n * 4);
    if (!rc) rc = grail_memcpy_h2d(ctx, d_len, &n, 4);
    if (!rc) rc = grail_spectrum_async(ctx, set, (const float *)d_rows, n, (const uint32_t *)d_len, 1, nullptr, (float *)d_bands, *n_frames,
                                       nullptr, nullptr);
    if (!rc) rc = grail_sync(ctx);
    if (!rc && !bands.empty()) rc = grail_memcpy_d2h(ctx, bands.data(), d_bands, bands.size() * 4);
    for (void *p : {d_rows, d_len, d_bands})
        if (p) grail_device_free(ctx, p);
    const int freed = grail_spectrum_free(ctx, set);
    grail::check(rc ? rc : freed);
    return bands;
}

}  // namespace

int main(int argc, char **argv)
{
    std::string out_path, mel_path, text;
    for (int i = 1; i < argc; ++i) {
        if ((!std::strcmp(argv[i], "-o") || !std::strcmp(argv[i], "--output")) && i + 1 < argc) out_path = argv[++i];
        else if (!std::strcmp(argv[i], "--mel") && i + 1 < argc) mel_path = argv[++i];
        else text += (text.empty() ? "" : " ") + std::string(argv[i]);
    }
    if (text.empty()) {
        std::fprintf(stderr, "usage: grail_say [-o out.wav] [--mel out.f32] text...\n");
        return 2;
    }
    try {
        const grail::Voice voice = grail::voices::generic();       // 44.1 kHz, as the CLI
        grail::Gpu gpu(0, {voice});
        const auto t0 = std::chrono::steady_clock::now();
        const auto pcm = gpu.say({text});                           // cli.rs:175-184
        const auto us = std::chrono::duration_cast<std::chrono::microseconds>(
                            std::chrono::steady_clock::now() - t0).count();
        std::printf("\"%s\"\n%.2f seconds of audio, generated in %lld microseconds\n", text.c_str(),
                    pcm[0].size() / voice.sample_rate, (long long)us);   // cli.rs:189-193
        if (!out_path.empty()) {
            std::printf("Writing generated sound to %s\n", out_path.c_str());
            gpu.save_wav(out_path, pcm[0], (uint32_t)voice.sample_rate);
        }
        if (!mel_path.empty()) {
            uint64_t n_frames = 0;
            const std::vector<float> bands = mel_energies(gpu.ctx(), pcm[0], (uint32_t)voice.sample_rate, &n_frames);
            std::printf("Writing %llu frames x %u mel energies (binary32) to %s\n", (unsigned long long)n_frames, MEL_BANDS, mel_path.c_str());
            std::FILE *f = std::fopen(mel_path.c_str(), "wb");
            if (!f || (!bands.empty() && std::fwrite(bands.data(), 4, bands.size(), f) != bands.size()) || std::fclose(f)) {
                std::fprintf(stderr, "grail_say: cannot write %s\n", mel_path.c_str());
                return 1;
            }
        }
    } catch (const grail::Error &e) {
        std::fprintf(stderr, "grail_say: %s (status %d)\n", e.what(), e.status);
        return 1;
    }
    return 0;
}
