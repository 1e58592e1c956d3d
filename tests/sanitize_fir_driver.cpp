// Drives the pure-host FIR functions of csrc/fir_plan.cpp under AddressSanitizer and UBSan (tests/test_fir_sanitize.py
// builds and runs it): every array lives on the heap at exactly the size the call is entitled to, so that a read or write
// one element past it is caught.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <memory>
#include <vector>

#include "../include/grail_hip.h"
#include "../grail-rs_amd/csrc/fir_plan.h"

#define CHECK(cond)                                                                  \
    do {                                                                             \
        if (!(cond)) {                                                               \
            std::fprintf(stderr, "sanitize fir driver: %s failed (line %d)\n", #cond, __LINE__); \
            return 1;                                                                \
        }                                                                            \
    } while (0)

int main()
{
    // designs into exactly K floats: even about the middle, finite, the middle tap the band's width
    const struct {
        uint32_t rate;
        double lo, hi;
        uint32_t K;
    } designs[] = {{8000, 300.0, 3400.0, 255}, {48000, 300.0, 3400.0, 1023}, {48000, 0.0, 8000.0, 255}, {48000, 100.0, 24000.0, 1023},
                   {8000, 0.0, 4000.0, 3}, {44100, 20.0, 22050.0, 4095}};
    for (const auto &d : designs) {
        std::unique_ptr<float[]> h(new float[d.K]);
        CHECK(grail_fir_design(d.rate, d.lo, d.hi, d.K, h.get()) == GRAIL_OK);
        for (uint32_t k = 0; k < d.K; ++k) CHECK(std::isfinite(h[k]) && h[k] == h[d.K - 1 - k]);
        CHECK(std::fabs((double)h[d.K / 2] - 2.0 * (d.hi - d.lo) / d.rate) <= 1e-6);
    }
    float one = 77.0f;
    const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
    CHECK(grail_fir_design(0, 0.0, 1.0, 255, &one) == GRAIL_ERR_INVALID_ARG);
    for (uint32_t K : {0u, 1u, 2u, 254u, 4096u, 4097u, 0xFFFFFFFFu}) CHECK(grail_fir_design(8000, 300.0, 3400.0, K, &one) == GRAIL_ERR_INVALID_ARG);
    const double bands[][2] = {{-1.0, 3400.0}, {3400.0, 3400.0}, {3400.0, 300.0}, {300.0, 4000.5}, {nan, 3400.0}, {300.0, nan}, {300.0, inf}, {-inf, 300.0}};
    for (const auto &b : bands) CHECK(grail_fir_design(8000, b[0], b[1], 255, &one) == GRAIL_ERR_INVALID_ARG);
    CHECK(grail_fir_design(8000, 300.0, 3400.0, 255, nullptr) == GRAIL_ERR_INVALID_ARG && one == 77.0f);

    // lengths
    uint64_t n_out = 77;
    CHECK(grail_fir_len(0, 9, 4, &n_out) == GRAIL_OK && n_out == 0);
    CHECK(grail_fir_len(100, 9, 4, &n_out) == GRAIL_OK && n_out == 104);
    CHECK(grail_fir_len(UINT64_MAX - 4095, 4096, 0, &n_out) == GRAIL_OK && n_out == UINT64_MAX);
    n_out = 77;
    CHECK(grail_fir_len(UINT64_MAX - 4094, 4096, 0, &n_out) == GRAIL_ERR_INVALID_ARG && n_out == 77);
    CHECK(grail_fir_len(5, 0, 0, &n_out) == GRAIL_ERR_INVALID_ARG && grail_fir_len(5, 4097, 0, &n_out) == GRAIL_ERR_INVALID_ARG);
    CHECK(grail_fir_len(5, 9, 9, &n_out) == GRAIL_ERR_INVALID_ARG && grail_fir_len(5, 9, 4, nullptr) == GRAIL_ERR_INVALID_ARG && n_out == 77);

    // set images: the taps of every filter as binary64, padded with +0.0 to a multiple of 8, one after another
    const uint32_t Ks[] = {1, 7, 8, 9, 4096};
    uint32_t total = 0;
    for (uint32_t K : Ks) total += K;
    std::unique_ptr<float[]> taps(new float[total]);
    std::unique_ptr<uint32_t[]> n_taps(new uint32_t[5]), origin(new uint32_t[5]);
    for (uint32_t i = 0; i < total; ++i) taps[i] = (float)(i % 13) - 6.5f;
    for (uint32_t f = 0; f < 5; ++f) n_taps[f] = Ks[f], origin[f] = f % 2 ? Ks[f] - 1 : 0;
    for (uint32_t first = 0; first < 5; ++first) {          // the set of filters first .. 4, and each filter alone
        for (uint32_t count : {5u - first, 1u}) {
            const float *t = taps.get();
            for (uint32_t f = 0; f < first; ++f) t += Ks[f];
            CHECK(grail::fir_set_error(t, n_taps.get() + first, origin.get() + first, count) == nullptr);
            std::vector<double> image;
            std::vector<uint32_t> desc;
            uint32_t tail = 77;
            grail::fir_set_image(t, n_taps.get() + first, origin.get() + first, count, image, desc, &tail);
            CHECK(desc.size() == (size_t)count * grail::FIR_DESC_WORDS);
            size_t at = 0, from = 0;
            uint32_t want_tail = 0;
            for (uint32_t f = 0; f < count; ++f) {
                const uint32_t K = Ks[first + f], padded = (K + 7u) / 8u * 8u;
                const uint32_t *d = &desc[(size_t)f * grail::FIR_DESC_WORDS];
                CHECK(d[0] == at && d[1] == padded && d[2] == K && d[3] == origin[first + f]);
                for (uint32_t k = 0; k < padded; ++k)
                    CHECK(k < K ? image[at + k] == (double)t[from + k] : (image[at + k] == 0.0 && !std::signbit(image[at + k])));
                want_tail = K - 1 - origin[first + f] > want_tail ? K - 1 - origin[first + f] : want_tail;
                at += padded, from += K;
            }
            CHECK(image.size() == at && tail == want_tail);
        }
    }
    // 64 filters of 4096 taps: the largest image
    {
        std::unique_ptr<float[]> big(new float[64 * 4096]);
        std::unique_ptr<uint32_t[]> ks(new uint32_t[64]), os(new uint32_t[64]);
        for (uint32_t i = 0; i < 64 * 4096; ++i) big[i] = 1.0f;
        for (uint32_t f = 0; f < 64; ++f) ks[f] = 4096, os[f] = 4095;
        CHECK(grail::fir_set_error(big.get(), ks.get(), os.get(), 64) == nullptr);
        std::vector<double> image;
        std::vector<uint32_t> desc;
        uint32_t tail = 77;
        grail::fir_set_image(big.get(), ks.get(), os.get(), 64, image, desc, &tail);
        CHECK(image.size() == 64u * 4096u && tail == 0 && desc[63 * 4] == 63u * 4096u);
        // every refused set; a tap that is not finite anywhere in it, and past it (not looked at: the array ends there)
        CHECK(grail::fir_set_error(big.get(), ks.get(), os.get(), 65) != nullptr && grail::fir_set_error(big.get(), ks.get(), os.get(), 0) != nullptr);
        CHECK(grail::fir_set_error(nullptr, ks.get(), os.get(), 1) != nullptr && grail::fir_set_error(big.get(), nullptr, os.get(), 1) != nullptr);
        CHECK(grail::fir_set_error(big.get(), ks.get(), nullptr, 1) != nullptr);
        big[64 * 4096 - 1] = std::numeric_limits<float>::infinity();
        CHECK(grail::fir_set_error(big.get(), ks.get(), os.get(), 64) != nullptr && grail::fir_set_error(big.get(), ks.get(), os.get(), 63) == nullptr);
        big[64 * 4096 - 1] = 1.0f, big[0] = std::numeric_limits<float>::quiet_NaN();
        CHECK(grail::fir_set_error(big.get(), ks.get(), os.get(), 1) != nullptr);
        big[0] = 1.0f;
        ks[1] = 0;
        CHECK(grail::fir_set_error(big.get(), ks.get(), os.get(), 2) != nullptr && grail::fir_set_error(big.get(), ks.get(), os.get(), 1) == nullptr);
        ks[1] = 4097;
        CHECK(grail::fir_set_error(big.get(), ks.get(), os.get(), 2) != nullptr);
        ks[1] = 4096, os[1] = 4096;
        CHECK(grail::fir_set_error(big.get(), ks.get(), os.get(), 2) != nullptr);
        os[1] = 0xFFFFFFFFu;
        CHECK(grail::fir_set_error(big.get(), ks.get(), os.get(), 2) != nullptr);
    }
    std::printf("sanitize fir driver: ok\n");
    return 0;
}
