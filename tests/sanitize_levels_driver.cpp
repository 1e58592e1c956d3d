// sanitize_levels_driver.cpp — drives csrc/level_gains.cpp under AddressSanitizer + UBSan (tests/test_levels_host.py):
// grail_level_gains in its three modes over arrays of exactly the documented sizes (an overread is ASan's to find), NULL
// arrays a mode does not need, rows that cannot be leveled, invalid arguments with the outputs untouched; and
// grail_active_level over rows whose last frame is short, silent rows and an empty row.
#include <cmath>
#include <cstdio>
#include <random>
#include <vector>

#include "../include/grail_hip.h"

static int failures = 0;
#define CHECK(c)                                                            \
    do {                                                                    \
        if (!(c)) {                                                         \
            std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c);         \
            ++failures;                                                     \
            return;                                                         \
        }                                                                   \
    } while (0)

static void gains_case(std::mt19937 &rng, uint32_t n_rows, uint32_t n_items)
{
    std::uniform_real_distribution<double> mag(1e-6, 4.0);
    std::uniform_real_distribution<float> db(-60.0f, 12.0f);
    std::vector<double> sumsq(n_rows), active(n_rows);
    std::vector<float> peak(n_rows);
    std::vector<uint32_t> bad(n_rows, 0u), len(n_rows);
    for (uint32_t r = 0; r < n_rows; ++r) {
        len[r] = 1u + rng() % 100000u;
        peak[r] = (float)mag(rng);
        sumsq[r] = mag(rng) * len[r];
        active[r] = mag(rng);
    }
    uint32_t expect_out = 0;
    if (n_rows >= 3) {
        len[0] = 0, sumsq[0] = 0.0, peak[0] = 0.0f, active[0] = 0.0;      // an empty row
        bad[1] = 3;                                                        // a row with non-finite samples
        sumsq[2] = 0.0, peak[2] = 0.0f, active[2] = 0.0;                   // a silent row
    }
    std::vector<uint32_t> rows(n_items);
    std::vector<float> level(n_items);
    for (uint32_t i = 0; i < n_items; ++i) {
        rows[i] = rng() % n_rows;
        level[i] = db(rng);
        if (n_rows >= 3 && rows[i] < 3) ++expect_out;
    }
    for (int mode = GRAIL_LEVEL_PEAK; mode <= GRAIL_LEVEL_ACTIVE; ++mode) {
        std::vector<float> g(n_items, -1.0f);
        uint32_t out = 0xFFFFFFFFu;
        // only what the mode needs is passed
        const int rc = grail_level_gains(mode, mode == GRAIL_LEVEL_RMS ? sumsq.data() : nullptr,
                                         mode == GRAIL_LEVEL_PEAK ? peak.data() : nullptr, bad.data(),
                                         mode == GRAIL_LEVEL_RMS ? len.data() : nullptr,
                                         mode == GRAIL_LEVEL_ACTIVE ? active.data() : nullptr, n_rows, rows.data(),
                                         level.data(), n_items, g.data(), &out);
        CHECK(rc == GRAIL_OK);
        CHECK(out == expect_out);
        for (uint32_t i = 0; i < n_items; ++i) {
            const uint32_t r = rows[i];
            const double lv = mode == GRAIL_LEVEL_PEAK ? (double)peak[r]
                              : mode == GRAIL_LEVEL_RMS ? (len[r] ? std::sqrt(sumsq[r] / len[r]) : 0.0) : active[r];
            if (n_rows >= 3 && r < 3) CHECK(g[i] == 0.0f);
            else CHECK(g[i] == (float)(std::pow(10.0, (double)level[i] / 20.0) / lv));
        }
        // an item past n_rows: refused, nothing written; so are a missing array and an unknown mode
        if (n_items) {
            std::vector<float> h(n_items, -1.0f);
            uint32_t keep = 77u;
            std::vector<uint32_t> wrong = rows;
            wrong[n_items - 1] = n_rows;
            CHECK(grail_level_gains(mode, sumsq.data(), peak.data(), bad.data(), len.data(), active.data(), n_rows,
                                    wrong.data(), level.data(), n_items, h.data(), &keep) == GRAIL_ERR_INVALID_ARG);
            CHECK(grail_level_gains(mode, nullptr, nullptr, bad.data(), nullptr, nullptr, n_rows, rows.data(), level.data(),
                                    n_items, h.data(), &keep) == GRAIL_ERR_INVALID_ARG);
            CHECK(grail_level_gains(3, sumsq.data(), peak.data(), bad.data(), len.data(), active.data(), n_rows, rows.data(),
                                    level.data(), n_items, h.data(), &keep) == GRAIL_ERR_INVALID_ARG);
            for (const float v : h) CHECK(v == -1.0f);
            CHECK(keep == 77u);
        }
        // nonfinite and n_unleveled may be NULL
        CHECK(grail_level_gains(mode, sumsq.data(), peak.data(), nullptr, len.data(), active.data(), n_rows, rows.data(),
                                level.data(), n_items, g.data(), nullptr) == GRAIL_OK);
    }
}

static void active_case(std::mt19937 &rng, uint32_t row_len, uint32_t frame)
{
    const uint32_t frames = row_len / frame + (row_len % frame != 0);
    std::vector<double> fs(frames);              // exactly ceil(row_len / frame) entries
    std::uniform_real_distribution<double> u(0.0, 1.0);
    double all = 0.0;
    for (uint32_t f = 0; f < frames; ++f) {
        const uint32_t count = f + 1 < frames ? frame : row_len - f * frame;
        fs[f] = u(rng) < 0.3 ? 0.0 : u(rng) * count;
        all += fs[f];
    }
    const double lv = grail_active_level(fs.data(), row_len, frame, 40.0f);
    CHECK(std::isfinite(lv) && lv >= 0.0);
    if (row_len) CHECK(lv + 1e-12 >= std::sqrt(all / row_len));       // leaving quiet frames out never lowers the level
    if (all == 0.0) CHECK(lv == 0.0);
    // a floor of 400 dB keeps every frame that is not silent: the whole-row RMS over the non-silent frames' samples
    const double wide = grail_active_level(fs.data(), row_len, frame, 400.0f);
    CHECK(wide <= lv + 1e-12 || all == 0.0);
    std::fill(fs.begin(), fs.end(), 0.0);
    CHECK(grail_active_level(fs.data(), row_len, frame, 40.0f) == 0.0);
}

int main()
{
    std::mt19937 rng(20240607u);
    for (int k = 0; k < 200; ++k) gains_case(rng, 1u + rng() % 50u, rng() % 200u);
    gains_case(rng, 3, 0);
    gains_case(rng, 1, 1);
    for (int k = 0; k < 300; ++k) active_case(rng, rng() % 300000u, 256u + rng() % 8000u);
    for (const uint32_t n : {0u, 1u, 255u, 256u, 257u, 4095u, 4096u, 4097u, 96006u}) active_case(rng, n, 4096u);
    active_case(rng, 0xFFFFFFFFu, 1048576u);
    if (grail_active_level(nullptr, 10, 256, 40.0f) != 0.0) ++failures;
    if (failures) {
        std::printf("sanitize levels driver: %d failures\n", failures);
        return 1;
    }
    std::printf("sanitize levels driver: ok\n");
    return 0;
}
