// sanitize_mix_driver.cpp — drives csrc/mix_plan.cpp under AddressSanitizer + UBSan (tests/test_mix_host.py): random mixes
// with items across and wholly past track_len, zero-length rows, ten thousand items stacked on one track, long mixes that
// take 8 samples per lane, and the invariants of what comes back — every (item, list tile) intersection listed exactly
// once, every list in accumulation order, nothing wholly past track_len, the geometry the kernel relies on.
#include <algorithm>
#include <cstdio>
#include <random>
#include <string>
#include <vector>

#include "../grail-rs_amd/csrc/mix_plan.h"
#include "../include/grail_hip.h"

using grail::mix::MixItem;
using grail::mix::Plan;

static int failures = 0;
#define CHECK(c)                                                            \
    do {                                                                    \
        if (!(c)) {                                                         \
            std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c);         \
            ++failures;                                                     \
            return;                                                         \
        }                                                                   \
    } while (0)

struct Case {
    std::vector<uint32_t> row_len, rows, tracks;
    std::vector<uint64_t> offs;
    std::vector<float> gains;
    uint64_t row_stride = 0, track_len = 0, track_stride = 0;
    uint32_t n_tracks = 1, cus = 256;
    bool null_tracks = false;
};

static void check_case(const Case &c)
{
    Plan p;
    std::string why;
    const uint32_t n_rows = (uint32_t)c.row_len.size(), n = (uint32_t)c.rows.size();
    const int rc = grail::mix::build_plan(c.row_len.data(), n_rows, c.row_stride, c.rows.data(),
                                          c.null_tracks ? nullptr : c.tracks.data(), c.offs.data(), c.gains.data(), n,
                                          c.n_tracks, c.track_len, c.track_stride, c.cus, p, &why);
    CHECK(rc == GRAIL_OK);
    // geometry
    CHECK(p.samples_per_lane == 1 || p.samples_per_lane == 8);
    CHECK(p.wg_samples % (256u * p.samples_per_lane) == 0 && p.tile_samples % p.wg_samples == 0);
    CHECK(p.wgs_per_track == (c.track_len + p.wg_samples - 1) / p.wg_samples);
    CHECK(p.tiles_per_track == (c.track_len + p.tile_samples - 1) / p.tile_samples);
    CHECK((double)c.n_tracks * (double)p.wgs_per_track <= 4194304.0);
    const size_t n_tiles = (size_t)c.n_tracks * p.tiles_per_track;
    CHECK(p.tile_start.size() == n_tiles + 1 && p.tile_start[0] == 0 && p.tile_start[n_tiles] == p.tile_items.size());
    for (size_t k = 0; k < n_tiles; ++k) CHECK(p.tile_start[k] <= p.tile_start[k + 1]);
    // the items that cover something, in accumulation order (ascending row, ties as given), described right
    std::vector<uint32_t> want;
    for (uint32_t i = 0; i < n; ++i)
        if (c.row_len[c.rows[i]] > 0 && c.offs[i] < c.track_len) want.push_back(i);
    std::stable_sort(want.begin(), want.end(), [&](uint32_t a, uint32_t b) { return c.rows[a] < c.rows[b]; });
    CHECK(p.items.size() == want.size());
    uint64_t covered = 0;
    for (size_t k = 0; k < want.size(); ++k) {
        const MixItem &m = p.items[k];
        const uint32_t i = want[k];
        CHECK(m.item == i);
        CHECK(m.lo == c.offs[i] && m.lo < m.hi && m.hi <= c.track_len);      // nothing wholly past track_len
        CHECK(m.hi == std::min<uint64_t>(c.track_len, c.offs[i] + c.row_len[c.rows[i]]));
        CHECK((uint64_t)m.base + m.lo == (uint64_t)c.rows[i] * c.row_stride);
        CHECK(m.gain == c.gains[i]);
        covered += m.hi - m.lo;
    }
    CHECK(covered == p.covered);
    // every list: on its track, in accumulation order, each entry intersects the tile; every intersection listed once
    std::vector<uint64_t> listed(p.items.size(), 0);
    for (uint32_t t = 0; t < c.n_tracks; ++t) {
        for (uint64_t tl = 0; tl < p.tiles_per_track; ++tl) {
            const size_t k = (size_t)t * p.tiles_per_track + tl;
            const uint64_t lo = tl * p.tile_samples, hi = std::min(c.track_len, lo + p.tile_samples);
            for (uint32_t e = p.tile_start[k]; e < p.tile_start[k + 1]; ++e) {
                const uint32_t it = p.tile_items[e];
                CHECK(it < p.items.size());
                CHECK(e == p.tile_start[k] || p.tile_items[e - 1] < it);                 // accumulation order, no repeat
                CHECK((c.null_tracks ? 0u : c.tracks[p.items[it].item]) == t);
                CHECK(p.items[it].lo < hi && p.items[it].hi > lo);
                ++listed[it];
            }
        }
    }
    for (size_t k = 0; k < p.items.size(); ++k) {
        const MixItem &m = p.items[k];
        uint64_t tiles = 0;
        for (uint64_t tl = 0; tl < p.tiles_per_track; ++tl)
            tiles += m.lo < std::min(c.track_len, (tl + 1) * p.tile_samples) && m.hi > tl * p.tile_samples;
        CHECK(listed[k] == tiles);
    }
}

static Case random_case(std::mt19937_64 &rng, bool stacked, bool lng)
{
    auto uni = [&rng](uint64_t lo, uint64_t hi) { return std::uniform_int_distribution<uint64_t>(lo, hi)(rng); };
    Case c;
    const uint32_t n_rows = (uint32_t)uni(1, stacked ? 400 : 120);
    for (uint32_t r = 0; r < n_rows; ++r) c.row_len.push_back(uni(0, 7) == 0 ? 0u : (uint32_t)uni(1, 5000));
    c.row_stride = *std::max_element(c.row_len.begin(), c.row_len.end()) + uni(0, 70);
    c.n_tracks = stacked ? 1u : (uint32_t)uni(1, lng ? 64 : 12);
    c.track_len = lng ? uni(200000, 1200000) : stacked ? uni(1000, 7000) : uni(0, 40000);
    c.track_stride = c.track_len + uni(0, 100);
    c.cus = (uint32_t[]){1, 4, 32, 256}[uni(0, 3)];
    c.null_tracks = !stacked && uni(0, 4) == 0;
    const uint32_t n = stacked ? 10000u : (uint32_t)uni(0, lng ? 400 : 1500);
    for (uint32_t i = 0; i < n; ++i) {
        c.rows.push_back((uint32_t)uni(0, n_rows - 1));
        c.tracks.push_back(c.null_tracks ? 0u : (uint32_t)uni(0, c.n_tracks - 1));
        uint64_t off;
        switch (stacked ? 0 : uni(0, 5)) {
        case 0: off = uni(0, stacked ? 1000 : (c.track_len ? c.track_len - 1 : 0)); break;
        case 1: off = c.track_len + uni(0, 3000); break;                         // wholly past track_len
        case 2: off = c.track_len > 3000 ? c.track_len - uni(1, 3000) : 0; break;  // across track_len
        case 3: off = UINT64_MAX - uni(0, 10); break;
        default: off = uni(0, c.track_len + 10); break;
        }
        c.offs.push_back(off);
        c.gains.push_back((float)std::uniform_real_distribution<double>(-2.0, 2.0)(rng));
    }
    return c;
}

static void check_invalid()
{
    Plan p;
    std::string why;
    const uint32_t row_len[2] = {10, 20}, rows[2] = {0, 1}, tracks[2] = {0, 1};
    const uint64_t offs[2] = {0, 5};
    auto run = [&](const uint32_t *rl, uint64_t row_stride, const uint32_t *r, const uint32_t *t, const uint64_t *o,
                   uint32_t n_tracks, uint64_t track_len, uint64_t track_stride) {
        return grail::mix::build_plan(rl, 2, row_stride, r, t, o, nullptr, 2, n_tracks, track_len, track_stride, 256, p, &why);
    };
    CHECK(run(row_len, 20, rows, tracks, offs, 2, 100, 100) == GRAIL_OK);
    const uint32_t bad_rows[2] = {0, 2}, bad_tracks[2] = {0, 2};
    CHECK(run(row_len, 20, bad_rows, tracks, offs, 2, 100, 100) == GRAIL_ERR_INVALID_ARG);     // row >= n_rows
    CHECK(run(row_len, 20, rows, bad_tracks, offs, 2, 100, 100) == GRAIL_ERR_INVALID_ARG);     // track >= n_tracks
    CHECK(run(row_len, 20, rows, tracks, offs, 2, 101, 100) == GRAIL_ERR_INVALID_ARG);         // track_len > stride
    CHECK(run(row_len, 19, rows, tracks, offs, 2, 100, 100) == GRAIL_ERR_INVALID_ARG);         // row_len > row_stride
    CHECK(run(row_len, 20, nullptr, tracks, offs, 2, 100, 100) == GRAIL_ERR_INVALID_ARG);
    CHECK(run(row_len, 20, rows, tracks, nullptr, 2, 100, 100) == GRAIL_ERR_INVALID_ARG);
    CHECK(run(nullptr, 20, rows, tracks, offs, 2, 100, 100) == GRAIL_ERR_INVALID_ARG);
    CHECK(run(row_len, 20, rows, nullptr, offs, 1, 100, 100) == GRAIL_OK);                     // NULL tracks: track 0
}

static void check_place_sequential(std::mt19937_64 &rng)
{
    auto uni = [&rng](int64_t lo, int64_t hi) { return std::uniform_int_distribution<int64_t>(lo, hi)(rng); };
    const uint32_t n_rows = (uint32_t)uni(1, 30), n_tracks = (uint32_t)uni(1, 5), n = (uint32_t)uni(0, 60);
    std::vector<uint32_t> row_len(n_rows), rows(n), tracks(n);
    std::vector<int64_t> gaps(n);
    for (auto &l : row_len) l = (uint32_t)uni(0, 3000);
    for (uint32_t i = 0; i < n; ++i) {
        rows[i] = (uint32_t)uni(0, n_rows - 1);
        tracks[i] = (uint32_t)uni(0, n_tracks - 1);
        gaps[i] = uni(-400, 2000);
    }
    std::vector<uint64_t> offs(n + 1), tl(n_tracks);
    const int rc = grail_mix_place_sequential(row_len.data(), n_rows, rows.data(), tracks.data(), gaps.data(), n, n_tracks,
                                              offs.data(), tl.data());
    std::vector<uint32_t> order(n);
    for (uint32_t i = 0; i < n; ++i) order[i] = i;
    std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return rows[a] < rows[b]; });
    std::vector<int64_t> cursor(n_tracks, 0), far(n_tracks, 0);
    bool ok = true;
    for (const uint32_t i : order) {
        const int64_t start = cursor[tracks[i]] + gaps[i];
        if (start < 0) { ok = false; break; }
        CHECK(rc != GRAIL_OK || offs[i] == (uint64_t)start);
        cursor[tracks[i]] = start + row_len[rows[i]];
        far[tracks[i]] = std::max(far[tracks[i]], cursor[tracks[i]]);
    }
    CHECK(rc == (ok ? GRAIL_OK : GRAIL_ERR_INVALID_ARG));
    for (uint32_t t = 0; ok && t < n_tracks; ++t) CHECK(tl[t] == (uint64_t)far[t]);
}

int main()
{
    std::mt19937_64 rng(20261016);
    check_invalid();
    for (int k = 0; k < 300 && !failures; ++k) check_case(random_case(rng, false, false));
    for (int k = 0; k < 12 && !failures; ++k) check_case(random_case(rng, false, true));
    for (int k = 0; k < 4 && !failures; ++k) check_case(random_case(rng, true, false));
    for (int k = 0; k < 300 && !failures; ++k) check_place_sequential(rng);
    if (failures) return 1;
    std::printf("sanitize mix driver: ok\n");
    return 0;
}
