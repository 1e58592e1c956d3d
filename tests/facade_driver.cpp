// facade_driver GROUP IN_DIR OUT_DIR — runs one named group of calls on the C++ facade (include/grail.hpp) over inputs that
// tests/test_facade_gpu.py / tests/test_facade_host.py wrote, and writes every result back.  It compares nothing: all
// judging is done in Python against the models.  Files are raw little-endian arrays (.f32 .f64 .u32 .bin); a set of rows
// NAME is NAME.len.u32 (one length per row) and NAME.f32 (the rows end to end); manifest.txt holds "key value ..." lines.
// A grail::Error ends the program with exit status 40 + status (the statuses are negative) and the message on stderr.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <map>
#include <sstream>
#include <string>
#include <vector>

#include "grail.hpp"

namespace {

using Rows = std::vector<std::vector<float>>;
std::string g_in, g_out;
std::map<std::string, std::vector<std::string>> g_manifest;

[[noreturn]] void die(const std::string &what)
{
    std::fprintf(stderr, "facade_driver: %s\n", what.c_str());
    std::exit(3);
}

template <typename T>
std::vector<T> rd(const std::string &name)
{
    std::ifstream f(g_in + "/" + name, std::ios::binary);
    if (!f) die("cannot read " + name);
    std::string bytes((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
    if (bytes.size() % sizeof(T)) die(name + ": not a whole number of elements");
    std::vector<T> out(bytes.size() / sizeof(T));
    if (!out.empty()) std::memcpy(out.data(), bytes.data(), bytes.size());
    return out;
}

void wr_bytes(const std::string &name, const void *p, size_t bytes)
{
    std::ofstream f(g_out + "/" + name, std::ios::binary);
    if (bytes) f.write((const char *)p, (std::streamsize)bytes);
    if (!f) die("cannot write " + name);
}

template <typename T>
void wr(const std::string &name, const std::vector<T> &v) { wr_bytes(name, v.data(), v.size() * sizeof(T)); }

template <typename T>
std::vector<std::vector<T>> split_rows(const std::vector<uint32_t> &lens, const std::vector<T> &flat, const std::string &name)
{
    std::vector<std::vector<T>> rows;
    size_t at = 0;
    for (uint32_t n : lens) {
        if (at + n > flat.size()) die(name + ": lengths past the data");
        rows.emplace_back(flat.begin() + at, flat.begin() + at + n);
        at += n;
    }
    if (at != flat.size()) die(name + ": data past the lengths");
    return rows;
}

Rows rd_rows(const std::string &name) { return split_rows(rd<uint32_t>(name + ".len.u32"), rd<float>(name + ".f32"), name); }

template <typename T>
void wr_rows(const std::string &name, const std::vector<std::vector<T>> &rows, const char *ext = ".f32")
{
    std::vector<uint32_t> lens;
    std::vector<T> flat;
    for (const auto &r : rows) {
        lens.push_back((uint32_t)r.size());
        flat.insert(flat.end(), r.begin(), r.end());
    }
    wr(name + ".len.u32", lens);
    wr(name + ext, flat);
}

void rd_manifest()
{
    std::ifstream f(g_in + "/manifest.txt");
    if (!f) die("cannot read manifest.txt");
    std::string line;
    while (std::getline(f, line)) {
        std::istringstream ss(line);
        std::string key, tok;
        if (!(ss >> key)) continue;
        while (ss >> tok) g_manifest[key].push_back(tok);
    }
}

const std::vector<std::string> &mf(const std::string &key)
{
    auto it = g_manifest.find(key);
    if (it == g_manifest.end()) die("manifest.txt has no " + key);
    return it->second;
}
uint32_t mf_u(const std::string &key, size_t i = 0) { return (uint32_t)std::stoul(mf(key).at(i)); }
double mf_d(const std::string &key, size_t i = 0) { return std::stod(mf(key).at(i)); }
std::vector<uint32_t> mf_us(const std::string &key)
{
    std::vector<uint32_t> out;
    for (const auto &t : mf(key)) out.push_back((uint32_t)std::stoul(t));
    return out;
}

// the status a call throws, GRAIL_OK if it returns
template <typename F>
int32_t thrown(F f)
{
    try {
        f();
    } catch (const grail::Error &e) {
        return e.status;
    }
    return GRAIL_OK;
}

std::vector<grail::Utterance> rd_utts(const std::string &name)
{
    const auto segs = rd<grail::PhonemeElem>(name + ".segs.bin");
    const auto offs = rd<uint32_t>(name + ".offs.u32"), vids = rd<uint32_t>(name + ".vids.u32"), seeds = rd<uint32_t>(name + ".seeds.u32");
    std::vector<grail::Utterance> utts;
    for (size_t u = 0; u + 1 < offs.size(); ++u) {
        grail::Utterance x;
        x.phonemes.assign(segs.begin() + offs[u], segs.begin() + offs[u + 1]);
        x.voice = vids.at(u);
        x.jitter_seed = seeds.at(u);
        utts.push_back(x);
    }
    return utts;
}

std::vector<grail::Fir> rd_filters(const std::string &name)
{
    const Rows taps = rd_rows(name);
    const auto origin = rd<uint32_t>(name + ".origin.u32");
    std::vector<grail::Fir> filters;
    for (size_t i = 0; i < taps.size(); ++i) {
        grail::Fir f;
        f.taps = taps[i];
        f.origin = origin.at(i);
        filters.push_back(f);
    }
    return filters;
}

void wr_limited(const std::string &name, const grail::Limited &l)
{
    wr_rows(name + ".out", l.rows);
    wr(name + ".gain.f32", l.min_gain);
    wr(name + ".nlim.u32", l.n_limited);
    wr(name + ".bad.u32", l.nonfinite);
    std::vector<uint32_t> refused;
    for (size_t g = 0; g < l.n_limited.size(); ++g) refused.push_back(l.refused(g) ? 1u : 0u);
    wr(name + ".refused.u32", refused);
}

// ---- group host: what needs no device --------------------------------------------------------------------------------
void group_host()
{
    const grail::Voice generic = grail::voices::generic();
    std::ifstream tf(g_in + "/text.txt", std::ios::binary);
    const std::string text((std::istreambuf_iterator<char>(tf)), std::istreambuf_iterator<char>());
    wr("phonemes.bin", grail::phoneme_elems(generic, text));
    wr("phonemes_of_nothing.bin", grail::phoneme_elems(generic, ""));

    const auto &d = mf("fir_design");           // rate lo hi taps, four tokens a design
    std::vector<uint32_t> origins;
    for (size_t i = 0; i + 3 < d.size(); i += 4) {
        const grail::Fir f = grail::fir_design((uint32_t)std::stoul(d[i]), std::stod(d[i + 1]), std::stod(d[i + 2]), (uint32_t)std::stoul(d[i + 3]));
        wr("design" + std::to_string(i / 4) + ".f32", f.taps);
        origins.push_back(f.origin);
    }
    wr("design_origins.u32", origins);
    const grail::Fir by_default = grail::fir_design(8000, 300.0, 3400.0);
    wr("design_default.f32", by_default.taps);

    const auto hops = split_rows(rd<uint32_t>("hops.len.u32"), rd<double>("hops.f64"), "hops");
    const uint32_t hop = mf_u("hop");
    std::vector<double> range, w4, w30;
    for (const auto &h : hops) {
        range.push_back(grail::loudness_range(h, hop));
        w4.push_back(grail::loudness_window_max(h, hop, 4));
        w30.push_back(grail::loudness_window_max(h, hop, 30));
    }
    wr("range.f64", range);
    wr("window4.f64", w4);
    wr("window30.f64", w30);

    std::vector<float> ceilings;
    for (float db : rd<float>("ceiling_db.f32")) ceilings.push_back(grail::limit_ceiling(db));
    wr("ceilings.f32", ceilings);

    std::vector<grail::Voice> at;
    std::vector<float> sharp{grail::voices::fast_sharpness(generic)};
    for (float rate : rd<float>("rates.f32")) {
        at.push_back(grail::voices::generic_at(rate));
        sharp.push_back(grail::voices::fast_sharpness(at.back()));
    }
    wr("voices_at.bin", at);
    wr("voice_generic.bin", std::vector<grail::Voice>{generic});
    wr("sharpness.f32", sharp);

    wr("phoneme_enum.i32", std::vector<int32_t>{(int32_t)grail::Phoneme::Silence, (int32_t)grail::Phoneme::Stop, (int32_t)grail::Phoneme::Glide,
                                                (int32_t)grail::Phoneme::A, (int32_t)grail::Phoneme::E});

    const Rows none, empty(3), full{std::vector<float>(64), {}, std::vector<float>(7)}, over{{}, std::vector<float>(65)};
    wr("chunk_stride.u32", std::vector<uint32_t>{(uint32_t)grail::detail::chunk_stride(nullptr), (uint32_t)grail::detail::chunk_stride(&none),
                                                 (uint32_t)grail::detail::chunk_stride(&empty), (uint32_t)grail::detail::chunk_stride(&full),
                                                 (uint32_t)grail::detail::chunk_stride(&over)});
}

// ---- group rows: the one-shot row calls --------------------------------------------------------------------------------
void group_rows()
{
    const grail::Gpu gpu(0, {grail::voices::generic()});

    const Rows lv = rd_rows("lv");
    const grail::Levels levels = gpu.levels(lv);
    wr("lv.sumsq.f64", levels.sumsq);
    wr("lv.peak.f32", levels.peak);
    wr("lv.bad.u32", levels.nonfinite);
    const grail::Levels of_none = gpu.levels({});
    wr("lv.none.u32", std::vector<uint32_t>{(uint32_t)of_none.sumsq.size(), (uint32_t)of_none.peak.size(), (uint32_t)of_none.nonfinite.size()});

    for (const char *name : {"lv", "tp"}) {
        const grail::TruePeak tp = gpu.true_peak(rd_rows(name));
        std::vector<double> db;
        for (size_t i = 0; i < tp.true_peak.size(); ++i) db.push_back(tp.db(i));
        wr(std::string(name) + ".tp.f64", tp.true_peak);
        wr(std::string(name) + ".tpbad.u32", tp.nonfinite);
        wr(std::string(name) + ".tpdb.f64", db);
    }

    const Rows ld = rd_rows("ld");
    const grail::Loudness loud = gpu.loudness(ld, mf_u("ld.rate"));
    std::vector<double> lufs;
    for (size_t i = 0; i < ld.size(); ++i) lufs.push_back(loud.lufs(i));
    wr("ld.ms.f64", loud.gated_ms);
    wr("ld.bad.u32", loud.nonfinite);
    wr("ld.lufs.f64", lufs);

    for (const std::string name : {"tl", "tl2"}) {
        const Rows tl = rd_rows(name);
        const grail::TrackLoudness track = gpu.track_loudness(tl, mf_u(name + ".rate"));
        std::vector<double> range, momentary, short_term;
        for (size_t i = 0; i < tl.size(); ++i) {
            range.push_back(track.range(i));
            momentary.push_back(track.momentary_max(i));
            short_term.push_back(track.short_term_max(i));
        }
        wr(name + ".ms.f64", track.gated_ms);
        wr(name + ".bad.u32", track.nonfinite);
        wr(name + ".hop.u32", std::vector<uint32_t>{track.hop});
        wr_rows(name + ".hops", track.hop_sumsq, ".f64");
        wr(name + ".range.f64", range);
        wr(name + ".momentary.f64", momentary);
        wr(name + ".short_term.f64", short_term);
    }

    const float ceiling = (float)mf_d("ceiling");
    const uint32_t ell = mf_u("lookahead_log2");
    wr_limited("lim1", gpu.limit(rd_rows("lim1"), ceiling, ell));
    wr_limited("lim2", gpu.limit(rd_rows("lim2"), ceiling, ell, 2));

    const Rows rs = rd_rows("rs");
    const auto pairs = mf_us("rs.pairs");
    for (size_t p = 0; p + 1 < pairs.size(); p += 2) wr_rows("rs" + std::to_string(p / 2) + ".out", gpu.resample(rs, pairs[p], pairs[p + 1]));

    const grail::FirSet set = gpu.fir_set(rd_filters("firset"));
    const Rows fr = rd_rows("fr");
    const std::vector<uint32_t> which = mf_us("fr.which");
    wr("firset.facts.u32", std::vector<uint32_t>{(uint32_t)set.tail(), set.longest()});
    wr_rows("fr.ring.out", gpu.fir(set, fr, which));
    wr_rows("fr.plain.out", gpu.fir(set, fr, which, false));
    wr_rows("fr.first_ring.out", gpu.fir(set, fr));
    wr_rows("fr.first_plain.out", gpu.fir(set, fr, {}, false));

    // the size checks that throw before anything is queued
    std::vector<int32_t> statuses;
    statuses.push_back(thrown([&] { gpu.fir(set, fr, {0, 1}); }));
    statuses.push_back(thrown([&] { gpu.limit(rd_rows("lim1"), ceiling, ell, 2); }));
    statuses.push_back(thrown([&] {
        grail::Utterance u;
        gpu.mix_leveled({u}, {grail::Placement{}, grail::Placement{}}, {-20.0f}, 1, 64);
    }));
    statuses.push_back(thrown([&] {
        grail::LimitStream ls = gpu.limit_stream(4, ceiling, ell, 2);
        ls.finish({1, 0, 0, 0});
    }));
    statuses.push_back(thrown([&] { gpu.limit(fr, ceiling, ell, 0); }));
    statuses.push_back(thrown([&] { gpu.fir_stream(set, 3, {0, 1}); }));
    wr("throws.i32", statuses);
}

// ---- group streams: the host-vector forms of the three chunked streams -----------------------------------------------------
// One stream through the calls of NAME.split.u32 (calls x rows: how many samples each row is fed per call; a call before
// which a unit has ended feeds that unit's rows again from their start), finish(which) after call `finish_after`, then
// finish() twice.  `open` makes a fresh stream: the second one is move-assigned onto the used one and fed the whole rows.
template <typename Open>
void drive_stream(const std::string &name, const Rows &rows, uint32_t group, Open open)
{
    const uint32_t n = (uint32_t)rows.size();
    const auto split = rd<uint32_t>(name + ".split.u32");
    const auto marks = rd<uint32_t>(name + ".marks.u32");          // one per unit: 1 ends at the first finish
    const uint32_t calls = (uint32_t)(split.size() / n), finish_after = mf_u(name + ".finish_after");
    const uint32_t unequal_before = g_manifest.count(name + ".unequal_before") ? mf_u(name + ".unequal_before") : 0xFFFFFFFFu;
    std::vector<size_t> at(n, 0);
    std::vector<uint8_t> ended(n / group, 0);
    auto stream = open();
    for (uint32_t c = 0; c < calls; ++c) {
        if (c == unequal_before) {         // the members of unit 0 fed different lengths: refused, nothing moves
            Rows chunks(n);
            for (uint32_t i = 0; i < group; ++i) chunks[i].assign(rows[i].begin() + at[i], rows[i].begin() + at[i] + 3 - (i ? 1 : 0));
            wr_rows(name + ".unequal", stream.next(chunks));
        }
        Rows chunks(n);
        for (uint32_t i = 0; i < n; ++i) {
            const uint32_t k = split[(size_t)c * n + i];
            const size_t from = ended[i / group] ? 0 : at[i];
            if (from + k > rows[i].size()) die(name + ": a split past its row");
            chunks[i].assign(rows[i].begin() + from, rows[i].begin() + from + k);
            if (!ended[i / group]) at[i] += k;
        }
        wr_rows(name + ".call" + std::to_string(c), stream.next(chunks));
        if (c == finish_after) {
            std::vector<uint8_t> which;
            for (size_t u = 0; u < ended.size(); ++u) which.push_back(ended[u] = (uint8_t)marks.at(u));
            wr_rows(name + ".finish_some", stream.finish(which));
        }
    }
    wr_rows(name + ".finish_rest", stream.finish());
    wr_rows(name + ".finish_again", stream.finish());
    stream = open();
    wr_rows(name + ".moved.call", stream.next(rows));
    wr_rows(name + ".moved.finish", stream.finish());
    wr(name + ".rows.u32", std::vector<uint32_t>{stream.rows(), (uint32_t)stream.tail()});
}

// LimitStream names its room delay(), not tail()
struct LimitStreamOfTheDriver : grail::LimitStream {
    LimitStreamOfTheDriver(grail::LimitStream &&s) : grail::LimitStream(std::move(s)) {}
    LimitStreamOfTheDriver &operator=(LimitStreamOfTheDriver &&o) noexcept
    {
        grail::LimitStream::operator=(std::move(o));
        return *this;
    }
    uint32_t tail() const { return delay(); }
};

void group_streams()
{
    const grail::Gpu gpu(0, {grail::voices::generic()});
    {
        const grail::FirSet set = gpu.fir_set(rd_filters("fsset"));
        const Rows rows = rd_rows("fs");
        const std::vector<uint32_t> which = mf_us("fs.which");
        wr_rows("fs.oneshot", gpu.fir(set, rows, which));
        drive_stream("fs", rows, 1, [&] { return gpu.fir_stream(set, (uint32_t)rows.size(), which); });
    }
    for (const char *name : {"ra", "rb"}) {
        const Rows rows = rd_rows(name);
        const uint32_t rate_in = mf_u(std::string(name) + ".rates", 0), rate_out = mf_u(std::string(name) + ".rates", 1);
        wr_rows(std::string(name) + ".oneshot", gpu.resample(rows, rate_in, rate_out));
        drive_stream(name, rows, 1, [&] { return gpu.resample_stream(rate_in, rate_out, (uint32_t)rows.size()); });
    }
    {
        const Rows rows = rd_rows("ls");
        const float ceiling = (float)mf_d("ceiling");
        const uint32_t ell = mf_u("lookahead_log2"), group = mf_u("ls.group");
        wr_limited("ls.oneshot", gpu.limit(rows, ceiling, ell, group));
        drive_stream("ls", rows, group, [&] { return LimitStreamOfTheDriver(gpu.limit_stream((uint32_t)rows.size(), ceiling, ell, group)); });
        grail::LimitStream facts = gpu.limit_stream((uint32_t)rows.size(), ceiling, ell, group);
        wr("ls.facts.u32", std::vector<uint32_t>{facts.rows(), facts.groups(), facts.delay()});

        // finish_async on device buffers: row 0 alone, fed in one call, its tail written where the caller says
        grail::LimitStream alone = gpu.limit_stream(1, ceiling, ell);
        const Rows head = alone.next({rows.at(0)});
        const uint64_t room = 64;          // >= delay()
        void *d_out = nullptr, *d_len = nullptr;
        uint32_t n = 0;
        grail::check(alone.delay() <= room ? GRAIL_OK : GRAIL_ERR_INVALID_ARG);
        grail::check(grail_device_alloc(gpu.ctx(), room * sizeof(float), &d_out));
        int rc = grail_device_alloc(gpu.ctx(), sizeof(uint32_t), &d_len);
        if (!rc) rc = thrown([&] { alone.finish_async((float *)d_out, room, (uint32_t *)d_len); });
        if (!rc) rc = grail_sync(gpu.ctx());
        if (!rc) rc = grail_memcpy_d2h(gpu.ctx(), &n, d_len, sizeof n);
        std::vector<float> tail(!rc && n <= room ? n : 0);
        if (!rc && !tail.empty()) rc = grail_memcpy_d2h(gpu.ctx(), tail.data(), d_out, tail.size() * sizeof(float));
        grail_device_free(gpu.ctx(), d_out);
        if (d_len) grail_device_free(gpu.ctx(), d_len);
        grail::check(rc);
        wr_rows("ls.async", Rows{head.at(0), tail});
    }
}

// ---- group chain: synthesis and what follows it ----------------------------------------------------------------------------
std::vector<grail::Placement> rd_placements(const std::string &name)
{
    const auto p = rd<uint32_t>(name + ".place.u32");      // utterance, track, offset per placement
    const auto gain = rd<float>(name + ".gain.f32");
    std::vector<grail::Placement> out;
    for (size_t i = 0; i * 3 + 2 < p.size(); ++i) out.push_back(grail::Placement{p[i * 3], p[i * 3 + 1], p[i * 3 + 2], gain.at(i)});
    return out;
}

void group_chain()
{
    const std::vector<grail::Voice> voices = rd<grail::Voice>("voices.bin");
    const grail::Gpu gpu(0, voices);
    wr("voices.count.u32", std::vector<uint32_t>{(uint32_t)gpu.voices().size()});

    const auto utts = rd_utts("syn");
    const Rows exact = gpu.synthesize(utts);
    wr_rows("syn.out", exact);
    wr("syn.lengths.u32", gpu.lengths(utts));
    {
        grail::Stream stream(gpu, utts, mf_u("chunk"));
        Rows joined(utts.size()), chunks;
        uint32_t pulls = 0, longest = 0;
        while (stream.next(chunks)) {
            ++pulls;
            for (size_t u = 0; u < chunks.size(); ++u) {
                joined[u].insert(joined[u].end(), chunks[u].begin(), chunks[u].end());
                longest = std::max<uint32_t>(longest, (uint32_t)chunks[u].size());
            }
        }
        grail::Stream of_nothing(gpu, {}, mf_u("chunk"));
        const uint32_t nothing = of_nothing.next(chunks) ? 1u : 0u;
        wr_rows("stream.out", joined);
        wr("stream.facts.u32", std::vector<uint32_t>{pulls, longest, nothing, (uint32_t)chunks.size()});
    }

    gpu.set_arithmetic(grail::Gpu::Arithmetic::Fast);
    const uint32_t served = gpu.fast_arithmetic_served() ? 1u : 0u;
    wr_rows("fast.out", gpu.synthesize(utts));
    gpu.set_arithmetic(grail::Gpu::Arithmetic::Exact);
    wr_rows("exact_again.out", gpu.synthesize(utts));
    wr("fast.served.u32", std::vector<uint32_t>{served, gpu.fast_arithmetic_served() ? 1u : 0u});

    const uint32_t n_tracks = mf_u("n_tracks"), track_len = mf_u("track_len");
    const auto mix_utts = rd_utts("mix");
    wr_rows("mix.rows", gpu.synthesize(mix_utts));
    wr_rows("mix.out", gpu.mix(mix_utts, rd_placements("mix"), n_tracks, track_len));

    const auto lev_utts = rd_utts("lev");
    const auto lev_place = rd_placements("lev");
    const auto level_db = rd<float>("lev.level_db.f32");
    std::vector<float> gains;
    uint32_t unleveled = 77, limited = 77;
    wr_rows("lev.rows", gpu.synthesize(lev_utts));
    wr_rows("lev.out", gpu.mix_leveled(lev_utts, lev_place, level_db, n_tracks, track_len, GRAIL_LEVEL_RMS, &gains, &unleveled));
    wr("lev.gains.f32", gains);
    wr("lev.counts.u32", std::vector<uint32_t>{unleveled});
    gains.clear();
    unleveled = 77;
    wr_rows("levlim.out", gpu.mix_leveled_limited(lev_utts, lev_place, level_db, (float)mf_d("ceiling_db"), n_tracks, track_len, GRAIL_LEVEL_RMS,
                                                  &gains, &unleveled, &limited));
    wr("levlim.gains.f32", gains);
    wr("levlim.counts.u32", std::vector<uint32_t>{unleveled, limited});
    wr_rows("lev.plain.out", gpu.mix_leveled(lev_utts, lev_place, level_db, n_tracks, track_len));      // no out-parameters

    const Rows wav = rd_rows("wav");          // row 0: mono; rows 1 and 2: the two tracks; row 3: a track of another length
    const uint32_t rate = mf_u("wav.rate");
    gpu.save_wav(g_out + "/mono.wav", wav.at(0), rate);
    gpu.save_wav_frames(g_out + "/stereo.wav", {wav.at(1), wav.at(2)}, rate);
    wr("wav.throws.i32", std::vector<int32_t>{thrown([&] { gpu.save_wav_frames(g_out + "/never.wav", {wav.at(1), wav.at(3)}, rate); })});

    {
        const auto live_utts = rd_utts("live");      // one chain, appended utterance by utterance
        grail::LiveStream live(gpu, mf_u("live.chunk"), live_utts.at(0).voice, live_utts.at(0).jitter_seed);
        std::vector<float> out;
        std::vector<uint32_t> pending{live.pending()}, pulled;
        for (const auto &u : live_utts) {
            live.append(u.phonemes);
            pending.push_back(live.pending());
            for (int pull = 0; pull < 3; ++pull) {      // a few pulls between appends: the chain may run dry and wait
                const std::vector<float> chunk = live.next();
                pulled.push_back((uint32_t)chunk.size());
                out.insert(out.end(), chunk.begin(), chunk.end());
            }
            pending.push_back(live.pending());
        }
        live.finish();
        for (uint32_t pull = 0; pull < 100000; ++pull) {
            const std::vector<float> chunk = live.next();
            pulled.push_back((uint32_t)chunk.size());
            if (chunk.empty()) break;
            out.insert(out.end(), chunk.begin(), chunk.end());
        }
        wr("live.out.f32", out);
        wr("live.pending.u32", pending);
        wr("live.pulled.u32", pulled);
        wr("live.chunk.u32", std::vector<uint32_t>{live.chunk()});
    }
}

}  // namespace

int main(int argc, char **argv)
{
    if (argc != 4) {
        std::fprintf(stderr, "usage: facade_driver GROUP IN_DIR OUT_DIR   (GROUP: host, rows, streams, chain)\n");
        return 2;
    }
    const std::string group = argv[1];
    g_in = argv[2];
    g_out = argv[3];
    try {
        rd_manifest();
        if (group == "host") group_host();
        else if (group == "rows") group_rows();
        else if (group == "streams") group_streams();
        else if (group == "chain") group_chain();
        else die("no group " + group);
    } catch (const grail::Error &e) {
        std::fprintf(stderr, "facade_driver: %s: %s\n", group.c_str(), e.what());
        return 40 + e.status;
    }
    std::printf("facade_driver: %s: done\n", group.c_str());
    return 0;
}
