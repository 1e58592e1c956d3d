// sanitize_owners_driver.cpp — the owner types of grail-rs_amd/csrc/api_internal.hpp (Event, Stream, DeviceBuffer,
// PinnedBuffer) and the structs that hold them (grail_ctx, grail_stream, grail_batch) under AddressSanitizer + UBSan with
// leak detection.  Built by tests/test_sanitizers.py with g++ and linked against tests/fake_hip.h instead of the HIP
// runtime: every statement below is about the fakes' log of calls and their set of live resources.
#include "../grail-rs_amd/csrc/api_internal.hpp"
#include "fake_hip.h"

// ---- the error helpers of grail_api.cpp (DeviceBuffer::reserve reports through them)
namespace grail {
namespace host {
static thread_local std::string g_err;
int fail(int status, const std::string &msg)
{
    g_err = msg;
    return status;
}
int hip_fail(hipError_t e, const char *what) { return fail(e == hipErrorOutOfMemory ? GRAIL_ERR_OUT_OF_MEMORY : GRAIL_ERR_HIP, what); }
std::string &last_error() { return g_err; }
}  // namespace host
}  // namespace grail
// ----

using namespace grail::host;
using fake_hip::names_since;

static fake_hip::State &F = fake_hip::state();

#define CHECK(cond)                                                                              \
    do {                                                                                         \
        if (!(cond)) {                                                                           \
            std::fprintf(stderr, "%s:%d: CHECK failed: %s\n  calls so far: %s\n", __FILE__, __LINE__, #cond, names_since(0).c_str()); \
            std::exit(1);                                                                        \
        }                                                                                        \
    } while (0)

// What every owner kind promises.  fill(owner) makes it hold a fresh resource through the call named `create`; `release`
// is the call that lets one go.
template <typename Owner, typename Fill>
static void owner_kind(const std::string &create, const std::string &release, Fill fill)
{
    CHECK(F.live.empty());
    size_t mark = F.log.size();
    {
        Owner o;                                    // default-constructed: no call, at either end
        CHECK(!o.get());
    }
    CHECK(F.log.size() == mark);
    {
        Owner o;                                    // allocate, destruct: exactly one release
        CHECK(fill(o) == hipSuccess && o.get() && F.live.count(o.get()) && F.live.size() == 1);
        CHECK(names_since(mark) == create);
        mark = F.log.size();
    }
    CHECK(names_since(mark) == release && F.live.empty());
    mark = F.log.size();
    {
        Owner a;                                    // move construction: the resource changes hands without a call
        CHECK(fill(a) == hipSuccess);
        const auto held = a.get();
        Owner b(std::move(a));
        CHECK(!a.get() && b.get() == held && names_since(mark) == create);
    }
    CHECK(names_since(mark) == create + " " + release && F.live.empty());   // (the moved-from one released nothing)
    {
        Owner a, b;                                 // move assignment: the target's own resource goes first
        CHECK(fill(a) == hipSuccess && fill(b) == hipSuccess && F.live.size() == 2);
        const auto held = a.get();
        const auto gone = b.get();
        mark = F.log.size();
        b = std::move(a);
        CHECK(names_since(mark) == release && F.log.back().what == gone && F.live.size() == 1);
        CHECK(!a.get() && b.get() == held);
        Owner &same = b;                            // self-move-assignment keeps it
        b = std::move(same);
        CHECK(b.get() == held && names_since(mark) == release && F.live.count(held));
        mark = F.log.size();
    }
    CHECK(names_since(mark) == release && F.live.empty());
    {
        Owner o;                                    // filled again: what was held is released first
        CHECK(fill(o) == hipSuccess);
        const auto first = o.get();
        mark = F.log.size();
        CHECK(fill(o) == hipSuccess && o.get());
        CHECK(names_since(mark) == release + " " + create && F.log[mark].what == first && F.live.size() == 1);
    }
    CHECK(F.live.empty());
    {
        Owner o;                                    // a failed allocation: holds nothing, releases nothing
        F.fail_at = 1;
        CHECK(fill(o) != hipSuccess && !o.get() && F.live.empty());
        mark = F.log.size();
    }
    CHECK(F.log.size() == mark);
    {
        Owner o;                                    // ... also over a held resource (which has gone by then)
        CHECK(fill(o) == hipSuccess);
        F.fail_at = 1;
        mark = F.log.size();
        CHECK(fill(o) != hipSuccess && !o.get() && F.live.empty() && names_since(mark) == release + " " + create);
        mark = F.log.size();
    }
    CHECK(F.log.size() == mark && F.stray_releases == 0);
}

static void device_buffer_reserve()
{
    const hipStream_t stream = reinterpret_cast<hipStream_t>(0x40);      // (the fake only logs it)
    {
        DeviceBuffer<double> b;
        CHECK(b.capacity() == 0);
        size_t mark = F.log.size();
        CHECK(b.reserve(stream, 4, 10) == GRAIL_OK);                       // empty: the allocation alone, no wait
        CHECK(names_since(mark) == "hipMalloc" && F.log.back().bytes == 10 * sizeof(double) && b.capacity() == 10 && b.get());
        mark = F.log.size();
        CHECK(b.reserve(stream, 10) == GRAIL_OK && b.reserve(stream, 3, 1000) == GRAIL_OK && b.reserve(stream, 0) == GRAIL_OK);
        CHECK(F.log.size() == mark && b.capacity() == 10);                 // enough room: no call at all
        const void *old = b.get();
        CHECK(b.reserve(stream, 11, 20) == GRAIL_OK);                      // too small: wait, free, allocate `want`
        CHECK(names_since(mark) == "hipStreamSynchronize hipFree hipMalloc");
        CHECK(F.log[mark].what == stream && F.log[mark + 1].what == old && F.log[mark + 2].bytes == 20 * sizeof(double));
        CHECK(b.capacity() == 20 && F.live.size() == 1);
        F.fail_at = 1;                                                     // a growth that fails: nothing held
        CHECK(b.reserve(stream, 21) == GRAIL_ERR_OUT_OF_MEMORY && !b.get() && b.capacity() == 0 && F.live.empty());
        mark = F.log.size();
    }
    for (const size_t n : {size_t(0), size_t(1)}) {                        // sizes 0 and 1: one element
        DeviceBuffer<uint32_t> b, c;
        size_t mark = F.log.size();
        CHECK(b.reserve(stream, n) == GRAIL_OK && b.capacity() == 1 && F.log.back().bytes == sizeof(uint32_t));
        CHECK(c.alloc(n) == hipSuccess && c.capacity() == 1 && F.log.back().bytes == sizeof(uint32_t));
        CHECK(names_since(mark) == "hipMalloc hipMalloc");
        mark = F.log.size();
        CHECK(b.reserve(stream, 0) == GRAIL_OK && b.reserve(stream, 1) == GRAIL_OK && F.log.size() == mark);
    }
    CHECK(F.live.empty());
}

// capacities: what was asked for while something is held, 0 otherwise
static void capacities()
{
    DeviceBuffer<float> d;
    PinnedBuffer h;
    CHECK(d.alloc(7) == hipSuccess && d.capacity() == 7 && F.log.back().bytes == 7 * sizeof(float));
    CHECK(h.alloc(100) == hipSuccess && h.capacity() == 100 && F.log.back().bytes == 100 && F.log.back().name == "hipHostMalloc");
    DeviceBuffer<float> d2(std::move(d));
    PinnedBuffer h2;
    h2 = std::move(h);
    CHECK(d.capacity() == 0 && d2.capacity() == 7 && h.capacity() == 0 && h2.capacity() == 100);
    F.fail_at = 1;
    CHECK(d2.alloc(9) == hipErrorOutOfMemory && !d2.get() && d2.capacity() == 0);
    F.fail_at = 1;
    CHECK(h2.alloc(9) == hipErrorOutOfMemory && !h2.get() && h2.capacity() == 0);
    const size_t mark = F.log.size();
    d2.reset();
    h2.reset();
    CHECK(F.log.size() == mark && F.live.empty());
}

// stands for a unit's private part of a context (HostPipe, MixState, LevelState)
struct Part : CtxPart {
    Stream side;
    Event ev[2];
    DeviceBuffer<float> d;
    PinnedBuffer h;
    bool fill()
    {
        return side.create() == hipSuccess && ev[0].create() == hipSuccess && ev[1].create() == hipSuccess &&
               d.alloc(16) == hipSuccess && h.alloc(64) == hipSuccess;
    }
};

static void fill_batch(grail_batch &b)
{
    CHECK(b.d_segs.alloc(4) == hipSuccess && b.d_offsets.alloc(3) == hipSuccess && b.d_voice_ids.alloc(2) == hipSuccess &&
          b.d_seeds.alloc(2) == hipSuccess && b.d_perm.alloc(2) == hipSuccess && b.d_len_bound.alloc(2) == hipSuccess &&
          b.d_elems.alloc(98) == hipSuccess);
    b.packed.resize(2);
    CHECK(b.packed[0].d_perm.alloc(2) == hipSuccess);                      // (packed[1]: "the plain order is as good")
    b.packed.resize(5);                                                    // (the vector moves its elements)
}

static void holders()
{
    CHECK(F.live.empty());
    size_t mark = F.log.size();
    size_t made = 0;
    {
        grail_ctx ctx;
        CHECK(F.log.size() == mark);
        CHECK(ctx.stream.create() == hipSuccess && ctx.ev_start.create(true) == hipSuccess && ctx.ev_stop.create(true) == hipSuccess);
        CHECK(ctx.d_truncated.alloc(TRUNCATED_WORDS) == hipSuccess && ctx.d_voices.alloc(2) == hipSuccess &&
              ctx.d_voice_elems.alloc(98) == hipSuccess);
        for (std::unique_ptr<CtxPart> *part : {&ctx.host_pipe, &ctx.mix_state, &ctx.level_state}) {
            Part *p = new Part();
            part->reset(p);
            CHECK(p->fill());
        }
        const hipStream_t s = ctx.stream;           // (the implicit conversions the call sites rely on)
        const hipEvent_t e = ctx.ev_stop;
        CHECK(s == ctx.stream.get() && e == ctx.ev_stop.get());
        made = F.live.size();
        CHECK(made == 6 + 3 * 5);
        mark = F.log.size();
    }
    // member order: the context's stream goes last, behind everything that may have been queued on it
    CHECK(F.log.size() == mark + made && F.live.empty());
    CHECK(F.log.back().name == "hipStreamDestroy");
    for (size_t i = mark; i + 1 < F.log.size(); ++i) CHECK(F.log[i].name != "hipStreamDestroy" || i < mark + 3 * 5);   // (the parts' own)
    {
        grail_stream *s = new grail_stream();
        for (DeviceBuffer<uint32_t> *d : {&s->d_state, &s->d_counts, &s->d_open, &s->d_consumed, &s->d_new_offs})
            CHECK(d->alloc(8) == hipSuccess);
        CHECK(s->d_new.alloc(8) == hipSuccess && s->d_new_elems.alloc(8) == hipSuccess);
        for (int i = 0; i < 2; ++i) CHECK(s->h_stage[i].alloc(256) == hipSuccess && s->ev_stage[i].create() == hipSuccess);
        s->own.reset(new grail_batch());            // a live stream owns its batch
        fill_batch(*s->own);
        CHECK(F.live.size() == 7 + 4 + 8);
        delete s;
        CHECK(F.live.empty());
        grail_batch *b = new grail_batch();
        fill_batch(*b);
        CHECK(F.live.size() == 8);
        delete b;
        CHECK(F.live.empty());
    }
}

int main()
{
    owner_kind<Event>("hipEventCreateWithFlags", "hipEventDestroy", [](Event &e) { return e.create(); });
    owner_kind<Event>("hipEventCreate", "hipEventDestroy", [](Event &e) { return e.create(true); });
    owner_kind<Stream>("hipStreamCreateWithFlags", "hipStreamDestroy", [](Stream &s) { return s.create(); });
    owner_kind<DeviceBuffer<float>>("hipMalloc", "hipFree", [](DeviceBuffer<float> &d) { return d.alloc(5); });
    owner_kind<PinnedBuffer>("hipHostMalloc", "hipHostFree", [](PinnedBuffer &h) { return h.alloc(100); });
    capacities();
    device_buffer_reserve();
    holders();
    CHECK(F.live.empty() && F.stray_releases == 0 && F.fail_at == 0);
    std::printf("sanitize owners driver: ok (%zu calls)\n", F.log.size());
    return 0;
}
