// fake_hip.h — the HIP entry points that the owner types of grail-rs_amd/csrc/api_internal.hpp reference (Event, Stream,
// DeviceBuffer, PinnedBuffer), as host functions over malloc / free for programs that are built with g++ and linked
// WITHOUT the HIP runtime (tests/sanitize_options_driver.cpp, tests/sanitize_owners_driver.cpp).  They keep a log of the
// calls in order and the set of what is live, and can make the k-th allocation fail.  The definitions are not inline:
// include this in exactly one translation unit of a program.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdlib>
#include <set>
#include <string>
#include <vector>

namespace fake_hip {

struct Call {
    std::string name;
    const void *what;          // the allocation or handle made / released / waited for
    size_t bytes;              // hipMalloc, hipHostMalloc: the size asked for
};

struct State {
    std::vector<Call> log;             // every call, in order
    std::set<const void *> live;       // allocations and handles made and not yet released
    long fail_at = 0;                  // k > 0: the k-th allocation (of any kind) from now fails; 0: none does
    int stray_releases = 0;            // releases of something that is not live (never freed for real)
};

inline State &state()
{
    static State s;
    return s;
}

// the names of the calls logged from `mark` on, separated by blanks
inline std::string names_since(size_t mark)
{
    std::string s;
    for (size_t i = mark; i < state().log.size(); ++i) s += (s.empty() ? "" : " ") + state().log[i].name;
    return s;
}

inline hipError_t make(const char *name, void **out, size_t bytes)
{
    State &s = state();
    if (s.fail_at > 0 && --s.fail_at == 0) {
        s.log.push_back({name, nullptr, bytes});
        *out = reinterpret_cast<void *>(0x10);     // (what a failed call leaves behind is not the caller's to keep or release)
        return hipErrorOutOfMemory;
    }
    *out = std::malloc(bytes ? bytes : 1);
    s.log.push_back({name, *out, bytes});
    s.live.insert(*out);
    return hipSuccess;
}

inline hipError_t release(const char *name, void *p)
{
    State &s = state();
    s.log.push_back({name, p, 0});
    if (!s.live.erase(p)) {
        ++s.stray_releases;
        return hipErrorInvalidValue;
    }
    std::free(p);
    return hipSuccess;
}

}  // namespace fake_hip

extern "C" {

hipError_t hipMalloc(void **ptr, size_t size) { return fake_hip::make("hipMalloc", ptr, size); }
hipError_t hipFree(void *ptr) { return fake_hip::release("hipFree", ptr); }
hipError_t hipHostMalloc(void **ptr, size_t size, unsigned int) { return fake_hip::make("hipHostMalloc", ptr, size); }
hipError_t hipHostFree(void *ptr) { return fake_hip::release("hipHostFree", ptr); }
hipError_t hipEventCreate(hipEvent_t *event) { return fake_hip::make("hipEventCreate", (void **)event, 0); }
hipError_t hipEventCreateWithFlags(hipEvent_t *event, unsigned) { return fake_hip::make("hipEventCreateWithFlags", (void **)event, 0); }
hipError_t hipEventDestroy(hipEvent_t event) { return fake_hip::release("hipEventDestroy", event); }
hipError_t hipStreamCreateWithFlags(hipStream_t *stream, unsigned int) { return fake_hip::make("hipStreamCreateWithFlags", (void **)stream, 0); }
hipError_t hipStreamDestroy(hipStream_t stream) { return fake_hip::release("hipStreamDestroy", stream); }
hipError_t hipStreamSynchronize(hipStream_t stream)
{
    fake_hip::state().log.push_back({"hipStreamSynchronize", stream, 0});
    return hipSuccess;
}

}  // extern "C"
