// transform_state.h — what transforms.cpp (rows limited, resampled and filtered at once) and transform_streams.cpp (the same
// as streams) keep per context, and how a caller's pointer is told to be one of the context's own.  Internal to those two.
#pragma once

#include "api_internal.hpp"

namespace grail {
namespace host {

// What a context owns by handle and the caller names by pointer.  A pointer from outside is looked up, never looked into: a
// stale one, or another context's, is not found.
template <typename T>
class Owned {
public:
    T *find(const T *p) const
    {
        for (const auto &q : items_)
            if (q.get() == p) return q.get();
        return nullptr;
    }
    T *add(std::unique_ptr<T> p) { return items_.emplace_back(std::move(p)).get(); }
    // (the caller has waited for whatever may still use it)
    void remove(const T *p)
    {
        items_.erase(std::remove_if(items_.begin(), items_.end(), [p](const auto &q) { return q.get() == p; }), items_.end());
    }
    template <typename Pred>
    bool any(Pred pred) const { return std::any_of(items_.begin(), items_.end(), [&](const auto &q) { return pred(*q); }); }

private:
    std::vector<std::unique_ptr<T>> items_;
};

struct ResampleTable {
    uint32_t up = 0, down = 0;              // 0: the slot holds no table
    uint64_t used = 0;                      // the call that last asked for it (the oldest is evicted)
    std::vector<int32_t> host;              // (kept while the upload may be in flight)
    DeviceBuffer<int32_t> dev;              // [up][taps]
};

// Per context (grail_ctx::transform_state), kept from call to call and only ever grown (DeviceBuffer::reserve, to the exact
// size), freed by grail_destroy: the chunk numbers that a limiter call folds (16 B per group and chunk of 4096 samples), the
// chunks' non-finite counts that a resampling call folds (4 B per chunk of 1024 outputs), the resampler's tables of the
// last few pairs of rates, the same counts of a filtering call (4 B per chunk of 2048 outputs), the filter sets the caller
// has created, the block states (16 B per section of the set's bound and block of 1024 steps) and counts of a blocked
// recursive-filtering call, the curve sets the caller has created, the non-finite counts of a spectrum
// call (4 B per row and chunk of 8 frames), the spectrum sets the caller has created, and the streams open (each with its rows' state: api_internal.hpp, ChunkedStream).  A stream's calls use the
// chunk scratch of their kind.
struct TransformState : CtxPart {
    DeviceBuffer<unsigned char> d_lstat;    // limiter chunks
    DeviceBuffer<uint32_t> d_rbad;          // resampler chunks: non-finite counts
    ResampleTable tables[4];
    uint64_t table_calls = 0;
    DeviceBuffer<uint32_t> d_firbad;        // FIR chunks: non-finite counts
    Owned<grail_fir> firs;                  // the filter sets alive
    Owned<grail_filter_stream> fir_streams; // ... and, after them (they die first), the filter streams open on them
    Owned<grail_resample_stream> resample_streams;  // the resample streams open (each with its own copy of its pair's table)
    Owned<grail_limit_stream> limit_streams;        // the limit streams open
    DeviceBuffer<double> d_mpeak;           // meter stream chunks (4096 output times each): the largest |y|
    DeviceBuffer<uint32_t> d_mbad;          // ... and the non-finite counts
    Owned<grail_meter_stream> meter_streams;        // the meter streams open
    DeviceBuffer<double> d_iirblock;        // blocked recursive filtering: 2 S' doubles of state a block (iir_plan.h)
    DeviceBuffer<uint32_t> d_iirbad;        // ... and the non-finite counts of its output pass's workgroups
    Owned<grail_iir> iirs;                  // the recursive filter sets alive
    Owned<grail_iir_stream> iir_streams;    // ... and, after them (they die first), the IIR streams open on them
    Owned<grail_dyn> dyns;                  // the curve sets alive
    Owned<grail_dyn_stream> dyn_streams;    // ... and, after them (they die first), the dynamics streams open on them
    DeviceBuffer<uint32_t> d_specbad;       // spectrum chunks (8 frames each): non-finite counts
    Owned<grail_spectrum> spectra;          // the spectrum sets alive
};

// what the context has, made by nobody: NULL before the first call that needed it
inline TransformState *peek(grail_ctx *ctx) { return static_cast<TransformState *>(ctx->transform_state.get()); }

// ... and made at first use (the refusal's words are from when levels.cpp kept this state)
inline int state(grail_ctx *ctx, TransformState **st)
{
    if (!ctx->transform_state) ctx->transform_state.reset(new (std::nothrow) TransformState());
    return (*st = peek(ctx)) ? GRAIL_OK : fail(GRAIL_ERR_OUT_OF_MEMORY, "level state");
}

// the caller's pointer as one of ctx's own, of the list named (&TransformState::firs, say), or NULL
template <typename T>
T *own(grail_ctx *ctx, Owned<T> TransformState::*list, const T *p)
{
    return peek(ctx) ? (peek(ctx)->*list).find(p) : nullptr;
}

}  // namespace host
}  // namespace grail
