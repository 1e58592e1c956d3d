// row_kernel_common.h — what the row-transform kernels share around their own loops (fir_kernels.hip, resample_kernels.hip,
// limiter_kernels.hip, iir_kernels.hip, meter_stream_kernels.hip; the finite test also loudness_common.h and
// true_peak_kernels.hip): the finite test, a stream's state word, the count of a chunk's non-finite samples on its way to
// cbad, the bookkeeping of a (row, chunk) workgroup, and what an advance or a totals kernel does with a row's chunks, its
// ring and its refusal.  The folds themselves are not here, and the resampler's chunk kernels keep the bookkeeping in their own
// text: DESIGN.md §4.21 says which copies are kept on purpose.  Device code only, no HIP runtime call.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace grail {

// false for NaN and Inf: the one meaning of "finite" in every count and every +0.0 that replaces a sample
__device__ __forceinline__ bool finite_f32(float x) { return __builtin_fabsf(x) <= 3.4028234663852886e38f; }

// ---- a stream's state word ----------------------------------------------------------------------------------------------------
// Word 0 of a row's (or a limiter group's) state, whatever follows it: N = the samples fed so far, with STREAM_ENDED set once
// the row has ended.  A call reads it in every kernel it launches; only the call's last kernel writes it: N + n, or
// N | STREAM_ENDED for a finishing call.  A row that has ended and is fed is refused (refuse_counts), its state as it was.
constexpr uint64_t STREAM_ENDED = 1ull << 63;
__device__ __forceinline__ bool stream_ended(uint64_t w) { return (w & STREAM_ENDED) != 0; }
__device__ __forceinline__ uint64_t stream_fed(uint64_t w) { return w & ~STREAM_ENDED; }

// what a refused row reads: 0xFFFFFFFF where its length (or count of results) would stand, no non-finite samples
__device__ __forceinline__ void refuse_counts(uint32_t *out_len, uint32_t *nonfinite, uint64_t u)
{
    if (out_len) out_len[u] = 0xFFFFFFFFu;
    if (nonfinite) nonfinite[u] = 0u;
}

// ---- counts: integers, so any order ---------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t wave_sum(uint32_t x)
{
#pragma unroll
    for (int s = 32; s > 0; s >>= 1) x += (uint32_t)__shfl_xor((int)x, s, 64);
    return x;
}

// the count of a workgroup of four waves into its chunk's slot; red: four words of LDS.  Every lane comes here (a barrier).
__device__ __forceinline__ void block_count_store(uint32_t bad, uint32_t *red, uint32_t tid, uint32_t *cbad,
                                                  uint64_t u, uint32_t grid_chunks, uint32_t c)
{
    bad = wave_sum(bad);
    if ((tid & 63u) == 0u) red[tid >> 6] = bad;
    __syncthreads();
    if (tid == 0u) cbad[u * grid_chunks + c] = red[0] + red[1] + red[2] + red[3];
}

// ---- a workgroup = one (row, chunk of CHUNK outputs) ------------------------------------------------------------------------
__device__ __forceinline__ void chunk_of_block(uint32_t grid_chunks, uint64_t &u, uint32_t &c)
{
    u = blockIdx.x / grid_chunks;
    c = (uint32_t)(blockIdx.x - u * grid_chunks);
}

// a chunk past the row's outputs has nothing to do, but for chunk 0: it runs even with no output to write, because it counts
__device__ __forceinline__ bool chunk_idle(uint64_t m0, uint64_t n_out, uint32_t c) { return m0 >= n_out && c != 0u; }

// is the chunk at output m0 the row's last, and how many outputs has it
template <uint32_t CHUNK>
__device__ __forceinline__ void chunk_extent(uint64_t m0, uint64_t n_out, bool &last, uint32_t &count)
{
    last = m0 + CHUNK >= n_out;
    count = m0 >= n_out ? 0u : (last ? (uint32_t)(n_out - m0) : CHUNK);
}

// the samples [own_lo, own_hi) of the n fed that the chunk at m0 counts non-finite ones in, where outputs and samples run
// at one rate: its own CHUNK, the last chunk to the end of them
template <uint32_t CHUNK>
__device__ __forceinline__ void chunk_owned(uint64_t m0, uint64_t n, bool last, int64_t &own_lo, int64_t &own_hi)
{
    own_lo = (int64_t)m0 < (int64_t)n ? (int64_t)m0 : (int64_t)n;
    own_hi = last || (int64_t)(m0 + CHUNK) > (int64_t)n ? (int64_t)n : (int64_t)(m0 + CHUNK);
}

// what a chunk owns past the stretch it staged, [from, to): counted from the row itself by the workgroup's 256 lanes
template <typename T>
__device__ __forceinline__ void count_owned_tail(const float *row, T from, T to, uint32_t tid, uint32_t &bad)
{
    for (T t = from + tid; t < to; t += 256u) bad += finite_f32(row[t]) ? 0u : 1u;
}

// ---- a row's chunks, read back by a totals kernel, one lane per row ----------------------------------------------------------
// the chunks that ran for a row of n samples and n_out outputs: none for no samples, chunk 0 whatever n_out
template <uint32_t CHUNK>
__device__ __forceinline__ uint64_t row_chunks(uint64_t n, uint64_t n_out)
{
    const uint64_t chunks = (n_out + CHUNK - 1u) / CHUNK;
    return n == 0 ? 0u : (chunks ? chunks : 1u);
}

__device__ __forceinline__ uint32_t sum_chunks(const uint32_t *cbad, uint64_t u, uint32_t grid_chunks, uint64_t chunks)
{
    uint32_t b = 0u;
    for (uint64_t c = 0; c < chunks; ++c) b += cbad[u * grid_chunks + c];
    return b;
}

// ---- a row's ring ---------------------------------------------------------------------------------------------------------
// Sample t of a row lies at t mod ring_cap (a power of two), +0.0 where it was not finite.  An advance kernel, the ring's only
// writer, keeps the call's last min(n, keep_max) samples, keep_max <= ring_cap: row holds the call's n, fed is N before it, or
// N's low 32 bits (N mod ring_cap is all that counts).
template <typename T>
__device__ __forceinline__ void ring_keep(const float *row, uint32_t n, T fed, float *hist, uint32_t ring_cap, uint32_t keep_max,
                                          uint32_t lane)
{
    const uint32_t keep = n < keep_max ? n : keep_max;
    for (uint32_t t = n - keep + lane; t < n; t += 64u) {
        const float x = row[t];
        hist[(fed + t) & (T)(ring_cap - 1u)] = finite_f32(x) ? x : 0.0f;
    }
}

}  // namespace grail
