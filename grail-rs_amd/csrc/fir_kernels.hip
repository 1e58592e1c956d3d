// fir_kernels.hip — FIR filtering of finished rows with the caller's own taps (grail_fir_async).  The contract
// (include/grail_hip.h, "levels, continued: FIR filtering"): output m of a row is the left fold acc = acc + (double)h[k] *
// v[m + o - k] over ascending k from +0.0 in binary64, rounded once to binary32.  Every product is exact (24 bits times
// 24), so acc = fma(h[k], v, acc) is the contract's multiply and add.  Time is parallel: one workgroup of four waves per
// (row, chunk of FIR_CHUNK outputs).  A plain convolution has the same coefficient in every lane and lets a lane own
// CONSECUTIVE outputs: a lane keeps eight accumulators and a window of the samples they meet in registers, so a tap step
// brings ONE new sample from LDS and issues EIGHT multiply-adds (the resampler reads LDS once per multiply-add: §4.13).
// No atomics, every store a plain vector store.  DESIGN.md §4.14.  The second half of the file is the same filter on rows fed
// chunk by chunk (grail_filter_stream_*, §4.15): the same loop over a stretch staged from a row's ring and the call's chunk.
// The bookkeeping of a chunk, the counts, the state word and the ring are row_kernel_common.h's (§4.21).
#include "kernels.h"
#include "row_kernel_common.h"

namespace grail {

namespace {

constexpr uint32_t FIR_THREADS = 256;
constexpr uint32_t FIR_OWN = FIR_CHUNK / FIR_THREADS;           // consecutive outputs per lane
static_assert(FIR_OWN == 8, "the tap loop is written for eight outputs per lane and blocks of eight taps");
constexpr uint32_t FIR_TAPS_PADDED_MAX = 4096;                  // GRAIL_FIR_TAPS_MAX, a multiple of 8
// The stretch of a chunk: FIR_CHUNK + Kp - 1 samples (Kp: the taps padded to a multiple of 8), at most 6143, in groups of
// eight.  Sample s of the stretch lies at word (s mod 8) * FIR_PITCH + s div 8: lane L reads "sample 8 (L + g) + r" for a
// wave-uniform g and r, which in the plain layout is eight words from its neighbour's, an eight-way conflict on the 32
// banks that a 4-byte read sees; here the 64 lanes of a wave read 64 consecutive words, free of conflicts, and r is a
// constant offset in the instruction.  The staging writes sample 4 i + e from lane i: neighbouring lanes alternate
// between rows r and r + 4 of the image, and 4 * FIR_PITCH = 16 mod 32 puts those on opposite halves of the banks.
constexpr uint32_t FIR_GROUPS = (FIR_CHUNK + FIR_TAPS_PADDED_MAX) / 8;      // 768: groups of a stretch (6143 samples)
constexpr uint32_t FIR_PITCH = FIR_GROUPS + 4;                              // 772
static_assert((4u * FIR_PITCH) % 32u == 16u, "rows r and r + 4 of the image on opposite halves of the banks");

// the filter of row u, or false: an index outside the set (the row is refused: nothing of it is touched)
struct FirFilter {
    uint32_t first, padded, taps, origin;
};
__device__ __forceinline__ bool fir_filter(const uint32_t *__restrict__ filter, const uint32_t *__restrict__ desc, uint32_t n_filters,
                                           uint64_t u, FirFilter &f)
{
    const uint32_t i = filter ? filter[u] : 0u;
    if (i >= n_filters) return false;
    const uint4 d = *reinterpret_cast<const uint4 *>(desc + 4u * i);
    f.first = d.x, f.padded = d.y, f.taps = d.z, f.origin = d.w;
    return true;
}

// n = min(len, row_stride) and n_out = min(n + K - 1 - o, out_stride), 0 for n = 0 (n < 2^32, K <= 2^12: no overflow)
__device__ __forceinline__ void fir_row(const uint32_t *__restrict__ len, uint64_t row_stride, uint64_t out_stride, uint64_t u,
                                        const FirFilter &f, uint64_t &n, uint64_t &n_out)
{
    n = len[u] < row_stride ? len[u] : row_stride;
    const uint64_t full = n ? n + (f.taps - 1u - f.origin) : 0u;
    n_out = full < out_stride ? full : out_stride;
}

// Eight taps h[0 .. 7] of a block against the lane's window.  Tap i meets, for the lane's output j, sample 7 + j - i of the
// fifteen that start at the block's group: 0 .. 7 are that group (fresh: eight LDS reads), 8 .. 14 the first seven of the
// group after it, which the block before brought in.  The caller swaps the two arrays from block to block, so the window
// moves by the names of the registers, not by copies.
__device__ __forceinline__ void fir_block(const float *__restrict__ at, const double *__restrict__ h, double (&fresh)[8],
                                          const double (&kept)[8], double (&acc)[8])
{
#pragma unroll
    for (uint32_t r = 0; r < 8; ++r) fresh[r] = (double)at[r * FIR_PITCH];
#pragma unroll
    for (uint32_t i = 0; i < 8; ++i) {
        const double c = h[i];
#pragma unroll
        for (uint32_t j = 0; j < 8; ++j) {
            const uint32_t x = 7u + j - i;
            acc[j] = __builtin_fma(c, x < 8u ? fresh[x] : kept[x - 8u], acc[j]);
        }
    }
}

// The eight outputs of lane `tid` from the stretch in LDS, stored at `to` (output 8 tid of the chunk); h: the filter's padded
// taps, Kp of them, behind a wave-uniform address.  fir_kernel and fir_stream_kernel share it: what differs between them is
// where the stretch came from.
template <bool VEC>
__device__ __forceinline__ void fir_outputs(const float *__restrict__ stage, uint32_t tid, uint32_t count, const double *__restrict__ h,
                                            uint32_t Kp, float *__restrict__ to)
{
    const uint32_t blocks = Kp >> 3;
    // block b (taps 8 b .. 8 b + 7) starts at group lane + blocks - 1 - b of the stretch
    const float *at = stage + tid + blocks;
    double a[8], b[8], acc[8];
#pragma unroll
    for (uint32_t r = 0; r < 8; ++r) acc[r] = 0.0, a[r] = 0.0;
#pragma unroll
    for (uint32_t r = 0; r < 7; ++r) b[r] = (double)at[r * FIR_PITCH];     // samples 8 .. 14 of block 0's window
    b[7] = 0.0;
    uint32_t k = 0;
    for (; k + 2u <= blocks; k += 2u) {
        fir_block(at - 1, h, a, b, acc);
        fir_block(at - 2, h + 8, b, a, acc);
        at -= 2, h += 16;
    }
    if (k < blocks) fir_block(at - 1, h, a, b, acc);

    // eight consecutive outputs per lane; a row's last partial group goes out in 4-byte stores
    if (VEC && 8u * tid + 8u <= count) {
        reinterpret_cast<float4 *>(to)[0] = make_float4((float)acc[0], (float)acc[1], (float)acc[2], (float)acc[3]);
        reinterpret_cast<float4 *>(to)[1] = make_float4((float)acc[4], (float)acc[5], (float)acc[6], (float)acc[7]);
    } else {
#pragma unroll
        for (uint32_t e = 0; e < 8; ++e)
            if (8u * tid + e < count) to[e] = (float)acc[e];
    }
}

// One workgroup = one (row, chunk of FIR_CHUNK outputs).  VEC: 16-byte loads and stores (both bases 16-byte aligned, both
// strides multiples of 4), else 4-byte ones: same bits.  The chunk's stretch (the samples its outputs' taps reach) goes to
// LDS once, zeroed where it lies outside the row or is not finite.  Chunk c counts the non-finite samples among inputs
// [c FIR_CHUNK, (c + 1) FIR_CHUNK), the row's last chunk to the row's end.
template <bool VEC>
__global__ __launch_bounds__(256) void fir_kernel(const float *__restrict__ rows, uint64_t row_stride, const uint32_t *__restrict__ len,
                                                  uint32_t n_rows, const uint32_t *__restrict__ filter, const double *__restrict__ taps,
                                                  const uint32_t *__restrict__ desc, uint32_t n_filters, uint32_t grid_chunks,
                                                  float *__restrict__ out, uint64_t out_stride, uint32_t *__restrict__ cbad)
{
    __shared__ float stage[8 * FIR_PITCH];
    __shared__ uint32_t red[FIR_THREADS / 64];
    const uint32_t tid = threadIdx.x;
    uint64_t u;
    uint32_t c;
    chunk_of_block(grid_chunks, u, c);
    if (u >= n_rows) return;
    FirFilter f;
    if (!fir_filter(filter, desc, n_filters, u, f)) return;
    uint64_t n, n_out;
    fir_row(len, row_stride, out_stride, u, f, n, n_out);
    const uint64_t m0 = (uint64_t)c * FIR_CHUNK;
    // a row of no samples has no chunk; chunk 0 of any other runs even with no output to write: it counts
    if (n == 0 || chunk_idle(m0, n_out, c)) return;
    bool last;
    uint32_t count;
    chunk_extent<FIR_CHUNK>(m0, n_out, last, count);
    const float *row = rows + u * row_stride;
    const uint32_t Kp = (uint32_t)__builtin_amdgcn_readfirstlane((int)f.padded);
    const int64_t t_hi = (int64_t)n - 1;
    // the input samples this chunk counts non-finite ones in
    int64_t own_lo, own_hi;
    chunk_owned<FIR_CHUNK>(m0, n, last, own_lo, own_hi);
    // the stretch: sample s of it is input time s_base + s; output m0 + r meets, at tap k, sample r + Kp - 1 - k.  The
    // lanes with an output to compute (each owns eight) reach samples 0 .. 8 lanes + Kp - 2.
    const uint32_t lanes = (count + 7u) >> 3;
    const int64_t s_base = (int64_t)m0 + (int64_t)f.origin - (int64_t)(Kp - 1u);
    const int64_t s_need = count ? (int64_t)(8u * lanes + Kp - 1u) : 0;
    uint32_t bad = 0u;
    int64_t counted_to = own_lo;            // what the staging has counted of [own_lo, own_hi)
    if (count) {
        // whole groups of 4 input samples, the first at a multiple of 4 at or below s_base (which may be negative)
        const int64_t g_first = s_base >> 2;
        const uint32_t groups = (uint32_t)(((s_base + s_need + 3) >> 2) - g_first);
        const int64_t g_hi = t_hi >> 2;
        for (uint32_t gi = tid; gi < groups; gi += FIR_THREADS) {
            const int64_t t0 = 4 * (g_first + (int64_t)gi);
            float x[4];
            if (VEC) {
                // the row's last group starts below n <= row_stride, a multiple of 4: inside the row
                int64_t g = g_first + (int64_t)gi;
                g = g < 0 ? 0 : g;
                g = g > g_hi ? g_hi : g;
                const float4 v = *reinterpret_cast<const float4 *>(row + 4 * g);
                x[0] = v.x, x[1] = v.y, x[2] = v.z, x[3] = v.w;
            } else {
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    int64_t t = t0 + e;
                    t = t < 0 ? 0 : t;
                    t = t > t_hi ? t_hi : t;
                    x[e] = row[t];
                }
            }
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int64_t t = t0 + e;
                const bool inside = t >= 0 && t <= t_hi;            // (what a clamped load brought is outside)
                const bool finite = finite_f32(x[e]);
                bad += (inside && !finite && t >= own_lo && t < own_hi) ? 1u : 0u;
                const int64_t s = t - s_base;
                if (s >= 0 && s < s_need) stage[((uint32_t)s & 7u) * FIR_PITCH + ((uint32_t)s >> 3)] = (inside && finite) ? x[e] : 0.0f;
            }
        }
        counted_to = 4 * (g_first + (int64_t)groups);
        counted_to = counted_to < own_lo ? own_lo : counted_to;
    }
    // what the chunk owns past its stretch (an out_stride or an origin that ends the outputs before the samples leaves
    // the last chunk the rest of the row): counted from the row itself
    count_owned_tail(row, counted_to, own_hi, tid, bad);
    __syncthreads();

    if (tid < lanes) {
        // the coefficient is the same in every lane: the taps are read through a wave-uniform address (scalar loads)
        const double *h = taps + (uint32_t)__builtin_amdgcn_readfirstlane((int)f.first);
        fir_outputs<VEC>(stage, tid, count, h, Kp, out + u * out_stride + m0 + 8u * tid);
    }
    block_count_store(bad, red, tid, cbad, u, grid_chunks, c);
}

// A row's numbers from its chunks, one lane per row; a row whose filter is outside the set is refused here.
__global__ __launch_bounds__(256) void fir_totals_kernel(const uint32_t *__restrict__ len, uint64_t row_stride, uint32_t n_rows,
                                                         const uint32_t *__restrict__ filter, const uint32_t *__restrict__ desc,
                                                         uint32_t n_filters, uint64_t out_stride, const uint32_t *__restrict__ cbad,
                                                         uint32_t grid_chunks, uint32_t *__restrict__ out_len,
                                                         uint32_t *__restrict__ nonfinite)
{
    const uint64_t u = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (u >= n_rows) return;
    FirFilter f;
    if (!fir_filter(filter, desc, n_filters, u, f)) {
        refuse_counts(out_len, nonfinite, u);
        return;
    }
    uint64_t n, n_out;
    fir_row(len, row_stride, out_stride, u, f, n, n_out);
    const uint32_t b = sum_chunks(cbad, u, grid_chunks, row_chunks<FIR_CHUNK>(n, n_out));
    if (out_len) out_len[u] = (uint32_t)n_out;
    if (nonfinite) nonfinite[u] = b;
}

// ---- streams (grail_filter_stream_*): rows fed chunk by chunk, DESIGN.md §4.15 ----------------------------------------------
// A row's state is the state word of row_kernel_common.h and nothing else; its ring (there too) holds at least the set's
// longest K - 1 samples.  In the frame of one call, local time = global time - N: the call's output r is the left fold of
// h[k] * v[r + d - k] with d = max(0, o - N); v is the ring below 0 (+0.0 before the row's first sample), the call's
// n samples from 0, +0.0 from n on (which only a finishing call reaches: its n is 0).
struct FirStreamRow {
    uint64_t fed;           // N
    uint32_t n, count, d;   // the samples this call feeds, the outputs it writes, the origin in its frame
    bool takes, refused;    // the call changes the row's state; the row has ended and is fed
};
__device__ __forceinline__ FirStreamRow fir_stream_row(const uint64_t *__restrict__ state, const uint32_t *__restrict__ in_len,
                                                       uint64_t in_stride, const uint8_t *__restrict__ mark, bool finishing, uint64_t u,
                                                       const FirFilter &f)
{
    FirStreamRow r;
    const uint64_t w = state[u];
    const bool ended = stream_ended(w);
    r.fed = stream_fed(w);
    r.d = r.fed < f.origin ? f.origin - (uint32_t)r.fed : 0u;
    if (finishing) {
        r.n = 0u;
        r.refused = false;
        r.takes = !ended && (!mark || mark[u]);
        // the tail: outputs E(N) .. N + K - 1 - o - 1, none for a row that was fed nothing
        r.count = r.takes && r.fed ? f.taps - 1u - f.origin + (r.fed < f.origin ? (uint32_t)r.fed : f.origin) : 0u;
    } else {
        r.n = in_len[u] < in_stride ? in_len[u] : (uint32_t)in_stride;
        r.refused = ended && r.n;
        r.takes = !ended;
        // E(N + n) - E(N) with E(N) = max(0, N - o): at most n
        const uint64_t to = r.fed + r.n;
        r.count = ended ? 0u : (uint32_t)((to > f.origin ? to - f.origin : 0u) - (r.fed > f.origin ? r.fed - f.origin : 0u));
    }
    return r;
}

// fir_kernel with the row's state in place of the filter's origin and the row's length: one workgroup = one (row, chunk of
// FIR_CHUNK of this call's outputs).  Reads the state and the ring, writes neither (fir_stream_advance_kernel, queued
// behind it, is their only writer).  Chunk c counts the non-finite samples among this call's inputs [c FIR_CHUNK, (c + 1)
// FIR_CHUNK), the last chunk to the end of them.
template <bool VEC>
__global__ __launch_bounds__(256) void fir_stream_kernel(const float *__restrict__ in, uint64_t in_stride, const uint32_t *__restrict__ in_len,
                                                         uint32_t n_rows, const uint32_t *__restrict__ filter, const double *__restrict__ taps,
                                                         const uint32_t *__restrict__ desc, uint32_t n_filters,
                                                         const uint64_t *__restrict__ state, const float *__restrict__ ring, uint32_t ring_cap,
                                                         const uint8_t *__restrict__ mark, uint32_t finishing, uint32_t grid_chunks,
                                                         float *__restrict__ out, uint64_t out_stride, uint32_t *__restrict__ cbad)
{
    __shared__ float stage[8 * FIR_PITCH];
    __shared__ uint32_t red[FIR_THREADS / 64];
    const uint32_t tid = threadIdx.x;
    uint64_t u;
    uint32_t c;
    chunk_of_block(grid_chunks, u, c);
    if (u >= n_rows) return;
    FirFilter f;
    if (!fir_filter(filter, desc, n_filters, u, f)) return;         // (the indices were checked when the stream was opened)
    const FirStreamRow r = fir_stream_row(state, in_len, in_stride, mark, finishing != 0u, u, f);
    const uint64_t n = r.n, n_out = r.count;
    const uint64_t m0 = (uint64_t)c * FIR_CHUNK;
    // a refused row and one with neither samples nor outputs have no chunk; chunk 0 of any other runs even with no output
    // to write: it counts
    if (r.refused || (n == 0 && n_out == 0) || chunk_idle(m0, n_out, c)) return;
    bool last;
    uint32_t count;
    chunk_extent<FIR_CHUNK>(m0, n_out, last, count);
    const float *row = in + u * in_stride;                          // (not read when n = 0)
    const float *hist = ring + u * ring_cap;
    const uint64_t ring_mask = ring_cap - 1u;
    const uint32_t Kp = (uint32_t)__builtin_amdgcn_readfirstlane((int)f.padded);
    const int64_t t_hi = (int64_t)n - 1;
    const int64_t t_lo = -(int64_t)(f.taps - 1u < r.fed ? f.taps - 1u : r.fed);   // how far back the taps and the row reach
    int64_t own_lo, own_hi;
    chunk_owned<FIR_CHUNK>(m0, n, last, own_lo, own_hi);
    // the stretch: sample s of it is local time s_base + s; output m0 + j meets, at tap k, sample j + Kp - 1 - k
    const uint32_t lanes = (count + 7u) >> 3;
    const int64_t s_base = (int64_t)m0 + (int64_t)r.d - (int64_t)(Kp - 1u);
    const int64_t s_need = count ? (int64_t)(8u * lanes + Kp - 1u) : 0;
    uint32_t bad = 0u;
    int64_t counted_to = own_lo;
    if (count) {
        const int64_t g_first = s_base >> 2;
        const uint32_t groups = (uint32_t)(((s_base + s_need + 3) >> 2) - g_first);
        const int64_t g_hi = t_hi >> 2;
        for (uint32_t gi = tid; gi < groups; gi += FIR_THREADS) {
            const int64_t t0 = 4 * (g_first + (int64_t)gi);
            float x[4] = {0.0f, 0.0f, 0.0f, 0.0f};
            if (t0 + 3 >= 0 && t0 <= t_hi) {                        // the group holds samples of this call
                if (VEC) {
                    // the call's last group starts below n <= in_stride, a multiple of 4: inside the row
                    int64_t g = g_first + (int64_t)gi;
                    g = g < 0 ? 0 : g;
                    g = g > g_hi ? g_hi : g;
                    const float4 v = *reinterpret_cast<const float4 *>(row + 4 * g);
                    x[0] = v.x, x[1] = v.y, x[2] = v.z, x[3] = v.w;
                } else {
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        int64_t t = t0 + e;
                        t = t < 0 ? 0 : t;
                        t = t > t_hi ? t_hi : t;
                        x[e] = row[t];
                    }
                }
            }
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int64_t t = t0 + e;
                float v = 0.0f;
                if (t < 0) {
                    // the ring holds the last ring_cap >= K - 1 samples fed, already +0.0 where they were not finite
                    if (t >= t_lo) v = hist[(r.fed + (uint64_t)t) & ring_mask];
                } else if (t <= t_hi) {
                    const bool finite = finite_f32(x[e]);
                    bad += (!finite && t >= own_lo && t < own_hi) ? 1u : 0u;
                    v = finite ? x[e] : 0.0f;
                }
                const int64_t s = t - s_base;
                if (s >= 0 && s < s_need) stage[((uint32_t)s & 7u) * FIR_PITCH + ((uint32_t)s >> 3)] = v;
            }
        }
        counted_to = 4 * (g_first + (int64_t)groups);
        counted_to = counted_to < own_lo ? own_lo : counted_to;
    }
    // what the chunk owns past its stretch (a row still short of its origin writes fewer outputs than it is fed)
    count_owned_tail(row, counted_to, own_hi, tid, bad);
    __syncthreads();

    if (tid < lanes) {
        const double *h = taps + (uint32_t)__builtin_amdgcn_readfirstlane((int)f.first);
        fir_outputs<VEC>(stage, tid, count, h, Kp, out + u * out_stride + m0 + 8u * tid);
    }
    block_count_store(bad, red, tid, cbad, u, grid_chunks, c);
}

// Behind fir_stream_kernel on the stream, one wave per row, the only writer of a stream's state: the row's numbers from its
// chunks, the call's last samples into the ring (ring_keep), then N + n (a finishing call: the row ended).  A row that has
// ended and is fed is refused (refuse_counts), its state as it was.
__global__ __launch_bounds__(256) void fir_stream_advance_kernel(const float *__restrict__ in, uint64_t in_stride,
                                                                 const uint32_t *__restrict__ in_len, uint32_t n_rows,
                                                                 const uint32_t *__restrict__ filter, const uint32_t *__restrict__ desc,
                                                                 uint32_t n_filters, uint64_t *__restrict__ state, float *__restrict__ ring,
                                                                 uint32_t ring_cap, const uint8_t *__restrict__ mark, uint32_t finishing,
                                                                 const uint32_t *__restrict__ cbad, uint32_t grid_chunks,
                                                                 uint32_t *__restrict__ out_len, uint32_t *__restrict__ nonfinite)
{
    const uint64_t u = (uint64_t)blockIdx.x * (FIR_THREADS / 64u) + (threadIdx.x >> 6);
    const uint32_t lane = threadIdx.x & 63u;
    if (u >= n_rows) return;
    FirFilter f;
    if (!fir_filter(filter, desc, n_filters, u, f)) return;
    const FirStreamRow r = fir_stream_row(state, in_len, in_stride, mark, finishing != 0u, u, f);
    if (r.refused) {
        if (lane == 0u) refuse_counts(out_len, nonfinite, u);
        return;
    }
    uint32_t bad = 0u;
    if (r.takes && r.n) {
        const uint32_t chunks = r.count ? (r.count + FIR_CHUNK - 1u) / FIR_CHUNK : 1u;
        for (uint32_t c = lane; c < chunks; c += 64u) bad += cbad[u * grid_chunks + c];
        ring_keep(in + u * in_stride, r.n, r.fed, ring + u * ring_cap, ring_cap, ring_cap, lane);
    }
    bad = wave_sum(bad);
    if (lane != 0u) return;
    if (out_len) out_len[u] = r.count;
    if (nonfinite) nonfinite[u] = bad;
    if (r.takes) state[u] = finishing ? (r.fed | STREAM_ENDED) : r.fed + r.n;
}

}  // namespace

uint64_t fir_grid_chunks(uint64_t row_stride, uint64_t out_stride, uint32_t tail_max)
{
    if (row_stride == 0) return 0;
    // (a row holds fewer than 2^32 samples: len is 32 bits wide)
    const uint64_t full = (row_stride < 0xFFFFFFFFull ? row_stride : 0xFFFFFFFFull) + tail_max;
    const uint64_t longest = full < out_stride ? full : out_stride;
    const uint64_t chunks = (longest + FIR_CHUNK - 1u) / FIR_CHUNK;
    return chunks ? chunks : 1u;
}

hipError_t launch_fir(const FirArgs &a, hipStream_t stream)
{
    const uint64_t workgroups = (uint64_t)a.n_rows * a.grid_chunks;
    hipError_t e;
    if (!grid_fits(workgroups, &e)) return e;
    launch_either(aligned16(a.rows, a.row_stride, a.out, a.out_stride), fir_kernel<true>, fir_kernel<false>, dim3((uint32_t)workgroups),
                  dim3(FIR_THREADS), 0, stream, a.rows, a.row_stride, a.len, a.n_rows, a.filter, a.taps, a.desc, a.n_filters, a.grid_chunks,
                  a.out, a.out_stride, a.cbad);
    return hipGetLastError();
}

hipError_t launch_fir_totals(const FirArgs &a, hipStream_t stream)
{
    if (a.n_rows == 0) return hipSuccess;
    hipLaunchKernelGGL(fir_totals_kernel, dim3((a.n_rows + 255u) / 256u), dim3(256), 0, stream, a.len, a.row_stride, a.n_rows, a.filter,
                       a.desc, a.n_filters, a.out_stride, a.cbad, a.grid_chunks, a.out_len, a.nonfinite);
    return hipGetLastError();
}

hipError_t launch_fir_stream(const FirArgs &a, hipStream_t stream)
{
    const uint64_t workgroups = (uint64_t)a.n_rows * a.grid_chunks;
    hipError_t e;
    if (!grid_fits(workgroups, &e)) return e;
    launch_either(aligned16(a.rows, a.row_stride, a.out, a.out_stride), fir_stream_kernel<true>, fir_stream_kernel<false>,
                  dim3((uint32_t)workgroups), dim3(FIR_THREADS), 0, stream, a.rows, a.row_stride, a.len, a.n_rows, a.filter, a.taps,
                  a.desc, a.n_filters, a.state, a.ring, a.ring_cap, a.mark, a.finishing ? 1u : 0u, a.grid_chunks, a.out, a.out_stride,
                  a.cbad);
    return hipGetLastError();
}

hipError_t launch_fir_stream_advance(const FirArgs &a, hipStream_t stream)
{
    if (a.n_rows == 0) return hipSuccess;
    const uint32_t rows_per_group = FIR_THREADS / 64u;
    hipLaunchKernelGGL(fir_stream_advance_kernel, dim3(a.n_rows / rows_per_group + (a.n_rows % rows_per_group != 0u)), dim3(FIR_THREADS), 0,
                       stream, a.rows, a.row_stride, a.len, a.n_rows, a.filter, a.desc, a.n_filters, a.state, a.ring, a.ring_cap, a.mark,
                       a.finishing ? 1u : 0u, a.cbad, a.grid_chunks, a.out_len, a.nonfinite);
    return hipGetLastError();
}

}  // namespace grail
