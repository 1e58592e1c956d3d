// iir_kernels.hip — recursive filtering of rows (grail_iir_async) and of streams (grail_iir_stream_*).  The contract
// (include/grail_hip.h, "levels, continued: recursive filtering"): S biquads in transposed direct form II along each row,
// binary64, every operation rounded by itself, one rounding to binary32 at the end.  It is the K-weighting recurrence of
// loudness_kernels.hip with the caller's coefficients, per lane, and it writes samples: one lane per row, 64 rows per wave,
// tiles of 64 samples in through LDS and out through LDS the other way.  No atomics, every store a plain vector store.
// DESIGN.md §4.19 (rows), §4.20 (streams).
#include "kernels.h"
#include "iir_plan.h"
#include "loudness_common.h"
#include "row_kernel_common.h"

#include "../../include/grail_hip.h"

#pragma clang fp contract(off)

namespace grail {

using namespace loud;

namespace {

// loud_load of loudness_kernels.hip: wave-instruction i reads samples [t0, t0 + 64) of the rows 4i .. 4i + 3 of the wave,
// lane l the four samples from 4 (l mod 16) on of row 4i + l / 16: whole 256-byte pieces of rows.  A row past the launch's
// last reads the last row; a group of four past the row's stride reads the row's last group: every load lies inside
// rows[n_rows][row_stride] and none sits behind a per-lane branch.  What such a slot holds is no sample t < n of any row and
// never enters a filter.
template <bool VEC>
__device__ __forceinline__ void iir_load(const float *__restrict__ rows, uint64_t row_stride, uint32_t n_rows, uint64_t row0,
                                         uint64_t t0, uint32_t lane, float (&x)[LOUD_LOADS][4])
{
    const uint64_t col = t0 + 4u * (lane & 15u);
#pragma unroll
    for (uint32_t i = 0; i < LOUD_LOADS; ++i) {
        uint64_t r = row0 + 4u * i + (lane >> 4);
        r = r < n_rows ? r : n_rows - 1u;
        const float *src = rows + r * row_stride;
        if (VEC) {
            const uint64_t o = col < row_stride ? col : row_stride - 4u;        // (row_stride is a multiple of 4 and >= 4)
            const float4 v = *reinterpret_cast<const float4 *>(src + o);
            x[i][0] = v.x;
            x[i][1] = v.y;
            x[i][2] = v.z;
            x[i][3] = v.w;
        } else {
#pragma unroll
            for (uint32_t k = 0; k < 4; ++k) {
                const uint64_t o = col + k < row_stride ? col + k : row_stride - 1u;
                x[i][k] = src[o];
            }
        }
    }
}

// The way back: the tile holds the outputs [t0, t0 + 64) of the wave's rows where it held their samples, and leaves in the
// pieces it came in: lane l the four outputs from 4 (l mod 16) on of row 4i + l / 16.  row_out[r] is row r's n_out (0 for a
// row past the launch's last, a refused one and one the call writes nothing for): an output at or past it is not stored, so
// every store lies inside [0, n_out) of a row of the launch.
template <bool VEC>
__device__ __forceinline__ void iir_store(const float *tile, const uint32_t *row_out, float *__restrict__ out,
                                          uint64_t out_stride, uint64_t row0, uint64_t t0, uint32_t lane)
{
    const uint64_t col = t0 + 4u * (lane & 15u);
#pragma unroll
    for (uint32_t i = 0; i < LOUD_LOADS; ++i) {
        const uint32_t rl = 4u * i + (lane >> 4);
        const uint64_t n_out = row_out[rl];
        if (col >= n_out) continue;
        const float *src = tile + rl * LOUD_PITCH + 4u * (lane & 15u);
        float *dst = out + (row0 + rl) * out_stride + col;
        if (VEC && col + 4u <= n_out) {
            float4 v;
            v.x = src[0];
            v.y = src[1];
            v.z = src[2];
            v.w = src[3];
            *reinterpret_cast<float4 *>(dst) = v;
        } else {
#pragma unroll
            for (uint32_t k = 0; k < 4; ++k)
                if (col + k < n_out) dst[k] = src[k];
        }
    }
}

// One sample through the lane's sections, in the contract's order.  SB is the kernel's section bound, S <= SB the lane's own
// count: section j >= S is computed on whatever reaches it and its result dropped by the select, so v leaves as section
// S - 1 left it (a section is never run as an identity: 1*v + 0.0 would turn -0.0 into +0.0).  KEEP (streams): a lane past its
// own last step leaves its state as it is.
template <uint32_t SB, bool KEEP>
__device__ __forceinline__ float iir_sample(float xf, bool counted, bool live, uint32_t S, const double (&c)[SB][5],
                                            double (&s1)[SB], double (&s2)[SB], uint32_t &bad)
{
    const bool finite = finite_f32(xf);
    bad += (counted && !finite) ? 1u : 0u;
    double v = (counted && finite) ? (double)xf : 0.0;
#pragma unroll
    for (uint32_t j = 0; j < SB; ++j) {
        const double y = c[j][0] * v + s1[j];
        const double n1 = (c[j][1] * v - c[j][3] * y) + s2[j];
        const double n2 = c[j][2] * v - c[j][4] * y;
        s1[j] = (!KEEP || live) ? n1 : s1[j];
        s2[j] = (!KEEP || live) ? n2 : s2[j];
        v = (SB == 1u || j < S) ? y : v;
    }
    return (float)v;
}

// One wave = 64 rows, lane r = row row0 + r, from the rows' first sample to the wave's longest row's last step in tiles of 64.
// The next tile's loads are issued before the current tile is filtered and land in LDS after its outputs have left, so they
// are in flight for the whole of a tile's arithmetic.  A lane's outputs overwrite its own samples in the tile (same lane, same
// word), and the tile is stored as it was loaded.  STREAM: the state comes from HBM and goes back there.
// Registers are the compiler's to spend (measured against a build held to two waves a SIMD): up to four
// sections a lane that leaves room for two waves a SIMD all the same, with eight it is one.
template <uint32_t SB, bool VEC, bool STREAM>
__global__ __launch_bounds__(64) void iir_kernel(IirArgs a)
{
    __shared__ float tile[LOUD_ROWS * LOUD_PITCH];
    __shared__ uint32_t row_out[LOUD_ROWS];
    const uint32_t lane = threadIdx.x;
    const uint64_t row0 = (uint64_t)blockIdx.x * LOUD_ROWS;
    const uint64_t u = row0 + lane;
    const bool mine = u < a.n_rows;
    const bool finishing = STREAM && a.finishing != 0u;        // (uniform)
    uint64_t n = 0, n_out = 0, fed = 0;
    uint32_t f = 0;
    bool refused = false, takes = false;
    double s1[SB], s2[SB];
#pragma unroll
    for (uint32_t j = 0; j < SB; ++j) s1[j] = s2[j] = 0.0;
    uint64_t *const w = a.state + u * iir_stream_state_words(SB);      // (formed into an address that is used by streams only)
    if (mine) {
        f = a.filter ? a.filter[u] : 0u;
        if (STREAM) {
            const uint64_t w0 = w[0];
            const bool ended = stream_ended(w0);
            fed = stream_fed(w0);
            if (finishing) {
                takes = !ended && (!a.mark || a.mark[u]);
                n_out = takes && fed ? a.tail : 0u;
            } else {
                const uint64_t fedn = a.len[u] < a.row_stride ? a.len[u] : a.row_stride;
                refused = ended && fedn;
                takes = !ended;
                n = n_out = takes ? fedn : 0u;
            }
#pragma unroll
            for (uint32_t j = 0; j < SB; ++j) {
                s1[j] = __longlong_as_double((long long)w[1u + 2u * j]);
                s2[j] = __longlong_as_double((long long)w[2u + 2u * j]);
            }
        } else {
            refused = f >= a.n_filters;
            if (!refused) n = a.len[u] < a.row_stride ? a.len[u] : a.row_stride;   // (never past the row, whatever len holds)
            const uint64_t whole = n + a.tail;
            n_out = n ? (whole < a.out_stride ? whole : a.out_stride) : 0u;
        }
    }
    // the lane's filter (an index outside the set reads filter 0 and filters nothing)
    const uint32_t fc = f < a.n_filters ? f : 0u;
    const uint32_t S = a.sections[fc];
    double c[SB][5];
#pragma unroll
    for (uint32_t j = 0; j < SB; ++j)
#pragma unroll
        for (uint32_t k = 0; k < 5; ++k) c[j][k] = a.image[(uint64_t)fc * IIR_IMAGE_DOUBLES + 5u * j + k];
    // the lane's steps: to its last output, and to its last sample where out_stride cut the outputs short (the count goes on)
    const uint64_t steps = n > n_out ? n : n_out;
    row_out[lane] = (uint32_t)n_out;                    // (n_out < 2^32: the host has refused strides that allow more)
    uint64_t longest = steps;
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {
        const uint64_t o = (uint64_t)__shfl_xor((long long)longest, d, 64);
        longest = o > longest ? o : longest;
    }
    longest = ((uint64_t)__builtin_amdgcn_readfirstlane((uint32_t)(longest >> 32)) << 32) |
              __builtin_amdgcn_readfirstlane((uint32_t)longest);
    float *mine_lds = tile + lane * LOUD_PITCH;
    float x[LOUD_LOADS][4];
    uint32_t bad = 0;
    if (longest && !finishing) {
        iir_load<VEC>(a.rows, a.row_stride, a.n_rows, row0, 0, lane, x);
        loud_stash(tile, lane, x);
    }
    __syncthreads();
    for (uint64_t t0 = 0; t0 < longest; t0 += LOUD_T) {
        const bool more = !finishing && t0 + LOUD_T < longest;
        if (more) iir_load<VEC>(a.rows, a.row_stride, a.n_rows, row0, t0 + LOUD_T, lane, x);
        const uint32_t run = longest - t0 < LOUD_T ? (uint32_t)(longest - t0) : LOUD_T;       // of the longest row
        constexpr uint32_t UNROLL = 4u;
        uint32_t i = 0;
        for (; i + UNROLL <= run; i += UNROLL) {
#pragma unroll
            for (uint32_t q = 0; q < UNROLL; ++q) {
                const uint64_t t = t0 + i + q;
                mine_lds[i + q] = iir_sample<SB, STREAM>(mine_lds[i + q], t < n, t < steps, S, c, s1, s2, bad);
            }
        }
#pragma unroll 1
        for (; i < run; ++i) {
            const uint64_t t = t0 + i;
            mine_lds[i] = iir_sample<SB, STREAM>(mine_lds[i], t < n, t < steps, S, c, s1, s2, bad);
        }
        __syncthreads();                                // every lane's outputs are in the tile
        iir_store<VEC>(tile, row_out, a.out, a.out_stride, row0, t0, lane);
        __syncthreads();                                // ... and have left it
        if (more) loud_stash(tile, lane, x);
        __syncthreads();
    }
    if (!mine) return;
    if (STREAM && takes) {
#pragma unroll
        for (uint32_t j = 0; j < SB; ++j) {
            w[1u + 2u * j] = (uint64_t)__double_as_longlong(s1[j]);
            w[2u + 2u * j] = (uint64_t)__double_as_longlong(s2[j]);
        }
        w[0] = (fed + n) | (finishing ? STREAM_ENDED : 0ull);
    }
    if (a.out_len) a.out_len[u] = refused ? GRAIL_LIMIT_REFUSED : (uint32_t)n_out;
    if (a.nonfinite) a.nonfinite[u] = bad;
}

template <uint32_t SB, bool STREAM>
void iir_launch_vec(const IirArgs &a, bool vec, uint32_t groups, hipStream_t stream)
{
    if (vec)
        hipLaunchKernelGGL((iir_kernel<SB, true, STREAM>), dim3(groups), dim3(64), 0, stream, a);
    else
        hipLaunchKernelGGL((iir_kernel<SB, false, STREAM>), dim3(groups), dim3(64), 0, stream, a);
}

template <bool STREAM>
void iir_launch_bound(const IirArgs &a, uint32_t bound, bool vec, uint32_t groups, hipStream_t stream)
{
    if (bound <= 1u)
        iir_launch_vec<1, STREAM>(a, vec, groups, stream);
    else if (bound == 2u)
        iir_launch_vec<2, STREAM>(a, vec, groups, stream);
    else if (bound <= 4u)
        iir_launch_vec<4, STREAM>(a, vec, groups, stream);
    else
        iir_launch_vec<8, STREAM>(a, vec, groups, stream);
}

}  // namespace

hipError_t launch_iir(const IirArgs &args, uint32_t bound, hipStream_t stream)
{
    if (args.n_rows == 0) return hipSuccess;
    const uint32_t groups = (args.n_rows + LOUD_ROWS - 1u) / LOUD_ROWS;
    const bool vec = aligned16(args.rows, args.row_stride, args.out, args.out_stride);
    if (args.state)
        iir_launch_bound<true>(args, bound, vec, groups, stream);
    else
        iir_launch_bound<false>(args, bound, vec, groups, stream);
    return hipGetLastError();
}

}  // namespace grail
