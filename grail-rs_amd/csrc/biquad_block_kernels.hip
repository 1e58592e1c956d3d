// biquad_block_kernels.hip — recursive filtering of rows, parallel in time (grail_biquad_blocked_async).  The contract
// (include/grail_hip.h, "levels, continued: recursive filtering, parallel in time"): a row's steps in blocks of B = 1024; the
// rest pass runs every block but the row's last from rest (z_k), the propagate carries the entry states from block to block
// through the filter's block matrix T (e_{k+1} = T e_k + z_k in the contract's order: the call's one serial chain), and the
// output pass runs every block again from its entry state and writes its outputs.  One lane per (row, block), 64 consecutive
// blocks of one row per workgroup of one wave: a block is to biquad_block_kernel what a row is to iir_kernel (iir_kernels.hip),
// tiles of 64 samples in through LDS and out through LDS the other way.  No atomics, every store a plain vector store.
// DESIGN.md §4.22.
#include "kernels.h"
#include "iir_plan.h"
#include "loudness_common.h"
#include "row_kernel_common.h"

#include "../../include/grail_hip.h"

#pragma clang fp contract(off)

namespace grail {

using namespace loud;

namespace {

static_assert(IIR_BLOCK_LANES == LOUD_ROWS && IIR_BLOCK % LOUD_T == 0, "a workgroup's blocks are the rows of a tile");

// what the call makes of row u, as grail_iir_async does: n samples, n_out outputs, steps = the later of the two ends, and
// the blocks that cover the steps.  A row whose filter index is outside the set has none of any (and reads filter 0).
struct BlockRow {
    uint64_t n, n_out, steps, blocks;
    uint32_t fc;
    bool refused;
};
__device__ __forceinline__ BlockRow block_row(const BiquadBlockArgs &a, uint64_t u)
{
    BlockRow r;
    const uint32_t f = a.filter ? a.filter[u] : 0u;
    r.refused = f >= a.n_filters;
    r.fc = r.refused ? 0u : f;
    r.n = 0;
    if (!r.refused) r.n = a.len[u] < a.row_stride ? a.len[u] : a.row_stride;      // (never past the row, whatever len holds)
    const uint64_t whole = r.n + a.tail;
    r.n_out = r.n ? (whole < a.out_stride ? whole : a.out_stride) : 0u;
    r.steps = r.n > r.n_out ? r.n : r.n_out;
    r.blocks = (r.steps + IIR_BLOCK - 1u) / IIR_BLOCK;          // (at most grid_blocks: steps <= min(row_stride, 2^32 - 1) + tail)
    return r;
}

// A workgroup's samples and outputs are addressed from its first step, k0 B, in 32 bits: its 64 blocks span 65 536 steps.
// What it may touch of the row ends `limit` steps from there (0 when the row ends before the workgroup's first step: its
// blocks lie in the tail), a row's end being anything up to 2^60.
__device__ __forceinline__ uint32_t steps_from(uint64_t from, uint64_t end)
{
    const uint64_t left = end > from ? end - from : 0u;
    return left < 0xFFFFFFFFull ? (uint32_t)left : 0xFFFFFFFFu;
}

// iir_load of iir_kernels.hip with the blocks of one row for rows: wave-instruction i reads the steps [t0, t0 + 64) of the
// blocks k0 + 4i .. k0 + 4i + 3, lane l the four samples from 4 (l mod 16) on of block k0 + 4i + l / 16: whole 256-byte pieces
// of the row.  piece = (l / 16) B + 4 (l mod 16): the lane's place in instruction 0 at t0 = 0, from the workgroup's first
// step.  from: the row at that step, or at its last group (sample) of four where the row_stride ends before it; last: the
// row's last group (sample) from there.  A load past the stride reads that last one: every load lies inside the row's
// row_stride samples (row_stride > 0: a row of no samples has no blocks and its workgroups have left), and none sits
// behind a per-lane branch.  What such a slot holds is no sample t < n and never enters a filter.
template <bool VEC>
__device__ __forceinline__ void block_load(const float *__restrict__ from, uint32_t last, uint32_t piece, uint32_t t0,
                                           float (&x)[LOUD_LOADS][4])
{
#pragma unroll
    for (uint32_t i = 0; i < LOUD_LOADS; ++i) {
        const uint32_t col = piece + 4u * i * IIR_BLOCK + t0;
        if (VEC) {
            const uint32_t o = col < last ? col : last;         // (row_stride is a multiple of 4 and >= 4, and so is col)
            const float4 v = *reinterpret_cast<const float4 *>(from + o);
            x[i][0] = v.x;
            x[i][1] = v.y;
            x[i][2] = v.z;
            x[i][3] = v.w;
        } else {
#pragma unroll
            for (uint32_t k = 0; k < 4; ++k) {
                const uint32_t o = col + k < last ? col + k : last;
                x[i][k] = from[o];
            }
        }
    }
}

// The way back, iir_store's: the tile holds the outputs [t0, t0 + 64) of the workgroup's blocks where it held their samples.
// to: the out row at the workgroup's first step; outs: the row's n_out from there.  An output at or past it is not stored, so
// every store lies inside [0, n_out) of the row; an output below it was computed (its block is lane 0's or a later one, and
// then lane 0's block is whole).
template <bool VEC>
__device__ __forceinline__ void block_store(const float *tile, uint32_t outs, float *__restrict__ to, uint32_t piece, uint32_t t0,
                                            uint32_t lane)
{
#pragma unroll
    for (uint32_t i = 0; i < LOUD_LOADS; ++i) {
        const uint32_t rl = 4u * i + (lane >> 4);
        const uint32_t col = piece + 4u * i * IIR_BLOCK + t0;
        if (col >= outs) continue;
        const float *src = tile + rl * LOUD_PITCH + 4u * (lane & 15u);
        float *dst = to + col;
        if (VEC && col + 4u <= outs) {
            float4 v;
            v.x = src[0];
            v.y = src[1];
            v.z = src[2];
            v.w = src[3];
            *reinterpret_cast<float4 *>(dst) = v;
        } else {
#pragma unroll
            for (uint32_t k = 0; k < 4; ++k)
                if (col + k < outs) dst[k] = src[k];
        }
    }
}

// One sample through the lane's sections, in the contract's order: iir_sample of iir_kernels.hip without its streams' KEEP,
// a copy kept on purpose (iir_kernels.hip stays as it is, text and registers).  Section j >= S is computed
// on whatever reaches it and its result dropped by the select; a section is never run as an identity.
template <uint32_t SB>
__device__ __forceinline__ float biquad_sample(float xf, bool counted, uint32_t S, const double (&c)[SB][5], double (&s1)[SB],
                                               double (&s2)[SB], uint32_t &bad)
{
    const bool finite = finite_f32(xf);
    bad += (counted && !finite) ? 1u : 0u;
    double v = (counted && finite) ? (double)xf : 0.0;
#pragma unroll
    for (uint32_t j = 0; j < SB; ++j) {
        const double y = c[j][0] * v + s1[j];
        const double n1 = (c[j][1] * v - c[j][3] * y) + s2[j];
        const double n2 = c[j][2] * v - c[j][4] * y;
        s1[j] = n1;
        s2[j] = n2;
        v = (SB == 1u || j < S) ? y : v;
    }
    return (float)v;
}

// One wave = 64 consecutive blocks of row u, lane l = block k0 + l, over the block's steps in tiles of 64.  The next tile's
// loads are issued before the current tile is filtered and land in LDS after its outputs have left.
// OUT = false, the rest pass: from rest, nothing stored but the 2 SB end states z_k, the row's last block skipped (nobody
// enters a block after it).  OUT = true, the output pass: from the entry state (+0.0 for block 0, slot k - 1 for block k),
// the outputs through the tile; this pass reads every sample below n and so is the one that counts.
// A lane whose block lies past the pass's last computes on +0.0 and clamped loads and stores nothing; a workgroup of such
// lanes only leaves at once.  The trip count is lane 0's block's: the steps left from its first, B at the most.
template <uint32_t SB, bool VEC, bool OUT>
__global__ __launch_bounds__(64) void biquad_block_kernel(BiquadBlockArgs a)
{
    __shared__ float tile[LOUD_ROWS * LOUD_PITCH];
    const uint32_t lane = threadIdx.x;
    const uint64_t u = blockIdx.x / a.groups;                           // (uniform, as is everything of the row)
    const uint32_t w = blockIdx.x - (uint32_t)u * a.groups;
    const BlockRow r = block_row(a, u);
    const uint64_t todo = OUT ? r.blocks : (r.blocks ? r.blocks - 1u : 0u);
    const uint64_t k0 = (uint64_t)w * IIR_BLOCK_LANES;
    if (k0 >= todo) return;
    const uint64_t k = k0 + lane;
    const bool active = k < todo;
    const uint32_t S = a.sections[r.fc];
    double c[SB][5];
#pragma unroll
    for (uint32_t j = 0; j < SB; ++j)
#pragma unroll
        for (uint32_t q = 0; q < 5; ++q) {
            c[j][q] = a.image[(uint64_t)r.fc * IIR_IMAGE_DOUBLES + 5u * j + q];
            // (the filter is the row's, so uniform: the compiler would keep 10 SB scalar registers of coefficients and spill
            // them from a bound of four on; there they live in vector registers like the states)
            if (SB >= 4u) asm volatile("" : "+v"(c[j][q]));
        }
    double s1[SB], s2[SB];
#pragma unroll
    for (uint32_t j = 0; j < SB; ++j) s1[j] = s2[j] = 0.0;
    if (OUT && active && k > 0u) {
        const double *e = a.state + (u * a.grid_blocks + (k - 1u)) * (2u * SB);
#pragma unroll
        for (uint32_t j = 0; j < SB; ++j) {
            s1[j] = e[2u * j];
            s2[j] = e[2u * j + 1u];
        }
    }
    // (the row's last group of four, or sample: where a load past the stride goes)
    const uint64_t start = k0 * IIR_BLOCK, row_last = a.row_stride - (VEC ? 4u : 1u);
    const uint64_t start_in = start < row_last ? start : row_last;
    const float *from = a.rows + u * a.row_stride + start_in;
    const uint32_t last = steps_from(start_in, row_last);
    float *to = a.out + u * a.out_stride + (start < r.n_out ? start : r.n_out);
    const uint32_t outs = steps_from(start, r.n_out);
    const uint64_t first = k * IIR_BLOCK;                               // the lane's first step
    const uint64_t left = r.steps - k0 * IIR_BLOCK;                     // (> 0: block k0 is one of the row's)
    const uint32_t extent = OUT && left < IIR_BLOCK ? (uint32_t)left : IIR_BLOCK;
    float *mine_lds = tile + lane * LOUD_PITCH;
    float x[LOUD_LOADS][4];
    uint32_t bad = 0;
    const uint32_t piece = (lane >> 4) * IIR_BLOCK + 4u * (lane & 15u);
    block_load<VEC>(from, last, piece, 0, x);
    loud_stash(tile, lane, x);
    __syncthreads();
    for (uint32_t t0 = 0; t0 < extent; t0 += LOUD_T) {
        const bool more = t0 + LOUD_T < extent;
        if (more) block_load<VEC>(from, last, piece, t0 + LOUD_T, x);
        const uint32_t run = extent - t0 < LOUD_T ? extent - t0 : LOUD_T;
        constexpr uint32_t UNROLL = 4u;
        uint32_t i = 0;
        for (; i + UNROLL <= run; i += UNROLL) {
#pragma unroll
            for (uint32_t q = 0; q < UNROLL; ++q) {
                const float y = biquad_sample<SB>(mine_lds[i + q], first + t0 + i + q < r.n, S, c, s1, s2, bad);
                if (OUT) mine_lds[i + q] = y;
            }
        }
#pragma unroll 1
        for (; i < run; ++i) {
            const float y = biquad_sample<SB>(mine_lds[i], first + t0 + i < r.n, S, c, s1, s2, bad);
            if (OUT) mine_lds[i] = y;
        }
        __syncthreads();                                // every lane's outputs are in the tile
        if (OUT) {
            block_store<VEC>(tile, outs, to, piece, t0, lane);
            __syncthreads();                            // ... and have left it
        }
        if (more) loud_stash(tile, lane, x);
        __syncthreads();
    }
    if (OUT) {
        bad = wave_sum(bad);
        if (lane == 0u) a.cbad[u * a.groups + w] = bad;
    } else if (active) {
        double *z = a.state + (u * a.grid_blocks + k) * (2u * SB);
#pragma unroll
        for (uint32_t j = 0; j < SB; ++j) {
            z[2u * j] = s1[j];
            z[2u * j + 1u] = s2[j];
        }
    }
}

// lane j's x in every lane, j a constant: two v_readlane_b32 into a pair of SGPRs
__device__ __forceinline__ double lane_value(double x, uint32_t j)
{
    const long long b = __double_as_longlong(x);
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)b, (int)j);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)((unsigned long long)b >> 32), (int)j);
    return __longlong_as_double((long long)(((unsigned long long)hi << 32) | lo));
}

// One wave = one row, lane i < 2 SB = state i (s1[0] s2[0] s1[1] ...) with row i of the filter's T in registers.  Per block k:
// e_k goes round the wave by readlane, e_{k+1}[i] is the contract's sum over j <= m = 2 (i / 2) + 1 in ascending order, then
// + z_k[i]; it is stored over z_k, where the output pass finds block k + 1's entry state.  The products do not depend on one
// another; a term past m enters the chain as -0.0, which changes no sum by a bit (x + -0.0 == x for every x, -0.0 and the
// NaNs included), so the chain is 2 SB additions a block and nothing else; z_{k+1} is loaded a block ahead.
// States past the filter's own 2 S carry whatever their sections computed: nobody keeps a result of theirs.
template <uint32_t SB>
__global__ __launch_bounds__(64) void biquad_block_propagate_kernel(BiquadBlockArgs a)
{
    const uint32_t lane = threadIdx.x;
    const uint64_t u = blockIdx.x;
    const BlockRow r = block_row(a, u);
    if (r.blocks < 2u) return;
    const bool own = lane < 2u * SB;
    const uint32_t i = own ? lane : 0u;                 // (the other lanes repeat lane 0's work and store nothing)
    const uint32_t m = 2u * (i / 2u) + 1u;
    double T[2u * SB];
#pragma unroll
    for (uint32_t j = 0; j < 2u * SB; ++j)
        T[j] = a.matrices[(uint64_t)r.fc * IIR_MATRIX_DOUBLES + i * IIR_MATRIX_STATES + j];
    double *slot = a.state + u * a.grid_blocks * (2u * SB) + i;
    const uint64_t last = r.blocks - 2u;                // the last block anybody leaves
    double e = 0.0;
    double z = slot[0];
    for (uint64_t k = 0; k <= last; ++k) {
        const uint64_t ahead = k < last ? k + 1u : k;
        const double z_next = slot[ahead * (2u * SB)];
        double acc = T[0] * lane_value(e, 0u);
#pragma unroll
        for (uint32_t j = 1; j < 2u * SB; ++j) {
            const double p = T[j] * lane_value(e, j);
            acc = acc + (j <= m ? p : -0.0);
        }
        e = acc + z;
        if (own) slot[k * (2u * SB)] = e;
        z = z_next;
    }
}

// a row's out_len and count, one lane per row: the counts of the workgroups that ran for it, ceil(blocks / 64) of them
__global__ __launch_bounds__(256) void biquad_block_totals_kernel(BiquadBlockArgs a, uint32_t *__restrict__ out_len,
                                                                  uint32_t *__restrict__ nonfinite)
{
    const uint64_t u = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (u >= a.n_rows) return;
    const BlockRow r = block_row(a, u);
    if (r.refused) {
        refuse_counts(out_len, nonfinite, u);
        return;
    }
    const uint64_t ran = (r.blocks + IIR_BLOCK_LANES - 1u) / IIR_BLOCK_LANES;
    uint32_t b = 0u;
    for (uint64_t w = 0; w < ran; ++w) b += a.cbad[u * a.groups + w];
    if (out_len) out_len[u] = (uint32_t)r.n_out;          // (n_out < 2^32: the host has refused strides that allow more)
    if (nonfinite) nonfinite[u] = b;
}

template <uint32_t SB, bool OUT>
void block_launch_vec(const BiquadBlockArgs &a, bool vec, uint32_t workgroups, hipStream_t stream)
{
    if (vec)
        hipLaunchKernelGGL((biquad_block_kernel<SB, true, OUT>), dim3(workgroups), dim3(64), 0, stream, a);
    else
        hipLaunchKernelGGL((biquad_block_kernel<SB, false, OUT>), dim3(workgroups), dim3(64), 0, stream, a);
}

template <bool OUT>
hipError_t block_launch(const BiquadBlockArgs &a, uint32_t bound, hipStream_t stream)
{
    const uint64_t workgroups = (uint64_t)a.n_rows * a.groups;
    if (workgroups == 0) return hipSuccess;
    if (workgroups > 0x7FFFFFFFull) return hipErrorInvalidValue;
    // (the rest pass writes no samples: what it loads decides alone)
    const bool vec = aligned16(a.rows, a.row_stride) && (!OUT || aligned16(a.out, a.out_stride));
    if (bound <= 1u)
        block_launch_vec<1, OUT>(a, vec, (uint32_t)workgroups, stream);
    else if (bound == 2u)
        block_launch_vec<2, OUT>(a, vec, (uint32_t)workgroups, stream);
    else if (bound <= 4u)
        block_launch_vec<4, OUT>(a, vec, (uint32_t)workgroups, stream);
    else
        block_launch_vec<8, OUT>(a, vec, (uint32_t)workgroups, stream);
    return hipGetLastError();
}

}  // namespace

hipError_t launch_biquad_block_rest(const BiquadBlockArgs &args, uint32_t bound, hipStream_t stream)
{
    return block_launch<false>(args, bound, stream);
}

hipError_t launch_biquad_block_output(const BiquadBlockArgs &args, uint32_t bound, hipStream_t stream)
{
    return block_launch<true>(args, bound, stream);
}

hipError_t launch_biquad_block_propagate(const BiquadBlockArgs &args, uint32_t bound, hipStream_t stream)
{
    if (args.n_rows == 0 || args.grid_blocks < 2u) return hipSuccess;
    if (bound <= 1u)
        hipLaunchKernelGGL(biquad_block_propagate_kernel<1>, dim3(args.n_rows), dim3(64), 0, stream, args);
    else if (bound == 2u)
        hipLaunchKernelGGL(biquad_block_propagate_kernel<2>, dim3(args.n_rows), dim3(64), 0, stream, args);
    else if (bound <= 4u)
        hipLaunchKernelGGL(biquad_block_propagate_kernel<4>, dim3(args.n_rows), dim3(64), 0, stream, args);
    else
        hipLaunchKernelGGL(biquad_block_propagate_kernel<8>, dim3(args.n_rows), dim3(64), 0, stream, args);
    return hipGetLastError();
}

hipError_t launch_biquad_block_totals(const BiquadBlockArgs &args, uint32_t *out_len, uint32_t *nonfinite, hipStream_t stream)
{
    if (args.n_rows == 0) return hipSuccess;
    hipLaunchKernelGGL(biquad_block_totals_kernel, dim3((args.n_rows + 255u) / 256u), dim3(256), 0, stream, args, out_len, nonfinite);
    return hipGetLastError();
}

}  // namespace grail
