// resample_kernels.hip — rational-ratio sample-rate conversion of finished rows (grail_resample_async).  The contract
// (include/grail_hip.h, "levels, continued: sample-rate conversion"): output m of a row sits at input time m D / U; with
// a = m D, p = a mod U, i0 = a div U it is the left fold acc = acc + C[p][k] * v[i0 + P/2 - k] over ascending k from +0.0
// in binary64, rounded once to binary32, C[p][k] = N / 2^26 a Kaiser-windowed sinc.  The filter is FIR, so time is
// parallel: one workgroup per (row, chunk of RESAMPLE_CHUNK outputs), one lane per output (four passes of 256), the fold
// serial in the lane.  The kernel folds with the integers themselves, acc' = fma((double)N, v, acc'): every N * v is exact
// (27 bits times 24) and nothing comes near the ends of binary64's range, so acc' is 2^26 acc bit for bit at every step,
// and y = (float)(acc' * 2^-26) is the contract's one rounding.  No atomics, every store a plain vector store.
// DESIGN.md §4.13.  The same fold on rows fed chunk by chunk (grail_resample_stream_*, §4.16): a stretch staged from a row's
// ring and the call's samples, the row's place kept as an input time and a phase.  The finite test, the state word, the ring
// and what the totals and advance kernels do are row_kernel_common.h's; the two chunk kernels keep their bookkeeping in their
// own text, because any call inside them moved their instruction streams and registers (§4.21).
#include "kernels.h"
#include "resample_plan.h"
#include "row_kernel_common.h"

namespace grail {

namespace {

constexpr uint32_t RS_THREADS = 256;
constexpr uint32_t RS_PASSES = RESAMPLE_CHUNK / RS_THREADS;     // outputs per lane
constexpr uint32_t RS_LDS_MAX = 65536 - 64;                     // bytes of LDS a workgroup may ask for (64 KB less the static words)
constexpr uint32_t RS_STAGE_SLACK = 8;                          // the stretch starts at a multiple of 4 and ends at one

// n = min(len, row_stride) and n_out = min(ceil(n U / D), out_stride) of a row (n < 2^32, U < 2^10: no overflow)
__device__ __forceinline__ void rs_row(const uint32_t *__restrict__ len, uint64_t row_stride, uint64_t out_stride, uint64_t u,
                                       uint32_t U, uint32_t D, uint64_t &n, uint64_t &n_out)
{
    n = len[u] < row_stride ? len[u] : row_stride;
    const uint64_t full = (n * U + (D - 1u)) / D;
    n_out = full < out_stride ? full : out_stride;
}

// One workgroup = one (row, chunk of RESAMPLE_CHUNK outputs).
//   STAGED: the chunk's input stretch (the samples its outputs' taps reach) goes to LDS once, zeroed where it lies outside
//     the row or is not finite; otherwise (a ratio whose stretch does not fit) the taps read the row itself, clamped.
//   VEC: 16-byte loads and stores (both bases 16-byte aligned, both strides multiples of 4), else 4-byte ones: same bits.
//   TAB: where a lane finds its coefficients.  RS_TAB_UNIFORM: U = 1, one phase: the coefficient of a tap is the same in
//     every lane and is loaded once per wave.  RS_TAB_LDS: a lane walks its own row p of the table, which the workgroup
//     copied to LDS (it fits beside the stretch) at a pitch of P + 1 words, odd, so that lanes on different rows fall on
//     different banks.  RS_TAB_GLOBAL: the same walk over the table where it lies (at most 128 KB: cache-resident).
// smem: [RESAMPLE_CHUNK] the chunk's outputs (a lane computes m0 + tid + 256 j, whose taps fall on neighbouring LDS
// words; the stores want four consecutive outputs in a lane), then [stage_words] the stretch, then the table.
constexpr int RS_TAB_GLOBAL = 0, RS_TAB_UNIFORM = 1, RS_TAB_LDS = 2;
template <bool STAGED, bool VEC, int TAB>
__global__ __launch_bounds__(256) void resample_kernel(const float *__restrict__ rows, uint64_t row_stride,
                                                       const uint32_t *__restrict__ len, uint32_t n_rows, uint32_t U, uint32_t D,
                                                       uint32_t P, const int32_t *__restrict__ table, uint32_t stage_words,
                                                       uint32_t grid_chunks, float *__restrict__ out, uint64_t out_stride,
                                                       uint32_t *__restrict__ cbad)
{
    extern __shared__ float smem[];
    float *yout = smem, *stage = smem + RESAMPLE_CHUNK;
    int32_t *ltab = reinterpret_cast<int32_t *>(smem + RESAMPLE_CHUNK + stage_words);
    const uint32_t pitch = TAB == RS_TAB_LDS ? P + 1u : P;
    const uint32_t tid = threadIdx.x;
    const uint64_t u = blockIdx.x / grid_chunks;
    const uint32_t c = (uint32_t)(blockIdx.x - u * grid_chunks);
    if (u >= n_rows) return;
    uint64_t n, n_out;
    rs_row(len, row_stride, out_stride, u, U, D, n, n_out);
    const uint64_t m0 = (uint64_t)c * RESAMPLE_CHUNK;
    // a row of no samples has no chunk; chunk 0 of any other runs even with no output to write: it counts
    if (n == 0 || (m0 >= n_out && c != 0u)) return;
    const bool last = m0 + RESAMPLE_CHUNK >= n_out;
    const uint32_t count = m0 >= n_out ? 0u : (last ? (uint32_t)(n_out - m0) : RESAMPLE_CHUNK);
    const float *row = rows + u * row_stride;
    const uint32_t half = P >> 1;

    // the chunk's first output: a = m0 D, in 64 bits; every other output of the chunk is fewer than 2^20 further
    const uint64_t a0 = m0 * D;
    const int64_t i_base = (int64_t)(a0 / U);
    const uint32_t p_base = (uint32_t)(a0 - (uint64_t)i_base * U);
    // the input samples this chunk counts non-finite ones in: those between its first output's time and the next
    // chunk's, rounded up; the row's last chunk takes the rest of the row
    const int64_t own_lo = c ? (int64_t)((a0 + U - 1u) / U) : 0;
    const int64_t own_hi = last ? (int64_t)n : (int64_t)(((m0 + RESAMPLE_CHUNK) * D + U - 1u) / U);
    // the stretch: from the last tap of the first output to the first tap of the last, s_base a multiple of 4 at or below
    const uint32_t span = count ? (uint32_t)(((uint64_t)p_base + (uint64_t)(count - 1u) * D) / U) : 0u;
    const int64_t s_lo = i_base + 1 - (int64_t)half, s_hi = i_base + (int64_t)span + (int64_t)half + 1;
    const int64_t s_base = s_lo & ~(int64_t)3;
    uint32_t bad = 0u;
    int64_t counted_to = own_lo;            // what the staging has counted of [own_lo, own_hi)
    if (STAGED && count) {
        const uint32_t groups = (uint32_t)((s_hi - s_base + 3) >> 2);
        const int64_t g_hi = (int64_t)((n - 1u) >> 2), t_hi = (int64_t)n - 1;
        for (uint32_t gi = tid; gi < groups; gi += RS_THREADS) {
            const int64_t t0 = s_base + 4 * (int64_t)gi;
            float x[4];
            if (VEC) {
                // the row's last group starts below n <= row_stride, a multiple of 4: inside the row
                int64_t g = t0 >> 2;
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
                stage[4u * gi + e] = (inside && finite) ? x[e] : 0.0f;
            }
        }
        counted_to = s_base + 4 * (int64_t)groups;
        counted_to = counted_to < own_lo ? own_lo : counted_to;
    }
    // what the chunk owns past its stretch (an out_stride that cuts the row short leaves the last chunk the rest of the
    // row; a chunk that is not staged owns all of its samples here): counted from the row itself
    for (int64_t t = counted_to + tid; t < own_hi; t += RS_THREADS) bad += finite_f32(row[t]) ? 0u : 1u;
    if (TAB == RS_TAB_LDS && count) {
        for (uint32_t i = tid; i < U * P; i += RS_THREADS) {
            const uint32_t p = i / P;
            ltab[p * pitch + (i - p * P)] = table[i];
        }
    }
    __syncthreads();

    if (count) {
        double acc[RS_PASSES];
        uint32_t at[RS_PASSES];             // STAGED: the LDS word of tap 0; else unused
        int64_t t_first[RS_PASSES];         // the input time of tap 0
        uint32_t tab[RS_PASSES];            // the first word of the lane's row of the table
#pragma unroll
        for (uint32_t j = 0; j < RS_PASSES; ++j) {
            uint32_t r = tid + RS_THREADS * j;
            r = r < count ? r : count - 1u;                         // (a lane past the chunk's last output repeats it, unstored)
            const uint32_t off = p_base + r * D;                    // < 2^10 + 2^10 2^10
            const uint32_t q = off / U, p = off - q * U;
            t_first[j] = i_base + (int64_t)q + (int64_t)half;
            at[j] = (uint32_t)(t_first[j] - s_base);
            tab[j] = TAB == RS_TAB_UNIFORM ? 0u : p * pitch;
            acc[j] = 0.0;
        }
        const int64_t t_hi = (int64_t)n - 1;
        for (uint32_t k = 0; k < P; ++k) {
#pragma unroll
            for (uint32_t j = 0; j < RS_PASSES; ++j) {
                float x;
                if (STAGED) {
                    x = stage[at[j] - k];
                } else {
                    const int64_t t = t_first[j] - (int64_t)k;
                    int64_t tc = t < 0 ? 0 : t;
                    tc = tc > t_hi ? t_hi : tc;
                    const float raw = row[tc];
                    x = (t >= 0 && t <= t_hi && finite_f32(raw)) ? raw : 0.0f;
                }
                const int32_t num = TAB == RS_TAB_LDS ? ltab[tab[j] + k] : table[tab[j] + k];
                acc[j] = __builtin_fma((double)num, (double)x, acc[j]);
            }
        }
#pragma unroll
        for (uint32_t j = 0; j < RS_PASSES; ++j) yout[tid + RS_THREADS * j] = (float)(acc[j] * 1.4901161193847656e-08);   // 2^-26
    }
    __syncthreads();
    // four consecutive outputs per lane; a row's last partial group goes out in 4-byte stores
    if (4u * tid < count) {
        float *to = out + u * out_stride + m0 + 4u * tid;
        if (VEC && 4u * tid + 4u <= count) {
            *reinterpret_cast<float4 *>(to) = *reinterpret_cast<const float4 *>(yout + 4u * tid);
        } else {
#pragma unroll
            for (uint32_t e = 0; e < 4; ++e)
                if (4u * tid + e < count) to[e] = yout[4u * tid + e];
        }
    }
    // the chunk's count: integers, so any order
#pragma unroll
    for (int s = 32; s > 0; s >>= 1) bad += (uint32_t)__shfl_xor((int)bad, s, 64);
    __shared__ uint32_t red[RS_THREADS / 64];
    if ((tid & 63u) == 0u) red[tid >> 6] = bad;
    __syncthreads();
    if (tid == 0u) cbad[u * grid_chunks + c] = red[0] + red[1] + red[2] + red[3];
}

// A row's numbers from its chunks, one lane per row.
__global__ __launch_bounds__(256) void resample_totals_kernel(const uint32_t *__restrict__ len, uint64_t row_stride,
                                                              uint32_t n_rows, uint32_t U, uint32_t D, uint64_t out_stride,
                                                              const uint32_t *__restrict__ cbad, uint32_t grid_chunks,
                                                              uint32_t *__restrict__ out_len, uint32_t *__restrict__ nonfinite)
{
    const uint64_t u = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (u >= n_rows) return;
    uint64_t n, n_out;
    rs_row(len, row_stride, out_stride, u, U, D, n, n_out);
    const uint32_t b = sum_chunks(cbad, u, grid_chunks, row_chunks<RESAMPLE_CHUNK>(n, n_out));
    if (out_len) out_len[u] = (uint32_t)n_out;
    if (nonfinite) nonfinite[u] = b;
}

// ---- streams (grail_resample_stream_*): rows fed chunk by chunk, DESIGN.md §4.16 ---------------------------------------------
// A row's state is three 64-bit words: the state word of row_kernel_common.h; i = floor(M D / U), the input time of the next
// output M; p = M D mod U, its phase (N U outgrows 64 bits long before N does, so nothing here is computed from N U).  Its
// ring (there too) holds at least P - 1 samples.  In the frame of one call, local time = global time - N: v is the ring
// below 0 (+0.0 before the row's first sample), the call's n samples from 0, +0.0 from n on (which only a finishing call
// reaches: its n is 0).  Output r of the call starts at local time (i - N) + (p + r D) div U and phase (p + r D) mod U.
constexpr uint32_t RS_STATE_WORDS = RESAMPLE_STREAM_STATE_WORDS;
constexpr uint32_t RS_STREAM_PASSES = RESAMPLE_STREAM_CHUNK / RS_THREADS;     // at most four: rs_outputs' NPASS below
static_assert(RS_STREAM_PASSES >= 1 && RS_STREAM_PASSES <= 4 && RESAMPLE_STREAM_CHUNK % RS_THREADS == 0, "the passes of a chunk");

struct RsStreamRow {
    uint64_t fed, i;        // N; the next output's input time
    uint32_t p, n, count;   // its phase; the samples this call feeds, the outputs it writes
    bool takes, refused;    // the call changes the row's state; the row has ended and is fed
};
__device__ __forceinline__ RsStreamRow rs_stream_row(const uint64_t *__restrict__ state, const uint32_t *__restrict__ in_len,
                                                     uint64_t in_stride, const uint8_t *__restrict__ mark, bool finishing, uint64_t u,
                                                     uint32_t U, uint32_t D, uint32_t half)
{
    RsStreamRow r;
    const uint64_t w = state[RS_STATE_WORDS * u];
    const bool ended = (w & STREAM_ENDED) != 0;
    r.fed = w & ~STREAM_ENDED;
    r.i = state[RS_STATE_WORDS * u + 1u];
    r.p = (uint32_t)state[RS_STATE_WORDS * u + 2u];
    int64_t T;              // the last input time an output of this call may start at
    if (finishing) {
        r.n = 0u;
        r.refused = false;
        r.takes = !ended && (!mark || mark[u]);
        T = (int64_t)r.fed - 1;                                     // the samples to come are +0.0: every i0 <= N - 1
    } else {
        r.n = in_len[u] < in_stride ? in_len[u] : (uint32_t)in_stride;
        r.refused = ended && r.n;
        r.takes = !ended;
        T = (int64_t)(r.fed + r.n) - 1 - (int64_t)half;             // output m needs sample i0 + h
    }
    // the outputs r with i + (p + r D) div U <= T: ceil(((T - i + 1) U - p) / D), T - i + 1 <= n + h < 2^33, U < 2^10
    r.count = r.takes && T >= (int64_t)r.i ? (uint32_t)(((uint64_t)(T - (int64_t)r.i + 1) * U - r.p + (D - 1u)) / D) : 0u;
    return r;
}

// The fold and the stores of a chunk of the stream kernel: resample_kernel's, line for line, for NPASS passes of 256 outputs
// and with `tap` for what an unstaged tap reads.  It is a copy on purpose: with both kernels on one inline function
// resample_kernel kept its registers and its LDS but ran 0.5 % slower at full size, more than its own runs differ, so
// resample_kernel stays textually as it was (profiles/r17_resample_stream.txt).  Output r of the chunk,
// r < count <= 256 NPASS, starts at input time i_base + (p_base + r D) div U and phase (p_base + r D) mod U; lane tid folds
// r = tid + 256 j serially over ascending k, the outputs go through yout to `to` (the chunk's first output in the row),
// four consecutive ones per lane.  Every lane of the workgroup comes here (there is a barrier inside).
template <bool STAGED, bool VEC, int TAB, uint32_t NPASS, typename Tap>
__device__ __forceinline__ void rs_outputs(float *yout, const float *stage, const int32_t *ltab, const int32_t *__restrict__ table,
                                           uint32_t pitch, uint32_t tid, uint32_t count, int64_t i_base, uint32_t p_base,
                                           int64_t s_base, uint32_t U, uint32_t D, uint32_t P, const Tap &tap, float *to)
{
    const uint32_t half = P >> 1;
    if (count) {
        double acc[NPASS];
        uint32_t at[NPASS];                 // STAGED: the LDS word of tap 0; else unused
        int64_t t_first[NPASS];             // the input time of tap 0
        uint32_t tab[NPASS];                // the first word of the lane's row of the table
#pragma unroll
        for (uint32_t j = 0; j < NPASS; ++j) {
            uint32_t r = tid + RS_THREADS * j;
            r = r < count ? r : count - 1u;                         // (a lane past the chunk's last output repeats it, unstored)
            const uint32_t off = p_base + r * D;                    // < 2^10 + 2^10 2^10
            const uint32_t q = off / U, p = off - q * U;
            t_first[j] = i_base + (int64_t)q + (int64_t)half;
            at[j] = (uint32_t)(t_first[j] - s_base);
            tab[j] = TAB == RS_TAB_UNIFORM ? 0u : p * pitch;
            acc[j] = 0.0;
        }
        for (uint32_t k = 0; k < P; ++k) {
#pragma unroll
            for (uint32_t j = 0; j < NPASS; ++j) {
                const float x = STAGED ? stage[at[j] - k] : tap(t_first[j] - (int64_t)k);
                const int32_t num = TAB == RS_TAB_LDS ? ltab[tab[j] + k] : table[tab[j] + k];
                acc[j] = __builtin_fma((double)num, (double)x, acc[j]);
            }
        }
#pragma unroll
        for (uint32_t j = 0; j < NPASS; ++j) yout[tid + RS_THREADS * j] = (float)(acc[j] * 1.4901161193847656e-08);   // 2^-26
    }
    __syncthreads();
    // four consecutive outputs per lane; a row's last partial group goes out in 4-byte stores
    if (4u * tid < count) {
        to += 4u * tid;
        if (VEC && 4u * tid + 4u <= count) {
            *reinterpret_cast<float4 *>(to) = *reinterpret_cast<const float4 *>(yout + 4u * tid);
        } else {
#pragma unroll
            for (uint32_t e = 0; e < 4; ++e)
                if (4u * tid + e < count) to[e] = yout[4u * tid + e];
        }
    }
}

// What a tap of the stream kernel reads where the stretch is not staged: the ring below local time 0, the call's samples
// from there, both addresses clamped and both loads issued, then selected.
struct RsStreamTap {
    const float *__restrict__ row;
    const float *__restrict__ hist;
    uint64_t fed, ring_mask;
    int64_t t_lo, t_hi, t_top;      // how far back the row reaches; n - 1; max(n - 1, 0)
    __device__ __forceinline__ float operator()(int64_t t) const
    {
        int64_t tc = t < 0 ? 0 : t;
        tc = tc > t_top ? t_top : tc;
        const float raw = row[tc];
        const float old = hist[(fed + (uint64_t)t) & ring_mask];
        const float cur = (t <= t_hi && finite_f32(raw)) ? raw : 0.0f;
        return t < 0 ? (t >= t_lo ? old : 0.0f) : cur;
    }
};

// resample_kernel with the row's state in place of m0 D and of the row's length: one workgroup = one (row, chunk of
// RESAMPLE_STREAM_CHUNK of this call's outputs).  Reads the state and the ring, writes neither (resample_stream_advance_kernel,
// queued behind it, is their only writer).  STAGED, VEC, TAB as in resample_kernel; the stretch is staged from the ring by
// 4-byte loads and from the call's samples by 16-byte ones (VEC), no load behind a branch.  Chunk c counts the non-finite
// samples among this call's inputs between its first output's time and the next chunk's, the last chunk to the end of them.
// A streaming call is small (480 samples of 48 000 -> 16 000 are 160 outputs): the passes of 256 outputs past the chunk's
// count are not run.
template <bool STAGED, bool VEC, int TAB>
__global__ __launch_bounds__(256) void resample_stream_kernel(const float *__restrict__ in, uint64_t in_stride,
                                                              const uint32_t *__restrict__ in_len, uint32_t n_rows, uint32_t U,
                                                              uint32_t D, uint32_t P, const int32_t *__restrict__ table,
                                                              uint32_t stage_words, uint32_t grid_chunks,
                                                              const uint64_t *__restrict__ state, const float *__restrict__ ring,
                                                              uint32_t ring_cap, const uint8_t *__restrict__ mark, uint32_t finishing,
                                                              float *__restrict__ out, uint64_t out_stride, uint32_t *__restrict__ cbad)
{
    extern __shared__ float smem[];
    float *yout = smem, *stage = smem + RESAMPLE_STREAM_CHUNK;
    int32_t *ltab = reinterpret_cast<int32_t *>(smem + RESAMPLE_STREAM_CHUNK + stage_words);
    const uint32_t pitch = TAB == RS_TAB_LDS ? P + 1u : P;
    const uint32_t tid = threadIdx.x;
    const uint64_t u = blockIdx.x / grid_chunks;
    const uint32_t c = (uint32_t)(blockIdx.x - u * grid_chunks);
    if (u >= n_rows) return;
    const uint32_t half = P >> 1;
    const RsStreamRow r = rs_stream_row(state, in_len, in_stride, mark, finishing != 0u, u, U, D, half);
    const int64_t n = r.n;
    const uint64_t n_out = r.count;
    const uint64_t m0 = (uint64_t)c * RESAMPLE_STREAM_CHUNK;
    // a refused row and one with neither samples nor outputs have no chunk; chunk 0 of any other runs even with no output
    // to write: it counts
    if (r.refused || (n == 0 && n_out == 0) || (m0 >= n_out && c != 0u)) return;
    const bool last = m0 + RESAMPLE_STREAM_CHUNK >= n_out;
    const uint32_t count = m0 >= n_out ? 0u : (last ? (uint32_t)(n_out - m0) : RESAMPLE_STREAM_CHUNK);
    const float *hist = ring + u * ring_cap;
    const float *row = n ? in + u * in_stride : hist;               // (a call of no samples: a clamped load lands in the ring)
    const uint64_t ring_mask = ring_cap - 1u;
    const int64_t t_hi = n - 1, t_top = n ? n - 1 : 0;
    const int64_t t_lo = -(int64_t)(P - 1u < r.fed ? P - 1u : r.fed);   // how far back the taps and the row reach

    // the chunk's first output in the call's frame: a = p + m0 D above (i - N) U; every other is fewer than 2^20 further
    const int64_t rel = (int64_t)(r.i - r.fed);                     // >= -h: what starts lower was written before
    const uint64_t a0 = (uint64_t)r.p + m0 * D;
    const int64_t i_base = rel + (int64_t)(a0 / U);
    const uint32_t p_base = (uint32_t)(a0 % U);
    // the call's samples this chunk counts non-finite ones in, cut to [0, n]
    int64_t own_lo = c ? rel + (int64_t)((a0 + U - 1u) / U) : 0;
    int64_t own_hi = last ? n : rel + (int64_t)((a0 + (uint64_t)RESAMPLE_STREAM_CHUNK * D + U - 1u) / U);
    own_lo = own_lo < 0 ? 0 : (own_lo > n ? n : own_lo);
    own_hi = own_hi < 0 ? 0 : (own_hi > n ? n : own_hi);
    const uint32_t span = count ? (uint32_t)(((uint64_t)p_base + (uint64_t)(count - 1u) * D) / U) : 0u;
    const int64_t s_lo = i_base + 1 - (int64_t)half, s_hi = i_base + (int64_t)span + (int64_t)half + 1;
    const int64_t s_base = s_lo & ~(int64_t)3;
    uint32_t bad = 0u;
    int64_t counted_to = own_lo;            // what the staging has counted of [own_lo, own_hi)
    if (STAGED && count) {
        const uint32_t groups = (uint32_t)((s_hi - s_base + 3) >> 2);
        const int64_t g_hi = t_top >> 2;
        for (uint32_t gi = tid; gi < groups; gi += RS_THREADS) {
            const int64_t t0 = s_base + 4 * (int64_t)gi;           // a multiple of 4: a group is all ring or all call
            float x[4], old[4];
            if (VEC) {
                // the call's last group starts below n <= in_stride, a multiple of 4: inside the row
                int64_t g = t0 >> 2;
                g = g < 0 ? 0 : g;
                g = g > g_hi ? g_hi : g;
                const float4 v = *reinterpret_cast<const float4 *>(row + 4 * g);
                x[0] = v.x, x[1] = v.y, x[2] = v.z, x[3] = v.w;
            } else {
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    int64_t t = t0 + e;
                    t = t < 0 ? 0 : t;
                    t = t > t_top ? t_top : t;
                    x[e] = row[t];
                }
            }
#pragma unroll
            for (int e = 0; e < 4; ++e) old[e] = hist[(r.fed + (uint64_t)(t0 + e)) & ring_mask];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int64_t t = t0 + e;
                const bool inside = t >= 0 && t <= t_hi;            // (what a clamped load brought is outside)
                const bool finite = finite_f32(x[e]);
                bad += (inside && !finite && t >= own_lo && t < own_hi) ? 1u : 0u;
                const float cur = (inside && finite) ? x[e] : 0.0f;
                // the ring holds the last ring_cap >= P - 1 samples fed, already +0.0 where they were not finite
                stage[4u * gi + e] = t < 0 ? (t >= t_lo ? old[e] : 0.0f) : cur;
            }
        }
        counted_to = s_base + 4 * (int64_t)groups;
        counted_to = counted_to < own_lo ? own_lo : counted_to;
    }
    // what the chunk owns past its stretch (a chunk that is not staged owns all of its samples here)
    for (int64_t t = counted_to + tid; t < own_hi; t += RS_THREADS) bad += finite_f32(row[t]) ? 0u : 1u;
    if (TAB == RS_TAB_LDS && count) {
        for (uint32_t i = tid; i < U * P; i += RS_THREADS) {
            const uint32_t p = i / P;
            ltab[p * pitch + (i - p * P)] = table[i];
        }
    }
    __syncthreads();

    const RsStreamTap tap{row, hist, r.fed, ring_mask, t_lo, t_hi, t_top};
    float *to = out + u * out_stride + m0;
    const uint32_t passes = (count + RS_THREADS - 1u) / RS_THREADS;     // the same in every lane of the workgroup
    if (passes <= 1u)
        rs_outputs<STAGED, VEC, TAB, 1>(yout, stage, ltab, table, pitch, tid, count, i_base, p_base, s_base, U, D, P, tap, to);
    else if (passes == 2u)
        rs_outputs<STAGED, VEC, TAB, 2>(yout, stage, ltab, table, pitch, tid, count, i_base, p_base, s_base, U, D, P, tap, to);
    else if (passes == 3u)
        rs_outputs<STAGED, VEC, TAB, 3>(yout, stage, ltab, table, pitch, tid, count, i_base, p_base, s_base, U, D, P, tap, to);
    else
        rs_outputs<STAGED, VEC, TAB, RS_STREAM_PASSES>(yout, stage, ltab, table, pitch, tid, count, i_base, p_base, s_base, U, D, P, tap, to);
    // the chunk's count: integers, so any order
#pragma unroll
    for (int s = 32; s > 0; s >>= 1) bad += (uint32_t)__shfl_xor((int)bad, s, 64);
    __shared__ uint32_t red[RS_THREADS / 64];
    if ((tid & 63u) == 0u) red[tid >> 6] = bad;
    __syncthreads();
    if (tid == 0u) cbad[u * grid_chunks + c] = red[0] + red[1] + red[2] + red[3];
}

// Behind resample_stream_kernel on the stream, one wave per row, the only writer of a stream's state: the row's numbers
// from its chunks, the call's last samples into the ring (ring_keep), then N + n (a finishing call: the row ended) and the
// next output's i and p.  A row that has ended and is fed is refused (refuse_counts), its state as it was.
__global__ __launch_bounds__(256) void resample_stream_advance_kernel(const float *__restrict__ in, uint64_t in_stride,
                                                                      const uint32_t *__restrict__ in_len, uint32_t n_rows, uint32_t U,
                                                                      uint32_t D, uint32_t P, uint64_t *__restrict__ state,
                                                                      float *__restrict__ ring, uint32_t ring_cap,
                                                                      const uint8_t *__restrict__ mark, uint32_t finishing,
                                                                      const uint32_t *__restrict__ cbad, uint32_t grid_chunks,
                                                                      uint32_t *__restrict__ out_len, uint32_t *__restrict__ nonfinite)
{
    const uint64_t u = (uint64_t)blockIdx.x * (RS_THREADS / 64u) + (threadIdx.x >> 6);
    const uint32_t lane = threadIdx.x & 63u;
    if (u >= n_rows) return;
    const RsStreamRow r = rs_stream_row(state, in_len, in_stride, mark, finishing != 0u, u, U, D, P >> 1);
    if (r.refused) {
        if (lane == 0u) refuse_counts(out_len, nonfinite, u);
        return;
    }
    uint32_t bad = 0u;
    if (r.takes && r.n) {
        const uint32_t chunks = r.count ? (r.count + RESAMPLE_STREAM_CHUNK - 1u) / RESAMPLE_STREAM_CHUNK : 1u;
        for (uint32_t c = lane; c < chunks; c += 64u) bad += cbad[u * grid_chunks + c];
        ring_keep(in + u * in_stride, r.n, r.fed, ring + u * ring_cap, ring_cap, ring_cap, lane);
    }
    bad = wave_sum(bad);
    if (lane != 0u) return;
    if (out_len) out_len[u] = r.count;
    if (nonfinite) nonfinite[u] = bad;
    if (r.takes) {
        const uint64_t a = (uint64_t)r.p + (uint64_t)r.count * D;  // < 2^10 + 2^32 2^10
        state[RS_STATE_WORDS * u] = finishing ? (r.fed | STREAM_ENDED) : r.fed + r.n;
        state[RS_STATE_WORDS * u + 1u] = r.i + a / U;
        state[RS_STATE_WORDS * u + 2u] = a % U;
    }
}

// The instantiation a launch runs, but for VEC (launch_either's to choose): TAB by `tab`, the table in LDS only beside a staged
// stretch.
template <bool STAGED, bool VEC>
auto resample_variant(int tab)
{
    return tab == RS_TAB_UNIFORM             ? resample_kernel<STAGED, VEC, RS_TAB_UNIFORM>
           : (STAGED && tab == RS_TAB_LDS) ? resample_kernel<STAGED, VEC, STAGED ? RS_TAB_LDS : RS_TAB_GLOBAL>
                                             : resample_kernel<STAGED, VEC, RS_TAB_GLOBAL>;
}
template <bool STAGED, bool VEC>
auto resample_stream_variant(int tab)
{
    return tab == RS_TAB_UNIFORM             ? resample_stream_kernel<STAGED, VEC, RS_TAB_UNIFORM>
           : (STAGED && tab == RS_TAB_LDS) ? resample_stream_kernel<STAGED, VEC, STAGED ? RS_TAB_LDS : RS_TAB_GLOBAL>
                                             : resample_stream_kernel<STAGED, VEC, RS_TAB_GLOBAL>;
}

}  // namespace

uint64_t resample_grid_chunks(uint64_t row_stride, uint64_t out_stride, uint32_t U, uint32_t D)
{
    if (row_stride == 0) return 0;
    const unsigned __int128 full = ((unsigned __int128)row_stride * U + (D - 1u)) / D;
    const uint64_t longest = full < out_stride ? (uint64_t)full : out_stride;
    const uint64_t chunks = (longest + RESAMPLE_CHUNK - 1u) / RESAMPLE_CHUNK;
    return chunks ? chunks : 1u;
}

hipError_t launch_resample(const ResampleArgs &a, hipStream_t stream)
{
    const uint64_t workgroups = (uint64_t)a.n_rows * a.grid_chunks;
    hipError_t e;
    if (!grid_fits(workgroups, &e)) return e;
    const uint32_t U = a.up, D = a.down, P = a.taps;
    // the longest stretch of a chunk: floor((U - 1 + (RESAMPLE_CHUNK - 1) D) / U) + P samples, and the rounding to groups of 4
    const uint64_t stretch = ((uint64_t)(U - 1u) + (uint64_t)(RESAMPLE_CHUNK - 1u) * D) / U + P + RS_STAGE_SLACK;
    const uint64_t staged_bytes = (RESAMPLE_CHUNK + stretch) * 4u, table_bytes = (uint64_t)U * (P + 1u) * 4u;
    const bool staged = staged_bytes <= RS_LDS_MAX;
    const int tab = U == 1u ? RS_TAB_UNIFORM : (staged && staged_bytes + table_bytes <= RS_LDS_MAX ? RS_TAB_LDS : RS_TAB_GLOBAL);
    const uint32_t stage_words = staged ? (uint32_t)stretch : 0u;
    const uint32_t lds = (uint32_t)((staged ? staged_bytes : RESAMPLE_CHUNK * 4u) + (tab == RS_TAB_LDS ? table_bytes : 0u));
    launch_either(aligned16(a.rows, a.row_stride, a.out, a.out_stride),
                  staged ? resample_variant<true, true>(tab) : resample_variant<false, true>(tab),
                  staged ? resample_variant<true, false>(tab) : resample_variant<false, false>(tab), dim3((uint32_t)workgroups),
                  dim3(RS_THREADS), lds, stream, a.rows, a.row_stride, a.len, a.n_rows, a.up, a.down, a.taps, a.table, stage_words,
                  a.grid_chunks, a.out, a.out_stride, a.cbad);
    return hipGetLastError();
}

hipError_t launch_resample_stream(const ResampleArgs &a, hipStream_t stream)
{
    const uint64_t workgroups = (uint64_t)a.n_rows * a.grid_chunks;
    hipError_t e;
    if (!grid_fits(workgroups, &e)) return e;
    const uint32_t U = a.up, D = a.down, P = a.taps;
    // the stretch, the table and the three ways to the coefficients as in launch_resample, for the stream's chunk
    const uint64_t stretch = ((uint64_t)(U - 1u) + (uint64_t)(RESAMPLE_STREAM_CHUNK - 1u) * D) / U + P + RS_STAGE_SLACK;
    const uint64_t staged_bytes = (RESAMPLE_STREAM_CHUNK + stretch) * 4u, table_bytes = (uint64_t)U * (P + 1u) * 4u;
    const bool staged = staged_bytes <= RS_LDS_MAX;
    const int tab = U == 1u ? RS_TAB_UNIFORM : (staged && staged_bytes + table_bytes <= RS_LDS_MAX ? RS_TAB_LDS : RS_TAB_GLOBAL);
    const uint32_t stage_words = staged ? (uint32_t)stretch : 0u;
    const uint32_t lds = (uint32_t)((staged ? staged_bytes : RESAMPLE_STREAM_CHUNK * 4u) + (tab == RS_TAB_LDS ? table_bytes : 0u));
    launch_either(aligned16(a.rows, a.row_stride, a.out, a.out_stride),
                  staged ? resample_stream_variant<true, true>(tab) : resample_stream_variant<false, true>(tab),
                  staged ? resample_stream_variant<true, false>(tab) : resample_stream_variant<false, false>(tab),
                  dim3((uint32_t)workgroups), dim3(RS_THREADS), lds, stream, a.rows, a.row_stride, a.len, a.n_rows, a.up, a.down, a.taps,
                  a.table, stage_words, a.grid_chunks, a.state, a.ring, a.ring_cap, a.mark, a.finishing ? 1u : 0u, a.out, a.out_stride,
                  a.cbad);
    return hipGetLastError();
}

hipError_t launch_resample_stream_advance(const ResampleArgs &a, hipStream_t stream)
{
    if (a.n_rows == 0) return hipSuccess;
    const uint32_t rows_per_group = RS_THREADS / 64u;
    hipLaunchKernelGGL(resample_stream_advance_kernel, dim3(a.n_rows / rows_per_group + (a.n_rows % rows_per_group != 0u)),
                       dim3(RS_THREADS), 0, stream, a.rows, a.row_stride, a.len, a.n_rows, a.up, a.down, a.taps, a.state, a.ring,
                       a.ring_cap, a.mark, a.finishing ? 1u : 0u, a.cbad, a.grid_chunks, a.out_len, a.nonfinite);
    return hipGetLastError();
}

hipError_t launch_resample_totals(const ResampleArgs &a, hipStream_t stream)
{
    if (a.n_rows == 0) return hipSuccess;
    hipLaunchKernelGGL(resample_totals_kernel, dim3((a.n_rows + 255u) / 256u), dim3(256), 0, stream, a.len, a.row_stride, a.n_rows, a.up,
                       a.down, a.out_stride, a.cbad, a.grid_chunks, a.out_len, a.nonfinite);
    return hipGetLastError();
}

}  // namespace grail
