// meter_stream_kernels.hip — the meters on streams (grail_meter_stream_*): K-weighted hop sums and the true peak of rows fed
// chunk by chunk, their state resident in HBM between calls.  The contract (include/grail_hip.h, "levels, continued: the
// meters on streams"): for any split of a row's samples into calls the hop sums are grail_loudness_async's and the largest of
// the calls' true peaks is grail_true_peak_async's, bit for bit.  The loudness recurrence is loud_sample's (loudness_common.h)
// and the taps are true_peak_taps.h's, so the order of operations is the one-shot kernels' by construction.  Four kernels a
// stream: the hops (one lane per row), the call's true peak (one wave per row and chunk of output times), the advance (the
// only writer of N, the ring, the running peak and the hop count) and the read.  No atomics, no scratch memory, every store a
// plain vector store.  DESIGN.md §4.18.
#include "kernels.h"
#include "loudness_common.h"
#include "row_kernel_common.h"
#include "true_peak_taps.h"

#include "../../include/grail_hip.h"

#pragma clang fp contract(off)

namespace grail {

using namespace loud;

namespace {

// A row's state: METER_STREAM_STATE_WORDS 64-bit words.  Every double crosses a call as its 64 bits.
//   0: the state word of row_kernel_common.h (N)                1 .. 4: s1 .. s4     5: acc (of the hop the next sample lies in)
//   6: the running true peak                                    7: the hops completed, floor(N / H)
// Its ring: METER_STREAM_RING floats, sample s of the row at s mod 16, +0.0 where it was not finite; the last eleven count.
constexpr uint32_t METER_WORDS = METER_STREAM_STATE_WORDS;
constexpr uint32_t METER_RING = METER_STREAM_RING;
constexpr uint32_t METER_TAIL = 11;         // the outputs after a row's last sample: taps - 1
constexpr uint32_t METER_CHUNK = METER_STREAM_CHUNK;

__device__ __forceinline__ double meter_double(uint64_t w) { return __longlong_as_double((long long)w); }
__device__ __forceinline__ uint64_t meter_bits(double d) { return (uint64_t)__double_as_longlong(d); }

// What a call does to a row, read alike by the three kernels of the call (the advance kernel, last of them, is the only one
// that writes what this reads).
struct MeterRow {
    uint64_t fed, hops;     // N; the hops completed before the call
    uint32_t n, pos;        // the samples this call feeds the row; N mod H, where the row stands inside its hop
    uint32_t new_hops;      // the hops this call completes
    uint32_t count;         // the output times of the call's true peak: n, or the eleven of a finishing call
    bool takes, refused;    // the call changes the row's state; the row has ended and is fed, or would outgrow its ledger
};
__device__ __forceinline__ MeterRow meter_row(const uint64_t *__restrict__ state, const uint32_t *__restrict__ in_len,
                                              uint64_t in_stride, const uint8_t *__restrict__ mark, bool finishing, uint64_t u,
                                              uint32_t H, uint64_t max_hops)
{
    MeterRow r;
    const uint64_t *w = state + u * METER_WORDS;
    const uint64_t w0 = w[0];
    const bool ended = stream_ended(w0);
    r.fed = stream_fed(w0);
    r.hops = w[7];
    r.pos = (uint32_t)(r.fed - r.hops * H);
    if (finishing) {
        r.n = 0u;
        r.new_hops = 0u;
        r.refused = false;
        r.takes = !ended && (!mark || mark[u]);
        r.count = r.takes ? METER_TAIL : 0u;
    } else {
        const uint64_t n = in_len[u] < in_stride ? in_len[u] : in_stride;       // (never past the row, whatever in_len holds)
        r.n = (uint32_t)n;
        r.new_hops = (uint32_t)(((uint64_t)r.pos + n) / H);
        r.refused = (ended && n) || r.hops + r.new_hops > max_hops;
        r.takes = !ended && !r.refused;
        r.count = r.takes ? r.n : 0u;
    }
    return r;
}

// loud_load of loudness_kernels.hip (which stays as it is, to the letter): wave-instruction i reads samples [t0, t0 + 64) of
// the rows 4i .. 4i + 3 of the wave, whole 256-byte pieces of rows.  A row past the launch's last reads the last row; a group
// of four past the row's stride reads the row's last group: every load lies inside in[n_rows][in_stride] and none sits behind
// a branch.  What such a slot holds is no sample of the call and is never filtered into a state that is kept.
template <bool VEC>
__device__ __forceinline__ void meter_load(const float *__restrict__ rows, uint64_t row_stride, uint32_t n_rows, uint64_t row0,
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

// One wave = 64 rows, lane r = row row0 + r, over the call's samples in the one-shot kernel's tiles (64 x 64 through LDS at
// pitch 65, the next tile's loads issued before the current tile's arithmetic).  Each lane starts from its row's s1 .. s4 and
// acc at its own place N mod H inside its hop, writes a hop's sum when ITS hop ends (to the caller's array at the call's own
// count, to the ledger at the row's), and leaves the state it had after its own n-th sample: a lane is not stepped past its
// n, whatever the tile holds and however long the wave's longest row goes on.
// Two walks, the same bits.  UNIFORM: every row of the wave stands at the same N mod H and is fed the same n (a live mix: all
// rows fed the same chunk; the lanes past the launch's last row walk along and store nothing).  Then a hop's end is
// wave-uniform as in the one-shot kernel and the tile is walked in runs that end at the tile's, the call's or the hop's end,
// with no per-lane test on a sample.  Otherwise PREDICATED: a compare a sample (is it one of the lane's?) and one a sample for
// the hop's end, lanes that have had their n masked off; against 21 binary64 operations a sample.
// Reads N and the hop count, writes neither (meter_stream_advance_kernel, two launches behind, is their only writer).
template <bool VEC>
__global__ __launch_bounds__(64) void meter_stream_hops_kernel(const float *__restrict__ in, uint64_t in_stride,
                                                               const uint32_t *__restrict__ in_len, uint32_t n_rows, uint32_t H,
                                                               LoudCoef coef, uint64_t *__restrict__ state,
                                                               double *__restrict__ ledger, uint64_t max_hops,
                                                               double *__restrict__ hops_out, uint64_t hops_stride)
{
    __shared__ float tile[LOUD_ROWS * LOUD_PITCH];
    const uint32_t lane = threadIdx.x;
    const uint64_t row0 = (uint64_t)blockIdx.x * LOUD_ROWS;
    const uint64_t u = row0 + lane;
    const bool mine = u < n_rows;
    uint32_t n = 0u, pos = 0u;
    uint64_t hop_at = 0u;
    KState k = {0.0, 0.0, 0.0, 0.0, 0.0, 0u};
    uint64_t *const w = state + u * METER_WORDS;
    if (mine) {
        const MeterRow r = meter_row(state, in_len, in_stride, nullptr, false, u, H, max_hops);
        n = r.takes ? r.n : 0u;             // (an ended row, a refused one and a paused one: nothing filtered, nothing stored)
        pos = r.pos;
        hop_at = r.hops;
        k.s1 = meter_double(w[1]);
        k.s2 = meter_double(w[2]);
        k.s3 = meter_double(w[3]);
        k.s4 = meter_double(w[4]);
        k.acc = meter_double(w[5]);
    }
    const bool live = mine && n != 0u;
    // lane 0 is a row of the launch.  Do all rows of the wave stand where it stands and take what it takes?
    const uint32_t n0 = __builtin_amdgcn_readfirstlane(n), pos0 = __builtin_amdgcn_readfirstlane(pos);
    const bool uniform = __builtin_amdgcn_ballot_w64(!mine || (n == n0 && pos == pos0)) == ~0ull;
    uint32_t longest = n;
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {
        const uint32_t o = (uint32_t)__shfl_xor((int)longest, d, 64);
        longest = o > longest ? o : longest;
    }
    longest = __builtin_amdgcn_readfirstlane(longest);
    double *const my_ledger = ledger + u * max_hops + hop_at;
    double *const my_hops = hops_out + u * hops_stride;         // (not formed into an address that is used when hops_out is NULL)
    const float *mine_lds = tile + lane * LOUD_PITCH;
    float x[LOUD_LOADS][4];
    if (longest) {
        meter_load<VEC>(in, in_stride, n_rows, row0, 0, lane, x);
        loud_stash(tile, lane, x);
    }
    __syncthreads();
    uint32_t call_hop = 0u;                 // the hops this call has completed for the lane's row
    uint32_t upos = pos0;                   // UNIFORM: where every row stands inside its hop
    for (uint64_t t0 = 0; t0 < longest; t0 += LOUD_T) {
        const bool more = t0 + LOUD_T < longest;
        if (more) meter_load<VEC>(in, in_stride, n_rows, row0, t0 + LOUD_T, lane, x);
        const uint32_t wave_cnt = longest - t0 < LOUD_T ? (uint32_t)(longest - t0) : LOUD_T;      // of the longest row
        if (uniform) {
            uint32_t i = 0;
            while (i < wave_cnt) {
                const uint32_t left = H - upos;
                const uint32_t run = left < wave_cnt - i ? left : wave_cnt - i;
                uint32_t j = 0;
                for (; j + 8u <= run; j += 8u) {
#pragma unroll
                    for (uint32_t q = 0; q < 8u; ++q) loud_sample(mine_lds[i + j + q], false, coef.c, k);
                }
                for (; j < run; ++j) loud_sample(mine_lds[i + j], false, coef.c, k);
                i += run;
                upos += run;
                if (upos == H) {
                    if (mine) {
                        if (hops_out) my_hops[call_hop] = k.acc;
                        my_ledger[call_hop] = k.acc;
                    }
                    k.acc = 0.0;
                    upos = 0u;
                    ++call_hop;
                }
            }
        } else {
            const uint32_t cnt = n > t0 ? (n - t0 < LOUD_T ? (uint32_t)(n - t0) : LOUD_T) : 0u;     // of the lane's own row
#pragma unroll 8
            for (uint32_t i = 0; i < wave_cnt; ++i) {
                if (i < cnt) {
                    loud_sample(mine_lds[i], false, coef.c, k);
                    if (++pos == H) {
                        if (hops_out) my_hops[call_hop] = k.acc;
                        my_ledger[call_hop] = k.acc;
                        k.acc = 0.0;
                        pos = 0u;
                        ++call_hop;
                    }
                }
            }
        }
        __syncthreads();                                // every lane has read the tile
        if (more) loud_stash(tile, lane, x);
        __syncthreads();
    }
    if (live) {
        w[1] = meter_bits(k.s1);
        w[2] = meter_bits(k.s2);
        w[3] = meter_bits(k.s3);
        w[4] = meter_bits(k.s4);
        w[5] = meter_bits(k.acc);
    }
}

// One wave = one (row, chunk of METER_CHUNK of the call's output times), as true_peak_frames_kernel: lane l of a step of 256
// outputs owns four, at the call's own indexes i0 .. i0 + 3 (output time N + i0 ..), and needs the samples i0 - 11 .. i0 + 3.
// Index i >= 0 is the call's sample i; below 0 it is the row's sample N + i out of the ring (+0.0 before the row's first
// sample), which only the first step of chunk 0 reaches; from n on it is +0.0 (a finishing call: the samples to come).  Every
// index is clamped into the call's n samples before it is loaded, a group of four into the row's groups: every load is in
// bounds and none sits behind a divergent branch.  A sample is counted where it is an output's own (i0 .. i0 + 3): once.
template <bool VEC>
__global__ __launch_bounds__(256) void meter_stream_peak_kernel(const float *__restrict__ in, uint64_t in_stride,
                                                                const uint32_t *__restrict__ in_len, uint32_t n_rows, uint32_t H,
                                                                const uint64_t *__restrict__ state, uint64_t max_hops,
                                                                const float *__restrict__ ring, const uint8_t *__restrict__ mark,
                                                                uint32_t finishing, uint32_t grid_chunks,
                                                                double *__restrict__ cmax, uint32_t *__restrict__ cbad)
{
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t wv = (uint64_t)blockIdx.x * 4u + wave;
    const uint64_t u = wv / grid_chunks;
    if (u >= n_rows) return;
    const uint32_t c = (uint32_t)(wv - u * grid_chunks);
    const MeterRow r = meter_row(state, in_len, in_stride, mark, finishing != 0u, u, H, max_hops);
    const uint64_t start = (uint64_t)c * METER_CHUNK;
    if (start >= r.count) return;                                       // chunks past the call's last: nothing written
    const uint32_t count = r.count - start < METER_CHUNK ? (uint32_t)(r.count - start) : METER_CHUNK;
    const float *row = in + u * in_stride;                              // (not read when n = 0)
    const float *hist = ring + u * METER_RING;
    const int64_t n = (int64_t)r.n;
    double best = 0.0;
    uint32_t bad = 0u;
    for (uint32_t s = 0; s < count; s += 256u) {
        const int64_t i0 = (int64_t)(start + s + 4u * lane);
        float x[16];
#pragma unroll
        for (int j = 0; j < 16; ++j) x[j] = 0.0f;
        if (n) {
            if (VEC) {
                // the call's last group starts below n <= in_stride, a multiple of 4: inside the row
                const int64_t g_hi = (n - 1) >> 2;
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    int64_t g = (i0 >> 2) - 3 + q;
                    g = g < 0 ? 0 : g;
                    g = g > g_hi ? g_hi : g;
                    const float4 v = *reinterpret_cast<const float4 *>(row + 4 * g);
                    x[4 * q + 0] = v.x;
                    x[4 * q + 1] = v.y;
                    x[4 * q + 2] = v.z;
                    x[4 * q + 3] = v.w;
                }
            } else {
#pragma unroll
                for (int j = 1; j < 16; ++j) {
                    int64_t i = i0 - 12 + j;
                    i = i < 0 ? 0 : i;
                    i = i > n - 1 ? n - 1 : i;
                    x[j] = row[i];
                }
            }
        }
        if (start + s == 0u) {                                          // (wave-uniform) the seam between the ring and the call
#pragma unroll
            for (int j = 1; j < 12; ++j) {
                const int64_t i = i0 - 12 + j;
                const int64_t at = (int64_t)r.fed + i;                  // the row's own sample index
                const float old = hist[(uint32_t)at & (METER_RING - 1u)];
                x[j] = i < 0 ? (at >= 0 ? old : 0.0f) : x[j];
            }
        }
        double v[16];
#pragma unroll
        for (int j = 1; j < 16; ++j) {
            const int64_t i = i0 - 12 + j;
            const bool finite = finite_f32(x[j]);
            if (j >= 12) bad += (i < n && !finite) ? 1u : 0u;           // (the lane's own four; what the ring holds is finite)
            v[j] = (double)((i < n && finite) ? x[j] : 0.0f);
        }
        // C * v is exact (a 13-bit numerator times a 24-bit significand), so the fused multiply-add is the contract's multiply
        // and add
#pragma unroll
        for (int out = 0; out < 4; ++out) {
            double y[4];
#pragma unroll
            for (int p = 0; p < 4; ++p) {
                double acc = 0.0;
#pragma unroll
                for (int kk = 0; kk < 12; ++kk) acc = __builtin_fma(true_peak_tap(p, kk), v[12 + out - kk], acc);
                y[p] = __builtin_fabs(acc);
            }
            const double peak = __builtin_fmax(__builtin_fmax(y[0], y[1]), __builtin_fmax(y[2], y[3]));
            // an output past the call's last is another call's, or nobody's
            best = __builtin_fmax(best, s + 4u * lane + (uint32_t)out < count ? peak : 0.0);
        }
    }
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {
        best = __builtin_fmax(best, __shfl_xor(best, d, 64));
        bad += (uint32_t)__shfl_xor((int)bad, d, 64);
    }
    if (lane == 0u) {
        const uint64_t at = u * grid_chunks + c;
        cmax[at] = best;
        cbad[at] = bad;
    }
}

// Behind the two on the stream, one wave per row, the only writer of N, the ring, the running peak and the hop count: the
// call's numbers from its chunks, the call's last min(n, 11) samples into the ring at (N + t) mod 16, then N + n and the hops
// (a finishing call: the row ended).  A refused row: GRAIL_LIMIT_REFUSED, NaN, 0, its state as it was.  No LDS.
__global__ __launch_bounds__(256) void meter_stream_advance_kernel(const float *__restrict__ in, uint64_t in_stride,
                                                                   const uint32_t *__restrict__ in_len, uint32_t n_rows, uint32_t H,
                                                                   uint64_t *__restrict__ state, uint64_t max_hops,
                                                                   float *__restrict__ ring, const uint8_t *__restrict__ mark,
                                                                   uint32_t finishing, const double *__restrict__ cmax,
                                                                   const uint32_t *__restrict__ cbad, uint32_t grid_chunks,
                                                                   uint32_t *__restrict__ n_hops, double *__restrict__ true_peak,
                                                                   uint32_t *__restrict__ nonfinite)
{
    const uint64_t u = (uint64_t)blockIdx.x * 4u + (threadIdx.x >> 6);
    const uint32_t lane = threadIdx.x & 63u;
    if (u >= n_rows) return;
    const MeterRow r = meter_row(state, in_len, in_stride, mark, finishing != 0u, u, H, max_hops);
    if (r.refused) {
        if (lane == 0u) {
            refuse_counts(n_hops, nonfinite, u);
            if (true_peak) true_peak[u] = meter_double(0x7FF8000000000000ull);
        }
        return;
    }
    double m = 0.0;
    uint32_t bad = 0u;
    if (r.count) {
        const uint32_t chunks = (r.count + METER_CHUNK - 1u) / METER_CHUNK;
        for (uint32_t c = lane; c < chunks; c += 64u) {
            m = __builtin_fmax(m, cmax[u * grid_chunks + c]);
            bad += cbad[u * grid_chunks + c];
        }
    }
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {
        m = __builtin_fmax(m, __shfl_xor(m, d, 64));
        bad += (uint32_t)__shfl_xor((int)bad, d, 64);
    }
    const bool moves = r.takes && (r.n != 0u || finishing != 0u);
    if (moves && r.n)
        ring_keep(in + u * in_stride, r.n, (uint32_t)r.fed, ring + u * METER_RING, METER_RING, METER_TAIL, lane);
    if (lane != 0u) return;
    if (n_hops) n_hops[u] = r.new_hops;
    if (true_peak) true_peak[u] = m;
    if (nonfinite) nonfinite[u] = bad;
    if (moves) {
        uint64_t *w = state + u * METER_WORDS;
        w[6] = meter_bits(__builtin_fmax(meter_double(w[6]), m));
        w[7] = r.hops + r.new_hops;
        w[0] = finishing ? (r.fed | STREAM_ENDED) : r.fed + r.n;
    }
}

// What a meter shows of a row at this moment, one lane per row: the gate over the ledger's hops (loudness_gate_kernel's
// arithmetic restated: that kernel takes lengths, and a stream's hops x H does not fit its 32 bits), the last block of four
// hops and the last of thirty, the running peak and the count.  It changes no state.
__global__ __launch_bounds__(256) void meter_stream_read_kernel(const uint64_t *__restrict__ state, uint32_t n_rows, uint32_t H,
                                                                const double *__restrict__ ledger, uint64_t max_hops,
                                                                double *__restrict__ integrated, double *__restrict__ momentary,
                                                                double *__restrict__ short_term, double *__restrict__ true_peak,
                                                                uint64_t *__restrict__ hops_out)
{
    const uint64_t u = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (u >= n_rows) return;
    const uint64_t *w = state + u * METER_WORDS;
    const uint64_t n_hops = w[7];
    const double *h = ledger + u * max_hops;
    if (true_peak) true_peak[u] = meter_double(w[6]);
    if (hops_out) hops_out[u] = n_hops;
    if (short_term) {
        double s = 0.0;
        if (n_hops >= 30u) {
            const double *b = h + (n_hops - 30u);
            s = b[0];
            for (uint32_t j = 1; j < 30u; ++j) s = s + b[j];
            s = s / (30.0 * (double)H);
        }
        short_term[u] = s;
    }
    const double per = 4.0 * (double)H;
    if (momentary) {
        double z = 0.0;
        if (n_hops >= 4u) {
            const uint64_t j = n_hops - 4u;
            z = (((h[j] + h[j + 1]) + h[j + 2]) + h[j + 3]) / per;
        }
        momentary[u] = z;
    }
    if (!integrated) return;
    if (n_hops < 4u) {
        integrated[u] = 0.0;
        return;
    }
    const uint64_t blocks = n_hops - 3u;
    double sum = 0.0;
    uint64_t count = 0;
    for (uint64_t j = 0; j < blocks; ++j) {
        const double z = (((h[j] + h[j + 1]) + h[j + 2]) + h[j + 3]) / per;
        if (z > GRAIL_LOUDNESS_ABS_GATE) {
            sum = sum + z;
            ++count;
        }
    }
    if (count == 0u) {
        integrated[u] = 0.0;
        return;
    }
    const double rel = 0.1 * (sum / (double)count);
    sum = 0.0;
    count = 0;
    for (uint64_t j = 0; j < blocks; ++j) {
        const double z = (((h[j] + h[j + 1]) + h[j + 2]) + h[j + 3]) / per;
        if (z > GRAIL_LOUDNESS_ABS_GATE && z > rel) {
            sum = sum + z;
            ++count;
        }
    }
    integrated[u] = count ? sum / (double)count : 0.0;
}

}  // namespace

hipError_t launch_meter_stream_hops(const MeterStreamArgs &a, hipStream_t stream)
{
    if (a.n_rows == 0 || a.row_stride == 0) return hipSuccess;
    LoudCoef coef;
    for (int i = 0; i < 10; ++i) coef.c[i] = a.coef[i];
    launch_either(aligned16(a.rows, a.row_stride), meter_stream_hops_kernel<true>, meter_stream_hops_kernel<false>,
                  dim3((a.n_rows + LOUD_ROWS - 1u) / LOUD_ROWS), dim3(64), 0, stream, a.rows, a.row_stride, a.len, a.n_rows, a.hop, coef,
                  a.state, a.ledger, a.max_hops, a.hops_out, a.hops_stride);
    return hipGetLastError();
}

hipError_t launch_meter_stream_peak(const MeterStreamArgs &a, hipStream_t stream)
{
    const uint64_t groups = ((uint64_t)a.n_rows * a.grid_chunks + 3u) / 4u;        // (four waves, one a (row, chunk), to a workgroup)
    hipError_t e;
    if (!grid_fits(groups, &e)) return e;
    launch_either(a.finishing || aligned16(a.rows, a.row_stride), meter_stream_peak_kernel<true>, meter_stream_peak_kernel<false>,
                  dim3((uint32_t)groups), dim3(256), 0, stream, a.rows, a.row_stride, a.len, a.n_rows, a.hop, a.state, a.max_hops, a.ring,
                  a.mark, a.finishing ? 1u : 0u, a.grid_chunks, a.cmax, a.cbad);
    return hipGetLastError();
}

hipError_t launch_meter_stream_advance(const MeterStreamArgs &a, hipStream_t stream)
{
    if (a.n_rows == 0) return hipSuccess;
    hipLaunchKernelGGL(meter_stream_advance_kernel, dim3(a.n_rows / 4u + (a.n_rows % 4u != 0u)), dim3(256), 0, stream, a.rows,
                       a.row_stride, a.len, a.n_rows, a.hop, a.state, a.max_hops, a.ring, a.mark, a.finishing ? 1u : 0u, a.cmax, a.cbad,
                       a.grid_chunks, a.n_hops, a.true_peak, a.nonfinite);
    return hipGetLastError();
}

hipError_t launch_meter_stream_read(const uint64_t *state, uint32_t n_rows, uint32_t hop, const double *ledger, uint64_t max_hops,
                                    double *integrated, double *momentary, double *short_term, double *true_peak, uint64_t *hops_out,
                                    hipStream_t stream)
{
    if (n_rows == 0) return hipSuccess;
    hipLaunchKernelGGL(meter_stream_read_kernel, dim3((n_rows + 255u) / 256u), dim3(256), 0, stream, state, n_rows, hop, ledger,
                       max_hops, integrated, momentary, short_term, true_peak, hops_out);
    return hipGetLastError();
}

}  // namespace grail
