// loudness_common.h — what the two K-weighting kernels share (loudness_kernels.hip: one lane per row;
// loudness_segment_kernels.hip: one lane per hop): the tile's shape in LDS, the filter's state and one sample through
// both sections in the contract's order (include/grail_hip.h, "levels, continued").  Device code only.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "row_kernel_common.h"

#pragma clang fp contract(off)

namespace grail {
namespace loud {

constexpr uint32_t LOUD_ROWS = 64;          // rows of a tile = lanes of the wave
constexpr uint32_t LOUD_T = 64;             // samples of a tile per row: 256 B of a row, 16 lanes x 16 B
constexpr uint32_t LOUD_PITCH = LOUD_T + 1; // floats between two rows of the tile in LDS: lane r reads word 65 r + t, bank
                                            // (r + t) mod 32, all distinct inside each half-wave
constexpr uint32_t LOUD_LOADS = LOUD_ROWS * LOUD_T / (64 * 4);      // 16-byte loads per lane and tile: 16

// a tile's loads on their way into LDS, transposed: tile[row][sample] at pitch 65
__device__ __forceinline__ void loud_stash(float *tile, uint32_t lane, const float (&x)[LOUD_LOADS][4])
{
#pragma unroll
    for (uint32_t i = 0; i < LOUD_LOADS; ++i) {
        float *dst = tile + (4u * i + (lane >> 4)) * LOUD_PITCH + 4u * (lane & 15u);
#pragma unroll
        for (uint32_t k = 0; k < 4; ++k) dst[k] = x[i][k];
    }
}

struct KState {
    double s1, s2, s3, s4, acc;
    uint32_t bad;
};

// one sample through both sections, in the contract's order
__device__ __forceinline__ void loud_sample(float xf, bool counted, const double (&c)[10], KState &k)
{
    const bool finite = finite_f32(xf);
    k.bad += (counted && !finite) ? 1u : 0u;
    const double v = finite ? (double)xf : 0.0;
    const double y = c[0] * v + k.s1;
    k.s1 = (c[1] * v - c[3] * y) + k.s2;
    k.s2 = c[2] * v - c[4] * y;
    const double z = c[5] * y + k.s3;
    k.s3 = (c[6] * y - c[8] * z) + k.s4;
    k.s4 = c[7] * y - c[9] * z;
    k.acc = k.acc + z * z;
}

struct LoudCoef {
    double c[10];
};

}  // namespace loud
}  // namespace grail
