// true_peak_taps.h — the 4x oversampling filter of ITU-R BS.1770-4 Annex 2 as include/grail_hip.h ("levels, continued:
// true peak") states it: four phases of twelve taps, C[p][k] = N[p][k] / 8192 with integer numerators; phases 2 and 3
// are phases 1 and 0 reversed.  Shared by the kernel (true_peak_kernels.hip) and grail_true_peak_coefficients
// (level_gains.cpp, pure host), so that the two cannot drift apart.
#pragma once

namespace grail {

// (a 13-bit numerator over 2^13: exact in binary64.  The numerators are locals so that host and device code both see them.)
constexpr double true_peak_tap(int p, int k)
{
    const int n0[12] = {14, 90, -161, 272, -487, 1125, 7964, -838, 390, -218, 122, -68};
    const int n1[12] = {-239, 240, -424, 730, -1364, 3810, 6388, -1641, 832, -477, 271, -155};
    return (double)(p == 0 ? n0[k] : p == 1 ? n1[k] : p == 2 ? n1[11 - k] : n0[11 - k]) / 8192.0;
}

}  // namespace grail
