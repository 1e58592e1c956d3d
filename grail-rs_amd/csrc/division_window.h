// division_window.h — the operand window of the short exact division (div_exact<true>, rcp_exact<true> in
// device_common.h), in one place for the device gate (pair_is_safe, blend_div_ok, clk_floor) and its host copies
// (live4_elems_ok, scan_elems_ok, the pitch tests of the planner).  The scan kernel has no IEEE fallback: for it the
// host copies are the only gate, so the two sides must read the same numbers.
// A formant frequency x and bandwidth w pass when, with jm = JITTER_MARGIN * |jitter_delta_formant_frequency|,
//   x * MARGIN_DOWN - jm >= X_LO,  x * MARGIN_UP + jm <= X_HI,  W_LO <= w <= W_HI
// (one rounding per operation, binary32); a pitch f with jf = JITTER_MARGIN * |jitter_delta_frequency| when
//   f * MARGIN_DOWN - jf >= X_LO,  f * MARGIN_UP + jf <= PITCH_HI.
// tests/division_window_cases.py restates this and tests/test_division_window_*.py hold both sides of every bound to
// the oracle.
#pragma once

namespace grail {
namespace window {

constexpr float X_LO = 9.5367431640625e-07f;          // 2^-20
constexpr float X_HI = 0.5f - 9.5367431640625e-07f;
constexpr float W_LO = 1.8189894035458565e-12f;       // 2^-39 (2x margin over 2^-40)
constexpr float W_HI = 512.0f;                        // 2^9   (2x margin under 2^10)
constexpr float PITCH_HI = 1.0f;
constexpr float MARGIN_DOWN = 0.999f;                 // the blend and the jitter's interpolation round a few times
constexpr float MARGIN_UP = 1.001f;
constexpr float JITTER_MARGIN = 1.002f;               // the jitter noise is in [-1, 1] up to its own roundings
// clk / blend_length by the short division: the blend length, the segment length and the clock step inside
// [BLEND_LO, BLEND_HI]; a clock below BLEND_LO takes the general step
constexpr float BLEND_LO = 0x1p-59f;
constexpr float BLEND_HI = 0x1p59f;

}  // namespace window
}  // namespace grail
