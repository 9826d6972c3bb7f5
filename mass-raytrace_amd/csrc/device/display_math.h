// display_math.h — the Rust scalar semantics the display code restates
// (main.rs:640-722), shared by passes.hip (tonemap) and denoise.hip.
#pragma once
#include <stdint.h>

#include "devbase.h"

namespace mrt {

// Rust f32::min/max (the non-NaN operand wins) and saturating `as u8`.
MRT_DEV float rs_min(float a, float b) { return a != a ? b : (b != b ? a : (a < b ? a : b)); }
MRT_DEV float rs_max(float a, float b) { return a != a ? b : (b != b ? a : (a > b ? a : b)); }
MRT_DEV uint32_t rs_u8(float v) { return !(v > 0.0f) ? 0u : (v >= 255.0f ? 255u : (uint32_t)v); }

}  // namespace mrt
