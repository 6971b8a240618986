// What the host-side launch plans (conv_plan.h, roi_plan.h) assume about the chip.  Host-only: no HIP.
#pragma once

namespace i2v {
constexpr int NUM_CU = 256;     // compute units of an MI355X (8 XCDs x 32)
}  // namespace i2v
