// Snake1d(x) = x + sin(alpha x)^2 / (alpha + 1e-9), the codec's activation, fused into the input staging of every DAC convolution
// (umoe_dac.hip, umoe_dac_mfma.hip).  One definition so that the direct and the MFMA kernels feed their sums the same fp32 values.
#pragma once

namespace {
__device__ __forceinline__ float snake(float v, float a) {
    const float s = __sinf(a * v);
    return v + s * s / (a + 1e-9f);
}
}  // namespace
