// What the weight gradients of the 3x3 gather convolutions share; gfx950 only.  Users: dconv.hip (dconv_wgrad_kernel: the dilated
// convolutions of the ContextNetwork in training) and dense_train.hip (dense_wgrad_kernel: a layer of the dense estimators, and
// the head's gradient): the step and chunk-plane constants, the pixel ranges (wgrad_plan) and the ordered reduce of the partials.
// The two kernels' loops are described in dconv.hip; they are still two copies (DESIGN.md 4.27 says why).
#pragma once
#include "ctx_common.h"

namespace dmc {
namespace ctxk {

constexpr int KP = 32;                       // pixels per step
constexpr int PLANE = KP * 32 + 128;         // bytes between chunk planes: = 128 (mod 256)
constexpr int NCHUNK = 8;                    // 16-channel chunks of the widest operand (128 channels)
constexpr int TILE_BYTES = 3 * NCHUNK * PLANE;
constexpr int MAX_RANGES = 64;               // pixel ranges of a small tensor (x 9 taps workgroups)
constexpr int MAX_RANGE_STEPS = 256;         // ... and of a large one: a range is at most 8 k pixels, so that one fp32 accumulator
                                             // never carries a longer sum (42 x 448^2 in 64 ranges of 131 k pixels: 1.4e-5 off)

struct WgPlan { int steps, ranges, per_range; };
inline WgPlan wgrad_plan(int N, int H, int W) {
    WgPlan p;
    const int M = N * H * W;
    p.steps = (M + KP - 1) / KP;
    int r = p.steps < MAX_RANGES ? p.steps : MAX_RANGES;
    p.per_range = (p.steps + r - 1) / r;
    if (p.per_range > MAX_RANGE_STEPS) p.per_range = MAX_RANGE_STEPS;
    p.ranges = (p.steps + p.per_range - 1) / p.per_range;
    return p;
}

// out[i] = the partials' element i added in order; one thread per element
static __global__ __launch_bounds__(256) void ordered_reduce_kernel(const float* __restrict__ part, float* __restrict__ out, int nparts, long numel) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= numel) return;
    float s = part[i];
    for (int k = 1; k < nparts; ++k) s += part[(size_t)k * numel + i];
    out[i] = s;
}

}  // namespace ctxk
}  // namespace dmc
