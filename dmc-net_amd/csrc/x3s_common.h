// Transfer addressing shared by the weight-gradient kernels of the pre-split bf16x3 convolutions (conv_x3s.hip, conv_x3q.hip);
// gfx950 only.  The split, the MFMA wrappers, the buffer transfers and the transposed reads they use are mma_bf16.h's.
#pragma once
#include "dmc_common.h"

namespace dmc {
namespace x3 {

// ---- transfer addressing of the weight-gradient kernels (x3s_wgrad_kernel, x3q_wgrad_kernel) ------------------------------
// Both walk the pixels in groups of R padded image rows (HP rows per image, HP % R == 0: a group never straddles two images).
// A lane's pixel within the group -- its row r and its column -- is the same in every step; only the group moves, and the
// group is wave-uniform.  So the lane keeps ONE constant per transfer, pre = (r W + col) 32 + lane half (NOPIX where the column
// is outside the image or the slot beyond the tile), and a step adds the scalar in-image base of its group:
//     t = ((y0 - 1) W) 32 + pre       (y0 = the group's first padded row within its image; row y0 - 1 + r of the image)
// t grows with (row, column) and the column is in range, so "the row is an image row" is 0 <= t < H W 32 as ONE unsigned
// compare: add, compare, select per transfer, no division.  The image's own byte offset n H W 32 goes into the scalar offset
// of the transfer.  A group outside the tensor (q = -1 in the prologue, n >= N behind the last image) gets the base NOPIX.
// NOPIX + any base or pre stays above every image size (an image plane is far below 2^30 bytes: plane_bytes is 32 bit).
constexpr unsigned NOPIX = 0x40000000u;

struct WgGroupPos { int n, y; };                 // padded row R q = row y of image n; carried from step to step in scalar registers
__device__ __forceinline__ WgGroupPos wg_group_at(int q, int R, int HP) {      // one scalar division, before the step loop
    const int g = R * q, n = g / HP;
    WgGroupPos p;
    p.n = __builtin_amdgcn_readfirstlane(n);
    p.y = __builtin_amdgcn_readfirstlane(g - n * HP);
    return p;
}
__device__ __forceinline__ WgGroupPos wg_group_next(WgGroupPos p, int R, int HP) {
    p.y += R;
    if (p.y >= HP) { p.y -= HP; ++p.n; }
    return p;
}
__device__ __forceinline__ WgGroupPos wg_group_prev(WgGroupPos p, int R, int HP) {
    p.y -= R;
    if (p.y < 0) { p.y += HP; --p.n; }
    return p;
}
// scalar parts of a group's transfers: in-image base of row y - 1 (or NOPIX) and the image's byte offset within a plane
__device__ __forceinline__ void wg_group_base(const WgGroupPos& p, int N, int W, unsigned img_bytes, unsigned& tbase, unsigned& img_off) {
    const bool in = p.n >= 0 && p.n < N;
    tbase = in ? (unsigned)((p.y - 1) * W) * 32u : NOPIX;
    img_off = in ? (unsigned)p.n * img_bytes : 0u;
}
__device__ __forceinline__ unsigned wg_lane_off(unsigned tbase, unsigned pre, unsigned img_bytes) {
    const unsigned t = tbase + pre;
    return t < img_bytes ? t : OOB;
}

}  // namespace x3
}  // namespace dmc
