// Device helpers shared by the pre-split bf16x3 convolution kernels (conv_x3s.hip, conv_x3q.hip); gfx950 only.
#pragma once
#include "dmc_common.h"

namespace dmc {
namespace x3 {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
typedef const __attribute__((address_space(3))) char* lds_cptr;

__device__ __forceinline__ f32x16 mfma_bf16(const u32x4& a, const u32x4& b, const f32x16& c) {
    return __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c, 0, 0, 0);
}

// fp32 -> three bf16 slices (truncation split: s0 = upper 16 bits, s1 = upper 16 bits of the exact remainder, s2 = the rest)
__device__ __forceinline__ void split3(float v, unsigned& u0, unsigned& u1, unsigned& u2) {
    u0 = __float_as_uint(v);
    const float r1 = v - __uint_as_float(u0 & 0xffff0000u);
    u1 = __float_as_uint(r1);
    u2 = __float_as_uint(r1 - __uint_as_float(u1 & 0xffff0000u));
}
__device__ __forceinline__ unsigned pack_hi(unsigned hi_of_second, unsigned hi_of_first) {   // (upper half of b, upper half of a)
    return __builtin_amdgcn_perm(hi_of_second, hi_of_first, 0x07060302u);
}

constexpr unsigned OOB = 0x80000000u;          // a transfer offset beyond num_records: the lane's 16 bytes arrive as zeros

// 16 bytes per lane global -> LDS through a buffer descriptor (range-checked: offsets >= num_records write zeros).
// LDS destination = lds_byte_addr + 16 * lane.  srd / soff / lds_byte_addr must be wave-uniform; the s_nops cover the
// M0 -> LDS-DMA wait state and an SGPR written by v_readfirstlane just in front of the statement.
__device__ __forceinline__ void dma_buf16(const u32x4& srd, unsigned voff, unsigned soff, unsigned lds_byte_addr) {
    asm volatile("s_mov_b32 m0, %2\n\ts_nop 3\n\tbuffer_load_dwordx4 %0, %1, %3 offen lds"
                 :: "v"(voff), "s"(srd), "s"(lds_byte_addr), "s"(soff) : "memory");
}
__device__ __forceinline__ u32x4 make_srd(const void* base) {
    const unsigned long long b = (unsigned long long)base;
    u32x4 srd;
    srd[0] = __builtin_amdgcn_readfirstlane((unsigned)b);
    srd[1] = __builtin_amdgcn_readfirstlane((unsigned)(b >> 32) & 0xffffu);
    srd[2] = 0x7fffffffu;
    srd[3] = 0x00020000u;
    return srd;
}

// ds_read_b64_tr_b16: a 16-lane group hands in the addresses of a [4 pixels][16 channels] block (lane L: pixel L / 4,
// channels 4 (L % 4) ..) and lane i receives channel i of the four pixels; two reads = eight consecutive k-values
typedef short s16x4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ void tr_read2(lds_cptr p0, lds_cptr p1, u32x4& f) {   // eight k-values = two transposed reads
    const s16x4 a = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)p0);
    const s16x4 b = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)p1);
    typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
    const u32x2 ua = __builtin_bit_cast(u32x2, a), ub = __builtin_bit_cast(u32x2, b);
    f[0] = ua[0]; f[1] = ua[1]; f[2] = ub[0]; f[3] = ub[1];
}

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

// ---- v_mfma_f32_16x16x32_bf16 users (conv_small.hip, gen_x3.hip) -----------------------------------------------------
typedef float f32x4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ f32x4 mfma16(const u32x4& a, const u32x4& b, const f32x4& c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c, 0, 0, 0);
}

// eight fp32 values -> three bf16x8 fragments (truncation split, as split3)
__device__ __forceinline__ void split8(const float4& lo, const float4& hi, u32x4& s0, u32x4& s1, u32x4& s2) {
    const float v[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
    unsigned u0[8], u1[8], u2[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) split3(v[e], u0[e], u1[e], u2[e]);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        s0[e] = pack_hi(u0[2 * e + 1], u0[2 * e]);
        s1[e] = pack_hi(u1[2 * e + 1], u1[2 * e]);
        s2[e] = pack_hi(u2[2 * e + 1], u2[2 * e]);
    }
}

}  // namespace x3
}  // namespace dmc
