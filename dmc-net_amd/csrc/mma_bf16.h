// Device primitives every bf16 matrix-core kernel of the library is written on (gfx950 only): the vector types, the bf16x3
// split of an fp32 value, the two bf16 MFMA wrappers, the LDS-DMA transfers, the transposed LDS read and the split-K reduce.
// Each exists ONCE, here; dmc_common.h includes this file.
#pragma once
#include <hip/hip_runtime.h>

namespace dmc {

// ---- vector types ------------------------------------------------------------------------------------------------------
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef short s16x4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) void* lds_ptr_t;
typedef const __attribute__((address_space(3))) char* lds_cptr;
__device__ __forceinline__ unsigned lds_addr_of(const void* p) { return (unsigned)(size_t)(lds_ptr_t)p; }

// ---- fp32 products from bf16 matrix-core instructions ("bf16x3") -------------------------------------------------------
// An fp32 value is the exact sum of three bf16 values: s0 = its upper 16 bits (sign, exponent, 7 mantissa bits:
// 8 significant bits, truncated), s1 = the upper 16 bits of the (exact) remainder, s2 = the second remainder,
// which has at most 8 significant bits left and is therefore a bf16 value itself.  The product of two such
// sums is formed from six of the nine slice products, (0,0) (0,1) (1,0) (0,2) (2,0) (1,1) -- each one exact in
// the fp32 accumulator's input precision -- and the three omitted ones are below 2^-23 of |a||b|, the size of
// one fp32 rounding of the product.  v_mfma_f32_32x32x16_bf16 retires 16 k-values per 32 cycles where
// v_mfma_f32_32x32x2_f32 retires 2 per 64: six of them per 16 k-values are 2.67x the fp32 instruction's rate.
// (Inf inputs become NaN, values below 2^-110 lose their low slices: neither occurs in a finite training run.)
// The ORDER in which a kernel adds its six products is that kernel's own and is documented there.

// the split as three raw words: slice k is the UPPER half of uk (the lower halves are what the next slice starts from)
__device__ __forceinline__ void split3(float v, unsigned& u0, unsigned& u1, unsigned& u2) {
    u0 = __float_as_uint(v);
    const float r1 = v - __uint_as_float(u0 & 0xffff0000u);
    u1 = __float_as_uint(r1);
    u2 = __float_as_uint(r1 - __uint_as_float(u1 & 0xffff0000u));
}
// the split as three 16-bit slices (the weight / input pack kernels, which store one bf16 per slice plane)
__device__ __forceinline__ void split3_bf16(float v, unsigned& s0, unsigned& s1, unsigned& s2) {
    unsigned u0, u1, u2;
    split3(v, u0, u1, u2);
    s0 = u0 >> 16; s1 = u1 >> 16; s2 = u2 >> 16;
}
// two bf16 in a dword as the MFMA operands want them: (upper half of the second word, upper half of the first)
__device__ __forceinline__ unsigned pack_hi(unsigned hi_of_second, unsigned hi_of_first) {
    return __builtin_amdgcn_perm(hi_of_second, hi_of_first, 0x07060302u);
}
// eight consecutive fp32 values -> three bf16x8 MFMA fragments
__device__ __forceinline__ void split8(const float (&v)[8], u32x4& s0, u32x4& s1, u32x4& s2) {
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
__device__ __forceinline__ void split8(const float4& lo, const float4& hi, u32x4& s0, u32x4& s1, u32x4& s2) {
    const float v[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
    split8(v, s0, s1, s2);
}
// the same as one value (the kernels that keep the fragments of several tiles in an array)
struct Split3 { u32x4 s[3]; };
__device__ __forceinline__ Split3 split8(const float (&v)[8]) {
    Split3 r;
    split8(v, r.s[0], r.s[1], r.s[2]);
    return r;
}
__device__ __forceinline__ Split3 split8(const f32x4& lo, const f32x4& hi) {
    const float v[8] = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
    return split8(v);
}
__device__ __forceinline__ Split3 split8(const float4& lo, const float4& hi) {
    const float v[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
    return split8(v);
}
// four consecutive values -> three 8-byte pieces (x3s_store4: the epilogues whose lanes hold four channels of a pixel)
struct Split3x2 { u32x2 s[3]; };
__device__ __forceinline__ Split3x2 split4(const float (&v)[4]) {
    unsigned u0[4], u1[4], u2[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) split3(v[e], u0[e], u1[e], u2[e]);
    Split3x2 r;
#pragma unroll
    for (int e = 0; e < 2; ++e) {
        r.s[0][e] = pack_hi(u0[2 * e + 1], u0[2 * e]);
        r.s[1][e] = pack_hi(u1[2 * e + 1], u1[2 * e]);
        r.s[2][e] = pack_hi(u2[2 * e + 1], u2[2 * e]);
    }
    return r;
}

// ---- bf16 MFMAs on u32x4 fragments (eight bf16 each) -------------------------------------------------------------------
__device__ __forceinline__ f32x16 mfma_bf16(const u32x4& a, const u32x4& b, const f32x16& c) {      // v_mfma_f32_32x32x16_bf16
    return __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c, 0, 0, 0);
}
__device__ __forceinline__ f32x4 mfma16(const u32x4& a, const u32x4& b, const f32x4& c) {           // v_mfma_f32_16x16x32_bf16
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c, 0, 0, 0);
}

// ---- LDS-DMA: global -> LDS without staging registers ------------------------------------------------------------------
// Through inline assembly: the compiler then inserts no vmcnt(0) in front of unrelated ds_reads; completion is tracked by
// hand with s_waitcnt vmcnt.  The LDS destination is lds_byte_addr + (bytes per lane) * lane; lds_byte_addr is wave-uniform.
// 16 bytes per lane, address = 64-bit scalar base + 32-bit per-lane byte offset (the address arithmetic stays on the SALU)
// (lds_dma16_sgpr: for an lds_byte_addr the compiler already keeps in a scalar register; lds_dma16 makes it one)
__device__ __forceinline__ void lds_dma16_sgpr(unsigned long long sbase, unsigned voff, unsigned lds_byte_addr) {
    asm volatile("s_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, %1"
                 :: "v"(voff), "s"(sbase), "s"(lds_byte_addr) : "memory");
}
__device__ __forceinline__ void lds_dma16(unsigned long long sbase, unsigned voff, unsigned lds_byte_addr) {
    lds_dma16_sgpr(sbase, voff, __builtin_amdgcn_readfirstlane(lds_byte_addr));
}
// 16 bytes per lane from a 64-bit per-lane address
__device__ __forceinline__ void lds_dma16_off(unsigned long long src, unsigned lds_byte_addr) {
    asm volatile("s_mov_b32 m0, %1\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, off"
                 :: "v"(src), "s"(__builtin_amdgcn_readfirstlane(lds_byte_addr)) : "memory");
}
__device__ __forceinline__ void lds_dma16_off(const void* src, unsigned lds_byte_addr) { lds_dma16_off((unsigned long long)src, lds_byte_addr); }
// 4 bytes per lane from a 64-bit per-lane address
__device__ __forceinline__ void lds_dma4_off(unsigned long long src, unsigned lds_byte_addr) {
    asm volatile("s_mov_b32 m0, %1\n\ts_nop 0\n\tglobal_load_lds_dword %0, off"
                 :: "v"(src), "s"(__builtin_amdgcn_readfirstlane(lds_byte_addr)) : "memory");
}

// 16 bytes per lane through a buffer descriptor (range-checked: offsets >= num_records write zeros).  srd / soff /
// lds_byte_addr must be wave-uniform; the s_nops cover the M0 -> LDS-DMA wait state and an SGPR written by v_readfirstlane
// just in front of the statement.
constexpr unsigned OOB = 0x80000000u;          // a transfer offset beyond num_records: the lane's 16 bytes arrive as zeros
__device__ __forceinline__ void dma_buf16(const u32x4& srd, unsigned voff, unsigned soff, unsigned lds_byte_addr) {
    asm volatile("s_mov_b32 m0, %2\n\ts_nop 3\n\tbuffer_load_dwordx4 %0, %1, %3 offen lds"
                 :: "v"(voff), "s"(srd), "s"(lds_byte_addr), "s"(soff) : "memory");
}
// the same with the scalar offset as the immediate 0 (no SGPR is spent on it)
__device__ __forceinline__ void dma_buf16_soff0(const u32x4& srd, unsigned voff, unsigned lds_byte_addr) {
    asm volatile("s_mov_b32 m0, %2\n\ts_nop 3\n\tbuffer_load_dwordx4 %0, %1, 0 offen lds"
                 :: "v"(voff), "s"(srd), "s"(lds_byte_addr) : "memory");
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

// ---- ds_read_b64_tr_b16 ------------------------------------------------------------------------------------------------
// A 16-lane group hands in the addresses of a [4 rows][16 columns] block of 16-bit values (lane L: row L / 4, columns
// 4 (L % 4) ..) and lane i receives column i of the four rows; two reads = the eight consecutive k-values of a fragment.
__device__ __forceinline__ u32x4 tr_read2(lds_cptr p0, lds_cptr p1) {
    const s16x4 a = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)p0);
    const s16x4 b = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)p1);
    const u32x2 ua = __builtin_bit_cast(u32x2, a), ub = __builtin_bit_cast(u32x2, b);
    return u32x4{ua[0], ua[1], ub[0], ub[1]};
}

// ---- split-K reduce: the body of the *_wgrad_reduce_kernel of conv_nhwc / conv_x3s / conv_x3q / conv3d_bf16 ------------
// Sum of the nparts partials part[k][numel] for the 64 elements from i0: 16 float4 outputs x 16 part lanes per workgroup of
// 256 threads (each lane sums every 16th part in order, then the 16 lanes are combined in order through LDS): fixed summation
// order.  store(i, t) writes the four sums of elements i .. i + 3.  The kernels call it from their grid-stride loop
//     for (long i0 = (long)blockIdx.x * 64; i0 < numel; i0 += (long)gridDim.x * 64)
// (the loop stays in the kernel: with it in here the compiler lays the kernel's blocks out differently).
template <class Store>
__device__ __forceinline__ void wgrad_reduce_step(const float* __restrict__ part, int nparts, long numel, long i0, Store store) {
    __shared__ float4 red[16][17];
    const int o = threadIdx.x & 15, sl = threadIdx.x >> 4;
    const long i = i0 + 4 * o;
    float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
    if (i < numel)
        for (int k = sl; k < nparts; k += 16) {
            const float4 v = *reinterpret_cast<const float4*>(part + (size_t)k * numel + i);
            s.x += v.x; s.y += v.y; s.z += v.z; s.w += v.w;
        }
    red[sl][o] = s;
    __syncthreads();
    if (sl == 0 && i < numel) {
        float4 t = red[0][o];
#pragma unroll
        for (int k = 1; k < 16; ++k) { const float4 v = red[k][o]; t.x += v.x; t.y += v.y; t.z += v.z; t.w += v.w; }
        store(i, t);
    }
    __syncthreads();
}
__device__ __forceinline__ void wgrad_reduce_step(const float* __restrict__ part, float* __restrict__ dw, int nparts, long numel, long i0) {
    wgrad_reduce_step(part, nparts, numel, i0, [&](long i, const float4& t) { *reinterpret_cast<float4*>(dw + i) = t; });
}

}  // namespace dmc
