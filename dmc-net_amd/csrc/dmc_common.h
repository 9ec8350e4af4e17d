// Shared host/device helpers for libdmcnet_hip.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdarg.h>
#include <stdio.h>

#include <atomic>

#include "dmcnet_hip.h"
#include "mma_bf16.h"

namespace dmc {

// ---- error reporting (thread-local, no global mutable state shared between threads) --------
inline char* err_buf() {
    static thread_local char buf[512] = {0};
    return buf;
}
inline int fail(int code, const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(err_buf(), 512, fmt, ap);
    va_end(ap);
    return code;
}
inline int check_launch(const char* what) {
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(DMC_E_LAUNCH, "%s: %s", what, hipGetErrorString(e));
    return DMC_OK;
}

// ---- dynamic LDS above 64 KB -----------------------------------------------------------------
// hipFuncAttributeMaxDynamicSharedMemorySize is a property of (kernel, DEVICE): one function-static per launch site
// remembers on which devices of this process it has been raised (a process that drives a second GPU would otherwise
// fail every > 64 KB launch there).  Thread-safe: a relaxed bit mask; setting the attribute twice is harmless.
struct LdsLimit {
    std::atomic<unsigned long long> raised{0};
    hipError_t raise(const void* kernel, int bytes) {
        int dev = 0;
        hipError_t e = hipGetDevice(&dev);
        if (e != hipSuccess) return e;
        if (dev >= 0 && dev < 64 && ((raised.load(std::memory_order_relaxed) >> dev) & 1ull)) return hipSuccess;
        e = hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
        if (e == hipSuccess && dev >= 0 && dev < 64) raised.fetch_or(1ull << dev, std::memory_order_relaxed);
        return e;
    }
};

// ---- kernel-selection options (dmc_set_option / dmc_get_option, storage in losses.hip) ----------
// The library never reads the environment.  These few integers select between kernel variants for
// A/B measurements; the defaults are the fastest measured path.  They are relaxed atomics read
// once per entry-point call -- the only process-wide state of the library.
enum Option { OPT_GEN_LAYER_PATH = 0, OPT_GEN_GATHER, OPT_GEN_FUSE45, OPT_GEN_WGRAD_PATH, OPT_GEN_FUSE_FWD,
              OPT_GEN_FUSE_BWD, OPT_GEN_FRAMES, OPT_CONV_PATH, OPT_CONV_CFG, OPT_CONV_ABLATE, OPT_GEN_ABLATE, OPT_CONV_ARITH, OPT_CONV3D_WGRAD, OPT_GEN_X3, OPT_GEN_WINO, OPT_GEN_STAGGER, OPT_GEN_FUSED, OPT_GRID_RESERVE_CUS, OPT_COUNT };
int option(Option o);
// CUs a PERSISTENT grid (one workgroup per CU walking a work list: gen_fused, the generator ring / gather / Winograd kernels,
// gen_wgrad_rs, conv3d_p3) may fill, out of `hw`: option "grid_reserve_cus" (default 0) leaves that many idle -- room for RCCL's
// channel kernels when gradients are exchanged while the backward pass runs; a multiple of 8 stays (one CU per XCD granularity).
inline int persistent_cus(int hw) {
    const int r = option(OPT_GRID_RESERVE_CUS);
    int n = hw - (r > 0 ? r : 0);
    n -= n % 8;
    return n < 8 ? (hw < 8 ? hw : 8) : n;
}
// Measurement-only options ("gen_ablate", "conv_ablate", "gen_stagger": parts of a kernel switched off, RESULTS WRONG) exist only
// in a -DDMC_MEASURE build (dmc-net_amd/build.py --measure -> libdmcnet_hip_measure.so, which tools/ load through DMC_HIP_LIB):
// the product library refuses to set them, reads them as 0, and DMC_ABL() folds every ablated path out of its kernels.
#ifdef DMC_MEASURE
#define DMC_ABL(x) (x)
constexpr bool MEASURE_BUILD = true;
#else
#define DMC_ABL(x) 0
constexpr bool MEASURE_BUILD = false;
#endif
constexpr bool measure_only(int o) { return o == OPT_GEN_ABLATE || o == OPT_CONV_ABLATE || o == OPT_GEN_STAGGER; }
// Kernel variants that LOST their A/B measurement are removed (DESIGN 4 and profiles/ keep the numbers): both builds refuse the option
// values that selected them -- the one-launch generator data gradient (gen_fused bit 1), the generator layer variants (ii) /
// (iii)-on-layer-3 / all-three-stage (gen_layer_path 3, 4, 5), the weight-gradient predecessors (gen_wgrad_path 0 .. 3).
constexpr bool accepted_value(int o, int v) {
    return o == OPT_GEN_FUSED ? (v == 0 || v == 1) : o == OPT_GEN_LAYER_PATH ? (v == 0 || v == 1)
         : o == OPT_GEN_WGRAD_PATH ? (v == 4 || v == 5) : true;
}

// ---- EstimatorDenseNetTiny geometry (code/dmcnet/model.py:172-194) --------------------------
// Physical channel order used by every kernel: [mv0 mv1 r0 r1 r2 | y0(8) | y1(8) | y2(6) | y3(4)
// | y4(2)] -- features are APPENDED, so layer k reads physical channels [0, CIN[k]).  The
// reference PREPENDS (torch.cat((conv(x), x), 1)); the weight repack maps between the two.
constexpr int NL = 6;
__host__ __device__ constexpr int cin_of(int k) {
    return k == 0 ? 5 : k == 1 ? 13 : k == 2 ? 21 : k == 3 ? 27 : k == 4 ? 31 : 33;
}
__host__ __device__ constexpr int cout_of(int k) {
    return k == 0 ? 8 : k == 1 ? 8 : k == 2 ? 6 : k == 3 ? 4 : 2;
}
// first physical channel of y_k (k = 0..4); yoff(5) = 33
__host__ __device__ constexpr int yoff(int k) { return cin_of(k); }
constexpr int NFEAT = 28;   // y0..y4 channels kept in the `saved` / `gbuf` buffers
constexpr int NIN = 5;

// packed parameter block (floats):  WF | BF | WB
//   WF[k][p][tap][co]   forward weights, p = physical input channel           (4554)
//   BF[k][co]                                                                  (30)
//   WB[j][c][tap][cd]   j = 0..4, data-gradient weights BY OUTPUT GROUP: the gradient of feature
//                       group y_j (cd in [0, COUT[j])) gathers from every later layer's g:
//                       input channel c runs over [g_{j+1} .. g_4, g_5], taps flipped  (3204)
__host__ __device__ constexpr int wf_off(int k) {
    int o = 0;
    for (int i = 0; i < k; ++i) o += cin_of(i) * 9 * cout_of(i);
    return o;
}
constexpr int WF_TOTAL = wf_off(6);   // 4554
__host__ __device__ constexpr int bf_off(int k) {
    int o = WF_TOTAL;
    for (int i = 0; i < k; ++i) o += cout_of(i);
    return o;
}
constexpr int NPARAM = bf_off(6);     // 4584
// number of gradient channels feeding feature group j: all g_k with k > j (30 - yoff(j+1) + 5)
__host__ __device__ constexpr int gin_of(int j) { return 35 - yoff(j + 1); }
__host__ __device__ constexpr int wb_off(int j) {
    int o = NPARAM;
    for (int i = 0; i < j; ++i) o += gin_of(i) * 9 * cout_of(i);
    return o;
}
constexpr int PACKED_TOTAL = wb_off(5);   // 7788
constexpr int ZERO_PAD = 256;             // zero words (1 KB: one LDS-DMA row) kept behind the packed parameters
// row-splits of the per-channel BatchNorm reductions: partial sums live in scratch as [channel][BN_MAX_SPLIT][2] doubles
// (dmc_bn_act_scratch_bytes); producers that reduce statistics in their epilogue (stem.hip) write the same layout
constexpr int BN_MAX_SPLIT = 1024;

// logical (reference, prepend order) input-channel index of physical channel p in layer k
__host__ __device__ inline int logical_of(int k, int p) {
    if (p < NIN) return (cin_of(k) - NIN) + p;
    int j = 0;
    while (p >= yoff(j) + cout_of(j)) ++j;
    int l = 0;
    for (int i = j + 1; i < k; ++i) l += cout_of(i);
    return l + (p - yoff(j));
}

struct ParamPtrs {
    const float* w[NL];
    const float* b[NL];
};
struct GradPtrs {
    float* w[NL];
    float* b[NL];
};

}  // namespace dmc

// ---- lane sums on the VALU's data-parallel primitives (DPP) -----------------------------------------------
// A butterfly of __shfl_xor is one ds_bpermute_b32 per dword and level -- an LDS-crossbar round trip each, waited for: the fp64
// BatchNorm sums of an accumulator tile (32 values x 5 levels x 2 dwords) cost more than a short convolution's main loop.
// Rotations within a row of 16 lanes (row_ror) and the broadcast of a row's lane 15 into the next row (row_bcast:15) are plain
// vector instructions.  The order of the additions is fixed (not the butterfly's).
namespace dmc {
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ double dpp_f64(double v) {
    const int lo = __builtin_amdgcn_update_dpp(0, __double2loint(v), CTRL, ROW_MASK, 0xf, false);
    const int hi = __builtin_amdgcn_update_dpp(0, __double2hiint(v), CTRL, ROW_MASK, 0xf, false);
    return __hiloint2double(hi, lo);
}
// every lane of a row of 16 (lanes 16 k .. 16 k + 15) gets the row's sum
__device__ __forceinline__ double row16_sum(double v) {
    v += dpp_f64<0x128, 0xf>(v);                           // row_ror:8
    v += dpp_f64<0x124, 0xf>(v);                           // row_ror:4
    v += dpp_f64<0x122, 0xf>(v);                           // row_ror:2
    v += dpp_f64<0x121, 0xf>(v);                           // row_ror:1
    return v;
}
// lanes 16 .. 31 (48 .. 63) get the sum of lanes 0 .. 31 (32 .. 63); the other lanes hold their row's sum
__device__ __forceinline__ double half32_sum_hi(double v) {
    v = row16_sum(v);
    v += dpp_f64<0x142, 0xa>(v);                           // row_bcast:15 into rows 1 and 3 (rows 0 and 2 add 0)
    return v;
}
}  // namespace dmc

// ---- BatchNorm with running statistics as a per-channel affine map (the eval epilogues of conv3d_bf16.hip, stem3d_bf16.hip) ----
// scale = gamma / sqrt(running_var + eps), shift = beta - running_mean * scale in fp32: each operation rounded once (division and
// square root correctly rounded; the product and the difference are NOT fused); channels c >= C get (0, 0).  Statistics are read,
// never written.
namespace dmc {
struct BnEval { const float* gamma; const float* beta; const float* mean; const float* var; float eps; };
__device__ __forceinline__ void bn_eval_affine(const BnEval& b, int C, int c, float* scale, float* shift) {
    float sc = 0.f, sh = 0.f;
    if (c < C) {
        sc = b.gamma[c] / sqrtf(b.var[c] + b.eps);
        const float ms = b.mean[c] * sc;
        sh = b.beta[c] - ms;
    }
    scale[c] = sc;
    shift[c] = sh;
}
}  // namespace dmc

// ---- bf16x3 slice tensors (conv_x3s.hip and their producers in bn_act.hip) -------------------------------
// An fp32 value is the exact sum of three bf16 values: s0 = its upper 16 bits, s1 = the upper 16 bits of the exact
// remainder, s2 = the second remainder.  A slice tensor of a [M][C] fp32 activation is bf16 [3][C / 16][M][16].
namespace dmc {
// the three slices of 8 consecutive channels (8 g .. 8 g + 7) of pixel m -> xs
__device__ __forceinline__ void x3s_store8(unsigned short* __restrict__ xs, const float (&v)[8], size_t M, int nchunk, size_t m, int g) {
    const Split3 sp = split8(v);
    const size_t plane = M * 16;
    const size_t w = ((size_t)(g >> 1) * M + m) * 16 + (size_t)(g & 1) * 8;
    *reinterpret_cast<u32x4*>(xs + w) = sp.s[0];
    *reinterpret_cast<u32x4*>(xs + (size_t)nchunk * plane + w) = sp.s[1];
    *reinterpret_cast<u32x4*>(xs + (size_t)2 * nchunk * plane + w) = sp.s[2];
}
// the three slices of 4 consecutive channels (4 q .. 4 q + 3) of pixel m -> xs: the same split and packing as x3s_store8, in
// 8-byte pieces (the eval epilogues of conv_x3s.hip / conv_x3q.hip, whose lanes hold four channels of a pixel)
__device__ __forceinline__ void x3s_store4(unsigned short* __restrict__ xs, const float (&v)[4], size_t M, int nchunk, size_t m, int q) {
    const Split3x2 sp = split4(v);
    const size_t plane = M * 16;
    const size_t w = ((size_t)(q >> 2) * M + m) * 16 + (size_t)(q & 3) * 4;
    *reinterpret_cast<u32x2*>(xs + w) = sp.s[0];
    *reinterpret_cast<u32x2*>(xs + (size_t)nchunk * plane + w) = sp.s[1];
    *reinterpret_cast<u32x2*>(xs + (size_t)2 * nchunk * plane + w) = sp.s[2];
}

// ---- BatchNorm with GIVEN statistics [+ shortcut] [+ ReLU] on one value: the expression and the order of bn_apply_fwd_kernel /
// bn_apply_fwd_x3s_kernel (bn_act.hip).  The build has -ffp-contract=off, so a convolution epilogue that applies it to its
// accumulator gives the bits of the convolution followed by that streaming pass.
__device__ __forceinline__ float bn_apply_act1(float x, float mean, float istd, float gamma, float beta, bool has_res, float res, bool relu) {
    float v = fmaf((x - mean) * istd, gamma, beta);
    if (has_res) v += res;
    if (relu) v = fmaxf(v, 0.f);
    return v;
}
}  // namespace dmc
