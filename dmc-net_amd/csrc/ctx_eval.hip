// ContextNetwork / ContextNetworkAtt in eval mode (code/dmcnet/model.py:45-104): every unit
//   Conv2d(3x3, dilation d, padding d, no bias) -> BatchNorm2d(running statistics) -> LeakyReLU(0.1)
// is ONE launch; nothing of a unit goes through memory except its input and its result.
//
//   first unit  (5 -> 32, d = 1)     NCHW in, NHWC out, plain fp32 FMAs in a fixed order (0.4 % of the arithmetic)
//   middle units (Cin, Cout in {32, 64, 96, 128}, d in {1, 2, 4, 8, 16})
//                                    NHWC in, NHWC out: implicit GEMM over (tap, ci) on v_mfma_f32_32x32x16_bf16 in the
//                                    bf16x3 arithmetic of conv_nhwc.hip's conv3_kernel -- six slice products per fp32 product
//   head(s)     (32 -> 2, d = 1)     NHWC in, NCHW out; predict_flow and predict_att (+ ReLU) of the attention network
//                                    in one launch over the same input
//
// Middle kernel = ctx_common.h's gather_gemm (the one main loop of this file, dconv.hip, dense_eval.hip and
// dense_train.hip's data gradient; what follows describes it for all of them) + this file's epilogue.  GEMM view: rows =
// output channels (A operand = weight slices), columns = output pixels (B operand = the input at the tap-shifted pixel),
// K = (tap, ci) in k-blocks of 16 channels.  Dilation enters through the tap offsets only: tap (ky, kx) reads pixel
// (y + (ky - 1) d, x + (kx - 1) d), zero outside the H x W frame (tested per coordinate, never on a linearised offset).
//   * A workgroup of four waves owns 128 TM consecutive pixels; each wave owns 32 TM of them and ALL Cout = 32 TN
//     channels (TN accumulator tiles of 32 x 32 per pixel tile).  Cout = 96 and 32 are simply TN = 3 and 1: no padded
//     channel is computed, stored or allocated.
//   * The B fragment of a 32x32x16 MFMA is, per lane, 8 consecutive channels of ONE pixel: 32 contiguous bytes of the
//     NHWC tensor.  Each lane gathers its own fragment from global memory into registers (two 16-byte loads, one step
//     ahead) and splits it there; activations never pass through the LDS, so how far a tap reaches costs nothing.
//   * Weights are split once per call (pack_kernel, ctx_common.h) into [tap][k-block][slice][co][16] bf16: the three slices of a
//     step's [Cout][16] panel are one contiguous chunk of 96 Cout bytes, copied global -> registers -> LDS by the whole
//     workgroup one step ahead (two buffers, one barrier per step), read by every wave as conflict-free ds_read_b128
//     (a wave's 64 lanes cover 2 KB of consecutive addresses).
//   * Epilogue per output channel: fmaf((acc - mean) * invstd, gamma, beta), LeakyReLU(0.1), one 16-byte store
//     (a lane holds 4 consecutive channels of a pixel in each accumulator quad).
// No atomics; a pixel's sum is formed in one fixed order by one lane column of the matrix core, whatever tile or batch
// the pixel is in: results are bit-identical from run to run and independent of the batch.
// All tensor offsets are 64-bit; dmc_ctx_unit_supported() bounds N H W so that the pixel index fits an int.
#include "ctx_common.h"

using namespace dmc;
using namespace dmc::ctxk;

namespace {

constexpr float SLOPE = 0.1f;

struct CtxArgs {
    GatherArgs g;                   // x [N][H][W][Cin], wpack [9][Cin / 16][3][Cout][16] bf16, the geometry
    const float* stats;             // mean[Cout], invstd[Cout]
    const float* gamma;
    const float* beta;
    float* y;                       // [N][H][W][Cout]
};

__device__ __forceinline__ float bn_leaky(float v, float mean, float istd, float gamma, float beta) {
    const float t = fmaf((v - mean) * istd, gamma, beta);
    return t > 0.f ? t : SLOPE * t;
}

// main loop: ctx_common.h's gather_gemm with stride = length = Cin from channel 0; the epilogue is this kernel's
template <int TN, int TM>
__global__ __launch_bounds__(256) void ctx_unit_kernel(CtxArgs a) {
    constexpr int COUT = 32 * TN;
    __shared__ __attribute__((aligned(16))) char lds[GatherLds<TN>::BYTES];
    f32x16 acc[TM][TN];
    const int m0 = gather_gemm<TN, TM>(a.g, lds, acc);
    const int lane = threadIdx.x & 63;
    const int l31 = lane & 31, khalf = lane >> 5;

    // ---- epilogue: lane holds pixel l31 of tile i, channels 32 j + 8 gq + 4 khalf + e in acc[i][j][4 gq + e] ----
#pragma unroll
    for (int j = 0; j < TN; ++j)
#pragma unroll
        for (int gq = 0; gq < 4; ++gq) {
            const int co = 32 * j + 8 * gq + 4 * khalf;
            const f32x4 mean = *reinterpret_cast<const f32x4*>(a.stats + co);
            const f32x4 istd = *reinterpret_cast<const f32x4*>(a.stats + COUT + co);
            const f32x4 gam = *reinterpret_cast<const f32x4*>(a.gamma + co);
            const f32x4 bet = *reinterpret_cast<const f32x4*>(a.beta + co);
#pragma unroll
            for (int i = 0; i < TM; ++i) {
                const int m = m0 + 32 * i + l31;
                if (m >= a.g.M) continue;
                f32x4 v;
#pragma unroll
                for (int e = 0; e < 4; ++e) v[e] = bn_leaky(acc[i][j][4 * gq + e], mean[e], istd[e], gam[e], bet[e]);
                *reinterpret_cast<f32x4*>(a.y + (long)m * COUT + co) = v;
            }
        }
}

// ---- first unit: x NCHW [N][5][H][W], w OIHW [32][5][3][3] -> y NHWC [N][H][W][32]; one thread per pixel,
// the sum over (ci, ky, kx) in that order with fmaf ----
__global__ __launch_bounds__(256) void ctx_first_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                        const float* __restrict__ stats, const float* __restrict__ gamma,
                                                        const float* __restrict__ beta, float* __restrict__ y, int H, int W, int M) {
    __shared__ __attribute__((aligned(16))) float ws[45 * 32];           // [ci * 9 + tap][co]
    for (int i = threadIdx.x; i < 45 * 32; i += 256) ws[(i % 45) * 32 + i / 45] = w[i];
    __syncthreads();
    const int m = blockIdx.x * 256 + threadIdx.x;
    if (m >= M) return;
    const int hw = H * W;
    const int n = m / hw, rem = m - n * hw;
    const int yy = rem / W, xx = rem - yy * W;
    float acc[32];
#pragma unroll
    for (int c = 0; c < 32; ++c) acc[c] = 0.f;
    const float* xn = x + (long)n * 5 * hw;
#pragma unroll 1
    for (int ci = 0; ci < 5; ++ci)
#pragma unroll
        for (int t = 0; t < 9; ++t) {
            const int iy = yy + t / 3 - 1, ix = xx + t % 3 - 1;
            const bool ok = iy >= 0 && iy < H && ix >= 0 && ix < W;
            const float xv = ok ? xn[(long)ci * hw + (long)iy * W + ix] : 0.f;
            const float* wk = ws + (ci * 9 + t) * 32;
#pragma unroll
            for (int c = 0; c < 32; ++c) acc[c] = fmaf(xv, wk[c], acc[c]);
        }
    float* yp = y + (long)m * 32;
#pragma unroll
    for (int q = 0; q < 8; ++q) {
        f32x4 v;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int c = 4 * q + e;
            v[e] = bn_leaky(acc[c], stats[c], stats[32 + c], gamma[c], beta[c]);
        }
        *reinterpret_cast<f32x4*>(yp + 4 * q) = v;
    }
}

// ---- heads: x NHWC [N][H][W][32], w OHWI [2][3][3][32] per head -> NCHW [N][2][H][W] per head.  Eight lanes share a pixel:
// lane q sums its channel quad 4 q .. 4 q + 3 over the taps in order (fmaf), so a pixel's 128 bytes are one coalesced read per
// tap; the eight partial sums are then added in a fixed butterfly (lane distances 1, 2, 4: every lane ends with the same bits).
// The attention head adds max(., 0) ----
struct HeadArgs {
    const float* x;
    const float* w[2];
    const float* stats[2];
    const float* gamma[2];
    const float* beta[2];
    float* out[2];
    int H, W, M, nheads;
};
__global__ __launch_bounds__(256) void ctx_heads_kernel(HeadArgs a) {
    __shared__ __attribute__((aligned(16))) float ws[2 * 576];            // [head][co][tap][ci]
    for (int i = threadIdx.x; i < a.nheads * 576; i += 256) ws[i] = a.w[i / 576][i % 576];
    __syncthreads();
    const int q = threadIdx.x & 7;
    const int hw = a.H * a.W;
#pragma unroll 1
    for (int g = 0; g < 4; ++g) {                                          // 4 x 32 pixels per workgroup
        const int m = blockIdx.x * 128 + g * 32 + (threadIdx.x >> 3);
        const bool live = m < a.M;                                        // (no lane leaves before the lane exchanges below)
        const int mm = live ? m : 0;
        const int n = mm / hw, rem = mm - n * hw;
        const int yy = rem / a.W, xx = rem - yy * a.W;
        float acc[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int t = 0; t < 9; ++t) {
            const int dy = t / 3 - 1, dx = t % 3 - 1;
            const int iy = yy + dy, ix = xx + dx;
            const bool ok = iy >= 0 && iy < a.H && ix >= 0 && ix < a.W;
            const f32x4 xv = ok ? *reinterpret_cast<const f32x4*>(a.x + ((long)mm + (long)dy * a.W + dx) * 32 + 4 * q) : (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                if (k >= 2 * a.nheads) break;
                const f32x4 wv = *reinterpret_cast<const f32x4*>(ws + (k * 9 + t) * 32 + 4 * q);
#pragma unroll
                for (int e = 0; e < 4; ++e) acc[k] = fmaf(xv[e], wv[e], acc[k]);
            }
        }
#pragma unroll
        for (int k = 0; k < 4; ++k)
#pragma unroll
            for (int o = 1; o < 8; o <<= 1) acc[k] += __shfl_xor(acc[k], o);
        // lane q < 2 nheads stores value q = (head q / 2, channel q % 2)
        const float sum = q == 0 ? acc[0] : q == 1 ? acc[1] : q == 2 ? acc[2] : acc[3];
        if (live && q < 2 * a.nheads) {
            const int h = q >> 1, c = q & 1;
            float v = bn_leaky(sum, a.stats[h][c], a.stats[h][2 + c], a.gamma[h][c], a.beta[h][c]);
            if (h == 1) v = fmaxf(v, 0.f);
            a.out[h][((long)n * 2 + c) * hw + rem] = v;
        }
    }
}

}  // namespace

extern "C" {

int dmc_ctx_unit_supported(int N, int H, int W, int Cin, int Cout, int dilation) {
    if (!index_ok(N, H, W)) return 0;
    if (Cin == 5 && Cout == 32) return dilation == 1;       // the first unit
    if (Cin == 32 && Cout == 2) return dilation == 1;       // the head(s)
    return middle_ok(Cin, Cout, dilation) ? 1 : 0;
}

size_t dmc_ctx_wpack_bytes(int Cin, int Cout) {
    if (!width_ok(Cin) || !width_ok(Cout)) return 0;
    return (size_t)Cin * Cout * 9 * 3 * 2;
}

int dmc_ctx_pack_weights(const float* w, void* wpack, int Cin, int Cout, dmc_stream_t stream) {
    if (!w || !wpack) return fail(DMC_E_INVALID, "dmc_ctx_pack_weights: null pointer");
    if (!width_ok(Cin) || !width_ok(Cout)) return fail(DMC_E_INVALID, "dmc_ctx_pack_weights: unsupported shape (Cin %d, Cout %d)", Cin, Cout);
    const int total = Cin * Cout * 9;
    pack_kernel<<<(total + 255) / 256, 256, 0, (hipStream_t)stream>>>(w, reinterpret_cast<unsigned short*>(wpack), Cin, Cout, 0);
    return check_launch("dmc_ctx_pack_weights");
}

int dmc_ctx_unit_eval(const float* x, const void* wpack, const float* stats, const float* gamma, const float* beta, float* y,
                      int N, int H, int W, int Cin, int Cout, int dilation, dmc_stream_t stream) {
    if (!x || !wpack || !stats || !gamma || !beta || !y) return fail(DMC_E_INVALID, "dmc_ctx_unit_eval: null pointer");
    if (!middle_ok(Cin, Cout, dilation) || !dmc_ctx_unit_supported(N, H, W, Cin, Cout, dilation))
        return fail(DMC_E_INVALID, "dmc_ctx_unit_eval: unsupported shape (N %d, H %d, W %d, Cin %d, Cout %d, dilation %d)", N, H, W, Cin, Cout, dilation);
    CtxArgs a;
    a.g.x = x; a.g.wpack = reinterpret_cast<const unsigned short*>(wpack); a.stats = stats; a.gamma = gamma; a.beta = beta; a.y = y;
    a.g.N = N; a.g.H = H; a.g.W = W; a.g.Cin = Cin; a.g.d = dilation; a.g.M = N * H * W;
    constexpr int TM = 2;
    const dim3 grid((a.g.M + 128 * TM - 1) / (128 * TM));
    hipStream_t s = (hipStream_t)stream;
    switch (Cout) {
        case 128: ctx_unit_kernel<4, TM><<<grid, 256, 0, s>>>(a); break;
        case 96: ctx_unit_kernel<3, TM><<<grid, 256, 0, s>>>(a); break;
        case 64: ctx_unit_kernel<2, TM><<<grid, 256, 0, s>>>(a); break;
        default: ctx_unit_kernel<1, TM><<<grid, 256, 0, s>>>(a); break;
    }
    return check_launch("dmc_ctx_unit_eval");
}

int dmc_ctx_first_eval(const float* x, const float* w, const float* stats, const float* gamma, const float* beta, float* y,
                       int N, int H, int W, dmc_stream_t stream) {
    if (!x || !w || !stats || !gamma || !beta || !y) return fail(DMC_E_INVALID, "dmc_ctx_first_eval: null pointer");
    if (!dmc_ctx_unit_supported(N, H, W, 5, 32, 1)) return fail(DMC_E_INVALID, "dmc_ctx_first_eval: unsupported shape (N %d, H %d, W %d)", N, H, W);
    const int M = N * H * W;
    ctx_first_kernel<<<(M + 255) / 256, 256, 0, (hipStream_t)stream>>>(x, w, stats, gamma, beta, y, H, W, M);
    return check_launch("dmc_ctx_first_eval");
}

int dmc_ctx_heads_eval(const float* x, const float* w_flow, const float* stats_flow, const float* gamma_flow, const float* beta_flow,
                       const float* w_att, const float* stats_att, const float* gamma_att, const float* beta_att, float* flow,
                       float* att, int N, int H, int W, dmc_stream_t stream) {
    if (!x || !w_flow || !stats_flow || !gamma_flow || !beta_flow || !flow) return fail(DMC_E_INVALID, "dmc_ctx_heads_eval: null pointer");
    const bool two = w_att != nullptr;
    if (two ? (!stats_att || !gamma_att || !beta_att || !att) : (att != nullptr))
        return fail(DMC_E_INVALID, "dmc_ctx_heads_eval: the attention head needs w_att, stats_att, gamma_att, beta_att and att together");
    if (!dmc_ctx_unit_supported(N, H, W, 32, 2, 1)) return fail(DMC_E_INVALID, "dmc_ctx_heads_eval: unsupported shape (N %d, H %d, W %d)", N, H, W);
    HeadArgs a;
    a.x = x;
    a.w[0] = w_flow; a.stats[0] = stats_flow; a.gamma[0] = gamma_flow; a.beta[0] = beta_flow; a.out[0] = flow;
    a.w[1] = w_att; a.stats[1] = stats_att; a.gamma[1] = gamma_att; a.beta[1] = beta_att; a.out[1] = att;
    a.H = H; a.W = W; a.M = N * H * W; a.nheads = two ? 2 : 1;
    ctx_heads_kernel<<<(a.M + 127) / 128, 256, 0, (hipStream_t)stream>>>(a);
    return check_launch("dmc_ctx_heads_eval");
}

}  // extern "C"
