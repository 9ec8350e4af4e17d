// EstimatorDenseNet / EstimatorDenseNetSmall in eval mode (code/dmcnet/model.py:122-170): the dense stack
//   for i in 0..4: x = cat(LeakyReLU_0.1(conv_i(x)), x);  predict_flow(x)
// without a single concatenation.  ONE NHWC fp32 feature buffer feat[M][CT] (M = N H W) holds every activation of a frame range
// in slots, in production order: slot 0 = the 5 input channels and 11 zeros, slot k = the output of conv_{k-1} padded with zeros
// to a multiple of 32 channels.  Layer k reads the prefix [0, K) of every pixel and appends the slot [K, K + R); the head reads
// all of it.  The host permutes each weight's input channels into that order (and zero-pads rows and columns) once per call.
//
//   ingest  x NCHW [N][5][H][W] -> feat[m][0..16): one thread per pixel, four 16-byte stores
//   layer   feat[m][K..K+R) = leaky(conv3x3(feat[.][0..K)) + bias): implicit GEMM over (tap, channel) on v_mfma_f32_32x32x16_bf16 in
//           the bf16x3 arithmetic: ctx_common.h's gather_gemm (the loop of ctx_eval.hip and dconv.hip) with the pixel stride
//           CT, the contraction length K, the first gathered channel 0 and dilation 1; the training route's data gradient
//           (dense_train.hip) is the same loop from channel K
//   head    predict_flow (K -> 2, no activation), NCHW out: plain fp32 FMAs in the form of ctx_eval.hip's ctx_heads_kernel
//   pack    ctxk::pack_kernel as it is, on the padded OHWI weight [R][3][3][K]: panels [9][K / 16][3][R][16] bf16
//
// The layer runs IN PLACE, through one non-const pointer.  A launch READS channels < K (of its own and of the neighbouring
// pixels) and WRITES channels >= K (of its own pixels only): the bytes read and the bytes written are disjoint sets of the same
// buffer, so no workgroup can observe another's stores, whatever the order in which tiles run -- there is no race and nothing to
// synchronise.  (K + R <= CT keeps the stores inside the pixel's row; K % 16 == 0 keeps every gather below K.)
//
// Layer kernel.  The main loop, its ownership of pixels and channels and the order of the six slice products are gather_gemm's
// (described in ctx_common.h and ctx_eval.hip's header); the B operand is the prefix at the tap-shifted pixel.
// Epilogue: v = acc + bias[co]; v > 0 ? v : 0.1f v; one 16-byte store per channel quad.
// No atomics; a pixel's sum is formed in one fixed order by one lane column of the matrix core whatever tile or batch the
// pixel is in: results are bit-identical from run to run and independent of the batch.
// All tensor offsets are 64-bit; dmc_dense_supported() bounds N H W CT below 2^31 so that the pixel index fits an int.
#include "ctx_common.h"

using namespace dmc;
using namespace dmc::ctxk;
using namespace dmc::densek;

namespace {

constexpr float SLOPE = 0.1f;
constexpr int HEAD_KMAX = 512;

template <int TN, int TM>
__global__ __launch_bounds__(256) void dense_layer_kernel(DenseArgs a) {
    __shared__ __attribute__((aligned(16))) char lds[GatherLds<TN>::BYTES];
    f32x16 acc[TM][TN];
    const int m0 = gather_gemm<TN, TM>(a, lds, acc);
    const int lane = threadIdx.x & 63;
    const int l31 = lane & 31, khalf = lane >> 5;

    // ---- epilogue: lane holds pixel l31 of tile i, channels 32 j + 8 gq + 4 khalf + e in acc[i][j][4 gq + e] ----
#pragma unroll
    for (int j = 0; j < TN; ++j)
#pragma unroll
        for (int gq = 0; gq < 4; ++gq) {
            const int co = 32 * j + 8 * gq + 4 * khalf;
            const f32x4 b = *reinterpret_cast<const f32x4*>(a.bias + co);
#pragma unroll
            for (int i = 0; i < TM; ++i) {
                const int m = m0 + 32 * i + l31;
                if (m >= a.M) continue;
                f32x4 v;
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const float t = acc[i][j][4 * gq + e] + b[e];
                    v[e] = t > 0.f ? t : SLOPE * t;
                }
                *reinterpret_cast<f32x4*>(a.feat + (long)m * a.CT + a.K + co) = v;
            }
        }
}

// ---- ingest: x NCHW [N][5][H][W] -> feat[m][0..16) = the 5 values, then 11 zeros; one thread per pixel ----
__global__ __launch_bounds__(256) void dense_ingest_kernel(const float* __restrict__ x, float* __restrict__ feat, int HW, int CT, int M) {
    const int m = blockIdx.x * 256 + threadIdx.x;
    if (m >= M) return;
    const int n = m / HW, rem = m - n * HW;
    const float* xp = x + (long)n * 5 * HW + rem;
    const f32x4 v0 = {xp[0], xp[HW], xp[2 * (long)HW], xp[3 * (long)HW]};
    const f32x4 v1 = {xp[4 * (long)HW], 0.f, 0.f, 0.f};
    const f32x4 z = {0.f, 0.f, 0.f, 0.f};
    f32x4* fp = reinterpret_cast<f32x4*>(feat + (long)m * CT);
    fp[0] = v0; fp[1] = v1; fp[2] = z; fp[3] = z;
}

// ---- head: feat[m][0..K) -> out NCHW [N][2][H][W]; w [2][9][K] in buffer order (LDS: 72 K bytes, dynamic).  Eight lanes share a
// pixel: lane q sums the channel quads q, q + 8, ... over the taps in order (fmaf), so the eight lanes read 128 contiguous bytes of
// a pixel at a time; the eight partial sums are then added in a fixed butterfly (lane distances 1, 2, 4: every lane ends with the
// same bits) and the bias is added last ----
__global__ __launch_bounds__(256) void dense_head_kernel(const float* __restrict__ feat, const float* __restrict__ w, const float* __restrict__ bias,
                                                         float* __restrict__ out, int H, int W, int CT, int K, int M) {
    extern __shared__ __attribute__((aligned(16))) float ws[];           // [co][tap][k]
    for (int i = threadIdx.x; i < 18 * K; i += 256) ws[i] = w[i];
    __syncthreads();
    const int q = threadIdx.x & 7;
    const int hw = H * W;
    const int nq = K >> 2;
#pragma unroll 1
    for (int g = 0; g < 4; ++g) {                                          // 4 x 32 pixels per workgroup
        const int m = blockIdx.x * 128 + g * 32 + (threadIdx.x >> 3);
        const bool live = m < M;                                          // (no lane leaves before the lane exchanges below)
        const int mm = live ? m : 0;
        const int n = mm / hw, rem = mm - n * hw;
        const int yy = rem / W, xx = rem - yy * W;
        float acc0 = 0.f, acc1 = 0.f;
#pragma unroll 1
        for (int t = 0; t < 9; ++t) {
            const int dy = t / 3 - 1, dx = t % 3 - 1;
            const int iy = yy + dy, ix = xx + dx;
            if (!(iy >= 0 && iy < H && ix >= 0 && ix < W)) continue;       // a tap outside the frame adds nothing
            const float* xp = feat + ((long)mm + (long)dy * W + dx) * CT;
            const float* w0 = ws + t * K;
            const float* w1 = ws + (9 + t) * K;
#pragma unroll 2
            for (int c = q; c < nq; c += 8) {
                const f32x4 xv = *reinterpret_cast<const f32x4*>(xp + 4 * c);
                const f32x4 a0 = *reinterpret_cast<const f32x4*>(w0 + 4 * c);
                const f32x4 a1 = *reinterpret_cast<const f32x4*>(w1 + 4 * c);
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    acc0 = fmaf(xv[e], a0[e], acc0);
                    acc1 = fmaf(xv[e], a1[e], acc1);
                }
            }
        }
#pragma unroll
        for (int o = 1; o < 8; o <<= 1) {
            acc0 += __shfl_xor(acc0, o);
            acc1 += __shfl_xor(acc1, o);
        }
        if (live && q < 2) out[((long)n * 2 + q) * hw + rem] = (q == 0 ? acc0 : acc1) + bias[q];
    }
}

bool pack_ok(int K, int R) { return K >= 16 && K % 16 == 0 && width_ok(R) && (long long)K * R * 9 < (1ll << 31); }

}  // namespace

extern "C" {

int dmc_dense_supported(int N, int H, int W, int CT, int K, int R) {
    if (N <= 0 || H <= 0 || W <= 0 || CT <= 0 || CT % 4 != 0 || K < 16 || K % 16 != 0) return 0;
    if ((long long)N * H * W * CT >= (1ll << 31)) return 0;
    if (R == 2) return (K <= CT && K <= HEAD_KMAX && K % 4 == 0) ? 1 : 0;
    return (width_ok(R) && (long long)K + R <= CT) ? 1 : 0;
}

size_t dmc_dense_wpack_bytes(int K, int R) {
    if (!pack_ok(K, R)) return 0;
    return (size_t)K * R * 9 * 3 * 2;
}

int dmc_dense_pack_weights(const float* w_ohwi_padded, void* wpack, int K, int R, dmc_stream_t stream) {
    if (!w_ohwi_padded || !wpack) return fail(DMC_E_INVALID, "dmc_dense_pack_weights: null pointer");
    if (!pack_ok(K, R)) return fail(DMC_E_INVALID, "dmc_dense_pack_weights: unsupported shape (K %d, R %d)", K, R);
    const int total = K * R * 9;
    pack_kernel<<<(total + 255) / 256, 256, 0, (hipStream_t)stream>>>(w_ohwi_padded, reinterpret_cast<unsigned short*>(wpack), K, R, 0);
    return check_launch("dmc_dense_pack_weights");
}

int dmc_dense_ingest(const float* x_nchw, float* feat, int N, int H, int W, int CT, dmc_stream_t stream) {
    if (!x_nchw || !feat) return fail(DMC_E_INVALID, "dmc_dense_ingest: null pointer");
    if (N <= 0 || H <= 0 || W <= 0 || CT < 16 || CT % 4 != 0 || (long long)N * H * W * CT >= (1ll << 31))
        return fail(DMC_E_INVALID, "dmc_dense_ingest: unsupported shape (N %d, H %d, W %d, CT %d)", N, H, W, CT);
    const int M = N * H * W;
    dense_ingest_kernel<<<(M + 255) / 256, 256, 0, (hipStream_t)stream>>>(x_nchw, feat, H * W, CT, M);
    return check_launch("dmc_dense_ingest");
}

int dmc_dense_layer_eval(float* feat, const void* wpack, const float* bias, int N, int H, int W, int CT, int K, int R, dmc_stream_t stream) {
    if (!feat || !wpack || !bias) return fail(DMC_E_INVALID, "dmc_dense_layer_eval: null pointer");
    if (!pack_ok(K, R) || !dmc_dense_supported(N, H, W, CT, K, R))
        return fail(DMC_E_INVALID, "dmc_dense_layer_eval: unsupported shape (N %d, H %d, W %d, CT %d, K %d, R %d)", N, H, W, CT, K, R);
    DenseArgs a;
    a.feat = feat; a.wpack = reinterpret_cast<const unsigned short*>(wpack); a.bias = bias;
    a.H = H; a.W = W; a.CT = CT; a.K = K; a.M = N * H * W;
    a.koff = 0; a.c0 = 0; a.cend = 0;
    constexpr int TM = 2;
    const dim3 grid((a.M + 128 * TM - 1) / (128 * TM));
    hipStream_t s = (hipStream_t)stream;
    switch (R) {
        case 128: dense_layer_kernel<4, TM><<<grid, 256, 0, s>>>(a); break;
        case 96: dense_layer_kernel<3, TM><<<grid, 256, 0, s>>>(a); break;
        case 64: dense_layer_kernel<2, TM><<<grid, 256, 0, s>>>(a); break;
        default: dense_layer_kernel<1, TM><<<grid, 256, 0, s>>>(a); break;
    }
    return check_launch("dmc_dense_layer_eval");
}

int dmc_dense_head_eval(const float* feat, const float* w, const float* bias, float* out_nchw, int N, int H, int W, int CT, int K,
                        dmc_stream_t stream) {
    if (!feat || !w || !bias || !out_nchw) return fail(DMC_E_INVALID, "dmc_dense_head_eval: null pointer");
    if (!dmc_dense_supported(N, H, W, CT, K, 2))
        return fail(DMC_E_INVALID, "dmc_dense_head_eval: unsupported shape (N %d, H %d, W %d, CT %d, K %d)", N, H, W, CT, K);
    const int M = N * H * W;
    dense_head_kernel<<<(M + 127) / 128, 256, 72 * K, (hipStream_t)stream>>>(feat, w, bias, out_nchw, H, W, CT, K, M);
    return check_launch("dmc_dense_head_eval");
}

}  // extern "C"
