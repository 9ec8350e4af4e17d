// EstimatorDenseNet / EstimatorDenseNetSmall in eval mode (code/dmcnet/model.py:122-170): the dense stack
//   for i in 0..4: x = cat(LeakyReLU_0.1(conv_i(x)), x);  predict_flow(x)
// without a single concatenation.  ONE NHWC fp32 feature buffer feat[M][CT] (M = N H W) holds every activation of a frame range
// in slots, in production order: slot 0 = the 5 input channels and 11 zeros, slot k = the output of conv_{k-1} padded with zeros
// to a multiple of 32 channels.  Layer k reads the prefix [0, K) of every pixel and appends the slot [K, K + R); the head reads
// all of it.  The host permutes each weight's input channels into that order (and zero-pads rows and columns) once per call.
//
//   ingest  x NCHW [N][5][H][W] -> feat[m][0..16): one thread per pixel, four 16-byte stores
//   layer   feat[m][K..K+R) = leaky(conv3x3(feat[.][0..K)) + bias): implicit GEMM over (tap, channel) on v_mfma_f32_32x32x16_bf16 in
//           the bf16x3 arithmetic of ctx_common.h's gather_gemm -- the same loop with the contraction length K and the pixel
//           stride CT as two numbers (gather_gemm has one, Cin, for both), dilation 1
//   head    predict_flow (K -> 2, no activation), NCHW out: plain fp32 FMAs in the form of ctx_eval.hip's ctx_heads_kernel
//   pack    ctxk::pack_kernel as it is, on the padded OHWI weight [R][3][3][K]: panels [9][K / 16][3][R][16] bf16
//
// The layer runs IN PLACE, through one non-const pointer.  A launch READS channels < K (of its own and of the neighbouring
// pixels) and WRITES channels >= K (of its own pixels only): the bytes read and the bytes written are disjoint sets of the same
// buffer, so no workgroup can observe another's stores, whatever the order in which tiles run -- there is no race and nothing to
// synchronise.  (K + R <= CT keeps the stores inside the pixel's row; K % 16 == 0 keeps every gather below K.)
//
// Layer kernel.  GEMM view: rows = output channels (A operand = weight slices), columns = output pixels (B operand = the
// prefix at the tap-shifted pixel), contraction = (tap, channel) in k-blocks of 16 channels; a tap outside the H x W frame is zero
// (tested per coordinate, never on a linearised offset).  Four waves own 128 TM consecutive pixels, each wave 32 TM of them and
// all R = 32 TN channels.  Per lane and step: two 16-byte gathers per pixel one step ahead, split into three bf16 slices in
// registers; the step's weight chunk (three slices of [R][16] bf16, 96 R bytes) goes global -> registers -> LDS one step ahead
// (two buffers, one barrier per step).  The six slice products are issued in the fixed order (w slice, x slice) =
// (0,2) (0,1) (0,0) | (1,1) (1,0) | (2,0).  Epilogue: v = acc + bias[co]; v > 0 ? v : 0.1f v; one 16-byte store per channel quad.
// No atomics; a pixel's sum is formed in one fixed order by one lane column of the matrix core whatever tile or batch the
// pixel is in: results are bit-identical from run to run and independent of the batch.
// All tensor offsets are 64-bit; dmc_dense_supported() bounds N H W CT below 2^31 so that the pixel index fits an int.
#include "ctx_common.h"
#include "mma_bf16.h"

using namespace dmc;
using namespace dmc::ctxk;

namespace {

constexpr float SLOPE = 0.1f;
constexpr int HEAD_KMAX = 512;

struct DenseArgs {
    float* feat;                    // [M][CT]; read below K, written in [K, K + 32 TN)
    const unsigned short* wpack;    // [9][K / 16][3][R][16] bf16
    const float* bias;              // [R]
    int H, W, CT, K, M;             // M = N H W
};

// gather_gemm (ctx_common.h) with the pixel stride CT and the contraction length K apart, dilation 1.  Same ownership and the
// same accumulator layout: on return the lane holds pixel m0 + 32 i + (lane & 31), channels 32 j + 8 gq + 4 (lane >> 5) + e in
// acc[i][j][4 gq + e].  lds: GatherLds<TN>::BYTES bytes, 16-byte aligned.
template <int TN, int TM>
__device__ __forceinline__ int dense_gemm(const DenseArgs& a, char* lds, f32x16 (&acc)[TM][TN]) {
    constexpr int COUT = GatherLds<TN>::COUT;
    constexpr int CH = GatherLds<TN>::CH;
    constexpr int NWR = (CH + 4095) / 4096;                // 16-byte pieces per thread

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l31 = lane & 31, khalf = lane >> 5;
    const int m0 = blockIdx.x * (128 * TM) + wave * (32 * TM);

    // ---- this lane's pixels: offset of (n, y, x, 8 khalf) and the taps that fall inside the frame ----
    long xbase[TM];
    unsigned tmask[TM];
#pragma unroll
    for (int i = 0; i < TM; ++i) {
        const int m = m0 + 32 * i + l31;
        xbase[i] = 0; tmask[i] = 0;
        if (m < a.M) {
            const int hw = a.H * a.W;
            const int rem = m % hw;
            const int yy = rem / a.W, xx = rem - yy * a.W;
            xbase[i] = (long)m * a.CT + 8 * khalf;
#pragma unroll
            for (int t = 0; t < 9; ++t) {
                const int iy = yy + t / 3 - 1, ix = xx + t % 3 - 1;
                if (iy >= 0 && iy < a.H && ix >= 0 && ix < a.W) tmask[i] |= 1u << t;
            }
        }
    }

    const int nkb = a.K >> 4;
    const int nsteps = 9 * nkb;
    int tap = 0, kb = 0;                                   // of the step being LOADED
    f32x4 xlo[TM], xhi[TM];
    u32x4 wr[NWR];
    auto load_step = [&](int s) {
        const int dy = tap / 3 - 1, dx = tap % 3 - 1;
        const long toff = ((long)dy * a.W + dx) * a.CT + 16 * kb;
#pragma unroll
        for (int i = 0; i < TM; ++i) {
            const bool ok = (tmask[i] >> tap) & 1;
            const float* p = a.feat + (ok ? xbase[i] + toff : 0);          // (a masked lane reads channels 0..15 of pixel 0: below K)
            const f32x4 lo = *reinterpret_cast<const f32x4*>(p), hi = *reinterpret_cast<const f32x4*>(p + 4);
            xlo[i] = ok ? lo : (f32x4){0.f, 0.f, 0.f, 0.f};
            xhi[i] = ok ? hi : (f32x4){0.f, 0.f, 0.f, 0.f};
        }
        const char* src = reinterpret_cast<const char*>(a.wpack) + (long)s * CH;
#pragma unroll
        for (int r = 0; r < NWR; ++r) {
            const int o = (r * 256 + tid) * 16;
            if (CH % 4096 == 0 || o < CH) wr[r] = *reinterpret_cast<const u32x4*>(src + o);
        }
        if (++kb == nkb) { kb = 0; ++tap; }
    };
    auto store_w = [&](int buf) {
#pragma unroll
        for (int r = 0; r < NWR; ++r) {
            const int o = (r * 256 + tid) * 16;
            if (CH % 4096 == 0 || o < CH) *reinterpret_cast<u32x4*>(lds + buf * CH + o) = wr[r];
        }
    };

#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;

    const int foff = l31 * 32 + khalf * 16;                // this lane's fragment inside a [32][16] bf16 panel

    load_step(0);
    store_w(0);
    __syncthreads();
#pragma unroll 1
    for (int s = 0; s < nsteps; ++s) {
        const int buf = s & 1;
        Split3 xs[TM];
#pragma unroll
        for (int i = 0; i < TM; ++i) xs[i] = split8(xlo[i], xhi[i]);
        if (s + 1 < nsteps) load_step(s + 1);              // in flight during the MFMAs below
        const char* wb = lds + buf * CH + foff;
        // the six slice products, grouped by weight slice: (0,2) (0,1) (0,0) | (1,1) (1,0) | (2,0)
#pragma unroll
        for (int wsl = 0; wsl < 3; ++wsl) {
            u32x4 wf[TN];
#pragma unroll
            for (int j = 0; j < TN; ++j) wf[j] = *reinterpret_cast<const u32x4*>(wb + (wsl * COUT + 32 * j) * 32);
#pragma unroll
            for (int xsl = 2 - wsl; xsl >= 0; --xsl)
#pragma unroll
                for (int i = 0; i < TM; ++i)
#pragma unroll
                    for (int j = 0; j < TN; ++j) acc[i][j] = mfma_bf16(wf[j], xs[i].s[xsl], acc[i][j]);
        }
        if (s + 1 < nsteps) store_w(buf ^ 1);              // nobody reads that buffer during this step
        __syncthreads();
    }
    return m0;
}

template <int TN, int TM>
__global__ __launch_bounds__(256) void dense_layer_kernel(DenseArgs a) {
    __shared__ __attribute__((aligned(16))) char lds[GatherLds<TN>::BYTES];
    f32x16 acc[TM][TN];
    const int m0 = dense_gemm<TN, TM>(a, lds, acc);
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

bool layer_width_ok(int R) { return R == 32 || R == 64 || R == 96 || R == 128; }
bool pack_ok(int K, int R) { return K >= 16 && K % 16 == 0 && layer_width_ok(R) && (long long)K * R * 9 < (1ll << 31); }

}  // namespace

extern "C" {

int dmc_dense_supported(int N, int H, int W, int CT, int K, int R) {
    if (N <= 0 || H <= 0 || W <= 0 || CT <= 0 || CT % 4 != 0 || K < 16 || K % 16 != 0) return 0;
    if ((long long)N * H * W * CT >= (1ll << 31)) return 0;
    if (R == 2) return (K <= CT && K <= HEAD_KMAX && K % 4 == 0) ? 1 : 0;
    return (layer_width_ok(R) && (long long)K + R <= CT) ? 1 : 0;
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
