// EstimatorDenseNetTinyEarlyFusionSum / EstimatorDenseNetTinyEarlyFusionStack (code/dmcnet/model.py:197-250), forward and backward:
//   m = LeakyReLU_0.1(conv_0_mv(x[:, :2])), r = LeakyReLU_0.1(conv_0_r(x[:, 2:]));  x = cat(m, r) (Stack) or m + r (Sum)
//   for i in 1..4: x = cat(LeakyReLU_0.1(conv_i(x)), x);  predict_flow(x)
// without a concatenation.  The widest layer has 8 output channels and the longest contraction 36: every layer is a "head-like"
// layer (dense_eval.hip's dense_head_kernel, dense_train.hip's head kernels), so everything here is plain fp32 fmaf in a fixed
// order, weights in LDS read as broadcasts, Cout accumulators per lane (templated, in registers), pixels read as 16-byte pieces.
//
// ONE NHWC fp32 feature buffer feat[M][CT] (M = N H W) per frame range, slots in production order, every slot padded with +0.0
// to a multiple of 4 channels (ops.early_fusion_layout):
//   Sum    s (0, 8)            y1 (8, 8)   y2 (16, 6)  y3 (24, 4)  y4 (28, 2)   CT 32
//   Stack  m (0, 8) r (8, 8)   y1 (16, 8)  y2 (24, 6)  y3 (32, 4)  y4 (36, 2)   CT 40
// The host permutes each weight's input channels into buffer order, with zero columns for the pad channels.
//
//   first        x NCHW [N][5][H][W] -> slot(s) of the base; a = conv_0_mv, b = conv_0_r each summed in its own fixed order (tap
//                outer, input channel inner, bias last), so Sum and Stack see the same a and b bits; optional sign plane
//                uint16 [M]: bit c = (a_c > 0), bit 8 + c = (b_c > 0)
//   layer        feat[m][K, K + R) = leaky(conv3x3(feat[.][0, K)) + bias), pads up to round_up4(R) = +0.0; IN PLACE
//   head         out NCHW [N][2][H][W] = conv3x3(feat[.][0, K)) + bias
//   head dgrad   G[m][c] = sum_t sum_co dout[m - o(t)][co] w[co][t][c], c < K; 0 for K <= c < CT: every float of G
//   head wgrad   dw [2][9][K], db [2]
//   layer mask   G[m][K + r] <- feat[m][K + r] > 0 ? g : 0.1f g over the padded slot, db [R] = sums of the result
//   layer wgrad  dw [R][9][K] = sum_m G[m][K + r] feat[m + o(t)][c]
//   layer dgrad  G[m][c] += sum_t sum_r G[m - o(t)][K + r] w[r][t][c], c < K; IN PLACE
//   first bwd    the weight and bias gradients of conv_0_mv and conv_0_r from G's base slot, x and the branch of each of the
//                two LeakyReLUs (the sign plane for Sum, the stored m and r for Stack: leaky(v) > 0 exactly when v > 0)
//
// The layer and the data gradient run IN PLACE through one non-const pointer.  A layer launch READS channels < K (of its own and
// of the neighbouring pixels) and WRITES channels [K, K + round_up4(R)) of its own pixel; a data-gradient launch reads
// [K, K + round_up4(R)) and writes channels < K of its own pixel, each (pixel, channel) by exactly one lane.  The bytes read and
// the bytes written are disjoint sets of the same buffer, so no workgroup can observe another's stores whatever the order in
// which they run: dense_eval.hip's argument, unchanged.  (K + round_up4(R) <= CT keeps every access inside the pixel's row.)
//
// Every sum over pixels (the weight and bias gradients) is formed by one thread over a run of at most PART_PIX = 1024
// consecutive pixels in order (the mask pass: 1024 pixels a workgroup, thread partials added in thread order); the runs'
// partial sums go to the caller's workspace and are added in run order by ef_reduce_kernel.  No atomics anywhere: results are
// bit-identical from run to run, and a forward result does not depend on the batch a frame is in.  All tensor offsets are
// 64-bit; dmc_ef_supported() bounds N H W CT below 2^31 so that a pixel index fits an int.  The caller owns every buffer;
// nothing allocates or synchronises.
#include "dmc_common.h"

using namespace dmc;

namespace {

constexpr float SLOPE = 0.1f;
constexpr int CT_MAX = 64;                   // channels per pixel of the buffer: bounds the LDS weight tiles
constexpr int PART_PIX = 1024;               // pixels per partial sum of a weight gradient (<= 8192)
constexpr int MASK_PIX = 1024;               // pixels per workgroup of the mask pass
constexpr int FIRST_W = 360;                 // conv_0_mv [8][2][9] and conv_0_r [8][3][9]
constexpr int FIRST_PART = FIRST_W + 16;     // ... and the two biases' gradients

inline int up4(int r) { return (r + 3) & ~3; }
inline bool width_ok(int r) { return r == 2 || r == 4 || r == 6 || r == 8; }
inline int parts_of(long long M) { return (int)((M + PART_PIX - 1) / PART_PIX); }

__device__ __forceinline__ float leaky(float v) { return v > 0.f ? v : SLOPE * v; }

// ---- first: one thread per pixel.  LDS: [tap][40] = conv_0_mv's (c, i) then conv_0_r's (c, i) at that tap; then the two biases ----
__global__ __launch_bounds__(256) void ef_first_kernel(const float* __restrict__ x, const float* __restrict__ wmv, const float* __restrict__ bmv,
                                                       const float* __restrict__ wr, const float* __restrict__ br, float* __restrict__ feat,
                                                       unsigned short* __restrict__ signs, int H, int W, int CT, int M, int stack) {
    __shared__ __attribute__((aligned(16))) float ws[9 * 40 + 16];
    for (int i = threadIdx.x; i < FIRST_PART; i += 256) {
        float v;
        if (i < FIRST_W) {
            const int t = i / 40, j = i - t * 40;
            v = j < 16 ? wmv[j * 9 + t] : wr[(j - 16) * 9 + t];
        } else {
            v = i < FIRST_W + 8 ? bmv[i - FIRST_W] : br[i - FIRST_W - 8];
        }
        ws[i] = v;
    }
    __syncthreads();
    const int m = blockIdx.x * 256 + threadIdx.x;
    if (m >= M) return;
    const int hw = H * W;
    const int n = m / hw, rem = m - n * hw;
    const int yy = rem / W, xx = rem - yy * W;
    const float* xp = x + (long)n * 5 * hw + rem;
    float a[8], b[8];
#pragma unroll
    for (int c = 0; c < 8; ++c) { a[c] = 0.f; b[c] = 0.f; }
#pragma unroll
    for (int t = 0; t < 9; ++t) {
        const int dy = t / 3 - 1, dx = t % 3 - 1;
        const int iy = yy + dy, ix = xx + dx;
        if (!(iy >= 0 && iy < H && ix >= 0 && ix < W)) continue;          // a tap outside the frame adds nothing
        const float* q = xp + dy * W + dx;
        const float v0 = q[0], v1 = q[hw], v2 = q[2 * (long)hw], v3 = q[3 * (long)hw], v4 = q[4 * (long)hw];
        const float* wt = ws + t * 40;
#pragma unroll
        for (int c = 0; c < 8; ++c) {
            a[c] = fmaf(v0, wt[2 * c], a[c]);
            a[c] = fmaf(v1, wt[2 * c + 1], a[c]);
            b[c] = fmaf(v2, wt[16 + 3 * c], b[c]);
            b[c] = fmaf(v3, wt[16 + 3 * c + 1], b[c]);
            b[c] = fmaf(v4, wt[16 + 3 * c + 2], b[c]);
        }
    }
    unsigned bitsv = 0;
#pragma unroll
    for (int c = 0; c < 8; ++c) {
        a[c] += ws[FIRST_W + c];
        b[c] += ws[FIRST_W + 8 + c];
        bitsv |= (a[c] > 0.f ? 1u : 0u) << c;
        bitsv |= (b[c] > 0.f ? 1u : 0u) << (8 + c);
        a[c] = leaky(a[c]);
        b[c] = leaky(b[c]);
    }
    f32x4* fp = reinterpret_cast<f32x4*>(feat + (long)m * CT);
    if (stack) {
        fp[0] = f32x4{a[0], a[1], a[2], a[3]};
        fp[1] = f32x4{a[4], a[5], a[6], a[7]};
        fp[2] = f32x4{b[0], b[1], b[2], b[3]};
        fp[3] = f32x4{b[4], b[5], b[6], b[7]};
    } else {
        fp[0] = f32x4{a[0] + b[0], a[1] + b[1], a[2] + b[2], a[3] + b[3]};
        fp[1] = f32x4{a[4] + b[4], a[5] + b[5], a[6] + b[6], a[7] + b[7]};
    }
    if (signs) signs[m] = (unsigned short)bitsv;
}

// ---- layer (HEAD = false) and head (HEAD = true): one thread per pixel, RR accumulators.  w [R][9][K] in buffer order.
// LDS: [tap][channel quad][r][4], rows r >= R zero.  A pixel's sum runs over the taps in order, the channels in order, the bias last ----
template <int RR, bool HEAD>
__global__ __launch_bounds__(256) void ef_conv_kernel(float* feat, const float* __restrict__ w, const float* __restrict__ bias,
                                                      float* __restrict__ out, int H, int W, int CT, int K, int R, int M) {
    __shared__ __attribute__((aligned(16))) float ws[RR * 9 * CT_MAX];
    const int nq = K >> 2;
    for (int i = threadIdx.x; i < RR * 9 * K; i += 256) {
        const int e = i & 3, r = (i >> 2) % RR, tq = (i >> 2) / RR;
        const int q = tq % nq, t = tq / nq;
        ws[i] = r < R ? w[((long)r * 9 + t) * K + 4 * q + e] : 0.f;
    }
    __syncthreads();
    const int m = blockIdx.x * 256 + threadIdx.x;
    if (m >= M) return;
    const int hw = H * W;
    const int n = m / hw, rem = m - n * hw;
    const int yy = rem / W, xx = rem - yy * W;
    float acc[RR];
#pragma unroll
    for (int r = 0; r < RR; ++r) acc[r] = 0.f;
#pragma unroll 1
    for (int t = 0; t < 9; ++t) {
        const int dy = t / 3 - 1, dx = t % 3 - 1;
        const int iy = yy + dy, ix = xx + dx;
        if (!(iy >= 0 && iy < H && ix >= 0 && ix < W)) continue;          // a tap outside the frame adds nothing
        const float* xp = feat + ((long)m + (long)dy * W + dx) * CT;
        const f32x4* wt = reinterpret_cast<const f32x4*>(ws) + t * nq * RR;
#pragma unroll 2
        for (int q = 0; q < nq; ++q) {
            const f32x4 xv = *reinterpret_cast<const f32x4*>(xp + 4 * q);
#pragma unroll
            for (int r = 0; r < RR; ++r) {
                const f32x4 wv = wt[q * RR + r];
#pragma unroll
                for (int e = 0; e < 4; ++e) acc[r] = fmaf(xv[e], wv[e], acc[r]);
            }
        }
    }
    if (HEAD) {
#pragma unroll
        for (int r = 0; r < RR; ++r) out[((long)n * 2 + r) * hw + rem] = acc[r] + bias[r];
    } else {
        float* op = feat + (long)m * CT + K;
#pragma unroll
        for (int j = 0; j < RR / 4; ++j) {
            f32x4 v;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int r = 4 * j + e;
                v[e] = r < R ? leaky(acc[r] + bias[r]) : 0.f;            // pad channels: +0.0
            }
            *reinterpret_cast<f32x4*>(op + 4 * j) = v;
        }
    }
}

// ---- head, data gradient: every float of G.  w [2][9][K]; LDS [co][tap][CT], zero from K on.  Eight lanes share a pixel and
// write 128 contiguous bytes at a time (dense_train.hip's head_dgrad_kernel) ----
__global__ __launch_bounds__(256) void ef_head_dgrad_kernel(const float* __restrict__ dout, const float* __restrict__ w, float* __restrict__ G,
                                                            int H, int W, int CT, int K, int M) {
    __shared__ __attribute__((aligned(16))) float ws[18 * CT_MAX];
    for (int i = threadIdx.x; i < 18 * CT; i += 256) {
        const int row = i / CT, c = i - row * CT;
        ws[i] = c < K ? w[row * K + c] : 0.f;
    }
    __syncthreads();
    const int q = threadIdx.x & 7;
    const int hw = H * W;
    const int nq = CT >> 2;
#pragma unroll 1
    for (int g = 0; g < 4; ++g) {                                          // 4 x 32 pixels per workgroup
        const int m = blockIdx.x * 128 + g * 32 + (threadIdx.x >> 3);
        if (m >= M) continue;
        const int n = m / hw, rem = m - n * hw;
        const int yy = rem / W, xx = rem - yy * W;
        float d0[9], d1[9];
#pragma unroll
        for (int t = 0; t < 9; ++t) {                                      // the output pixel m - o(t), tested per coordinate
            const int py = yy - (t / 3 - 1), px = xx - (t % 3 - 1);
            const bool ok = py >= 0 && py < H && px >= 0 && px < W;
            const long o = (long)n * 2 * hw + (ok ? py * W + px : 0);
            const float a0 = dout[o], a1 = dout[o + hw];
            d0[t] = ok ? a0 : 0.f;
            d1[t] = ok ? a1 : 0.f;
        }
        float* gp = G + (long)m * CT;
#pragma unroll 1
        for (int c = q; c < nq; c += 8) {
            f32x4 s = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int t = 0; t < 9; ++t) {
                const f32x4 a0 = *reinterpret_cast<const f32x4*>(ws + t * CT + 4 * c);
                const f32x4 a1 = *reinterpret_cast<const f32x4*>(ws + (9 + t) * CT + 4 * c);
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    s[e] = fmaf(d0[t], a0[e], s[e]);
                    s[e] = fmaf(d1[t], a1[e], s[e]);
                }
            }
            *reinterpret_cast<f32x4*>(gp + 4 * c) = s;
        }
    }
}

// ---- weight gradient of a layer (HEAD = false: dy = G[.][K, K + RR)) or of the head (HEAD = true: dy = dout NCHW, RR = 2, and the
// bias gradient).  A thread owns (run p of PART_PIX pixels, tap t, channel quad q): 4 RR accumulators over the run's pixels in
// order.  part: [parts][R][9][K], then for the head [parts][2] ----
template <int RR, bool HEAD>
__global__ __launch_bounds__(256) void ef_wgrad_kernel(const float* __restrict__ feat, const float* __restrict__ dy, float* __restrict__ part,
                                                       int H, int W, int CT, int K, int R, int M, int parts) {
    const int nq = K >> 2, T = 9 * nq;
    const long gid = (long)blockIdx.x * 256 + threadIdx.x;
    const int p = (int)(gid / T);
    if (p >= parts) return;
    const int j = (int)(gid - (long)p * T);
    const int t = j / nq, q = j - t * nq;
    const int dy_ = t / 3 - 1, dx_ = t % 3 - 1;
    const long toff = ((long)dy_ * W + dx_) * CT + 4 * q;
    const int hw = H * W;
    const int m0 = p * PART_PIX;
    const int m1 = m0 + PART_PIX < M ? m0 + PART_PIX : M;
    int n = m0 / hw, rem = m0 - n * hw;
    int yy = rem / W, xx = rem - yy * W;
    f32x4 acc[RR];
#pragma unroll
    for (int r = 0; r < RR; ++r) acc[r] = f32x4{0.f, 0.f, 0.f, 0.f};
    float b0 = 0.f, b1 = 0.f;
#pragma unroll 1
    for (int m = m0; m < m1; ++m) {
        float g[RR];
        if (HEAD) {
            const float* dp = dy + (long)n * 2 * hw + rem;
            g[0] = dp[0];
            g[1] = dp[hw];
            b0 += g[0];
            b1 += g[1];
        } else {
#pragma unroll
            for (int i = 0; i < RR / 4; ++i) {
                const f32x4 v = *reinterpret_cast<const f32x4*>(dy + (long)m * CT + K + 4 * i);
#pragma unroll
                for (int e = 0; e < 4; ++e) g[4 * i + e] = v[e];
            }
        }
        const int iy = yy + dy_, ix = xx + dx_;
        if (iy >= 0 && iy < H && ix >= 0 && ix < W) {
            const f32x4 xv = *reinterpret_cast<const f32x4*>(feat + (long)m * CT + toff);
#pragma unroll
            for (int r = 0; r < RR; ++r)
#pragma unroll
                for (int e = 0; e < 4; ++e) acc[r][e] = fmaf(g[r], xv[e], acc[r][e]);
        }
        ++rem;
        if (++xx == W) {
            xx = 0;
            if (++yy == H) { yy = 0; rem = 0; ++n; }
        }
    }
    float* out = part + (size_t)p * R * 9 * K + (size_t)t * K + 4 * q;
#pragma unroll
    for (int r = 0; r < RR; ++r)
        if (r < R) *reinterpret_cast<f32x4*>(out + (size_t)r * 9 * K) = acc[r];
    if (HEAD && j == 0) {
        float* pb = part + (size_t)parts * R * 9 * K + 2 * (size_t)p;
        pb[0] = b0;
        pb[1] = b1;
    }
}

// ---- out[i] = part[0][i] + part[1][i] + ... in order, i < numel; the partials are `stride` floats apart ----
__global__ __launch_bounds__(256) void ef_reduce_kernel(const float* __restrict__ part, float* __restrict__ out, int nparts, long stride, int numel) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= numel) return;
    float s = part[i];
    for (int k = 1; k < nparts; ++k) s += part[(size_t)k * stride + i];
    out[i] = s;
}

// ---- mask pass: the padded slot [K, K + R4) of G in place and the bias gradient's partial sums [workgroup][R4].  Thread =
// (pixel lane, channel quad); 256 / (R4 / 4) pixel lanes (dense_train.hip's mask_kernel) ----
__global__ __launch_bounds__(256) void ef_mask_kernel(const float* __restrict__ feat, float* __restrict__ G, float* __restrict__ part, int CT, int K,
                                                      int R4, int M) {
    __shared__ f32x4 red[256];
    const int nq = R4 >> 2, npl = 256 / nq;
    const int q = threadIdx.x % nq, pl = threadIdx.x / nq;
    const int p0 = blockIdx.x * MASK_PIX;
    const int p1 = p0 + MASK_PIX < M ? p0 + MASK_PIX : M;
    f32x4 s = {0.f, 0.f, 0.f, 0.f};
#pragma unroll 1
    for (int p = p0 + pl; p < p1; p += npl) {
        const long o = (long)p * CT + K + 4 * q;
        const f32x4 f = *reinterpret_cast<const f32x4*>(feat + o);
        const f32x4 g = *reinterpret_cast<const f32x4*>(G + o);
        f32x4 v;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            v[e] = f[e] > 0.f ? g[e] : SLOPE * g[e];
            s[e] += v[e];
        }
        *reinterpret_cast<f32x4*>(G + o) = v;
    }
    red[threadIdx.x] = s;
    __syncthreads();
    if (threadIdx.x < nq) {
        f32x4 t = red[threadIdx.x];
        for (int j = 1; j < npl; ++j) {
            const f32x4 u = red[j * nq + threadIdx.x];
#pragma unroll
            for (int e = 0; e < 4; ++e) t[e] += u[e];
        }
        *reinterpret_cast<f32x4*>(part + (size_t)blockIdx.x * R4 + 4 * threadIdx.x) = t;
    }
}

// ---- layer, data gradient: one thread per pixel.  The nine taps' RR slot values in registers (zeros outside the frame), then
// per channel quad: read, add the taps in order (r inner), write.  LDS: [quad][tap][r][4] = w[r][tap][4 quad + e], rows r >= R zero ----
template <int RR>
__global__ __launch_bounds__(256) void ef_dgrad_kernel(float* G, const float* __restrict__ w, int H, int W, int CT, int K, int R, int M) {
    __shared__ __attribute__((aligned(16))) float ws[RR * 9 * CT_MAX];
    const int nq = K >> 2;
    for (int i = threadIdx.x; i < RR * 9 * K; i += 256) {
        const int e = i & 3, r = (i >> 2) % RR, qt = (i >> 2) / RR;
        const int t = qt % 9, q = qt / 9;
        ws[i] = r < R ? w[((long)r * 9 + t) * K + 4 * q + e] : 0.f;
    }
    __syncthreads();
    const int m = blockIdx.x * 256 + threadIdx.x;
    if (m >= M) return;
    const int hw = H * W;
    const int rem = m % hw;
    const int yy = rem / W, xx = rem - yy * W;
    float g[9][RR];
#pragma unroll
    for (int t = 0; t < 9; ++t) {                                          // the output pixel m - o(t), tested per coordinate
        const int dy = t / 3 - 1, dx = t % 3 - 1;
        const int py = yy - dy, px = xx - dx;
        const bool ok = py >= 0 && py < H && px >= 0 && px < W;
        const float* gp = G + ((long)m - (ok ? (long)dy * W + dx : 0)) * CT + K;
#pragma unroll
        for (int i = 0; i < RR / 4; ++i) {
            const f32x4 v = *reinterpret_cast<const f32x4*>(gp + 4 * i);
#pragma unroll
            for (int e = 0; e < 4; ++e) g[t][4 * i + e] = ok ? v[e] : 0.f;
        }
    }
    float* op = G + (long)m * CT;
    const f32x4* w4 = reinterpret_cast<const f32x4*>(ws);
#pragma unroll 1
    for (int q = 0; q < nq; ++q) {
        f32x4 s = *reinterpret_cast<const f32x4*>(op + 4 * q);
#pragma unroll
        for (int t = 0; t < 9; ++t)
#pragma unroll
            for (int r = 0; r < RR; ++r) {
                const f32x4 wv = w4[(q * 9 + t) * RR + r];
#pragma unroll
                for (int e = 0; e < 4; ++e) s[e] = fmaf(g[t][r], wv[e], s[e]);
            }
        *reinterpret_cast<f32x4*>(op + 4 * q) = s;
    }
}

// ---- first, backward: a thread owns (run p of PART_PIX pixels, input channel i of x, tap t): the eight output channels'
// gradients of conv_0_mv (i < 2) or conv_0_r (i >= 2), and the bias gradient.  The LeakyReLU's branch: the sign plane (Sum) or
// the stored activation (Stack).  part: [parts][376] = dw_mv [8][2][9] | dw_r [8][3][9] | db_mv [8] | db_r [8] ----
__global__ __launch_bounds__(256) void ef_first_bwd_kernel(const float* __restrict__ G, const float* __restrict__ x, const unsigned short* __restrict__ signs,
                                                           const float* __restrict__ feat, float* __restrict__ part, int H, int W, int CT, int M,
                                                           int parts, int stack) {
    const long gid = (long)blockIdx.x * 256 + threadIdx.x;
    const int p = (int)(gid / 45);
    if (p >= parts) return;
    const int j = (int)(gid - (long)p * 45);
    const int i = j / 9, t = j - i * 9;
    const bool mv = i < 2;
    const int dy = t / 3 - 1, dx = t % 3 - 1;
    const int slot = (stack && !mv) ? 8 : 0;
    const int hw = H * W;
    const int m0 = p * PART_PIX;
    const int m1 = m0 + PART_PIX < M ? m0 + PART_PIX : M;
    int n = m0 / hw, rem = m0 - n * hw;
    int yy = rem / W, xx = rem - yy * W;
    float acc[8], bacc[8];
#pragma unroll
    for (int c = 0; c < 8; ++c) { acc[c] = 0.f; bacc[c] = 0.f; }
#pragma unroll 1
    for (int m = m0; m < m1; ++m) {
        const float* gp = G + (long)m * CT + slot;
        const f32x4 g0 = *reinterpret_cast<const f32x4*>(gp), g1 = *reinterpret_cast<const f32x4*>(gp + 4);
        unsigned pos = 0;
        if (stack) {
            const float* fp = feat + (long)m * CT + slot;
            const f32x4 f0 = *reinterpret_cast<const f32x4*>(fp), f1 = *reinterpret_cast<const f32x4*>(fp + 4);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                pos |= (f0[e] > 0.f ? 1u : 0u) << e;
                pos |= (f1[e] > 0.f ? 1u : 0u) << (4 + e);
            }
        } else {
            const unsigned s = signs[m];
            pos = mv ? (s & 0xffu) : (s >> 8);
        }
        float gm[8];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            gm[e] = (pos >> e) & 1u ? g0[e] : SLOPE * g0[e];
            gm[4 + e] = (pos >> (4 + e)) & 1u ? g1[e] : SLOPE * g1[e];
        }
#pragma unroll
        for (int c = 0; c < 8; ++c) bacc[c] += gm[c];
        const int iy = yy + dy, ix = xx + dx;
        if (iy >= 0 && iy < H && ix >= 0 && ix < W) {
            const float xv = x[((long)n * 5 + i) * hw + rem + dy * W + dx];
#pragma unroll
            for (int c = 0; c < 8; ++c) acc[c] = fmaf(gm[c], xv, acc[c]);
        }
        ++rem;
        if (++xx == W) {
            xx = 0;
            if (++yy == H) { yy = 0; rem = 0; ++n; }
        }
    }
    float* out = part + (size_t)p * FIRST_PART;
#pragma unroll
    for (int c = 0; c < 8; ++c) {
        if (mv) out[(c * 2 + i) * 9 + t] = acc[c];
        else out[144 + (c * 3 + (i - 2)) * 9 + t] = acc[c];
    }
    if (j == 0 || j == 18) {                                               // (i, t) = (0, 0): db_mv; (2, 0): db_r
#pragma unroll
        for (int c = 0; c < 8; ++c) out[FIRST_W + (mv ? 0 : 8) + c] = bacc[c];
    }
}

bool geom_ok(int N, int H, int W, int CT) {
    return N > 0 && H > 0 && W > 0 && CT > 0 && CT % 4 == 0 && CT <= CT_MAX && (long long)N * H * W * CT < (1ll << 31);
}
bool pix_ok(int N, int H, int W) { return N > 0 && H > 0 && W > 0 && (long long)N * H * W < (1ll << 31); }

int reduce(const float* part, float* out, int nparts, long stride, int numel, hipStream_t s, const char* what) {
    ef_reduce_kernel<<<(numel + 255) / 256, 256, 0, s>>>(part, out, nparts, stride, numel);
    return check_launch(what);
}

}  // namespace

extern "C" {

int dmc_ef_supported(int N, int H, int W, int CT, int K, int R) {
    if (!geom_ok(N, H, W, CT) || K <= 0 || K % 4 != 0 || !width_ok(R)) return 0;
    if (K + up4(R) <= CT) return 1;                       // a layer (and a head that leaves room)
    return (R == 2 && K <= CT) ? 1 : 0;                   // the head
}

size_t dmc_ef_head_wgrad_workspace_bytes(int N, int H, int W, int K) {
    if (!pix_ok(N, H, W) || K <= 0 || K % 4 != 0 || K > CT_MAX) return 0;
    return (size_t)parts_of((long long)N * H * W) * (18 * K + 2) * sizeof(float);
}

size_t dmc_ef_layer_wgrad_workspace_bytes(int N, int H, int W, int K, int R) {
    if (!pix_ok(N, H, W) || K <= 0 || K % 4 != 0 || K > CT_MAX || !width_ok(R)) return 0;
    return (size_t)parts_of((long long)N * H * W) * R * 9 * K * sizeof(float);
}

size_t dmc_ef_layer_mask_workspace_bytes(int N, int H, int W, int R) {
    if (!pix_ok(N, H, W) || !width_ok(R)) return 0;
    const long long M = (long long)N * H * W;
    return (size_t)((M + MASK_PIX - 1) / MASK_PIX) * up4(R) * sizeof(float);
}

size_t dmc_ef_first_bwd_workspace_bytes(int N, int H, int W) {
    if (!pix_ok(N, H, W)) return 0;
    return (size_t)parts_of((long long)N * H * W) * FIRST_PART * sizeof(float);
}

int dmc_ef_first(const float* x_nchw, const float* w_mv, const float* b_mv, const float* w_r, const float* b_r, float* feat,
                 unsigned short* signs, int N, int H, int W, int CT, int stack, dmc_stream_t stream) {
    if (!x_nchw || !w_mv || !b_mv || !w_r || !b_r || !feat) return fail(DMC_E_INVALID, "dmc_ef_first: null pointer");
    if (!geom_ok(N, H, W, CT) || CT < (stack ? 16 : 8) || (stack != 0 && stack != 1))
        return fail(DMC_E_INVALID, "dmc_ef_first: unsupported shape (N %d, H %d, W %d, CT %d, stack %d)", N, H, W, CT, stack);
    const int M = N * H * W;
    ef_first_kernel<<<(M + 255) / 256, 256, 0, (hipStream_t)stream>>>(x_nchw, w_mv, b_mv, w_r, b_r, feat, signs, H, W, CT, M, stack);
    return check_launch("dmc_ef_first");
}

int dmc_ef_layer(float* feat, const float* w, const float* bias, int N, int H, int W, int CT, int K, int R, dmc_stream_t stream) {
    if (!feat || !w || !bias) return fail(DMC_E_INVALID, "dmc_ef_layer: null pointer");
    if (!dmc_ef_supported(N, H, W, CT, K, R) || K + up4(R) > CT)
        return fail(DMC_E_INVALID, "dmc_ef_layer: unsupported shape (N %d, H %d, W %d, CT %d, K %d, R %d)", N, H, W, CT, K, R);
    const int M = N * H * W;
    const dim3 grid((M + 255) / 256);
    hipStream_t s = (hipStream_t)stream;
    if (R > 4) ef_conv_kernel<8, false><<<grid, 256, 0, s>>>(feat, w, bias, nullptr, H, W, CT, K, R, M);
    else ef_conv_kernel<4, false><<<grid, 256, 0, s>>>(feat, w, bias, nullptr, H, W, CT, K, R, M);
    return check_launch("dmc_ef_layer");
}

int dmc_ef_head(const float* feat, const float* w, const float* bias, float* out_nchw, int N, int H, int W, int CT, int K, dmc_stream_t stream) {
    if (!feat || !w || !bias || !out_nchw) return fail(DMC_E_INVALID, "dmc_ef_head: null pointer");
    if (!dmc_ef_supported(N, H, W, CT, K, 2))
        return fail(DMC_E_INVALID, "dmc_ef_head: unsupported shape (N %d, H %d, W %d, CT %d, K %d)", N, H, W, CT, K);
    const int M = N * H * W;
    ef_conv_kernel<2, true><<<(M + 255) / 256, 256, 0, (hipStream_t)stream>>>(const_cast<float*>(feat), w, bias, out_nchw, H, W, CT, K, 2, M);
    return check_launch("dmc_ef_head");
}

int dmc_ef_head_dgrad(const float* dout_nchw, const float* w, float* G, int N, int H, int W, int CT, int K, dmc_stream_t stream) {
    if (!dout_nchw || !w || !G) return fail(DMC_E_INVALID, "dmc_ef_head_dgrad: null pointer");
    if (!dmc_ef_supported(N, H, W, CT, K, 2))
        return fail(DMC_E_INVALID, "dmc_ef_head_dgrad: unsupported shape (N %d, H %d, W %d, CT %d, K %d)", N, H, W, CT, K);
    const int M = N * H * W;
    ef_head_dgrad_kernel<<<(M + 127) / 128, 256, 0, (hipStream_t)stream>>>(dout_nchw, w, G, H, W, CT, K, M);
    return check_launch("dmc_ef_head_dgrad");
}

int dmc_ef_head_wgrad(const float* dout_nchw, const float* feat, float* dw, float* db, void* workspace, int N, int H, int W, int CT, int K,
                      dmc_stream_t stream) {
    if (!dout_nchw || !feat || !dw || !db || !workspace) return fail(DMC_E_INVALID, "dmc_ef_head_wgrad: null pointer");
    if (!dmc_ef_supported(N, H, W, CT, K, 2))
        return fail(DMC_E_INVALID, "dmc_ef_head_wgrad: unsupported shape (N %d, H %d, W %d, CT %d, K %d)", N, H, W, CT, K);
    const int M = N * H * W, parts = parts_of(M);
    float* part = reinterpret_cast<float*>(workspace);
    hipStream_t s = (hipStream_t)stream;
    const long threads = (long)parts * 9 * (K / 4);
    ef_wgrad_kernel<2, true><<<(int)((threads + 255) / 256), 256, 0, s>>>(feat, dout_nchw, part, H, W, CT, K, 2, M, parts);
    int rc = check_launch("dmc_ef_head_wgrad");
    if (rc) return rc;
    rc = reduce(part, dw, parts, 18l * K, 18 * K, s, "dmc_ef_head_wgrad");
    if (rc) return rc;
    return reduce(part + (size_t)parts * 18 * K, db, parts, 2, 2, s, "dmc_ef_head_wgrad");
}

int dmc_ef_layer_mask(const float* feat, float* G, float* db, void* workspace, int N, int H, int W, int CT, int K, int R, dmc_stream_t stream) {
    if (!feat || !G || !db || !workspace) return fail(DMC_E_INVALID, "dmc_ef_layer_mask: null pointer");
    if (!dmc_ef_supported(N, H, W, CT, K, R) || K + up4(R) > CT)
        return fail(DMC_E_INVALID, "dmc_ef_layer_mask: unsupported shape (N %d, H %d, W %d, CT %d, K %d, R %d)", N, H, W, CT, K, R);
    const int M = N * H * W;
    const int blocks = (M + MASK_PIX - 1) / MASK_PIX;
    float* part = reinterpret_cast<float*>(workspace);
    hipStream_t s = (hipStream_t)stream;
    ef_mask_kernel<<<blocks, 256, 0, s>>>(feat, G, part, CT, K, up4(R), M);
    const int rc = check_launch("dmc_ef_layer_mask");
    if (rc) return rc;
    return reduce(part, db, blocks, up4(R), R, s, "dmc_ef_layer_mask");
}

int dmc_ef_layer_wgrad(const float* feat, const float* G, float* dw, void* workspace, int N, int H, int W, int CT, int K, int R,
                       dmc_stream_t stream) {
    if (!feat || !G || !dw || !workspace) return fail(DMC_E_INVALID, "dmc_ef_layer_wgrad: null pointer");
    if (!dmc_ef_supported(N, H, W, CT, K, R) || K + up4(R) > CT)
        return fail(DMC_E_INVALID, "dmc_ef_layer_wgrad: unsupported shape (N %d, H %d, W %d, CT %d, K %d, R %d)", N, H, W, CT, K, R);
    const int M = N * H * W, parts = parts_of(M);
    float* part = reinterpret_cast<float*>(workspace);
    hipStream_t s = (hipStream_t)stream;
    const long threads = (long)parts * 9 * (K / 4);
    const int grid = (int)((threads + 255) / 256);
    if (R > 4) ef_wgrad_kernel<8, false><<<grid, 256, 0, s>>>(feat, G, part, H, W, CT, K, R, M, parts);
    else ef_wgrad_kernel<4, false><<<grid, 256, 0, s>>>(feat, G, part, H, W, CT, K, R, M, parts);
    const int rc = check_launch("dmc_ef_layer_wgrad");
    if (rc) return rc;
    return reduce(part, dw, parts, (long)R * 9 * K, R * 9 * K, s, "dmc_ef_layer_wgrad");
}

int dmc_ef_layer_dgrad(float* G, const float* w, int N, int H, int W, int CT, int K, int R, dmc_stream_t stream) {
    if (!G || !w) return fail(DMC_E_INVALID, "dmc_ef_layer_dgrad: null pointer");
    if (!dmc_ef_supported(N, H, W, CT, K, R) || K + up4(R) > CT)
        return fail(DMC_E_INVALID, "dmc_ef_layer_dgrad: unsupported shape (N %d, H %d, W %d, CT %d, K %d, R %d)", N, H, W, CT, K, R);
    const int M = N * H * W;
    const dim3 grid((M + 255) / 256);
    hipStream_t s = (hipStream_t)stream;
    if (R > 4) ef_dgrad_kernel<8><<<grid, 256, 0, s>>>(G, w, H, W, CT, K, R, M);
    else ef_dgrad_kernel<4><<<grid, 256, 0, s>>>(G, w, H, W, CT, K, R, M);
    return check_launch("dmc_ef_layer_dgrad");
}

int dmc_ef_first_bwd(const float* G, const float* x_nchw, const unsigned short* signs, const float* feat, float* dw_mv, float* db_mv,
                     float* dw_r, float* db_r, void* workspace, int N, int H, int W, int CT, int stack, dmc_stream_t stream) {
    if (!G || !x_nchw || !dw_mv || !db_mv || !dw_r || !db_r || !workspace || (stack ? !feat : !signs))
        return fail(DMC_E_INVALID, "dmc_ef_first_bwd: null pointer");
    if (!geom_ok(N, H, W, CT) || CT < (stack ? 16 : 8) || (stack != 0 && stack != 1))
        return fail(DMC_E_INVALID, "dmc_ef_first_bwd: unsupported shape (N %d, H %d, W %d, CT %d, stack %d)", N, H, W, CT, stack);
    const int M = N * H * W, parts = parts_of(M);
    float* part = reinterpret_cast<float*>(workspace);
    hipStream_t s = (hipStream_t)stream;
    const long threads = (long)parts * 45;
    ef_first_bwd_kernel<<<(int)((threads + 255) / 256), 256, 0, s>>>(G, x_nchw, signs, feat, part, H, W, CT, M, parts, stack);
    int rc = check_launch("dmc_ef_first_bwd");
    if (rc) return rc;
    if ((rc = reduce(part, dw_mv, parts, FIRST_PART, 144, s, "dmc_ef_first_bwd"))) return rc;
    if ((rc = reduce(part + 144, dw_r, parts, FIRST_PART, 216, s, "dmc_ef_first_bwd"))) return rc;
    if ((rc = reduce(part + FIRST_W, db_mv, parts, FIRST_PART, 8, s, "dmc_ef_first_bwd"))) return rc;
    return reduce(part + FIRST_W + 8, db_r, parts, FIRST_PART, 8, s, "dmc_ef_first_bwd");
}

}  // extern "C"
