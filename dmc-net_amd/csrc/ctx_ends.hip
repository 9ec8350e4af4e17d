// The two ends of ContextNetwork / ContextNetworkAtt in training (code/dmcnet/model.py:45-104; gfx950): the first unit's
// Conv2d(5, 32, 3, 1, 1, 1), the heads' Conv2d(32, 2, 3, 1, 1, 1) -- forward, data gradient, weight gradient -- and the heads'
// BatchNorm2d(2) (batch statistics) + LeakyReLU (+ ReLU behind predict_att), forward and backward.  With dconv.hip and
// ctx_bn.hip every convolution and every BatchNorm of a ContextNetwork training step is this library's.
//
// All arithmetic is fp32 with explicit fmaf (the build has -ffp-contract=off); every sum that crosses threads, workgroups or
// pixel ranges is added in one fixed order; no atomics: bit-identical from run to run.
//
// The six convolution passes are three kernels (o(t) = (t / 3 - 1, t % 3 - 1); MIRROR reads p - o(t) instead of p + o(t)):
//   planes_to_c32<MIRROR>   K in {5, 2, 4} NCHW planes in, NHWC [M][32] out: ctx_eval.hip's ctx_first_kernel without its
//                           epilogue -- one thread per pixel, 32 accumulators, the sum over (plane, ky, kx) in that order.
//                           First unit forward (K = 5); heads data gradient (K = 2 per head, MIRROR: both heads in one sum).
//   c32_to_planes<K, MIRROR> NHWC [M][32] in, K in {2, 4, 5} NCHW planes out: ctx_heads_kernel without its epilogue -- eight
//                           lanes per pixel, a channel quad each, the butterfly over lane distances 1, 2, 4.
//                           Heads forward (K = 2 per head, the trunk read once); first-unit data gradient (K = 5, MIRROR).
//   wgrad_partial<K, MIRROR> + wgrad_final: dW[k][t][c] = sum_p T[p][c] plane_k[p +- o(t)].  A workgroup takes a range of
//                           RANGE = 2048 pixels; thread (c = tid & 31, g = tid >> 5) keeps acc[K][9] for channel c over the
//                           range's pixels = g (mod 8) (a 256-long fp32 chain at most), reads its row of T coalesced and the
//                           9 K plane values as broadcasts -- from a copy of the range's planes (and a row either side) in LDS
//                           where that fits 64 KB (W <= 383 at K = 5), from global memory otherwise; the eight groups are added
//                           in order through LDS (fp32), the ranges in order in fp64 by wgrad_final, which writes OIHW (first
//                           unit) or OHWI per head.
// The heads' BatchNorm follows ctx_bn.hip on planes [N][2][H][W]: fp64 sums from the first addition, per-workgroup partials, a
// fixed-order final, (mean, invstd) rounded to fp32 once, the backward recomputes t and never reads y.  Element e of the flat
// tensor has channel (e / (H W)) & 1: scalar loads, so an odd H W (planes not 16-byte aligned) is the same code.  The grid is not
// capped: a thread owns BN_PER = 4 elements, a workgroup 1024.
// All tensor offsets are 64-bit; index_ok() bounds N H W so that pixel and element indices fit an int.
#include "ctx_common.h"

using namespace dmc;
using namespace dmc::ctxk;

namespace {

constexpr int RANGE = 2048;            // pixels of one weight-gradient workgroup
constexpr int BN_PER = 4;              // elements per thread of the BatchNorm kernels
constexpr int BN_TILE = 256 * BN_PER;

// K planes spread over up to two tensors of PT planes each: plane k is channel k % PT of tensor k / PT
struct Planes {
    const float* src[2];
    int PT;
};
struct PlanesOut {
    float* dst[2];
    int PT;
};

// ---- few planes in, 32 channels out ----
// ws[k * 9 + t][c]: the first unit's OIHW weight transposed (w[c][k][t]) or the heads' OHWI weights as they are (w_h[kk][t][c])
template <bool MIRROR>
__global__ __launch_bounds__(256) void planes_to_c32(Planes in, int K, const float* __restrict__ w0, const float* __restrict__ w1,
                                                     float* __restrict__ y, int H, int W, int M) {
    __shared__ __attribute__((aligned(16))) float ws[45 * 32];
    if (!MIRROR) {
        for (int i = threadIdx.x; i < 45 * 32; i += 256) ws[(i % 45) * 32 + i / 45] = w0[i];
    } else {
        for (int i = threadIdx.x; i < K * 288; i += 256) ws[i] = i < 576 ? w0[i] : w1[i - 576];
    }
    __syncthreads();
    const int m = blockIdx.x * 256 + threadIdx.x;
    if (m >= M) return;
    const int hw = H * W;
    const int n = m / hw, rem = m - n * hw;
    const int yy = rem / W, xx = rem - yy * W;
    float acc[32];
#pragma unroll
    for (int c = 0; c < 32; ++c) acc[c] = 0.f;
#pragma unroll 1
    for (int k = 0; k < K; ++k) {
        const int ti = k >= in.PT ? 1 : 0;
        const float* xp = (ti ? in.src[1] : in.src[0]) + ((long)n * in.PT + (k - ti * in.PT)) * hw;
#pragma unroll
        for (int t = 0; t < 9; ++t) {
            const int dy = MIRROR ? 1 - t / 3 : t / 3 - 1, dx = MIRROR ? 1 - t % 3 : t % 3 - 1;
            const int iy = yy + dy, ix = xx + dx;
            const bool ok = iy >= 0 && iy < H && ix >= 0 && ix < W;
            const float xv = ok ? xp[(long)iy * W + ix] : 0.f;
            const float* wk = ws + (k * 9 + t) * 32;
#pragma unroll
            for (int c = 0; c < 32; ++c) acc[c] = fmaf(xv, wk[c], acc[c]);
        }
    }
    float* yp = y + (long)m * 32;
#pragma unroll
    for (int q = 0; q < 8; ++q) {
        f32x4 v;
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = acc[4 * q + e];
        *reinterpret_cast<f32x4*>(yp + 4 * q) = v;
    }
}

// ---- 32 channels in, few planes out ----
// ws[k * 9 + t][c]: the heads' OHWI weights as they are, or the first unit's OIHW weight as w[c][k][t]
template <int K, bool MIRROR>
__global__ __launch_bounds__(256) void c32_to_planes(const float* __restrict__ x, const float* __restrict__ w0, const float* __restrict__ w1,
                                                     PlanesOut out, int H, int W, int M) {
    __shared__ __attribute__((aligned(16))) float ws[K * 288];
    if (MIRROR) {
        for (int i = threadIdx.x; i < 45 * 32; i += 256) ws[(i % 45) * 32 + i / 45] = w0[i];
    } else {
        for (int i = threadIdx.x; i < K * 288; i += 256) ws[i] = i < 576 ? w0[i] : w1[i - 576];
    }
    __syncthreads();
    const int q = threadIdx.x & 7;
    const int hw = H * W;
#pragma unroll 1
    for (int g = 0; g < 4; ++g) {                                          // 4 x 32 pixels per workgroup
        const int m = blockIdx.x * 128 + g * 32 + (threadIdx.x >> 3);
        const bool live = m < M;                                          // (no lane leaves before the lane exchanges below)
        const int mm = live ? m : 0;
        const int n = mm / hw, rem = mm - n * hw;
        const int yy = rem / W, xx = rem - yy * W;
        float acc[K];
#pragma unroll
        for (int k = 0; k < K; ++k) acc[k] = 0.f;
#pragma unroll
        for (int t = 0; t < 9; ++t) {
            const int dy = MIRROR ? 1 - t / 3 : t / 3 - 1, dx = MIRROR ? 1 - t % 3 : t % 3 - 1;
            const int iy = yy + dy, ix = xx + dx;
            const bool ok = iy >= 0 && iy < H && ix >= 0 && ix < W;
            const f32x4 xv = ok ? *reinterpret_cast<const f32x4*>(x + ((long)mm + (long)dy * W + dx) * 32 + 4 * q) : (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int k = 0; k < K; ++k) {
                const f32x4 wv = *reinterpret_cast<const f32x4*>(ws + (k * 9 + t) * 32 + 4 * q);
#pragma unroll
                for (int e = 0; e < 4; ++e) acc[k] = fmaf(xv[e], wv[e], acc[k]);
            }
        }
#pragma unroll
        for (int k = 0; k < K; ++k)
#pragma unroll
            for (int o = 1; o < 8; o <<= 1) acc[k] += __shfl_xor(acc[k], o);
        // lane q < K stores plane q
        float sum = acc[0];
#pragma unroll
        for (int k = 1; k < K; ++k) sum = q == k ? acc[k] : sum;
        if (live && q < K) {
            const int ti = q >= out.PT ? 1 : 0;
            (ti ? out.dst[1] : out.dst[0])[((long)n * out.PT + (q - ti * out.PT)) * hw + rem] = sum;
        }
    }
}

// ---- weight gradient of a (K planes) x (32 channels) pair ----
// partial[range][(k * 9 + t) * 32 + c] = sum over the range's pixels p of T[p][c] plane_k[p +- o(t)], groups added 0 .. 7
// STAGED: the workgroup first copies, per plane, the pixels [p0 - W - 1, p0 + RANGE + W + 1) -- every pixel a tap of the range can
// reach, in pixel order across frame boundaries -- into LDS (K (RANGE + 2 W + 2) floats, zero outside [0, M)); a tap inside the frame
// is then pixel p +- (dy W + dx) of that copy, a broadcast LDS read.  Host code takes this variant when the copy fits (staged_ok);
// otherwise the taps are read from global memory.  Both add the same products in the same order: the same bits.
template <int K, bool MIRROR, bool STAGED>
__global__ __launch_bounds__(256) void wgrad_partial(const float* __restrict__ T, Planes in, float* __restrict__ partial, int H, int W, int M) {
    __shared__ float sm[8][9 * 32];
    extern __shared__ float stage[];
    const int c = threadIdx.x & 31, g = threadIdx.x >> 5;
    const int hw = H * W;
    const int p0 = blockIdx.x * RANGE;
    const int p1 = p0 + RANGE < M ? p0 + RANGE : M;
    const int span = RANGE + 2 * W + 2, base = p0 - W - 1;
    if (STAGED) {
        for (int i = threadIdx.x; i < K * span; i += 256) {
            const int k = i / span, p = base + (i - k * span);
            float v = 0.f;
            if (p >= 0 && p < M) {
                const int n = p / hw, ti = k >= in.PT ? 1 : 0;
                v = (ti ? in.src[1] : in.src[0])[((long)n * in.PT + (k - ti * in.PT)) * hw + (p - n * hw)];
            }
            stage[i] = v;
        }
        __syncthreads();
    }
    float acc[K][9];
#pragma unroll
    for (int k = 0; k < K; ++k)
#pragma unroll
        for (int t = 0; t < 9; ++t) acc[k][t] = 0.f;
    float nxt[4];                                                    // this thread's next four pixels of T, one step ahead
#pragma unroll
    for (int j = 0; j < 4; ++j) nxt[j] = p0 + g + 8 * j < p1 ? T[(long)(p0 + g + 8 * j) * 32 + c] : 0.f;
#pragma unroll 1
    for (int pb = p0 + g; pb < p1; pb += 32) {
        float tvs[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            tvs[j] = nxt[j];
            nxt[j] = pb + 32 + 8 * j < p1 ? T[(long)(pb + 32 + 8 * j) * 32 + c] : 0.f;
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int p = pb + 8 * j;
            if (p >= p1) break;
            const float tv = tvs[j];
            const int n = p / hw, rem = p - n * hw;
            const int yy = rem / W, xx = rem - yy * W;
            int off[9];                                              // of the tap inside its plane, or inside the staged copy
            bool ok[9];
#pragma unroll
            for (int t = 0; t < 9; ++t) {
                const int dy = MIRROR ? 1 - t / 3 : t / 3 - 1, dx = MIRROR ? 1 - t % 3 : t % 3 - 1;
                const int iy = yy + dy, ix = xx + dx;
                ok[t] = iy >= 0 && iy < H && ix >= 0 && ix < W;
                off[t] = STAGED ? p - base + dy * W + dx : iy * W + ix;
            }
#pragma unroll
            for (int k = 0; k < K; ++k) {
                const int ti = k >= in.PT ? 1 : 0;
                const float* xp = STAGED ? stage + k * span : (ti ? in.src[1] : in.src[0]) + ((long)n * in.PT + (k - ti * in.PT)) * hw;
#pragma unroll
                for (int t = 0; t < 9; ++t) {
                    const float xv = ok[t] ? xp[off[t]] : 0.f;
                    acc[k][t] = fmaf(tv, xv, acc[k][t]);
                }
            }
        }
    }
    float* dst = partial + (long)blockIdx.x * (K * 288);
#pragma unroll
    for (int k = 0; k < K; ++k) {
#pragma unroll
        for (int t = 0; t < 9; ++t) sm[g][t * 32 + c] = acc[k][t];
        __syncthreads();
        for (int i = threadIdx.x; i < 288; i += 256) {
            float s = sm[0][i];
#pragma unroll
            for (int gg = 1; gg < 8; ++gg) s += sm[gg][i];
            dst[k * 288 + i] = s;
        }
        __syncthreads();
    }
}

// out element (k, t, c) = the ranges' partials added in order in fp64.  first != 0: dw OIHW [32][5][3][3] at c * 45 + k * 9 + t;
// else plane k belongs to head dst[k / 2], OHWI [2][3][3][32] at (k % 2) * 288 + t * 32 + c
__global__ __launch_bounds__(256) void wgrad_final(const float* __restrict__ partial, int nranges, int K, int first, float* dw0, float* dw1) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= K * 288) return;
    double s = 0.0;
    for (int r = 0; r < nranges; ++r) s += (double)partial[(long)r * (K * 288) + i];
    const int k = i / 288, t = (i % 288) / 32, c = i & 31;
    if (first) dw0[c * 45 + k * 9 + t] = (float)s;
    else (k >= 2 ? dw1 : dw0)[(k & 1) * 288 + t * 32 + c] = (float)s;
}

// ---- the heads' BatchNorm2d(2) + LeakyReLU (+ ReLU) on planes [N][2][H][W] ----
struct BnpArgs {
    const float* z;
    const float* dy;
    const float* gamma;
    const float* beta;
    const float* stats;       // mean[2], invstd[2]
    const float* means;       // backward: (sum g) / M [2], (sum g xhat) / M [2]
    float* out;               // y (forward) or dz (backward)
    int total;                // 2 M elements
    int hw;
    float slope;              // of t <= 0 in the forward
    float low;                // factor of dy where t <= 0: slope, or 0 under relu
    int relu;
};

__device__ __forceinline__ float bn_t(float v, float mean, float istd, float gamma, float beta) {
    return fmaf((v - mean) * istd, gamma, beta);
}

// adds v[0 .. 3] over the workgroup in a fixed tree (lanes, then the four waves in order); the sums are valid in thread 0
__device__ __forceinline__ void block_sum4(double (&v)[4]) {
    __shared__ double red[4][4];
#pragma unroll
    for (int k = 0; k < 4; ++k)
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) v[k] += __shfl_down(v[k], o, 64);
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int k = 0; k < 4; ++k) red[k][threadIdx.x >> 6] = v[k];
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 4; ++k) v[k] = red[k][0] + red[k][1] + red[k][2] + red[k][3];
}

// MODE 0: per channel (sum z, sum z^2).  MODE 1: (sum g, sum g xhat).  scratch [workgroup][channel][2] fp64
template <int MODE>
__global__ __launch_bounds__(256) void bnp_partial_kernel(BnpArgs a, double* __restrict__ scratch) {
    double v[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int j = 0; j < BN_PER; ++j) {
        const int e = blockIdx.x * BN_TILE + j * 256 + (int)threadIdx.x;
        if (e >= a.total) continue;
        const int c = (e / a.hw) & 1;
        const float x = a.z[e];
        double s0, s1;
        if (MODE == 0) {
            s0 = (double)x;
            s1 = s0 * s0;
        } else {
            const float xh = (x - a.stats[c]) * a.stats[2 + c];
            const float t = fmaf(xh, a.gamma[c], a.beta[c]);
            const float d = a.dy[e];
            const float g = t > 0.f ? d : d * a.low;
            s0 = (double)g;
            s1 = (double)g * (double)xh;
        }
        // (each product is exact in fp64; the additions below are the only roundings)
        v[0] += c == 0 ? s0 : 0.0;
        v[1] += c == 0 ? s1 : 0.0;
        v[2] += c == 1 ? s0 : 0.0;
        v[3] += c == 1 ? s1 : 0.0;
    }
    block_sum4(v);
    if (threadIdx.x == 0) {
#pragma unroll
        for (int k = 0; k < 4; ++k) scratch[(size_t)blockIdx.x * 4 + k] = v[k];
    }
}

// one workgroup: thread i adds partials i, i + 256, ... in order, then the fixed tree
__device__ __forceinline__ void reduce_partials(const double* __restrict__ scratch, int nblocks, double (&v)[4]) {
#pragma unroll
    for (int k = 0; k < 4; ++k) v[k] = 0.0;
    for (int b = threadIdx.x; b < nblocks; b += 256)
#pragma unroll
        for (int k = 0; k < 4; ++k) v[k] += scratch[(size_t)b * 4 + k];
    block_sum4(v);
}

__global__ __launch_bounds__(256) void bnp_stats_final_kernel(const double* __restrict__ scratch, float* __restrict__ stats,
                                                              float* __restrict__ running_mean, float* __restrict__ running_var, int M,
                                                              int nblocks, float eps, float momentum) {
    double v[4];
    reduce_partials(scratch, nblocks, v);
    if (threadIdx.x != 0) return;
    for (int c = 0; c < 2; ++c) {
        const double mean = v[2 * c] / (double)M;
        double var = v[2 * c + 1] / (double)M - mean * mean;
        if (var < 0.0) var = 0.0;
        stats[c] = (float)mean;
        stats[2 + c] = (float)(1.0 / sqrt(var + (double)eps));
        if (running_mean) {
            const double m = (double)momentum, unbiased = var * (double)M / (double)(M - 1);
            running_mean[c] = (float)((1.0 - m) * (double)running_mean[c] + m * mean);
            running_var[c] = (float)((1.0 - m) * (double)running_var[c] + m * unbiased);
        }
    }
}

__global__ __launch_bounds__(256) void bnp_bwd_final_kernel(const double* __restrict__ scratch, float* __restrict__ dgamma,
                                                            float* __restrict__ dbeta, float* __restrict__ means, int M, int nblocks) {
    double v[4];
    reduce_partials(scratch, nblocks, v);
    if (threadIdx.x != 0) return;
    for (int c = 0; c < 2; ++c) {
        dbeta[c] = (float)v[2 * c];
        dgamma[c] = (float)v[2 * c + 1];
        means[c] = (float)(v[2 * c] / (double)M);
        means[2 + c] = (float)(v[2 * c + 1] / (double)M);
    }
}

// BWD 0: y = t > 0 ? t : slope t (max(y, 0) under relu).   BWD 1: dz = gamma invstd (g - mean(g) - xhat mean(g xhat))
template <int BWD>
__global__ __launch_bounds__(256) void bnp_apply_kernel(BnpArgs a) {
#pragma unroll
    for (int j = 0; j < BN_PER; ++j) {
        const int e = blockIdx.x * BN_TILE + j * 256 + (int)threadIdx.x;
        if (e >= a.total) continue;
        const int c = (e / a.hw) & 1;
        const float istd = a.stats[2 + c], gam = a.gamma[c];
        const float xh = (a.z[e] - a.stats[c]) * istd;
        const float t = fmaf(xh, gam, a.beta[c]);
        float r;
        if (BWD) {
            const float d = a.dy[e];
            const float g = t > 0.f ? d : d * a.low;
            r = gam * istd * (g - a.means[c] - xh * a.means[2 + c]);
        } else {
            r = t > 0.f ? t : a.slope * t;
            if (a.relu) r = fmaxf(r, 0.f);
        }
        a.out[e] = r;
    }
}

int nranges_of(int M) { return (M + RANGE - 1) / RANGE; }
// bytes of wgrad_partial's staged copy, or 0 when it does not fit the 64 KB of a launch without opt-in (beside the 9 KB of sm)
size_t stage_bytes(int K, int W) {
    const size_t b = (size_t)K * ((size_t)RANGE + 2 * (size_t)W + 2) * sizeof(float);
    return b + 8 * 288 * sizeof(float) <= 65536 ? b : 0;
}
template <int K, bool MIRROR>
void launch_wgrad_partial(const float* T, const Planes& in, float* partial, int H, int W, int M, hipStream_t s) {
    const size_t sb = stage_bytes(K, W);
    if (sb) wgrad_partial<K, MIRROR, true><<<nranges_of(M), 256, sb, s>>>(T, in, partial, H, W, M);
    else wgrad_partial<K, MIRROR, false><<<nranges_of(M), 256, 0, s>>>(T, in, partial, H, W, M);
}
int bn_blocks_of(int M) { return (int)((2L * M + BN_TILE - 1) / BN_TILE); }
bool planes_ok(int planes) { return planes == 2 || planes == 4 || planes == 5; }
bool bn_shape_ok(int N, int H, int W) { return index_ok(N, H, W) && (long)N * H * W >= 2; }

}  // namespace

extern "C" {

int dmc_ctxends_supported(int N, int H, int W) { return index_ok(N, H, W) ? 1 : 0; }

size_t dmc_ctxends_wgrad_workspace_bytes(int N, int H, int W, int planes) {
    if (!index_ok(N, H, W) || !planes_ok(planes)) return 0;
    return (size_t)nranges_of(N * H * W) * planes * 288 * sizeof(float);
}

// partials [workgroups][2][2] fp64, then the backward's four means fp32 (the forward does not touch those)
size_t dmc_ctxends_bn_scratch_bytes(int N, int H, int W) {
    if (!bn_shape_ok(N, H, W)) return 0;
    return (size_t)bn_blocks_of(N * H * W) * 4 * sizeof(double) + 4 * sizeof(float);
}

int dmc_ctxends_first_fwd(const float* x, const float* w, float* z, int N, int H, int W, dmc_stream_t stream) {
    if (!x || !w || !z) return fail(DMC_E_INVALID, "dmc_ctxends_first_fwd: null pointer");
    if (!index_ok(N, H, W)) return fail(DMC_E_INVALID, "dmc_ctxends_first_fwd: unsupported shape (N %d, H %d, W %d)", N, H, W);
    const int M = N * H * W;
    Planes in = {{x, nullptr}, 5};
    planes_to_c32<false><<<(M + 255) / 256, 256, 0, (hipStream_t)stream>>>(in, 5, w, nullptr, z, H, W, M);
    return check_launch("dmc_ctxends_first_fwd");
}

int dmc_ctxends_first_dgrad(const float* dz, const float* w, float* dx, int N, int H, int W, dmc_stream_t stream) {
    if (!dz || !w || !dx) return fail(DMC_E_INVALID, "dmc_ctxends_first_dgrad: null pointer");
    if (!index_ok(N, H, W)) return fail(DMC_E_INVALID, "dmc_ctxends_first_dgrad: unsupported shape (N %d, H %d, W %d)", N, H, W);
    const int M = N * H * W;
    PlanesOut out = {{dx, nullptr}, 5};
    c32_to_planes<5, true><<<(M + 127) / 128, 256, 0, (hipStream_t)stream>>>(dz, w, nullptr, out, H, W, M);
    return check_launch("dmc_ctxends_first_dgrad");
}

int dmc_ctxends_first_wgrad(const float* x, const float* dz, float* dw, void* workspace, int N, int H, int W, dmc_stream_t stream) {
    if (!x || !dz || !dw || !workspace) return fail(DMC_E_INVALID, "dmc_ctxends_first_wgrad: null pointer");
    if (!index_ok(N, H, W)) return fail(DMC_E_INVALID, "dmc_ctxends_first_wgrad: unsupported shape (N %d, H %d, W %d)", N, H, W);
    const int M = N * H * W, nr = nranges_of(M);
    hipStream_t s = (hipStream_t)stream;
    float* partial = static_cast<float*>(workspace);
    Planes in = {{x, nullptr}, 5};
    launch_wgrad_partial<5, false>(dz, in, partial, H, W, M, s);
    int rc;
    if ((rc = check_launch("dmc_ctxends_first_wgrad (partial)"))) return rc;
    wgrad_final<<<(5 * 288 + 255) / 256, 256, 0, s>>>(partial, nr, 5, 1, dw, nullptr);
    return check_launch("dmc_ctxends_first_wgrad");
}

int dmc_ctxends_heads_fwd(const float* t, const float* w_flow, const float* w_att, float* z_flow, float* z_att, int N, int H, int W,
                          dmc_stream_t stream) {
    if (!t || !w_flow || !z_flow) return fail(DMC_E_INVALID, "dmc_ctxends_heads_fwd: null pointer");
    if ((w_att == nullptr) != (z_att == nullptr))
        return fail(DMC_E_INVALID, "dmc_ctxends_heads_fwd: the attention head needs w_att and z_att together");
    if (!index_ok(N, H, W)) return fail(DMC_E_INVALID, "dmc_ctxends_heads_fwd: unsupported shape (N %d, H %d, W %d)", N, H, W);
    const int M = N * H * W;
    const dim3 grid((M + 127) / 128);
    hipStream_t s = (hipStream_t)stream;
    PlanesOut out = {{z_flow, z_att}, 2};
    if (w_att) c32_to_planes<4, false><<<grid, 256, 0, s>>>(t, w_flow, w_att, out, H, W, M);
    else c32_to_planes<2, false><<<grid, 256, 0, s>>>(t, w_flow, nullptr, out, H, W, M);
    return check_launch("dmc_ctxends_heads_fwd");
}

int dmc_ctxends_heads_dgrad(const float* dz_flow, const float* dz_att, const float* w_flow, const float* w_att, float* dt, int N,
                            int H, int W, dmc_stream_t stream) {
    if (!w_flow || !dt) return fail(DMC_E_INVALID, "dmc_ctxends_heads_dgrad: null pointer");
    if (dz_att && !w_att) return fail(DMC_E_INVALID, "dmc_ctxends_heads_dgrad: the attention head needs w_att with dz_att");
    if (!dz_flow && !dz_att) return fail(DMC_E_INVALID, "dmc_ctxends_heads_dgrad: null pointer (no head has a gradient)");
    if (!index_ok(N, H, W)) return fail(DMC_E_INVALID, "dmc_ctxends_heads_dgrad: unsupported shape (N %d, H %d, W %d)", N, H, W);
    const int M = N * H * W;
    const dim3 grid((M + 255) / 256);
    hipStream_t s = (hipStream_t)stream;
    if (dz_flow && dz_att) {
        Planes in = {{dz_flow, dz_att}, 2};
        planes_to_c32<true><<<grid, 256, 0, s>>>(in, 4, w_flow, w_att, dt, H, W, M);
    } else {
        Planes in = {{dz_flow ? dz_flow : dz_att, nullptr}, 2};
        planes_to_c32<true><<<grid, 256, 0, s>>>(in, 2, dz_flow ? w_flow : w_att, nullptr, dt, H, W, M);
    }
    return check_launch("dmc_ctxends_heads_dgrad");
}

int dmc_ctxends_heads_wgrad(const float* t, const float* dz_flow, const float* dz_att, float* dw_flow, float* dw_att,
                            void* workspace, int N, int H, int W, dmc_stream_t stream) {
    if (!t || !workspace) return fail(DMC_E_INVALID, "dmc_ctxends_heads_wgrad: null pointer");
    if ((dz_flow == nullptr) != (dw_flow == nullptr) || (dz_att == nullptr) != (dw_att == nullptr))
        return fail(DMC_E_INVALID, "dmc_ctxends_heads_wgrad: a head's dz and dw are given together or not at all");
    if (!dz_flow && !dz_att) return fail(DMC_E_INVALID, "dmc_ctxends_heads_wgrad: null pointer (no head has a gradient)");
    if (!index_ok(N, H, W)) return fail(DMC_E_INVALID, "dmc_ctxends_heads_wgrad: unsupported shape (N %d, H %d, W %d)", N, H, W);
    const int M = N * H * W, nr = nranges_of(M);
    hipStream_t s = (hipStream_t)stream;
    float* partial = static_cast<float*>(workspace);
    int rc;
    if (dz_flow && dz_att) {
        Planes in = {{dz_flow, dz_att}, 2};
        launch_wgrad_partial<4, true>(t, in, partial, H, W, M, s);
        if ((rc = check_launch("dmc_ctxends_heads_wgrad (partial)"))) return rc;
        wgrad_final<<<(4 * 288 + 255) / 256, 256, 0, s>>>(partial, nr, 4, 0, dw_flow, dw_att);
    } else {
        Planes in = {{dz_flow ? dz_flow : dz_att, nullptr}, 2};
        launch_wgrad_partial<2, true>(t, in, partial, H, W, M, s);
        if ((rc = check_launch("dmc_ctxends_heads_wgrad (partial)"))) return rc;
        wgrad_final<<<(2 * 288 + 255) / 256, 256, 0, s>>>(partial, nr, 2, 0, dz_flow ? dw_flow : dw_att, nullptr);
    }
    return check_launch("dmc_ctxends_heads_wgrad");
}

int dmc_ctxends_bn_fwd(const float* z, const float* gamma, const float* beta, float* running_mean, float* running_var, float* y,
                       float* stats, void* scratch_, int N, int H, int W, float slope, float eps, float momentum, int relu,
                       dmc_stream_t stream) {
    if (!z || !gamma || !beta || !y || !stats || !scratch_) return fail(DMC_E_INVALID, "dmc_ctxends_bn_fwd: null pointer");
    if ((running_mean == nullptr) != (running_var == nullptr))
        return fail(DMC_E_INVALID, "dmc_ctxends_bn_fwd: running_mean and running_var are given together or not at all");
    if (!bn_shape_ok(N, H, W)) return fail(DMC_E_INVALID, "dmc_ctxends_bn_fwd: unsupported shape (N %d, H %d, W %d)", N, H, W);
    if (!(eps > 0.f)) return fail(DMC_E_INVALID, "dmc_ctxends_bn_fwd: eps=%g must be positive", (double)eps);
    if (!(slope > 0.f && slope < 1.f)) return fail(DMC_E_INVALID, "dmc_ctxends_bn_fwd: slope=%g is outside (0, 1)", (double)slope);
    if (!(momentum >= 0.f && momentum <= 1.f)) return fail(DMC_E_INVALID, "dmc_ctxends_bn_fwd: momentum=%g is outside [0, 1]", (double)momentum);
    hipStream_t s = (hipStream_t)stream;
    const int M = N * H * W, nb = bn_blocks_of(M);
    BnpArgs a = {z, nullptr, gamma, beta, stats, nullptr, y, 2 * M, H * W, slope, relu ? 0.f : slope, relu ? 1 : 0};
    double* scratch = static_cast<double*>(scratch_);
    int rc;
    bnp_partial_kernel<0><<<nb, 256, 0, s>>>(a, scratch);
    if ((rc = check_launch("dmc_ctxends_bn_fwd (partial)"))) return rc;
    bnp_stats_final_kernel<<<1, 256, 0, s>>>(scratch, stats, running_mean, running_var, M, nb, eps, momentum);
    if ((rc = check_launch("dmc_ctxends_bn_fwd (final)"))) return rc;
    bnp_apply_kernel<0><<<nb, 256, 0, s>>>(a);
    return check_launch("dmc_ctxends_bn_fwd");
}

int dmc_ctxends_bn_bwd(const float* z, const float* dy, const float* gamma, const float* beta, const float* stats, void* scratch_,
                       float* dz, float* dgamma, float* dbeta, int N, int H, int W, float slope, int relu, dmc_stream_t stream) {
    if (!z || !dy || !gamma || !beta || !stats || !scratch_ || !dz || !dgamma || !dbeta)
        return fail(DMC_E_INVALID, "dmc_ctxends_bn_bwd: null pointer");
    if (!bn_shape_ok(N, H, W)) return fail(DMC_E_INVALID, "dmc_ctxends_bn_bwd: unsupported shape (N %d, H %d, W %d)", N, H, W);
    if (!(slope > 0.f && slope < 1.f)) return fail(DMC_E_INVALID, "dmc_ctxends_bn_bwd: slope=%g is outside (0, 1)", (double)slope);
    hipStream_t s = (hipStream_t)stream;
    const int M = N * H * W, nb = bn_blocks_of(M);
    double* scratch = static_cast<double*>(scratch_);
    float* means = reinterpret_cast<float*>(scratch + (size_t)nb * 4);
    BnpArgs a = {z, dy, gamma, beta, stats, means, dz, 2 * M, H * W, slope, relu ? 0.f : slope, relu ? 1 : 0};
    int rc;
    bnp_partial_kernel<1><<<nb, 256, 0, s>>>(a, scratch);
    if ((rc = check_launch("dmc_ctxends_bn_bwd (partial)"))) return rc;
    bnp_bwd_final_kernel<<<1, 256, 0, s>>>(scratch, dgamma, dbeta, means, M, nb);
    if ((rc = check_launch("dmc_ctxends_bn_bwd (final)"))) return rc;
    bnp_apply_kernel<1><<<nb, 256, 0, s>>>(a);
    return check_launch("dmc_ctxends_bn_bwd");
}

}  // extern "C"
