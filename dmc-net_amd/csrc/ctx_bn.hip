// BatchNorm2d (batch statistics) + LeakyReLU for the ContextNetwork units in training (gfx950), forward and backward.
//
// Replaces, in the units Conv2d -> BatchNorm2d -> LeakyReLU(0.1, inplace) of ContextNetwork / ContextNetworkAtt
// (code/dmcnet/model.py:45-104), the two modules behind the convolution: nn.BatchNorm2d in train() (batch statistics, biased
// variance for the normalisation, unbiased for running_var) and the in-place LeakyReLU, and what autograd computes for them.
// Pure HBM streaming: 3 passes over the [M][C] activation forward (statistics read z; apply reads z, writes y) and 5 backward
// (sums read z, dy; apply reads z, dy, writes dz) where the stock modules make 5 and 8.  The backward recomputes
// t = fmaf((z - mean) * invstd, gamma, beta) with the forward's expression (ctx_eval.hip's bn_leaky; the build has
// -ffp-contract=off), so the slope of every element is bit for bit the forward's choice and y is not read.
//
// Layout: z, y, dy, dz are [M][C] fp32 row-major, M = N*H*W (a channels_last tensor's memory), C in {32, 64, 96, 128}.
// A thread owns one float4 column of channels: workgroups have 256 threads (192 for C = 96), a multiple of C / 4, and the grid
// stride is a multiple of the workgroup, so the column of a thread -- and its mean, invstd, gamma, beta -- never changes.
// Every sum is fp64 from the first addition (x^2 and g * xhat are exact as fp64 products of fp32 values): thread sums, the
// workgroup's column sums through LDS, the partials [C][blocks][2] in the caller's scratch, their fixed-order reduction and the
// statistics.  No atomics: bit-identical from run to run.
#include "dmc_common.h"

using namespace dmc;

namespace {

constexpr int MAX_BLOCKS = 2048;      // one resident round of 256-thread workgroups on 256 CUs; the rest is grid stride

struct BnlArgs {
    const float* z;
    const float* dy;
    const float* gamma;
    const float* beta;
    const float* stats;       // mean[C], invstd[C]
    const float* means;       // backward: (sum g) / M [C], (sum g xhat) / M [C]
    float* out;               // y (forward) or dz (backward)
    long total;               // M * C / 4 float4s
    int C;
    float slope;
};

__host__ __device__ constexpr int block_of(int C) { return C == 96 ? 192 : 256; }

int blocks_of(int M, int C) {
    const long total = (long)M * (C / 4), bs = block_of(C);
    const long b = (total + bs - 1) / bs;
    return (int)(b > MAX_BLOCKS ? MAX_BLOCKS : b);
}

bool shape_ok(int M, int C) {
    return (C == 32 || C == 64 || C == 96 || C == 128) && M >= 2 && (long)M * C < (1L << 31);
}

__device__ __forceinline__ float4 ld4(const float* p, long i) { return reinterpret_cast<const float4*>(p)[i]; }

__device__ __forceinline__ float bn_t(float v, float mean, float istd, float gamma, float beta) {
    return fmaf((v - mean) * istd, gamma, beta);
}

// MODE 0: per-channel (sum z, sum z^2).   MODE 1: (sum g, sum g * xhat), g = dy * (t > 0 ? 1 : slope)
template <int MODE>
__global__ __launch_bounds__(256) void bnl_partial_kernel(BnlArgs a, double* __restrict__ scratch) {
    __shared__ double sm[2][256][4];
    const int cq = a.C >> 2, bs = (int)blockDim.x;
    const int tx = (int)threadIdx.x % cq, rows = bs / cq;
    const long stride = (long)gridDim.x * bs;
    double s0[4] = {0.0, 0.0, 0.0, 0.0}, s1[4] = {0.0, 0.0, 0.0, 0.0};
    float4 mean, istd, gam, bet;
    if (MODE == 1) {
        mean = ld4(a.stats, tx); istd = ld4(a.stats + a.C, tx); gam = ld4(a.gamma, tx); bet = ld4(a.beta, tx);
    }
    auto add = [&](const float4 x, const float4 d) {
        const float xv[4] = {x.x, x.y, x.z, x.w};
        if (MODE == 0) {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const double v = (double)xv[e];
                s0[e] += v;
                s1[e] = fma(v, v, s1[e]);
            }
        } else {
            const float dv[4] = {d.x, d.y, d.z, d.w}, mv[4] = {mean.x, mean.y, mean.z, mean.w}, iv[4] = {istd.x, istd.y, istd.z, istd.w};
            const float gv[4] = {gam.x, gam.y, gam.z, gam.w}, bv[4] = {bet.x, bet.y, bet.z, bet.w};
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float xh = (xv[e] - mv[e]) * iv[e];
                const float t = fmaf(xh, gv[e], bv[e]);
                const float g = t > 0.f ? dv[e] : dv[e] * a.slope;
                s0[e] += (double)g;
                s1[e] = fma((double)g, (double)xh, s1[e]);
            }
        }
    };
    long o = (long)blockIdx.x * bs + threadIdx.x;
    const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
    for (; o + 3 * stride < a.total; o += 4 * stride) {          // four independent 16-byte loads (eight in the backward) in flight
        float4 x[4], d[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            x[k] = ld4(a.z, o + k * stride);
            d[k] = MODE == 1 ? ld4(a.dy, o + k * stride) : zero;
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) add(x[k], d[k]);
    }
    for (; o < a.total; o += stride) add(ld4(a.z, o), MODE == 1 ? ld4(a.dy, o) : zero);
#pragma unroll
    for (int e = 0; e < 4; ++e) { sm[0][threadIdx.x][e] = s0[e]; sm[1][threadIdx.x][e] = s1[e]; }
    __syncthreads();
    // fixed-order column sums over the `rows` thread rows; scratch is [channel][block][2]
    for (int i = threadIdx.x; i < cq * 8; i += bs) {
        const int col = i >> 3, which = (i >> 2) & 1, e = i & 3;
        double acc = 0.0;
        for (int t = 0; t < rows; ++t) acc += sm[which][t * cq + col][e];
        scratch[((size_t)(col * 4 + e) * gridDim.x + blockIdx.x) * 2 + which] = acc;
    }
}

// One workgroup per channel: thread i adds partials i, i + 256, ... in order, then a fixed tree over the 256 threads.
__device__ __forceinline__ void reduce_channel(const double* __restrict__ scratch, int nblocks, double& s, double& ss) {
    __shared__ double red[2][4];
    const double2* row = reinterpret_cast<const double2*>(scratch) + (size_t)blockIdx.x * nblocks;
    double2 v[MAX_BLOCKS / 256];
#pragma unroll
    for (int k = 0; k < MAX_BLOCKS / 256; ++k) {
        const int sp = (int)threadIdx.x + 256 * k;
        v[k] = sp < nblocks ? row[sp] : make_double2(0.0, 0.0);
    }
    s = 0.0; ss = 0.0;
#pragma unroll
    for (int k = 0; k < MAX_BLOCKS / 256; ++k) { s += v[k].x; ss += v[k].y; }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { s += __shfl_down(s, o, 64); ss += __shfl_down(ss, o, 64); }
    if ((threadIdx.x & 63) == 0) { red[0][threadIdx.x >> 6] = s; red[1][threadIdx.x >> 6] = ss; }
    __syncthreads();
    s = red[0][0] + red[0][1] + red[0][2] + red[0][3];
    ss = red[1][0] + red[1][1] + red[1][2] + red[1][3];
}

__global__ __launch_bounds__(256) void bnl_stats_final_kernel(const double* __restrict__ scratch, float* __restrict__ stats,
                                                              float* __restrict__ running_mean, float* __restrict__ running_var,
                                                              int C, int M, int nblocks, float eps, float momentum) {
    double s, ss;
    reduce_channel(scratch, nblocks, s, ss);
    if (threadIdx.x != 0) return;
    const int c = blockIdx.x;
    const double mean = s / (double)M;
    double var = ss / (double)M - mean * mean;
    if (var < 0.0) var = 0.0;
    stats[c] = (float)mean;
    stats[C + c] = (float)(1.0 / sqrt(var + (double)eps));
    if (running_mean) {
        const double m = (double)momentum, unbiased = var * (double)M / (double)(M - 1);
        running_mean[c] = (float)((1.0 - m) * (double)running_mean[c] + m * mean);
        running_var[c] = (float)((1.0 - m) * (double)running_var[c] + m * unbiased);
    }
}

// dbeta = sum g, dgamma = sum g xhat; their means go behind the partials for the second pass
__global__ __launch_bounds__(256) void bnl_bwd_final_kernel(const double* __restrict__ scratch, float* __restrict__ dgamma,
                                                            float* __restrict__ dbeta, float* __restrict__ means, int C, int M,
                                                            int nblocks) {
    double s, ss;
    reduce_channel(scratch, nblocks, s, ss);
    if (threadIdx.x != 0) return;
    const int c = blockIdx.x;
    dbeta[c] = (float)s;
    dgamma[c] = (float)ss;
    means[c] = (float)(s / (double)M);
    means[C + c] = (float)(ss / (double)M);
}

// BWD 0: y = t > 0 ? t : slope t.   BWD 1: dz = gamma invstd (g - mean(g) - xhat mean(g xhat))
template <int BWD>
__global__ __launch_bounds__(256) void bnl_apply_kernel(BnlArgs a) {
    const int cq = a.C >> 2, bs = (int)blockDim.x;
    const int tx = (int)threadIdx.x % cq;
    const long stride = (long)gridDim.x * bs;
    const float4 mean = ld4(a.stats, tx), istd = ld4(a.stats + a.C, tx), gam = ld4(a.gamma, tx), bet = ld4(a.beta, tx);
    float4 mb = make_float4(0.f, 0.f, 0.f, 0.f), mg = mb;
    if (BWD) { mb = ld4(a.means, tx); mg = ld4(a.means + a.C, tx); }
    const float mv[4] = {mean.x, mean.y, mean.z, mean.w}, iv[4] = {istd.x, istd.y, istd.z, istd.w};
    const float gv[4] = {gam.x, gam.y, gam.z, gam.w}, bv[4] = {bet.x, bet.y, bet.z, bet.w};
    const float mbv[4] = {mb.x, mb.y, mb.z, mb.w}, mgv[4] = {mg.x, mg.y, mg.z, mg.w};
    auto apply = [&](const float4 x, const float4 d) -> float4 {
        const float xv[4] = {x.x, x.y, x.z, x.w}, dv[4] = {d.x, d.y, d.z, d.w};
        float r[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const float xh = (xv[e] - mv[e]) * iv[e];
            const float t = fmaf(xh, gv[e], bv[e]);
            if (BWD) {
                const float g = t > 0.f ? dv[e] : dv[e] * a.slope;
                r[e] = gv[e] * iv[e] * (g - mbv[e] - xh * mgv[e]);
            } else {
                r[e] = t > 0.f ? t : a.slope * t;
            }
        }
        return make_float4(r[0], r[1], r[2], r[3]);
    };
    float4* out = reinterpret_cast<float4*>(a.out);
    const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
    long o = (long)blockIdx.x * bs + threadIdx.x;
    for (; o + 3 * stride < a.total; o += 4 * stride) {
        float4 x[4], d[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            x[k] = ld4(a.z, o + k * stride);
            d[k] = BWD ? ld4(a.dy, o + k * stride) : zero;
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) out[o + k * stride] = apply(x[k], d[k]);
    }
    for (; o < a.total; o += stride) out[o] = apply(ld4(a.z, o), BWD ? ld4(a.dy, o) : zero);
}

}  // namespace

extern "C" {

int dmc_bnlrelu_supported(int M, int C) { return shape_ok(M, C) ? 1 : 0; }

// partials [C][blocks][2] fp64, then the backward's two means [2][C] fp32 (the forward does not touch those)
size_t dmc_bnlrelu_scratch_bytes(int M, int C) {
    if (!shape_ok(M, C)) return 0;
    return (size_t)blocks_of(M, C) * C * 2 * sizeof(double) + (size_t)2 * C * sizeof(float);
}

int dmc_bnlrelu_fwd(const float* z, const float* gamma, const float* beta, float* running_mean, float* running_var, float* y,
                    float* stats, void* scratch_, int M, int C, float slope, float eps, float momentum, dmc_stream_t stream) {
    if (!z || !gamma || !beta || !y || !stats || !scratch_) return fail(DMC_E_INVALID, "dmc_bnlrelu_fwd: null pointer");
    if ((running_mean == nullptr) != (running_var == nullptr))
        return fail(DMC_E_INVALID, "dmc_bnlrelu_fwd: running_mean and running_var are given together or not at all");
    if (!shape_ok(M, C)) return fail(DMC_E_INVALID, "dmc_bnlrelu_fwd: unsupported shape M=%d C=%d", M, C);
    if (!(eps > 0.f)) return fail(DMC_E_INVALID, "dmc_bnlrelu_fwd: eps=%g must be positive", (double)eps);
    if (!(slope > 0.f && slope < 1.f)) return fail(DMC_E_INVALID, "dmc_bnlrelu_fwd: slope=%g is outside (0, 1)", (double)slope);
    if (!(momentum >= 0.f && momentum <= 1.f)) return fail(DMC_E_INVALID, "dmc_bnlrelu_fwd: momentum=%g is outside [0, 1]", (double)momentum);
    hipStream_t s = (hipStream_t)stream;
    const int nb = blocks_of(M, C), bs = block_of(C);
    BnlArgs a = {z, nullptr, gamma, beta, stats, nullptr, y, (long)M * (C / 4), C, slope};
    double* scratch = static_cast<double*>(scratch_);
    int rc;
    bnl_partial_kernel<0><<<nb, bs, 0, s>>>(a, scratch);
    if ((rc = check_launch("bnl_partial"))) return rc;
    bnl_stats_final_kernel<<<C, 256, 0, s>>>(scratch, stats, running_mean, running_var, C, M, nb, eps, momentum);
    if ((rc = check_launch("bnl_stats_final"))) return rc;
    bnl_apply_kernel<0><<<nb, bs, 0, s>>>(a);
    return check_launch("bnl_apply_fwd");
}

int dmc_bnlrelu_bwd(const float* z, const float* dy, const float* gamma, const float* beta, const float* stats, void* scratch_,
                    float* dz, float* dgamma, float* dbeta, int M, int C, float slope, dmc_stream_t stream) {
    if (!z || !dy || !gamma || !beta || !stats || !scratch_ || !dz || !dgamma || !dbeta)
        return fail(DMC_E_INVALID, "dmc_bnlrelu_bwd: null pointer");
    if (!shape_ok(M, C)) return fail(DMC_E_INVALID, "dmc_bnlrelu_bwd: unsupported shape M=%d C=%d", M, C);
    if (!(slope > 0.f && slope < 1.f)) return fail(DMC_E_INVALID, "dmc_bnlrelu_bwd: slope=%g is outside (0, 1)", (double)slope);
    hipStream_t s = (hipStream_t)stream;
    const int nb = blocks_of(M, C), bs = block_of(C);
    double* scratch = static_cast<double*>(scratch_);
    float* means = reinterpret_cast<float*>(scratch + (size_t)nb * C * 2);
    BnlArgs a = {z, dy, gamma, beta, stats, means, dz, (long)M * (C / 4), C, slope};
    int rc;
    bnl_partial_kernel<1><<<nb, bs, 0, s>>>(a, scratch);
    if ((rc = check_launch("bnl_bwd_partial"))) return rc;
    bnl_bwd_final_kernel<<<C, 256, 0, s>>>(scratch, dgamma, dbeta, means, C, M, nb);
    if ((rc = check_launch("bnl_bwd_final"))) return rc;
    bnl_apply_kernel<1><<<nb, bs, 0, s>>>(a);
    return check_launch("bnl_apply_bwd");
}

}  // extern "C"
