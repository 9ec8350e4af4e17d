// Discriminator4's middle block: Conv2d(8, 16, 3, stride 2, padding 1) on NHWC activations, code/dmcnet_GAN/model.py:254-265 as
// instantiated at :369-385 (`discriminator_block(8, 16)` between the 2 -> 8 block of disc_first.hip and the 16 -> 32 block of
// conv_nhwc.hip), with the epilogue contract of dmc_conv_nhwc_fwd: + bias, LeakyReLU(0.2), Dropout2d keep mask, fp64 BatchNorm
// statistic partials per workgroup.
//
// 72 multiply-adds per output value, 3.6 M per 112 x 112 frame, 8 input channels: below what dmc_conv_nhwc_supported accepts (multiples
// of 16) and too thin for the matrix cores, so these are direct fp32 fmaf kernels in a fixed order (exact fp32, as early_fusion.hip
// decided for Cout <= 8).
//   forward   x [N,H,W,8] -> z [N,OH,OW,16]: a thread = (output pixel, channel quad); the 1152 weights sit transposed in LDS
//             ([tap][ci][co]: one 16-byte read serves 4 FMAs, the same address in 16 lanes of a wave), the four lanes of a pixel
//             share its 18 16-byte input reads and store 64 consecutive bytes.  A workgroup owns 256 consecutive output pixels; its
//             per-channel (sum, sum of squares) go through LDS in slot order.
//   dgrad     g [N,OH,OW,16] -> dx [N,H,W,8]: a thread = one 2 x 2 group of input pixels, whose taps are static (even row: ky = 1;
//             odd row: ky = 0 from the next output row and ky = 2 from this one; columns alike): it reads the four output pixels
//             (a .. a + 1, b .. b + 1) once and the weights through the scalar cache.
//   wgrad     dw [16,3,3,8], db [16]: a workgroup owns a run of 512 consecutive output pixels; thread j < 72 = (tap, ci) keeps
//             its 16 sums (one per co) in registers, g of the pixel is wave-uniform (scalar cache), 16 more threads sum db.  The
//             runs' partial sums [run][1168] are added in run order by the final kernel: deterministic, no atomics.
#include "dmc_common.h"

using namespace dmc;

namespace {

constexpr int C8_CI = 8, C8_CO = 16, C8_K = 72;                      // K = 9 taps x 8 input channels
constexpr int C8_FWD_PIX = 256;                                      // output pixels per forward workgroup (4 passes of 64)
constexpr int C8_RUN = 512;                                          // output pixels per weight-gradient partial
constexpr int C8_NOUT = C8_CO * C8_K + C8_CO;                        // 1152 dw + 16 db
constexpr long C8_MAX_BYTES = 1L << 31;

__global__ __launch_bounds__(256) void disc_c8_fwd_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                          const float* __restrict__ bias, const float* __restrict__ keep,
                                                          float* __restrict__ z, double* __restrict__ part, long total, int H,
                                                          int W, int OH, int OW, int act) {
    __shared__ __attribute__((aligned(16))) float wl[C8_K * C8_CO];          // [tap * 8 + ci][co]
    __shared__ double red[64][C8_CO][2];
    const int tid = threadIdx.x;
    for (int i = tid; i < C8_CO * C8_K; i += 256) {
        const int co = i / C8_K, k = i - co * C8_K;                          // w is OHWI: [co][tap][ci]
        wl[k * C8_CO + co] = w[i];
    }
    const int c4 = tid & 3, slot = tid >> 2;
    float br[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) br[e] = bias ? bias[4 * c4 + e] : 0.f;
    __syncthreads();
    double s[4] = {0.0, 0.0, 0.0, 0.0}, q[4] = {0.0, 0.0, 0.0, 0.0};
    const long p0 = (long)blockIdx.x * C8_FWD_PIX;
    for (int it = 0; it < C8_FWD_PIX / 64; ++it) {
        const long p = p0 + it * 64 + slot;
        if (p >= total) break;
        const int n = (int)(p / ((long)OH * OW));
        const int rem = (int)(p - (long)n * OH * OW);
        const int oy = rem / OW, ox = rem - oy * OW;
        float acc[4] = {br[0], br[1], br[2], br[3]};
#pragma unroll
        for (int ky = 0; ky < 3; ++ky) {
            const int iy = 2 * oy + ky - 1;
            if (iy < 0 || iy >= H) continue;
#pragma unroll
            for (int kx = 0; kx < 3; ++kx) {
                const int ix = 2 * ox + kx - 1;
                if (ix < 0 || ix >= W) continue;
                const float4* xp = reinterpret_cast<const float4*>(x + (((long)n * H + iy) * W + ix) * C8_CI);
                const float4 xa = xp[0], xb = xp[1];
                const float xv[8] = {xa.x, xa.y, xa.z, xa.w, xb.x, xb.y, xb.z, xb.w};
#pragma unroll
                for (int ci = 0; ci < C8_CI; ++ci) {
                    const float4 wv = *reinterpret_cast<const float4*>(wl + ((ky * 3 + kx) * C8_CI + ci) * C8_CO + 4 * c4);
                    acc[0] = fmaf(xv[ci], wv.x, acc[0]);
                    acc[1] = fmaf(xv[ci], wv.y, acc[1]);
                    acc[2] = fmaf(xv[ci], wv.z, acc[2]);
                    acc[3] = fmaf(xv[ci], wv.w, acc[3]);
                }
            }
        }
        float o[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            float t = acc[e];
            if (act) t = t > 0.f ? t : 0.2f * t;
            if (keep) t *= keep[(long)n * C8_CO + 4 * c4 + e];
            o[e] = t;
            if (part) {
                s[e] += (double)t;
                q[e] += (double)t * (double)t;
            }
        }
        *reinterpret_cast<float4*>(z + p * C8_CO + 4 * c4) = make_float4(o[0], o[1], o[2], o[3]);
    }
    if (!part) return;                                                       // (uniform)
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        red[slot][4 * c4 + e][0] = s[e];
        red[slot][4 * c4 + e][1] = q[e];
    }
    __syncthreads();
    if (tid < 2 * C8_CO) {
        const int c = tid >> 1, which = tid & 1;
        double t = 0.0;
        for (int sl = 0; sl < 64; ++sl) t += red[sl][c][which];              // slot order: fixed
        part[((size_t)blockIdx.x * C8_CO + c) * 2 + which] = t;
    }
}

__global__ __launch_bounds__(256) void disc_c8_dgrad_kernel(const float* __restrict__ g, const float* __restrict__ w,
                                                            float* __restrict__ dx, long total, int H, int W, int OH, int OW) {
    // one group per thread, no grid-stride loop: around a loop the compiler keeps all 1152 weights in scalar registers and spills them
    const long t = (long)blockIdx.x * 256 + threadIdx.x;
    if (t < total) {
        const int n = (int)(t / ((long)OH * OW));
        const int rem = (int)(t - (long)n * OH * OW);
        const int a = rem / OW, b = rem - a * OW;
        float gv[2][2][C8_CO];
#pragma unroll
        for (int dy = 0; dy < 2; ++dy)
#pragma unroll
            for (int dc = 0; dc < 2; ++dc) {
                const bool ok = a + dy < OH && b + dc < OW;
                const float4* gp = reinterpret_cast<const float4*>(g + (((long)n * OH + (ok ? a + dy : a)) * OW + (ok ? b + dc : b)) * C8_CO);
#pragma unroll
                for (int c4 = 0; c4 < 4; ++c4) {
                    const float4 v = ok ? gp[c4] : make_float4(0.f, 0.f, 0.f, 0.f);
                    gv[dy][dc][4 * c4] = v.x; gv[dy][dc][4 * c4 + 1] = v.y; gv[dy][dc][4 * c4 + 2] = v.z; gv[dy][dc][4 * c4 + 3] = v.w;
                }
            }
#pragma unroll
        for (int py = 0; py < 2; ++py)
#pragma unroll
            for (int px = 0; px < 2; ++px) {
                float acc[C8_CI] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
                // input row 2 a + py = 2 oy + ky - 1: py 0 -> (ky 1, oy a); py 1 -> (ky 0, oy a + 1), (ky 2, oy a)
#pragma unroll
                for (int ty = 0; ty < (py ? 2 : 1); ++ty) {
                    const int ky = py ? 2 * ty : 1, dy = py ? 1 - ty : 0;
#pragma unroll
                    for (int tx = 0; tx < (px ? 2 : 1); ++tx) {
                        const int kx = px ? 2 * tx : 1, dc = px ? 1 - tx : 0;
#pragma unroll
                        for (int co = 0; co < C8_CO; ++co)
#pragma unroll
                            for (int ci = 0; ci < C8_CI; ++ci)
                                acc[ci] = fmaf(gv[dy][dc][co], w[(co * 9 + ky * 3 + kx) * C8_CI + ci], acc[ci]);
                    }
                }
                const int iy = 2 * a + py, ix = 2 * b + px;
                if (iy < H && ix < W) {
                    float4* dst = reinterpret_cast<float4*>(dx + (((long)n * H + iy) * W + ix) * C8_CI);
                    dst[0] = make_float4(acc[0], acc[1], acc[2], acc[3]);
                    dst[1] = make_float4(acc[4], acc[5], acc[6], acc[7]);
                }
            }
    }
}

__global__ __launch_bounds__(128) void disc_c8_wgrad_kernel(const float* __restrict__ x, const float* __restrict__ g,
                                                            float* __restrict__ part, long total, int H, int W, int OH, int OW) {
    const int tid = threadIdx.x;
    const bool isw = tid < C8_K, isb = tid >= C8_K && tid < C8_K + C8_CO;
    const int tap = (isw ? tid : 0) >> 3, ci = tid & 7, ky = tap / 3, kx = tap - 3 * ky;
    const long p0 = (long)blockIdx.x * C8_RUN;
    long p1 = p0 + C8_RUN;
    if (p1 > total) p1 = total;
    // the run's pixel coordinates are the same in every lane and advance without divisions
    int n = (int)(p0 / ((long)OH * OW));
    const int rem = (int)(p0 - (long)n * OH * OW);
    int oy = rem / OW, ox = rem - oy * OW;
    float acc[C8_CO];
#pragma unroll
    for (int co = 0; co < C8_CO; ++co) acc[co] = 0.f;
    float dbacc = 0.f;
#pragma unroll 4
    for (long p = p0; p < p1; ++p) {
        float xv = 0.f;
        const int iy = 2 * oy + ky - 1, ix = 2 * ox + kx - 1;
        if (isw && iy >= 0 && iy < H && ix >= 0 && ix < W) xv = x[(((long)n * H + iy) * W + ix) * C8_CI + ci];
        const float* gp = g + p * C8_CO;
#pragma unroll
        for (int co = 0; co < C8_CO; ++co) acc[co] = fmaf(gp[co], xv, acc[co]);
        if (isb) dbacc += gp[tid - C8_K];
        if (++ox == OW) {
            ox = 0;
            if (++oy == OH) { oy = 0; ++n; }
        }
    }
    float* out = part + (size_t)blockIdx.x * C8_NOUT;
    if (isw) {
#pragma unroll
        for (int co = 0; co < C8_CO; ++co) out[co * C8_K + tid] = acc[co];   // OHWI: [co][tap][ci]
    }
    if (isb) out[C8_CO * C8_K + tid - C8_K] = dbacc;
}

__global__ __launch_bounds__(256) void disc_c8_wgrad_final_kernel(const float* __restrict__ part, int nruns, float* __restrict__ dw,
                                                                  float* __restrict__ db) {
    // 16 outputs per workgroup, 16 lanes of run slices each: slice s adds runs s, s + 16, ... in order, then the slices in order
    __shared__ double red[16][16];
    const int ol = threadIdx.x & 15, sl = threadIdx.x >> 4;
    const int o = blockIdx.x * 16 + ol;                                      // < C8_NOUT = 73 * 16
    double t = 0.0;
    for (int r = sl; r < nruns; r += 16) t += (double)part[(size_t)r * C8_NOUT + o];
    red[sl][ol] = t;
    __syncthreads();
    if (threadIdx.x >= 16) return;
    double v = 0.0;
#pragma unroll
    for (int k = 0; k < 16; ++k) v += red[k][ol];
    if (o < C8_CO * C8_K) dw[o] = (float)v;
    else if (db) db[o - C8_CO * C8_K] = (float)v;
}

long c8_pixels(int N, int H, int W) { return (long)N * ((H - 1) / 2 + 1) * ((W - 1) / 2 + 1); }

}  // namespace

extern "C" {

int dmc_disc_c8_supported(int N, int H, int W) {
    if (N <= 0 || H <= 0 || W <= 0 || (H & 1) || (W & 1)) return 0;
    // x is the largest tensor (32 bytes per input pixel against 16 of z per input pixel); the weight-gradient partials stay below it
    long e = (long)N * H;                                                    // every factor < 2^31: each running product fits 64 bits
    if (e >= C8_MAX_BYTES) return 0;
    e *= W;
    if (e >= C8_MAX_BYTES / (C8_CI * (long)sizeof(float))) return 0;
    if (c8_pixels(N, H, W) * C8_CO * (long)sizeof(float) >= C8_MAX_BYTES) return 0;
    return 1;
}

int dmc_disc_c8_stat_blocks(int N, int H, int W) {
    if (!dmc_disc_c8_supported(N, H, W)) return 0;
    return (int)((c8_pixels(N, H, W) + C8_FWD_PIX - 1) / C8_FWD_PIX);
}

int dmc_disc_c8_fwd(const float* x, const float* w, const float* bias, const float* keep, float* z, double* stat_partials,
                    int stat_blocks, int N, int H, int W, int act, dmc_stream_t stream) {
    if (!x || !w || !z) return fail(DMC_E_INVALID, "dmc_disc_c8_fwd: null pointer");
    if (!dmc_disc_c8_supported(N, H, W)) return fail(DMC_E_INVALID, "dmc_disc_c8_fwd: unsupported shape N=%d H=%d W=%d", N, H, W);
    const int nb = dmc_disc_c8_stat_blocks(N, H, W);
    if (stat_partials && stat_blocks != nb)
        return fail(DMC_E_INVALID, "dmc_disc_c8_fwd: statistics partials have %d rows but this launch writes %d (dmc_disc_c8_stat_blocks)",
                    stat_blocks, nb);
    disc_c8_fwd_kernel<<<nb, 256, 0, (hipStream_t)stream>>>(x, w, bias, keep, z, stat_partials, c8_pixels(N, H, W), H, W, (H - 1) / 2 + 1,
                                                            (W - 1) / 2 + 1, act);
    return check_launch("disc_c8_fwd");
}

int dmc_disc_c8_dgrad(const float* g, const float* w, float* dx, int N, int H, int W, dmc_stream_t stream) {
    if (!g || !w || !dx) return fail(DMC_E_INVALID, "dmc_disc_c8_dgrad: null pointer");
    if (!dmc_disc_c8_supported(N, H, W)) return fail(DMC_E_INVALID, "dmc_disc_c8_dgrad: unsupported shape N=%d H=%d W=%d", N, H, W);
    const long groups = c8_pixels(N, H, W);                                  // one 2 x 2 input group per output pixel
    disc_c8_dgrad_kernel<<<(unsigned)((groups + 255) / 256), 256, 0, (hipStream_t)stream>>>(g, w, dx, groups, H, W, (H - 1) / 2 + 1,
                                                                                            (W - 1) / 2 + 1);
    return check_launch("disc_c8_dgrad");
}

size_t dmc_disc_c8_wgrad_bytes(int N, int H, int W) {
    if (!dmc_disc_c8_supported(N, H, W)) return 0;
    return (size_t)((c8_pixels(N, H, W) + C8_RUN - 1) / C8_RUN) * C8_NOUT * sizeof(float);
}

int dmc_disc_c8_wgrad(const float* x, const float* g, float* dw, float* db, void* workspace, int N, int H, int W,
                      dmc_stream_t stream) {
    if (!x || !g || !dw || !workspace) return fail(DMC_E_INVALID, "dmc_disc_c8_wgrad: null pointer");
    if (!dmc_disc_c8_supported(N, H, W)) return fail(DMC_E_INVALID, "dmc_disc_c8_wgrad: unsupported shape N=%d H=%d W=%d", N, H, W);
    const long total = c8_pixels(N, H, W);
    const int nruns = (int)((total + C8_RUN - 1) / C8_RUN);
    float* part = static_cast<float*>(workspace);
    hipStream_t s = (hipStream_t)stream;
    disc_c8_wgrad_kernel<<<nruns, 128, 0, s>>>(x, g, part, total, H, W, (H - 1) / 2 + 1, (W - 1) / 2 + 1);
    int rc = check_launch("disc_c8_wgrad");
    if (rc) return rc;
    disc_c8_wgrad_final_kernel<<<C8_NOUT / 16, 256, 0, s>>>(part, nruns, dw, db);
    return check_launch("disc_c8_wgrad_final");
}

}  // extern "C"
