// The discriminators' head: adv_layer = Linear(C * H * W -> 2) on the flattened last activation, code/dmcnet_GAN/model.py:290,297-298
// (`self.adv_layer = nn.Sequential(nn.Linear(128 * ds_size ** 2, 2))`, `out.view(out.shape[0], -1)`), read from the NHWC
// (channels_last) activation the blocks leave: x [M][H][W][C].  The weight [2][C * H * W] and the bias [2] stay in the reference's
// (c, h, w) column order; no permuted copy of either is made.
//
// Nothing here is compute: the forward is one streaming read of x, the backward one read and / or one write.
//   forward   one workgroup of 512 threads per frame, ONE launch.  A wave walks (16 pixels x 16 channels) tiles: lane (pixel l >> 2,
//             channel quad l & 3) reads 16 bytes of x (four lanes 64 consecutive bytes) and its eight weights w[j][(c + e) HW + hw]
//             -- for a fixed e the 16 pixels of the tile are 64 consecutive bytes of the L2-resident weight -- and keeps two fp32
//             fmaf sums.  Lanes, then waves, are added in a fixed order; the bias is added last.
//   backward  a thread owns four consecutive NHWC features and a slice of 16 frames: it gathers its eight weights once (dx only),
//             then walks the frames: reads x (dweight only) and / or writes dx = dv0 w0 + dv1 w1; dv is wave-uniform.  The slices'
//             dweight partials [slice][2][F] (NHWC order) are added in slice order and transposed into the weight's layout by the
//             final kernel, which also sums dbias over the frames in a fixed order.  No atomics; a dx-only call reads neither x
//             nor the workspace.
#include "dmc_common.h"

using namespace dmc;

namespace {

constexpr int HD_FRAMES = 16;                    // frames per backward slice
constexpr long HD_MAX_ELEMS = 1L << 31;

__global__ __launch_bounds__(512) void disc_head_fwd_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                            const float* __restrict__ bias, float* __restrict__ out, int C, int HW) {
    __shared__ float red[8][2];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int hl = lane >> 2, cq = lane & 3;
    const size_t F = (size_t)C * HW;
    const float* xm = x + (size_t)blockIdx.x * F;
    const int ctiles = C / 16, ntiles = ctiles * ((HW + 15) / 16);
    float a0 = 0.f, a1 = 0.f;
    for (int t = wave; t < ntiles; t += 8) {
        const int ht = t / ctiles, ct = t - ht * ctiles;                     // channel tiles first: neighbouring waves share x's lines
        const int hw = ht * 16 + hl, c = ct * 16 + 4 * cq;
        if (hw >= HW) continue;
        const float4 xv = *reinterpret_cast<const float4*>(xm + (size_t)hw * C + c);
        const float* w0 = w + (size_t)c * HW + hw;
        const float* w1 = w0 + F;
        a0 = fmaf(xv.x, w0[0], a0);
        a1 = fmaf(xv.x, w1[0], a1);
        a0 = fmaf(xv.y, w0[HW], a0);
        a1 = fmaf(xv.y, w1[HW], a1);
        a0 = fmaf(xv.z, w0[2 * (size_t)HW], a0);
        a1 = fmaf(xv.z, w1[2 * (size_t)HW], a1);
        a0 = fmaf(xv.w, w0[3 * (size_t)HW], a0);
        a1 = fmaf(xv.w, w1[3 * (size_t)HW], a1);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        a0 += __shfl_down(a0, o, 64);
        a1 += __shfl_down(a1, o, 64);
    }
    if (lane == 0) { red[wave][0] = a0; red[wave][1] = a1; }
    __syncthreads();
    if (threadIdx.x < 2) {
        float v = red[0][threadIdx.x];
#pragma unroll
        for (int k = 1; k < 8; ++k) v += red[k][threadIdx.x];
        out[(size_t)blockIdx.x * 2 + threadIdx.x] = bias[threadIdx.x] + v;
    }
}

template <bool DX, bool DW>
__global__ __launch_bounds__(256) void disc_head_bwd_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                            const float* __restrict__ dv, float* __restrict__ dx,
                                                            float* __restrict__ part, int M, int C, int HW, int nb) {
    const size_t F = (size_t)C * HW;
    const int slice = blockIdx.x / nb, b = blockIdx.x - slice * nb;
    const size_t f = 4 * ((size_t)b * 256 + threadIdx.x);                    // four consecutive channels of one pixel (C % 4 == 0)
    if (f >= F) return;
    const int m0 = slice * HD_FRAMES, m1 = m0 + HD_FRAMES < M ? m0 + HD_FRAMES : M;
    float w0[4] = {0.f, 0.f, 0.f, 0.f}, w1[4] = {0.f, 0.f, 0.f, 0.f};
    if (DX) {
        const int hw = (int)(f / C), c = (int)(f - (size_t)hw * C);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            w0[e] = w[(size_t)(c + e) * HW + hw];
            w1[e] = w[F + (size_t)(c + e) * HW + hw];
        }
    }
    float a0[4] = {0.f, 0.f, 0.f, 0.f}, a1[4] = {0.f, 0.f, 0.f, 0.f};
    for (int m = m0; m < m1; ++m) {
        const float d0 = dv[2 * m], d1 = dv[2 * m + 1];
        if (DW) {
            const float4 v = *reinterpret_cast<const float4*>(x + (size_t)m * F + f);
            const float xv[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                a0[e] = fmaf(d0, xv[e], a0[e]);
                a1[e] = fmaf(d1, xv[e], a1[e]);
            }
        }
        if (DX) {
            float o[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) o[e] = fmaf(d1, w1[e], d0 * w0[e]);
            *reinterpret_cast<float4*>(dx + (size_t)m * F + f) = make_float4(o[0], o[1], o[2], o[3]);
        }
    }
    if (DW) {
        *reinterpret_cast<float4*>(part + ((size_t)slice * 2 + 0) * F + f) = make_float4(a0[0], a0[1], a0[2], a0[3]);
        *reinterpret_cast<float4*>(part + ((size_t)slice * 2 + 1) * F + f) = make_float4(a1[0], a1[1], a1[2], a1[3]);
    }
}

// blocks [0, nbw): dweight[j][c HW + hw] = the slices' partials [s][j][hw C + c] in slice order; block nbw (present when dbias is
// wanted): dbias[j] = sum over the frames, 64 lanes striding, then a fixed tree
__global__ __launch_bounds__(256) void disc_head_bwd_final_kernel(const float* __restrict__ part, int nslices,
                                                                  float* __restrict__ dweight, const float* __restrict__ dv,
                                                                  float* __restrict__ dbias, int M, int C, int HW, int nbw) {
    const size_t F = (size_t)C * HW;
    if ((int)blockIdx.x < nbw) {
        const size_t o = (size_t)blockIdx.x * 256 + threadIdx.x;
        if (o >= 2 * F) return;
        const int j = o >= F ? 1 : 0;
        const size_t r = o - (size_t)j * F;
        const int c = (int)(r / HW), hw = (int)(r - (size_t)c * HW);
        const size_t fn = (size_t)hw * C + c;
        float t = 0.f;
        for (int s = 0; s < nslices; ++s) t += part[((size_t)s * 2 + j) * F + fn];
        dweight[o] = t;
        return;
    }
    if (threadIdx.x >= 128) return;
    const int j = threadIdx.x >> 6, lane = threadIdx.x & 63;
    float t = 0.f;
    for (int m = lane; m < M; m += 64) t += dv[2 * m + j];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) t += __shfl_down(t, o, 64);
    if (lane == 0) dbias[j] = t;
}

int head_slices(int M) { return (M + HD_FRAMES - 1) / HD_FRAMES; }

}  // namespace

extern "C" {

int dmc_disc_head_supported(int M, int C, int H, int W) {
    if (M <= 0 || C <= 0 || H <= 0 || W <= 0 || (C & 15)) return 0;
    long e = (long)C * H;                                                    // every factor < 2^31: each running product fits 64 bits
    if (e >= HD_MAX_ELEMS) return 0;
    e *= W;
    if (e >= HD_MAX_ELEMS) return 0;
    e *= M;
    return e < HD_MAX_ELEMS ? 1 : 0;
}

int dmc_disc_head_fwd(const float* x, const float* weight, const float* bias, float* validity, int M, int C, int H, int W,
                      dmc_stream_t stream) {
    if (!x || !weight || !bias || !validity) return fail(DMC_E_INVALID, "dmc_disc_head_fwd: null pointer");
    if (!dmc_disc_head_supported(M, C, H, W))
        return fail(DMC_E_INVALID, "dmc_disc_head_fwd: unsupported shape M=%d C=%d H=%d W=%d", M, C, H, W);
    disc_head_fwd_kernel<<<M, 512, 0, (hipStream_t)stream>>>(x, weight, bias, validity, C, H * W);
    return check_launch("disc_head_fwd");
}

size_t dmc_disc_head_bwd_bytes(int M, int C, int H, int W) {
    if (!dmc_disc_head_supported(M, C, H, W)) return 0;
    return (size_t)head_slices(M) * 2 * C * H * W * sizeof(float);
}

int dmc_disc_head_bwd(const float* x, const float* weight, const float* dvalidity, float* dx, float* dweight, float* dbias,
                      void* workspace, int M, int C, int H, int W, dmc_stream_t stream) {
    if (!dvalidity) return fail(DMC_E_INVALID, "dmc_disc_head_bwd: null pointer (dvalidity)");
    if (dx && !weight) return fail(DMC_E_INVALID, "dmc_disc_head_bwd: dx needs the weight");
    if (dweight && (!x || !workspace)) return fail(DMC_E_INVALID, "dmc_disc_head_bwd: dweight needs x and the workspace");
    if (!dx && !dweight && !dbias) return fail(DMC_E_INVALID, "dmc_disc_head_bwd: no output requested");
    if (!dmc_disc_head_supported(M, C, H, W))
        return fail(DMC_E_INVALID, "dmc_disc_head_bwd: unsupported shape M=%d C=%d H=%d W=%d", M, C, H, W);
    hipStream_t s = (hipStream_t)stream;
    const int HW = H * W;
    const size_t F = (size_t)C * HW;
    const int nslices = head_slices(M);
    const int nb = (int)((F / 4 + 255) / 256);
    const size_t grid = (size_t)nb * nslices;
    if (grid >= (1ul << 31)) return fail(DMC_E_INVALID, "dmc_disc_head_bwd: grid too large");
    float* part = static_cast<float*>(workspace);
    if (dx && dweight) disc_head_bwd_kernel<true, true><<<(unsigned)grid, 256, 0, s>>>(x, weight, dvalidity, dx, part, M, C, HW, nb);
    else if (dx) disc_head_bwd_kernel<true, false><<<(unsigned)grid, 256, 0, s>>>(nullptr, weight, dvalidity, dx, nullptr, M, C, HW, nb);
    else if (dweight) disc_head_bwd_kernel<false, true><<<(unsigned)grid, 256, 0, s>>>(x, nullptr, dvalidity, nullptr, part, M, C, HW, nb);
    if (dx || dweight) {
        int rc = check_launch("disc_head_bwd");
        if (rc) return rc;
    }
    if (!dweight && !dbias) return DMC_OK;
    const int nbw = dweight ? (int)((2 * F + 255) / 256) : 0;
    disc_head_bwd_final_kernel<<<nbw + (dbias ? 1 : 0), 256, 0, s>>>(part, nslices, dweight, dvalidity, dbias, M, C, HW, nbw);
    return check_launch("disc_head_bwd_final");
}

}  // extern "C"
