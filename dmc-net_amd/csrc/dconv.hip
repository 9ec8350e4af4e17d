// The dilated 3x3 convolutions of ContextNetwork / ContextNetworkAtt in TRAINING (code/dmcnet/model.py:45-104): the raw
// convolution -- forward and data gradient -- and the weight gradient of the middle units
//   Conv2d(Cin, Cout, 3, stride 1, padding d, dilation d, bias=False),   Cin, Cout in {32, 64, 96, 128}, d in {1, 2, 4, 8, 16}
// over NHWC fp32 tensors.  BatchNorm and LeakyReLU stay with their modules; this file replaces the convolutions only.
//
// dconv_fwd_kernel.  ctx_common.h's gather_gemm (the main loop of ctx_eval.hip's unit kernel, described there) with a raw
// epilogue: one 16-byte store per accumulator quad.  With stride 1 and padding = dilation the DATA GRADIENT is the same
// convolution: dx[p][ci] = sum over (t, co) of dy[p + o(t)][co] w[co][8 - t][ci], because o(8 - t) = -o(t) -- so the caller
// packs the weights transposed (pack_kernel, transposed = 1) and calls the same entry point with Cin and Cout exchanged.
//
// dconv_wgrad_kernel.  dw[co][t][ci] = sum over pixels p of dy[p][co] x[p + o(t)][ci], the pixels whose tap lies inside the
// frame (tested per coordinate, never on a linearised offset).  A GEMM over PIXELS (K) while both tensors are channel-contiguous:
//   * grid = (pixel ranges, 9 taps).  wgrad_plan (ctx_wgrad.h, with the constants and the reduce; dense_train.hip shares them):
//     steps = ceil(N H W / 32) are dealt to min(steps, 64) ranges, a range is capped at 256 steps (8 k pixels: the length of
//     one fp32 accumulation), ranges = ceil(steps / per_range).  A workgroup of four waves owns the whole [Cout][Cin] block of its
//     tap -- up to sixteen 32 x 32 tiles, tile q of the block with wave q % 4, at most four per wave (64 accumulator registers) --
//     over its range.
//   * a step is KP = 32 pixels: the workgroup loads dy[32][Cout] and the tap-shifted x[32][Cin] (zeros where the tap leaves the
//     frame or the pixel is past the tensor) into registers one step ahead, splits each value into its three bf16 slices ONCE and
//     stores them as chunk planes [slice][16-channel chunk][pixel][16] (32 bytes per pixel, 16-byte writes).  Plane stride
//     1152 bytes = 128 (mod 256): the two 16-lane groups of a half-wave read planes that are an odd multiple of 128 bytes
//     apart, four consecutive pixels are 128 contiguous bytes -- the layout of x3s_wgrad_kernel (conv_x3s.hip).
//   * fragments leave the LDS transposed (ds_read_b64_tr_b16, two reads = the eight consecutive pixels of an operand row);
//     every wave executes them with all lanes (the tile test is wave-uniform).
//   * partial sums [range][Cout][9][Cin] go to the caller's workspace; ordered_reduce_kernel adds the ranges in order.
// No atomics anywhere: results are bit-identical from run to run.  All tensor offsets are 64-bit; dmc_dconv_supported bounds
// N H W 128 below 2^31 so that pixel indices fit an int.
#include "ctx_wgrad.h"

using namespace dmc;
using namespace dmc::ctxk;

namespace {

struct FwdArgs {
    GatherArgs g;
    float* y;                       // [N][H][W][Cout]
};

template <int TN, int TM>
__global__ __launch_bounds__(256) void dconv_fwd_kernel(FwdArgs a) {
    constexpr int COUT = 32 * TN;
    __shared__ __attribute__((aligned(16))) char lds[GatherLds<TN>::BYTES];
    f32x16 acc[TM][TN];
    const int m0 = gather_gemm<TN, TM>(a.g, lds, acc);
    const int lane = threadIdx.x & 63;
    const int l31 = lane & 31, khalf = lane >> 5;
#pragma unroll
    for (int i = 0; i < TM; ++i) {
        const int m = m0 + 32 * i + l31;
        if (m >= a.g.M) continue;
        float* yp = a.y + (long)m * COUT + 4 * khalf;
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int gq = 0; gq < 4; ++gq) {
                f32x4 v;
#pragma unroll
                for (int e = 0; e < 4; ++e) v[e] = acc[i][j][4 * gq + e];
                *reinterpret_cast<f32x4*>(yp + 32 * j + 8 * gq) = v;
            }
    }
}

// ---- weight gradient ---------------------------------------------------------------------------------------------------
struct WgArgs {
    const float* x;                 // [N][H][W][Cin]
    const float* dy;                // [N][H][W][Cout]
    float* part;                    // [ranges][Cout][9][Cin]
    int H, W, Cin, Cout, d, M;
    int steps_per_range, steps;
};

__global__ __launch_bounds__(256) void dconv_wgrad_kernel(WgArgs a) {
    __shared__ __attribute__((aligned(1024))) char lds[2 * TILE_BYTES];        // dy tile | x tile
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l31 = lane & 31, khalf = lane >> 5, L = lane & 15, grp = (lane >> 4) & 1;
    const int tap = blockIdx.y;
    const int oy = (tap / 3 - 1) * a.d, ox = (tap % 3 - 1) * a.d;
    const long toff = ((long)oy * a.W + ox) * a.Cin;
    const int hw = a.H * a.W;
    const int s_begin = blockIdx.x * a.steps_per_range;
    const int s_end = s_begin + a.steps_per_range < a.steps ? s_begin + a.steps_per_range : a.steps;

    // ---- staging: item = (pixel of the step, 8 consecutive channels); the same items in every step ----
    // dy has KP Cout / 8 items, x has KP Cin / 8: at most 512 each, two per thread
    const int go = a.Cout >> 3, gi = a.Cin >> 3;
    int dpix[2], dcg[2], xpix[2], xcg[2];
    bool dlive[2], xlive[2];
#pragma unroll
    for (int r = 0; r < 2; ++r) {
        const int idx = r * 256 + tid;
        dlive[r] = idx < KP * go; xlive[r] = idx < KP * gi;
        dpix[r] = idx / go; dcg[r] = idx - dpix[r] * go;
        xpix[r] = idx / gi; xcg[r] = idx - xpix[r] * gi;
    }
    f32x4 dlo[2], dhi[2], xlo[2], xhi[2];
    const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};
    auto load_step = [&](int s) {
        const int p0 = s * KP;
#pragma unroll
        for (int r = 0; r < 2; ++r) {
            dlo[r] = zero4; dhi[r] = zero4; xlo[r] = zero4; xhi[r] = zero4;
            const int pd = p0 + dpix[r];
            if (dlive[r] && pd < a.M) {
                const float* q = a.dy + (long)pd * a.Cout + 8 * dcg[r];
                dlo[r] = *reinterpret_cast<const f32x4*>(q); dhi[r] = *reinterpret_cast<const f32x4*>(q + 4);
            }
            const int px = p0 + xpix[r];
            if (xlive[r] && px < a.M) {
                const int rem = px % hw;
                const int yy = rem / a.W, xx = rem - yy * a.W;
                const int iy = yy + oy, ix = xx + ox;
                if (iy >= 0 && iy < a.H && ix >= 0 && ix < a.W) {
                    const float* q = a.x + (long)px * a.Cin + toff + 8 * xcg[r];
                    xlo[r] = *reinterpret_cast<const f32x4*>(q); xhi[r] = *reinterpret_cast<const f32x4*>(q + 4);
                }
            }
        }
    };
    auto store_step = [&]() {
#pragma unroll
        for (int r = 0; r < 2; ++r) {
            if (dlive[r]) {
                const Split3 s3 = split8(dlo[r], dhi[r]);
                char* q = lds + (dcg[r] >> 1) * PLANE + dpix[r] * 32 + (dcg[r] & 1) * 16;
#pragma unroll
                for (int sl = 0; sl < 3; ++sl) *reinterpret_cast<u32x4*>(q + sl * NCHUNK * PLANE) = s3.s[sl];
            }
            if (xlive[r]) {
                const Split3 s3 = split8(xlo[r], xhi[r]);
                char* q = lds + TILE_BYTES + (xcg[r] >> 1) * PLANE + xpix[r] * 32 + (xcg[r] & 1) * 16;
#pragma unroll
                for (int sl = 0; sl < 3; ++sl) *reinterpret_cast<u32x4*>(q + sl * NCHUNK * PLANE) = s3.s[sl];
            }
        }
    };

    // ---- this wave's tiles: q = wave + 4 j < tiles; co tile q / tni, ci tile q % tni (wave-uniform) ----
    const int tni = a.Cin >> 5, tiles = (a.Cout >> 5) * tni;
    f32x16 acc[4];
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[j][e] = 0.f;

    // fragment address of this lane inside a 32-channel tile's pair of planes: unit (kb, u) is pixel 16 kb + 8 khalf + 4 u + L / 4
    const int frag = grp * PLANE + (8 * khalf + (L >> 2)) * 32 + (L & 3) * 8;
    lds_cptr const LB = (lds_cptr)lds;

    if (s_begin < s_end) {
        load_step(s_begin);
        store_step();
    }
    __syncthreads();
#pragma unroll 1
    for (int s = s_begin; s < s_end; ++s) {
        if (s + 1 < s_end) load_step(s + 1);               // in flight during the MFMAs below
#pragma unroll
        for (int kb = 0; kb < KP / 16; ++kb) {
            int have_a = -1, have_b = -1;
            u32x4 A[3], B[3];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int q = wave + 4 * j;
                if (q >= tiles) break;
                const int tco = q / tni, tci = q - tco * tni;
                if (tco != have_a) {
                    have_a = tco;
                    const int o = frag + 2 * tco * PLANE + kb * 16 * 32;
#pragma unroll
                    for (int sl = 0; sl < 3; ++sl) A[sl] = tr_read2(LB + o + sl * NCHUNK * PLANE, LB + o + sl * NCHUNK * PLANE + 4 * 32);
                }
                if (tci != have_b) {
                    have_b = tci;
                    const int o = TILE_BYTES + frag + 2 * tci * PLANE + kb * 16 * 32;
#pragma unroll
                    for (int sl = 0; sl < 3; ++sl) B[sl] = tr_read2(LB + o + sl * NCHUNK * PLANE, LB + o + sl * NCHUNK * PLANE + 4 * 32);
                }
                // the six slice products, the smallest first (the order of x3s_wgrad_kernel)
                acc[j] = mfma_bf16(A[0], B[2], acc[j]);
                acc[j] = mfma_bf16(A[2], B[0], acc[j]);
                acc[j] = mfma_bf16(A[1], B[1], acc[j]);
                acc[j] = mfma_bf16(A[0], B[1], acc[j]);
                acc[j] = mfma_bf16(A[1], B[0], acc[j]);
                acc[j] = mfma_bf16(A[0], B[0], acc[j]);
            }
        }
        __syncthreads();                                   // every wave has read the step's tiles
        if (s + 1 < s_end) store_step();
        __syncthreads();
    }

    // ---- partials: the lane holds ci = 32 tci + l31, co = 32 tco + 8 gq + 4 khalf + e in acc[j][4 gq + e] ----
    float* out = a.part + (size_t)blockIdx.x * a.Cout * 9 * a.Cin;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int q = wave + 4 * j;
        if (q >= tiles) break;
        const int tco = q / tni, tci = q - tco * tni;
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            const int co = 32 * tco + 8 * (e >> 2) + 4 * khalf + (e & 3);
            out[((size_t)co * 9 + tap) * a.Cin + 32 * tci + l31] = acc[j][e];
        }
    }
}

}  // namespace

extern "C" {

int dmc_dconv_supported(int N, int H, int W, int Cin, int Cout, int dilation) {
    return index_ok(N, H, W) && middle_ok(Cin, Cout, dilation) ? 1 : 0;
}

size_t dmc_dconv_wpack_bytes(int Cin, int Cout) {
    if (!width_ok(Cin) || !width_ok(Cout)) return 0;
    return (size_t)Cin * Cout * 9 * 3 * 2;
}

size_t dmc_dconv_wgrad_workspace_bytes(int N, int H, int W, int Cin, int Cout) {
    if (!index_ok(N, H, W) || !width_ok(Cin) || !width_ok(Cout)) return 0;
    return (size_t)wgrad_plan(N, H, W).ranges * Cout * 9 * Cin * sizeof(float);
}

int dmc_dconv_pack_weights(const float* w_ohwi, void* wpack, int Cin, int Cout, int transposed, dmc_stream_t stream) {
    if (!w_ohwi || !wpack) return fail(DMC_E_INVALID, "dmc_dconv_pack_weights: null pointer");
    if (!width_ok(Cin) || !width_ok(Cout)) return fail(DMC_E_INVALID, "dmc_dconv_pack_weights: unsupported shape (Cin %d, Cout %d)", Cin, Cout);
    const int total = Cin * Cout * 9;
    pack_kernel<<<(total + 255) / 256, 256, 0, (hipStream_t)stream>>>(w_ohwi, reinterpret_cast<unsigned short*>(wpack), Cin, Cout, transposed ? 1 : 0);
    return check_launch("dmc_dconv_pack_weights");
}

int dmc_dconv_fwd(const float* x, const void* wpack, float* y, int N, int H, int W, int Cin, int Cout, int dilation, dmc_stream_t stream) {
    if (!x || !wpack || !y) return fail(DMC_E_INVALID, "dmc_dconv_fwd: null pointer");
    if (!dmc_dconv_supported(N, H, W, Cin, Cout, dilation))
        return fail(DMC_E_INVALID, "dmc_dconv_fwd: unsupported shape (N %d, H %d, W %d, Cin %d, Cout %d, dilation %d)", N, H, W, Cin, Cout, dilation);
    FwdArgs a;
    a.g.x = x; a.g.wpack = reinterpret_cast<const unsigned short*>(wpack); a.y = y;
    a.g.N = N; a.g.H = H; a.g.W = W; a.g.Cin = Cin; a.g.d = dilation; a.g.M = N * H * W;
    constexpr int TM = 2;
    const dim3 grid((a.g.M + 128 * TM - 1) / (128 * TM));
    hipStream_t s = (hipStream_t)stream;
    switch (Cout) {
        case 128: dconv_fwd_kernel<4, TM><<<grid, 256, 0, s>>>(a); break;
        case 96: dconv_fwd_kernel<3, TM><<<grid, 256, 0, s>>>(a); break;
        case 64: dconv_fwd_kernel<2, TM><<<grid, 256, 0, s>>>(a); break;
        default: dconv_fwd_kernel<1, TM><<<grid, 256, 0, s>>>(a); break;
    }
    return check_launch("dmc_dconv_fwd");
}

int dmc_dconv_wgrad(const float* x, const float* dy, float* dw_ohwi, void* workspace, int N, int H, int W, int Cin, int Cout, int dilation,
                    dmc_stream_t stream) {
    if (!x || !dy || !dw_ohwi || !workspace) return fail(DMC_E_INVALID, "dmc_dconv_wgrad: null pointer");
    if (!dmc_dconv_supported(N, H, W, Cin, Cout, dilation))
        return fail(DMC_E_INVALID, "dmc_dconv_wgrad: unsupported shape (N %d, H %d, W %d, Cin %d, Cout %d, dilation %d)", N, H, W, Cin, Cout, dilation);
    const WgPlan p = wgrad_plan(N, H, W);
    WgArgs a;
    a.x = x; a.dy = dy; a.part = reinterpret_cast<float*>(workspace);
    a.H = H; a.W = W; a.Cin = Cin; a.Cout = Cout; a.d = dilation; a.M = N * H * W;
    a.steps_per_range = p.per_range; a.steps = p.steps;
    hipStream_t s = (hipStream_t)stream;
    dconv_wgrad_kernel<<<dim3(p.ranges, 9), 256, 0, s>>>(a);
    const int rc = check_launch("dmc_dconv_wgrad");
    if (rc) return rc;
    const long numel = (long)Cout * 9 * Cin;
    ordered_reduce_kernel<<<(int)((numel + 255) / 256), 256, 0, s>>>(a.part, dw_ohwi, p.ranges, numel);
    return check_launch("dmc_dconv_wgrad");
}

}  // extern "C"
