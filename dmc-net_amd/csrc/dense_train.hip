// EstimatorDenseNet / EstimatorDenseNetSmall in TRAINING (code/dmcnet/model.py:122-170): the backward of the dense stack
//   for i in 0..4: x = cat(LeakyReLU_0.1(conv_i(x)), x);  predict_flow(x)
// on the feature buffer of dense_eval.hip.  The forward is that file's (ingest, five layer launches, head) and leaves
// feat[M][CT] (NHWC fp32, slots in production order) behind; it holds every activation, and the LeakyReLU's branch is the sign of
// the stored output (leaky(v) > 0 exactly when v > 0).  A second buffer G[M][CT] of the same layout holds dL/d(feat): the gradient
// of a concatenation is a sum, and G accumulates it in place.  Given dout NCHW [N][2][H][W]:
//
//   head dgrad   G[m][c] = sum_t sum_co dout[m - o(t)][co] w_head[co][t][c] for EVERY c < CT: the launch writes every float of G
//                (no memset; nothing later reads a float of G that was not written).  fp32 FMAs in a fixed order (two output
//                rows would waste a 32-row matrix-core tile); 8 lanes share a pixel and write 128 contiguous bytes at a time.
//   head wgrad   dW_head[co][t][c] = sum_q feat[q][c] dout[q - o(t)][co], db_head[co] = sum_q dout[q][co]: one thread per channel,
//                fmaf over the pixels of a range in order (at most 8 k pixels per fp32 accumulation), partials per range to the
//                caller's workspace, an ordered reduce.
//   for k = 4 .. 0, K = K_k, R = R_k:
//   mask         G[m][K + r] <- feat[m][K + r] > 0 ? g : 0.1f g in place (pad channels: feat = 0, g = 0, stay 0); the bias
//                gradient db_k[r] = sum_m of the masked value from the same pass: per thread over its pixels in order, the
//                workgroup's threads in order, per-workgroup partials, an ordered final reduce.
//   wgrad        dW_k[r][t][c] = sum_m G[m][K + r] feat[m + o(t)][c], c < K, buffer order: a copy of dconv.hip's
//                dconv_wgrad_kernel with ctx_wgrad.h's wgrad_plan, constants and reduce (bf16x3, the six slice products smallest
//                first, 32-pixel steps, ranges of at most 256 steps = 8 k pixels per fp32 accumulation, partials to the caller's
//                workspace, ordered reduce) with both operands at pixel stride CT, at channel offsets K and 0, and a third grid
//                dimension over 128-channel blocks of c (a workgroup owns at most 128 input channels).  K = 16 + 32 n: the last
//                32-channel tile of the last block has 16 live columns; its other 16 are staged as zeros and never stored.  No
//                read leaves the pixel's row of CT floats, no store leaves dW.
//   dgrad        G[m][c] += sum_t sum_r G[m - o(t)][K + r] W_k[r][t][c], c < K (skipped for k = 0 unless x needs a gradient):
//                ctx_common.h's gather_gemm on the transposed, tap-mirrored pack (ctxk::pack_kernel, transposed = 1) of a block
//                of at most 128 output channels; contraction length R at channel offset K; one launch per block, the last one
//                masked to c < K at the store.
//   export       slot 0's five live channels of G -> dx NCHW.
//
// The data gradient runs IN PLACE.  Its gathers read channels [K, K + R) (of the lane's own and of the neighbouring pixels; a
// masked lane reads those channels of pixel 0); its epilogue reads, adds and writes channels < K of the workgroup's OWN pixels,
// each (pixel, channel) by exactly one lane.  The bytes gathered and the bytes written are disjoint sets of the same buffer, and
// no two workgroups touch the same written byte: no workgroup can observe another's stores, whatever the order in which tiles
// run -- the argument of dense_eval.hip's header with the two channel ranges exchanged.  (K + R <= CT keeps the gathers inside
// the pixel's row.)  The blocks of one layer are separate launches on one stream; they write disjoint channels.  For every channel
// the order of the sum is fixed: head, then layer 4, 3, ...
//
// No atomics anywhere: results are bit-identical from run to run.  All tensor offsets are 64-bit; dmc_densetrain_supported()
// bounds N H W CT below 2^31 so that the pixel index fits an int.  The caller owns every buffer; nothing allocates or synchronises.
#include "ctx_wgrad.h"

using namespace dmc;
using namespace dmc::ctxk;
using namespace dmc::densek;

namespace {

constexpr float SLOPE = 0.1f;
constexpr int HEAD_CTMAX = 512;              // 72 CT bytes of LDS hold the head's weight
constexpr int MASK_PIX = 1024;               // pixels per workgroup of the mask pass

// ---- head, data gradient: every float of G.  w [2][9][CT] in LDS (72 CT bytes, dynamic) ----
__global__ __launch_bounds__(256) void head_dgrad_kernel(const float* __restrict__ dout, const float* __restrict__ w, float* __restrict__ G,
                                                         int H, int W, int CT, int M) {
    extern __shared__ __attribute__((aligned(16))) float ws[];           // [co][tap][c]
    for (int i = threadIdx.x; i < 18 * CT; i += 256) ws[i] = w[i];
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

// ---- head, weight and bias gradient: grid (ranges, CT / 256); the thread owns channel c over the range's pixels in order.
// part: [ranges][18][CT] then [ranges][2] ----
__global__ __launch_bounds__(256) void head_wgrad_kernel(const float* __restrict__ dout, const float* __restrict__ feat, float* __restrict__ part,
                                                         int H, int W, int CT, int M, int per_range, int ranges) {
    const int c = blockIdx.y * 256 + threadIdx.x;
    const bool live = c < CT;
    const int hw = H * W;
    const int q0 = blockIdx.x * per_range * KP;
    const int q1 = q0 + per_range * KP < M ? q0 + per_range * KP : M;
    float acc0[9], acc1[9];
#pragma unroll
    for (int t = 0; t < 9; ++t) { acc0[t] = 0.f; acc1[t] = 0.f; }
    float b0 = 0.f, b1 = 0.f;
#pragma unroll 1
    for (int qp = q0; qp < q1; ++qp) {                                     // the input pixel; the output pixel of tap t is qp - o(t)
        const int n = qp / hw, rem = qp - n * hw;
        const int yy = rem / W, xx = rem - yy * W;
        const float f = live ? feat[(long)qp * CT + c] : 0.f;
        const float* dp = dout + (long)n * 2 * hw;
#pragma unroll
        for (int t = 0; t < 9; ++t) {
            const int py = yy - (t / 3 - 1), px = xx - (t % 3 - 1);
            if (py >= 0 && py < H && px >= 0 && px < W) {                  // (uniform over the workgroup)
                const float a0 = dp[py * W + px], a1 = dp[hw + py * W + px];
                acc0[t] = fmaf(a0, f, acc0[t]);
                acc1[t] = fmaf(a1, f, acc1[t]);
                if (t == 4) { b0 += a0; b1 += a1; }
            }
        }
    }
    if (live) {
        float* out = part + (size_t)blockIdx.x * 18 * CT + c;
#pragma unroll
        for (int t = 0; t < 9; ++t) {
            out[(size_t)t * CT] = acc0[t];
            out[(size_t)(9 + t) * CT] = acc1[t];
        }
    }
    if (blockIdx.y == 0 && threadIdx.x == 0) {
        float* pb = part + (size_t)ranges * 18 * CT + 2 * blockIdx.x;
        pb[0] = b0; pb[1] = b1;
    }
}

// ---- mask pass: the slot [K, K + R) of G in place, and the bias gradient's partial sums [workgroup][R].  Thread = (pixel lane,
// channel quad); 256 / (R / 4) pixel lanes (R = 96: 10 lanes, 16 threads idle) ----
__global__ __launch_bounds__(256) void mask_kernel(const float* __restrict__ feat, float* __restrict__ G, float* __restrict__ part, int CT, int K,
                                                   int R, int M) {
    __shared__ f32x4 red[256];
    const int nq = R >> 2, npl = 256 / nq;
    const int q = threadIdx.x % nq, pl = threadIdx.x / nq;
    const int p0 = blockIdx.x * MASK_PIX;
    const int p1 = p0 + MASK_PIX < M ? p0 + MASK_PIX : M;
    f32x4 s = {0.f, 0.f, 0.f, 0.f};
    if (pl < npl) {
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
        *reinterpret_cast<f32x4*>(part + (size_t)blockIdx.x * R + 4 * threadIdx.x) = t;
    }
}

// ---- layer, weight gradient: dconv_wgrad_kernel at pixel stride CT; grid (ranges, 9 taps, 128-channel blocks of c) ----
struct WgArgs {
    const float* feat;              // [M][CT]: x = channels [0, K)
    const float* G;                 // [M][CT]: dy = channels [K, K + R)
    float* part;                    // [ranges][R][9][K]
    int H, W, CT, K, R, M;
    int steps_per_range, steps;
};

__global__ __launch_bounds__(256) void dense_wgrad_kernel(WgArgs a) {
    __shared__ __attribute__((aligned(1024))) char lds[2 * TILE_BYTES];        // dy tile | x tile
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l31 = lane & 31, khalf = lane >> 5, L = lane & 15, grp = (lane >> 4) & 1;
    const int tap = blockIdx.y;
    const int oy = tap / 3 - 1, ox = tap % 3 - 1;
    const int c0 = blockIdx.z * 128;
    const int live = a.K - c0 < 128 ? a.K - c0 : 128;                          // this block's input channels: a multiple of 16
    const int tni = (live + 31) >> 5;                                          // ... in 32-channel tiles, the last one maybe half live
    const long toff = ((long)oy * a.W + ox) * a.CT + c0;
    const int hw = a.H * a.W;
    const int s_begin = blockIdx.x * a.steps_per_range;
    const int s_end = s_begin + a.steps_per_range < a.steps ? s_begin + a.steps_per_range : a.steps;

    // ---- staging: item = (pixel of the step, 8 consecutive channels); the same items in every step ----
    // dy has KP R / 8 items, x has KP 4 tni (the dead half of a half-live tile is staged as zeros): at most 512 each, two per thread
    const int go = a.R >> 3, gi = tni * 4;
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
                const float* q = a.G + (long)pd * a.CT + a.K + 8 * dcg[r];
                dlo[r] = *reinterpret_cast<const f32x4*>(q); dhi[r] = *reinterpret_cast<const f32x4*>(q + 4);
            }
            const int px = p0 + xpix[r];
            if (xlive[r] && px < a.M && 8 * xcg[r] < live) {
                const int rem = px % hw;
                const int yy = rem / a.W, xx = rem - yy * a.W;
                const int iy = yy + oy, ix = xx + ox;
                if (iy >= 0 && iy < a.H && ix >= 0 && ix < a.W) {
                    const float* q = a.feat + (long)px * a.CT + toff + 8 * xcg[r];
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

    // ---- this wave's tiles: q = wave + 4 j < tiles; r tile q / tni, c tile q % tni (wave-uniform) ----
    const int tiles = (a.R >> 5) * tni;
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
                // the six slice products, the smallest first (the order of dconv_wgrad_kernel)
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

    // ---- partials: the lane holds c = c0 + 32 tci + l31, r = 32 tco + 8 gq + 4 khalf + e in acc[j][4 gq + e] ----
    float* out = a.part + (size_t)blockIdx.x * a.R * 9 * a.K;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int q = wave + 4 * j;
        if (q >= tiles) break;
        const int tco = q / tni, tci = q - tco * tni;
        const int ci = 32 * tci + l31;
        if (ci >= live) continue;                          // the dead half of the last tile
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            const int co = 32 * tco + 8 * (e >> 2) + 4 * khalf + (e & 3);
            out[((size_t)co * 9 + tap) * a.K + c0 + ci] = acc[j][e];
        }
    }
}

// ---- layer, data gradient: gather_gemm over G[.][K, K + R) on the transposed pack of output channels [c0, c0 + 32 TN); the
// epilogue adds into G[m][c], c < cend, of the workgroup's own pixels ----
template <int TN, int TM>
__global__ __launch_bounds__(256) void dense_dgrad_kernel(DenseArgs a) {
    __shared__ __attribute__((aligned(16))) char lds[GatherLds<TN>::BYTES];
    f32x16 acc[TM][TN];
    const int m0 = gather_gemm<TN, TM>(a, lds, acc);
    const int lane = threadIdx.x & 63;
    const int l31 = lane & 31, khalf = lane >> 5;
#pragma unroll
    for (int j = 0; j < TN; ++j)
#pragma unroll
        for (int gq = 0; gq < 4; ++gq) {
            const int c = a.c0 + 32 * j + 8 * gq + 4 * khalf;
            if (c >= a.cend) continue;                     // (cend % 16 == 0: a quad is wholly inside or wholly outside)
#pragma unroll
            for (int i = 0; i < TM; ++i) {
                const int m = m0 + 32 * i + l31;
                if (m >= a.M) continue;
                float* p = a.feat + (long)m * a.CT + c;
                f32x4 v = *reinterpret_cast<const f32x4*>(p);
#pragma unroll
                for (int e = 0; e < 4; ++e) v[e] += acc[i][j][4 * gq + e];
                *reinterpret_cast<f32x4*>(p) = v;
            }
        }
}

// ---- export: G[m][0..5) -> dx NCHW [N][5][H][W]; one thread per pixel ----
__global__ __launch_bounds__(256) void export_kernel(const float* __restrict__ G, float* __restrict__ dx, int HW, int CT, int M) {
    const int m = blockIdx.x * 256 + threadIdx.x;
    if (m >= M) return;
    const int n = m / HW, rem = m - n * HW;
    const float* gp = G + (long)m * CT;
    const f32x4 v = *reinterpret_cast<const f32x4*>(gp);
    float* xp = dx + (long)n * 5 * HW + rem;
    xp[0] = v[0]; xp[HW] = v[1]; xp[2 * (long)HW] = v[2]; xp[3 * (long)HW] = v[3]; xp[4 * (long)HW] = gp[4];
}

}  // namespace

extern "C" {

int dmc_densetrain_supported(int N, int H, int W, int CT, int K, int R) {
    if (!dmc_dense_supported(N, H, W, CT, K, R)) return 0;
    if (R == 2) return (K == CT && CT <= HEAD_CTMAX) ? 1 : 0;     // the head's backward covers the whole buffer
    return 1;
}

size_t dmc_densetrain_mask_workspace_bytes(int N, int H, int W, int R) {
    if (N <= 0 || H <= 0 || W <= 0 || !width_ok(R) || (long long)N * H * W >= (1ll << 31)) return 0;
    const long long M = (long long)N * H * W;
    return (size_t)((M + MASK_PIX - 1) / MASK_PIX) * R * sizeof(float);
}

size_t dmc_densetrain_wgrad_workspace_bytes(int N, int H, int W, int K, int R) {
    if (N <= 0 || H <= 0 || W <= 0 || K < 16 || K % 16 != 0 || !width_ok(R) || (long long)N * H * W >= (1ll << 31)) return 0;
    return (size_t)wgrad_plan(N, H, W).ranges * R * 9 * K * sizeof(float);
}

size_t dmc_densetrain_head_workspace_bytes(int N, int H, int W, int CT) {
    if (N <= 0 || H <= 0 || W <= 0 || CT < 16 || CT % 4 != 0 || CT > HEAD_CTMAX || (long long)N * H * W >= (1ll << 31)) return 0;
    return (size_t)wgrad_plan(N, H, W).ranges * (18 * CT + 2) * sizeof(float);
}

int dmc_densetrain_head_dgrad(const float* dout_nchw, const float* w, float* G, int N, int H, int W, int CT, dmc_stream_t stream) {
    if (!dout_nchw || !w || !G) return fail(DMC_E_INVALID, "dmc_densetrain_head_dgrad: null pointer");
    if (!dmc_densetrain_supported(N, H, W, CT, CT, 2))
        return fail(DMC_E_INVALID, "dmc_densetrain_head_dgrad: unsupported shape (N %d, H %d, W %d, CT %d)", N, H, W, CT);
    const int M = N * H * W;
    head_dgrad_kernel<<<(M + 127) / 128, 256, 72 * CT, (hipStream_t)stream>>>(dout_nchw, w, G, H, W, CT, M);
    return check_launch("dmc_densetrain_head_dgrad");
}

int dmc_densetrain_head_wgrad(const float* dout_nchw, const float* feat, float* dw, float* db, void* workspace, int N, int H, int W, int CT,
                              dmc_stream_t stream) {
    if (!dout_nchw || !feat || !dw || !db || !workspace) return fail(DMC_E_INVALID, "dmc_densetrain_head_wgrad: null pointer");
    if (!dmc_densetrain_supported(N, H, W, CT, CT, 2))
        return fail(DMC_E_INVALID, "dmc_densetrain_head_wgrad: unsupported shape (N %d, H %d, W %d, CT %d)", N, H, W, CT);
    const WgPlan p = wgrad_plan(N, H, W);
    float* part = reinterpret_cast<float*>(workspace);
    hipStream_t s = (hipStream_t)stream;
    head_wgrad_kernel<<<dim3(p.ranges, (CT + 255) / 256), 256, 0, s>>>(dout_nchw, feat, part, H, W, CT, N * H * W, p.per_range, p.ranges);
    int rc = check_launch("dmc_densetrain_head_wgrad");
    if (rc) return rc;
    const long numel = 18l * CT;
    ordered_reduce_kernel<<<(int)((numel + 255) / 256), 256, 0, s>>>(part, dw, p.ranges, numel);
    rc = check_launch("dmc_densetrain_head_wgrad");
    if (rc) return rc;
    ordered_reduce_kernel<<<1, 256, 0, s>>>(part + (size_t)p.ranges * numel, db, p.ranges, 2);
    return check_launch("dmc_densetrain_head_wgrad");
}

int dmc_densetrain_mask(const float* feat, float* G, float* db, void* workspace, int N, int H, int W, int CT, int K, int R, dmc_stream_t stream) {
    if (!feat || !G || !db || !workspace) return fail(DMC_E_INVALID, "dmc_densetrain_mask: null pointer");
    if (R == 2 || !dmc_densetrain_supported(N, H, W, CT, K, R))
        return fail(DMC_E_INVALID, "dmc_densetrain_mask: unsupported shape (N %d, H %d, W %d, CT %d, K %d, R %d)", N, H, W, CT, K, R);
    const int M = N * H * W;
    const int blocks = (M + MASK_PIX - 1) / MASK_PIX;
    float* part = reinterpret_cast<float*>(workspace);
    hipStream_t s = (hipStream_t)stream;
    mask_kernel<<<blocks, 256, 0, s>>>(feat, G, part, CT, K, R, M);
    const int rc = check_launch("dmc_densetrain_mask");
    if (rc) return rc;
    ordered_reduce_kernel<<<1, 256, 0, s>>>(part, db, blocks, R);
    return check_launch("dmc_densetrain_mask");
}

int dmc_densetrain_layer_wgrad(const float* feat, const float* G, float* dw_ohwi, void* workspace, int N, int H, int W, int CT, int K, int R,
                               dmc_stream_t stream) {
    if (!feat || !G || !dw_ohwi || !workspace) return fail(DMC_E_INVALID, "dmc_densetrain_layer_wgrad: null pointer");
    if (R == 2 || !dmc_densetrain_supported(N, H, W, CT, K, R))
        return fail(DMC_E_INVALID, "dmc_densetrain_layer_wgrad: unsupported shape (N %d, H %d, W %d, CT %d, K %d, R %d)", N, H, W, CT, K, R);
    const WgPlan p = wgrad_plan(N, H, W);
    WgArgs a;
    a.feat = feat; a.G = G; a.part = reinterpret_cast<float*>(workspace);
    a.H = H; a.W = W; a.CT = CT; a.K = K; a.R = R; a.M = N * H * W;
    a.steps_per_range = p.per_range; a.steps = p.steps;
    hipStream_t s = (hipStream_t)stream;
    dense_wgrad_kernel<<<dim3(p.ranges, 9, (K + 127) / 128), 256, 0, s>>>(a);
    const int rc = check_launch("dmc_densetrain_layer_wgrad");
    if (rc) return rc;
    const long numel = (long)R * 9 * K;
    ordered_reduce_kernel<<<(int)((numel + 255) / 256), 256, 0, s>>>(a.part, dw_ohwi, p.ranges, numel);
    return check_launch("dmc_densetrain_layer_wgrad");
}

int dmc_densetrain_layer_dgrad(float* G, const void* wpack_t, int N, int H, int W, int CT, int K, int R, int c0, int cb, dmc_stream_t stream) {
    if (!G || !wpack_t) return fail(DMC_E_INVALID, "dmc_densetrain_layer_dgrad: null pointer");
    if (R == 2 || !dmc_densetrain_supported(N, H, W, CT, K, R) || !width_ok(cb) || c0 < 0 || c0 % 16 != 0 || c0 >= K || c0 + cb > K + 16)
        return fail(DMC_E_INVALID, "dmc_densetrain_layer_dgrad: unsupported shape (N %d, H %d, W %d, CT %d, K %d, R %d, c0 %d, cb %d)", N, H, W, CT, K,
                    R, c0, cb);
    DenseArgs a;
    a.feat = G; a.wpack = reinterpret_cast<const unsigned short*>(wpack_t); a.bias = nullptr;
    a.H = H; a.W = W; a.CT = CT; a.K = R; a.M = N * H * W;      // the contraction runs over the layer's R output channels ...
    a.koff = K;                                                  // ... which start at buffer channel K
    a.c0 = c0; a.cend = c0 + cb < K ? c0 + cb : K;
    constexpr int TM = 2;
    const dim3 grid((a.M + 128 * TM - 1) / (128 * TM));
    hipStream_t s = (hipStream_t)stream;
    switch (cb) {
        case 128: dense_dgrad_kernel<4, TM><<<grid, 256, 0, s>>>(a); break;
        case 96: dense_dgrad_kernel<3, TM><<<grid, 256, 0, s>>>(a); break;
        case 64: dense_dgrad_kernel<2, TM><<<grid, 256, 0, s>>>(a); break;
        default: dense_dgrad_kernel<1, TM><<<grid, 256, 0, s>>>(a); break;
    }
    return check_launch("dmc_densetrain_layer_dgrad");
}

int dmc_densetrain_export(const float* G, float* dx_nchw, int N, int H, int W, int CT, dmc_stream_t stream) {
    if (!G || !dx_nchw) return fail(DMC_E_INVALID, "dmc_densetrain_export: null pointer");
    if (N <= 0 || H <= 0 || W <= 0 || CT < 16 || CT % 4 != 0 || (long long)N * H * W * CT >= (1ll << 31))
        return fail(DMC_E_INVALID, "dmc_densetrain_export: unsupported shape (N %d, H %d, W %d, CT %d)", N, H, W, CT);
    const int M = N * H * W;
    export_kernel<<<(M + 255) / 256, 256, 0, (hipStream_t)stream>>>(G, dx_nchw, H * W, CT, M);
    return check_launch("dmc_densetrain_export");
}

}  // extern "C"
