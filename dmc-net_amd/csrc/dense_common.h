// Device code shared by the dense-estimator routes (dense_eval.hip: the layers in eval mode and the forward of the training
// route; dense_train.hip: the data gradient of a layer); gfx950 only.
//
// dense_gemm<TN, TM> is ctx_common.h's gather_gemm with the pixel stride (CT), the contraction length (K) and the channel at
// which the contraction starts (koff) as three numbers: the per-lane gather with the 9-bit tap mask, the double-buffered weight
// panel in LDS, the six bf16x3 slice products in one fixed order.  The epilogue is the caller's.
#pragma once
#include "ctx_common.h"
#include "mma_bf16.h"

namespace dmc {
namespace densek {

struct DenseArgs {
    float* feat;                    // [M][CT]; gathered in [koff, koff + K), written by the caller's epilogue
    const unsigned short* wpack;    // [9][K / 16][3][32 TN][16] bf16
    const float* bias;              // [32 TN] (the forward's epilogue; unused by the data gradient)
    int H, W, CT, K, M;             // M = N H W
    int koff;                       // first gathered channel: 0 in the forward, the layer's slot in the data gradient
    int c0, cend;                   // the data gradient's output channels: [c0, c0 + 32 TN), stored below cend
};

// Same ownership and the same accumulator layout as gather_gemm: on return the lane holds pixel m0 + 32 i + (lane & 31), channels
// 32 j + 8 gq + 4 (lane >> 5) + e in acc[i][j][4 gq + e].  lds: GatherLds<TN>::BYTES bytes, 16-byte aligned.
template <int TN, int TM>
__device__ __forceinline__ int dense_gemm(const DenseArgs& a, char* lds, f32x16 (&acc)[TM][TN]) {
    using ctxk::GatherLds;
    constexpr int COUT = GatherLds<TN>::COUT;
    constexpr int CH = GatherLds<TN>::CH;
    constexpr int NWR = (CH + 4095) / 4096;                // 16-byte pieces per thread

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l31 = lane & 31, khalf = lane >> 5;
    const int m0 = blockIdx.x * (128 * TM) + wave * (32 * TM);

    // ---- this lane's pixels: offset of (n, y, x, koff + 8 khalf) and the taps that fall inside the frame ----
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
            xbase[i] = (long)m * a.CT + a.koff + 8 * khalf;
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
            const float* p = a.feat + (ok ? xbase[i] + toff : (long)a.koff);   // (a masked lane reads channels koff .. koff + 15 of pixel 0: gathered ones)
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

}  // namespace densek
}  // namespace dmc
