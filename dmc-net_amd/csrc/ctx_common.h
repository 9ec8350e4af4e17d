// Device code shared by the 3x3 gather convolutions; gfx950 only.  Users: ctx_eval.hip (conv + BatchNorm + LeakyReLU in eval mode),
// dconv.hip (the raw dilated convolution of the training route, forward and data gradient), dense_eval.hip (a layer of the dense
// estimators, in place on the feature buffer) and dense_train.hip (that layer's data gradient).
//
// gather_gemm<TN, TM> is the ONE main loop of all four: the per-lane activation gather with the 9-bit tap mask, the
// double-buffered weight panel in LDS, the six bf16x3 slice products in one fixed order.  What it reads it asks of the kernel's
// own argument struct (GatherArgs, DenseArgs: the view); what happens to the accumulators afterwards (the epilogue) is the
// caller's.  pack_kernel writes the weight panels the loop reads, in either orientation.  What the weight gradients of the same
// routes share is in ctx_wgrad.h.
#pragma once
#include "dmc_common.h"

namespace dmc {
namespace ctxk {

struct GatherArgs {
    const float* x;                 // [N][H][W][Cin]
    const unsigned short* wpack;    // [9][Cin / 16][3][Cout][16] bf16
    int N, H, W, Cin, d, M;         // M = N H W
    // the view gather_gemm reads: pixel stride = contraction length = Cin, from channel 0, at dilation d
    __device__ const float* base() const { return x; }
    __device__ int stride() const { return Cin; }
    __device__ int length() const { return Cin; }
    __device__ int first() const { return 0; }
    __device__ int dilation() const { return d; }
};

template <int TN>
struct GatherLds {
    static constexpr int COUT = 32 * TN;
    static constexpr int CH = 3 * COUT * 32;               // bytes of one step's weight chunk (three slices of [COUT][16] bf16)
    static constexpr int BYTES = 2 * CH;
};

// The view V: channels [first(), first() + length()) of pixel rows that are stride() floats apart, from base(), at dilation();
// H, W, M and wpack [9][length() / 16][3][32 TN][16] bf16 by these names.  It is the kernel's argument struct, read in place.
//
// GEMM view: rows = output channels (A operand = weight slices), columns = output pixels (B operand = the input at the
// tap-shifted pixel), contraction = (tap, channel) in k-blocks of 16 channels.  A workgroup of four waves (256 threads) owns 128 TM
// consecutive pixels from blockIdx.x * 128 TM; the wave owns 32 TM of them, from m0 (returned), and all 32 TN channels.
// On return the lane holds pixel m0 + 32 i + (lane & 31), channels 32 j + 8 gq + 4 (lane >> 5) + e in acc[i][j][4 gq + e].
// lds: GatherLds<TN>::BYTES bytes, 16-byte aligned.
template <int TN, int TM, class V>
__device__ __forceinline__ int gather_gemm(const V& a, char* lds, f32x16 (&acc)[TM][TN]) {
    constexpr int COUT = GatherLds<TN>::COUT;
    constexpr int CH = GatherLds<TN>::CH;
    constexpr int NWR = (CH + 4095) / 4096;                // 16-byte pieces per thread

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l31 = lane & 31, khalf = lane >> 5;
    const int m0 = blockIdx.x * (128 * TM) + wave * (32 * TM);

    // ---- this lane's pixels: offset of (n, y, x, first() + 8 khalf) and the taps that fall inside the frame ----
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
            xbase[i] = (long)m * a.stride() + a.first() + 8 * khalf;
#pragma unroll
            for (int t = 0; t < 9; ++t) {
                const int iy = yy + (t / 3 - 1) * a.dilation(), ix = xx + (t % 3 - 1) * a.dilation();
                if (iy >= 0 && iy < a.H && ix >= 0 && ix < a.W) tmask[i] |= 1u << t;
            }
        }
    }

    const int nkb = a.length() >> 4;
    const int nsteps = 9 * nkb;
    int tap = 0, kb = 0;                                   // of the step being LOADED
    f32x4 xlo[TM], xhi[TM];
    u32x4 wr[NWR];
    auto load_step = [&](int s) {
        const int dy = (tap / 3 - 1) * a.dilation(), dx = (tap % 3 - 1) * a.dilation();
        const long toff = ((long)dy * a.W + dx) * a.stride() + 16 * kb;
#pragma unroll
        for (int i = 0; i < TM; ++i) {
            const bool ok = (tmask[i] >> tap) & 1;
            // (a masked lane reads the first 16 gathered channels of pixel 0)
            const float* p = a.base() + (ok ? xbase[i] + toff : (long)a.first());
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

// w [Cout][9][Cin] fp32 (OHWI) -> bf16 slices [9][K / 16][3][R][16], the panels gather_gemm reads with Cin = K, Cout = R.
//   transposed == 0: the forward's pack, K = Cin, R = Cout: element (tap, ci, co) = w[co][tap][ci];
//   transposed != 0: the data gradient's, K = Cout, R = Cin: element (tap', co, ci) = w[co][8 - tap'][ci] (the taps mirrored:
//                    offset(8 - t) = -offset(t) with stride 1 and padding = dilation).
static __global__ __launch_bounds__(256) void pack_kernel(const float* __restrict__ w, unsigned short* __restrict__ wp, int Cin, int Cout,
                                                          int transposed) {
    const int total = Cout * 9 * Cin;
    const int K = transposed ? Cout : Cin, R = transposed ? Cin : Cout;
    const int nkb = K >> 4;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < total; i += gridDim.x * 256) {
        const int ci = i % Cin, tap = (i / Cin) % 9, co = i / (9 * Cin);
        unsigned s0, s1, s2;
        split3_bf16(w[i], s0, s1, s2);
        const int t = transposed ? 8 - tap : tap, k = transposed ? co : ci, r = transposed ? ci : co;
        const long panel = ((long)(t * nkb + (k >> 4)) * 3) * R;            // in rows of 16
        const long o = (panel + r) * 16 + (k & 15);
        wp[o] = (unsigned short)s0;
        wp[o + (long)R * 16] = (unsigned short)s1;
        wp[o + (long)R * 32] = (unsigned short)s2;
    }
}

inline bool dilation_ok(int d) { return d == 1 || d == 2 || d == 4 || d == 8 || d == 16; }
inline bool width_ok(int c) { return c == 32 || c == 64 || c == 96 || c == 128; }
inline bool middle_ok(int Cin, int Cout, int d) { return width_ok(Cin) && width_ok(Cout) && dilation_ok(d); }
// one launch indexes pixels (and the tile rows past the last one) with an int and the widest tensor with 31 bits
inline bool index_ok(int N, int H, int W) { return N > 0 && H > 0 && W > 0 && (long long)N * H * W * 128 < (1ll << 31); }

}  // namespace ctxk

namespace densek {

// kernel arguments of dense_eval.hip's layer and dense_train.hip's data gradient of a layer
struct DenseArgs {
    float* feat;                    // [M][CT]; gathered in [koff, koff + K), written by the caller's epilogue
    const unsigned short* wpack;    // [9][K / 16][3][32 TN][16] bf16
    const float* bias;              // [32 TN] (the forward's epilogue; unused by the data gradient)
    int H, W, CT, K, M;             // M = N H W
    int koff;                       // first gathered channel: 0 in the forward, the layer's slot in the data gradient
    int c0, cend;                   // the data gradient's output channels: [c0, c0 + 32 TN), stored below cend
    // the view gather_gemm reads: pixel stride CT, contraction length K from channel koff, dilation 1
    __device__ const float* base() const { return feat; }
    __device__ int stride() const { return CT; }
    __device__ int length() const { return K; }
    __device__ int first() const { return koff; }
    __device__ int dilation() const { return 1; }
};

}  // namespace densek
}  // namespace dmc
