// GPU-side clip preparation for the I3D variant, modality 'flow+mp4': a decoded uint8 clip [H0][W0][T*7] (frame t =
// channels 7t .. 7t+6 = flow_x flow_y mv_x mv_y res0 res1 res2) -> the fp32 tensor [7][T][OH][OW] the reference's loader
// hands to the network, bit for bit.
//
// Reference behaviour: code/dmcnet_I3D/data/iterator_factory.py:49-56,72-77 (which transforms), image_transforms.py:138-200
// (CenterCrop / RandomCrop / RandomHorizontalFlip: mirror along W, flow_x and mv_x of every frame -> (256 - v) as uint8, so 0
// stays 0), video_transforms.py:23-70 (ToTensor: rearrange, the two flow channels replaced by their f x f block means --
// ragged blocks zero-padded and still divided by f^2, the mean TRUNCATED because it is assigned into the uint8 array --, then
// float / 255) and image_transforms.py:47-59 (Normalize: zip over the FIRST dimension stops at len(mean), so only channels
// 0 .. n_norm-1 -- flow_x, flow_y, mv_x for the recipe's three means -- get (v - mean) / std).  The random draws stay on the
// host: a plan (y1, x1, flip) per clip.
//
// A byte-granular transpose.  The source is pixel-major (a pixel is a record of 7T bytes, a cropped row one contiguous run),
// the destination plane-major (every (c, t, y) row is OW contiguous floats).  A work unit is (clip, band of rows, chunk of XC
// output pixels, chunk of TC frames); per row the unit's records go through the LDS:
//   in : aligned dword loads + v_alignbyte, whatever the run's byte phase is (the 16 spare bytes behind the clips cover the
//        last dword), re-pitched to an ODD number of dwords per pixel -- the 16 quads of a plane row then read banks
//        4 q P mod 64, sixteen distinct ones (a record of 112 dwords at T = 64 would put all of them on one bank);
//   out: a lane owns 4 consecutive x of one (c, t) plane: four LDS byte reads (the mirror is the index reversal here),
//        the 256-entry table of its channel (u / 255, then (v - mean) / std: fp32, each operation rounded once), one
//        16-byte store.
// flow_ds_factor >= 2: the band is the f rows of a block row; the flow bytes are summed per (t, c, block column) in LDS
// while the other five channels stream out, and the flow planes are written from floor(sum / f^2) after the band's last
// row -- one pass over the source, no workspace.
// HBM traffic = the algorithmic 7 B read + 28 B written per output pixel-frame.
#include <stdint.h>

#include "dmc_common.h"

using namespace dmc;

namespace {

struct ClipArgs {
    const unsigned char* clips;    // [B][H0][W0][T*7]
    const int* plans;              // [B][3] = y1, x1, flip
    float* out;                    // [B][7][T][OH][OW]
    int B, T, H0, W0, OH, OW, f;
    int n_norm;
    float mean[7], stdv[7];
    int XC, TC, P, BR, nbc;        // chunk of output pixels / of frames, LDS pitch of a record (dwords), rows per band, blocks per chunk
    int nxc, ntc, nby;
    int vec4;                      // 16-byte stores (OW % 4 == 0 and out 16-byte aligned)
    long long units;
    unsigned long long ff;         // f * f
};

__device__ __forceinline__ void store4(const ClipArgs& a, float* dst, int x, int wv, const float (&o)[4]) {
    if (a.vec4) {
        *reinterpret_cast<float4*>(dst) = make_float4(o[0], o[1], o[2], o[3]);
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (x + j < wv) dst[j] = o[j];
    }
}

__global__ __launch_bounds__(256) void clip_prep_kernel(ClipArgs a) {
    __shared__ float lut[7][256];
    extern __shared__ unsigned clip_lds[];
    unsigned* rowbuf = clip_lds;                                     // [XC][P]
    unsigned* sums = clip_lds + (size_t)a.XC * a.P;                  // [TC][2][nbc]
    const int tid = threadIdx.x;
    for (int i = tid; i < 7 * 256; i += 256) {
        const int c = i >> 8;
        float v = (float)(i & 255) / 255.0f;
        if (c < a.n_norm) {
            v = v - a.mean[c];
            v = v / a.stdv[c];
        }
        lut[c][i & 255] = v;
    }
    const bool blockify = a.f >= 2;
    const size_t R = (size_t)7 * a.T;
    for (long long unit = blockIdx.x; unit < a.units; unit += gridDim.x) {
        const int xc = (int)(unit % a.nxc);
        long long u = unit / a.nxc;
        const int tc = (int)(u % a.ntc);
        u /= a.ntc;
        const int by = (int)(u % a.nby), b = (int)(u / a.nby);
        const int y1 = a.plans[3 * b], x1 = a.plans[3 * b + 1];
        const bool flip = a.plans[3 * b + 2] != 0;
        const int t0 = tc * a.TC, tcn = a.T - t0 < a.TC ? a.T - t0 : a.TC;
        const int RB = 7 * tcn, PD = (RB + 3) >> 2;                   // bytes / dwords of a pixel's part of the record
        const int xo0 = xc * a.XC, wv = a.OW - xo0 < a.XC ? a.OW - xo0 : a.XC;
        const int yb0 = by * a.BR, rows = a.OH - yb0 < a.BR ? a.OH - yb0 : a.BR;
        const int xs0 = flip ? x1 + a.OW - xo0 - wv : x1 + xo0;       // first source pixel of the chunk (ascending in memory)
        const int nq = (wv + 3) >> 2;
        if (blockify)
            for (int i = tid; i < tcn * 2 * a.nbc; i += 256) sums[i] = 0;   // (the first row's barrier orders this before the adds)
        for (int r = 0; r < rows; ++r) {
            const int y = yb0 + r;
            const size_t rowoff = (((size_t)b * a.H0 + (y1 + y)) * a.W0 + xs0) * R + (size_t)7 * t0;
            for (int i = tid; i < wv * PD; i += 256) {
                const int p = i / PD, j = i - p * PD;
                const size_t off = rowoff + (size_t)p * R + (size_t)4 * j;
                const unsigned* w = reinterpret_cast<const unsigned*>(a.clips + (off & ~(size_t)3));
                const unsigned sh = (unsigned)(off & 3);
                const unsigned d0 = w[0];
                const unsigned d1 = sh ? w[1] : 0u;                  // (at most 6 bytes past the record: inside the spare bytes)
                rowbuf[p * a.P + j] = __builtin_amdgcn_alignbyte(d1, d0, sh);
            }
            __syncthreads();
            const unsigned char* rb = reinterpret_cast<const unsigned char*>(rowbuf);
            for (int i = tid; i < RB * nq; i += 256) {
                const int k = i / nq, q = i - k * nq;                 // k: byte of the record = plane (t0 + k / 7, k % 7)
                const int tl = k / 7, c = k - 7 * tl;
                const bool neg = flip && (c == 0 || c == 2);
                int v[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    int x = 4 * q + j;
                    x = x < wv ? x : wv - 1;
                    const int ps = flip ? wv - 1 - x : x;
                    const int s = rb[(size_t)ps * a.P * 4 + k];
                    v[j] = neg ? (256 - s) & 255 : s;
                }
                if (blockify && c < 2) {
                    unsigned* srow = sums + (tl * 2 + c) * a.nbc;
                    if ((a.f & 3) == 0 && 4 * q + 3 < wv) {           // the quad lies in one block column
                        atomicAdd(&srow[4 * q / a.f], (unsigned)(v[0] + v[1] + v[2] + v[3]));
                    } else {
#pragma unroll
                        for (int j = 0; j < 4; ++j)
                            if (4 * q + j < wv) atomicAdd(&srow[(4 * q + j) / a.f], (unsigned)v[j]);
                    }
                } else {
                    const float o[4] = {lut[c][v[0]], lut[c][v[1]], lut[c][v[2]], lut[c][v[3]]};
                    float* dst = a.out + ((((size_t)b * 7 + c) * a.T + (t0 + tl)) * a.OH + y) * a.OW + xo0 + 4 * q;
                    store4(a, dst, 4 * q, wv, o);
                }
            }
            __syncthreads();
        }
        if (blockify) {
            for (int i = tid; i < tcn * 2 * a.nbc; i += 256) sums[i] = (unsigned)((unsigned long long)sums[i] / a.ff);
            __syncthreads();
            const int per_row = tcn * 2 * nq;
            for (long long i = tid; i < (long long)rows * per_row; i += 256) {
                const int r = (int)(i / per_row), e = (int)(i - (long long)r * per_row);
                const int k = e / nq, q = e - k * nq;                 // k = tl * 2 + c
                const int tl = k >> 1, c = k & 1;
                const unsigned* srow = sums + k * a.nbc;
                float o[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    int x = 4 * q + j;
                    x = x < wv ? x : wv - 1;
                    o[j] = lut[c][srow[x / a.f]];
                }
                float* dst = a.out + ((((size_t)b * 7 + c) * a.T + (t0 + tl)) * a.OH + (yb0 + r)) * a.OW + xo0 + 4 * q;
                store4(a, dst, 4 * q, wv, o);
            }
            __syncthreads();
        }
    }
}

// Tiling: XC output pixels x TC frames of one row in the LDS at a time.  XC is a multiple of lcm(4, f) -- whole block columns
// and 16-byte-aligned quads per chunk -- or covers the row; the record's pitch is the odd dword count above its bytes.  The
// pair is shrunk until the row buffer and the block sums fit LDS_BUDGET (any T fits: TC goes down to one frame), and further
// until there are enough work units to fill the device (a band of f rows x 64 pixels x all T frames leaves 168 units for
// the recipe's batch of 3 clips).
constexpr size_t LDS_BUDGET = 40 * 1024;
#ifndef DMC_CLIP_MIN_UNITS
#define DMC_CLIP_MIN_UNITS 1024
#endif
#ifndef DMC_CLIP_XC
#define DMC_CLIP_XC 64
#endif
#ifndef DMC_CLIP_XC_FLOOR
#define DMC_CLIP_XC_FLOOR 32
#endif
#ifndef DMC_CLIP_TC_FLOOR
#define DMC_CLIP_TC_FLOOR 8
#endif
#ifndef DMC_CLIP_GRID
#define DMC_CLIP_GRID 2048
#endif

struct ClipCfg { int XC, TC, P, BR, nbc, nxc, ntc, nby; size_t lds; long long units; };

bool clip_cfg(int B, int T, int OH, int OW, int f, ClipCfg* c) {
    const long long W4 = ((long long)OW + 3) & ~3ll;
    long long unit = 4;
    if (f >= 2) unit = (f % 4 == 0) ? f : (f % 2 == 0 ? 2ll * f : 4ll * f);
    if (unit > W4) unit = W4;                                        // one chunk covers the row
    long long n = unit >= DMC_CLIP_XC ? 1 : DMC_CLIP_XC / unit;
    if (n > (W4 + unit - 1) / unit) n = (W4 + unit - 1) / unit;
    int TC = T;
    auto fill = [&]() {
        c->XC = (int)(n * unit); c->TC = TC; c->P = ((7 * TC + 3) / 4) | 1;
        c->nbc = f >= 2 ? (c->XC + f - 1) / f : 0;
        c->lds = (size_t)c->XC * c->P * 4 + (size_t)TC * 2 * c->nbc * 4;
        c->BR = f >= 2 ? (f < OH ? f : OH) : (OH < 8 ? OH : 8);
        c->nxc = (int)((OW + c->XC - 1) / c->XC); c->ntc = (T + TC - 1) / TC; c->nby = (OH + c->BR - 1) / c->BR;
        c->units = (long long)B * c->nby * c->ntc * c->nxc;
    };
    if (unit * 3 * 4 + 2 * 4 * ((f >= 2) ? (unit + f - 1) / f : 0) > (long long)LDS_BUDGET) return false;   // one frame of one unit
    fill();
    while (c->lds > LDS_BUDGET) {
        if (n > 1 && (n / 2) * unit >= 16) n /= 2;
        else if (TC > 1) TC = (TC + 1) / 2;
        else n /= 2;                                                 // (n > 1 here: one frame of one unit fits)
        fill();
    }
    while (c->units < DMC_CLIP_MIN_UNITS) {
        if (n > 1 && (n / 2) * unit >= DMC_CLIP_XC_FLOOR) n /= 2;
        else if (TC > DMC_CLIP_TC_FLOOR) TC = (TC + 1) / 2;
        else break;
        fill();
    }
    return true;
}

}  // namespace

extern "C" {

size_t dmc_prepare_clip_workspace_bytes(int B, int T, int OH, int OW, int flow_ds_factor) {
    (void)B; (void)T; (void)OH; (void)OW; (void)flow_ds_factor;
    return 0;                                                        // the block sums live in LDS
}

int dmc_prepare_clip(const unsigned char* clips_u8, const int* plans, float* out, void* workspace,
                     int B, int T, int H0, int W0, int OH, int OW, int flow_ds_factor,
                     int n_norm, const float* mean_host, const float* std_host, dmc_stream_t stream) {
    (void)workspace;                                                 // dmc_prepare_clip_workspace_bytes() == 0: NULL is accepted
    if (!clips_u8 || !plans || !out) return fail(DMC_E_INVALID, "dmc_prepare_clip: null pointer");
    if (n_norm < 0 || n_norm > 7) return fail(DMC_E_INVALID, "dmc_prepare_clip: n_norm %d outside 0 .. 7", n_norm);
    if (n_norm > 0 && (!mean_host || !std_host)) return fail(DMC_E_INVALID, "dmc_prepare_clip: null mean / std with n_norm %d", n_norm);
    if (B <= 0 || T <= 0 || H0 <= 0 || W0 <= 0 || OH <= 0 || OW <= 0)
        return fail(DMC_E_INVALID, "dmc_prepare_clip: bad shape");
    if (flow_ds_factor < 0) return fail(DMC_E_INVALID, "dmc_prepare_clip: negative flow_ds_factor");
    if (OH > H0 || OW > W0) return fail(DMC_E_INVALID, "dmc_prepare_clip: output %d x %d exceeds the clip's %d x %d", OH, OW, H0, W0);
    if (T > INT32_MAX / 7) return fail(DMC_E_INVALID, "dmc_prepare_clip: T too large");
    if (((uintptr_t)clips_u8 & 3) || ((uintptr_t)out & 3) || ((uintptr_t)plans & 3))
        return fail(DMC_E_INVALID, "dmc_prepare_clip: pointers must be 4-byte aligned");
    const int f = flow_ds_factor;
    if (f >= 2) {                                                    // the 32-bit block sums must hold 255 per summed pixel
        const unsigned long long bh = f < OH ? f : OH, bw = f < OW ? f : OW;
        if (255ull * bh * bw > 0xffffffffull) return fail(DMC_E_INVALID, "dmc_prepare_clip: block of %d x %d pixels overflows the sums", (int)bh, (int)bw);
    }
    ClipCfg c;
    if (!clip_cfg(B, T, OH, OW, f, &c))
        return fail(DMC_E_INVALID, "dmc_prepare_clip: flow_ds_factor %d over %d columns: one block column does not fit the LDS", f, OW);
    ClipArgs a;
    a.clips = clips_u8; a.plans = plans; a.out = out;
    a.B = B; a.T = T; a.H0 = H0; a.W0 = W0; a.OH = OH; a.OW = OW; a.f = f;
    a.n_norm = n_norm;
    for (int i = 0; i < 7; ++i) { a.mean[i] = i < n_norm ? mean_host[i] : 0.f; a.stdv[i] = i < n_norm ? std_host[i] : 1.f; }
    a.XC = c.XC; a.TC = c.TC; a.P = c.P; a.BR = c.BR; a.nbc = c.nbc; a.nxc = c.nxc; a.ntc = c.ntc; a.nby = c.nby;
    a.vec4 = (OW % 4 == 0) && !((uintptr_t)out & 15);
    a.units = c.units;
    a.ff = f >= 2 ? (unsigned long long)f * f : 1ull;
    const int grid = (int)(c.units < DMC_CLIP_GRID ? c.units : DMC_CLIP_GRID);
    clip_prep_kernel<<<grid, 256, c.lds, (hipStream_t)stream>>>(a);
    return check_launch("prepare_clip");
}

}  // extern "C"
