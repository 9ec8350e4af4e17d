"""fp64 references, operands and seeds for the two ends of the ContextNetwork training route (csrc/ctx_ends.hip: the first unit's
5 -> 32 convolution, the heads' 32 -> 2 convolutions and the heads' BatchNorm2d(2) + LeakyReLU (+ ReLU)).

Convolutions: F.conv2d(padding=1) and its autograd in torch.double on the CPU, computed once per shape and never modified.

    first unit   z = conv(x, w),            x [N,5,H,W], w [32,5,3,3];   dx, dw from dz [N,32,H,W]
    heads        z_k = conv(t, w_k),        t [N,32,H,W], w_k [2,32,3,3]; dt_k (per head: the kernel sums them), dw_k from dz_k

BatchNorm on planes: the helpers of tests/ctx_bn_ref.py applied to the [M][2] view of the planes (M = N H W), plus the ReLU form
of the attention head:

    y = max(leaky(t), 0) = max(t, 0),    g = dy (t > 0 ? 1 : 0)        (t == 0 takes the lower branch, as torch does)

Seeds follow the rule of tests/ctx_bn_ref.py: the first seed from 51 at which the fp64 reference alone keeps every
|t| >= 2^-20 max |t| (tests/test_ctx_ends_cpu.py recomputes them)."""
import functools

import numpy as np
import torch
import torch.nn.functional as F

from tests import ctx_bn_ref as R

U32 = R.U32
SLOPE, EPS, MOMENTUM = R.SLOPE, R.EPS, R.MOMENTUM

#: weight-gradient pixel range of ctx_ends.hip (the issue suggested 8192; 2048 gives four times the workgroups at the measured
#: batch).  (3, 61, 47), M = 8601, crosses it four times and leaves a partial last range of 409 pixels.
RANGE = 2048
#: elements per workgroup of the planes' BatchNorm kernels (256 threads x 4); the grid is not capped, so no thread strides
BN_TILE = 1024

#: (N, H, W): only the centre tap inside | tiny | odd everything | H W = 357 odd (planes not 16-byte aligned), a partial workgroup |
#: one full range | M = 8601 crosses the weight-gradient range | three wide single frames at which the weight gradient's copy of
#: the planes no longer fits LDS and the taps come from global memory: at 5 planes (W > 383), at 4 (W > 735), at 2 (W > 2495)
SHAPES = [(1, 1, 1), (2, 2, 3), (7, 5, 3), (2, 21, 17), (2, 33, 18), (3, 61, 47), (1, 3, 400), (1, 2, 740), (1, 1, 2500)]
#: the BatchNorm needs M >= 2: (2, 1, 1) stands in for (1, 1, 1)
BN_SHAPES = [(2, 1, 1), (2, 2, 3), (7, 5, 3), (2, 21, 17), (2, 33, 18), (3, 61, 47)]
#: what R.kink_free_seed(M, 2, "normal") returns
BN_SEEDS = {2: 51, 12: 51, 105: 51, 714: 51, 1188: 51, 8601: 51}


def nranges(m):
    return -(-m // RANGE)


def stage_bytes(planes, w):
    """Bytes of the weight-gradient kernel's LDS copy of its planes, 0 when it does not fit 64 KB beside the 9 KB of group sums."""
    b = planes * (RANGE + 2 * w + 2) * 4
    return b if b + 8 * 288 * 4 <= 65536 else 0


def wgrad_workspace_bytes(n, h, w, planes):
    return nranges(n * h * w) * planes * 288 * 4


def bn_scratch_bytes(n, h, w):
    return -(-(2 * n * h * w) // BN_TILE) * 32 + 16


def rnd(seed, shape, scale=1.0):
    return torch.from_numpy((np.random.RandomState(seed).standard_normal(shape) * scale).astype(np.float32))


@functools.lru_cache(maxsize=None)
def first_case(n, h, w, seed=951):
    """dict(x, w, dz fp32; z, dx, dw fp64) of the first unit's convolution."""
    x, wt, dz = rnd(seed, (n, 5, h, w)), rnd(seed + 1, (32, 5, 3, 3), 0.2), rnd(seed + 2, (n, 32, h, w))
    x64, w64 = x.double().requires_grad_(True), wt.double().requires_grad_(True)
    z = F.conv2d(x64, w64, None, 1, 1, 1)
    z.backward(dz.double())
    return dict(x=x, w=wt, dz=dz, z=z.detach(), dx=x64.grad, dw=w64.grad)


@functools.lru_cache(maxsize=None)
def heads_case(n, h, w, seed=961):
    """dict(t, w [2 heads], dz [2] fp32; z [2], dt [2] (each head's own), dw [2] fp64) of the heads' convolutions."""
    t = rnd(seed, (n, 32, h, w))
    ws = [rnd(seed + 1 + k, (2, 32, 3, 3), 0.1) for k in range(2)]
    dzs = [rnd(seed + 3 + k, (n, 2, h, w)) for k in range(2)]
    zs, dts, dws = [], [], []
    for wt, dz in zip(ws, dzs):
        t64, w64 = t.double().requires_grad_(True), wt.double().requires_grad_(True)
        z = F.conv2d(t64, w64, None, 1, 1, 1)
        z.backward(dz.double())
        zs.append(z.detach()); dts.append(t64.grad); dws.append(w64.grad)
    return dict(t=t, w=ws, dz=dzs, z=zs, dt=dts, dw=dws)


# ------------------------------------------------------------------------------------------ planes <-> [M][2]
def to_planes(t2, n, h, w):
    """[M][2] -> contiguous [N, 2, H, W]."""
    return t2.view(n, h, w, 2).permute(0, 3, 1, 2).contiguous()


def to_rows(t4):
    """[N, 2, H, W] -> [M][2]."""
    return t4.permute(0, 2, 3, 1).reshape(-1, t4.shape[1])


def bn_case(n, h, w, kind="normal"):
    """R.bn_case at C = 2 and the seed of BN_SEEDS: z, dy [M][2], gamma, beta, rm, rv [2] fp32 on the CPU, plus the frame shape."""
    m = n * h * w
    c = R.bn_case(m, 2, BN_SEEDS[m], kind)
    c["frames"] = (n, h, w)
    return c


def crafted_case():
    """(2, 33, 18): channel 1 holds -1, 0, +1 in equal numbers with gamma = 1, beta = 0 (R.crafted_case)."""
    c = R.crafted_case(1188, 2, 1, 51)
    c["frames"] = (2, 33, 18)
    return c


def forward_ref(z, gamma, beta, mean, invstd, relu=False, slope=SLOPE):
    """(y, t, xhat) in fp64 on [M][2] rows; with ``relu`` the attention head's max(., 0) behind the LeakyReLU."""
    y, t, xh = R.forward_ref(z, gamma, beta, mean, invstd, slope)
    return (y.clamp_min(0.0) if relu else y), t, xh


def backward_ref(z, dy, gamma, mean, invstd, positive, relu=False, slope=SLOPE):
    """(dz, dgamma, dbeta) in fp64; ``positive``: the decision t > 0.  With ``relu`` an element at t <= 0 passes nothing."""
    if not relu:
        return R.backward_ref(z, dy, gamma, mean, invstd, positive, slope)
    M = z.shape[0]
    xh = (z.double() - mean.double()) * invstd.double()
    g = dy.double() * positive.double()
    sb, sg = g.sum(0), (g * xh).sum(0)
    return gamma.double() * invstd.double() * (g - sb / M - xh * sg / M), sg, sb
