"""fp64 references, derived error bounds and an fp32 emulation for the classifier's fp32 BatchNorm2d family
(csrc/bn_act.hip: conv -> bn [-> add] [-> relu] of every ResNet unit, the stem tail bn1 -> relu -> maxpool, the
discriminator's keep / LeakyReLU tail; conv_stats_final_kernel of csrc/conv_nhwc.hip).

Everything works on [M pixels][C channels] views of channels_last memory.  A stage is compared on the operands it really
had: the statistics against the fp64 statistics of x, every later stage against fp64 arithmetic on the kernel's STORED
statistics (mean, invstd as fp32), the ReLU decision of a backward from the kernel's own forward output (y > 0, or the
mask bytes), the pool's gradient routing from the kernel's codes.  A defect therefore shows in the stage that has it,
and the conditioning of the statistics (cond, below) enters the bounds of the statistics only.

Notation as in bn3d_ref.py: u = 2^-24, one rounded fp32 operation errs by <= u |result|; a chain of n rounded additions
of terms t_i by <= n u SLACK sum |t_i|.  fmaf(a, b, c) is one rounding.  The build has -ffp-contract=off, so the source
order of bn_act.hip is the arithmetic.

The two parts of a bound (bn3d_ref.Bound), and what goes where for fp32 results:
    fmt    every rounding that happens ONCE on the way to the element: the rounding of the stored value itself, the
           (<= 9) other roundings of the element's own formula, the one rounding of a stored statistic that the formula
           reads.  A correct kernel attains each of them (over 10^6 elements some element has all of them near their
           worst at once), so they have no headroom to give: a sum of four roundings cannot be asked to stay below one
           and three quarters.
    arith  what the SUMMATION CHAINS accumulate: n u sum |t_i| of the thread sums, and everything that inherits it (the
           statistics' conditioning, dbeta / M and dgamma / M inside dx).  This is the part a worst-case derivation
           overstates (errors of n additions rarely align), and the part test_bn2d_ref_cpu.py asks headroom of.
For the per-channel results that are stored once after an fp64 reduction (mean, invstd, dgamma, dbeta) fmt is exactly
the one fp32 rounding of the stored value.  ratio() and the GPU tests use fmt + arith; the split only matters to the
headroom test and to excess().

fp64 parts of the kernels (LDS column sums, the partials' reduction, the final statistics) err by a few hundred 2^-53:
U64N stands for them wherever a chain length is 0, so that a bound never claims more than one fp32 rounding can give.
"""
import numpy as np
import torch

from tests.bn3d_ref import Bound, ratio, excess, f32, U32, SLACK  # noqa: F401  (re-exported for the tests)

BN_MAX_SPLIT = 1024
PT = 8                                                          # pooled windows per tile side (pool_bwd_kernel)
#: fp64 operations behind a statistic, in units of u: 4096 roundings of 2^-53 = 2^-17 u (256 thread rows, 12,000 / 256
#: partials per lane, two trees; the test's own fp64 partial sums of <= 2,048 elements)
U64N = 2.0 ** -17
#: worst |rsqrtf(q) - q^-1/2| in ulps of the result, measured on an MI355X against fp64 (never against the kernel: a
#: stand-alone program, same compiler flags) over 2^20 values of q log-uniform in [2^-4, 2^4) -- two periods of the
#: function, and a superset of every running_var + eps of the cases below, which lie in (0.5, 2) -- and over the 59,028
#: running_var values themselves: 0.851 and 0.835 ulp.  (The ROCm device-library documentation is not installed with the
#: toolchain.)  The bar is twice the measurement.
RSQRT_ULP_MEASURED = 0.851
RSQRT_ULP = 2.0 * RSQRT_ULP_MEASURED


# ------------------------------------------------------------------------------------------ launch geometry
def split_of(M, C):
    """bn_act.hip's split_of: row-splits (workgroups) of a per-channel reduction."""
    return max(1, min(M * C // 8192, BN_MAX_SPLIT))


def geometry(M, C, split=None):
    """dict(split, per, rows, iters, empty) of bn_partial_kernel: `per` rows per workgroup, `rows` = 1024 / C thread rows,
    the most iterations a thread makes (= the fp32 chain length of its sums), and the workgroups whose range is empty."""
    split = split_of(M, C) if split is None else split
    per = -(-M // split)
    rows = 1024 // C
    return dict(split=split, per=per, rows=rows, iters=-(-per // rows), empty=sum(1 for b in range(split) if b * per >= M))


def stream_blocks(total):
    """bn_act.hip's stream_blocks: workgroups of a streaming kernel over `total` threads' worth of work, capped at 8192."""
    return int(min(max(-(-total // 256), 1), 8192))


def stream_wraps(M, C, width=4):
    """True when a streaming kernel with `width` channels per thread makes a second grid-stride pass."""
    total = M * (C // width)
    return total > stream_blocks(total) * 256


def pool_dims(H, W):
    return (H - 1) // 2 + 1, (W - 1) // 2 + 1


def pool_tiles(N, H, W):
    PH, PW = pool_dims(H, W)
    return N * (-(-PH // PT)) * (-(-PW // PT))


def pool_blocks(N, H, W):
    """workgroups of pool_bwd_kernel<1> (= its partials)"""
    return min(pool_tiles(N, H, W), BN_MAX_SPLIT)


def pool_tile_chain(N, H, W, C):
    """fp32 chain of a thread's sums in pool_bwd_kernel<1>: 4 PT^2 / rows pixels per tile, its tiles in turn (the three
    additions that gather a pixel's gradient from <= 4 windows are backward_ref's `extra_sum`)."""
    tiles, blocks = pool_tiles(N, H, W), pool_blocks(N, H, W)
    rows = 1024 // C
    return -(-tiles // blocks) * -(-(4 * PT * PT) // rows)


# ------------------------------------------------------------------------------------------ statistics
def exact_sums(x, chain_free_bits=24):
    """Per channel: True when EVERY fp32 partial sum of x and of x^2 is exact, proved from the data: all values of the
    channel lie on a grid 2^k (k = the lowest set bit over the channel), sum |x| < 2^24 grid units and sum x^2 < 2^24
    units of the grid squared.  Any sub-sum is then an integer below 2^24 in those units, hence representable."""
    x64 = x.double()
    C = x.shape[1]
    ok = torch.zeros(C, dtype=torch.bool, device=x.device)
    amax = x64.abs().amax(0)
    for k in range(-40, 12):
        g = 2.0 ** k
        on = ((x64 / g) == (x64 / g).round()).all(0)
        fits = (x64.abs().sum(0) / g < 2.0 ** chain_free_bits) & ((x64 * x64).sum(0) / (g * g) < 2.0 ** chain_free_bits)
        ok |= on & fits & (amax > 0)
    return ok | (amax == 0)


class Stats:
    """fp64 statistics of an fp32 x [M][C] and the bounds of the stored (mean, invstd), for thread sums that carry a
    chain of n fp32 operations (n a number or a [C] tensor; 0: fp64 partials, or fp32 sums proved exact by exact_sums).

    bn_partial_kernel<0>: a thread adds its rows in fp32 (s += x; ss = fmaf(x, x, ss): ONE rounding per step each), the
    thread rows and the workgroups' partials are summed in fp64.  With ne = n + U64N:
    Sums.  |S1' - S1| <= ne u sum|x|,  |S2' - S2| <= ne u sum x^2.
    mean.  fp64 S1' / M, rounded to fp32: d_mean = ne u mabs (arith; mabs = sum|x| / M), u |mean| (fmt).
    var.   var' = S2'/M - mean'^2 in fp64 (mean' BEFORE its rounding), clamped at 0 (the true variance is >= 0: the
           clamp only moves var' towards it): |var' - var| <= ne u S2/M + 2 |mean| d_mean + d_mean^2.
           With q = var + eps and cond = 1 + mean^2 / q:  S2/M = var + mean^2 <= cond q  and
           2 |mean| mabs <= 2 |mean| sqrt(S2/M) <= mean^2 + S2/M <= (2 cond - 1) q,  hence
           delta = |var' - var| / q <= 3 ne u cond + d_mean^2 / q.
           A constant channel whose sums are exact has var' = 0 EXACTLY (c^2 - c^2), whatever cond.
    invstd = q^-1/2.  |(1 + t)^-1/2 - 1| <= (|t| / 2) (1 - |t|)^-3/2 for |t| < 1, so r_inv = (delta / 2) (1 - delta)^-3/2
           relative (arith; infinite once delta >= 1), then the rounding to fp32, u (fmt).  eps enters as the fp32 the
           kernel is handed; var << eps (the 2^-10 channels) makes q ~ eps and cond ~ mean^2 / eps.
    A relative error of S2 reaches invstd multiplied by cond / 2: cond is what the E[x^2] - E[x]^2 form costs."""

    def __init__(self, x, eps, n):
        x64 = x.double()
        self.M, self.C = x.shape
        M = self.M
        self.eps = f32(eps)
        n = torch.as_tensor(n, dtype=torch.float64, device=x.device)
        ne = (n + U64N) * U32 * SLACK
        self.s1, self.s2, self.sabs = x64.sum(0), (x64 * x64).sum(0), x64.abs().sum(0)
        self.mean = self.s1 / M
        self.var = ((x64 - self.mean) ** 2).sum(0) / M          # two-pass: no cancellation in the reference
        q = self.var + self.eps
        self.invstd = q.rsqrt()
        self.cond = 1.0 + self.mean ** 2 / q
        self.b_s1 = Bound(torch.zeros_like(self.s1), ne * self.sabs)
        self.b_s2 = Bound(torch.zeros_like(self.s2), ne * self.s2)
        self.d_mean = ne * self.sabs / M
        self.b_mean = Bound(U32 * self.mean.abs(), self.d_mean)
        self.delta = 3.0 * ne * self.cond + self.d_mean ** 2 / q
        self.d_var = self.delta * q
        ok = self.delta < 1.0
        self.r_inv = torch.where(ok, 0.5 * self.delta * (1.0 - self.delta.clamp_max(0.999)) ** -1.5,
                                 torch.full_like(self.delta, float("inf")))
        self.b_invstd = Bound(U32 * self.invstd, self.r_inv * self.invstd)

    def running(self, rm0, rv0, momentum):
        """nn.BatchNorm2d's update with the UNBIASED variance (M / (M - 1); count == 1 keeps var), in the kernel's fp32
        arithmetic r' = fl(fl(fl(1 - m) r0) + fl(m fl(v))): against r = (1 - m) r0 + m v in fp64 (m the fp32 momentum)
        the roundings are 2u |(1 - m) r0| + 2u |m v| + u |r| (all fmt: once per channel), and the statistic's own error
        arrives multiplied by m: m d_mean, m k d_var with k = M / (M - 1) (arith)."""
        mom, M = f32(momentum), self.M
        k = M / (M - 1.0) if M > 1 else 1.0
        unb = self.var * k
        rm0, rv0 = rm0.double().to(self.mean.device), rv0.double().to(self.mean.device)
        rm = (1.0 - mom) * rm0 + mom * self.mean
        rv = (1.0 - mom) * rv0 + mom * unb
        f_rm = U32 * SLACK * (2 * ((1.0 - mom) * rm0).abs() + 2 * (mom * self.mean).abs() + rm.abs())
        f_rv = U32 * SLACK * (2 * ((1.0 - mom) * rv0).abs() + 2 * (mom * unb).abs() + rv.abs())
        return (rm, Bound(f_rm, mom * self.d_mean)), (rv, Bound(f_rv, mom * k * self.d_var))


def eval_stats(rm, rv, eps):
    """Eval mode: stats = (running_mean, rsqrtf(fl(running_var + eps))).  The mean is copied: exact.  The sum rounds once
    (u, reaching the result halved), rsqrtf errs by <= RSQRT_ULP ulps (<= 2u relative each), all of it fmt."""
    q = rv.double() + f32(eps)
    inv = q.rsqrt()
    return (rm.double(), Bound(torch.zeros_like(inv), torch.zeros_like(inv))), \
           (inv, Bound((0.5 + 2.0 * RSQRT_ULP) * U32 * SLACK * inv, torch.zeros_like(inv)))


# ------------------------------------------------------------------------------------------ forward
def preact_ref(x, mean, invstd, gamma, beta, res=None):
    """z = fmaf((x - mean) * invstd, gamma, beta) [+ res] in fp64 from the STORED statistics, and the bound of the fp32
    value before its ReLU.  Four roundings (three without a residual), all fmt:
        t1 = fl(x - mean)          u |x - mean|, reaching z multiplied by |invstd gamma|
        t2 = fl(t1 invstd)         u |xh|, multiplied by |gamma|
        w  = fmaf(t2, gamma, beta) u |w|   (none when gamma == 0: fmaf(t, 0, beta) = beta exactly)
        z  = fl(w + res)           u |z|
    -> |z' - z| <= (2u |xh gamma| + u |w| [+ u |z|]) SLACK."""
    x64 = x.double()
    g, b = gamma.double().to(x.device), beta.double().to(x.device)
    xh = (x64 - mean.double()) * invstd.double()
    w = xh * g + b
    bw = (2 * (xh * g).abs() + torch.where(g == 0, torch.zeros_like(w), w.abs())) * U32 * SLACK
    if res is None:
        return w, bw, xh
    z = w + res.double()
    return z, bw + U32 * SLACK * z.abs(), xh


def forward_ref(x, mean, invstd, gamma, beta, res=None, relu=True):
    """relu?(z) and its bound (ReLU is 1-Lipschitz, and a value whose sign the roundings flip is within the bound of 0);
    also z and its bound, for the sign-agreement check and the mask bytes."""
    z, bz, _ = preact_ref(x, mean, invstd, gamma, beta, res)
    ref = z.clamp_min(0.0) if relu else z
    return ref, Bound(bz, torch.zeros_like(bz)), z, bz


def mask_bits_of(y, width=4):
    """The mask bytes a forward must have written for its stored y [M][C]: one byte per float4, bit e = (y[4q + e] > 0).
    (The 8-channel kernels write two such bytes per thread: the same bytes in the same places.)"""
    M, C = y.shape
    bits = (y > 0).view(M, C // 4, 4).to(torch.uint8)
    wgt = torch.tensor([1, 2, 4, 8], dtype=torch.uint8, device=y.device)
    return (bits * wgt).sum(-1).to(torch.uint8).reshape(-1)


def mask_to_bool(mask, M, C):
    m = mask.view(M, C // 4, 1)
    sh = torch.tensor([0, 1, 2, 3], dtype=torch.uint8, device=mask.device)
    return ((m >> sh) & 1).bool().reshape(M, C)


# ------------------------------------------------------------------------------------------ backward
def backward_ref(x, dy, mean, invstd, gamma, n, keep_mask=None, keep=None, hw=1, slope=0.0, given=None,
                 d_abs=None, extra_sum=0, extra_dx=0, count=None):
    """d = dy [mask], dbeta = sum d, dgamma = sum d xh, dx = g invstd (d - dbeta/M - xh dgamma/M) [* keep (x > 0 ? 1 : slope)]
    in fp64 from the stored statistics, with their bounds for thread sums behind a chain of n fp32 operations.

    keep_mask: the ReLU decision [M][C] (bool) taken from the kernel's forward; None: no ReLU.
    given = (dgamma', dbeta') as the kernel was handed them (dmc_bn_act_bwd_x3s_apply): dx is then referenced from those.
    d_abs / extra_sum / extra_dx: the pool's d is itself a sum of <= 4 pooled gradients (3 fp32 additions over d_abs = sum |.|)
    where the kernel gathers it: in the tile pass' sums (extra_sum) and in every dx pass (extra_dx).  The streaming pass adds
    the windows' gradients one by one, so the sums' bounds run over d_abs: two windows that share an arg-max pixel may cancel.
    count: the divisor of the means when it is not the number of rows of x (pool: the input map's pixels).

    xh' = fl(fl(x - mean) invstd): |xh' - xh| <= 2u |xh|.
    dbeta.   s += d: the first addition (to 0) is exact, n - 1 round: (n - 1) u sum d_abs [+ extra_sum u sum d_abs] (arith;
             d_abs = |d| outside the pool), u |dbeta| (fmt).
    dgamma.  ss = fmaf(d, xh', ss): every term passes three roundings of its own, xh''s two and its fmaf's (with n = 1 that
             is all there is, and a one-term sum attains them): 3 u sum d_abs |xh| and u |dgamma| (fmt); the n - 1 further
             steps of the chain add (n - 1) u sum d_abs |xh| (arith).
    dx.      r = fl(fl(g invstd) fl(fl(d - fl(db' ic)) - fl(fl(xh' dg') ic))), ic = fl(1 / M).  Roundings behind each of the
             three addends d, MB = dbeta/M, xh MG = xh dgamma/M (fmt, times |SC| = |g invstd|):
                 d      the two differences, the last product, SC's own product                      4u
                 MB     db's stored rounding, ic, their product, and the four above                   7u
                 xh MG  xh''s two, dg's stored rounding, ic, two products, the second difference,
                        the last product, SC's                                                        9u
             and the sums' errors: |SC| (e_dbeta + |xh| e_dgamma) / M (arith), |SC| |xh| 3 u sum d_abs |xh| / M (fmt).
             The keep / slope tail multiplies by fl(k s) and rounds twice more: 2u |dx| (fmt)."""
    x64, d = x.double(), dy.double()
    if keep_mask is not None:
        d = d * keep_mask
    if d_abs is None:
        d_abs = d.abs()
    M = x.shape[0] if count is None else count
    g = gamma.double().to(x.device)
    mean, invstd = mean.double(), invstd.double()
    SC = g * invstd
    xh = (x64 - mean) * invstd
    SB, SG = d.sum(0), (d * xh).sum(0)
    nu = (torch.as_tensor(n, dtype=torch.float64, device=x.device) - 1.0).clamp_min(0.0) * U32 * SLACK
    sum_d, sum_dx = d_abs.sum(0), (d_abs * xh.abs()).sum(0)
    e_sb = (nu + extra_sum * U32 * SLACK) * sum_d + U64N * U32 * SB.abs()                # arith of dbeta
    e_sg = (nu + extra_sum * U32 * SLACK) * sum_dx + U64N * U32 * SG.abs()               # arith of dgamma
    f_sg = 3 * U32 * SLACK * sum_dx                                                       # each term's own three roundings
    if given is not None:
        SGu, SBu = given[0].double(), given[1].double()
        a_sb = a_sg = f_g = torch.zeros_like(SB)
    else:
        SGu, SBu, a_sb, a_sg, f_g = SG, SB, e_sb, e_sg, f_sg
    MB, MG = SBu / M, SGu / M
    dx = SC * (d - MB - xh * MG)
    fmt = SC.abs() * ((4 * d.abs() + extra_dx * d_abs + 7 * MB.abs() + 9 * (xh * MG).abs()) * U32 * SLACK + xh.abs() * f_g / M)
    arith = SC.abs() * (a_sb + xh.abs() * a_sg) / M * SLACK
    if slope != 0.0:
        k = torch.ones_like(dx) if keep is None else keep.double().repeat_interleave(hw, dim=0)[:x.shape[0]]
        f = k * torch.where(x > 0, torch.ones_like(dx), torch.full_like(dx, f32(slope)))
        dx, fmt, arith = dx * f, (fmt + 2 * U32 * SLACK * dx.abs()) * f.abs(), arith * f.abs()
    return dict(dx=(dx, Bound(fmt, arith)), dgamma=(SG, Bound(U32 * SG.abs() + f_sg, e_sg)), dbeta=(SB, Bound(U32 * SB.abs(), e_sb)), d=d)


def act_mask_ref(z, dz, keep, hw, slope):
    """act_mask_bwd_kernel (gamma == NULL): dx = fl(dz fl(keep (z > 0 ? 1 : slope))): two roundings."""
    k = torch.ones_like(z, dtype=torch.float64) if keep is None else keep.double().repeat_interleave(hw, dim=0)[:z.shape[0]]
    f = k * torch.where(z > 0, torch.ones_like(k), torch.full_like(k, f32(slope)))
    ref = dz.double() * f
    return ref, Bound(2 * U32 * SLACK * ref.abs(), torch.zeros_like(ref))


# ------------------------------------------------------------------------------------------ the stem tail: bn -> relu -> maxpool(3, 2, 1)
def _window_index(H, W, device):
    PH, PW = pool_dims(H, W)
    k = torch.arange(9, device=device)
    iy = 2 * torch.arange(PH, device=device)[None, :] + (k // 3)[:, None] - 1           # [9][PH]
    ix = 2 * torch.arange(PW, device=device)[None, :] + (k % 3)[:, None] - 1            # [9][PW]
    return iy, ix, (iy >= 0) & (iy < H), (ix >= 0) & (ix < W)


def pool_ref(x, mean, invstd, gamma, beta):
    """x [N][H][W][C] fp32.  fp64 relu(bn(x)) per 3x3 window (stride 2, padding 1) with PyTorch's rule: row-major scan of the
    in-bounds positions, strictly greater wins (ties go to the first).

    The kernel's value at a position, v' = max(z', 0) with |z' - z| <= bz (preact_ref, three roundings), is a function of
    (x, channel) alone: positions of a window with the SAME raw x are tied bit for bit in the kernel as in the reference,
    and so are all positions of a gamma == 0 channel (z' = beta exactly, bz = 0).  A window is DECIDED when either
      (a) every in-bounds z_k <= -bz_k (so z'_k <= 0): all values are 0 and the first in-bounds position is taken, or
      (b) the best z is > its bz (so it survives the ReLU), and every in-bounds position that is not tied with it lies
          below it by more than the two bounds together.
    In a decided window the expected code is the first in-bounds position of the tie set, xmax the raw x there (exact),
    the pooled value relu(z_best) within bz_best.  Returns a dict; `undecided` is the share of (window, channel) pairs."""
    N, H, W, C = x.shape
    PH, PW = pool_dims(H, W)
    z, bz, xh = preact_ref(x.reshape(-1, C), mean, invstd, gamma, beta)
    z, bz = z.view(N, H, W, C), bz.view(N, H, W, C)
    iy, ix, oky, okx = _window_index(H, W, x.device)
    iyc, ixc = iy.clamp(0, H - 1), ix.clamp(0, W - 1)
    gat = lambda t: torch.stack([t[:, iyc[k]][:, :, ixc[k]] for k in range(9)])          # [9][N][PH][PW][C]
    zw, bw, xw = gat(z), gat(bz), gat(x)
    inb = (oky[:, None, :, None, None] & okx[:, None, None, :, None]).expand(9, N, PH, PW, C)
    neg = torch.full_like(zw, -float("inf"))
    zin = torch.where(inb, zw, neg)
    best, kbest = zin.max(0)                                                             # (any position of the maximum)
    pick = lambda t: torch.gather(t, 0, kbest[None])[0]
    bbest, xbest = pick(bw), pick(xw)
    tied = inb & ((xw == xbest[None]) | ((bw == 0) & (bbest[None] == 0) & (zw == best[None])))
    case_a = (~inb | (zw <= -bw)).all(0)
    case_b = (best > bbest) & (~inb | tied | (best[None] - zw > bbest[None] + bw)).all(0)
    first_in = inb.to(torch.uint8).argmax(0)
    first_tied = tied.to(torch.uint8).argmax(0)
    code = torch.where(case_a, first_in, first_tied)
    decided = case_a | case_b
    xmax = torch.gather(xw, 0, code[None])[0]
    ypool = torch.where(case_a, torch.zeros_like(best), best.clamp_min(0.0))
    return dict(y=ypool, b_y=Bound(torch.where(case_a, torch.zeros_like(bbest), bbest), torch.zeros_like(bbest)),
                code=code.to(torch.uint8), xmax=xmax, decided=decided, undecided=float((~decided).double().mean()),
                n_undecided=int((~decided).sum()), windows=decided.numel())


def pool_backward_ref(x, dpool, codes, mean, invstd, gamma, beta, n, extra_sum):
    """The stem tail's backward through the kernel's `codes` [N][PH][PW][C] (uint8 positions 0..8): every window's pooled
    gradient goes to its arg-max pixel, d = (sum of the <= 4 arriving gradients) [z > 0], then the BatchNorm backward over
    the N H W input pixels.  One reference, two chains: n = geometry(MP, C)['iters'], extra_sum = 0 for the streaming pass
    of dmc_bn_relu_pool_bwd_arg over (d_pool, xmax) -- sum over windows = sum over pixels, each window counted at its
    arg-max -- and n = pool_tile_chain(), extra_sum = 3 for dmc_bn_relu_pool_bwd's tile pass, which gathers first.
    `undecided_relu`: pixels that receive a gradient while |z| <= bz (their ReLU decision is not the reference's to make)."""
    N, H, W, C = x.shape
    PH, PW = pool_dims(H, W)
    dev = x.device
    k = codes.long()
    py = torch.arange(PH, device=dev)[None, :, None, None]
    px = torch.arange(PW, device=dev)[None, None, :, None]
    iy, ix = 2 * py + k // 3 - 1, 2 * px + k % 3 - 1
    assert bool(((iy >= 0) & (iy < H) & (ix >= 0) & (ix < W)).all()), "a code points outside the map"
    nn = torch.arange(N, device=dev)[:, None, None, None]
    cc = torch.arange(C, device=dev)[None, None, None, :]
    flat = (((nn * H + iy) * W + ix) * C + cc).reshape(-1)
    d = torch.zeros(N * H * W * C, dtype=torch.float64, device=dev).index_add_(0, flat, dpool.double().reshape(-1))
    dab = torch.zeros_like(d).index_add_(0, flat, dpool.double().abs().reshape(-1))
    x2 = x.reshape(-1, C)
    z, bz, _ = preact_ref(x2, mean, invstd, gamma, beta)
    got_grad = dab.view(-1, C) > 0
    out = backward_ref(x2, d.view(-1, C), mean, invstd, gamma, n, keep_mask=(z > 0), d_abs=dab.view(-1, C) * (z > 0), extra_sum=extra_sum, extra_dx=3)
    out["undecided_relu"] = int((got_grad & (z.abs() <= bz) & (bz > 0)).sum())      # (bz == 0: z' = z exactly)
    return out


# ------------------------------------------------------------------------------------------ test data
#: per-channel regimes, channel c takes REGIMES[c % 16]: (mean / std, log2 scale, gamma sign (0: gamma == 0), beta, constant)
REGIMES = [(0.0, 0, 1, None, False), (0.0, 0, 1, None, True), (0.5, 0, 0, None, False), (8.0, 0, -1, None, False),
           (-8.0, 0, 1, None, False), (64.0, 0, 1, None, False), (-64.0, 0, -1, None, False), (128.0, 0, 1, None, False),
           (0.0, -10, 1, None, False), (0.0, 10, -1, None, False), (0.0, 0, 1, 12.0, False), (0.0, 0, 1, -12.0, False),
           (0.0, 0, -1, None, False), (8.0, 10, 1, None, False), (0.5, 0, 1, None, False), (-64.0, -10, 1, None, False)]
CONST_VALUE = 0.75                                              # the constant channel: M c and M c^2 are exact for M < 2^20


def bn2d_case(shape, C=None, seed=0, kind="normal"):
    """Operands of one shape, (N, C, H, W) or M with C: x, res, dy [M][C] fp32, gamma, beta, rm, rv [C], hw, regimes.

    kind="normal": continuous data; channel c is in regime REGIMES[c % 16]: mean / std of 0, +-8, +-64, 128 (cond up to
    ~2 10^4), scales 2^-10 (var << eps) and 2^10, one exactly constant channel (exact sums: var' = 0, invstd = eps^-1/2,
    y = beta exactly), both signs of gamma, gamma == 0, a beta that lets the ReLU pass everything and one that passes nothing.
    kind="dyadic": x = (round(4 N(0,1)) / 4 + offset) scale with offsets {0, 0, 4, -8, 16}[c % 5] and scales {1, 1, 1/8, 8}[c % 4]
    (exact partial sums where exact_sums() proves it, many ties inside pool windows), |gamma| >= 1/4 on a 1/4 grid or exactly 0,
    every third gamma negative; the constant, gamma == 0 and the two beta channels as above.
    kind="plain": N(0, 1) in every channel, gamma in (0.5, 1.5): what the suite's older tests present (for the old metric)."""
    if isinstance(shape, tuple):
        N, C, H, W = shape
        M, hw = N * H * W, H * W
    else:
        M, hw = int(shape), 1
    r = np.random.RandomState(seed)
    cidx = np.arange(C)
    reg = [REGIMES[c % 16] for c in cidx]
    x = r.standard_normal((M, C)).astype(np.float32)
    gamma = r.uniform(0.5, 1.5, C)
    beta = r.uniform(-0.5, 0.5, C)
    if kind == "plain":                                         # the old suite's data: N(0, 1) in every channel
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))
        return dict(x=t(x), res=t(r.standard_normal((M, C))), dy=t(r.standard_normal((M, C))), gamma=t(gamma), beta=t(beta),
                    rm=t(r.uniform(-1.0, 1.0, C)), rv=t(r.uniform(0.5, 2.0, C)), hw=hw, M=M, C=C)
    if kind == "dyadic":
        off = np.array([0.0, 0.0, 4.0, -8.0, 16.0])[cidx % 5]
        sc = np.array([1.0, 1.0, 0.125, 8.0])[cidx % 4]
        x = ((np.round(x * 4) / 4 + off.astype(np.float32)) * sc.astype(np.float32)).astype(np.float32)
        gamma = np.maximum(np.round(gamma * 4) / 4, 0.25)
        gamma[::3] *= -1
        beta = np.round(beta * 4) / 4
        for c in cidx:
            if reg[c][2] == 0:
                gamma[c] = 0.0
    else:
        sc = np.array([2.0 ** g[1] for g in reg])
        off = np.array([g[0] for g in reg]) * sc
        x = (x * sc.astype(np.float32) + off.astype(np.float32)).astype(np.float32)
        gamma = gamma * np.array([float(g[2]) for g in reg])
    for c in cidx:
        if reg[c][4]:
            x[:, c] = CONST_VALUE
        if reg[c][3] is not None:
            beta[c] = reg[c][3]                                 # |gamma xh| < 1.5 x 6: the ReLU passes all / nothing
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))
    return dict(x=t(x), res=t(r.standard_normal((M, C))), dy=t(r.standard_normal((M, C))), gamma=t(gamma), beta=t(beta),
                rm=t(r.uniform(-1.0, 1.0, C)), rv=t(r.uniform(0.5, 2.0, C)), hw=hw, M=M, C=C)


def chain_of(x, M, C, split=None):
    """Per-channel chain length of bn_partial_kernel<0>'s sums over x: 0 where exact_sums proves them exact."""
    it = geometry(M, C, split)["iters"]
    return torch.where(exact_sums(x), torch.zeros(C, dtype=torch.float64, device=x.device),
                       torch.full((C,), float(it), dtype=torch.float64, device=x.device))


def make_partials64(x, nblk, layout="conv"):
    """fp64 (sum, sum of squares) partials as a test hands them to dmc_conv_nhwc_stats_final ([nblk][C][2]) or, layout="bn",
    to the stat_split of dmc_bn_relu_pool_fwd_arg ([C][1024][2]): rows dealt to the nblk blocks in contiguous runs."""
    M, C = x.shape
    per = -(-M // nblk)
    x64 = torch.zeros((nblk * per, C), dtype=torch.float64, device=x.device)
    x64[:M] = x.double()
    x64 = x64.view(nblk, per, C)
    part = torch.stack((x64.sum(1), (x64 * x64).sum(1)), dim=2)                          # [nblk][C][2]
    if layout == "conv":
        return part.contiguous()
    out = torch.full((C, BN_MAX_SPLIT, 2), float("nan"), dtype=torch.float64, device=x.device)
    out[:, :nblk] = part.permute(1, 0, 2)
    return out.contiguous()


# ------------------------------------------------------------------------------------------ fp32 emulation (numpy)
F32 = np.float32


def _fma(a, b, c):
    """fmaf as one rounding: the fp32 product is exact in fp64; the fp64 sum rounds at 2^-53 before the fp32 rounding
    (a double rounding that can move an exact tie only)."""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(F32)


def emu_partials(t0, t1a, t1b, M, C, split, empty_fill=0.0):
    """bn_partial_kernel's sums: s0 += t0, s1 = fmaf(t1a, t1b, s1) per thread over its rows r0 + ty, + rows, ... in fp32,
    then the thread rows in fp64 -> [split][C] pairs.  Workgroups with an empty range write zeros (empty_fill: what a
    defective kernel would leave there)."""
    geo = geometry(M, C, split)
    per, rows, iters = geo["per"], geo["rows"], geo["iters"]
    k, b, ty = np.meshgrid(np.arange(iters), np.arange(split), np.arange(rows), indexing="ij")
    local = k * rows + ty
    r = b * per + local
    ok = (local < per) & (r < M)
    rc = np.where(ok, r, 0)
    s0 = np.zeros((split, rows, C), dtype=F32)
    s1 = np.zeros((split, rows, C), dtype=F32)
    for i in range(iters):
        m = ok[i][..., None]
        s0 = s0 + np.where(m, t0[rc[i]], F32(0))
        s1 = _fma(np.where(m, t1a[rc[i]], F32(0)), np.where(m, t1b[rc[i]], F32(0)), s1)
    p0, p1 = s0.astype(np.float64).sum(1), s1.astype(np.float64).sum(1)
    if empty_fill != 0.0:
        dead = np.arange(split) * per >= M
        p0[dead], p1[dead] = empty_fill, empty_fill
    return p0, p1


def emu_stats_final(p0, p1, M, rm0, rv0, eps, momentum, defect=None):
    """bn_stats_final_kernel / conv_stats_final_kernel from fp64 partials [blocks][C]: fp64 mean, var, invstd; fp32 momentum
    arithmetic.  defect: 'biased', 'tail_partial' (the last partial dropped when blocks % 32 != 0), 'mean32_sq' (mean rounded
    to fp32 before it is squared)."""
    if defect == "tail_partial" and p0.shape[0] % 32 != 0:
        p0, p1 = p0[:-1], p1[:-1]
    s, ss = p0.sum(0), p1.sum(0)
    mean = s / M
    msq = mean.astype(F32).astype(np.float64) ** 2 if defect == "mean32_sq" else mean * mean
    var = np.maximum(ss / M - msq, 0.0)
    e, mom = F32(eps), F32(momentum)
    with np.errstate(all="ignore"):
        inv32 = (1.0 / np.sqrt(var + np.float64(e))).astype(F32)
        unb = var if (defect == "biased" or M == 1) else var * M / (M - 1)
        rm = (F32(1) - mom) * rm0 + mom * mean.astype(F32)
        rv = (F32(1) - mom) * rv0 + mom * unb.astype(F32)
    return dict(mean=mean.astype(F32), invstd=inv32, rm=rm.astype(F32), rv=rv.astype(F32))


def emu_apply_fwd(x, mean, inv, gamma, beta, res, relu, defect=None):
    """bn_apply_fwd_kernel: y and the mask bytes.  defect: 'mask_reversed' (bits 3..0 instead of 0..3 of each float4)."""
    v = _fma((x - mean) * inv, np.broadcast_to(gamma, x.shape), np.broadcast_to(beta, x.shape))
    if res is not None:
        v = v + res
    mask = None
    if relu:
        M, C = x.shape
        bits = (v > 0).reshape(M, C // 4, 4)
        w = np.array([8, 4, 2, 1] if defect == "mask_reversed" else [1, 2, 4, 8], dtype=np.uint8)
        mask = (bits * w).sum(-1).astype(np.uint8).reshape(-1)
        v = np.maximum(v, F32(0))
    return v.astype(F32), mask


def emu_backward(x, dy, mean, inv, gamma, beta, res, relu, mask, keep=None, hw=1, slope=0.0, defect=None, split=None):
    """bn_partial_kernel<1> + bn_bwd_final_kernel + bn_apply_bwd_kernel.  mask: the forward's bytes (or None: the sign is
    recomputed from x [+ res]).  defect: 'relu_no_res' (recomputed without the residual), 'swap' (dgamma and dbeta exchanged),
    'keep_row' (keep indexed by row instead of frame), 'empty_uninit' (NaN left in the empty workgroups' partials)."""
    M, C = x.shape
    split = split_of(M, C) if split is None else split
    xh = (x - mean) * inv
    d = dy
    if relu:
        if mask is not None:
            keepm = ((mask.reshape(M, C // 4, 1) >> np.arange(4, dtype=np.uint8)) & 1).astype(bool).reshape(M, C)
        else:
            v = _fma(xh, np.broadcast_to(gamma, x.shape), np.broadcast_to(beta, x.shape))
            if res is not None and defect != "relu_no_res":
                v = v + res
            keepm = v > 0
        d = np.where(keepm, dy, F32(0))
    p0, p1 = emu_partials(d, d, xh, M, C, split, empty_fill=float("nan") if defect == "empty_uninit" else 0.0)
    db, dg = p0.sum(0).astype(F32), p1.sum(0).astype(F32)
    if defect == "swap":
        db, dg = dg, db
    ic = F32(1) / F32(M)
    with np.errstate(all="ignore"):
        r = gamma * inv * (d - db * ic - xh * dg * ic)
        if slope != 0.0:
            if keep is None:
                k = np.ones_like(x)
            elif defect == "keep_row":
                k = keep[np.arange(M) % keep.shape[0]]
            else:
                k = keep[np.arange(M) // hw]
            r = r * (k * np.where(x > 0, F32(1), F32(slope)))
    return dict(dx=r.astype(F32), dgamma=dg, dbeta=db, dres=d.astype(F32))


def emu_pool_fwd(x, mean, inv, gamma, beta, defect=None):
    """pool_fwd_x3s_kernel with the arg-max record: x [N][H][W][C] -> pooled y, codes (uint8), xmax.
    defect: 'tie_last' (>= instead of >), 'clamped_wins' (the in-bounds test dropped: a clamped copy scanned earlier wins)."""
    N, H, W, C = x.shape
    PH, PW = pool_dims(H, W)
    v = np.maximum(_fma((x - mean) * inv, np.broadcast_to(gamma, x.shape), np.broadcast_to(beta, x.shape)), F32(0))
    mx = np.full((N, PH, PW, C), -np.inf, dtype=F32)
    bx = np.zeros((N, PH, PW, C), dtype=F32)
    ck = np.zeros((N, PH, PW, C), dtype=np.uint8)
    for k in range(9):
        iy, ix = 2 * np.arange(PH) + k // 3 - 1, 2 * np.arange(PW) + k % 3 - 1
        inb = ((iy >= 0) & (iy < H))[:, None] & ((ix >= 0) & (ix < W))[None, :]
        if defect == "clamped_wins":
            inb = np.ones_like(inb)
        iyc, ixc = np.clip(iy, 0, H - 1), np.clip(ix, 0, W - 1)
        vk, xk = v[:, iyc][:, :, ixc], x[:, iyc][:, :, ixc]
        take = inb[None, :, :, None] & ((vk >= mx) if defect == "tie_last" else (vk > mx))
        mx, bx, ck = np.where(take, vk, mx), np.where(take, xk, bx), np.where(take, np.uint8(k), ck)
    return dict(y=mx, code=ck, xmax=bx)


def _emu_pool_gather(x, dpool, code, mean, inv, gamma, beta):
    """Step B of pool_bwd_kernel: per input pixel the gradients of its <= 4 windows whose code names it, added in (py, px) order in
    fp32, then the ReLU sign recomputed from x.  Returns (d, xh)."""
    N, H, W, C = x.shape
    PH, PW = pool_dims(H, W)
    d = np.zeros((N, H, W, C), dtype=F32)
    iyp, ixp = np.arange(H), np.arange(W)
    for jy in (0, 1):
        for jx in (0, 1):
            py, px = iyp // 2 + jy, ixp // 2 + jx
            oky, okx = (jy < 1 + (iyp & 1)) & (py < PH), (jx < 1 + (ixp & 1)) & (px < PW)
            pyc, pxc = np.where(oky, py, 0), np.where(okx, px, 0)
            kk = ((iyp - 2 * py + 1) * 3)[:, None] + (ixp - 2 * px + 1)[None, :]
            hit = (oky[:, None] & okx[None, :])[None, :, :, None] & (code[:, pyc][:, :, pxc] == kk[None, :, :, None])
            d = d + np.where(hit, dpool[:, pyc][:, :, pxc], F32(0))
    xh = (x - mean) * inv
    v = _fma(xh, np.broadcast_to(gamma, x.shape), np.broadcast_to(beta, x.shape))
    return np.where(v > 0, d, F32(0)), xh


def emu_pool_bwd_arg(x, dpool, code, xmax, mean, inv, gamma, beta, defect=None):
    """dmc_bn_relu_pool_bwd_arg: pass 1 = bn_partial_kernel<1> over (d_pool, xmax) with the ReLU sign recomputed, pass 2 =
    pool_bwd_kernel<2> through the recorded codes.  defect: 'inv_count_pooled' (1 / (N PH PW) instead of 1 / (N H W))."""
    N, H, W, C = x.shape
    PH, PW = pool_dims(H, W)
    MP = N * PH * PW
    e = emu_backward(xmax.reshape(MP, C), dpool.reshape(MP, C), mean, inv, gamma, beta, None, 1, None)
    dg, db = e["dgamma"], e["dbeta"]
    d, xh = _emu_pool_gather(x, dpool, code, mean, inv, gamma, beta)
    ic = F32(1) / F32(MP if defect == "inv_count_pooled" else N * H * W)
    dx = gamma * inv * (d - db * ic - xh * dg * ic)
    return dict(dx=dx.astype(F32), dgamma=dg, dbeta=db)


def emu_pool_bwd_tile(x, dpool, code, mean, inv, gamma, beta):
    """dmc_bn_relu_pool_bwd: pass 1 = pool_bwd_kernel<1>, a thread's fp32 sums over its pixels pi = ty, ty + rows, ... of a
    16 x 16-pixel tile and over the workgroup's tiles b, b + blocks, ...; thread rows and workgroups in fp64.  (The codes the
    kernel recomputes are those of the forward: the same arithmetic on the same values.)"""
    N, H, W, C = x.shape
    PH, PW = pool_dims(H, W)
    d, xh = _emu_pool_gather(x, dpool, code, mean, inv, gamma, beta)
    tiles_y, tiles_x, blocks, rows = -(-PH // PT), -(-PW // PT), pool_blocks(N, H, W), 1024 // C
    n_, iy, ix = np.meshgrid(np.arange(N), np.arange(H), np.arange(W), indexing="ij")
    tile = (n_ * tiles_y + iy // (2 * PT)) * tiles_x + ix // (2 * PT)
    pi = (iy % (2 * PT)) * (2 * PT) + ix % (2 * PT)
    blk, ty = tile % blocks, pi % rows
    seq = (tile // blocks) * (-(-(4 * PT * PT) // rows)) + pi // rows
    s0 = np.zeros((blocks, rows, C), dtype=F32)
    s1 = np.zeros((blocks, rows, C), dtype=F32)
    for k in np.unique(seq):
        m = seq == k                                           # each (workgroup, thread row) at most once per step
        s0[blk[m], ty[m]] = s0[blk[m], ty[m]] + d[m]
        s1[blk[m], ty[m]] = _fma(d[m], xh[m], s1[blk[m], ty[m]])
    db = s0.astype(np.float64).sum((0, 1)).astype(F32)
    dg = s1.astype(np.float64).sum((0, 1)).astype(F32)
    ic = F32(1) / F32(N * H * W)
    dx = gamma * inv * (d - db * ic - xh * dg * ic)
    return dict(dx=dx.astype(F32), dgamma=dg, dbeta=db)


# ------------------------------------------------------------------------------------------ the shapes of the GPU file
#: (N, C, H, W): M, split, thread iterations -- what each reaches is in test_bn2d_fp64_gpu.py's table
BN_SHAPES = [(1, 4, 1, 1), (2, 16, 5, 7), (1, 1024, 3, 3), (5, 512, 7, 7), (977, 64, 1, 1), (3, 256, 37, 61), (4, 64, 56, 56),
             (32717, 64, 1, 1), (32769, 64, 1, 1), (32996, 64, 1, 1), (131004, 64, 1, 1),       # split 255, 256, 257, 1023
             (3, 64, 210, 210), (6, 512, 53, 53), (6, 64, 210, 210)]
POOL_SHAPES = [(2, 64, 17, 23), (1, 64, 1, 5), (2, 64, 30, 31), (2, 128, 8, 8), (3, 64, 112, 112), (1, 16, 2, 2), (2, 64, 129, 127)]


def rows_of(shape):
    return shape[0] * shape[2] * shape[3]


# ------------------------------------------------------------------------------------------ one unit, judged
def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and bool((a.contiguous().view(torch.uint8) == b.contiguous().view(torch.uint8)).all())


def flag(ok):
    """An exact condition as a ratio: 0 passes, inf fails."""
    return 0.0 if ok else float("inf")


def unit_ratios(case, got, res, relu, n_stats=None, headroom=1.0, keep=None, slope=0.0, eps=1e-5, momentum=0.1, training=True,
                n_bwd=None, given=None):
    """error / bound of everything one conv -> bn [-> add] [-> relu] unit wrote (tensors on one device).  got: mean, invstd
    and whatever else there is of rm, rv, y, mask, dx, dgamma, dbeta, dres.  n_stats None: the statistics are not judged
    (they were given).  The backward's ReLU decision: the mask bytes if there are any, else y > 0."""
    x, C, M = case["x"], case["C"], case["M"]
    mean, inv = got["mean"], got["invstd"]
    new = {}
    if n_stats is not None and training:
        st = Stats(x, eps, n_stats)
        new.update(mean=ratio(mean, st.mean, st.b_mean, headroom), invstd=ratio(inv, st.invstd, st.b_invstd, headroom))
        new["cond"] = float(st.cond.max())
        if "rm" in got:
            (rm, b_rm), (rv, b_rv) = st.running(case["rm"], case["rv"], momentum)
            new.update(rm=ratio(got["rm"], rm, b_rm, headroom), rv=ratio(got["rv"], rv, b_rv, headroom))
    elif not training:
        (rm, b_rm), (iv, b_iv) = eval_stats(case["rm"], case["rv"], eps)
        new.update(mean=flag(same_bits(mean, case["rm"])), invstd=ratio(inv, iv, b_iv, headroom))
        new.update(rm=flag(same_bits(got["rm"], case["rm"])), rv=flag(same_bits(got["rv"], case["rv"])))
    if not (bool(torch.isfinite(mean).all()) and bool(torch.isfinite(inv).all())):
        return new
    r = case["res"] if res else None
    keep_mask = None
    if "y" in got:
        ref, b, z, bz = forward_ref(x, mean, inv, case["gamma"], case["beta"], r, relu)
        y = got["y"]
        new["y"] = ratio(y, ref, b, headroom)
        if relu:
            new["sign"] = flag(bool(((y > 0) == (z > 0))[z.abs() > bz].all()))
            keep_mask = y > 0
    if relu and got.get("mask") is not None:
        if "y" in got:
            new["mask"] = flag(torch.equal(got["mask"], mask_bits_of(got["y"])))
        keep_mask = mask_to_bool(got["mask"], M, C)
    if "dgamma" in got:
        n_bwd = geometry(M, C)["iters"] if n_bwd is None else n_bwd
        back = backward_ref(x, case["dy"], mean, inv, case["gamma"], n_bwd, keep_mask=keep_mask, keep=keep, hw=case["hw"],
                            slope=slope, given=given)
        for k in ("dx", "dgamma", "dbeta"):
            if got.get(k) is not None and not (given is not None and k != "dx"):
                new[k] = ratio(got[k], back[k][0], back[k][1], headroom)
        if got.get("dx") is not None:
            new["dx_arith"] = excess(got["dx"], *back["dx"])
        if got.get("dres") is not None:
            new["dres"] = flag(torch.equal(got["dres"].double(), back["d"]))
    return new
