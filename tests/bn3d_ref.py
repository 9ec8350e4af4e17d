"""fp64 references, derived error bounds and an fp32 emulation for the training-mode BatchNorm3d (+ ReLU) of the I3D
trunk's conv -> BatchNorm3d -> ReLU unit (csrc/bn3d_bf16.hip, the statistics epilogues of csrc/conv3d_bf16.hip).

Everything works on 2-D [M pixels][C channels] views of the NDHWC tensors.  The references take the kernel's own
bf16 tensors (y, dout, the kernel's `out` for the ReLU mask), so a stage is compared on the operands it really had.

Notation of the derivations: u = 2^-24 is the unit roundoff of fp32 (one rounded operation: |fl(a op b) - (a op b)|
<= u |a op b|), 2^-8 |v| the largest distance from v to the nearest bf16 (8 significant bits).  A chain of n rounded
fp32 additions of the terms t_i errs by at most ((1 + u)^n - 1) sum |t_i| <= n u SLACK sum |t_i|; SLACK = 1 + 2^-10
covers every second-order product of the small quantities below (n u <= 2^-13 for the chains here; the conditioning
term is kept exact where it can grow).  The fp64 parts of the kernels (n 2^-53) are below SLACK's reach as well.

A bound has two parts (class Bound):
    fmt    the one rounding with which the stored value enters its format (u |ref| of an fp32 result, 2^-8 |ref| of a
           bf16 one).  The format attains it whatever the arithmetic before it, so it has no headroom to give.
    arith  everything accumulated before that rounding.  ratio(..., headroom=h) divides this part by h.
"""
import numpy as np
import torch

U32 = 2.0 ** -24
UBF = 2.0 ** -8
SLACK = 1.0 + 2.0 ** -10

#: accumulator rows a lane adds (<= 4: the patch-resident kernel's TM), the 5 steps of the 32-lane tree (c3d_sum32),
#: the waves of a tile summed through LDS (<= 4: the 256 x 128 tile) -- the longest chain over all tile configurations
CONV_STAT_CHAIN = 4 + 5 + 4
#: partial rows made by a test: one fp64 sum per block of PART_BLOCK pixels, rounded to fp32 once
PART_BLOCK = 128
TEST_PART_CHAIN = 1


class Bound:
    def __init__(self, fmt, arith):
        self.fmt, self.arith = fmt, arith

    def total(self, headroom=1.0):
        return self.fmt + self.arith / headroom


def ratio(got, ref, bound, headroom=1.0):
    """Largest |got - ref| / bound over the elements: <= 1 passes.  An element that is not finite, or that differs
    where the bound is zero, counts as infinitely far."""
    got, ref = torch.as_tensor(got).double(), torch.as_tensor(ref).double().to(torch.as_tensor(got).device)
    lim = bound.total(headroom).to(got.device).expand_as(ref)
    err = (got - ref).abs()
    r = torch.where(err <= lim, err / lim.clamp_min(1e-300), torch.full_like(err, float("inf")))
    r = torch.where(err == 0, torch.zeros_like(r), r)        # (0 / 0: an exact value under a zero bound)
    return float(r.max())


def excess(got, ref, bound):
    """Largest share of the arith part that an element uses once its fmt part is spent: (|got - ref| - fmt)+ / arith.  Where fmt
    dominates (every bf16 output) ratio() sits near 1 by construction and this is the figure that shows the headroom."""
    got, ref = torch.as_tensor(got).double(), torch.as_tensor(ref).double().to(torch.as_tensor(got).device)
    over = ((got - ref).abs() - bound.fmt.to(got.device)).clamp_min(0.0)
    r = torch.where(over > 0, over / bound.arith.to(got.device).expand_as(over).clamp_min(1e-300), torch.zeros_like(over))
    return float(torch.nan_to_num(r, nan=float("inf")).max())


def f32(v):
    """The double that the kernel sees for a float argument (eps, momentum)."""
    return float(np.float32(v))


# ------------------------------------------------------------------------------------------ launch geometry
def bn3_geometry(M, C):
    """(P, nblk, iters) of bn3d_bf16.hip's streaming kernels: P pixels per workgroup and iteration, bn3_blocks()
    workgroups (two pixel groups per thread, capped at BN3_MAXBLK = 1024 with a grid-stride loop), and the most
    iterations a thread makes."""
    P = 256 // (C // 8)
    groups = (M + P - 1) // P
    nblk = min(max((groups + 1) // 2, 1), 1024)
    return P, nblk, (groups + nblk - 1) // nblk


def bn3_bwd_chain(M, C):
    """Longest chain of fp32 additions behind one partial of bn3d_bwd_partial_kernel: a thread's iterations, then the
    P pixel lanes summed in order through LDS.  The partials themselves are summed in fp64."""
    P, _, iters = bn3_geometry(M, C)
    return iters + P


def make_partials(y):
    """[nblk][C][2] fp32 rows as a test hands them to dmc_bn3d_bf16_fwd_ld: fp64 (sum, sum of squares) per block of
    PART_BLOCK pixels, rounded to fp32."""
    M, C = y.shape
    nblk = (M + PART_BLOCK - 1) // PART_BLOCK
    y64 = torch.zeros((nblk * PART_BLOCK, C), dtype=torch.float64, device=y.device)
    y64[:M] = y.double()
    y64 = y64.view(nblk, PART_BLOCK, C)
    return torch.stack((y64.sum(1), (y64 * y64).sum(1)), dim=2).float().contiguous()


# ------------------------------------------------------------------------------------------ statistics
class Stats:
    """fp64 statistics of a bf16 y [M][C] with their bounds, for partial sums that carry a chain of n fp32 additions.

    Sums.  |S1' - S1| <= n u sum|y|, |S2' - S2| <= n u sum y^2 (the squares of bf16 values are exact in fp32).
    mean.  The kernel divides the fp64 sum of the partials by M and rounds to fp32:
           d_mean = n u mabs (arith, mabs = sum|y| / M), u |mean| (fmt).
    var.   var' = S2'/M - mean'^2 in fp64 from the same partials (mean' before its rounding), clamped at 0 (the true
           variance is >= 0, so the clamp only moves var' towards it):
           |var' - var| <= n u S2/M + 2 |mean| d_mean + d_mean^2.
           With q = var + eps and cond = 1 + mean^2 / q: S2/M = var + mean^2 <= cond q, and
           2 |mean| mabs <= 2 |mean| sqrt(S2/M) <= mean^2 + S2/M <= (2 cond - 1) q, hence
           delta = |var' - var| / q <= 3 n u cond + d_mean^2 / q.
    invstd = q^-1/2.  |(1 + x)^-1/2 - 1| <= (|x| / 2) (1 - |x|)^-3/2 for |x| < 1 (mean value theorem), so the relative
           error is r_inv = (delta / 2) (1 - delta)^-3/2 (arith; infinite once delta >= 1: nothing can be promised),
           then one rounding to fp32, u (fmt).  A relative error in S2 thus reaches invstd multiplied by cond / 2.
    """

    def __init__(self, y, eps, n):
        y64 = y.double()
        self.M, self.C = y.shape
        M = self.M
        self.eps = f32(eps)
        self.s1, self.s2, self.sabs = y64.sum(0), (y64 * y64).sum(0), y64.abs().sum(0)
        self.mean = self.s1 / M
        self.var = ((y64 - self.mean) ** 2).sum(0) / M          # two-pass: no cancellation in the reference
        q = self.var + self.eps
        self.invstd = q.rsqrt()
        self.cond = 1.0 + self.mean ** 2 / q
        self.b_s1 = Bound(torch.zeros_like(self.s1), n * U32 * SLACK * self.sabs)
        self.b_s2 = Bound(torch.zeros_like(self.s2), n * U32 * SLACK * self.s2)
        self.d_mean = n * U32 * SLACK * self.sabs / M
        self.b_mean = Bound(U32 * self.mean.abs(), self.d_mean)
        self.delta = 3.0 * n * U32 * SLACK * self.cond + self.d_mean ** 2 / q
        self.d_var = self.delta * q
        ok = self.delta < 1.0
        self.r_inv = torch.where(ok, 0.5 * self.delta * (1.0 - self.delta.clamp_max(0.999)) ** -1.5,
                                 torch.full_like(self.delta, float("inf")))
        self.b_invstd = Bound(U32 * self.invstd, self.r_inv * self.invstd)
        # what the later stages inherit: the stored fp32 values' total errors
        self.e_mean = self.d_mean + U32 * self.mean.abs()
        self.e_inv = (1.0 + self.r_inv) * (1.0 + U32) - 1.0    # relative

    def running(self, rm0, rv0, momentum):
        """nn.BatchNorm3d's update, r = (1 - momentum) r0 + momentum v with the UNBIASED variance (M / (M - 1); the
        kernel keeps var itself for M = 1), evaluated in fp64 and rounded to fp32: momentum times the error of the
        statistic (arith) and u |r| (fmt)."""
        mom, M = f32(momentum), self.M
        unb = self.var * M / (M - 1) if M > 1 else self.var
        k = M / (M - 1.0) if M > 1 else 1.0
        rm = (1.0 - mom) * rm0.double().to(self.mean.device) + mom * self.mean
        rv = (1.0 - mom) * rv0.double().to(self.mean.device) + mom * unb
        return (rm, Bound(U32 * rm.abs(), mom * self.d_mean)), (rv, Bound(U32 * rv.abs(), mom * k * self.d_var))


def forward_ref(y, st, gamma, beta, relu):
    """relu?(gamma (y - mean) invstd + beta) in fp64 and its bound.

    bn3d_apply_kernel evaluates, all in fp32, sc = gamma * invstd', sh = beta - mean' * sc, v = y * sc + sh (no
    contraction: the build has -ffp-contract=off; an fma would only drop roundings), rectifies and rounds to bf16.
    With SC = gamma invstd and rs = e_inv + u (invstd's error, the product's rounding) the three addends of
    z = y SC - mean SC + beta carry
        y SC:     rs, the product's rounding, the last addition's            -> rs + 2u
        mean SC:  rs, the product's, sh's and the last addition's rounding,  -> rs + 3u, and e_mean |SC|
        beta:     sh's and the last addition's rounding                      -> 2u
    so |v - z| <= a = (|y SC| + |mean SC| + |beta|) (rs + 3u) SLACK + e_mean |SC|.  rs carries cond through e_inv.
    ReLU is 1-Lipschitz; the bf16 rounding of v adds 2^-8 |v| <= 2^-8 (|ref| + a)."""
    g64, b64 = gamma.double().to(y.device), beta.double().to(y.device)
    y64 = y.double()
    SC = g64 * st.invstd
    z = (y64 - st.mean) * SC + b64
    ref = z.clamp_min(0.0) if relu else z
    rs = st.e_inv + U32
    a = ((y64 * SC).abs() + (st.mean * SC).abs() + b64.abs()) * (rs + 3 * U32) * SLACK + st.e_mean * SC.abs()
    return ref, Bound(UBF * ref.abs(), (1.0 + UBF) * a)


def backward_ref(dout, y, out, st, gamma, relu, n):
    """dy, dgamma, dbeta in fp64 from dout, y and gamma, with the ReLU mask read from `out` (out > 0, what
    threshold_backward uses -- NOT recomputed from z), and their bounds for partials behind a chain of n fp32
    additions (bn3_bwd_chain).

    g = dout [out > 0], xh = (y - mean) invstd, SG = sum g, SGX = sum g xh, MG = SG / M, MGX = SGX / M,
    dbeta = SG, dgamma = SGX, dy = SC (g - MG - xh MGX).

    dbeta.   n u sum|g| (arith), u |SG| (fmt: the fp64 total is stored as fp32).
    xh'      = fl(fl(y - mean') * invstd'): |xh' - xh| <= |xh| (e_inv + 2u) + e_mean invstd = |xh| ex_rel + ex_abs.
    dgamma.  a term g xh' has one more rounding: sum|g xh| ((n + 1) u + ex_rel) SLACK + sum|g| ex_abs (arith), u |SGX|.
    dy.      mg' = fl(SG'/M), mgx' = fl(SGX'/M): d_mg = e_SG / M + u |MG|, d_mgx = e_SGX / M + u |MGX| -- the sums'
             bounds divided by M.  bn3d_bwd_apply_kernel then forms sc * ((g - mg') - xh' * mgx') in fp32: the
             addends g, MG and xh MGX each pass three roundings (their own difference or product, the difference of
             the two, the product with sc) and sc's relative error rs = e_inv + u:
             a = |SC| [(|g| + |MG| + |xh MGX|) (rs + 3u) + d_mg + |xh| d_mgx + (|xh| ex_rel + ex_abs) |MGX|] SLACK,
             and the bf16 rounding as in the forward."""
    g = dout.double()
    if relu:
        g = g * (out.double() > 0)
    y64, M = y.double(), st.M
    g64 = gamma.double().to(y.device)
    SC = g64 * st.invstd
    xh = (y64 - st.mean) * st.invstd
    SG, SGX = g.sum(0), (g * xh).sum(0)
    sabs_g, sabs_gx = g.abs().sum(0), (g * xh).abs().sum(0)
    ex_rel, ex_abs = st.e_inv + 2 * U32, st.e_mean * st.invstd
    e_sg = n * U32 * SLACK * sabs_g
    e_sgx = sabs_gx * ((n + 1) * U32 + ex_rel) * SLACK + sabs_g * ex_abs
    MG, MGX = SG / M, SGX / M
    d_mg, d_mgx = e_sg / M + U32 * MG.abs(), e_sgx / M + U32 * MGX.abs()
    dy = SC * (g - MG - xh * MGX)
    rs = st.e_inv + U32
    a = SC.abs() * ((g.abs() + MG.abs() + (xh * MGX).abs()) * (rs + 3 * U32) + d_mg + xh.abs() * d_mgx
                    + (xh.abs() * ex_rel + ex_abs) * MGX.abs()) * SLACK
    return dict(dy=(dy, Bound(UBF * dy.abs(), (1.0 + UBF) * a)),
                dgamma=(SGX, Bound(U32 * SGX.abs(), e_sgx)),
                dbeta=(SG, Bound(U32 * SG.abs(), e_sg)))


# ------------------------------------------------------------------------------------------ test data
def bn_case(M, C, seed, spread=False):
    """Operands of one BatchNorm shape: y, dout (bf16 [M][C]), gamma, beta, running_mean, running_var (fp32 [C]).
    Channel 1 has a negative gamma, channel 2 gamma = 0 exactly, channel 3 is constant (var = 0, invstd = eps^-1/2).
    spread: every other channel's mean is +-4 .. 8 of its deviations (var = E[y^2] - mean^2 loses bits there)."""
    r = np.random.RandomState(seed)
    sigma = r.uniform(0.5, 2.0, C)
    mean = r.uniform(4.0, 8.0, C) * r.choice([-1.0, 1.0], C) * sigma if spread else r.uniform(-1.0, 1.0, C) * sigma
    y = r.standard_normal((M, C)) * sigma + mean
    y[:, 3] = 1.5 if spread else 0.75
    gamma = r.uniform(0.5, 1.5, C)
    gamma[1] = -gamma[1]
    gamma[2] = 0.0
    beta = r.uniform(-0.5, 0.5, C)
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dt)
    return dict(y=t(y, torch.bfloat16), dout=t(r.standard_normal((M, C)), torch.bfloat16), gamma=t(gamma, torch.float32),
                beta=t(beta, torch.float32), rm=t(r.uniform(-1.0, 1.0, C), torch.float32), rv=t(r.uniform(0.5, 2.0, C), torch.float32))


#: (M, C, spread) of the direct BatchNorm tests
BN_SHAPES = [(2, 8, False), (7, 16, False),
             (333, 208, False),                  # C/8 = 26: P = 9 pixels per iteration, 22 idle threads
             (2500, 64, True),                   # channel means of +-4 .. 8 deviations
             (2500, 2048, False),                # P = 1, the block cap reached
             (2 * 1024 * 256 + 77, 8, False)]    # the cap at P = 256: a third, ragged grid-stride iteration


# ------------------------------------------------------------------------------------------ fp32 emulation (numpy)
def _bf16_round(v):
    """fp32 array -> nearest-even bf16, returned as fp32 (f2bf of the kernels; no NaNs expected here)."""
    b = np.ascontiguousarray(v, dtype=np.float32).view(np.uint32).astype(np.uint64)
    b = ((b + 0x7fff + ((b >> 16) & 1)) >> 16) << 16
    return b.astype(np.uint32).view(np.float32)


def emulate_forward(y, part, gamma, beta, rm0, rv0, eps, momentum, relu, defect=None):
    """bn3d_stats_final_kernel + bn3d_apply_kernel with their rounding points: fp64 over the fp32 partials, fp32 stats,
    fp32 sc / sh / v, bf16 out.  numpy arrays in (y fp32 holding bf16 values), dict of numpy arrays out.
    defect: 'biased' (running variance not unbiased), 'momentum' (applied the wrong way round), 'noeps' (eps dropped
    on channel 3)."""
    M, C = y.shape
    one = np.float32(1.0)
    s, ss = part[:, :, 0].astype(np.float64).sum(0), part[:, :, 1].astype(np.float64).sum(0)
    mean = s / M
    var = np.maximum(ss / M - mean * mean, 0.0)
    e = np.full(C, f32(eps))
    if defect == "noeps":
        e[3] = 0.0
    with np.errstate(divide="ignore", invalid="ignore"):
        inv32 = (1.0 / np.sqrt(var + e)).astype(np.float32)
        mean32 = mean.astype(np.float32)
        mom = f32(momentum)
        unb = var if (defect == "biased" or M == 1) else var * M / (M - 1)
        a, b = (mom, 1.0 - mom) if defect == "momentum" else (1.0 - mom, mom)
        rm = (a * rm0.astype(np.float64) + b * mean).astype(np.float32)
        rv = (a * rv0.astype(np.float64) + b * unb).astype(np.float32)
        sc = gamma * inv32
        sh = beta - mean32 * sc
        v = y * sc + sh
        if relu:
            v = np.where(v > 0, v, np.float32(0.0))
        out = _bf16_round(v * one)
    return dict(mean=mean32, invstd=inv32, rm=rm, rv=rv, out=out)


def emulate_backward(dout, y, mean32, inv32, gamma, beta, relu, defect=None):
    """bn3d_bwd_partial / _final / _apply with their rounding points and summation order: per thread over its grid-stride
    pixels, then over the P pixel lanes, both fp32; the workgroups' partials in fp64.
    defect: ('flip', m, c) one mask element inverted, 'nomask_dgamma' (sum g xhat taken over the unmasked dout)."""
    M, C = y.shape
    P, nblk, iters = bn3_geometry(M, C)
    sc = gamma * inv32
    sh = beta - mean32 * sc
    keep = (y * sc + sh > 0) if relu else np.ones((M, C), dtype=bool)
    if isinstance(defect, tuple) and defect[0] == "flip":
        keep[defect[1], defect[2]] ^= True
    g = np.where(keep, dout, np.float32(0.0))
    xh = (y - mean32) * inv32
    t2 = (dout if defect == "nomask_dgamma" else g) * xh

    def block_sums(t):
        pad = np.zeros((iters * nblk * P, C), dtype=np.float32)
        pad[:M] = t                                            # pixel m -> iteration m // (nblk P), workgroup, lane
        pad = pad.reshape(iters, nblk, P, C)
        acc = np.zeros((nblk, P, C), dtype=np.float32)
        for k in range(iters):
            acc = acc + pad[k]
        tot = np.zeros((nblk, C), dtype=np.float32)
        for p in range(P):
            tot = tot + acc[:, p]
        return tot.astype(np.float64).sum(0)

    s, ss = block_sums(g), block_sums(t2)
    mg, mgx = (s / M).astype(np.float32), (ss / M).astype(np.float32)
    dy = _bf16_round(sc * ((g - mg) - xh * mgx))
    return dict(dy=dy, dgamma=ss.astype(np.float32), dbeta=s.astype(np.float32))
