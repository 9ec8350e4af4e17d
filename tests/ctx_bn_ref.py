"""fp64 reference of the training-mode BatchNorm2d + LeakyReLU of a ContextNetwork unit (csrc/ctx_bn.hip, ops.bn_leaky), the
operands of its op-level tests and the seeds at which those operands keep clear of the LeakyReLU kink.

Everything works on [M pixels][C channels] views of channels_last memory, in torch.double, on whatever device the operands are.

    mean = sum z / M,  var = sum (z - mean)^2 / M (biased, two-pass),  invstd = (var + eps)^-1/2
    xhat = (z - mean) invstd,  t = xhat gamma + beta,  y = t > 0 ? t : slope t              (t == 0 takes slope, as torch does)
    g = dy (t > 0 ? 1 : slope),  dbeta = sum g,  dgamma = sum g xhat,  dz = gamma invstd (g - dbeta / M - xhat dgamma / M)
    running_mean' = (1 - m) running_mean + m mean,  running_var' = (1 - m) running_var + m var M / (M - 1)

eps, slope and the momentum m enter as the fp32 values the C ABI is handed (f32()).  test_ctx_bn_cpu.py holds these formulas to
torch's autograd over BatchNorm2d().double() + LeakyReLU."""
import numpy as np
import torch

U32 = 2.0 ** -24
KINK_MARGIN = 2.0 ** -20          # as tests/test_dconv_gpu.py: sixteen fp32 ulps of the largest BatchNorm output
EPS, SLOPE, MOMENTUM = 1e-5, 0.1, 0.1


def f32(v):
    return float(np.float32(v))


def stats_ref(z, eps=EPS):
    z = z.double()
    mean = z.mean(0)
    var = ((z - mean) ** 2).mean(0)
    return mean, var, (var + f32(eps)).rsqrt()


def forward_ref(z, gamma, beta, mean, invstd, slope=SLOPE):
    """(y, t, xhat) in fp64 from the given statistics (the true ones, or the fp32 pair a kernel stored)."""
    xh = (z.double() - mean.double()) * invstd.double()
    t = xh * gamma.double() + beta.double()
    return torch.where(t > 0, t, f32(slope) * t), t, xh


def backward_ref(z, dy, gamma, mean, invstd, positive, slope=SLOPE):
    """(dz, dgamma, dbeta) in fp64; ``positive``: the [M][C] bool decision t > 0 (the forward's, bit for bit)."""
    M = z.shape[0]
    xh = (z.double() - mean.double()) * invstd.double()
    g = dy.double() * torch.where(positive, torch.ones_like(xh), torch.full_like(xh, f32(slope)))
    sb, sg = g.sum(0), (g * xh).sum(0)
    dz = gamma.double() * invstd.double() * (g - sb / M - xh * sg / M)
    return dz, sg, sb


def running_ref(mean, var, M, rm0, rv0, momentum=MOMENTUM):
    m = f32(momentum)
    return (1.0 - m) * rm0.double() + m * mean, (1.0 - m) * rv0.double() + m * var * (M / (M - 1.0))


# ------------------------------------------------------------------------------------------ launch geometry (ctx_bn.hip)
MAX_BLOCKS = 2048


def block_of(C):
    return 192 if C == 96 else 256


def blocks_of(M, C):
    return min(-(-(M * (C // 4)) // block_of(C)), MAX_BLOCKS)


# ------------------------------------------------------------------------------------------ operands
def bn_case(M, C, seed, kind="normal"):
    """fp32 CPU operands of one case: z, dy [M][C], gamma, beta, rm, rv [C].

    kind="normal": z ~ N(0, 1) per element, gamma in +-(0.5, 1.5) (every fifth negative), beta in (-0.5, 0.5).
    kind="cond":   the same with a per-channel offset of 64 standard deviations (mean = 64 std: E[z^2] - E[z]^2 loses 12 bits).
    kind="gapped": |z| = 1 + |N(0, 1)| with a random sign, |beta / gamma| < 0.4: no element's t can come near 0 (xhat stays outside
                   (-0.55, 0.55) while the kink sits at xhat = -beta / gamma), whatever the size -- for the shape that is too large
                   for a kink-free draw of the normal kind (15 M elements at C = 128)."""
    r = np.random.RandomState(seed)
    z = r.standard_normal((M, C))
    gamma = r.uniform(0.5, 1.5, C)
    gamma[::5] *= -1.0
    beta = r.uniform(-0.5, 0.5, C)
    if kind == "cond":
        z = z + 64.0
    elif kind == "gapped":
        z = np.sign(z) * (1.0 + np.abs(z))
        beta = r.uniform(-0.2, 0.2, C)
    elif kind != "normal":
        raise ValueError(kind)
    dy = r.standard_normal((M, C))
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))
    return dict(z=t(z), dy=t(dy), gamma=t(gamma), beta=t(beta), rm=t(r.uniform(-1.0, 1.0, C)), rv=t(r.uniform(0.5, 2.0, C)), M=M, C=C)


def crafted_case(M, C, channel, seed):
    """bn_case(normal) whose ``channel`` holds -1, 0, +1 in equal numbers with gamma = 1, beta = 0: mean = 0 exactly (the fp64 sums
    of +-1 are exact), xhat = t = 0 exactly at the zeros, which therefore take ``slope`` in the backward and give y == 0."""
    assert M % 3 == 0
    c = bn_case(M, C, seed)
    c["z"][:, channel] = torch.tensor([-1.0, 0.0, 1.0]).repeat(M // 3)[torch.from_numpy(np.random.RandomState(seed + 1).permutation(M))]
    c["gamma"][channel], c["beta"][channel] = 1.0, 0.0
    return c


def margin(case):
    """min |t| / max |t| of the fp64 reference's BatchNorm outputs."""
    mean, _, invstd = stats_ref(case["z"])
    _, t, _ = forward_ref(case["z"], case["gamma"], case["beta"], mean, invstd)
    return float(t.abs().min() / t.abs().max())


#: the geometry shape: see tests/test_ctx_bn_gpu.py
M_GEOMETRY = 120001
#: (M, C, kind) of the op-level GPU cases
OP_CASES = ([(2, 32, "normal"), (2, 96, "normal"), (105, 96, "normal"), (105, 128, "normal")]
            + [(1188, c, "normal") for c in (32, 64, 96, 128)] + [(8601, c, "normal") for c in (32, 64, 96, 128)]
            + [(M_GEOMETRY, 32, "gapped"), (M_GEOMETRY, 128, "gapped"), (1188, 96, "cond")])


def kink_free_seed(M, C, kind, first=51, tries=400):
    """The first seed from ``first`` upwards at which the fp64 reference alone keeps every BatchNorm output at
    |t| >= KINK_MARGIN max |t|: two correct fp32 routes then take the same LeakyReLU slope for every element."""
    for seed in range(first, first + tries):
        if margin(bn_case(M, C, seed, kind)) >= KINK_MARGIN:
            return seed
    raise AssertionError("no kink-free operands among %d seeds for %s" % (tries, (M, C, kind)))


#: what kink_free_seed() returns (test_ctx_bn_cpu.py recomputes it)
OP_SEEDS = {(2, 32, "normal"): 51, (2, 96, "normal"): 51, (105, 96, "normal"): 51, (105, 128, "normal"): 51,
            (1188, 32, "normal"): 51, (1188, 64, "normal"): 52, (1188, 96, "normal"): 51, (1188, 128, "normal"): 51,
            (8601, 32, "normal"): 55, (8601, 64, "normal"): 53, (8601, 96, "normal"): 136, (8601, 128, "normal"): 92,
            (M_GEOMETRY, 32, "gapped"): 51, (M_GEOMETRY, 128, "gapped"): 51, (1188, 96, "cond"): 51}
