"""Reference side of the two small discriminator kernels (csrc/disc_c8.hip: the 8 -> 16, stride-2 block; csrc/disc_head.hip:
adv_layer on the NHWC activation): seeded inputs and fp64 results in plain torch on the CPU, with the error bars of an fp32 sum of
K products,

    |out - out64| <= (K + 2) * 2^-24 * S,    S = the same contraction of absolute values in fp64 (+ |bias|),

elementwise.  K: 72 + 1 for the block's forward and data gradient (72 fmaf roundings, then at most the LeakyReLU's and the keep
mask's product -- the bias is the sum's first term), N * OH * OW for its weight gradient, C * H * W for the head's forward, M for
its dweight / dbias, 2 for its dx.  Nothing here reads a kernel's result; every cached tensor is left unchanged."""
import functools

import torch
import torch.nn.functional as F

U = 2.0 ** -24
C8_SHAPES = [(1, 2, 2), (1, 4, 6), (3, 12, 20), (2, 18, 34), (1, 112, 112)]
C8_ODD_SHAPES = [(1, 7, 9), (2, 5, 12)]
#: the last head shape is ours: 37 frames are two full backward slices of 16 and a ragged one
HEAD_SHAPES = [(1, 16, 2, 3), (3, 32, 28, 28), (5, 128, 14, 14), (12, 128, 14, 14), (37, 16, 2, 3)]


def sid(shape):
    return "x".join(map(str, shape))


def rnd(seed, shape, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(shape, generator=g) * 2 - 1) * scale


def out_hw(h, w):
    return (h - 1) // 2 + 1, (w - 1) // 2 + 1


def nchw(t):
    return t.permute(0, 3, 1, 2)


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


@functools.lru_cache(maxsize=None)
def c8_inputs(shape):
    """x [N,H,W,8], w OHWI [16,3,3,8], bias [16], keep [N,16] (0 or 1 / 0.75), g [N,OH,OW,16]: fp32, CPU."""
    n, h, w = shape
    oh, ow = out_hw(h, w)
    keep = (rnd(14, (n, 16)) > -0.5).float() / 0.75
    return {"x": rnd(11, (n, h, w, 8)), "w": rnd(12, (16, 3, 3, 8), 0.2), "bias": rnd(13, (16,), 0.3), "keep": keep,
            "g": rnd(15, (n, oh, ow, 16))}


def _oihw(w_ohwi):
    return w_ohwi.permute(0, 3, 1, 2)


@functools.lru_cache(maxsize=None)
def c8_forward(shape, with_bias, with_keep, act):
    """(z64, bound) NHWC: the block's forward in fp64 and its bar.  Where the fp64 pre-activation is within its own bar of zero the
    fp32 run may take the other LeakyReLU branch: the bar there is the unscaled one (|a p - b p64| <= |p - p64| when the signs
    differ)."""
    d = c8_inputs(shape)
    x, w = nchw(d["x"]).double(), _oihw(d["w"]).double()
    b = d["bias"].double() if with_bias else None
    pre = F.conv2d(x, w, b, 2, 1)
    s = F.conv2d(x.abs(), w.abs(), b.abs() if with_bias else None, 2, 1)
    bar = (73 + 2) * U * s
    z = pre
    if act:
        slope = float(torch.tensor(0.2, dtype=torch.float32))       # the fp32 constant of the kernel (and of torch's fp32 LeakyReLU)
        z = torch.where(pre > 0, pre, slope * pre)
        bar = torch.where(pre < -bar, slope * bar, bar)
    if with_keep:
        k = d["keep"].double()[:, :, None, None]
        z, bar = z * k, bar * k
    return nhwc(z), nhwc(bar)


@functools.lru_cache(maxsize=None)
def c8_grads(shape):
    """fp64 (dx NHWC, dw OHWI, db) of sum(conv(x, w) * g) and their bars."""
    d = c8_inputs(shape)
    n, h, w_ = shape
    oh, ow = out_hw(h, w_)

    def grads(x, w, g):
        x = nchw(x).double().contiguous().requires_grad_(True)
        w = _oihw(w).double().contiguous().requires_grad_(True)
        b = torch.zeros(16, dtype=torch.float64, requires_grad=True)
        gx, gw, gb = torch.autograd.grad((F.conv2d(x, w, b, 2, 1) * nchw(g).double()).sum(), [x, w, b])
        return nhwc(gx), gw.permute(0, 2, 3, 1).contiguous(), gb
    dx, dw, db = grads(d["x"], d["w"], d["g"])
    sx, sw, sb = grads(d["x"].abs(), d["w"].abs(), d["g"].abs())
    k = n * oh * ow
    return {"dx": dx, "dw": dw, "db": db, "dx_bar": (73 + 2) * U * sx, "dw_bar": (k + 2) * U * sw, "db_bar": (k + 2) * U * sb}


@functools.lru_cache(maxsize=None)
def head_inputs(shape):
    """x [M,H,W,C] (NHWC memory), weight [2, C H W] in (c, h, w) column order, bias [2], dv [M,2]: fp32, CPU."""
    m, c, h, w = shape
    return {"x": rnd(21, (m, h, w, c)), "weight": rnd(22, (2, c * h * w), 0.05), "bias": rnd(23, (2,), 0.5), "dv": rnd(24, (m, 2))}


def head_flat(x_nhwc):
    """[M,H,W,C] -> [M, C H W] in the reference's flattening order."""
    return nchw(x_nhwc).reshape(x_nhwc.shape[0], -1)


@functools.lru_cache(maxsize=None)
def head_ref(shape):
    d = head_inputs(shape)
    m, c, h, w = shape
    xf, wt, b, dv = head_flat(d["x"]).double(), d["weight"].double(), d["bias"].double(), d["dv"].double()

    def unflat(t):
        return nhwc(t.reshape(m, c, h, w))
    return {"v": xf @ wt.t() + b, "v_bar": (c * h * w + 2) * U * (xf.abs() @ wt.abs().t() + b.abs()),
            "dx": unflat(dv @ wt), "dx_bar": (2 + 2) * U * unflat(dv.abs() @ wt.abs()),
            "dw": dv.t() @ xf, "dw_bar": (m + 2) * U * (dv.abs().t() @ xf.abs()),
            "db": dv.sum(0), "db_bar": (m + 2) * U * dv.abs().sum(0)}


def ratio(got, ref64, bar):
    """The worst error / bar over the tensor (0 / 0 counts as 0: an exactly reproduced zero under a zero bar)."""
    err = (got.detach().double().cpu() - ref64).abs()
    r = torch.where(err == 0, torch.zeros_like(err), err / bar.clamp_min(1e-300))
    return float(r.max()) if r.numel() else 0.0
