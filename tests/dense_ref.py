"""Reference side of the dense-estimator eval route (csrc/dense_eval.hip, ops.dense_eval*), on the CPU in plain torch / numpy.

  * the fp64 stack: F.conv2d in float64, F.leaky_relu(., 0.1), torch.cat((y, x), 1) -- the reference's forward, nothing else;
  * a buffer builder that scatters reference-order tensors into the slot order of the feature buffer, using the description
    ops.dense_eval_layout itself returns (offsets and the per-layer index maps), and its inverse;
  * seeded parameters: Gaussian weights scaled by 1.4 / sqrt(9 Cin), biases 0.1 N(0, 1).

Nothing here reads a kernel's result."""
import functools

import numpy as np
import torch
import torch.nn.functional as F

from dmcnet_amd import ops

WIDTHS = {"DenseNet": (128, 128, 96, 64, 32), "DenseNetSmall": (32, 32, 24, 16, 8)}
#: the documented shapes of the two buffers: K per layer, R per layer, CT
EXPECTED = {"DenseNet": ((16, 144, 272, 368, 432), (128, 128, 96, 64, 32), 464),
            "DenseNetSmall": ((16, 48, 80, 112, 144), (32, 32, 32, 32, 32), 176)}
SLOPE = 0.1
SEED = 811


def net_of_ct(ct):
    return {464: "DenseNet", 176: "DenseNetSmall"}[ct]


def rnd(seed, shape, scale=1.0):
    return torch.from_numpy((np.random.RandomState(seed).standard_normal(shape) * scale).astype(np.float32))


@functools.lru_cache(maxsize=None)
def params(name, seed=SEED, ch_in=5):
    """[(weight [Cout, Cin, 3, 3], bias [Cout]), ...] fp32 for conv_0 .. conv_4 and predict_flow, in the reference's channel order."""
    r = np.random.RandomState(seed)
    out, cin = [], ch_in
    for cout in tuple(WIDTHS[name]) + (2,):
        w = (r.standard_normal((cout, cin, 3, 3)) * (1.4 / np.sqrt(9.0 * cin))).astype(np.float32)
        b = (0.1 * r.standard_normal((cout,))).astype(np.float32)
        out.append((torch.from_numpy(w), torch.from_numpy(b)))
        if cout != 2:
            cin += cout
    return tuple(out)


def load_into(net, name, seed=SEED):
    """Copies params(name, seed) into a model.EstimatorDenseNet / EstimatorDenseNetSmall."""
    ps = params(name, seed)
    with torch.no_grad():
        for i, (w, b) in enumerate(ps[:-1]):
            conv = getattr(net, "conv_%d" % i)[0]
            conv.weight.copy_(w)
            conv.bias.copy_(b)
        net.predict_flow.weight.copy_(ps[-1][0])
        net.predict_flow.bias.copy_(ps[-1][1])
    return net


def stack(ps, x, upto=None, dtype=torch.float64):
    """The reference forward in ``dtype``.  Returns (pre, ys, out): the pre-activations and the activations y_k of conv_0 ..
    conv_{upto - 1} (all five by default) and predict_flow's result (None when ``upto`` stops short)."""
    depth = len(ps) - 1
    upto = depth if upto is None else upto
    x = x.to(dtype)
    pre, ys = [], []
    for w, b in ps[:upto]:
        p = F.conv2d(x, w.to(dtype), b.to(dtype), 1, 1)
        y = F.leaky_relu(p, SLOPE)
        pre.append(p)
        ys.append(y)
        x = torch.cat((y, x), 1)
    out = F.conv2d(x, ps[-1][0].to(dtype), ps[-1][1].to(dtype), 1, 1) if upto == depth else None
    return pre, ys, out


def stock_forward(net, x):
    """The hand-written stock loop of DenseEstimatorBase.forward on the network's own modules."""
    for i in range(net.depth):
        x = torch.cat((getattr(net, "conv_%d" % i)(x), x), 1)
    return net.predict_flow(x)


# ---------------------------------------------------------------- the feature buffer, from ops.dense_eval_layout's own description
def layout(name):
    return ops.dense_eval_layout(WIDTHS[name])


def to_buffer(lay, x, ys, fill=float("nan"), dtype=torch.float32):
    """[N, H, W, CT]: x [N, 5, H, W] in slot 0, ys[k] in slot k + 1, zeros in the pad channels of every slot that is present and
    ``fill`` in the slots that are not (len(ys) may stop short)."""
    n, c, h, w = x.shape
    off = list(lay["offsets"]) + [lay["ct"]]
    buf = torch.full((n, h, w, lay["ct"]), fill, dtype=dtype)
    for k, t in enumerate([x] + list(ys)):
        buf[..., off[k]:off[k + 1]] = 0
        buf[..., off[k]:off[k] + t.shape[1]] = t.permute(0, 2, 3, 1).to(dtype)
    return buf


def from_buffer(lay, buf, k, width):
    """Slot k of a buffer [N, H, W, CT] as [N, width, H, W] (the inverse of to_buffer for one slot) and its pad channels."""
    off = list(lay["offsets"]) + [lay["ct"]]
    return buf[..., off[k]:off[k] + width].permute(0, 3, 1, 2), buf[..., off[k] + width:off[k + 1]]


def gather_input(lay, k, buf):
    """The reference-order input [N, Cin, H, W] of conv_k (k == depth: predict_flow) read back out of a buffer through the map."""
    kk, _, index = lay["layers"][k] if k < len(lay["layers"]) else lay["head"]
    live = (index >= 0).nonzero().reshape(-1)
    cin = int(index.max()) + 1
    out = torch.zeros(buf.shape[:3] + (cin,), dtype=buf.dtype)
    out[..., index[live]] = buf[..., live]
    return out.permute(0, 3, 1, 2)


def buffer_weight(w, b, k, r, index):
    """(weight OHWI [r, 3, 3, k], bias [r]) in buffer order: column c holds input channel index[c] of ``w`` [Cout, Cin, 3, 3], zero
    columns for the pads, zero rows and bias entries past Cout."""
    cout = w.shape[0]
    live = (index >= 0).nonzero().reshape(-1)
    wb = torch.zeros((r, 3, 3, k), dtype=w.dtype)
    wb[:cout][..., live] = w.permute(0, 2, 3, 1)[..., index[live]]
    bb = torch.zeros((r,), dtype=b.dtype)
    bb[:cout] = b
    return wb, bb


def reference_weight(wb, cout, index):
    """The inverse of buffer_weight: [Cout, Cin, 3, 3] in the reference's order."""
    live = (index >= 0).nonzero().reshape(-1)
    cin = int(index.max()) + 1
    w = torch.zeros((cout, 3, 3, cin), dtype=wb.dtype)
    w[..., index[live]] = wb[:cout][..., live]
    return w.permute(0, 3, 1, 2).contiguous()
