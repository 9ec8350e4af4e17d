"""Reference side of the early-fusion estimators' own route (csrc/early_fusion.hip, ops.early_fusion_*), on the CPU in plain torch.

  * the restatement: F.conv2d, F.leaky_relu(., 0.1), torch.cat and one add in any dtype -- the reference's forward
    (code/dmcnet/model.py:197-250), nothing else; its gradients are autograd's of exactly that;
  * seeded parameters: O.seeded_state_fill(O.build_estimator(name), seed=25), the draw of the reference's own golden;
  * a buffer builder that scatters reference-order tensors into the slot order ops.early_fusion_layout itself describes.

Nothing here reads a kernel's result."""
import functools

import torch
import torch.nn.functional as F

from dmcnet_amd import model, ops
from oracle import dmc_oracle as O
from tests.dense_ref import rnd  # noqa: F401  (the tests' inputs: rnd(31, shape))

SLOPE = 0.1
SEED = 25
NETS = ["Sum", "Stack"]
ARCH = {"Sum": "DenseNetTinyEarlyFusionSum", "Stack": "DenseNetTinyEarlyFusionStack"}
CLS = {"Sum": model.EstimatorDenseNetTinyEarlyFusionSum, "Stack": model.EstimatorDenseNetTinyEarlyFusionStack}
MAIN_SHAPES = [(1, 5, 20, 37), (3, 5, 33, 18), (3, 5, 14, 14)]
DEGENERATE_SHAPES = [(2, 5, 1, 7), (2, 5, 9, 1)]
ROW_SHAPE = (2, 5, 224, 224)
#: the fourteen parameters in the order ops.early_fusion_train passes them
UNITS = ["conv_0_mv.0", "conv_0_r.0", "conv_1.0", "conv_2.0", "conv_3.0", "conv_4.0", "predict_flow"]
PARAM_NAMES = [u + s for u in UNITS for s in (".weight", ".bias")]


def sid(shape):
    return "x".join(map(str, shape))


@functools.lru_cache(maxsize=None)
def state(name):
    """The seeded state dict (fp32 CPU tensors); never modified."""
    return {k: v.detach().clone() for k, v in O.seeded_state_fill(O.build_estimator(ARCH[name]), seed=SEED).state_dict().items()}


def params(name, dtype=torch.float32):
    """[(weight, bias)] of conv_0_mv, conv_0_r, conv_1 .. conv_4, predict_flow in ``dtype`` (fresh tensors)."""
    st = state(name)
    return [(st[u + ".weight"].to(dtype).clone(), st[u + ".bias"].to(dtype).clone()) for u in UNITS]


def net(name, device="cpu", dtype=torch.float32):
    m = CLS[name]()
    m.load_state_dict(state(name))
    return m.to(device=device, dtype=dtype)


def forward(ps, x, stack, upto=5):
    """The reference forward on the parameter list ``ps`` in the dtype of its tensors.  Returns a dict: "a", "b" (the two first
    pre-activations), "m", "r", "base" (cat(m, r) or m + r), "pre" / "ys" (the pre-activations and the activations of conv_1 ..
    conv_{upto - 1}) and "out" (predict_flow's result, None when ``upto`` stops short of 5)."""
    x = x.to(ps[0][0].dtype)
    a = F.conv2d(x[:, :2], ps[0][0], ps[0][1], 1, 1)
    b = F.conv2d(x[:, 2:], ps[1][0], ps[1][1], 1, 1)
    m, r = F.leaky_relu(a, SLOPE), F.leaky_relu(b, SLOPE)
    base = torch.cat((m, r), 1) if stack else m + r
    t, pre, ys = base, [], []
    for k in range(1, upto):
        p = F.conv2d(t, ps[1 + k][0], ps[1 + k][1], 1, 1)
        y = F.leaky_relu(p, SLOPE)
        pre.append(p)
        ys.append(y)
        t = torch.cat((y, t), 1)
    out = F.conv2d(t, ps[6][0], ps[6][1], 1, 1) if upto == 5 else None
    return {"a": a, "b": b, "m": m, "r": r, "base": base, "pre": pre, "ys": ys, "out": out}


@functools.lru_cache(maxsize=None)
def reference(name, shape, seed=31):
    """(x fp32, the fp64 forward dict, the fp32 forward's out) for rnd(seed, shape); computed once, never modified."""
    x = rnd(seed, shape)
    with torch.no_grad():
        f64 = forward(params(name, torch.float64), x, name == "Stack")
        o32 = forward(params(name), x, name == "Stack")["out"]
    return x, f64, o32


def gradients(name, x, r, dtype):
    """(out, [fourteen gradients in PARAM_NAMES order]) of sum(out * r) through the restatement in ``dtype``."""
    ps = [(w.requires_grad_(True), b.requires_grad_(True)) for w, b in params(name, dtype)]
    out = forward(ps, x.to(dtype), name == "Stack")["out"]
    flat = [t for pair in ps for t in pair]
    return out.detach(), list(torch.autograd.grad((out * r.to(dtype)).sum(), flat))


def stock_forward(m, x):
    """The hand-written stock loop of model._EarlyFusion.forward on the network's own modules."""
    a, b = m.conv_0_mv(x[:, :2]), m.conv_0_r(x[:, 2:])
    x = torch.cat((a, b), 1) if m.stack else a + b
    for i in (1, 2, 3, 4):
        x = torch.cat((getattr(m, "conv_%d" % i)(x), x), 1)
    return m.predict_flow(x)


# ---------------------------------------------------------------- the feature buffer, from ops.early_fusion_layout's own description
def layout(name):
    return ops.early_fusion_layout(name == "Stack")


def to_buffer(name, fwd, upto, fill=float("nan"), dtype=torch.float32):
    """[N, H, W, CT]: the base slot(s) and y_1 .. y_{upto - 1} of the forward dict ``fwd``, zeros in the pad channels of every slot that
    is present and ``fill`` in the slots that are not."""
    lay = layout(name)
    n, _, h, w = fwd["a"].shape
    buf = torch.full((n, h, w, lay["ct"]), fill, dtype=dtype)
    slots = [("m", fwd["m"]), ("r", fwd["r"])] if name == "Stack" else [("s", fwd["base"])]
    slots += [("y%d" % (j + 1), y) for j, y in enumerate(fwd["ys"][:upto - 1])]
    for key, t in slots:
        first, live = lay["offsets"][key]
        buf[..., first:first + (live + 3) // 4 * 4] = 0
        buf[..., first:first + live] = t.permute(0, 2, 3, 1).to(dtype)
    return buf


def gather_input(index, buf):
    """The reference-order input [N, Cin, H, W] of a layer read back out of a buffer through its index map."""
    live = (index >= 0).nonzero().reshape(-1)
    out = torch.zeros(buf.shape[:3] + (int(index.max()) + 1,), dtype=buf.dtype)
    out[..., index[live]] = buf[..., live]
    return out.permute(0, 3, 1, 2)


def buffer_weight(w, k, index):
    """[R, 9, K] in buffer order: column c holds input channel index[c] of ``w`` [R, Cin, 3, 3], zero columns for the pads."""
    live = (index >= 0).nonzero().reshape(-1)
    wb = torch.zeros((w.shape[0], 3, 3, k), dtype=w.dtype)
    wb[..., live] = w.permute(0, 2, 3, 1)[..., index[live]]
    return wb.reshape(w.shape[0], 9, k).contiguous()
