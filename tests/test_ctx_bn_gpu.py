"""GPU: BatchNorm2d + LeakyReLU of the ContextNetwork training route (csrc/ctx_bn.hip, ops.bn_leaky, model.CTX_TRAIN_BN).

Through the C ABI with every output prefilled with NaN and the scratch at exactly the reported size, on the shapes of
ctx_bn_ref.OP_CASES (the smallest at which these kernels can go wrong, see GEOMETRY below), each stage judged on the operands it
really had:

  statistics   stored mean / invstd against the fp64 statistics of the same z, per channel, e <= max(2 e_ref, 4u |ref|) with e_ref
               the error of torch.native_batch_norm's save_mean / save_invstd on the same device; the running statistics after one
               call by the same rule against the stock module's buffers;
  apply        y against fp64 arithmetic on the kernel's STORED statistics, |y - y64| <= 4u (|gamma xhat| + |beta|): the expression
               fmaf((z - mean) * invstd, gamma, beta) and the slope have four roundings (sub, mul, fma, slope) -- derived, not measured;
  slope        (y > 0) == (t_ref > 0) everywhere (the seeds of ctx_bn_ref.OP_SEEDS guarantee it of the reference); a crafted channel
               of -1, 0, +1 whose zeros give y == 0 and take `slope` in dz;
  backward     dz, dgamma, dbeta against ctx_bn_ref in fp64 with the mask from the kernel's own y > 0, e <= max(2 e_ref, 8u max|ref|)
               per tensor, e_ref the error of the stock fp32 BatchNorm2d + LeakyReLU autograd on the same device (2: what two correct
               fp32 routes with different summation orders may differ by; the floor: a stock result that happens to be near exact);
  run to run   forward and backward twice, bit-equal.

Then ops.bn_leaky, the whole networks with both flags on (the cases, seeds and bar of tests/test_dconv_gpu.py), the dispatch, and
both launching entry points in guarded arenas (tests/abi_arena.py).  Every (e, e_ref, max|ref|) is printed.

Measured on an MI355X, worst over the op-level cases: mean, invstd and both running statistics within one fp32
rounding of the fp64 value (e / u|ref| <= 1.00; e_ref the same or larger); |y - y64| <= 0.67 of its bound; dz e 5.1e-7 against
e_ref 5.9e-7 at 120001 x 32 (the case closest to its bar), dgamma 1.6e-5 against 2.7e-5, dbeta 3.4e-6 against 4.2e-6; the crafted
zeros |dz - ref(slope)| 3.6e-8 against |dz - ref(1)| 3.5; whole networks, worst pair: grad:predict_flow.0.weight e 1.1e-4,
e_ref 6.7e-5, max|ref| 55.8."""
import copy

import numpy as np
import pytest
import torch

from dmcnet_amd import _lib, model, ops
from tests import abi_cases
from tests import ctx_bn_ref as R
from tests import test_dconv_gpu as G
from tests.abi_arena import run_case

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U8 = torch.uint8
CL = torch.channels_last
U = R.U32
NAN = float("nan")


def P(t):
    return _lib.ptr(t)


def dev(case):
    return {k: (v.to(DEV) if torch.is_tensor(v) else v) for k, v in case.items()}


def nan(*shape):
    return torch.full(shape, NAN, dtype=torch.float32, device=DEV)


def scratch_for(M, C):
    return torch.full((_lib.load().dmc_bnlrelu_scratch_bytes(M, C),), 0xFF, dtype=U8, device=DEV)


def run_fwd(c, running=True):
    """dict(y, mean, invstd, rm, rv) of dmc_bnlrelu_fwd on the device operands ``c``; rm / rv: copies, updated (None without)."""
    M, C = c["M"], c["C"]
    y, stats = nan(M, C), nan(2 * C)
    rm, rv = (c["rm"].clone(), c["rv"].clone()) if running else (None, None)
    _lib.check(_lib.load().dmc_bnlrelu_fwd(P(c["z"]), P(c["gamma"]), P(c["beta"]), P(rm), P(rv), P(y), P(stats), P(scratch_for(M, C)), M, C,
                                           R.SLOPE, R.EPS, R.MOMENTUM, ops._stream()), "dmc_bnlrelu_fwd")
    return dict(y=y, stats=stats, mean=stats[:C], invstd=stats[C:], rm=rm, rv=rv)


def run_bwd(c, stats):
    M, C = c["M"], c["C"]
    dz, dgamma, dbeta = nan(M, C), nan(C), nan(C)
    _lib.check(_lib.load().dmc_bnlrelu_bwd(P(c["z"]), P(c["dy"]), P(c["gamma"]), P(c["beta"]), P(stats), P(scratch_for(M, C)), P(dz), P(dgamma),
                                           P(dbeta), M, C, R.SLOPE, ops._stream()), "dmc_bnlrelu_bwd")
    return dict(dz=dz, dgamma=dgamma, dbeta=dbeta)


#: M = N H W as the frames it stands for: the stock modules get an ordinary [N, C, H, W] tensor
FRAMES = {2: (2, 1, 1), 105: (7, 5, 3), 1188: (2, 33, 18), 8601: (3, 61, 47), R.M_GEOMETRY: (49, 31, 79)}


def as4(t):
    """[M][C] -> the same memory as a channels_last [N, C, H, W] tensor."""
    n, h, w = FRAMES[t.shape[0]]
    assert n * h * w == t.shape[0]
    return t.view(n, h, w, t.shape[1]).permute(0, 3, 1, 2)


def as2(t4):
    return t4.permute(0, 2, 3, 1).reshape(-1, t4.shape[1])


def stock_module(c):
    bn = torch.nn.BatchNorm2d(c["C"], eps=R.EPS, momentum=R.MOMENTUM).to(DEV).train()
    with torch.no_grad():
        bn.weight.copy_(c["gamma"])
        bn.bias.copy_(c["beta"])
        bn.running_mean.copy_(c["rm"])
        bn.running_var.copy_(c["rv"])
    return bn


def stock_step(c):
    """The stock fp32 route on the same device: dict(y, dz, dgamma, dbeta, rm, rv)."""
    bn = stock_module(c)
    x4 = as4(c["z"]).detach().clone(memory_format=torch.preserve_format).requires_grad_(True)
    y4 = torch.nn.LeakyReLU(R.SLOPE, inplace=True)(bn(x4))
    y4.backward(as4(c["dy"]))
    return dict(y=as2(y4.detach()), dz=as2(x4.grad), dgamma=bn.weight.grad, dbeta=bn.bias.grad, rm=bn.running_mean.detach(),
                rv=bn.running_var.detach(), nbt=int(bn.num_batches_tracked))


def err(a, ref):
    return float((a.double() - ref).abs().max())


def judge(tag, name, got, ref, stock, floor_u, bad, per_channel=False):
    """e <= max(2 e_ref, floor_u u |ref|): per channel (|ref| of the channel) or per tensor (max |ref|).  Prints the figures."""
    e, e_ref = (got.double() - ref).abs(), (stock.double() - ref).abs()
    if per_channel:
        ok = bool((e <= torch.maximum(2 * e_ref, floor_u * U * ref.abs())).all())
        k = int((e / torch.maximum(2 * e_ref, floor_u * U * ref.abs()).clamp_min(1e-300)).argmax())
        fig = (float(e[k]), float(e_ref[k]), float(ref[k].abs()))
    else:
        top = float(ref.abs().max())
        fig = (float(e.max()), float(e_ref.max()), top)
        ok = fig[0] <= max(2 * fig[1], floor_u * U * top)
    print("bnlrelu %-22s %-8s e %.3e e_ref %.3e |ref| %.3e  (e / u|ref| = %.2f)" % ((tag, name) + fig + (fig[0] / max(U * fig[2], 1e-300),)))
    if not ok:
        bad.append((name,) + fig)


def check_case(tag, c, crafted_channel=None):
    """All op-level checks of one case through the C ABI."""
    M, C = c["M"], c["C"]
    assert _lib.load().dmc_bnlrelu_supported(M, C) == 1
    bad = []
    f = run_fwd(c)
    for t in f.values():
        assert not bool(torch.isnan(t).any())
    st = stock_step(c)
    # 1. statistics
    mean, var, invstd = R.stats_ref(c["z"])
    _, sm, si = torch.native_batch_norm(as4(c["z"]), c["gamma"], c["beta"], c["rm"].clone(), c["rv"].clone(), True, R.MOMENTUM, R.EPS)
    judge(tag, "mean", f["mean"], mean, sm, 4, bad, per_channel=True)
    judge(tag, "invstd", f["invstd"], invstd, si, 4, bad, per_channel=True)
    rm, rv = R.running_ref(mean, var, M, c["rm"], c["rv"])
    judge(tag, "run_mean", f["rm"], rm, st["rm"], 4, bad, per_channel=True)
    judge(tag, "run_var", f["rv"], rv, st["rv"], 4, bad, per_channel=True)
    # 2. apply, on the stored statistics
    y64, _, xh = R.forward_ref(c["z"], c["gamma"], c["beta"], f["mean"], f["invstd"])
    bound = 4 * U * ((c["gamma"].double() * xh).abs() + c["beta"].double().abs())
    ey = (f["y"].double() - y64).abs()
    print("bnlrelu %-22s %-8s worst |y - y64| / bound %.3f" % (tag, "y", float((ey / bound.clamp_min(1e-300)).max())))
    assert bool((ey <= bound).all()), float((ey / bound.clamp_min(1e-300)).max())
    # 3. slope agreement with the fp64 reference
    _, t_ref, _ = R.forward_ref(c["z"], c["gamma"], c["beta"], mean, invstd)
    pos = f["y"] > 0
    assert torch.equal(pos, t_ref > 0)
    # 4. backward, mask from the kernel's own y
    b = run_bwd(c, f["stats"])
    for t in b.values():
        assert not bool(torch.isnan(t).any())
    dz, dgamma, dbeta = R.backward_ref(c["z"], c["dy"], c["gamma"], mean, invstd, pos)
    judge(tag, "dz", b["dz"], dz, st["dz"], 8, bad)
    judge(tag, "dgamma", b["dgamma"], dgamma, st["dgamma"], 8, bad)
    judge(tag, "dbeta", b["dbeta"], dbeta, st["dbeta"], 8, bad)
    if crafted_channel is not None:
        k = crafted_channel
        zero = c["z"][:, k] == 0
        assert int(zero.sum()) == M // 3
        assert float(f["mean"][k]) == 0.0 and bool((f["y"][:, k][zero] == 0).all())
        # the zeros took `slope`: against the reference that lets them pass with 1 the error is of the size of the gradient
        e_slope = float((b["dz"][:, k][zero].double() - dz[:, k][zero]).abs().max())
        dz1, _, _ = R.backward_ref(c["z"], c["dy"], c["gamma"], mean, invstd, t_ref >= 0)
        e_one = float((b["dz"][:, k][zero].double() - dz1[:, k][zero]).abs().max())
        print("bnlrelu %-22s zeros: |dz - ref(slope)| %.3e, |dz - ref(1)| %.3e" % (tag, e_slope, e_one))
        assert e_slope <= 8 * U * float(dz.abs().max()) and e_one > 1e-2
    # 5. run to run
    f2 = run_fwd(c)
    for k in ("y", "stats", "rm", "rv"):
        assert torch.equal(f[k], f2[k]), k
    b2 = run_bwd(c, f["stats"])
    for k in b:
        assert torch.equal(b[k], b2[k]), k
    # without running pointers: the same statistics and values, nothing else touched
    f3 = run_fwd(c, running=False)
    assert torch.equal(f3["y"], f["y"]) and torch.equal(f3["stats"], f["stats"])
    assert not bad, bad


#: GEOMETRY (ctx_bn.hip).  A workgroup has 256 threads (192 at C = 96), a thread owns one float4 column; the partial and the apply
#: kernels run blocks_of(M, C) = min(ceil(M C / 4 / block), 2048) workgroups and stride the grid, four strides per pass of their
#: unrolled loop and one per pass of the tail loop; the finalising kernels add the partials of a channel 256 at a time.
#: R.M_GEOMETRY = 120001 is the smallest round M (+ 1: ragged) at which, within 64 MB per tensor at C = 128 (61.4 MB),
#:   * at C = 128 the unrolled loop makes a second pass for some threads: M C / 4 > 7 strides of 2048 * 256 float4s <=> M > 114688,
#:     and the tail loop runs behind it (7.32 strides);
#:   * at C = 32 (the same M: 1.83 strides) the tail loop alone makes a second pass;
#:   * both run 2048 workgroups: a finalising thread adds 8 partials (more than one reduction step).
def test_geometry_shape_reaches_what_it_is_for():
    M = R.M_GEOMETRY
    stride = R.MAX_BLOCKS * 256
    assert M * 128 * 4 <= 64 << 20
    assert R.blocks_of(M, 32) == R.blocks_of(M, 128) == R.MAX_BLOCKS > 256
    assert 7 * stride < M * 32 < 8 * stride                       # C = 128: float4s
    assert stride < M * 8 < 2 * stride                            # C = 32
    # and the small shapes sit on the other side of every threshold: one workgroup, a partly filled one, a ragged last one
    assert R.blocks_of(2, 32) == 1 and R.blocks_of(105, 96) == 14 and 105 * 24 % 192 != 0 and R.blocks_of(8601, 128) == 1076


@pytest.mark.parametrize("case", R.OP_CASES, ids=["%dx%d-%s" % c for c in R.OP_CASES])
def test_forward_and_backward_vs_fp64(case):
    M, C, kind = case
    check_case("%dx%d-%s" % case, dev(R.bn_case(M, C, R.OP_SEEDS[case], kind)))


def test_zeros_of_the_batchnorm_output_take_the_slope():
    M, C, k = 1188, 32, 5
    check_case("1188x32-crafted", dev(R.crafted_case(M, C, k, R.OP_SEEDS[(M, C, "normal")])), crafted_channel=k)


# ---------------------------------------------------------------------------------------------------------------------
# the autograd op
# ---------------------------------------------------------------------------------------------------------------------
OP = (2, 96, 33, 18)                                               # M = 1188, C = 96


def op_case():
    n, c, h, w = OP
    return dev(R.bn_case(n * h * w, c, R.OP_SEEDS[(n * h * w, c, "normal")]))


def to4(t, fmt):
    n, c, h, w = OP
    return t.view(n, h, w, c).permute(0, 3, 1, 2).contiguous(memory_format=fmt)


def test_autograd_op_vs_fp64_and_stock():
    n, c, h, w = OP
    case = op_case()
    M = case["M"]
    bn = stock_module(case)
    lrelu = torch.nn.LeakyReLU(R.SLOPE)
    xi = to4(case["z"], torch.contiguous_format).requires_grad_(True)          # NCHW: the op makes it channels_last itself
    assert ops.bn_leaky_supported(xi, bn, lrelu)
    y = ops.bn_leaky(xi, bn, R.SLOPE)
    assert tuple(y.shape) == OP and y.is_contiguous(memory_format=CL)
    y.backward(to4(case["dy"], CL))
    assert int(bn.num_batches_tracked) == 1
    st = stock_step(case)
    assert st["nbt"] == 1
    mean, var, invstd = R.stats_ref(case["z"])
    y64, t_ref, _ = R.forward_ref(case["z"], case["gamma"], case["beta"], mean, invstd)
    assert torch.equal(as2(y.detach()) > 0, t_ref > 0)
    dz, dgamma, dbeta = R.backward_ref(case["z"], case["dy"], case["gamma"], mean, invstd, t_ref > 0)
    rm, rv = R.running_ref(mean, var, M, case["rm"], case["rv"])
    bad = []
    judge("ops.bn_leaky", "y", as2(y.detach()), y64, st["y"], 8, bad)
    judge("ops.bn_leaky", "x.grad", as2(xi.grad), dz, st["dz"], 8, bad)
    judge("ops.bn_leaky", "dgamma", bn.weight.grad, dgamma, st["dgamma"], 8, bad)
    judge("ops.bn_leaky", "dbeta", bn.bias.grad, dbeta, st["dbeta"], 8, bad)
    judge("ops.bn_leaky", "run_mean", bn.running_mean, rm, st["rm"], 4, bad, per_channel=True)
    judge("ops.bn_leaky", "run_var", bn.running_var, rv, st["rv"], 4, bad, per_channel=True)
    assert not bad, bad
    # what the op refuses
    assert not ops.bn_leaky_supported(xi.cpu(), bn, lrelu) and not ops.bn_leaky_supported(xi.double(), bn, lrelu)
    assert not ops.bn_leaky_supported(xi, copy.deepcopy(bn).eval(), lrelu)
    assert not ops.bn_leaky_supported(xi, bn, torch.nn.ReLU())
    assert not ops.bn_leaky_supported(xi, torch.nn.BatchNorm2d(c, affine=False).to(DEV), lrelu)
    assert not ops.bn_leaky_supported(xi, torch.nn.BatchNorm2d(c, track_running_stats=False).to(DEV), lrelu)
    assert not ops.bn_leaky_supported(xi, torch.nn.BatchNorm2d(c, momentum=None).to(DEV), lrelu)
    assert not ops.bn_leaky_supported(xi[:, :48], torch.nn.BatchNorm2d(48).to(DEV), lrelu)
    with pytest.raises(_lib.DmcHipError):
        ops.bn_leaky(xi, copy.deepcopy(bn).eval(), R.SLOPE)
    with pytest.raises(_lib.DmcHipError):
        ops.bn_leaky(xi[:, :48], torch.nn.BatchNorm2d(48).to(DEV), R.SLOPE)


def test_contiguous_grad_output_gives_the_same_gradients():
    case = op_case()
    grads = []
    for fmt in (CL, torch.contiguous_format):
        bn = stock_module(case)
        xi = to4(case["z"], CL).requires_grad_(True)
        g = to4(case["dy"], fmt)
        assert g.is_contiguous(memory_format=fmt)
        ops.bn_leaky(xi, bn, R.SLOPE).backward(g)
        grads.append((xi.grad, bn.weight.grad, bn.bias.grad))
    for a, b in zip(*grads):
        assert torch.equal(a, b)


def test_frozen_operands_get_no_gradient():
    case = op_case()
    full = None
    for x_grad, g_grad, b_grad in ((True, True, True), (False, True, True), (True, False, True), (True, True, False), (True, False, False)):
        bn = stock_module(case)
        bn.weight.requires_grad_(g_grad)
        bn.bias.requires_grad_(b_grad)
        xi = to4(case["z"], CL).requires_grad_(x_grad)
        ops.bn_leaky(xi, bn, R.SLOPE).backward(to4(case["dy"], CL))
        got = (xi.grad, bn.weight.grad, bn.bias.grad)
        if full is None:
            full = got
        for have, want, asked in zip(got, full, (x_grad, g_grad, b_grad)):
            assert (have is None) == (not asked)
            assert have is None or torch.equal(have, want)


# ---------------------------------------------------------------------------------------------------------------------
# whole networks
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("att", [0, 1])
@pytest.mark.parametrize("ds,shape", [(0, (2, 5, 21, 17)), (0, (3, 5, 33, 18)), (16, (3, 5, 14, 14))], ids=["21x17", "33x18", "ds16-14x14"])
def test_whole_network_training_step_with_both_flags(att, ds, shape, monkeypatch):
    net = G.build_net(att, ds)
    x, r = G.rnd(G.INPUT_SEEDS[(att, ds, shape)], shape), G.rnd(52, (shape[0], 2) + tuple(shape[2:]))
    monkeypatch.setattr(model, "CTX_TRAIN", True)
    monkeypatch.setattr(model, "CTX_TRAIN_BN", True)
    margins = []
    ref = G.train_step(copy.deepcopy(net).double(), x.double(), r.double(), margins)  # CPU: the stock modules whatever the flags
    assert len(margins) == (8 if att else 7) and min(margins) >= G.KINK_MARGIN, margins
    net_dev = copy.deepcopy(net).to(DEV)
    ours = G.train_step(net_dev, x.to(DEV), r.to(DEV))
    monkeypatch.setattr(model, "CTX_TRAIN", False)
    monkeypatch.setattr(model, "CTX_TRAIN_BN", False)
    stock = G.train_step(net_dev, x.to(DEV), r.to(DEV))
    assert sorted(ours) == sorted(ref) == sorted(stock) and len(ours) > 40
    worst, bad = None, []
    for k in sorted(ref):
        if ref[k].dtype == torch.int64:                            # num_batches_tracked
            assert int(ours[k]) == int(ref[k]) == int(stock[k]) == 1, k
            continue
        assert tuple(ours[k].shape) == tuple(ref[k].shape), k
        e = float((ours[k].double().cpu() - ref[k]).abs().max())
        e_ref = float((stock[k].double().cpu() - ref[k]).abs().max())
        top = float(ref[k].abs().max())
        print("ctx train+bn att=%d ds=%d %s %-48s e %.3e e_ref %.3e max|ref| %.3e" % (att, ds, tuple(shape), k, e, e_ref, top))
        if worst is None or e / max(top, 1e-30) > worst[1] / max(worst[3], 1e-30):
            worst = (k, e, e_ref, top)
        if not e <= max(4 * e_ref, 2e-5 * top):
            bad.append((k, e, e_ref, top))
    print("ctx train+bn att=%d ds=%d %s worst: %s e %.3e e_ref %.3e max|ref| %.3e" % ((att, ds, tuple(shape)) + worst))
    assert not bad, bad


def step(net, x, r):
    """One forward + backward of ``net`` as it stands (G.train_step would put every module back into train())."""
    xi = x.clone().requires_grad_(True)
    outs = G.as_tuple(net(xi))
    sum((t * r).sum() for t in outs).backward()


@pytest.mark.parametrize("att", [0, 1])
def test_routes(att, monkeypatch):
    net = G.build_net(att, 0).to(DEV)
    x, r = G.rnd(51, (2, 5, 21, 17)).to(DEV), G.rnd(52, (2, 2, 21, 17)).to(DEV)
    stock_bn = []
    orig = torch.nn.BatchNorm2d.forward
    monkeypatch.setattr(torch.nn.BatchNorm2d, "forward", lambda self, t: (stock_bn.append(self.num_features), orig(self, t))[1])
    rec = G.Recorder(_lib.load())
    monkeypatch.setattr(_lib, "load", lambda: rec)
    monkeypatch.setattr(model, "CTX_TRAIN", True)
    monkeypatch.setattr(model, "CTX_TRAIN_BN", True)               # both flags
    step(copy.deepcopy(net).train(), x, r)
    assert rec.count("dmc_bnlrelu_fwd") == 6 and rec.count("dmc_bnlrelu_bwd") == 6, rec.names()
    assert rec.count("dmc_dconv_fwd") == 10 and rec.count("dmc_dconv_wgrad") == 5
    assert stock_bn == [2] * (2 if att else 1), stock_bn              # the head(s) alone
    assert [a[9] for nm, a in rec.calls if nm == "dmc_bnlrelu_fwd"] == [32, 128, 128, 96, 64, 32]
    del rec.calls[:], stock_bn[:]
    one = copy.deepcopy(net).train()                               # one middle BatchNorm in eval(): that unit alone stays stock
    one.conv_context[3][1].eval()
    before = copy.deepcopy(one.conv_context[3][1].state_dict())
    step(one, x, r)
    assert rec.count("dmc_bnlrelu_fwd") == 5 and rec.count("dmc_bnlrelu_bwd") == 5, rec.names()
    assert rec.count("dmc_dconv_fwd") == 10 and rec.count("dmc_dconv_wgrad") == 5
    assert stock_bn == [96] + [2] * (2 if att else 1), stock_bn
    for k, v in one.conv_context[3][1].state_dict().items():
        assert torch.equal(v, before[k]), k
    assert int(one.conv_context[2][1].num_batches_tracked) == 1
    del rec.calls[:], stock_bn[:]
    ev = copy.deepcopy(net).eval()                                 # eval() + no_grad: the eval route keeps precedence
    with torch.no_grad():
        ev(x)
    assert rec.names() and all(nm.startswith("dmc_ctx_") for nm in rec.names()), rec.names()
    assert stock_bn == []
    del rec.calls[:], stock_bn[:]
    monkeypatch.setattr(model, "CTX_TRAIN_BN", False)              # DMC_CTX_TRAIN=1 alone: as before
    step(copy.deepcopy(net).train(), x, r)
    assert not any(nm.startswith("dmc_bnlrelu_") for nm in rec.names()), rec.names()
    assert rec.count("dmc_dconv_fwd") == 10 and len(stock_bn) == (8 if att else 7)
    del rec.calls[:], stock_bn[:]
    monkeypatch.setattr(model, "CTX_TRAIN", False)                 # CTX_TRAIN_BN without CTX_TRAIN has no effect
    monkeypatch.setattr(model, "CTX_TRAIN_BN", True)
    step(copy.deepcopy(net).train(), x, r)
    assert rec.names() == [] and len(stock_bn) == (8 if att else 7)


# ---------------------------------------------------------------------------------------------------------------------
# the memory contract
# ---------------------------------------------------------------------------------------------------------------------
def bn_arena_case(M, C):
    def fn(a):
        lib = _lib.load()
        c = R.bn_case(M, C, R.OP_SEEDS[(M, C, "normal")])
        z, dy, gamma, beta = a.inp("z", c["z"]), a.inp("dy", c["dy"]), a.inp("gamma", c["gamma"]), a.inp("beta", c["beta"])
        rm, rv = a.inout("running_mean", c["rm"]), a.inout("running_var", c["rv"])
        stats = a.out("stats", (2 * C,))
        nbytes = lib.dmc_bnlrelu_scratch_bytes(M, C)
        a.call("dmc_bnlrelu_fwd", z, gamma, beta, rm, rv, a.out("y", (M, C)), stats, a.work("scratch_fwd", nbytes), M, C, R.SLOPE, R.EPS, R.MOMENTUM)
        a.call("dmc_bnlrelu_bwd", z, dy, gamma, beta, stats, a.work("scratch_bwd", nbytes), a.out("dz", (M, C)), a.out("dgamma", (C,)),
               a.out("dbeta", (C,)), M, C, R.SLOPE)
    return fn


def _bn_arena_check(M, C):
    def check(bufs):
        c = dev(R.bn_case(M, C, R.OP_SEEDS[(M, C, "normal")]))
        mean, var, invstd = R.stats_ref(c["z"])
        y64, t, _ = R.forward_ref(c["z"], c["gamma"], c["beta"], mean, invstd)
        dz, dgamma, dbeta = R.backward_ref(c["z"], c["dy"], c["gamma"], mean, invstd, t > 0)
        rm, rv = R.running_ref(mean, var, M, c["rm"], c["rv"])
        for name, ref in (("y", y64), ("dz", dz), ("dgamma", dgamma), ("dbeta", dbeta), ("running_mean", rm), ("running_var", rv)):
            assert err(bufs[name].t, ref) <= 1e-5 * float(ref.abs().max()), name
    return check


def refused_fwd_case(a):       # 48 channels: refused, nothing written
    M, C = 64, 48
    a.call("dmc_bnlrelu_fwd", a.inp("z", torch.zeros(M, C)), a.inp("gamma", torch.ones(C)), a.inp("beta", torch.zeros(C)),
           a.inout("running_mean", torch.zeros(C)), a.inout("running_var", torch.ones(C)), a.out("y", (M, C)), a.out("stats", (2 * C,)),
           a.work("scratch", 1 << 16), M, C, R.SLOPE, R.EPS, R.MOMENTUM)


def refused_bwd_case(a):       # slope 1: refused, nothing written
    M, C = 64, 32
    a.call("dmc_bnlrelu_bwd", a.inp("z", torch.zeros(M, C)), a.inp("dy", torch.zeros(M, C)), a.inp("gamma", torch.ones(C)),
           a.inp("beta", torch.zeros(C)), a.inp("stats", torch.ones(2 * C)), a.work("scratch", 1 << 16), a.out("dz", (M, C)),
           a.out("dgamma", (C,)), a.out("dbeta", (C,)), M, C, 1.0)


ARENA_CASES = []
for _m, _c in ((1188, 96), (105, 128)):
    ARENA_CASES.append(abi_cases.Case(abi_cases.tag("dmc_bnlrelu", _m, _c), ["dmc_bnlrelu_fwd", "dmc_bnlrelu_bwd"], bn_arena_case(_m, _c),
                                      check=_bn_arena_check(_m, _c), capacity=32 << 20))
ARENA_CASES.append(abi_cases.Case("dmc_bnlrelu_fwd-refused-width-48", ["dmc_bnlrelu_fwd"], refused_fwd_case, expect_rc=abi_cases.DMC_E_INVALID,
                                  capacity=32 << 20))
ARENA_CASES.append(abi_cases.Case("dmc_bnlrelu_bwd-refused-slope-1", ["dmc_bnlrelu_bwd"], refused_bwd_case, expect_rc=abi_cases.DMC_E_INVALID,
                                  capacity=32 << 20))
_known = {c.id for c in abi_cases.CASES}
abi_cases.CASES.extend(c for c in ARENA_CASES if c.id not in _known)


@pytest.mark.parametrize("case", ARENA_CASES, ids=[c.id for c in ARENA_CASES])
def test_bnlrelu_entries_memory_contract(case):
    try:
        bufs = run_case(case.fn, device=DEV, capacity=case.capacity, expect_rc=case.expect_rc)
        if case.check is not None:
            case.check(bufs)
    except RuntimeError as e:
        if "HIP error" in str(e) or "illegal memory access" in str(e):
            # a faulted device serves nothing more: end the session here instead of launching the remaining cases on it
            pytest.exit("GPU fault in %s: %s" % (case.id, str(e).splitlines()[0]), returncode=3)
        raise
