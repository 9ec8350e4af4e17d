"""GPU: the two ends of the ContextNetwork training route (csrc/ctx_ends.hip, ops.ctx_first_conv, ops.ctx_head_convs,
ops.bn_leaky_planes, model.CTX_TRAIN_ENDS).

Convolutions, through the C ABI with every output prefilled with NaN and the workspace at exactly the reported size, on
ctx_ends_ref.SHAPES: the six passes against fp64 stock convolutions at rel_err < 1e-5 (the bar of tests/test_dconv_gpu.py; these
are exact fp32 sums and sit far inside it), each run twice and bit-equal; on (1, 1, 1) the eight outer taps of both weight
gradients are exactly 0 and written; a frame alone and in a batch is bit-identical; the heads' data gradient is the fp64 sum of
both heads, and with one dz NULL the other head's alone.  The weight-gradient range is 2048 pixels (the issue suggested 8192):
(3, 61, 47), M = 8601, crosses it four times and leaves a partial last range.  The BatchNorm kernels do not cap their grid (a
thread owns four elements, no stride), so there is no second-stride case.

One arithmetic for train and eval: dmc_ctx_first_eval / dmc_ctx_heads_eval with mean 0, invstd 1, gamma 1, beta 0 return exactly
the LeakyReLU (and max(., 0) on the attention head) of dmc_ctxends_first_fwd / dmc_ctxends_heads_fwd, bit for bit.

The planes' BatchNorm by the rules and bars of tests/test_ctx_bn_gpu.py (its judge()), with relu 0 and 1; the autograd ops; the
whole networks with all three flags (cases, seeds and bar of tests/test_dconv_gpu.py); the dispatch; every launching entry point
in guarded arenas (tests/abi_arena.py).  Every figure is printed before it is asserted."""
import copy

import pytest
import torch

from dmcnet_amd import _lib, model, ops
from tests import abi_cases
from tests import ctx_bn_ref as R
from tests import ctx_ends_ref as E
from tests import test_ctx_bn_gpu as B
from tests import test_dconv_gpu as G
from tests.abi_arena import run_case

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U8 = torch.uint8
CL = torch.channels_last
U = R.U32
NAN = float("nan")
IDS = ["x".join(map(str, s)) for s in E.SHAPES]
BN_IDS = ["x".join(map(str, s)) for s in E.BN_SHAPES]
rel_err, nhwc, nchw = G.rel_err, G.nhwc, G.nchw


def P(t):
    return _lib.ptr(t)


def nan(*shape):
    return torch.full(shape, NAN, dtype=torch.float32, device=DEV)


def work(nbytes):
    return torch.full((nbytes,), 0xFF, dtype=U8, device=DEV)


def ok(rc, what):
    _lib.check(rc, what)


# ---- the six passes through the C ABI: x, dx NCHW; z, dz, t, dt NHWC; head planes NCHW; w_first OIHW; head weights OHWI
def first_fwd(x, w, n, h, wd):
    z = nan(n, h, wd, 32)
    ok(_lib.load().dmc_ctxends_first_fwd(P(x), P(w), P(z), n, h, wd, ops._stream()), "dmc_ctxends_first_fwd")
    return z


def first_dgrad(dz, w, n, h, wd):
    dx = nan(n, 5, h, wd)
    ok(_lib.load().dmc_ctxends_first_dgrad(P(dz), P(w), P(dx), n, h, wd, ops._stream()), "dmc_ctxends_first_dgrad")
    return dx


def first_wgrad(x, dz, n, h, wd):
    lib = _lib.load()
    dw = nan(32, 5, 3, 3)
    ok(lib.dmc_ctxends_first_wgrad(P(x), P(dz), P(dw), P(work(lib.dmc_ctxends_wgrad_workspace_bytes(n, h, wd, 5))), n, h, wd, ops._stream()),
       "dmc_ctxends_first_wgrad")
    return dw


def heads_fwd(t, ws, n, h, wd):
    zs = [nan(n, 2, h, wd) for _ in ws] + [None]
    ws = list(ws) + [None]
    ok(_lib.load().dmc_ctxends_heads_fwd(P(t), P(ws[0]), P(ws[1]), P(zs[0]), P(zs[1]), n, h, wd, ops._stream()), "dmc_ctxends_heads_fwd")
    return zs[:len(ws) - 1]


def heads_dgrad(dzs, ws, n, h, wd):
    dt = nan(n, h, wd, 32)
    ok(_lib.load().dmc_ctxends_heads_dgrad(P(dzs[0]), P(dzs[1]), P(ws[0]), P(ws[1]), P(dt), n, h, wd, ops._stream()), "dmc_ctxends_heads_dgrad")
    return dt


def heads_wgrad(t, dzs, n, h, wd):
    lib = _lib.load()
    dws = [nan(2, 3, 3, 32) if d is not None else None for d in dzs]
    planes = 2 * sum(d is not None for d in dzs)
    ok(lib.dmc_ctxends_heads_wgrad(P(t), P(dzs[0]), P(dzs[1]), P(dws[0]), P(dws[1]), P(work(lib.dmc_ctxends_wgrad_workspace_bytes(n, h, wd, planes))),
                                   n, h, wd, ops._stream()), "dmc_ctxends_heads_wgrad")
    return dws


def first_dev(shape):
    c = E.first_case(*shape)
    return c, c["x"].to(DEV), c["w"].to(DEV), nhwc(c["dz"]).to(DEV)


def heads_dev(shape):
    c = E.heads_case(*shape)
    return c, nhwc(c["t"]).to(DEV), [nhwc(w).to(DEV) for w in c["w"]], [d.to(DEV) for d in c["dz"]]


@pytest.mark.parametrize("shape", E.SHAPES, ids=IDS)
def test_six_passes_vs_fp64(shape):
    n, h, w = shape
    assert _lib.load().dmc_ctxends_supported(n, h, w) == 1
    c, x, wt, dz = first_dev(shape)
    hc, t, ws, dzs = heads_dev(shape)
    runs = []
    for _ in range(2):
        z, dx, dw = first_fwd(x, wt, *shape), first_dgrad(dz, wt, *shape), first_wgrad(x, dz, *shape)
        zh, dt, dwh = heads_fwd(t, ws, *shape), heads_dgrad(dzs, ws, *shape), heads_wgrad(t, dzs, *shape)
        runs.append([z, dx, dw] + zh + [dt] + dwh)
    for a, b in zip(*runs):                                        # run to run
        assert not bool(torch.isnan(a).any()) and torch.equal(a, b)
    z, dx, dw, zf, za, dt, dwf, dwa = runs[0]
    e = dict(first_fwd=rel_err(nchw(z), c["z"]), first_dgrad=rel_err(dx, c["dx"]), first_wgrad=rel_err(dw, c["dw"]),
             heads_fwd_flow=rel_err(zf, hc["z"][0]), heads_fwd_att=rel_err(za, hc["z"][1]),
             heads_dgrad=rel_err(nchw(dt), hc["dt"][0] + hc["dt"][1]),
             heads_wgrad_flow=rel_err(nchw(dwf), hc["dw"][0]), heads_wgrad_att=rel_err(nchw(dwa), hc["dw"][1]))
    # one head alone: the forward, and a NULL dz (that head got no gradient) in the gradients
    (zf1,) = heads_fwd(t, ws[:1], *shape)
    assert torch.equal(zf1, zf)
    for k in range(2):
        only = [dzs[0] if k == 0 else None, dzs[1] if k == 1 else None]
        dt1 = heads_dgrad(only, ws, *shape)
        e["heads_dgrad_only%d" % k] = rel_err(nchw(dt1), hc["dt"][k])
        assert torch.equal(dt1, heads_dgrad([dzs[k], None], [ws[k], None], *shape))      # the one-head network's launch
        dw1 = heads_wgrad(t, only, *shape)
        assert dw1[1 - k] is None and torch.equal(dw1[k], (dwf, dwa)[k])
    print("ctxends %s: rel_err %s" % (shape, ", ".join("%s %.3e" % kv for kv in sorted(e.items()))))
    assert all(v < 1e-5 for v in e.values()), e
    if shape == (1, 1, 1):                                         # no pixel has a neighbour: the outer taps are exactly 0, and written
        centre = torch.zeros(3, 3, dtype=torch.bool)
        centre[1, 1] = True
        assert bool((c["dw"][:, :, ~centre] == 0).all()) and bool((dw.cpu()[:, :, ~centre] == 0).all()) and bool((dw[:, :, 1, 1] != 0).any())
        for d in (dwf, dwa):
            assert bool((d.cpu()[:, ~centre, :] == 0).all()) and bool((d[:, 1, 1, :] != 0).any())


def test_the_weight_gradient_ranges_are_in_play():
    lib = _lib.load()
    assert lib.dmc_ctxends_wgrad_workspace_bytes(3, 61, 47, 5) == 5 * 5 * 288 * 4        # five ranges of 2048, the last of 409 pixels
    assert lib.dmc_ctxends_wgrad_workspace_bytes(2, 33, 18, 5) == 5 * 288 * 4
    assert lib.dmc_ctxends_bn_scratch_bytes(2, 21, 17) == 2 * 32 + 16 and 2 * 714 % E.BN_TILE != 0   # a partial second workgroup


def test_frame_results_are_independent_of_the_batch():
    shape = (2, 21, 17)
    n, h, w = shape
    c, x, wt, dz = first_dev(shape)
    hc, t, ws, dzs = heads_dev(shape)
    z, dx = first_fwd(x, wt, *shape), first_dgrad(dz, wt, *shape)
    zh, dt = heads_fwd(t, ws, *shape), heads_dgrad(dzs, ws, *shape)
    for f in range(n):
        s = slice(f, f + 1)
        assert torch.equal(z[s], first_fwd(x[s].contiguous(), wt, 1, h, w)), f
        assert torch.equal(dx[s], first_dgrad(dz[s].contiguous(), wt, 1, h, w)), f
        z1 = heads_fwd(t[s].contiguous(), ws, 1, h, w)
        assert torch.equal(zh[0][s], z1[0]) and torch.equal(zh[1][s], z1[1]), f
        assert torch.equal(dt[s], heads_dgrad([d[s].contiguous() for d in dzs], ws, 1, h, w)), f


@pytest.mark.parametrize("shape", [(2, 21, 17), (2, 33, 18)], ids=["2x21x17", "2x33x18"])
def test_train_and_eval_share_one_arithmetic(shape):
    n, h, w = shape
    lib = _lib.load()
    c, x, wt, _ = first_dev(shape)
    hc, t, ws, _ = heads_dev(shape)
    slope = torch.tensor(0.1, dtype=torch.float32, device=DEV)

    def leaky(z):
        return torch.where(z > 0, z, slope * z)

    one, zero = torch.ones(32, device=DEV), torch.zeros(32, device=DEV)
    y = nan(n, h, w, 32)
    ok(lib.dmc_ctx_first_eval(P(x), P(wt), P(torch.cat([zero, one])), P(one), P(zero), P(y), n, h, w, ops._stream()), "dmc_ctx_first_eval")
    assert torch.equal(y, leaky(first_fwd(x, wt, *shape)))
    st = torch.tensor([0.0, 0.0, 1.0, 1.0], device=DEV)
    flow, att = nan(n, 2, h, w), nan(n, 2, h, w)
    ok(lib.dmc_ctx_heads_eval(P(t), P(ws[0]), P(st), P(one), P(zero), P(ws[1]), P(st), P(one), P(zero), P(flow), P(att), n, h, w, ops._stream()),
       "dmc_ctx_heads_eval")
    zf, za = heads_fwd(t, ws, *shape)
    assert torch.equal(flow, leaky(zf)) and torch.equal(att, leaky(za).clamp_min(0.0))
    flow1 = nan(n, 2, h, w)
    ok(lib.dmc_ctx_heads_eval(P(t), P(ws[0]), P(st), P(one), P(zero), None, None, None, None, P(flow1), None, n, h, w, ops._stream()),
       "dmc_ctx_heads_eval")
    assert torch.equal(flow1, leaky(heads_fwd(t, ws[:1], *shape)[0]))
    assert float(y.abs().max()) > 0 and bool((y < 0).any()) and bool((att == 0).any()) and bool((att > 0).any())


# ---------------------------------------------------------------------------------------------------------------------
# the planes' BatchNorm + LeakyReLU (+ ReLU)
# ---------------------------------------------------------------------------------------------------------------------
def bn_dev(case):
    n, h, w = case["frames"]
    c = {k: (v.to(DEV) if torch.is_tensor(v) else v) for k, v in case.items()}
    c["zp"], c["dyp"] = E.to_planes(c["z"], n, h, w), E.to_planes(c["dy"], n, h, w)
    return c


def bn_fwd(c, relu, running=True):
    n, h, w = c["frames"]
    lib = _lib.load()
    y, stats = nan(n, 2, h, w), nan(4)
    rm, rv = (c["rm"].clone(), c["rv"].clone()) if running else (None, None)
    ok(lib.dmc_ctxends_bn_fwd(P(c["zp"]), P(c["gamma"]), P(c["beta"]), P(rm), P(rv), P(y), P(stats), P(work(lib.dmc_ctxends_bn_scratch_bytes(n, h, w))),
                              n, h, w, E.SLOPE, E.EPS, E.MOMENTUM, relu, ops._stream()), "dmc_ctxends_bn_fwd")
    return dict(y=y, stats=stats, mean=stats[:2], invstd=stats[2:], rm=rm, rv=rv)


def bn_bwd(c, stats, relu):
    n, h, w = c["frames"]
    lib = _lib.load()
    dz, dgamma, dbeta = nan(n, 2, h, w), nan(2), nan(2)
    ok(lib.dmc_ctxends_bn_bwd(P(c["zp"]), P(c["dyp"]), P(c["gamma"]), P(c["beta"]), P(stats), P(work(lib.dmc_ctxends_bn_scratch_bytes(n, h, w))),
                              P(dz), P(dgamma), P(dbeta), n, h, w, E.SLOPE, relu, ops._stream()), "dmc_ctxends_bn_bwd")
    return dict(dz=dz, dgamma=dgamma, dbeta=dbeta)


def stock_module(c):
    bn = torch.nn.BatchNorm2d(2, eps=E.EPS, momentum=E.MOMENTUM).to(DEV).train()
    with torch.no_grad():
        bn.weight.copy_(c["gamma"]); bn.bias.copy_(c["beta"]); bn.running_mean.copy_(c["rm"]); bn.running_var.copy_(c["rv"])
    return bn


def stock_step(c, relu):
    """The stock fp32 modules on the same device, on the same planes: rows [M][2] of y, dz; dgamma, dbeta, rm, rv."""
    bn = stock_module(c)
    x4 = c["zp"].clone().requires_grad_(True)
    y4 = torch.nn.LeakyReLU(E.SLOPE, inplace=True)(bn(x4))
    if relu:
        y4 = torch.nn.ReLU()(y4)
    y4.backward(c["dyp"])
    return dict(y=E.to_rows(y4.detach()), dz=E.to_rows(x4.grad), dgamma=bn.weight.grad, dbeta=bn.bias.grad, rm=bn.running_mean.detach(),
                rv=bn.running_var.detach())


def check_bn_case(tag, c, relu, crafted_channel=None):
    n, h, w = c["frames"]
    M = n * h * w
    bad = []
    f = bn_fwd(c, relu)
    for t in f.values():
        assert not bool(torch.isnan(t).any())
    st = stock_step(c, relu)
    z, dy = c["z"], c["dy"]
    # 1. statistics
    mean, var, invstd = R.stats_ref(z)
    _, sm, si = torch.native_batch_norm(c["zp"], c["gamma"], c["beta"], c["rm"].clone(), c["rv"].clone(), True, E.MOMENTUM, E.EPS)
    B.judge(tag, "mean", f["mean"], mean, sm, 4, bad, per_channel=True)
    B.judge(tag, "invstd", f["invstd"], invstd, si, 4, bad, per_channel=True)
    rm, rv = R.running_ref(mean, var, M, c["rm"], c["rv"])
    B.judge(tag, "run_mean", f["rm"], rm, st["rm"], 4, bad, per_channel=True)
    B.judge(tag, "run_var", f["rv"], rv, st["rv"], 4, bad, per_channel=True)
    # 2. apply, on the stored statistics
    y = E.to_rows(f["y"])
    y64, _, xh = E.forward_ref(z, c["gamma"], c["beta"], f["mean"], f["invstd"], relu)
    bound = 4 * U * ((c["gamma"].double() * xh).abs() + c["beta"].double().abs())
    ey = (y.double() - y64).abs()
    print("ctxends bn %-22s y        worst |y - y64| / bound %.3f" % (tag, float((ey / bound.clamp_min(1e-300)).max())))
    assert bool((ey <= bound).all()), float((ey / bound.clamp_min(1e-300)).max())
    # 3. sign agreement with the fp64 reference (y > 0 exactly where t > 0, with and without the ReLU)
    _, t_ref, _ = E.forward_ref(z, c["gamma"], c["beta"], mean, invstd, relu)
    pos = y > 0
    assert torch.equal(pos, t_ref > 0)
    if relu:
        assert bool((y >= 0).all()) and bool((y[~pos] == 0).all())
    # 4. backward, mask from the kernel's own y
    b = bn_bwd(c, f["stats"], relu)
    for t in b.values():
        assert not bool(torch.isnan(t).any())
    dz, dgamma, dbeta = E.backward_ref(z, dy, c["gamma"], mean, invstd, pos, relu)
    B.judge(tag, "dz", E.to_rows(b["dz"]), dz, st["dz"], 8, bad)
    B.judge(tag, "dgamma", b["dgamma"], dgamma, st["dgamma"], 8, bad)
    B.judge(tag, "dbeta", b["dbeta"], dbeta, st["dbeta"], 8, bad)
    if crafted_channel is not None:
        k = crafted_channel
        zero = z[:, k] == 0
        assert int(zero.sum()) == M // 3
        assert float(f["mean"][k]) == 0.0 and bool((y[:, k][zero] == 0).all())
        # the zeros took the lower branch (slope, or 0 under the ReLU): against the reference that lets them pass with 1 the error
        # is of the size of the gradient
        got = E.to_rows(b["dz"])[:, k][zero].double()
        e_low = float((got - dz[:, k][zero]).abs().max())
        dz1, _, _ = E.backward_ref(z, dy, c["gamma"], mean, invstd, t_ref >= 0, relu)
        e_one = float((got - dz1[:, k][zero]).abs().max())
        print("ctxends bn %-22s zeros: |dz - ref(lower branch)| %.3e, |dz - ref(1)| %.3e" % (tag, e_low, e_one))
        assert e_low <= 8 * U * float(dz.abs().max()) and e_one > 1e-2
    # 5. run to run
    f2, b2 = bn_fwd(c, relu), bn_bwd(c, f["stats"], relu)
    for k in ("y", "stats", "rm", "rv"):
        assert torch.equal(f[k], f2[k]), k
    for k in b:
        assert torch.equal(b[k], b2[k]), k
    f3 = bn_fwd(c, relu, running=False)                            # without running pointers: the same statistics and values
    assert torch.equal(f3["y"], f["y"]) and torch.equal(f3["stats"], f["stats"])
    assert not bad, bad


@pytest.mark.parametrize("relu", [0, 1])
@pytest.mark.parametrize("shape", E.BN_SHAPES, ids=BN_IDS)
def test_planes_batchnorm_vs_fp64(shape, relu):
    check_bn_case("%s relu=%d" % ("x".join(map(str, shape)), relu), bn_dev(E.bn_case(*shape)), relu)


@pytest.mark.parametrize("relu", [0, 1])
def test_zeros_of_the_batchnorm_output_take_the_lower_branch(relu):
    check_bn_case("2x33x18-crafted relu=%d" % relu, bn_dev(E.crafted_case()), relu, crafted_channel=1)


# ---------------------------------------------------------------------------------------------------------------------
# the autograd ops
# ---------------------------------------------------------------------------------------------------------------------
OP = (2, 21, 17)


def test_first_conv_op_vs_fp64():
    n, h, w = OP
    c = E.first_case(*OP)
    xi = c["x"].to(DEV).requires_grad_(True)
    wi = c["w"].to(DEV).requires_grad_(True)
    conv = torch.nn.Conv2d(5, 32, 3, 1, 1, 1, bias=False).to(DEV)
    assert ops.ctx_first_conv_supported(xi, conv)
    y = ops.ctx_first_conv(xi, wi)
    assert tuple(y.shape) == (n, 32, h, w) and y.is_contiguous(memory_format=CL)
    y.backward(c["dz"].to(DEV).contiguous(memory_format=CL))
    assert xi.grad.stride() == xi.stride() and wi.grad.stride() == wi.stride()
    e = (rel_err(y, c["z"]), rel_err(xi.grad, c["dx"]), rel_err(wi.grad, c["dw"]))
    print("ops.ctx_first_conv %s: rel_err value %.3e, x.grad %.3e, weight.grad %.3e" % ((OP,) + e))
    assert max(e) < 1e-5, e
    # a channels_last input and weight, a contiguous grad_output: the same bits, the weight gradient in the weight's strides
    x2 = c["x"].to(DEV).contiguous(memory_format=CL).requires_grad_(True)
    w2 = c["w"].to(DEV).contiguous(memory_format=CL).requires_grad_(True)
    y2 = ops.ctx_first_conv(x2, w2)
    y2.backward(c["dz"].to(DEV))
    assert torch.equal(y2, y) and torch.equal(x2.grad, xi.grad) and torch.equal(w2.grad, wi.grad)
    assert w2.grad.stride() == w2.stride() != wi.stride()
    assert not ops.ctx_first_conv_supported(xi.cpu(), conv) and not ops.ctx_first_conv_supported(xi.double(), conv)
    assert not ops.ctx_first_conv_supported(xi, torch.nn.Conv2d(5, 32, 3, 1, 1, 1, bias=True).to(DEV))
    assert not ops.ctx_first_conv_supported(xi, torch.nn.Conv2d(5, 32, 3, 1, 2, 2, bias=False).to(DEV))
    assert not ops.ctx_first_conv_supported(xi, torch.nn.Conv2d(5, 64, 3, 1, 1, 1, bias=False).to(DEV))
    with pytest.raises(_lib.DmcHipError):
        ops.ctx_first_conv(xi, torch.zeros(64, 5, 3, 3, device=DEV))


def test_head_convs_op_vs_fp64():
    n, h, w = OP
    c = E.heads_case(*OP)
    ti = c["t"].to(DEV).contiguous(memory_format=CL).requires_grad_(True)
    wis = [wt.to(DEV).requires_grad_(True) for wt in c["w"]]
    convs = [torch.nn.Conv2d(32, 2, 3, 1, 1, 1, bias=False).to(DEV) for _ in range(2)]
    assert ops.ctx_head_convs_supported(ti, convs) and ops.ctx_head_convs_supported(ti, convs[:1])
    zs = ops.ctx_head_convs(ti, wis)
    assert len(zs) == 2 and all(tuple(z.shape) == (n, 2, h, w) and z.is_contiguous() for z in zs)
    sum((z * d.to(DEV)).sum() for z, d in zip(zs, c["dz"])).backward()
    e = [rel_err(zs[0], c["z"][0]), rel_err(zs[1], c["z"][1]), rel_err(ti.grad, c["dt"][0] + c["dt"][1]),
         rel_err(wis[0].grad, c["dw"][0]), rel_err(wis[1].grad, c["dw"][1])]
    print("ops.ctx_head_convs %s: rel_err values %.3e %.3e, t.grad %.3e, weight.grad %.3e %.3e" % ((OP,) + tuple(e)))
    assert max(e) < 1e-5, e
    assert all(wi.grad.stride() == wi.stride() for wi in wis) and ti.grad.is_contiguous(memory_format=CL)
    # channels_last weights and grad_outputs, a contiguous input: the same bits
    t2 = c["t"].to(DEV).requires_grad_(True)
    w2 = [wt.to(DEV).contiguous(memory_format=CL).requires_grad_(True) for wt in c["w"]]
    z2 = ops.ctx_head_convs(t2, w2)
    torch.autograd.backward(z2, [d.to(DEV).contiguous(memory_format=CL) for d in c["dz"]])
    assert torch.equal(z2[0], zs[0]) and torch.equal(z2[1], zs[1]) and torch.equal(t2.grad, ti.grad)
    for a, b in zip(w2, wis):
        assert a.grad.stride() == a.stride() != b.stride() and torch.equal(a.grad, b.grad)
    # one head's output unused: the other head's gradients alone
    t3 = c["t"].to(DEV).requires_grad_(True)
    w3 = [wt.to(DEV).requires_grad_(True) for wt in c["w"]]
    z3 = ops.ctx_head_convs(t3, w3)
    (z3[1] * c["dz"][1].to(DEV)).sum().backward()
    assert w3[0].grad is None and torch.equal(w3[1].grad, wis[1].grad) and rel_err(t3.grad, c["dt"][1]) < 1e-5
    (z1,) = ops.ctx_head_convs(ti.detach(), wis[:1])
    assert torch.equal(z1, zs[0])
    assert not ops.ctx_head_convs_supported(ti.cpu(), convs) and not ops.ctx_head_convs_supported(ti, convs + convs[:1])
    assert not ops.ctx_head_convs_supported(ti, [torch.nn.Conv2d(32, 2, 3, 1, 1, 1, bias=True).to(DEV)])
    with pytest.raises(_lib.DmcHipError):
        ops.ctx_head_convs(ti, [torch.zeros(4, 32, 3, 3, device=DEV)])


def test_conv_ops_launch_only_what_is_needed(monkeypatch):
    c, hc = E.first_case(*OP), E.heads_case(*OP)
    rec = G.Recorder(_lib.load())
    monkeypatch.setattr(_lib, "load", lambda: rec)
    dz = c["dz"].to(DEV).contiguous(memory_format=CL)

    def first(x_grad, w_grad):
        del rec.calls[:]
        xi, wi = c["x"].to(DEV).requires_grad_(x_grad), c["w"].to(DEV).requires_grad_(w_grad)
        ops.ctx_first_conv(xi, wi).backward(dz)
        return xi.grad, wi.grad, [rec.count("dmc_ctxends_first_" + k) for k in ("fwd", "dgrad", "wgrad")]

    gx, gw, n = first(True, True)
    assert n == [1, 1, 1]
    gx2, gw2, n = first(False, True)
    assert gx2 is None and n == [1, 0, 1] and torch.equal(gw2, gw)
    gx3, gw3, n = first(True, False)
    assert gw3 is None and n == [1, 1, 0] and torch.equal(gx3, gx)

    def heads(t_grad, w_grads):
        del rec.calls[:]
        ti = hc["t"].to(DEV).contiguous(memory_format=CL).requires_grad_(t_grad)
        wis = [wt.to(DEV).requires_grad_(g) for wt, g in zip(hc["w"], w_grads)]
        zs = ops.ctx_head_convs(ti, wis)
        torch.autograd.backward(zs, [d.to(DEV) for d in hc["dz"]])
        planes = [a[3] for nm, a in rec.calls if nm == "dmc_ctxends_wgrad_workspace_bytes"]
        return ti.grad, [wi.grad for wi in wis], [rec.count("dmc_ctxends_heads_" + k) for k in ("fwd", "dgrad", "wgrad")], planes

    gt, gws, n, _ = heads(True, (True, True))
    assert n == [1, 1, 1]
    gt2, gws2, n, _ = heads(False, (True, True))
    assert gt2 is None and n == [1, 0, 1] and all(torch.equal(a, b) for a, b in zip(gws2, gws))
    gt3, gws3, n, _ = heads(True, (False, False))
    assert gws3 == [None, None] and n == [1, 1, 0] and torch.equal(gt3, gt)
    gt4, gws4, n, planes = heads(True, (False, True))                 # one frozen head: a two-plane weight gradient
    assert gws4[0] is None and n == [1, 1, 1] and torch.equal(gws4[1], gws[1]) and torch.equal(gt4, gt) and planes == [2]
    nulls = [[a[i].value is None for i in (1, 2, 3, 4)] for nm, a in rec.calls if nm == "dmc_ctxends_heads_wgrad"]
    assert nulls == [[False, True, False, True]], nulls


@pytest.mark.parametrize("relu", [False, True])
def test_bn_leaky_planes_op_vs_fp64_and_stock(relu):
    n, h, w = OP
    case = bn_dev(E.bn_case(*OP))
    M = n * h * w
    bn, lrelu = stock_module(case), torch.nn.LeakyReLU(E.SLOPE)
    zi = case["zp"].contiguous(memory_format=CL).requires_grad_(True)      # the op makes it contiguous itself
    assert ops.bn_leaky_planes_supported(zi, bn, lrelu, torch.nn.ReLU() if relu else None)
    y = ops.bn_leaky_planes(zi, bn, E.SLOPE, relu)
    assert tuple(y.shape) == (n, 2, h, w) and y.is_contiguous()
    y.backward(case["dyp"])
    assert int(bn.num_batches_tracked) == 1
    st = stock_step(case, relu)
    mean, var, invstd = R.stats_ref(case["z"])
    y64, t_ref, _ = E.forward_ref(case["z"], case["gamma"], case["beta"], mean, invstd, relu)
    assert torch.equal(E.to_rows(y.detach()) > 0, t_ref > 0)
    dz, dgamma, dbeta = E.backward_ref(case["z"], case["dy"], case["gamma"], mean, invstd, t_ref > 0, relu)
    rm, rv = R.running_ref(mean, var, M, case["rm"], case["rv"])
    bad, tag = [], "ops.bn_leaky_planes r=%d" % relu
    B.judge(tag, "y", E.to_rows(y.detach()), y64, st["y"], 8, bad)
    B.judge(tag, "z.grad", E.to_rows(zi.grad), dz, st["dz"], 8, bad)
    B.judge(tag, "dgamma", bn.weight.grad, dgamma, st["dgamma"], 8, bad)
    B.judge(tag, "dbeta", bn.bias.grad, dbeta, st["dbeta"], 8, bad)
    B.judge(tag, "run_mean", bn.running_mean, rm, st["rm"], 4, bad, per_channel=True)
    B.judge(tag, "run_var", bn.running_var, rv, st["rv"], 4, bad, per_channel=True)
    assert not bad, bad
    # a channels_last grad_output: the same bits; frozen operands get None
    full = (zi.grad, bn.weight.grad, bn.bias.grad)
    for z_grad, g_grad, b_grad, fmt in ((True, True, True, CL), (False, True, True, None), (True, False, False, None)):
        bn2 = stock_module(case)
        bn2.weight.requires_grad_(g_grad); bn2.bias.requires_grad_(b_grad)
        z2 = case["zp"].clone().requires_grad_(z_grad)
        ops.bn_leaky_planes(z2, bn2, E.SLOPE, relu).backward(case["dyp"].contiguous(memory_format=fmt) if fmt is not None else case["dyp"])
        for have, want, asked in zip((z2.grad, bn2.weight.grad, bn2.bias.grad), full, (z_grad, g_grad, b_grad)):
            assert (have is None) == (not asked) and (have is None or torch.equal(have, want))
    assert not ops.bn_leaky_planes_supported(zi.cpu(), bn, lrelu) and not ops.bn_leaky_planes_supported(zi, copy.deepcopy(bn).eval(), lrelu)
    assert not ops.bn_leaky_planes_supported(zi, bn, torch.nn.ReLU()) and not ops.bn_leaky_planes_supported(zi, bn, lrelu, torch.nn.Sigmoid())
    assert not ops.bn_leaky_planes_supported(zi[:1, :, :1, :1], bn, lrelu)                 # N H W = 1
    assert not ops.bn_leaky_planes_supported(torch.zeros(2, 32, 3, 3, device=DEV), torch.nn.BatchNorm2d(32).to(DEV), lrelu)
    with pytest.raises(_lib.DmcHipError):
        ops.bn_leaky_planes(zi, copy.deepcopy(bn).eval(), E.SLOPE)


# ---------------------------------------------------------------------------------------------------------------------
# whole networks
# ---------------------------------------------------------------------------------------------------------------------
FLAGS = ("CTX_TRAIN", "CTX_TRAIN_BN", "CTX_TRAIN_ENDS")


@pytest.mark.parametrize("att", [0, 1])
@pytest.mark.parametrize("ds,shape", [(0, (2, 5, 21, 17)), (0, (3, 5, 33, 18)), (16, (3, 5, 14, 14))], ids=["21x17", "33x18", "ds16-14x14"])
def test_whole_network_training_step_with_all_three_flags(att, ds, shape, monkeypatch):
    net = G.build_net(att, ds)
    x, r = G.rnd(G.INPUT_SEEDS[(att, ds, shape)], shape), G.rnd(52, (shape[0], 2) + tuple(shape[2:]))
    for flag in FLAGS:
        monkeypatch.setattr(model, flag, True)
    margins = []
    ref = G.train_step(copy.deepcopy(net).double(), x.double(), r.double(), margins)  # CPU: the stock modules whatever the flags
    assert len(margins) == (8 if att else 7) and min(margins) >= G.KINK_MARGIN, margins       # the heads' BatchNorms included
    net_dev = copy.deepcopy(net).to(DEV)
    ours = G.train_step(net_dev, x.to(DEV), r.to(DEV))
    for flag in FLAGS:
        monkeypatch.setattr(model, flag, False)
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
        print("ctx train+bn+ends att=%d ds=%d %s %-48s e %.3e e_ref %.3e max|ref| %.3e" % (att, ds, tuple(shape), k, e, e_ref, top))
        if worst is None or e / max(top, 1e-30) > worst[1] / max(worst[3], 1e-30):
            worst = (k, e, e_ref, top)
        if not e <= max(4 * e_ref, 2e-5 * top):
            bad.append((k, e, e_ref, top))
    print("ctx train+bn+ends att=%d ds=%d %s worst: %s e %.3e e_ref %.3e max|ref| %.3e" % ((att, ds, tuple(shape)) + worst))
    assert not bad, bad


@pytest.mark.parametrize("att", [0, 1])
def test_routes(att, monkeypatch):
    net = G.build_net(att, 0).to(DEV)
    x, r = G.rnd(51, (2, 5, 21, 17)).to(DEV), G.rnd(52, (2, 2, 21, 17)).to(DEV)
    stock_bn, stock_conv = [], []
    orig_bn, orig_conv = torch.nn.BatchNorm2d.forward, torch.nn.Conv2d._conv_forward
    monkeypatch.setattr(torch.nn.BatchNorm2d, "forward", lambda self, t: (stock_bn.append(self.num_features), orig_bn(self, t))[1])
    monkeypatch.setattr(torch.nn.Conv2d, "_conv_forward", lambda self, t, w, b: (stock_conv.append(tuple(w.shape)), orig_conv(self, t, w, b))[1])
    rec = G.Recorder(_lib.load())
    monkeypatch.setattr(_lib, "load", lambda: rec)
    nh = 2 if att else 1

    def step(net_, x_grad=True):
        del rec.calls[:], stock_bn[:], stock_conv[:]
        xi = x.clone().requires_grad_(x_grad)
        outs = G.as_tuple(net_(xi))
        sum((t * r).sum() for t in outs).backward()

    def ends(*names):
        return [rec.count("dmc_ctxends_" + nm) for nm in names]

    for flag in FLAGS:
        monkeypatch.setattr(model, flag, True)                     # all three flags
    for x_grad in (True, False):
        step(copy.deepcopy(net).train(), x_grad)
        assert stock_conv == [] and stock_bn == [], (stock_conv, stock_bn)
        assert rec.count("dmc_dconv_fwd") == 10 and rec.count("dmc_dconv_wgrad") == 5
        assert rec.count("dmc_bnlrelu_fwd") == 6 and rec.count("dmc_bnlrelu_bwd") == 6
        assert ends("first_fwd", "first_wgrad", "heads_fwd", "heads_dgrad", "heads_wgrad") == [1] * 5, rec.names()
        assert ends("bn_fwd", "bn_bwd") == [nh, nh] and ends("first_dgrad") == [int(x_grad)]
        assert [a[14] for nm, a in rec.calls if nm == "dmc_ctxends_bn_fwd"] == [0, 1][:nh]       # relu on the attention head alone
    one = copy.deepcopy(net).train()                               # a head's BatchNorm in eval(): that head alone stays stock
    head_bn = (one.predict_att[0] if att else one.conv_context[-1])[1]
    head_bn.eval()
    before = copy.deepcopy(head_bn.state_dict())
    step(one)
    assert stock_conv == [] and stock_bn == [2] and ends("bn_fwd", "bn_bwd") == [nh - 1, nh - 1]
    assert ends("heads_fwd", "heads_dgrad", "heads_wgrad") == [1, 1, 1] and rec.count("dmc_bnlrelu_fwd") == 6
    for k, v in head_bn.state_dict().items():
        assert torch.equal(v, before[k]), k
    if att:
        assert int(one.predict_flow[1].num_batches_tracked) == 1
    monkeypatch.setattr(model, "CTX_TRAIN_BN", False)              # ENDS without BN: our convolutions, every BatchNorm stock
    step(copy.deepcopy(net).train())
    assert stock_conv == [] and len(stock_bn) == (8 if att else 7)
    assert ends("first_fwd", "first_dgrad", "first_wgrad", "heads_fwd", "heads_dgrad", "heads_wgrad", "bn_fwd", "bn_bwd") == [1] * 6 + [0, 0]
    assert not any(nm.startswith("dmc_bnlrelu_") for nm in rec.names())
    monkeypatch.setattr(model, "CTX_TRAIN_BN", True)
    ev = copy.deepcopy(net).eval()                                 # eval() + no_grad: the eval route keeps precedence
    del rec.calls[:], stock_bn[:], stock_conv[:]
    with torch.no_grad():
        ev(x)
    assert rec.names() and all(nm.startswith("dmc_ctx_") for nm in rec.names()), rec.names()
    assert stock_bn == [] and stock_conv == []
    monkeypatch.setattr(model, "CTX_TRAIN_ENDS", False)            # CTX_TRAIN + BN without ENDS: as tests/test_ctx_bn_gpu.py::test_routes
    step(copy.deepcopy(net).train())
    assert not any(nm.startswith("dmc_ctxends_") for nm in rec.names()), rec.names()
    assert rec.count("dmc_bnlrelu_fwd") == 6 and rec.count("dmc_bnlrelu_bwd") == 6
    assert rec.count("dmc_dconv_fwd") == 10 and rec.count("dmc_dconv_wgrad") == 5
    assert stock_bn == [2] * nh and stock_conv == [(32, 5, 3, 3)] + [(2, 32, 3, 3)] * nh
    monkeypatch.setattr(model, "CTX_TRAIN", False)                 # ENDS (and BN) without CTX_TRAIN: no library call
    monkeypatch.setattr(model, "CTX_TRAIN_ENDS", True)
    step(copy.deepcopy(net).train())
    assert rec.names() == [] and len(stock_bn) == (8 if att else 7) and len(stock_conv) == (8 if att else 7)


# ---------------------------------------------------------------------------------------------------------------------
# the memory contract
# ---------------------------------------------------------------------------------------------------------------------
def ends_arena_case(shape):
    n, h, w = shape

    def fn(a):
        lib = _lib.load()
        c, hc = E.first_case(*shape), E.heads_case(*shape)
        x, wt, dz = a.inp("x", c["x"]), a.inp("w", c["w"]), a.inp("dz", nhwc(c["dz"]))
        a.call("dmc_ctxends_first_fwd", x, wt, a.out("z", (n, h, w, 32)), n, h, w)
        a.call("dmc_ctxends_first_dgrad", dz, wt, a.out("dx", (n, 5, h, w)), n, h, w)
        a.call("dmc_ctxends_first_wgrad", x, dz, a.out("dw", (32, 5, 3, 3)), a.work("ws_first", lib.dmc_ctxends_wgrad_workspace_bytes(n, h, w, 5)), n, h, w)
        t = a.inp("t", nhwc(hc["t"]))
        ws = [a.inp("w_flow", nhwc(hc["w"][0])), a.inp("w_att", nhwc(hc["w"][1]))]
        dzs = [a.inp("dz_flow", hc["dz"][0]), a.inp("dz_att", hc["dz"][1])]
        a.call("dmc_ctxends_heads_fwd", t, ws[0], ws[1], a.out("z_flow", (n, 2, h, w)), a.out("z_att", (n, 2, h, w)), n, h, w)
        a.call("dmc_ctxends_heads_fwd", t, ws[0], None, a.out("z_flow1", (n, 2, h, w)), None, n, h, w)
        a.call("dmc_ctxends_heads_dgrad", dzs[0], dzs[1], ws[0], ws[1], a.out("dt", (n, h, w, 32)), n, h, w)
        a.call("dmc_ctxends_heads_dgrad", None, dzs[1], ws[0], ws[1], a.out("dt_att", (n, h, w, 32)), n, h, w)
        a.call("dmc_ctxends_heads_wgrad", t, dzs[0], dzs[1], a.out("dw_flow", (2, 3, 3, 32)), a.out("dw_att", (2, 3, 3, 32)),
               a.work("ws_heads", lib.dmc_ctxends_wgrad_workspace_bytes(n, h, w, 4)), n, h, w)
        a.call("dmc_ctxends_heads_wgrad", t, None, dzs[1], None, a.out("dw_att1", (2, 3, 3, 32)),
               a.work("ws_heads1", lib.dmc_ctxends_wgrad_workspace_bytes(n, h, w, 2)), n, h, w)
        b = E.bn_case(*shape)
        z, dy = a.inp("bn_z", E.to_planes(b["z"], n, h, w)), a.inp("bn_dy", E.to_planes(b["dy"], n, h, w))
        gamma, beta = a.inp("gamma", b["gamma"]), a.inp("beta", b["beta"])
        nbytes = lib.dmc_ctxends_bn_scratch_bytes(n, h, w)
        for relu in (0, 1):
            stats = a.out("stats%d" % relu, (4,))
            a.call("dmc_ctxends_bn_fwd", z, gamma, beta, a.inout("running_mean%d" % relu, b["rm"]), a.inout("running_var%d" % relu, b["rv"]),
                   a.out("y%d" % relu, (n, 2, h, w)), stats, a.work("scratch_fwd%d" % relu, nbytes), n, h, w, E.SLOPE, E.EPS, E.MOMENTUM, relu)
            a.call("dmc_ctxends_bn_bwd", z, dy, gamma, beta, stats, a.work("scratch_bwd%d" % relu, nbytes), a.out("bn_dz%d" % relu, (n, 2, h, w)),
                   a.out("dgamma%d" % relu, (2,)), a.out("dbeta%d" % relu, (2,)), n, h, w, E.SLOPE, relu)
    return fn


def _ends_arena_check(shape):
    n, h, w = shape

    def check(bufs):
        c, hc = E.first_case(*shape), E.heads_case(*shape)
        for name, ref in (("z", nhwc(c["z"])), ("dx", c["dx"]), ("dw", c["dw"]), ("z_flow", hc["z"][0]), ("z_att", hc["z"][1]),
                          ("z_flow1", hc["z"][0]), ("dt", nhwc(hc["dt"][0] + hc["dt"][1])), ("dt_att", nhwc(hc["dt"][1])),
                          ("dw_flow", nhwc(hc["dw"][0])), ("dw_att", nhwc(hc["dw"][1])), ("dw_att1", nhwc(hc["dw"][1]))):
            assert rel_err(bufs[name].t, ref) < 1e-5, name
        b = bn_dev(E.bn_case(*shape))
        mean, var, invstd = R.stats_ref(b["z"])
        rm, rv = R.running_ref(mean, var, n * h * w, b["rm"], b["rv"])
        for relu in (0, 1):
            y64, t, _ = E.forward_ref(b["z"], b["gamma"], b["beta"], mean, invstd, relu)
            dz, dgamma, dbeta = E.backward_ref(b["z"], b["dy"], b["gamma"], mean, invstd, t > 0, relu)
            for name, ref in (("y", E.to_planes(y64, n, h, w)), ("bn_dz", E.to_planes(dz, n, h, w)), ("dgamma", dgamma), ("dbeta", dbeta),
                              ("running_mean", rm), ("running_var", rv)):
                assert B.err(bufs[name + str(relu)].t, ref) <= 1e-5 * float(ref.abs().max()), (name, relu)
    return check


def _refused(name):
    """One refused call of entry point ``name`` (zero frames; a slope of 1 for the BatchNorm backward): nothing may be written."""
    def fn(a):
        n, h, w = 2, 4, 5
        f = lambda nm, *s: a.inp(nm, torch.zeros(*s))
        o = lambda nm, *s: a.out(nm, s)
        wk = lambda nm: a.work(nm, 1 << 16)
        if name == "dmc_ctxends_first_fwd":
            a.call(name, f("x", n, 5, h, w), f("w", 32, 5, 3, 3), o("z", n, h, w, 32), 0, h, w)
        elif name == "dmc_ctxends_first_dgrad":
            a.call(name, f("dz", n, h, w, 32), None, o("dx", n, 5, h, w), n, h, w)
        elif name == "dmc_ctxends_first_wgrad":
            a.call(name, f("x", n, 5, h, w), f("dz", n, h, w, 32), o("dw", 32, 5, 3, 3), wk("ws"), n, -h, w)
        elif name == "dmc_ctxends_heads_fwd":         # half an attention group: w_att without z_att
            a.call(name, f("t", n, h, w, 32), f("w_flow", 2, 3, 3, 32), f("w_att", 2, 3, 3, 32), o("z_flow", n, 2, h, w), None, n, h, w)
        elif name == "dmc_ctxends_heads_dgrad":       # dz_att without w_att
            a.call(name, f("dz_flow", n, 2, h, w), f("dz_att", n, 2, h, w), f("w_flow", 2, 3, 3, 32), None, o("dt", n, h, w, 32), n, h, w)
        elif name == "dmc_ctxends_heads_wgrad":       # dz_att without dw_att
            a.call(name, f("t", n, h, w, 32), f("dz_flow", n, 2, h, w), f("dz_att", n, 2, h, w), o("dw_flow", 2, 3, 3, 32), None, wk("ws"), n, h, w)
        elif name == "dmc_ctxends_bn_fwd":            # exactly one running pointer
            a.call(name, f("z", n, 2, h, w), f("gamma", 2), f("beta", 2), a.inout("running_mean", torch.zeros(2)), None, o("y", n, 2, h, w),
                   o("stats", 4), wk("scratch"), n, h, w, E.SLOPE, E.EPS, E.MOMENTUM, 0)
        else:                                         # slope 1
            a.call(name, f("z", n, 2, h, w), f("dy", n, 2, h, w), f("gamma", 2), f("beta", 2), f("stats", 4), wk("scratch"), o("dz", n, 2, h, w),
                   o("dgamma", 2), o("dbeta", 2), n, h, w, 1.0, 1)
    return fn


LAUNCHING = ["dmc_ctxends_first_fwd", "dmc_ctxends_first_dgrad", "dmc_ctxends_first_wgrad", "dmc_ctxends_heads_fwd", "dmc_ctxends_heads_dgrad",
             "dmc_ctxends_heads_wgrad", "dmc_ctxends_bn_fwd", "dmc_ctxends_bn_bwd"]
ARENA_CASES = []
for _shape in ((2, 21, 17), (3, 61, 47)):
    ARENA_CASES.append(abi_cases.Case(abi_cases.tag("dmc_ctxends", *_shape), LAUNCHING, ends_arena_case(_shape), check=_ends_arena_check(_shape),
                                      capacity=96 << 20))
for _name in LAUNCHING:
    ARENA_CASES.append(abi_cases.Case(_name + "-refused", [_name], _refused(_name), expect_rc=abi_cases.DMC_E_INVALID, capacity=32 << 20))
_known = {c.id for c in abi_cases.CASES}
abi_cases.CASES.extend(c for c in ARENA_CASES if c.id not in _known)


@pytest.mark.parametrize("case", ARENA_CASES, ids=[c.id for c in ARENA_CASES])
def test_ctxends_entries_memory_contract(case):
    try:
        bufs = run_case(case.fn, device=DEV, capacity=case.capacity, expect_rc=case.expect_rc)
        if case.check is not None:
            case.check(bufs)
    except RuntimeError as e:
        if "HIP error" in str(e) or "illegal memory access" in str(e):
            # a faulted device serves nothing more: end the session here instead of launching the remaining cases on it
            pytest.exit("GPU fault in %s: %s" % (case.id, str(e).splitlines()[0]), returncode=3)
        raise
