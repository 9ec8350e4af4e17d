"""GPU: the reconstruction criteria of the reference on the device -- ``--loss-mse`` MSELoss | SmoothL1Loss | L1
(code/dmcnet/train.py:166-172) and the attention-weighted form criterion(att * gen, att * flow) (code/dmcnet/train.py:335,
code/dmcnet_GAN/train.py:352): dmc_flow_loss_fwd / _bwd stand-alone, dmc_gen_tiny_fwd_loss in the generator's one-launch
forward, and the trainers that reach them.

Reference for values: torch's own F.mse_loss / F.smooth_l1_loss / F.l1_loss (what the reference's criterion_mse IS), in fp32 on
the CPU, at the tolerance of test_hip_parity.test_flow_mse: 1e-5 relative (largest error over largest reference element) on
the loss and on each gradient; one case per kind against the same functions in fp64.

The arena cases of the four launching entry points are built here and appended to the registry of tests/abi_cases.py at import
(the registry's coverage check, tests/test_abi_arena_cpu.py, then sees the entry points); they are RUN here."""
import copy

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import dmcnet_amd
from dmcnet_amd import _lib, ops
from dmcnet_amd import train as T
from oracle import dmc_oracle as O
from tests import abi_cases
from tests.abi_arena import run_case

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
KINDS = ("MSELoss", "SmoothL1Loss", "L1")
STOCK = {"MSELoss": F.mse_loss, "SmoothL1Loss": F.smooth_l1_loss, "L1": F.l1_loss}


def rnd(seed, shape, scale=1.0):
    return torch.from_numpy((np.random.RandomState(seed).standard_normal(shape) * scale).astype(np.float32))


def rel_err(a, b):
    a, b = a.detach().double().cpu(), torch.as_tensor(b).detach().double().cpu()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))


# ---------------------------------------------------------------------------------------------------------------------
# 1. stand-alone: every kind, with and without attention
# ---------------------------------------------------------------------------------------------------------------------
# 1, 3: only the scalar tail; 4: one vector, no tail; 5: both; 1023 / 1188: a ragged block, 1188 = the 2 x 2 x 9 x 33 of a small
# batch; 12800: several blocks; the last: all 2048 blocks, a second trip of the grid-stride loop and a 3-element tail
NUMELS = (1, 3, 4, 5, 1023, 1188, 12800, 2048 * 256 * 4 + 3)
_INPUTS = {}


def inputs(numel):
    """(gen, flow, att) on the CPU, made once per size and never modified: randn x 1.5 (37 % of |gen - flow| below 1: both
    SmoothL1 branches); att = ReLU(randn) (half of it exact zeros, as the attention head gives).  From 3 elements on: element 0
    has d == 0, elements 1 / 2 have d == +1 / -1 exactly (att 1 there), so sign(0) and the SmoothL1 seam are met."""
    if numel not in _INPUTS:
        gen, flow, att = rnd(11, (numel,), 1.5), rnd(12, (numel,), 1.5), torch.relu(rnd(13, (numel,)))
        if numel >= 3:
            gen[0], flow[0], att[0] = 0.75, 0.75, 1.0
            gen[1], flow[1], att[1] = 2.5, 1.5, 1.0
            gen[2], flow[2], att[2] = -0.25, 0.75, 1.0
        if numel >= 5:
            att[4] = 0.0
        _INPUTS[numel] = (gen, flow, att)
    return _INPUTS[numel]


def stock(kind, gen, flow, att, dtype=torch.float32, scale=10.0):
    """(loss * scale, grad_gen, grad_att) of the stock criterion on the CPU."""
    g = gen.to(dtype).clone().requires_grad_(True)
    f = flow.to(dtype)
    a = None if att is None else att.to(dtype).clone().requires_grad_(True)
    loss = (STOCK[kind](g, f) if a is None else STOCK[kind](a * g, a * f)) * scale
    loss.backward()
    return loss.detach(), g.grad, None if a is None else a.grad


def device(kind, gen, flow, att, scale=10.0):
    g = gen.to(DEV).requires_grad_(True)
    a = None if att is None else att.to(DEV).requires_grad_(True)
    loss = ops.flow_loss(kind, g, flow.to(DEV), a) * scale
    loss.backward()
    return loss.detach(), g.grad, None if a is None else a.grad


@pytest.mark.parametrize("numel", NUMELS)
@pytest.mark.parametrize("with_att", [False, True], ids=["plain", "att"])
@pytest.mark.parametrize("kind", KINDS)
def test_flow_loss_vs_torch(kind, with_att, numel):
    gen, flow, att = inputs(numel)
    att = att if with_att else None
    lo, ggo, gao = stock(kind, gen, flow, att)
    l, gg, ga = device(kind, gen, flow, att)                    # loss * 10: the upstream gradient is not 1
    e = [rel_err(l, lo), rel_err(gg, ggo)] + ([rel_err(ga, gao)] if with_att else [])
    print("flow_loss %s att=%d numel=%d: loss %.2e grad_gen %.2e%s" % (kind, with_att, numel, e[0], e[1], " grad_att %.2e" % e[2] if with_att else ""))
    assert max(e) < 1e-5, e
    if kind == "L1" and numel >= 3:
        assert float(gg[0]) == 0.0 and (not with_att or float(ga[0]) == 0.0)      # sign(0) = 0, exactly
    l2, gg2, ga2 = device(kind, gen, flow, att)
    assert torch.equal(l, l2) and torch.equal(gg, gg2) and (not with_att or torch.equal(ga, ga2))      # fixed order: bit-identical
    if kind == "MSELoss" and not with_att:                      # the old entries' kernels: their bits
        g = gen.to(DEV).requires_grad_(True)
        lm = ops.flow_mse(g, flow.to(DEV)) * 10.0
        lm.backward()
        assert torch.equal(l, lm) and torch.equal(gg, g.grad)


@pytest.mark.parametrize("with_att", [False, True], ids=["plain", "att"])
@pytest.mark.parametrize("kind", KINDS)
def test_flow_loss_vs_torch_fp64(kind, with_att):
    gen, flow, att = inputs(1188)
    att = att if with_att else None
    lo, ggo, gao = stock(kind, gen, flow, att, torch.float64)
    l, gg, ga = device(kind, gen, flow, att)
    assert rel_err(l, lo) < 1e-5 and rel_err(gg, ggo) < 1e-5 and (not with_att or rel_err(ga, gao) < 1e-5)


def test_flow_loss_wrapper_contract():
    g, f = rnd(1, (2, 2, 5, 7)).to(DEV), rnd(2, (2, 2, 5, 7)).to(DEV)
    with pytest.raises(NotImplementedError):
        ops.flow_loss("L1", g, f.clone().requires_grad_(True))
    with pytest.raises(ValueError):
        ops.flow_loss("L1", g, f[:1])
    with pytest.raises(ValueError):
        ops.flow_loss("L1", g, f, f[:, :1])
    # an attention map nobody differentiates: grad_att == NULL at the C ABI
    a = torch.relu(rnd(3, (2, 2, 5, 7))).to(DEV)
    gr = g.clone().requires_grad_(True)
    ops.flow_loss("SmoothL1Loss", gr, f, a).backward()
    _, ggo, _ = stock("SmoothL1Loss", g.cpu(), f.cpu(), a.cpu(), scale=1.0)
    assert rel_err(gr.grad, ggo) < 1e-5
    # train.flow_loss: device tensors take the library for every combination, plain MSE the old op
    for kind in KINDS:
        for att in (None, a):
            l = T.flow_loss(kind, g, f, att)
            ref = STOCK[kind](g.cpu(), f.cpu()) if att is None else STOCK[kind](a.cpu() * g.cpu(), a.cpu() * f.cpu())
            assert rel_err(l, ref) < 1e-5
    assert torch.equal(T.flow_loss("MSELoss", g, f), ops.flow_mse(g, f))


# ---------------------------------------------------------------------------------------------------------------------
# 2. the loss in the generator's one-launch forward against generator + stand-alone loss
# ---------------------------------------------------------------------------------------------------------------------
# (3, 40, 40): one strip; (6, 224, 224): two strips, both halves of each; (2, 19, 37): W % 4 != 0, which the one-launch forward
# serves as well (odd strip width, scalar row offsets) -- these three run the kind's own instantiation of the fused kernel;
# (1, 8, 228): W > 224, the only fallback: the layer-by-layer forward + the streaming reduction inside the entry point
FUSED_SHAPES = [(3, 40, 40), (6, 224, 224), (2, 19, 37), (1, 8, 228)]


def gen_and_data(shape):
    n, h, w = shape
    torch.manual_seed(5)
    gen = dmcnet_amd.model.EstimatorDenseNetTiny(5).to(DEV)
    mv, res, flow = rnd(301, (n, 2, h, w)).to(DEV), rnd(302, (n, 3, h, w)).to(DEV), rnd(303, (n, 2, h, w)).to(DEV)
    return gen, mv, res, flow, rnd(304, (n, 2, h, w)).to(DEV)


@pytest.mark.parametrize("shape", FUSED_SHAPES)
@pytest.mark.parametrize("kind", ["SmoothL1Loss", "L1"])
def test_generator_fused_flow_loss_equals_separate_ops(kind, shape):
    """The comparison of test_generator_fused_flow_mse_equals_separate_ops for the other two criteria: identical gen_flow,
    the loss within 2e-6 relative (two fixed summation orders), parameter gradients within 1e-6 for loss-only, output-only
    and mixed upstream gradients, a repeated run bit-identical."""
    gen, mv, res, flow, r = gen_and_data(shape)
    params = list(gen.parameters())
    for lw, ow in ((10.0, 0.0), (0.0, 1.0), (10.0, 0.5)):
        gen.zero_grad()
        y0 = gen.forward_mv_res(mv, res, True)
        l0 = ops.flow_loss(kind, y0, flow)
        (lw * l0 + ow * (y0 * r).sum()).backward()
        g0 = [p.grad.clone() for p in params]
        gen.zero_grad()
        y1, l1 = gen.forward_mv_res_loss(kind, mv, res, flow, True)
        (lw * l1 + ow * (y1 * r).sum()).backward()
        assert torch.equal(y0, y1)
        print("fused %s %s: loss %.9g separate %.9g" % (kind, shape, float(l1), float(l0)))
        assert abs(float(l0) - float(l1)) <= 2e-6 * abs(float(l0))
        for a, b in zip([p.grad for p in params], g0):
            assert rel_err(a, b) < 1e-6
    y2, l2 = gen.forward_mv_res_loss(kind, mv, res, flow, True)
    assert torch.equal(y1, y2) and float(l1) == float(l2)          # deterministic
    assert rel_err(l1, STOCK[kind](y1.cpu(), flow.cpu())) < 1e-5   # and it IS the criterion


@pytest.mark.parametrize("shape", [(3, 40, 40), (2, 19, 37), (1, 8, 228)])
def test_generator_fused_loss_kind_mse_is_gen_tiny_mse(shape):
    gen, mv, res, flow, r = gen_and_data(shape)
    params = list(gen.parameters())
    got = []
    for fwd in (lambda: gen.forward_mv_res_mse(mv, res, flow, True), lambda: gen.forward_mv_res_loss("MSELoss", mv, res, flow, True)):
        gen.zero_grad()
        y, l = fwd()
        (10.0 * l + 0.5 * (y * r).sum()).backward()
        got.append([y.detach(), l.detach()] + [p.grad.clone() for p in params])
    assert all(torch.equal(a, b) for a, b in zip(*got))


# ---------------------------------------------------------------------------------------------------------------------
# 3. trainers
# ---------------------------------------------------------------------------------------------------------------------
class Recorder(object):
    """A stand-in for the loaded library that records the name of every entry point called through it."""

    def __init__(self, lib):
        self._lib, self.calls = lib, []

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if not name.startswith("dmc_"):
            return fn

        def call(*args):
            self.calls.append(name)
            return fn(*args)
        return call


def stock_dmcnet_step(step, batch, kind):
    """DmcnetTrainStep.step with the reconstruction loss on the stock route: F.* on the device tensors."""
    input_flow, input_mv, input_residual, target = batch
    flow = input_flow.reshape((-1,) + tuple(input_mv.shape[-3:]))
    step.optimizer_cls.zero_grad(set_to_none=True)
    step.optimizer_gf.zero_grad(set_to_none=True)
    output, gen_flow = step.model(input_mv, input_residual)
    loss_cls, _ = ops.consensus_ce(output, target, step.num_segments)
    loss_mse = STOCK[kind](gen_flow, flow)
    loss = loss_cls * step.lr_cls + loss_mse * step.lr_mse
    with ops.wgrad_side_stream():
        loss.backward()
    step.optimizer_cls.step()
    step.optimizer_gf.step()
    return {"loss": loss.detach(), "loss_cls": loss_cls.detach(), "loss_mse": loss_mse.detach()}


@pytest.mark.parametrize("kind", KINDS)
def test_dmcnet_train_step_per_kind(kind, monkeypatch):
    """B = 2, S = 3, resnet18 + DenseNetTiny: the step takes the fused forward for every kind, and agrees with the same step on
    the stock loss: losses at 1e-5, post-step generator weights within the step tests' fraction of an Adam step.  Frames of
    224 x 224, as in every other step test: the classifier ends in AvgPool2d(7), which needs a 7 x 7 map after the /32 trunk, so
    nothing below 193 x 193 passes through it (a 40 x 40 frame arrives there as 2 x 2)."""
    kw = dict(base_model="resnet18", use_databn=0, gen_flow_or_delta=1, arch_estimator="DenseNetTiny")
    m = dmcnet_amd.Model(51, 3, "mv", **kw)
    m.load_state_dict(O.seeded_state_fill(O.OracleModel(51, 3, "mv", **kw), seed=81).state_dict())
    m.to(DEV).train()
    m2 = copy.deepcopy(m)
    batch = tuple(t.to(DEV) for t in O.synthetic_batch(seed=82, batch=2, num_segments=3, num_class=51))
    hp = dict(lr=0.01, weight_decay=1e-4, lr_cls_mult=0.01, lr_mse_mult=1.0)
    ref = stock_dmcnet_step(T.DmcnetTrainStep(m2, 3, 1.0, 10.0, loss_mse=kind, **hp), batch, kind)
    rec = Recorder(_lib.load())
    monkeypatch.setattr(_lib, "load", lambda: rec)
    got = T.DmcnetTrainStep(m, 3, 1.0, 10.0, loss_mse=kind, **hp).step(batch)
    calls = rec.calls
    if kind == "MSELoss":       # the default recipe keeps its entry points
        assert calls.count("dmc_gen_tiny_fwd_mse") == 1 and calls.count("dmc_flow_mse_bwd") == 1
        assert not any(c.startswith("dmc_flow_loss") or c == "dmc_gen_tiny_fwd_loss" for c in calls), calls
    else:
        assert calls.count("dmc_gen_tiny_fwd_loss") == 1 and calls.count("dmc_flow_loss_bwd") == 1, calls
        assert not any(c.startswith("dmc_flow_mse") for c in calls) and "dmc_gen_tiny_fwd_mse" not in calls, calls
        assert "dmc_flow_loss_fwd" not in calls and "dmc_gen_tiny_fwd" not in calls, calls      # one forward, the loss in its epilogue
    for k in ("loss", "loss_cls", "loss_mse"):
        print("step %s %s: %.9g stock %.9g" % (kind, k, float(got[k]), float(ref[k])))
        assert rel_err(got[k], ref[k]) < 1e-5, k
    for (k, p), (_, q) in zip(m.gen_flow_model.named_parameters(), m2.gen_flow_model.named_parameters()):
        # Adam normalises the update: a weight moves by ~lr whatever its gradient's size, so the comparison is absolute, at a
        # small fraction of the step (test_dmcnet_train_step_vs_reference_golden)
        assert float((p - q).abs().max()) < 2e-4 * max(1.0, float(q.abs().max())), k


def stock_flow_loss(kind, gen_flow, flow, att_flow=None):
    if att_flow is not None:
        gen_flow, flow = att_flow * gen_flow, att_flow * flow
    return STOCK[kind](gen_flow, flow)


def att_model(gan, seed):
    torch.manual_seed(seed)
    m = dmcnet_amd.Model(51, 3, "mv", base_model="resnet18", use_databn=0, gen_flow_or_delta=1, arch_estimator="ContextNetwork",
                         arch_d="Discriminator3" if gan else None, att=1)
    return m.to(DEV)


@pytest.mark.parametrize("kind", KINDS)
def test_validate_with_attention(kind, monkeypatch):
    from dmcnet_amd import driver
    m = att_model(False, 91)
    batch = O.synthetic_batch(seed=92, batch=2, num_segments=3, num_class=51)       # 224 x 224: the classifier's AvgPool2d(7), see above
    rec = Recorder(_lib.load())
    monkeypatch.setattr(_lib, "load", lambda: rec)
    got = driver.validate([batch], m, 3, 1.0, 10.0, DEV, log=None, loss_mse=kind)
    assert rec.calls.count("dmc_flow_loss_fwd") == 1
    monkeypatch.setattr(T, "flow_loss", stock_flow_loss)
    ref = driver.validate([batch], m, 3, 1.0, 10.0, DEV, log=None, loss_mse=kind)
    for k in ("loss", "loss_mse"):
        print("validate att %s %s: %.9g stock %.9g" % (kind, k, got[k], ref[k]))
        assert abs(got[k] - ref[k]) <= 1e-5 * abs(ref[k]), k


@pytest.mark.parametrize("kind", ["SmoothL1Loss"])
def test_gan_generator_step_with_attention(kind, monkeypatch):
    """One G step (i odd) of the GAN trainer with att = 1 at 224 x 224, the smallest frame the discriminator's flatten
    accepts, one clip of three segments: its losses against the same step on the stock loss."""
    m = att_model(True, 93).train()
    m2 = copy.deepcopy(m)
    masks = O.seeded_dropout_masks(94, m.discriminator, 3)
    m.discriminator.forced_masks, m2.discriminator.forced_masks = masks, masks
    batch = tuple(t.to(DEV) for t in O.synthetic_batch(seed=95, batch=1, num_segments=3, num_class=51))
    args = (3, 1.0, 1.0, 0.01, 10.0, 0.01, 1e-4, 0.01, 1.0, 1.0)
    rec = Recorder(_lib.load())
    monkeypatch.setattr(_lib, "load", lambda: rec)
    got = T.GanTrainStep(m, *args, loss_mse=kind, att=1).step(batch, 1)
    assert rec.calls.count("dmc_flow_loss_fwd") == 1 and rec.calls.count("dmc_flow_loss_bwd") == 1
    monkeypatch.setattr(T, "flow_loss", stock_flow_loss)
    ref = T.GanTrainStep(m2, *args, loss_mse=kind, att=1).step(batch, 1)
    for k in ("loss", "loss_mse"):
        print("GAN G step att %s %s: %.9g stock %.9g" % (kind, k, float(got[k]), float(ref[k])))
        assert rel_err(got[k], ref[k]) < 1e-5, k


# ---------------------------------------------------------------------------------------------------------------------
# 4. memory contract: the four launching entry points in guarded arenas (tests/abi_arena.py)
# ---------------------------------------------------------------------------------------------------------------------
def arena_inputs(numel):
    gen, flow, att = rnd(5, (numel,), 1.5), rnd(6, (numel,), 1.5), torch.relu(rnd(7, (numel,)))
    return gen, flow, att


def flow_loss_case(kind, numel, with_att, with_grad_att):
    def fn(a):
        L = _lib.load()
        gen, flow, att = arena_inputs(numel)
        g, f = a.inp("gen_flow", gen), a.inp("flow", flow)
        t = a.inp("att", att) if with_att else None
        loss = a.out("loss", (1,))
        a.call("dmc_flow_loss_fwd", kind, g, f, t, loss, a.work("partials", L.dmc_flow_loss_partials_bytes()), numel)
        gl = a.inp("grad_loss", torch.tensor([0.75]))
        ga = a.out("grad_att", (numel,)) if with_grad_att else None
        a.call("dmc_flow_loss_bwd", kind, g, f, t, gl, a.out("grad_gen", (numel,)), ga, numel)

    def check(bufs):                    # bit for bit what the wrapper computes (it makes these very calls)
        gen, flow, att = arena_inputs(numel)
        g = gen.to(DEV).requires_grad_(True)
        t = att.to(DEV).requires_grad_(bool(with_grad_att)) if with_att else None
        loss = ops.flow_loss(KINDS[kind], g, flow.to(DEV), t)
        (loss * 0.75).backward()
        assert abi_cases.same(bufs["loss"], loss) and abi_cases.same(bufs["grad_gen"], g.grad)
        if with_grad_att:
            assert abi_cases.same(bufs["grad_att"], t.grad)
    return fn, check


def flow_loss_refused(which):
    def fn(a):
        L = _lib.load()
        gen, flow, att = arena_inputs(5)
        g, f, t = a.inp("gen_flow", gen), a.inp("flow", flow), a.inp("att", att)
        loss, part = a.out("loss", (1,)), a.work("partials", L.dmc_flow_loss_partials_bytes())
        gl, gg, ga = a.inp("grad_loss", torch.tensor([0.75])), a.out("grad_gen", (5,)), a.out("grad_att", (5,))
        if which == "fwd-kind":
            a.call("dmc_flow_loss_fwd", 3, g, f, t, loss, part, 5)
        elif which == "fwd-empty":
            a.call("dmc_flow_loss_fwd", 1, g, f, t, loss, part, 0)
        elif which == "bwd-kind":
            a.call("dmc_flow_loss_bwd", -1, g, f, t, gl, gg, ga, 5)
        else:
            a.call("dmc_flow_loss_bwd", 2, g, f, None, gl, gg, ga, 5)      # grad_att without att
    return fn


def fused_loss_case(kind, shape):
    n, h, w = shape

    def fn(a):
        L = _lib.load()
        mv, res, ws, bs = abi_cases.gen_inputs(n, h, w)
        mv, res = a.inp("mv", mv), a.inp("res", res)
        ws = [a.inp("w%d" % i, t) for i, t in enumerate(ws)]
        bs = [a.inp("b%d" % i, t) for i, t in enumerate(bs)]
        flow, out, loss = a.inp("flow", rnd(3, (n, 2, h, w))), a.out("out", (n, 2, h, w)), a.out("loss", (1,))
        saved = a.out("saved", nbytes=L.dmc_gen_tiny_saved_bytes(n, h, w))
        a.call("dmc_gen_tiny_fwd_loss", kind, mv, res, ws, bs, flow, out, saved, a.work("workspace", L.dmc_gen_tiny_workspace_bytes()), loss,
               a.work("mse_partials", L.dmc_gen_tiny_mse_partials_bytes()), n, h, w, 1)

    def check(bufs):
        mv, res, ws, bs = abi_cases.gen_inputs(n, h, w)
        ws, bs = [t.to(DEV).requires_grad_(True) for t in ws], [t.to(DEV).requires_grad_(True) for t in bs]
        out, loss = ops.gen_tiny_loss(KINDS[kind], mv.to(DEV), res.to(DEV), rnd(3, (n, 2, h, w)).to(DEV), ws, bs, add_mv=True)
        assert abi_cases.same(bufs["out"], out) and abi_cases.same(bufs["loss"], loss)
    return fn, check


def fused_loss_refused(a):
    L = _lib.load()
    n, h, w = 1, 3, 5
    mv, res, ws, bs = abi_cases.gen_inputs(n, h, w)
    mv, res = a.inp("mv", mv), a.inp("res", res)
    ws = [a.inp("w%d" % i, t) for i, t in enumerate(ws)]
    bs = [a.inp("b%d" % i, t) for i, t in enumerate(bs)]
    flow, out, loss = a.inp("flow", rnd(3, (n, 2, h, w))), a.out("out", (n, 2, h, w)), a.out("loss", (1,))
    saved = a.out("saved", nbytes=L.dmc_gen_tiny_saved_bytes(n, h, w))
    a.call("dmc_gen_tiny_fwd_loss", 3, mv, res, ws, bs, flow, out, saved, a.work("workspace", L.dmc_gen_tiny_workspace_bytes()), loss,
           a.work("mse_partials", L.dmc_gen_tiny_mse_partials_bytes()), n, h, w, 1)


_FLOW_COVERS = ["dmc_flow_loss_fwd", "dmc_flow_loss_bwd"]
ARENA_CASES = []
for _kind in (0, 1, 2):
    for _numel in (5, 1188):
        for _att, _gatt in ((0, 0), (1, 1), (1, 0)):
            _fn, _ck = flow_loss_case(_kind, _numel, _att, _gatt)
            ARENA_CASES.append(abi_cases.Case(abi_cases.tag("dmc_flow_loss", KINDS[_kind], _numel, ("att" if _att else "plain") + ("-gradatt" if _gatt else "")),
                                              _FLOW_COVERS, _fn, check=_ck, capacity=16 << 20))
    for _shape in ((1, 3, 5), (1, 8, 32)):
        _fn, _ck = fused_loss_case(_kind, _shape)
        ARENA_CASES.append(abi_cases.Case(abi_cases.tag("dmc_gen_tiny_fwd_loss", KINDS[_kind], *_shape), ["dmc_gen_tiny_fwd_loss"], _fn, check=_ck,
                                          capacity=32 << 20))
for _which in ("fwd-kind", "fwd-empty", "bwd-kind", "bwd-gradatt-without-att"):
    ARENA_CASES.append(abi_cases.Case("dmc_flow_loss-refused-" + _which, ["dmc_flow_loss_fwd" if _which.startswith("fwd") else "dmc_flow_loss_bwd"],
                                      flow_loss_refused(_which), expect_rc=abi_cases.DMC_E_INVALID, capacity=24 << 20))
ARENA_CASES.append(abi_cases.Case("dmc_gen_tiny_fwd_loss-refused-kind", ["dmc_gen_tiny_fwd_loss"], fused_loss_refused, expect_rc=abi_cases.DMC_E_INVALID,
                                  capacity=32 << 20))
_known = {c.id for c in abi_cases.CASES}
abi_cases.CASES.extend(c for c in ARENA_CASES if c.id not in _known)


@pytest.mark.parametrize("case", ARENA_CASES, ids=[c.id for c in ARENA_CASES])
def test_flow_loss_memory_contract(case):
    try:
        bufs = run_case(case.fn, device=DEV, capacity=case.capacity, expect_rc=case.expect_rc)
        if case.check is not None:
            case.check(bufs)
    except RuntimeError as e:
        if "HIP error" in str(e) or "illegal memory access" in str(e):
            # a faulted device serves nothing more: end the session here instead of launching the remaining cases on it
            pytest.exit("GPU fault in %s: %s" % (case.id, str(e).splitlines()[0]), returncode=3)
        raise
