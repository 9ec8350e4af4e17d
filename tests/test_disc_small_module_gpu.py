"""GPU, module level (4 frames of 224 x 224): the discriminators with the 8 -> 16 block on csrc/disc_c8.hip (model.DISC_C8) and
adv_layer on csrc/disc_head.hip (model.DISC_HEAD).

  * train mode with forced Dropout2d masks against the fp64 graph with the LeakyReLU branch pattern of the run under test (the z
    tensors of ops.DEBUG_DISC_Z), at the bars tests/test_hip_parity.py applies to a pinned discriminator: 1e-4 on the validity and
    the state, 5e-5 on every gradient -- Discriminator4 is pinned by itself now: every block reports its z;
  * Discriminator4 in eval mode against the reference-held golden of G2;
  * with F.conv2d, F.linear and adv_layer.forward made to raise, forward + backward of all five arch_d complete;
  * the switches at "0" give the stock route, twice the same bits; the own route is deterministic;
  * the head's forward + backward captured in a torch.cuda.graph and replayed on new values equals the eager result bit for bit."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import dmcnet_amd
from dmcnet_amd import model, ops
from oracle import dmc_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ARCHS = ["Discriminator4", "Discriminator"]
TGT = torch.tensor([0, 0, 1, 1])


def rnd(seed, shape):
    return torch.from_numpy(np.random.RandomState(seed).standard_normal(shape).astype(np.float32))


def rel_err(a, b):
    a, b = a.detach().double().cpu(), torch.as_tensor(b).double().cpu()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))


@functools.lru_cache(maxsize=None)
def inputs(arch):
    o = O.seeded_state_fill(O.OracleDiscriminator(arch), seed=31)
    return rnd(32, (4, 2, 224, 224)), O.seeded_dropout_masks(33, o, 4)


def run(arch, monkeypatch, own):
    """One train-mode forward + backward of ``arch`` with both switches at ``own``: validity, {name: gradient} (with "input"), the
    z tensors of the blocks that report them, the state dict after the step."""
    monkeypatch.setattr(model, "DISC_C8", own)
    monkeypatch.setattr(model, "DISC_HEAD", own)
    xin, masks = inputs(arch)
    m = model._DISCRIMINATORS[arch](2)
    m.load_state_dict(O.seeded_state_fill(O.OracleDiscriminator(arch), seed=31).state_dict())
    m.to(DEV).train()
    m.forced_masks = masks
    xg = xin.to(DEV).requires_grad_(True)
    ops.DEBUG_DISC_Z = []
    try:
        v = m(xg)
        zs = [z.detach().cpu() for z in ops.DEBUG_DISC_Z]
    finally:
        ops.DEBUG_DISC_Z = None
    F.cross_entropy(v, TGT.to(DEV)).backward()
    grads = {k: p.grad.detach().clone() for k, p in m.named_parameters()}
    grads["input"] = xg.grad.detach().clone()
    return v.detach(), grads, zs, {k: t.detach().clone() for k, t in m.state_dict().items()}


def fp64_graph(arch, zs):
    """The fp64 evaluation of the same graph; ``zs`` (one per block) pins every LeakyReLU branch to the run under test, None
    leaves them to the fp64 pre-activations.  Returns validity, {name: gradient}, the state dict after the step."""
    xin, masks = inputs(arch)
    o64 = O.seeded_state_fill(O.OracleDiscriminator(arch), seed=31).double().train()
    x64 = xin.double().requires_grad_(True)
    if zs is None:
        o64.forced_masks = {k: v_.double() for k, v_ in masks.items()}
        v64 = o64(x64)
    else:
        assert len(zs) == len(o64.names)
        cur = x64
        for name, zk in zip(o64.names, zs):
            blk = getattr(o64, name)
            slope = torch.where(zk.double() > 0, 1.0, 0.2)
            cur = blk[0](cur) * slope * masks[name].double()[:, :, None, None]
            if len(blk) == 4:
                cur = blk[3](cur)
        v64 = o64.adv_layer(cur.reshape(cur.shape[0], -1))
    F.cross_entropy(v64, TGT).backward()
    grads = {k: p.grad for k, p in o64.named_parameters()}
    grads["input"] = x64.grad
    return v64.detach(), grads, o64.state_dict()


def hold_to_pinned_bars(arch, v, grads, zs, state):
    v64, g64, s64 = fp64_graph(arch, zs)
    assert rel_err(v, v64) < 1e-4
    for k in s64:
        assert rel_err(state[k].float(), s64[k].float()) < 1e-4, k
    worst = max((rel_err(grads[k], g64[k]), k) for k in g64)
    print("%s: worst gradient error against the pinned fp64 graph %.1e (%s)" % (arch, worst[0], worst[1]))
    for k in g64:
        assert rel_err(grads[k], g64[k]) < 5e-5, (k, rel_err(grads[k], g64[k]))


@pytest.mark.parametrize("arch", ARCHS)
def test_own_route_train_mode_vs_pinned_fp64(monkeypatch, arch):
    v, grads, zs, state = run(arch, monkeypatch, True)
    assert len(zs) == len(O.OracleDiscriminator(arch).names)            # every block is a HIP block and reports its z
    hold_to_pinned_bars(arch, v, grads, zs, state)
    v2, grads2, zs2, state2 = run(arch, monkeypatch, True)              # deterministic: the same bits again
    assert torch.equal(v, v2) and all(torch.equal(a, b) for a, b in zip(zs, zs2))
    for k in grads:
        assert torch.equal(grads[k], grads2[k]), k
    for k in state:
        assert torch.equal(state[k], state2[k]), k


@pytest.mark.parametrize("arch", ARCHS)
def test_switches_off_is_the_stock_route_and_both_routes_agree_with_fp64(monkeypatch, arch):
    """Two runs of the stock route give the same bits in the validity, the state and every gradient.  The library's default
    weight-gradient algorithm for Discriminator4's stock Conv2d(8, 16) adds with atomics -- two runs differed in the last bit of
    that one tensor, 1.2e-7 on values of 0.37, everything else equal -- so the stock route is compared under
    torch.backends.cudnn.deterministic, where it is reproducible."""
    monkeypatch.setattr(torch.backends.cudnn, "deterministic", True)
    v0, g0, zs0, s0 = run(arch, monkeypatch, False)
    v1, g1, zs1, s1 = run(arch, monkeypatch, False)
    assert torch.equal(v0, v1) and all(torch.equal(g0[k], g1[k]) for k in g0) and all(torch.equal(s0[k], s1[k]) for k in s0)
    names = O.OracleDiscriminator(arch).names
    if len(zs0) == len(names):                   # every block pinned (only the head differs between the routes)
        hold_to_pinned_bars(arch, v0, g0, zs0, s0)
        return
    # Discriminator4's stock 8 -> 16 block reports no z: the unpinned comparison of tests/test_hip_parity.py, against the fp32 CPU
    # oracle's own distance from the fp64 graph
    assert arch == "Discriminator4" and len(zs0) == len(names) - 1
    xin, masks = inputs(arch)
    o = O.seeded_state_fill(O.OracleDiscriminator(arch), seed=31).train()
    o.forced_masks = masks
    xo = xin.clone().requires_grad_(True)
    F.cross_entropy(o(xo), TGT).backward()
    go = {k: p.grad for k, p in o.named_parameters()}
    go["input"] = xo.grad
    v64, g64, _ = fp64_graph(arch, None)
    assert rel_err(v0, v64) < 1e-4
    for k in g64:
        e_hip, e_cpu = rel_err(g0[k], g64[k]), rel_err(go[k], g64[k])
        assert e_hip <= max(4 * e_cpu, 1e-1), (k, e_hip, e_cpu)


def test_discriminator4_eval_mode_vs_golden(golden, monkeypatch):
    monkeypatch.setattr(model, "DISC_C8", True)
    monkeypatch.setattr(model, "DISC_HEAD", True)
    g = golden("g2_model_eval")
    xd = rnd(27, (2, 2, 224, 224)).to(DEV)
    o = O.seeded_state_fill(O.OracleDiscriminator("Discriminator4"), seed=28)
    m = model._DISCRIMINATORS["Discriminator4"](2)
    m.load_state_dict(o.state_dict())
    m.to(DEV).eval()
    ops.DEBUG_DISC_Z = []
    try:
        with torch.no_grad():
            v = m(xd)
        assert len(ops.DEBUG_DISC_Z) == 3
    finally:
        ops.DEBUG_DISC_Z = None
    assert rel_err(v, g["disc_Discriminator4"]) < 1e-4


@pytest.mark.parametrize("arch", sorted(model._DISCRIMINATORS))
def test_no_stock_convolution_or_linear_in_any_pass(monkeypatch, arch):
    """With both switches on, a discriminator's forward + backward touches neither F.conv2d nor F.linear nor adv_layer's own
    forward."""
    def refuse(*a, **k):
        raise AssertionError("a stock convolution / linear op was called")
    monkeypatch.setattr(model, "DISC_C8", True)
    monkeypatch.setattr(model, "DISC_HEAD", True)
    m = model._DISCRIMINATORS[arch](2).to(DEV).train()
    x = rnd(41, (4, 2, 224, 224)).to(DEV).requires_grad_(True)
    monkeypatch.setattr(model.F, "conv2d", refuse)
    monkeypatch.setattr(model.F, "linear", refuse)
    monkeypatch.setattr(m.adv_layer, "forward", refuse)
    v = m(x)
    ops.consensus_ce(v, TGT.to(DEV), 1)[0].backward()
    assert v.shape == (4, 2) and bool(torch.isfinite(v).all()) and bool(torch.isfinite(x.grad).all())
    for k, p in m.named_parameters():
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()), k


def test_head_forward_backward_replays_from_a_graph_bit_for_bit():
    """One small capture without parallel branches: forward, then the three gradients, replayed twice on new values."""
    shape = (5, 128, 14, 14)
    m, c, h, w = shape

    def fresh(seed):
        return (rnd(seed, (m, h, w, c)).to(DEV).permute(0, 3, 1, 2), rnd(seed + 1, (m, 2)).to(DEV))
    wt = (rnd(50, (2, c * h * w)) * 0.05).to(DEV).requires_grad_(True)
    b = rnd(51, (2,)).to(DEV).requires_grad_(True)

    def step(x, dv):
        v = ops.disc_head(x, wt, b)
        return (v,) + torch.autograd.grad(v, [x, wt, b], dv)
    x0, dv0 = fresh(60)
    xs, dvs = x0.clone(memory_format=torch.channels_last).requires_grad_(True), dv0.clone()
    assert ops.disc_head_supported(xs, torch.nn.Linear(c * h * w, 2).to(DEV))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step(xs, dvs)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        outs = step(xs, dvs)
    for seed in (70, 80):
        x1, dv1 = fresh(seed)
        with torch.no_grad():
            xs.copy_(x1)
            dvs.copy_(dv1)
        graph.replay()
        torch.cuda.synchronize()
        got = [t.clone() for t in outs]
        want = step(x1.clone(memory_format=torch.channels_last).requires_grad_(True), dv1)
        for a, e in zip(got, want):
            assert torch.equal(a, e)
