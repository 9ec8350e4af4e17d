"""CPU checks of the flow-loss entry points (dmc_flow_loss_fwd / _bwd, dmc_gen_tiny_fwd_loss): every refusal the header
promises is made on the host, before any launch, with the entry point's name in dmc_last_error(); the Python routes keep
their CPU behaviour (train.flow_loss = the stock ops bit for bit, ops.flow_loss raises)."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

import dmcnet_amd
from dmcnet_amd import _lib, ops, train

P = ctypes.c_void_p


class HostBufs(object):
    """Host memory standing in for device buffers: a refused call never dereferences a pointer, and must leave these bytes alone."""

    def __init__(self, n):
        self.raw = [(ctypes.c_ubyte * 64)(*([0xA5] * 64)) for _ in range(n)]

    def __getitem__(self, i):
        return ctypes.cast(self.raw[i], P)

    def untouched(self):
        return all(bytes(r) == b"\xA5" * 64 for r in self.raw)


def refused(lib, name, *args):
    rc = getattr(lib, name)(*args)
    text = lib.dmc_last_error()
    assert rc == -1, (name, rc)
    assert name.encode() in text, (name, text)


def test_flow_loss_fwd_refusals():
    lib = _lib.load()
    b = HostBufs(5)
    gen, flow, att, loss, part = b[0], b[1], b[2], b[3], b[4]
    for kind in (-1, 3, 7):
        refused(lib, "dmc_flow_loss_fwd", kind, gen, flow, att, loss, part, 8, None)
        refused(lib, "dmc_flow_loss_fwd", kind, gen, flow, None, loss, part, 8, None)
    for kind in (0, 1, 2):
        for a in (att, None):
            refused(lib, "dmc_flow_loss_fwd", kind, None, flow, a, loss, part, 8, None)
            refused(lib, "dmc_flow_loss_fwd", kind, gen, None, a, loss, part, 8, None)
            refused(lib, "dmc_flow_loss_fwd", kind, gen, flow, a, None, part, 8, None)
            refused(lib, "dmc_flow_loss_fwd", kind, gen, flow, a, loss, None, 8, None)
            refused(lib, "dmc_flow_loss_fwd", kind, gen, flow, a, loss, part, 0, None)
    assert b.untouched()


def test_flow_loss_bwd_refusals():
    lib = _lib.load()
    b = HostBufs(6)
    gen, flow, att, gl, gg, ga = b[0], b[1], b[2], b[3], b[4], b[5]
    for kind in (-1, 3):
        refused(lib, "dmc_flow_loss_bwd", kind, gen, flow, att, gl, gg, ga, 8, None)
    for kind in (0, 1, 2):
        for a, g in ((att, ga), (att, None), (None, None)):
            refused(lib, "dmc_flow_loss_bwd", kind, None, flow, a, gl, gg, g, 8, None)
            refused(lib, "dmc_flow_loss_bwd", kind, gen, None, a, gl, gg, g, 8, None)
            refused(lib, "dmc_flow_loss_bwd", kind, gen, flow, a, None, gg, g, 8, None)
            refused(lib, "dmc_flow_loss_bwd", kind, gen, flow, a, gl, None, g, 8, None)
            refused(lib, "dmc_flow_loss_bwd", kind, gen, flow, a, gl, gg, g, 0, None)
        refused(lib, "dmc_flow_loss_bwd", kind, gen, flow, None, gl, gg, ga, 8, None)        # grad_att without att
    assert b"grad_att" in lib.dmc_last_error()
    assert b.untouched()


def test_gen_tiny_fwd_loss_refusals():
    lib = _lib.load()
    b = HostBufs(10)
    mv, res, flow, out, saved, work, loss, part = (b[i] for i in range(8))
    w = (P * 6)(*[b[8].value] * 6)
    bs = (P * 6)(*[b[9].value] * 6)
    good = [mv, res, w, bs, flow, out, saved, work, loss, part]
    for kind in (-1, 3):
        refused(lib, "dmc_gen_tiny_fwd_loss", kind, *good, 1, 8, 32, 1, None)
    for kind in (0, 1, 2):
        for i in range(len(good)):
            if i == 6:          # saved == NULL is the inference form, not a refusal
                continue
            args = list(good)
            args[i] = None
            refused(lib, "dmc_gen_tiny_fwd_loss", kind, *args, 1, 8, 32, 1, None)
        for shape in ((0, 8, 32), (1, 0, 32), (1, 8, 0), (-1, 8, 32)):
            refused(lib, "dmc_gen_tiny_fwd_loss", kind, *good, *shape, 1, None)
    assert b.untouched()


def test_partials_query_matches_the_mse_entries():
    lib = _lib.load()
    assert lib.dmc_flow_loss_partials_bytes() == lib.dmc_flow_mse_partials_bytes() > 0
    assert lib.dmc_gen_tiny_mse_partials_bytes() >= lib.dmc_flow_loss_partials_bytes()     # the fused entry's fallback fits its workspace


def test_train_flow_loss_on_cpu_tensors_is_the_stock_route():
    torch.manual_seed(3)
    g, f = torch.randn(2, 2, 9, 7) * 1.5, torch.randn(2, 2, 9, 7) * 1.5
    att = torch.relu(torch.randn(2, 2, 9, 7))
    fns = {"MSELoss": F.mse_loss, "SmoothL1Loss": F.smooth_l1_loss, "L1": F.l1_loss}
    for kind, fn in fns.items():
        if kind != "MSELoss":       # (plain MSE has no CPU route: tests/test_host_cpu.py)
            assert torch.equal(train.flow_loss(kind, g, f), fn(g, f))
        gr, ar = g.clone().requires_grad_(True), att.clone().requires_grad_(True)
        l = train.flow_loss(kind, gr, f, ar)
        assert torch.equal(l, fn(att * g, att * f))
        l.backward()
        g2, a2 = g.clone().requires_grad_(True), att.clone().requires_grad_(True)
        fn(a2 * g2, a2 * f).backward()
        assert torch.equal(gr.grad, g2.grad) and torch.equal(ar.grad, a2.grad)


def test_ops_flow_loss_refuses_cpu_tensors_and_unknown_kinds():
    g, f = torch.zeros(4), torch.zeros(4)
    for kind in ("MSELoss", "SmoothL1Loss", "L1"):
        with pytest.raises(_lib.DmcHipError):
            ops.flow_loss(kind, g, f)
        with pytest.raises(_lib.DmcHipError):
            ops.flow_loss(kind, g, f, torch.ones(4))
    with pytest.raises(ValueError):
        ops.flow_loss("Huber", g, f)
    with pytest.raises(ValueError):
        ops.gen_tiny_loss("Huber", g, f, f, [], [])
    m = dmcnet_amd.Model(51, 3, "mv", base_model="resnet18", use_databn=0, gen_flow_or_delta=1, arch_estimator="DenseNetTiny")
    mv, res, flow = torch.zeros(1, 3, 2, 32, 32), torch.zeros(1, 3, 3, 32, 32), torch.zeros(3, 2, 32, 32)
    with pytest.raises(_lib.DmcHipError):
        m.forward_with_flow_loss("L1", mv, res, flow)
    with pytest.raises(ValueError):
        m.forward_with_flow_loss("Huber", mv, res, flow)


def test_attention_head_is_differentiable():
    """The attention-weighted loss sends a gradient through ContextNetworkAtt.predict_att (LeakyReLU, then ReLU): the stock
    criterion's backward must run, and give the attention map the gradient of the out-of-place formula."""
    torch.manual_seed(4)
    net = dmcnet_amd.model.ContextNetworkAtt(5, True, 0).train()
    x, f = torch.randn(2, 5, 16, 16), torch.randn(2, 2, 16, 16)
    gen, att = net(x)
    assert float(att.min()) == 0.0                                  # a ReLU head: exact zeros
    train.flow_loss("SmoothL1Loss", gen, f, att).backward()
    g = net.predict_att[0][0].weight.grad
    assert g is not None and bool(torch.isfinite(g).all()) and float(g.abs().max()) > 0.0
