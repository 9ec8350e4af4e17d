"""CPU: the host side of the ContextNetwork training BatchNorm + LeakyReLU (csrc/ctx_bn.hip, ops.bn_leaky, model.CTX_TRAIN_BN).

The header declares the four dmc_bnlrelu_* entry points, the library exports them and _lib.SIGNATURES binds them; the queries run
without a GPU; every refusal of the two launching entry points happens before any launch with the entry point's name in
dmc_last_error(); the flag is off by default, read once, and with both flags forced on CPU networks stay on the stock modules
bit for bit; ops.bn_leaky has no CPU fallback; the fp64 reference of tests/ctx_bn_ref.py agrees with torch's autograd; the seed
table of the op-level GPU cases is what the kink criterion returns."""
import copy
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from dmcnet_amd import _lib, model, ops
from oracle import dmc_oracle as O
from tests import ctx_bn_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["dmc_bnlrelu_bwd", "dmc_bnlrelu_fwd", "dmc_bnlrelu_scratch_bytes", "dmc_bnlrelu_supported"]
WIDTHS = (32, 64, 96, 128)


def rnd(seed, shape):
    return torch.from_numpy(np.random.RandomState(seed).standard_normal(shape).astype(np.float32))


def test_header_library_and_signatures_have_the_entry_points():
    import __graft_entry__ as g
    g.build()
    text = open(os.path.join(ROOT, "include", "dmcnet_hip.h")).read()
    comments = " ".join(re.findall(r"/\*.*?\*/", text, flags=re.S))
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(dmc_[a-z0-9_]+)\s*\(", code))
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW:
        assert name in declared, name + " is not declared in include/dmcnet_hip.h"
        assert hasattr(lib, name), "libdmcnet_hip.so does not export " + name
        assert name in _lib.SIGNATURES, name
        assert re.search(name + r" \(code/dmcnet/model\.py:45-104\)", comments), name + " does not cite the reference"
    assert sorted(n for n in declared if n.startswith("dmc_bnlrelu_")) == NEW
    assert re.search(r"Replaces: nn\.BatchNorm2d[^/]*code/dmcnet/model\.py:45-104", comments, flags=re.S)
    I, Z, P, F = ctypes.c_int, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_float
    assert _lib.SIGNATURES["dmc_bnlrelu_supported"] == (I, [I, I])
    assert _lib.SIGNATURES["dmc_bnlrelu_scratch_bytes"] == (Z, [I, I])
    assert _lib.SIGNATURES["dmc_bnlrelu_fwd"] == (I, [P] * 8 + [I, I, F, F, F, P])
    assert _lib.SIGNATURES["dmc_bnlrelu_bwd"] == (I, [P] * 9 + [I, I, F, P])
    assert "ctx_bn.hip" in __import__("dmcnet_amd.build", fromlist=["SOURCES"]).SOURCES


def test_queries_without_gpu():
    lib = _lib.load()
    for c in range(0, 161, 16):
        for m in (2, 105, 8601, 24 * 224 * 224):
            want = int(c in WIDTHS)
            assert lib.dmc_bnlrelu_supported(m, c) == want, (m, c)
            assert (lib.dmc_bnlrelu_scratch_bytes(m, c) > 0) == bool(want), (m, c)
        for m in (1, 0, -3):
            assert lib.dmc_bnlrelu_supported(m, c) == 0 and lib.dmc_bnlrelu_scratch_bytes(m, c) == 0, (m, c)
    for c in (4, 8, 24, 100, 256):
        assert lib.dmc_bnlrelu_supported(1188, c) == 0 and lib.dmc_bnlrelu_scratch_bytes(1188, c) == 0
    for c in WIDTHS:                                              # the index bound: M C < 2^31
        m = -(-2 ** 31 // c)                                       # the first M with M C >= 2^31 (= 2^31 except at C = 96)
        assert (m - 1) * c < 2 ** 31 <= m * c and (c == 96 or m * c == 2 ** 31)
        assert lib.dmc_bnlrelu_supported(m, c) == 0 and lib.dmc_bnlrelu_scratch_bytes(m, c) == 0
        assert lib.dmc_bnlrelu_supported(m - 1, c) == 1 and lib.dmc_bnlrelu_scratch_bytes(m - 1, c) > 0
        # exactly the partials [C][workgroups][2] fp64 and the backward's 2 C floats (ctx_bn_ref mirrors the launch geometry)
        for m in (2, 105, 1188, 8601, R.M_GEOMETRY, 24 * 224 * 224):
            assert lib.dmc_bnlrelu_scratch_bytes(m, c) == R.blocks_of(m, c) * c * 16 + 8 * c, (m, c)


def _fwd_args(p, **kw):
    a = dict(z=p, gamma=p, beta=p, rm=p, rv=p, y=p, stats=p, scratch=p, M=8, C=32, slope=0.1, eps=1e-5, momentum=0.1)
    a.update(kw)
    return [a[k] for k in ("z", "gamma", "beta", "rm", "rv", "y", "stats", "scratch", "M", "C", "slope", "eps", "momentum")] + [None]


def _bwd_args(p, **kw):
    a = dict(z=p, dy=p, gamma=p, beta=p, stats=p, scratch=p, dz=p, dgamma=p, dbeta=p, M=8, C=32, slope=0.1)
    a.update(kw)
    return [a[k] for k in ("z", "dy", "gamma", "beta", "stats", "scratch", "dz", "dgamma", "dbeta", "M", "C", "slope")] + [None]


def test_refusals_are_loud_and_launch_nothing():
    """Every refusal returns DMC_E_INVALID from the argument checks, in front of the first launch: there is no GPU here, so a call
    that got as far as a launch would come back with DMC_E_LAUNCH instead."""
    lib = _lib.load()
    p = _lib.ptr(torch.zeros(16))                                 # any non-null pointer: nothing is launched

    def refused(name, rc):
        assert rc == -1, (name, rc, lib.dmc_last_error())
        assert name.encode() in lib.dmc_last_error(), (name, lib.dmc_last_error())

    for k in ("z", "gamma", "beta", "y", "stats", "scratch"):
        refused("dmc_bnlrelu_fwd", lib.dmc_bnlrelu_fwd(*_fwd_args(p, **{k: None})))
    refused("dmc_bnlrelu_fwd", lib.dmc_bnlrelu_fwd(*_fwd_args(p, rm=None)))          # exactly one running pointer
    refused("dmc_bnlrelu_fwd", lib.dmc_bnlrelu_fwd(*_fwd_args(p, rv=None)))
    for k in ("z", "dy", "gamma", "beta", "stats", "scratch", "dz", "dgamma", "dbeta"):
        refused("dmc_bnlrelu_bwd", lib.dmc_bnlrelu_bwd(*_bwd_args(p, **{k: None})))
    for m, c in ((8, 48), (8, 0), (8, 160), (1, 32), (0, 64), (2 ** 31 // 128, 128)):
        refused("dmc_bnlrelu_fwd", lib.dmc_bnlrelu_fwd(*_fwd_args(p, M=m, C=c)))
        assert b"unsupported shape" in lib.dmc_last_error()
        refused("dmc_bnlrelu_bwd", lib.dmc_bnlrelu_bwd(*_bwd_args(p, M=m, C=c)))
        assert b"unsupported shape" in lib.dmc_last_error()
    for eps in (0.0, -1e-5, float("nan")):
        refused("dmc_bnlrelu_fwd", lib.dmc_bnlrelu_fwd(*_fwd_args(p, eps=eps)))
    for slope in (0.0, -0.1, 1.0, 1.5, float("nan")):
        refused("dmc_bnlrelu_fwd", lib.dmc_bnlrelu_fwd(*_fwd_args(p, slope=slope)))
        refused("dmc_bnlrelu_bwd", lib.dmc_bnlrelu_bwd(*_bwd_args(p, slope=slope)))
    for mom in (-0.01, 1.01, float("nan")):
        refused("dmc_bnlrelu_fwd", lib.dmc_bnlrelu_fwd(*_fwd_args(p, momentum=mom)))


def test_flag_is_off_by_default_and_read_from_the_environment_once():
    code = "import sys; sys.path.insert(0, %r); from dmcnet_amd import model; print(int(model.CTX_TRAIN_BN))" % ROOT
    for value, want in ((None, "0"), ("0", "0"), ("1", "1")):
        env = dict(os.environ)
        env.pop("DMC_CTX_TRAIN_BN", None)
        if value is not None:
            env["DMC_CTX_TRAIN_BN"] = value
        out = subprocess.run([sys.executable, "-c", code], env=env, stdout=subprocess.PIPE, check=True, universal_newlines=True).stdout
        assert out.strip().splitlines()[-1] == want, (value, out)
    if os.environ.get("DMC_CTX_TRAIN_BN", "0") != "1":
        assert model.CTX_TRAIN_BN is False


def _stock(net, x):
    if isinstance(net, model.ContextNetworkAtt):
        t = net.conv_context(x)
        return net.predict_flow(t), net.predict_att(t)
    return (net.conv_context(x),)


@pytest.mark.parametrize("att,ds", [(0, 0), (0, 16), (1, 0), (1, 16)])
def test_both_flags_on_keep_cpu_networks_on_the_stock_modules(att, ds, monkeypatch):
    monkeypatch.setattr(model, "CTX_TRAIN", True)
    monkeypatch.setattr(model, "CTX_TRAIN_BN", True)
    cls = model.ContextNetworkAtt if att else model.ContextNetwork
    net0 = O.seeded_state_fill(cls(5, True, ds), 3).train()
    x = rnd(1, (2, 5, 12, 9))
    r = rnd(2, (2, 2, 12, 9))
    unit = net0.conv_context[1]
    assert not ops.bn_leaky_supported(rnd(5, (2, 128, 12, 9)), unit[1], unit[2])      # a CPU tensor, CPU parameters

    def run(fwd):
        net = copy.deepcopy(net0)
        xi = x.clone().requires_grad_(True)
        outs = fwd(net, xi)
        outs = outs if isinstance(outs, tuple) else (outs,)
        sum((t * r).sum() for t in outs).backward()
        return [t.detach() for t in outs] + [xi.grad] + [p.grad for p in net.parameters()] + list(net.buffers())

    a, b = run(lambda net, xi: net(xi)), run(_stock)
    assert len(a) == len(b)
    for s, t in zip(a, b):
        assert torch.equal(s, t)
    with pytest.raises(_lib.DmcHipError):
        ops.context_train(net0, x, fused_bn=True)


def test_bn_leaky_has_no_cpu_fallback():
    bn = torch.nn.BatchNorm2d(32).train()
    before = copy.deepcopy(bn.state_dict())
    with pytest.raises(_lib.DmcHipError):
        ops.bn_leaky(rnd(1, (2, 32, 5, 7)), bn, 0.1)
    with pytest.raises(_lib.DmcHipError):
        ops.bn_leaky(rnd(1, (2, 32, 5, 7)).contiguous(memory_format=torch.channels_last).requires_grad_(True), bn, 0.1)
    for k, v in bn.state_dict().items():                          # nothing was counted or updated on the way to the refusal
        assert torch.equal(v, before[k]), k


@pytest.mark.parametrize("shape,seed", [((2, 32, 1, 1), 1), ((3, 96, 7, 5), 2), ((2, 128, 33, 18), 3)], ids=["2x32", "105x96", "1188x128"])
def test_reference_agrees_with_torch_autograd_in_fp64(shape, seed):
    """forward_ref / backward_ref / running_ref against BatchNorm2d().double() + LeakyReLU(0.1) and its autograd, to 1e-12 of the
    largest value; a third of one channel sits at t == 0 exactly and takes the slope in both."""
    n, c, h, w = shape
    M = n * h * w
    case = R.crafted_case(M, c, 5, seed) if M % 3 == 0 else R.bn_case(M, c, seed)
    z, dy, gamma, beta = (case[k].double() for k in ("z", "dy", "gamma", "beta"))
    slope = R.f32(R.SLOPE)
    bn = torch.nn.BatchNorm2d(c, eps=R.f32(R.EPS), momentum=R.f32(R.MOMENTUM)).double().train()
    with torch.no_grad():
        bn.weight.copy_(gamma)
        bn.bias.copy_(beta)
        bn.running_mean.copy_(case["rm"])
        bn.running_var.copy_(case["rv"])
    x4 = z.view(n, h, w, c).permute(0, 3, 1, 2).clone().requires_grad_(True)
    y4 = torch.nn.LeakyReLU(slope)(bn(x4))
    y4.backward(dy.view(n, h, w, c).permute(0, 3, 1, 2))
    mean, var, invstd = R.stats_ref(z)
    y, t, _ = R.forward_ref(z, gamma, beta, mean, invstd)
    dz, dgamma, dbeta = R.backward_ref(z, dy, gamma, mean, invstd, t > 0)
    rm, rv = R.running_ref(mean, var, M, case["rm"], case["rv"])
    if M % 3 == 0:
        zero = z[:, 5] == 0
        assert int(zero.sum()) == M // 3 and bool((t[:, 5][zero] == 0).all()) and bool((y[:, 5][zero] == 0).all())
        # at t == 0 the gradient passes multiplied by the slope, not by 1: the other choice is far outside 1e-12
        dz1, _, _ = R.backward_ref(z, dy, gamma, mean, invstd, t >= 0)
        assert float((dz1 - dz).abs().max()) > 1e-3

    def close(a, b):
        assert float((a - b).abs().max()) <= 1e-12 * float(b.abs().max()), float((a - b).abs().max())

    close(y, y4.detach().permute(0, 2, 3, 1).reshape(M, c))
    close(dz, x4.grad.permute(0, 2, 3, 1).reshape(M, c))
    close(dgamma, bn.weight.grad)
    close(dbeta, bn.bias.grad)
    close(rm, bn.running_mean)
    close(rv, bn.running_var)


@pytest.mark.parametrize("case", R.OP_CASES, ids=["%dx%d-%s" % c for c in R.OP_CASES])
def test_op_seeds_are_what_the_kink_criterion_returns(case):
    """tests/test_ctx_bn_gpu.py draws its operands at the first seed from 51 upwards at which the fp64 reference alone keeps every
    BatchNorm output at |t| >= 2^-20 max |t| (at 8601 x 128 about one seed in 60 does; 400 tries, as tests/test_dconv_gpu.py)."""
    assert sorted(R.OP_SEEDS) == sorted(R.OP_CASES)
    assert R.OP_SEEDS[case] == R.kink_free_seed(*case)
