"""CPU: the host side of the two ends of the ContextNetwork training route (csrc/ctx_ends.hip, ops.ctx_first_conv,
ops.ctx_head_convs, ops.bn_leaky_planes, model.CTX_TRAIN_ENDS).

The header declares the eleven dmc_ctxends_* entry points, the library exports them and _lib.SIGNATURES binds them; the queries
run without a GPU and are exact at their edges; every refusal of the eight launching entry points happens before any launch with
the entry point's name in dmc_last_error(); the flag is off by default and read once; the predicates are False and the ops raise
on CPU tensors; the fp64 references of tests/ctx_ends_ref.py agree with torch's autograd; the seed table is what the kink
criterion returns."""
import copy
import ctypes
import inspect
import os
import re
import subprocess
import sys

import pytest
import torch

from dmcnet_amd import _lib, model, ops
from oracle import dmc_oracle as O
from tests import ctx_bn_ref as R
from tests import ctx_ends_ref as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["dmc_ctxends_bn_bwd", "dmc_ctxends_bn_fwd", "dmc_ctxends_bn_scratch_bytes", "dmc_ctxends_first_dgrad", "dmc_ctxends_first_fwd",
       "dmc_ctxends_first_wgrad", "dmc_ctxends_heads_dgrad", "dmc_ctxends_heads_fwd", "dmc_ctxends_heads_wgrad", "dmc_ctxends_supported",
       "dmc_ctxends_wgrad_workspace_bytes"]


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
    assert sorted(n for n in declared if n.startswith("dmc_ctxends_")) == NEW
    assert sorted(n for n in _lib.SIGNATURES if n.startswith("dmc_ctxends_")) == NEW
    I, Z, P, F = ctypes.c_int, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_float
    S = _lib.SIGNATURES
    assert S["dmc_ctxends_supported"] == (I, [I] * 3)
    assert S["dmc_ctxends_wgrad_workspace_bytes"] == (Z, [I] * 4)
    assert S["dmc_ctxends_bn_scratch_bytes"] == (Z, [I] * 3)
    assert S["dmc_ctxends_first_fwd"] == S["dmc_ctxends_first_dgrad"] == (I, [P] * 3 + [I] * 3 + [P])
    assert S["dmc_ctxends_first_wgrad"] == (I, [P] * 4 + [I] * 3 + [P])
    assert S["dmc_ctxends_heads_fwd"] == S["dmc_ctxends_heads_dgrad"] == (I, [P] * 5 + [I] * 3 + [P])
    assert S["dmc_ctxends_heads_wgrad"] == (I, [P] * 6 + [I] * 3 + [P])
    assert S["dmc_ctxends_bn_fwd"] == (I, [P] * 8 + [I] * 3 + [F, F, F, I, P])
    assert S["dmc_ctxends_bn_bwd"] == (I, [P] * 9 + [I] * 3 + [F, I, P])
    assert "ctx_ends.hip" in __import__("dmcnet_amd.build", fromlist=["SOURCES"]).SOURCES


def test_queries_without_gpu():
    lib = _lib.load()
    # the index bound every ContextNetwork entry point has: N H W 128 < 2^31 -- 334 frames of 224 x 224 pass, 335 do not
    assert 334 * 224 * 224 * 128 < 2 ** 31 <= 335 * 224 * 224 * 128
    for n, want in ((334, 1), (335, 0)):
        assert lib.dmc_ctxends_supported(n, 224, 224) == want
        for planes in (2, 4, 5):
            assert lib.dmc_ctxends_wgrad_workspace_bytes(n, 224, 224, planes) == want * E.wgrad_workspace_bytes(n, 224, 224, planes)
        assert lib.dmc_ctxends_bn_scratch_bytes(n, 224, 224) == want * E.bn_scratch_bytes(n, 224, 224)
    for shape in ((0, 5, 5), (5, 0, 5), (5, 5, 0), (-1, 5, 5), (5, -2, 5), (5, 5, -3), (0, 0, 0)):
        assert lib.dmc_ctxends_supported(*shape) == 0
        assert lib.dmc_ctxends_bn_scratch_bytes(*shape) == 0
        assert lib.dmc_ctxends_wgrad_workspace_bytes(*(shape + (5,))) == 0
    # N H W = 1: the convolutions serve it, the BatchNorm (unbiased variance over M - 1) does not
    assert lib.dmc_ctxends_supported(1, 1, 1) == 1 and lib.dmc_ctxends_bn_scratch_bytes(1, 1, 1) == 0
    assert lib.dmc_ctxends_bn_scratch_bytes(2, 1, 1) == lib.dmc_ctxends_bn_scratch_bytes(1, 2, 1) == 48
    for planes in (-1, 0, 1, 3, 6, 32):
        assert lib.dmc_ctxends_wgrad_workspace_bytes(2, 21, 17, planes) == 0
    for n, h, w in E.SHAPES + [(24, 224, 224)]:
        assert lib.dmc_ctxends_supported(n, h, w) == 1
        for planes in (2, 4, 5):
            assert lib.dmc_ctxends_wgrad_workspace_bytes(n, h, w, planes) == E.wgrad_workspace_bytes(n, h, w, planes) > 0
        if n * h * w >= 2:
            assert lib.dmc_ctxends_bn_scratch_bytes(n, h, w) == E.bn_scratch_bytes(n, h, w)
    # the range and the LDS threshold the GPU shapes are chosen around: each wide shape puts one more plane count on the global path
    assert [[bool(E.stage_bytes(k, w)) for k in (5, 4, 2)] for w in (47, 383, 384, 400, 735, 736, 740, 2495, 2496, 2500)] == [
        [True, True, True], [True, True, True], [False, True, True], [False, True, True], [False, True, True], [False, False, True],
        [False, False, True], [False, False, True], [False, False, False], [False, False, False]]
    assert E.nranges(2048) == 1 and E.nranges(2049) == 2 and E.nranges(8601) == 5 and 8601 % E.RANGE == 409


ARGS = {
    "dmc_ctxends_first_fwd": ("x", "w", "z"),
    "dmc_ctxends_first_dgrad": ("dz", "w", "dx"),
    "dmc_ctxends_first_wgrad": ("x", "dz", "dw", "workspace"),
    "dmc_ctxends_heads_fwd": ("t", "w_flow", "w_att", "z_flow", "z_att"),
    "dmc_ctxends_heads_dgrad": ("dz_flow", "dz_att", "w_flow", "w_att", "dt"),
    "dmc_ctxends_heads_wgrad": ("t", "dz_flow", "dz_att", "dw_flow", "dw_att", "workspace"),
    "dmc_ctxends_bn_fwd": ("z", "gamma", "beta", "running_mean", "running_var", "y", "stats", "scratch"),
    "dmc_ctxends_bn_bwd": ("z", "dy", "gamma", "beta", "stats", "scratch", "dz", "dgamma", "dbeta"),
}
#: per entry point: the pointer sets whose absence is a refusal (everything else may be NULL in some combination)
NULL_REFUSED = {
    "dmc_ctxends_first_fwd": [("x",), ("w",), ("z",)],
    "dmc_ctxends_first_dgrad": [("dz",), ("w",), ("dx",)],
    "dmc_ctxends_first_wgrad": [("x",), ("dz",), ("dw",), ("workspace",)],
    "dmc_ctxends_heads_fwd": [("t",), ("w_flow",), ("z_flow",), ("w_att",), ("z_att",)],                       # the last two: half a group
    "dmc_ctxends_heads_dgrad": [("w_flow",), ("dt",), ("w_att",), ("dz_flow", "dz_att"), ("dz_flow", "dz_att", "w_att")],
    "dmc_ctxends_heads_wgrad": [("t",), ("workspace",), ("dz_flow",), ("dw_flow",), ("dz_att",), ("dw_att",),
                                ("dz_flow", "dw_flow", "dz_att", "dw_att")],
    "dmc_ctxends_bn_fwd": [("z",), ("gamma",), ("beta",), ("y",), ("stats",), ("scratch",), ("running_mean",), ("running_var",)],
    "dmc_ctxends_bn_bwd": [(k,) for k in ARGS["dmc_ctxends_bn_bwd"]],
}


def call(name, p, null=(), shape=(2, 3, 4), **kw):
    lib = _lib.load()
    args = [None if k in null else p for k in ARGS[name]] + list(shape)
    if name == "dmc_ctxends_bn_fwd":
        args += [kw.get("slope", 0.1), kw.get("eps", 1e-5), kw.get("momentum", 0.1), kw.get("relu", 0)]
    elif name == "dmc_ctxends_bn_bwd":
        args += [kw.get("slope", 0.1), kw.get("relu", 0)]
    return getattr(lib, name)(*(args + [None]))


def test_refusals_are_loud_and_launch_nothing():
    """Every refusal returns DMC_E_INVALID from the argument checks, in front of the first launch: there is no GPU here, so a call
    that got as far as a launch would come back with DMC_E_LAUNCH instead."""
    lib = _lib.load()
    p = _lib.ptr(torch.zeros(16))                                 # any non-null pointer: nothing is launched

    def refused(name, rc):
        assert rc == -1, (name, rc, lib.dmc_last_error())
        assert name.encode() in lib.dmc_last_error(), (name, lib.dmc_last_error())

    assert sorted(ARGS) == sorted(n for n in NEW if not n.endswith(("_supported", "_bytes")))
    for name in ARGS:
        for null in NULL_REFUSED[name]:
            refused(name, call(name, p, null=null))
        for shape in ((0, 3, 4), (2, 0, 4), (2, 3, 0), (-2, 3, 4), (335, 224, 224)):
            refused(name, call(name, p, shape=shape))
            assert b"unsupported shape" in lib.dmc_last_error()
    for name in ("dmc_ctxends_bn_fwd", "dmc_ctxends_bn_bwd"):
        refused(name, call(name, p, shape=(1, 1, 1)))             # N H W = 1
        assert b"unsupported shape" in lib.dmc_last_error()
        for slope in (0.0, -0.1, 1.0, 1.5, float("nan")):
            refused(name, call(name, p, slope=slope))
    for eps in (0.0, -1e-5, float("nan")):
        refused("dmc_ctxends_bn_fwd", call("dmc_ctxends_bn_fwd", p, eps=eps))
    for mom in (-0.01, 1.01, float("nan")):
        refused("dmc_ctxends_bn_fwd", call("dmc_ctxends_bn_fwd", p, momentum=mom))


def test_flag_is_off_by_default_and_read_from_the_environment_once():
    code = "import sys; sys.path.insert(0, %r); from dmcnet_amd import model; print(int(model.CTX_TRAIN_ENDS))" % ROOT
    for value, want in ((None, "0"), ("0", "0"), ("1", "1")):
        env = dict(os.environ)
        env.pop("DMC_CTX_TRAIN_ENDS", None)
        if value is not None:
            env["DMC_CTX_TRAIN_ENDS"] = value
        out = subprocess.run([sys.executable, "-c", code], env=env, stdout=subprocess.PIPE, check=True, universal_newlines=True).stdout
        assert out.strip().splitlines()[-1] == want, (value, out)
    if os.environ.get("DMC_CTX_TRAIN_ENDS", "0") != "1":
        assert model.CTX_TRAIN_ENDS is False
    assert inspect.signature(ops.context_train).parameters["own_ends"].default is False


def test_predicates_are_false_and_the_ops_raise_on_the_cpu():
    first = torch.nn.Conv2d(5, 32, 3, 1, 1, 1, bias=False)
    head = torch.nn.Conv2d(32, 2, 3, 1, 1, 1, bias=False)
    bn, act = torch.nn.BatchNorm2d(2).train(), torch.nn.LeakyReLU(0.1)
    x, t, z = E.rnd(1, (2, 5, 6, 7)), E.rnd(2, (2, 32, 6, 7)), E.rnd(3, (2, 2, 6, 7))
    assert not ops.ctx_first_conv_supported(x, first)
    assert not ops.ctx_head_convs_supported(t, [head]) and not ops.ctx_head_convs_supported(t, [head, copy.deepcopy(head)])
    assert not ops.bn_leaky_planes_supported(z, bn, act) and not ops.bn_leaky_planes_supported(z, bn, act, torch.nn.ReLU())
    before = copy.deepcopy(bn.state_dict())
    with pytest.raises(_lib.DmcHipError):
        ops.ctx_first_conv(x, first.weight)
    with pytest.raises(_lib.DmcHipError):
        ops.ctx_head_convs(t, [head.weight])
    with pytest.raises(_lib.DmcHipError):
        ops.bn_leaky_planes(z, bn, 0.1)
    with pytest.raises(_lib.DmcHipError):
        ops.bn_leaky_planes(z.requires_grad_(True), bn, 0.1, relu=True)
    for k, v in bn.state_dict().items():                          # nothing was counted or updated on the way to the refusal
        assert torch.equal(v, before[k]), k


@pytest.mark.parametrize("att", [0, 1])
def test_all_flags_on_keep_cpu_networks_on_the_stock_modules(att, monkeypatch):
    for flag in ("CTX_TRAIN", "CTX_TRAIN_BN", "CTX_TRAIN_ENDS"):
        monkeypatch.setattr(model, flag, True)
    cls = model.ContextNetworkAtt if att else model.ContextNetwork
    net0 = O.seeded_state_fill(cls(5, True, 0), 3).train()
    x, r = E.rnd(1, (2, 5, 12, 9)), E.rnd(2, (2, 2, 12, 9))

    def run(fwd):
        net = copy.deepcopy(net0)
        xi = x.clone().requires_grad_(True)
        outs = fwd(net, xi)
        outs = outs if isinstance(outs, tuple) else (outs,)
        sum((t * r).sum() for t in outs).backward()
        return [t.detach() for t in outs] + [xi.grad] + [p.grad for p in net.parameters()] + list(net.buffers())

    def stock(net, xi):
        if att:
            t = net.conv_context(xi)
            return net.predict_flow(t), net.predict_att(t)
        return net.conv_context(xi)

    for s, t in zip(run(lambda net, xi: net(xi)), run(stock)):
        assert torch.equal(s, t)
    with pytest.raises(_lib.DmcHipError):
        ops.context_train(net0, x, fused_bn=True, own_ends=True)


def close(a, b):
    assert float((a - b).abs().max()) <= 1e-12 * float(b.abs().max()), float((a - b).abs().max())


@pytest.mark.parametrize("shape", [(2, 2, 3), (2, 21, 17)], ids=["2x2x3", "2x21x17"])
def test_convolution_references_agree_with_stock_modules_in_fp64(shape):
    """first_case / heads_case against nn.Conv2d().double() modules of the network's own form and their autograd; the heads' data
    gradient of the network is the sum of the two per-head references."""
    n, h, w = shape
    c = E.first_case(n, h, w)
    conv = torch.nn.Conv2d(5, 32, 3, 1, 1, 1, bias=False).double()
    with torch.no_grad():
        conv.weight.copy_(c["w"])
    x = c["x"].double().requires_grad_(True)
    z = conv(x)
    z.backward(c["dz"].double())
    close(c["z"], z.detach()); close(c["dx"], x.grad); close(c["dw"], conv.weight.grad)
    hc = E.heads_case(n, h, w)
    heads = [torch.nn.Conv2d(32, 2, 3, 1, 1, 1, bias=False).double() for _ in range(2)]
    t = hc["t"].double().requires_grad_(True)
    zs = []
    for k, m in enumerate(heads):
        with torch.no_grad():
            m.weight.copy_(hc["w"][k])
        zs.append(m(t))
    sum((z * dz.double()).sum() for z, dz in zip(zs, hc["dz"])).backward()
    for k in range(2):
        close(hc["z"][k], zs[k].detach()); close(hc["dw"][k], heads[k].weight.grad)
    close(hc["dt"][0] + hc["dt"][1], t.grad)


@pytest.mark.parametrize("relu", [0, 1])
@pytest.mark.parametrize("shape", [(2, 2, 3), (2, 21, 17), (2, 33, 18)], ids=["2x2x3", "2x21x17", "2x33x18-crafted"])
def test_plane_references_agree_with_torch_autograd_in_fp64(shape, relu):
    """forward_ref / backward_ref / running_ref on the [M][2] rows of the planes against BatchNorm2d(2).double() + LeakyReLU(0.1)
    (+ ReLU) on the contiguous planes and its autograd, to 1e-12 of the largest value.  In the crafted case a third of channel 1
    sits at t == 0 exactly: it takes the slope (0 under the ReLU) in both."""
    n, h, w = shape
    M = n * h * w
    case = E.crafted_case() if shape == (2, 33, 18) else E.bn_case(n, h, w)
    z, dy, gamma, beta = (case[k].double() for k in ("z", "dy", "gamma", "beta"))
    bn = torch.nn.BatchNorm2d(2, eps=R.f32(E.EPS), momentum=R.f32(E.MOMENTUM)).double().train()
    with torch.no_grad():
        bn.weight.copy_(gamma); bn.bias.copy_(beta); bn.running_mean.copy_(case["rm"]); bn.running_var.copy_(case["rv"])
    x4 = E.to_planes(z, n, h, w).requires_grad_(True)
    y4 = torch.nn.LeakyReLU(R.f32(E.SLOPE))(bn(x4))
    if relu:
        y4 = torch.nn.ReLU()(y4)
    y4.backward(E.to_planes(dy, n, h, w))
    mean, var, invstd = R.stats_ref(z)
    y, t, _ = E.forward_ref(z, gamma, beta, mean, invstd, relu)
    dz, dgamma, dbeta = E.backward_ref(z, dy, gamma, mean, invstd, t > 0, relu)
    rm, rv = R.running_ref(mean, var, M, case["rm"], case["rv"])
    if shape == (2, 33, 18):
        zero = z[:, 1] == 0
        assert int(zero.sum()) == M // 3 and bool((t[:, 1][zero] == 0).all()) and bool((y[:, 1][zero] == 0).all())
        dz1, _, _ = E.backward_ref(z, dy, gamma, mean, invstd, t >= 0, relu)
        assert float((dz1 - dz).abs().max()) > 1e-3
    close(y, E.to_rows(y4.detach())); close(dz, E.to_rows(x4.grad))
    close(dgamma, bn.weight.grad); close(dbeta, bn.bias.grad)
    close(rm, bn.running_mean); close(rv, bn.running_var)


def test_seeds_are_what_the_kink_criterion_returns():
    assert sorted(E.BN_SEEDS) == sorted({n * h * w for n, h, w in E.BN_SHAPES})
    for m, seed in E.BN_SEEDS.items():
        assert seed == R.kink_free_seed(m, 2, "normal"), m
    c = E.crafted_case()                                           # the crafted channel aside, seed 51 keeps its margin there too
    mean, _, invstd = R.stats_ref(c["z"])
    _, t, _ = R.forward_ref(c["z"], c["gamma"], c["beta"], mean, invstd)
    assert float(t[:, 0].abs().min() / t.abs().max()) >= R.KINK_MARGIN
