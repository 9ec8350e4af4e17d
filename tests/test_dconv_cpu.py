"""CPU: the host side of the ContextNetwork training route (csrc/dconv.hip, ops.dilated_conv, model.CTX_TRAIN).

The header declares the six dmc_dconv_* entry points, the library exports them and _lib.SIGNATURES binds them; the queries run
without a GPU (the supported set, the index bound, the pack and workspace sizes); every launching entry point refuses null
pointers and unsupported shapes before any launch with its name in dmc_last_error(); the flag is off by default and, switched
on, leaves CPU networks on the stock modules bit for bit; ops.dilated_conv has no CPU fallback."""
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

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["dmc_dconv_fwd", "dmc_dconv_pack_weights", "dmc_dconv_supported", "dmc_dconv_wgrad", "dmc_dconv_wgrad_workspace_bytes",
       "dmc_dconv_wpack_bytes"]
WIDTHS = (32, 64, 96, 128)
DILATIONS = (1, 2, 4, 8, 16)


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
    assert sorted(n for n in declared if n.startswith("dmc_dconv_")) == NEW
    I, Z, P = ctypes.c_int, ctypes.c_size_t, ctypes.c_void_p
    assert _lib.SIGNATURES["dmc_dconv_supported"] == (I, [I] * 6)
    assert _lib.SIGNATURES["dmc_dconv_wpack_bytes"] == (Z, [I] * 2)
    assert _lib.SIGNATURES["dmc_dconv_wgrad_workspace_bytes"] == (Z, [I] * 5)
    assert _lib.SIGNATURES["dmc_dconv_pack_weights"] == (I, [P, P, I, I, I, P])
    assert _lib.SIGNATURES["dmc_dconv_fwd"] == (I, [P] * 3 + [I] * 6 + [P])
    assert _lib.SIGNATURES["dmc_dconv_wgrad"] == (I, [P] * 4 + [I] * 6 + [P])


def test_queries_without_gpu():
    lib = _lib.load()
    for cin in range(0, 161, 16):
        for cout in range(0, 161, 16):
            for d in range(0, 34):
                want = int(cin in WIDTHS and cout in WIDTHS and d in DILATIONS)
                assert lib.dmc_dconv_supported(2, 20, 20, cin, cout, d) == want, (cin, cout, d)
                # a dilation the eval route's middle units accept, and no other
                assert want == int(cin in WIDTHS and cout in WIDTHS and lib.dmc_ctx_unit_supported(2, 20, 20, cin, cout, d))
    for cin, cout in ((5, 32), (32, 2), (48, 64), (64, 48), (256, 128)):
        assert lib.dmc_dconv_supported(2, 20, 20, cin, cout, 1) == 0
        assert lib.dmc_dconv_wpack_bytes(cin, cout) == 0
        assert lib.dmc_dconv_wgrad_workspace_bytes(2, 20, 20, cin, cout) == 0
    for n, h, w in ((0, 8, 8), (1, 0, 8), (1, 8, -1)):
        assert lib.dmc_dconv_supported(n, h, w, 32, 128, 2) == 0
        assert lib.dmc_dconv_wgrad_workspace_bytes(n, h, w, 32, 128) == 0
    # the index bound: N H W 128 < 2^31
    assert 334 * 224 * 224 * 128 < 2 ** 31 <= 335 * 224 * 224 * 128
    for cin in WIDTHS:
        for cout in WIDTHS:
            assert lib.dmc_dconv_supported(334, 224, 224, cin, cout, 4) == 1
            assert lib.dmc_dconv_supported(335, 224, 224, cin, cout, 4) == 0
            assert lib.dmc_dconv_wpack_bytes(cin, cout) == cin * cout * 9 * 3 * 2
            for n, h, w in ((1, 1, 1), (1, 20, 37), (24, 224, 224), (334, 224, 224)):
                ws = lib.dmc_dconv_wgrad_workspace_bytes(n, h, w, cin, cout)
                assert ws > 0 and ws % (cin * cout * 9 * 4) == 0, (n, h, w, cin, cout, ws)
            assert lib.dmc_dconv_wgrad_workspace_bytes(335, 224, 224, cin, cout) == 0


def test_refusals_are_loud_and_launch_nothing():
    lib = _lib.load()
    p = _lib.ptr(torch.zeros(16))                                 # any non-null pointer: nothing is launched

    def refused(name, rc):
        assert rc == -1, name
        assert name.encode() in lib.dmc_last_error(), (name, lib.dmc_last_error())

    good = (1, 8, 8, 32, 128, 2)
    for i in range(3):
        a = [p] * 3
        a[i] = None
        refused("dmc_dconv_fwd", lib.dmc_dconv_fwd(*a, *good, None))
    for i in range(4):
        a = [p] * 4
        a[i] = None
        refused("dmc_dconv_wgrad", lib.dmc_dconv_wgrad(*a, *good, None))
    for tr in (0, 1):
        refused("dmc_dconv_pack_weights", lib.dmc_dconv_pack_weights(None, p, 32, 128, tr, None))
        refused("dmc_dconv_pack_weights", lib.dmc_dconv_pack_weights(p, None, 32, 128, tr, None))
        refused("dmc_dconv_pack_weights", lib.dmc_dconv_pack_weights(p, p, 48, 128, tr, None))
        refused("dmc_dconv_pack_weights", lib.dmc_dconv_pack_weights(p, p, 32, 48, tr, None))
    for shape in ((1, 8, 8, 48, 64, 1), (1, 8, 8, 64, 48, 1), (1, 8, 8, 32, 128, 3), (0, 8, 8, 32, 128, 2), (335, 224, 224, 128, 128, 4),
                  (1, 8, 8, 5, 32, 1), (1, 8, 8, 32, 2, 1)):
        refused("dmc_dconv_fwd", lib.dmc_dconv_fwd(p, p, p, *shape, None))
        assert b"unsupported shape" in lib.dmc_last_error() and str(shape[3]).encode() in lib.dmc_last_error()
        refused("dmc_dconv_wgrad", lib.dmc_dconv_wgrad(p, p, p, p, *shape, None))
        assert b"unsupported shape" in lib.dmc_last_error()


def test_flag_is_off_by_default_and_read_from_the_environment_once():
    code = "import sys; sys.path.insert(0, %r); from dmcnet_amd import model; print(int(model.CTX_TRAIN))" % ROOT
    for value, want in ((None, "0"), ("0", "0"), ("1", "1")):
        env = dict(os.environ)
        env.pop("DMC_CTX_TRAIN", None)
        if value is not None:
            env["DMC_CTX_TRAIN"] = value
        out = subprocess.run([sys.executable, "-c", code], env=env, stdout=subprocess.PIPE, check=True, universal_newlines=True).stdout
        assert out.strip().splitlines()[-1] == want, (value, out)
    if os.environ.get("DMC_CTX_TRAIN", "0") != "1":
        assert model.CTX_TRAIN is False


def _stock(net, x):
    if isinstance(net, model.ContextNetworkAtt):
        t = net.conv_context(x)
        return net.predict_flow(t), net.predict_att(t)
    return (net.conv_context(x),)


@pytest.mark.parametrize("att,ds", [(0, 0), (0, 16), (1, 0), (1, 16)])
def test_flag_on_keeps_cpu_networks_on_the_stock_modules(att, ds, monkeypatch):
    monkeypatch.setattr(model, "CTX_TRAIN", True)
    cls = model.ContextNetworkAtt if att else model.ContextNetwork
    net0 = O.seeded_state_fill(cls(5, True, ds), 3).train()
    x = rnd(1, (2, 5, 12, 9))
    r = rnd(2, (2, 2, 12, 9))
    assert not ops.context_train_supported(net0, x)               # a CPU tensor, CPU weights
    assert not ops.dilated_conv_supported(rnd(5, (2, 32, 12, 9)), net0.conv_context[1][0])

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
        ops.context_train(net0, x)


def test_dilated_conv_has_no_cpu_fallback():
    with pytest.raises(_lib.DmcHipError):
        ops.dilated_conv(rnd(1, (1, 32, 8, 8)), rnd(2, (64, 32, 3, 3)), 2)
    with pytest.raises(_lib.DmcHipError):
        ops.dilated_conv(rnd(1, (1, 32, 8, 8)).contiguous(memory_format=torch.channels_last), rnd(2, (64, 32, 3, 3)).requires_grad_(True), 1)


@pytest.mark.parametrize("att", [0, 1])
@pytest.mark.parametrize("ds,shape", [(0, (2, 5, 21, 17)), (0, (3, 5, 33, 18)), (16, (3, 5, 14, 14))], ids=["21x17", "33x18", "ds16-14x14"])
def test_whole_network_input_seeds_are_what_the_kink_criterion_returns(att, ds, shape):
    """tests/test_dconv_gpu.py draws its whole-network inputs at the first seed from 51 upwards whose fp64 stock reference keeps
    every BatchNorm output away from the LeakyReLU kink: the table there is exactly what kink_free_seed() finds on the CPU."""
    from tests import test_dconv_gpu as G
    assert G.INPUT_SEEDS[(att, ds, shape)] == G.kink_free_seed(att, ds, shape)
    assert sorted(G.INPUT_SEEDS) == sorted((a, d, s) for a in (0, 1) for d, s in ((0, (2, 5, 21, 17)), (0, (3, 5, 33, 18)), (16, (3, 5, 14, 14))))
