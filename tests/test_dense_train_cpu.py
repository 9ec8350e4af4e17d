"""CPU: the host side of the dense-estimator training route (csrc/dense_train.hip, ops.dense_train*, model.DENSE_TRAIN).

The header declares the dmc_densetrain_* entry points with the signatures _lib.SIGNATURES binds and the library exports them; the
buffer-order -> parameter-order gradient map is the exact inverse of ops._dense_weight; the data gradient's channel blocks tile
[0, K); the predicate is False wherever the route must not be taken and the forward is then the stock loop's; the flag is read
from the environment once and is off by default; the size queries and the refusals run without a GPU; the reference helpers of
tests/dense_train_ref.py agree with torch autograd."""
import ctypes
import os
import re
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as F

from dmcnet_amd import _lib, model, ops
from tests import dense_ref as D
from tests import dense_train_ref as TR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NETS = ["DenseNet", "DenseNetSmall"]
#: name -> (return type, argument kinds: p pointer, i int, s stream) as include/dmcnet_hip.h declares them
NEW = {
    "dmc_densetrain_supported": ("int", "iiiiii"),
    "dmc_densetrain_mask_workspace_bytes": ("size_t", "iiii"),
    "dmc_densetrain_wgrad_workspace_bytes": ("size_t", "iiiii"),
    "dmc_densetrain_head_workspace_bytes": ("size_t", "iiii"),
    "dmc_densetrain_head_dgrad": ("int", "pppiiiis"),
    "dmc_densetrain_head_wgrad": ("int", "pppppiiiis"),
    "dmc_densetrain_mask": ("int", "ppppiiiiiis"),
    "dmc_densetrain_layer_wgrad": ("int", "ppppiiiiiis"),
    "dmc_densetrain_layer_dgrad": ("int", "ppiiiiiiiis"),
    "dmc_densetrain_export": ("int", "ppiiiis"),
}


def test_header_library_and_signatures_have_the_entry_points():
    import __graft_entry__ as g
    g.build()
    text = open(os.path.join(ROOT, "include", "dmcnet_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    lib = ctypes.CDLL(_lib.LIB_PATH)
    kinds = {"p": _lib._P, "i": _lib._I, "s": _lib._P}
    for name, (ret, args) in NEW.items():
        m = re.search(r"\b(int|size_t)\s+%s\s*\(([^)]*)\)\s*;" % name, text)
        assert m, name + " is not declared in include/dmcnet_hip.h"
        assert m.group(1) == ret, name
        declared = ""
        for arg in m.group(2).split(","):
            arg = arg.strip()
            declared += "s" if arg.startswith("dmc_stream_t") else "p" if "*" in arg else "i" if arg.startswith("int ") else "?"
        assert declared == args, (name, declared)
        assert hasattr(lib, name), "libdmcnet_hip.so does not export " + name
        rt, at = _lib.SIGNATURES[name]
        assert rt is (_lib._Z if ret == "size_t" else _lib._I) and at == [kinds[c] for c in args], name
    assert "dense_train.hip" in __import__("dmcnet_amd.build", fromlist=["SOURCES"]).SOURCES


# ---------------------------------------------------------------- the gradient map
@pytest.mark.parametrize("name", NETS)
def test_gradient_map_is_the_exact_inverse_of_the_weight_map(name):
    lay = ops.dense_eval_layout(D.WIDTHS[name])
    ps = D.params(name)
    for li, ((w, b), (k, r, index)) in enumerate(zip(ps, lay["layers"] + [lay["head"]])):
        conv = torch.nn.Conv2d(w.shape[1], w.shape[0], 3, 1, 1)
        g = D.rnd(700 + li, tuple(w.shape))                        # a "gradient" in the module's order
        with torch.no_grad():
            conv.weight.copy_(g)
        gb, _ = ops._dense_weight(conv, k, r, index)               # ... in buffer order
        assert torch.equal(ops._dense_weight_grad(gb, w.shape[0], index).view(torch.int32), g.view(torch.int32))
        # pad rows and pad columns do not leak: poison them
        poisoned = gb.clone()
        poisoned[w.shape[0]:] = float("nan")
        poisoned[..., index < 0] = float("nan")
        back = ops._dense_weight_grad(poisoned, w.shape[0], index)
        assert tuple(back.shape) == tuple(w.shape) and back.is_contiguous()
        assert torch.equal(back.view(torch.int32), g.view(torch.int32))
        assert torch.equal(back, D.reference_weight(gb, w.shape[0], index))


def test_data_gradient_blocks_tile_the_prefix():
    for name in NETS:
        for k in D.EXPECTED[name][0]:
            blocks = ops._dense_dgrad_blocks(k)
            assert blocks[0][0] == 0 and all(c0 % 128 == 0 and cb in (32, 64, 96, 128) for c0, cb in blocks)
            assert [c0 for c0, _ in blocks] == list(range(0, k, 128))
            c0, cb = blocks[-1]
            assert c0 < k <= c0 + cb <= k + 16 and all(b == 128 for _, b in blocks[:-1])


# ---------------------------------------------------------------- the predicate, the flag, the dispatch
def _small():
    torch.manual_seed(5)
    return model.EstimatorDenseNetSmall()


def test_predicate_is_false_where_the_route_must_not_be_taken():
    x = D.rnd(1, (2, 5, 12, 9))
    net = _small()
    assert torch.is_grad_enabled()
    assert not ops.dense_train_supported(net, x)                   # a CPU tensor
    with torch.no_grad():
        assert not ops.dense_train_supported(net, x)               # autograd off
    assert not ops.dense_train_supported(model.EstimatorDenseNetTiny(), x)
    bad = _small()
    bad.conv_2[1] = torch.nn.LeakyReLU(0.2)
    assert not ops.dense_train_supported(bad, x) and ops._dense_plan(bad, on_device=False) is None
    for t in (x.double(), x[:, :4], x[0], x[:0], None):
        assert not ops.dense_train_supported(net, t)
    with pytest.raises(_lib.DmcHipError):
        ops.dense_train(net, x)


def test_flag_is_off_by_default_and_the_forward_is_the_stock_loop(monkeypatch):
    assert model.DENSE_TRAIN is False or os.environ.get("DMC_DENSE_TRAIN") == "1"
    monkeypatch.setattr(model, "DENSE_TRAIN", False)
    monkeypatch.setattr(ops, "dense_train_supported", lambda net, x: pytest.fail("the predicate is not consulted with the flag off"))
    for name in NETS:
        net = model._ESTIMATORS[name]()
        x = D.rnd(2, (1, 5, 7, 6))
        got = net(x)
        assert got.requires_grad and torch.equal(got, D.stock_forward(net, x))


def test_flag_on_consults_the_predicate_and_tiny_never_does(monkeypatch):
    asked = []
    monkeypatch.setattr(model, "DENSE_TRAIN", True)
    monkeypatch.setattr(ops, "dense_train_supported", lambda net, x: (asked.append(type(net).__name__), True)[1])
    monkeypatch.setattr(ops, "dense_train", lambda net, x: "route")
    x = torch.zeros(1, 5, 6, 6)
    assert model.EstimatorDenseNet()(x) == "route" and model.EstimatorDenseNetSmall()(x) == "route"
    assert asked == ["EstimatorDenseNet", "EstimatorDenseNetSmall"]
    assert model.EstimatorDenseNetTiny.forward is not model.DenseEstimatorBase.forward
    assert not issubclass(model._EarlyFusion, model.DenseEstimatorBase)
    monkeypatch.setattr(ops, "dense_train_supported", lambda net, x: False)      # refused: the stock loop
    net = _small()
    y = D.rnd(3, (1, 5, 6, 6))
    assert torch.equal(net(y), D.stock_forward(net, y))


def test_flag_is_read_from_the_environment_once():
    code = "import sys; sys.path.insert(0, %r); from dmcnet_amd import model; print(int(model.DENSE_TRAIN))" % ROOT
    for value, want in ((None, "0"), ("0", "0"), ("1", "1"), ("yes", "0")):
        env = dict(os.environ)
        env.pop("DMC_DENSE_TRAIN", None)
        if value is not None:
            env["DMC_DENSE_TRAIN"] = value
        out = subprocess.run([sys.executable, "-c", code], env=env, stdout=subprocess.PIPE, check=True, universal_newlines=True).stdout
        assert out.strip().splitlines()[-1] == want, (value, out)


# ---------------------------------------------------------------- the C ABI without a GPU
def test_size_and_capability_queries_without_gpu():
    lib = _lib.load()
    for name in NETS:
        ks, rs, ct = D.EXPECTED[name]
        for k, r in zip(ks, rs):
            assert lib.dmc_densetrain_supported(24, 224, 224, ct, k, r) == 1, (name, k, r)
        assert lib.dmc_densetrain_supported(24, 224, 224, ct, ct, 2) == 1
    assert lib.dmc_densetrain_supported(92, 224, 224, 464, 432, 32) == 1 and lib.dmc_densetrain_supported(93, 224, 224, 464, 432, 32) == 0
    assert lib.dmc_densetrain_supported(1, 8, 8, 560, 432, 128) == 1
    assert lib.dmc_densetrain_supported(1, 8, 8, 464, 432, 2) == 0             # the head's backward covers the whole buffer
    assert lib.dmc_densetrain_supported(1, 8, 8, 512, 512, 2) == 1 and lib.dmc_densetrain_supported(1, 8, 8, 528, 528, 2) == 0
    for bad in ((0, 8, 8, 464, 16, 128), (1, 8, 8, 462, 16, 128), (1, 8, 8, 464, 24, 128), (1, 8, 8, 464, 16, 48), (1, 8, 8, 464, 448, 32)):
        assert lib.dmc_densetrain_supported(*bad) == 0, bad
    # 3 x 33 x 18 = 1782 pixels: 56 steps of 32 pixels, one range each; 2 mask workgroups
    assert lib.dmc_densetrain_wgrad_workspace_bytes(3, 33, 18, 432, 32) == 56 * 32 * 9 * 432 * 4
    assert lib.dmc_densetrain_head_workspace_bytes(3, 33, 18, 464) == 56 * (18 * 464 + 2) * 4
    assert lib.dmc_densetrain_mask_workspace_bytes(3, 33, 18, 96) == 2 * 96 * 4
    # 11 x 224 x 224: 17248 steps, 270 a range without the cap, 256 with it: 68 ranges
    assert lib.dmc_densetrain_wgrad_workspace_bytes(11, 224, 224, 16, 32) == 68 * 32 * 9 * 16 * 4
    # the largest workspace of a 92-frame range of EstimatorDenseNet (564 ranges): layer 2
    sizes = [lib.dmc_densetrain_wgrad_workspace_bytes(92, 224, 224, k, r) for k, r in zip(*D.EXPECTED["DenseNet"][:2])]
    assert max(sizes) == sizes[2] == 564 * 96 * 9 * 272 * 4
    assert lib.dmc_densetrain_wgrad_workspace_bytes(1, 8, 8, 24, 32) == 0 and lib.dmc_densetrain_wgrad_workspace_bytes(1, 8, 8, 16, 48) == 0
    assert lib.dmc_densetrain_mask_workspace_bytes(1, 8, 8, 2) == 0 and lib.dmc_densetrain_head_workspace_bytes(1, 8, 8, 528) == 0
    assert lib.dmc_densetrain_head_workspace_bytes(0, 8, 8, 464) == 0


def test_refusals_are_loud_and_launch_nothing():
    lib = _lib.load()
    p = _lib.ptr(torch.zeros(16))                                 # any non-null pointer: nothing is launched

    def refused(name, rc):
        assert rc == -1, name
        assert name.encode() in lib.dmc_last_error(), (name, lib.dmc_last_error())

    shape = (1, 8, 8, 464)
    for i in range(3):
        a = [p] * 3
        a[i] = None
        refused("dmc_densetrain_head_dgrad", lib.dmc_densetrain_head_dgrad(*a, *shape, None))
    for i in range(5):
        a = [p] * 5
        a[i] = None
        refused("dmc_densetrain_head_wgrad", lib.dmc_densetrain_head_wgrad(*a, *shape, None))
    for i in range(4):
        a = [p] * 4
        a[i] = None
        refused("dmc_densetrain_mask", lib.dmc_densetrain_mask(*a, *shape, 432, 32, None))
        refused("dmc_densetrain_layer_wgrad", lib.dmc_densetrain_layer_wgrad(*a, *shape, 432, 32, None))
    for i in range(2):
        a = [p] * 2
        a[i] = None
        refused("dmc_densetrain_layer_dgrad", lib.dmc_densetrain_layer_dgrad(*a, *shape, 432, 32, 0, 128, None))
        refused("dmc_densetrain_export", lib.dmc_densetrain_export(*a, *shape, None))
    for k, r in ((24, 32), (16, 48), (448, 32), (464, 2)):
        refused("dmc_densetrain_mask", lib.dmc_densetrain_mask(p, p, p, p, *shape, k, r, None))
        refused("dmc_densetrain_layer_wgrad", lib.dmc_densetrain_layer_wgrad(p, p, p, p, *shape, k, r, None))
        refused("dmc_densetrain_layer_dgrad", lib.dmc_densetrain_layer_dgrad(p, p, *shape, k, r, 0, 32, None))
        assert b"unsupported shape" in lib.dmc_last_error()
    for c0, cb in ((0, 48), (8, 32), (432, 32), (-16, 32), (384, 96), (384, 128)):       # K = 432: the last block is (384, 64)
        refused("dmc_densetrain_layer_dgrad", lib.dmc_densetrain_layer_dgrad(p, p, *shape, 432, 32, c0, cb, None))
    assert lib.dmc_densetrain_supported(1, 8, 8, 464, 432, 32) == 1
    for ct in (528, 462):
        refused("dmc_densetrain_head_dgrad", lib.dmc_densetrain_head_dgrad(p, p, p, 1, 8, 8, ct, None))
        refused("dmc_densetrain_head_wgrad", lib.dmc_densetrain_head_wgrad(p, p, p, p, p, 1, 8, 8, ct, None))
    refused("dmc_densetrain_export", lib.dmc_densetrain_export(p, p, 93, 224, 224, 464, None))


# ---------------------------------------------------------------- the reference helpers against torch autograd
@pytest.mark.parametrize("shape", [(2, 5, 7, 16, 32), (1, 1, 4, 48, 8), (1, 3, 1, 5, 3)], ids=["2-5-7", "1-1-4", "1-3-1"])
def test_reference_helpers_agree_with_autograd(shape):
    n, h, w, k, r = shape
    x = D.rnd(11, (n, k, h, w)).double().requires_grad_(True)
    wt = D.rnd(12, (r, k, 3, 3)).double().requires_grad_(True)
    dz = D.rnd(13, (n, r, h, w)).double()
    (F.conv2d(x, wt, None, 1, 1) * dz).sum().backward()
    dzb, xb, wb = dz.permute(0, 2, 3, 1), x.detach().permute(0, 2, 3, 1), wt.detach().permute(0, 2, 3, 1)
    assert torch.allclose(TR.dgrad(dzb, wb), x.grad.permute(0, 2, 3, 1), rtol=0, atol=1e-12)
    assert torch.allclose(TR.wgrad(dzb, xb), wt.grad.permute(0, 2, 3, 1), rtol=0, atol=1e-12)
