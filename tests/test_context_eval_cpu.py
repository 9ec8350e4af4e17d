"""CPU: the host side of the ContextNetwork eval route (csrc/ctx_eval.hip, ops.context_eval*, model.CTX_EVAL).

The header declares the dmc_ctx_* entry points, the library exports them and _lib.SIGNATURES binds them; the dispatch predicate
is False wherever the route must not be taken (and the forward is then the stock Sequential's, bit for bit); the frame ranges of
the launches tile the batch and stay indexable; every entry point refuses null pointers and unsupported shapes before any launch
with its name in dmc_last_error(); the size queries run without a GPU."""
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
NEW = ["dmc_ctx_first_eval", "dmc_ctx_heads_eval", "dmc_ctx_pack_weights", "dmc_ctx_unit_eval", "dmc_ctx_unit_supported",
       "dmc_ctx_wpack_bytes"]


def rnd(seed, shape):
    return torch.from_numpy(np.random.RandomState(seed).standard_normal(shape).astype(np.float32))


def test_header_library_and_signatures_have_the_entry_points():
    import __graft_entry__ as g
    g.build()
    text = open(os.path.join(ROOT, "include", "dmcnet_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(dmc_[a-z0-9_]+)\s*\(", text))
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW:
        assert name in declared, name + " is not declared in include/dmcnet_hip.h"
        assert hasattr(lib, name), "libdmcnet_hip.so does not export " + name
        assert name in _lib.SIGNATURES, name
    assert _lib.SIGNATURES["dmc_ctx_unit_supported"] == (ctypes.c_int, [ctypes.c_int] * 6)
    assert _lib.SIGNATURES["dmc_ctx_wpack_bytes"] == (ctypes.c_size_t, [ctypes.c_int] * 2)
    assert len(_lib.SIGNATURES["dmc_ctx_unit_eval"][1]) == 13 and len(_lib.SIGNATURES["dmc_ctx_first_eval"][1]) == 10
    assert len(_lib.SIGNATURES["dmc_ctx_heads_eval"][1]) == 15 and len(_lib.SIGNATURES["dmc_ctx_pack_weights"][1]) == 5
    assert sorted(n for n in declared if n.startswith("dmc_ctx_")) == NEW


def _stock(net, x):
    if isinstance(net, model.ContextNetworkAtt):
        t = net.conv_context(x)
        return net.predict_flow(t), net.predict_att(t)
    return (net.conv_context(x),)


def _same_as_stock(net, x):
    got = net(x)
    got = got if isinstance(got, tuple) else (got,)
    want = _stock(net, x)
    assert len(got) == len(want)
    for a, b in zip(got, want):
        assert torch.equal(a, b)


@pytest.mark.parametrize("att,ds", [(0, 0), (0, 16), (1, 0), (1, 16)])
def test_unsupported_cases_take_the_stock_forward(att, ds):
    cls = model.ContextNetworkAtt if att else model.ContextNetwork
    x = rnd(1, (2, 5, 12, 9))
    net = O.seeded_state_fill(cls(5, True, ds), 3).eval()
    assert sorted(net.state_dict()) == sorted(O.build_estimator("ContextNetwork", ds, att).state_dict())
    with torch.no_grad():                                          # a CPU tensor
        assert not ops.context_eval_supported(net, x)
        _same_as_stock(net, x)
    assert not ops.context_eval_supported(net, x)                  # grad enabled
    _same_as_stock(net, x)
    net.train()                                                    # BatchNorms in training mode (fresh copies: train() updates statistics)
    with torch.no_grad():
        assert not ops.context_eval_supported(net, x)
    net.eval()
    net.conv_context[2][1].train()                                 # one BatchNorm in training mode
    with torch.no_grad():
        assert not ops.context_eval_supported(net, x)
    net.eval()
    plain = O.seeded_state_fill(cls(5, False, ds), 4).eval()       # batch_norm=False
    with torch.no_grad():
        assert not ops.context_eval_supported(plain, x)
        _same_as_stock(plain, x)
    conv = net.conv_context[3][0]                                  # a convolution that has been given a bias
    conv.bias = torch.nn.Parameter(torch.full((conv.out_channels,), 0.25))
    with torch.no_grad():
        assert not ops.context_eval_supported(net, x)
        _same_as_stock(net, x)
    with pytest.raises(_lib.DmcHipError):
        with torch.no_grad():
            ops.context_eval(net, x)


def test_predicate_looks_at_every_property_it_promises():
    """Without a GPU the predicate is False at its first test (a CPU tensor); the structural part (_ctx_plan) is checked on its own."""
    net = model.ContextNetwork(5).eval()
    assert ops._ctx_plan(net) is None                              # CPU parameters: not served
    assert ops._ctx_unit_parts(torch.nn.Sequential(torch.nn.Conv2d(32, 32, 3, 1, 1), torch.nn.LeakyReLU(0.1))) is None
    with torch.no_grad():
        for bad in (torch.zeros(2, 5, 8, 8, dtype=torch.float64), torch.zeros(2, 4, 8, 8), torch.zeros(5, 8, 8), None):
            assert not ops.context_eval_supported(net, bad)


def test_chunks_tile_the_batch_and_stay_indexable():
    assert ops.context_eval_chunks(25, 224, 224) == [(0, 25)]
    for n, h, w in ((250, 224, 224), (1, 224, 224), (334, 224, 224), (335, 224, 224), (7, 1024, 1024), (3, 33, 18), (1000, 56, 448)):
        ch = ops.context_eval_chunks(n, h, w)
        assert ch[0][0] == 0 and ch[-1][1] == n
        for (a, b), (c, _) in zip(ch, ch[1:] + [(n, n)]):
            assert a < b and b == c
            assert (b - a) * h * w * 128 < 2 ** 31
    assert len(ops.context_eval_chunks(250, 224, 224)) == 1 and len(ops.context_eval_chunks(335, 224, 224)) == 2
    assert ops.context_eval_chunks(3, 4096, 4095) == [(0, 1), (1, 2), (2, 3)]
    for bad in ((0, 8, 8), (2, 0, 8), (1, 4096, 4097)):
        with pytest.raises(ValueError):
            ops.context_eval_chunks(*bad)


def test_size_and_capability_queries_without_gpu():
    lib = _lib.load()
    for cin, cout, d in ((32, 128, 2), (128, 128, 4), (128, 96, 8), (96, 64, 16), (96, 64, 1), (64, 32, 1), (5, 32, 1), (32, 2, 1)):
        assert lib.dmc_ctx_unit_supported(25, 224, 224, cin, cout, d) == 1, (cin, cout, d)
        assert lib.dmc_ctx_unit_supported(250, 224, 224, cin, cout, d) == 1
        assert lib.dmc_ctx_unit_supported(335, 224, 224, cin, cout, d) == 0           # 335 * 224^2 * 128 >= 2^31
    for n, h, w, cin, cout, d in ((0, 8, 8, 32, 128, 2), (1, 0, 8, 32, 128, 2), (1, 8, -1, 32, 128, 2), (1, 8, 8, 32, 128, 3), (1, 8, 8, 48, 64, 1),
                                  (1, 8, 8, 64, 48, 1), (1, 8, 8, 5, 32, 2), (1, 8, 8, 32, 2, 2), (1, 8, 8, 5, 64, 1), (1, 8, 8, 64, 2, 1),
                                  (1, 8, 8, 256, 128, 1), (1, 8, 8, 128, 128, 32), (1, 8, 8, 128, 128, 0)):
        assert lib.dmc_ctx_unit_supported(n, h, w, cin, cout, d) == 0, (n, h, w, cin, cout, d)
    for cin, cout in ((32, 128), (128, 128), (128, 96), (96, 64), (64, 32)):
        assert lib.dmc_ctx_wpack_bytes(cin, cout) == cin * cout * 9 * 3 * 2
    assert lib.dmc_ctx_wpack_bytes(5, 32) == 0 and lib.dmc_ctx_wpack_bytes(32, 2) == 0


def test_refusals_are_loud_and_launch_nothing():
    lib = _lib.load()
    p = _lib.ptr(torch.zeros(16))                                 # any non-null pointer: nothing is launched

    def refused(name, rc):
        assert rc == -1, name
        assert name.encode() in lib.dmc_last_error(), (name, lib.dmc_last_error())

    for i in range(6):                                            # every pointer of dmc_ctx_unit_eval / dmc_ctx_first_eval
        a = [p] * 6
        a[i] = None
        refused("dmc_ctx_unit_eval", lib.dmc_ctx_unit_eval(*a, 1, 8, 8, 32, 128, 2, None))
        refused("dmc_ctx_first_eval", lib.dmc_ctx_first_eval(*a, 1, 8, 8, None))
    for shape in ((1, 8, 8, 32, 128, 3), (1, 8, 8, 48, 64, 1), (1, 8, 8, 64, 80, 1), (0, 8, 8, 32, 128, 2), (335, 224, 224, 128, 128, 4),
                  (1, 8, 8, 5, 32, 1), (1, 8, 8, 32, 2, 1)):      # (the first unit and the heads have entry points of their own)
        refused("dmc_ctx_unit_eval", lib.dmc_ctx_unit_eval(p, p, p, p, p, p, *shape, None))
        assert b"unsupported shape" in lib.dmc_last_error()
    for n, h, w in ((0, 8, 8), (1, -2, 8), (335, 224, 224)):
        refused("dmc_ctx_first_eval", lib.dmc_ctx_first_eval(p, p, p, p, p, p, n, h, w, None))
        refused("dmc_ctx_heads_eval", lib.dmc_ctx_heads_eval(p, p, p, p, p, None, None, None, None, p, None, n, h, w, None))
        refused("dmc_ctx_heads_eval", lib.dmc_ctx_heads_eval(p, p, p, p, p, p, p, p, p, p, p, n, h, w, None))
    for i in (0, 1, 2, 3, 4, 9):                                   # the flow head's pointers
        a = [p] * 11
        a[i] = None
        refused("dmc_ctx_heads_eval", lib.dmc_ctx_heads_eval(*a, 1, 8, 8, None))
    for i in (6, 7, 8, 10):                                        # an incomplete attention group
        a = [p] * 11
        a[i] = None
        refused("dmc_ctx_heads_eval", lib.dmc_ctx_heads_eval(*a, 1, 8, 8, None))
    refused("dmc_ctx_heads_eval", lib.dmc_ctx_heads_eval(p, p, p, p, p, None, None, None, None, p, p, 1, 8, 8, None))   # att without w_att
    refused("dmc_ctx_pack_weights", lib.dmc_ctx_pack_weights(None, p, 32, 128, None))
    refused("dmc_ctx_pack_weights", lib.dmc_ctx_pack_weights(p, None, 32, 128, None))
    refused("dmc_ctx_pack_weights", lib.dmc_ctx_pack_weights(p, p, 5, 32, None))
    refused("dmc_ctx_pack_weights", lib.dmc_ctx_pack_weights(p, p, 32, 100, None))


def test_flag_is_read_from_the_environment_once():
    code = "import sys; sys.path.insert(0, %r); from dmcnet_amd import model; print(int(model.CTX_EVAL))" % ROOT
    for value, want in ((None, "1"), ("0", "0"), ("1", "1")):
        env = dict(os.environ)
        env.pop("DMC_CTX_EVAL", None)
        if value is not None:
            env["DMC_CTX_EVAL"] = value
        out = subprocess.run([sys.executable, "-c", code], env=env, stdout=subprocess.PIPE, check=True, universal_newlines=True).stdout
        assert out.strip().splitlines()[-1] == want, (value, out)
