"""CPU: the host side of the early-fusion estimators' route (csrc/early_fusion.hip, ops.early_fusion_*, model.EF_EVAL / EF_TRAIN).

The layout is what DESIGN.md 4.28 documents; the fp64 restatement of tests/ef_ref.py is the stock module's forward and autograd's
gradients; the header declares the dmc_ef_* entry points with the signatures _lib.SIGNATURES binds and the library exports them;
the queries and the refusals run without a GPU; the seeded inputs of the GPU tests exercise both LeakyReLU branches everywhere;
the predicates are False wherever the route must not be taken, and the flags are read once and leave the stock loop alone."""
import ctypes
import os
import re

import pytest
import torch

from dmcnet_amd import _lib, model, ops
from tests import ef_ref as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
#: name -> (return type, argument kinds: p pointer, i int, s stream) as include/dmcnet_hip.h declares them
NEW = {
    "dmc_ef_supported": ("int", "iiiiii"),
    "dmc_ef_head_wgrad_workspace_bytes": ("size_t", "iiii"),
    "dmc_ef_layer_wgrad_workspace_bytes": ("size_t", "iiiii"),
    "dmc_ef_layer_mask_workspace_bytes": ("size_t", "iiii"),
    "dmc_ef_first_bwd_workspace_bytes": ("size_t", "iii"),
    "dmc_ef_first": ("int", "pppppppiiiiis"),
    "dmc_ef_layer": ("int", "pppiiiiiis"),
    "dmc_ef_head": ("int", "ppppiiiiis"),
    "dmc_ef_head_dgrad": ("int", "pppiiiiis"),
    "dmc_ef_head_wgrad": ("int", "pppppiiiiis"),
    "dmc_ef_layer_mask": ("int", "ppppiiiiiis"),
    "dmc_ef_layer_wgrad": ("int", "ppppiiiiiis"),
    "dmc_ef_layer_dgrad": ("int", "ppiiiiiis"),
    "dmc_ef_first_bwd": ("int", "pppppppppiiiiis"),
}
#: DESIGN.md 4.28: per net the (K, R) of conv_1 .. conv_4, the head's K and CT
EXPECTED = {"Sum": (((8, 8), (16, 6), (24, 4), (28, 2)), 32, 32), "Stack": (((16, 8), (24, 6), (32, 4), (36, 2)), 40, 40)}
SLOTS = {"Sum": {"s": (0, 8), "y1": (8, 8), "y2": (16, 6), "y3": (24, 4), "y4": (28, 2)},
         "Stack": {"m": (0, 8), "r": (8, 8), "y1": (16, 8), "y2": (24, 6), "y3": (32, 4), "y4": (36, 2)}}


# ---------------------------------------------------------------- the layout
@pytest.mark.parametrize("name", E.NETS)
def test_layout_invariants(name):
    lay = E.layout(name)
    layers, hk, ct = EXPECTED[name]
    assert lay["ct"] == ct and lay["offsets"] == SLOTS[name]
    assert [(k, r) for k, r, _ in lay["layers"]] == list(layers) and lay["head"][:2] == (hk, 2)
    spans = sorted((first, first + (live + 3) // 4 * 4) for first, live in lay["offsets"].values())
    assert spans[0][0] == 0 and spans[-1][1] == ct
    assert all(a % 4 == 0 and b % 4 == 0 for a, b in spans)                      # 4-aligned
    assert all(spans[i][1] == spans[i + 1][0] for i in range(len(spans) - 1))    # disjoint, and they tile [0, CT)
    base = 16 if name == "Stack" else 8
    cin = base
    for (k, r, index), width in zip(lay["layers"] + [lay["head"]], (8, 6, 4, 2, 2)):
        assert index.dtype == torch.int64 and tuple(index.shape) == (k,) and k % 4 == 0
        live = index[index >= 0]
        assert sorted(live.tolist()) == list(range(cin))                         # every reference input channel exactly once
        pads = set((index < 0).nonzero().reshape(-1).tolist())
        want_pads = {c for first, n in lay["offsets"].values() for c in range(first + n, first + (n + 3) // 4 * 4) if c < k}
        assert pads == want_pads
        assert index[:base].tolist() == list(range(cin - base, cin))             # the base comes last in the reference's order
        cin += width
    y1 = lay["offsets"]["y1"][0]
    assert lay["layers"][1][2][y1:y1 + 8].tolist() == list(range(0, 8))          # conv_2's input starts with y_1
    assert ops.early_fusion_layout(name == "Stack")["layers"][0][2] is not lay["layers"][0][2]       # a pure function: fresh objects


# ---------------------------------------------------------------- the restatement
@pytest.mark.parametrize("name", E.NETS)
def test_restatement_is_the_stock_module_in_fp64(name):
    m = E.net(name, dtype=torch.float64)
    x = E.rnd(31, (2, 5, 9, 11)).double()
    r = E.rnd(32, (2, 2, 9, 11)).double()
    assert list(dict(m.named_parameters())) == E.PARAM_NAMES
    got = m(x)
    assert got.requires_grad and torch.equal(got, E.stock_forward(m, x))
    want, grads = E.gradients(name, x, r, torch.float64)
    assert torch.equal(got.detach(), want)
    auto = torch.autograd.grad((got * r).sum(), list(m.parameters()))
    for pname, g, a in zip(E.PARAM_NAMES, grads, auto):
        assert g.shape == a.shape and torch.equal(g, a), pname
    with torch.no_grad():
        assert torch.equal(E.forward(E.params(name, torch.float64), x, name == "Stack")["out"], want)
        o = __import__("oracle.dmc_oracle", fromlist=["x"])
        ref = o.seeded_state_fill(o.build_estimator(E.ARCH[name]), seed=E.SEED).double()
        assert torch.equal(ref(x), want)                                         # ... and the oracle's module


# ---------------------------------------------------------------- the ABI
def test_header_library_and_signatures_have_the_entry_points():
    import __graft_entry__ as g
    g.build()
    text = open(os.path.join(ROOT, "include", "dmcnet_hip.h")).read()
    comments = " ".join(re.findall(r"/\*.*?\*/", text, flags=re.S))
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
    assert sorted(n for n in _lib.SIGNATURES if n.startswith("dmc_ef_")) == sorted(NEW)
    assert re.search(r"code/dmcnet/model\.py:197-250", comments)
    build = __import__("dmcnet_amd.build", fromlist=["SOURCES"])
    assert "early_fusion.hip" in build.SOURCES
    assert "dmc-net_amd/csrc/early_fusion.hip" in build.read_manifest()["sources"]


def test_supported_and_size_queries_return_what_the_header_says():
    lib = _lib.load()
    for name in E.NETS:
        layers, hk, ct = EXPECTED[name]
        for k, r in layers:
            assert lib.dmc_ef_supported(3, 33, 18, ct, k, r) == 1
        assert lib.dmc_ef_supported(3, 33, 18, ct, hk, 2) == 1                   # the head: K == CT
    ok = (2, 7, 9, 40, 16, 8)
    assert lib.dmc_ef_supported(*ok) == 1
    for i, bad in ((0, 0), (1, 0), (2, -1), (3, 0), (3, 38), (3, 68), (4, 0), (4, 18), (5, 1), (5, 3), (5, 5), (5, 7), (5, 10), (5, 0)):
        args = list(ok)
        args[i] = bad
        assert lib.dmc_ef_supported(*args) == 0, args
    assert lib.dmc_ef_supported(2, 7, 9, 40, 36, 8) == 0 and lib.dmc_ef_supported(2, 7, 9, 40, 36, 6) == 0       # K + round_up4(R) > CT
    assert lib.dmc_ef_supported(2, 7, 9, 40, 36, 4) == 1 and lib.dmc_ef_supported(2, 7, 9, 40, 36, 2) == 1
    assert lib.dmc_ef_supported(2, 7, 9, 40, 40, 2) == 1 and lib.dmc_ef_supported(2, 7, 9, 40, 40, 4) == 0       # only the head may have K == CT
    assert lib.dmc_ef_supported(2, 7, 9, 64, 60, 4) == 1 and lib.dmc_ef_supported(2, 7, 9, 40, 44, 2) == 0
    assert lib.dmc_ef_supported(540, 224, 224, 40, 16, 8) == 1                   # 1.08e9 elements, 4.3 GB
    assert lib.dmc_ef_supported(1070, 224, 224, 40, 16, 8) == 0                  # 2^31 elements or more
    parts = lambda n, h, w: (n * h * w + 1023) // 1024
    for n, h, w in ((1, 1, 1), (3, 33, 18), (2, 224, 224), (1, 32, 32)):
        p = parts(n, h, w)
        assert lib.dmc_ef_head_wgrad_workspace_bytes(n, h, w, 40) == p * (18 * 40 + 2) * 4
        assert lib.dmc_ef_layer_wgrad_workspace_bytes(n, h, w, 24, 6) == p * 6 * 9 * 24 * 4
        assert lib.dmc_ef_layer_mask_workspace_bytes(n, h, w, 6) == p * 8 * 4
        assert lib.dmc_ef_layer_mask_workspace_bytes(n, h, w, 2) == p * 4 * 4
        assert lib.dmc_ef_first_bwd_workspace_bytes(n, h, w) == p * 376 * 4
    assert lib.dmc_ef_head_wgrad_workspace_bytes(0, 4, 4, 40) == 0 and lib.dmc_ef_head_wgrad_workspace_bytes(1, 4, 4, 42) == 0
    assert lib.dmc_ef_layer_wgrad_workspace_bytes(1, 4, 4, 24, 5) == 0 and lib.dmc_ef_layer_wgrad_workspace_bytes(1, 4, 4, 68, 4) == 0
    assert lib.dmc_ef_layer_mask_workspace_bytes(1, 4, 4, 3) == 0 and lib.dmc_ef_first_bwd_workspace_bytes(1, 0, 4) == 0


def test_refused_calls_return_invalid_before_any_launch():
    """(No GPU here: a call that got as far as a launch would not return DMC_E_INVALID.)"""
    lib = _lib.load()
    host = torch.zeros(64)
    p, z, s = _lib.ptr(host), _lib._P(0), _lib._P(0)
    calls = [("dmc_ef_first", lambda: lib.dmc_ef_first(p, p, p, p, p, p, z, 1, 4, 4, 12, 1, s)),              # Stack needs CT >= 16
             ("dmc_ef_first", lambda: lib.dmc_ef_first(p, p, p, p, p, p, z, 1, 4, 4, 4, 0, s)),
             ("dmc_ef_first", lambda: lib.dmc_ef_first(p, p, p, p, p, p, z, 1, 4, 4, 40, 2, s)),
             ("dmc_ef_first", lambda: lib.dmc_ef_first(p, p, z, p, p, p, z, 1, 4, 4, 40, 1, s)),
             ("dmc_ef_layer", lambda: lib.dmc_ef_layer(p, p, p, 1, 4, 4, 40, 36, 8, s)),
             ("dmc_ef_layer", lambda: lib.dmc_ef_layer(p, p, p, 1, 4, 4, 40, 40, 2, s)),                      # the head's shape
             ("dmc_ef_layer", lambda: lib.dmc_ef_layer(p, p, p, 1, 4, 4, 40, 16, 5, s)),
             ("dmc_ef_layer", lambda: lib.dmc_ef_layer(p, z, p, 1, 4, 4, 40, 16, 8, s)),
             ("dmc_ef_head", lambda: lib.dmc_ef_head(p, p, p, p, 1, 4, 4, 40, 44, s)),
             ("dmc_ef_head", lambda: lib.dmc_ef_head(p, p, p, z, 1, 4, 4, 40, 40, s)),
             ("dmc_ef_head_dgrad", lambda: lib.dmc_ef_head_dgrad(p, p, p, 1, 4, 4, 72, 40, s)),
             ("dmc_ef_head_wgrad", lambda: lib.dmc_ef_head_wgrad(p, p, p, p, z, 1, 4, 4, 40, 40, s)),
             ("dmc_ef_layer_mask", lambda: lib.dmc_ef_layer_mask(p, p, p, p, 1, 4, 4, 40, 38, 2, s)),
             ("dmc_ef_layer_wgrad", lambda: lib.dmc_ef_layer_wgrad(p, p, p, p, 1, 4, 4, 40, 36, 6, s)),
             ("dmc_ef_layer_dgrad", lambda: lib.dmc_ef_layer_dgrad(p, p, 0, 4, 4, 40, 16, 8, s)),
             ("dmc_ef_first_bwd", lambda: lib.dmc_ef_first_bwd(p, p, z, p, p, p, p, p, p, 1, 4, 4, 32, 0, s)),    # Sum needs the sign plane
             ("dmc_ef_first_bwd", lambda: lib.dmc_ef_first_bwd(p, p, p, z, p, p, p, p, p, 1, 4, 4, 40, 1, s)),    # Stack needs feat
             ("dmc_ef_first_bwd", lambda: lib.dmc_ef_first_bwd(p, p, p, p, p, p, p, p, p, 1, 4, 4, 12, 1, s))]
    for name, call in calls:
        assert call() == -1, name
        assert name.encode() in lib.dmc_last_error(), name
    assert not host.any()


# ---------------------------------------------------------------- what the seeded inputs exercise
@pytest.mark.parametrize("shape", E.MAIN_SHAPES + E.DEGENERATE_SHAPES, ids=E.sid)
@pytest.mark.parametrize("name", E.NETS)
def test_seeded_inputs_reach_every_sign_combination_of_the_two_first_convolutions(name, shape):
    _, f, _ = E.reference(name, shape)
    a, b = f["a"] > 0, f["b"] > 0
    shares = [float((a == sa).logical_and(b == sb).double().mean()) for sa in (False, True) for sb in (False, True)]
    print("ef signs %s %s: %s" % (name, shape, " ".join("%.3f" % s for s in shares)))
    assert min(shares) >= 0.15, shares


@pytest.mark.parametrize("shape", E.MAIN_SHAPES, ids=E.sid)
@pytest.mark.parametrize("name", E.NETS)
def test_seeded_inputs_use_both_branches_of_every_hidden_layer(name, shape):
    _, f, _ = E.reference(name, shape)
    shares = [float((p <= 0).double().mean()) for p in f["pre"]]
    print("ef non-positive %s %s: %s" % (name, shape, " ".join("%.3f" % s for s in shares)))
    assert len(shares) == 4 and all(0.15 <= s <= 0.85 for s in shares), shares


# ---------------------------------------------------------------- the predicates, the flags, the dispatch
def test_predicates_are_false_where_the_route_must_not_be_taken():
    x = E.rnd(1, (2, 5, 12, 9))
    for name in E.NETS:
        m = E.net(name)
        assert ops._ef_plan(m, on_device=False) is not None and ops._ef_plan(m) is None          # structure fine, parameters on the CPU
        assert not ops.early_fusion_train_supported(m, x)
        with torch.no_grad():
            assert not ops.early_fusion_supported(m, x)
            for t in (x.double(), x[:, :4], x[0], x[:0], None):
                assert not ops.early_fusion_supported(m, t)
        with pytest.raises(_lib.DmcHipError):
            ops.early_fusion_eval(m, x)
        with pytest.raises(_lib.DmcHipError):
            ops.early_fusion_train(m, x)
    for what in ("slope", "bias", "width", "dense", "forward"):
        m = E.net("Sum")
        if what == "slope":
            m.conv_2[1] = torch.nn.LeakyReLU(0.2)
        elif what == "bias":
            m.conv_3[0] = torch.nn.Conv2d(22, 4, 3, 1, 1, bias=False)
        elif what == "width":
            m.conv_0_r[0] = torch.nn.Conv2d(3, 8, 5, 1, 2)
        elif what == "dense":
            m = model.EstimatorDenseNetSmall()
        else:
            m = type("Other", (model.EstimatorDenseNetTinyEarlyFusionSum,), {"forward": lambda self, t: t})()
        assert ops._ef_plan(m, on_device=False) is None, what


def test_flags_are_read_once_and_leave_the_stock_loop_alone(monkeypatch):
    assert model.EF_TRAIN is False or os.environ.get("DMC_EF_TRAIN") == "1"
    assert model.EF_EVAL is True or os.environ.get("DMC_EF_EVAL") == "0"
    assert model.EF_EVAL_ALL is (os.environ.get("DMC_EF_EVAL") == "1")
    x = E.rnd(2, (1, 5, 7, 6))
    monkeypatch.setattr(model, "EF_TRAIN", False)
    monkeypatch.setattr(ops, "early_fusion_train_supported", lambda net, t: pytest.fail("the predicate is not consulted with the flag off"))
    for name in E.NETS:
        m = E.net(name)
        got = m(x)
        assert got.requires_grad and torch.equal(got, E.stock_forward(m, x))
    asked = []
    monkeypatch.setattr(model, "EF_TRAIN", True)
    monkeypatch.setattr(model, "EF_EVAL", True)
    monkeypatch.setattr(model, "EF_EVAL_ALL", True)
    monkeypatch.setattr(ops, "early_fusion_train_supported", lambda net, t: (asked.append("train"), torch.is_grad_enabled())[1])
    monkeypatch.setattr(ops, "early_fusion_supported", lambda net, t: (asked.append("eval"), not torch.is_grad_enabled())[1])
    monkeypatch.setattr(ops, "early_fusion_train", lambda net, t: "train route")
    monkeypatch.setattr(ops, "early_fusion_eval", lambda net, t: "eval route")
    m = E.net("Stack")
    assert m(x) == "train route" and asked == ["eval", "train"]
    with torch.no_grad():
        assert m(x) == "eval route"
    monkeypatch.setattr(model, "EF_EVAL", False)                                  # DMC_EF_EVAL=0: the stock modules
    with torch.no_grad():
        assert torch.equal(m(x), E.stock_forward(m, x))
    monkeypatch.setattr(model, "EF_EVAL", True)
    monkeypatch.setattr(model, "EF_EVAL_ALL", False)                              # unset: by class
    del asked[:]
    with torch.no_grad():
        for name in E.NETS:
            m = E.net(name)
            assert (m(x) == "eval route") if m.EF_EVAL_BY_DEFAULT else torch.equal(m(x), E.stock_forward(m, x))
