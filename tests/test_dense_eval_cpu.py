"""CPU: the host side of the dense-estimator eval route (csrc/dense_eval.hip, ops.dense_eval*, model.DENSE_EVAL).

The header declares the dmc_dense_* entry points, the library exports them and _lib.SIGNATURES binds them; the layout of the
feature buffer is the documented one and its channel maps are permutations of the reference's input channels; the frame ranges
tile the batch, stay indexable and within the byte budget; the dispatch predicate is False wherever the route must not be taken
(and the forward is then the stock loop's, bit for bit); every entry point refuses null pointers and unsupported shapes before
any launch with its name in dmc_last_error(); the size queries run without a GPU."""
import copy
import ctypes
import os
import re
import subprocess
import sys

import pytest
import torch

from dmcnet_amd import _lib, model, ops
from tests import dense_ref as D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["dmc_dense_head_eval", "dmc_dense_ingest", "dmc_dense_layer_eval", "dmc_dense_pack_weights", "dmc_dense_supported",
       "dmc_dense_wpack_bytes"]
NETS = ["DenseNet", "DenseNetSmall"]


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
    assert _lib.SIGNATURES["dmc_dense_supported"] == (ctypes.c_int, [ctypes.c_int] * 6)
    assert _lib.SIGNATURES["dmc_dense_wpack_bytes"] == (ctypes.c_size_t, [ctypes.c_int] * 2)
    assert len(_lib.SIGNATURES["dmc_dense_pack_weights"][1]) == 5 and len(_lib.SIGNATURES["dmc_dense_ingest"][1]) == 7
    assert len(_lib.SIGNATURES["dmc_dense_layer_eval"][1]) == 10 and len(_lib.SIGNATURES["dmc_dense_head_eval"][1]) == 10
    assert sorted(n for n in declared if n.startswith("dmc_dense_")) == NEW


# ---------------------------------------------------------------- the layout
@pytest.mark.parametrize("name", NETS)
def test_layout_is_the_documented_one(name):
    widths = D.WIDTHS[name]
    ks, rs, ct = D.EXPECTED[name]
    lay = ops.dense_eval_layout(widths)
    assert lay["ct"] == ct
    assert tuple(k for k, _, _ in lay["layers"]) == ks and tuple(r for _, r, _ in lay["layers"]) == rs
    assert lay["head"][0] == ct and lay["head"][1] == 2
    assert tuple(lay["offsets"]) == (0,) + ks                     # slot k + 1 starts where layer k's prefix ends
    for k, (kk, r, index) in enumerate(lay["layers"] + [lay["head"]]):
        cin = 5 + sum(widths[:k])
        assert index.dtype == torch.int64 and tuple(index.shape) == (kk,)
        live = index[index >= 0]
        assert sorted(live.tolist()) == list(range(cin))          # every reference channel exactly once
        assert int((index < 0).sum()) == kk - cin                 # ... and every other buffer channel is a pad
        # slot 0 holds x, which is LAST in the reference's order; slot j + 1 holds y_j
        assert index[:5].tolist() == list(range(cin - 5, cin)) and bool((index[5:16] == -1).all())
        for j in range(k):
            o = lay["offsets"][j + 1]
            first = sum(widths[j + 1:k])
            assert index[o:o + widths[j]].tolist() == list(range(first, first + widths[j]))
            assert bool((index[o + widths[j]:o + (widths[j] + 31) // 32 * 32] == -1).all())
    assert ops.dense_eval_layout(widths) is not lay and torch.equal(ops.dense_eval_layout(widths)["head"][2], lay["head"][2])


@pytest.mark.parametrize("name", NETS)
def test_weights_go_through_the_map_and_back_unchanged(name):
    lay = ops.dense_eval_layout(D.WIDTHS[name])
    ps = D.params(name)
    for (w, b), (k, r, index) in zip(ps, lay["layers"] + [lay["head"]]):
        wb, bb = D.buffer_weight(w, b, k, r, index)
        assert tuple(wb.shape) == (r, 3, 3, k) and tuple(bb.shape) == (r,)
        assert torch.equal(D.reference_weight(wb, w.shape[0], index), w)
        assert not bool(wb[w.shape[0]:].any()) and not bool(bb[w.shape[0]:].any())          # pad rows
        assert not bool(wb[..., index < 0].any())                                           # pad columns
        assert torch.equal(bb[:w.shape[0]], b)
        assert int((wb != 0).sum()) == int((w != 0).sum())
        # the package's own host-side permutation builds the same tensors
        conv = torch.nn.Conv2d(w.shape[1], w.shape[0], 3, 1, 1)
        with torch.no_grad():
            conv.weight.copy_(w)
            conv.bias.copy_(b)
        wo, bo = ops._dense_weight(conv, k, r, index)
        assert torch.equal(wo, wb) and torch.equal(bo, bb) and wo.is_contiguous()


@pytest.mark.parametrize("name", NETS)
def test_buffer_builder_and_its_inverse(name):
    lay = ops.dense_eval_layout(D.WIDTHS[name])
    x = D.rnd(3, (2, 5, 4, 6))
    _, ys, _ = D.stack(D.params(name), x, dtype=torch.float32)
    buf = D.to_buffer(lay, x, ys)
    assert tuple(buf.shape) == (2, 4, 6, lay["ct"]) and not bool(torch.isnan(buf).any())
    for k, t in enumerate([x] + ys):
        got, pads = D.from_buffer(lay, buf, k, t.shape[1])
        assert torch.equal(got, t) and not bool(pads.any())
    ref_in = x
    for k in range(len(ys) + 1):                                   # the input of conv_k read back through the map is the concatenation
        assert torch.equal(D.gather_input(lay, k, buf), ref_in)
        if k < len(ys):
            ref_in = torch.cat((ys[k], ref_in), 1)
    short = D.to_buffer(lay, x, ys[:2])
    assert bool(torch.isnan(short[..., lay["offsets"][3]:]).all()) and not bool(torch.isnan(short[..., :lay["offsets"][3]]).any())


def test_layout_refuses_nonsense():
    for bad in (((), 5), ((8, 0), 5), ((8, 8), 0), ((8, 8), 17)):
        with pytest.raises(ValueError):
            ops.dense_eval_layout(*bad)


# ---------------------------------------------------------------- the frame ranges
def test_chunks_tile_the_batch_within_both_bounds():
    assert ops.DENSE_EVAL_BUDGET == 4 << 30
    for ct in (464, 176):
        assert ops.dense_eval_chunks(25, 224, 224, ct) == [(0, 25)]           # the evaluator's batch is one range
    cases = [(250, 224, 224, 464, None), (250, 224, 224, 176, None), (1, 224, 224, 464, None), (47, 224, 224, 464, None), (7, 1024, 1024, 176, None),
             (3, 33, 18, 464, None), (1000, 56, 448, 176, None), (5, 20, 37, 464, 2 * 20 * 37 * 464 * 4), (5, 20, 37, 176, 2 * 20 * 37 * 176 * 4 + 3),
             (9, 8, 8, 464, 1 << 40)]
    for n, h, w, ct, budget in cases:
        ch = ops.dense_eval_chunks(n, h, w, ct) if budget is None else ops.dense_eval_chunks(n, h, w, ct, budget_bytes=budget)
        assert ch[0][0] == 0 and ch[-1][1] == n
        for (a, b), (c, _) in zip(ch, ch[1:] + [(n, n)]):
            assert a < b and b == c
            assert (b - a) * h * w * ct < 2 ** 31
            assert (b - a) * h * w * ct * 4 <= (ops.DENSE_EVAL_BUDGET if budget is None else budget)
    assert ops.dense_eval_chunks(5, 20, 37, 464, budget_bytes=2 * 20 * 37 * 464 * 4) == [(0, 2), (2, 4), (4, 5)]
    assert len(ops.dense_eval_chunks(250, 224, 224, 464)) == 6 and len(ops.dense_eval_chunks(250, 224, 224, 176)) == 3
    # the index bound alone (a budget that never binds): 2^31 elements
    big = ops.dense_eval_chunks(100, 224, 224, 464, budget_bytes=1 << 40)
    assert big[0] == (0, (2 ** 31 - 1) // (224 * 224 * 464)) and big[0][1] == 92
    for bad in ((0, 8, 8, 464), (2, 0, 8, 464), (2, 8, 8, 0), (1, 4096, 4096, 176)):
        with pytest.raises(ValueError):
            ops.dense_eval_chunks(*bad)
    with pytest.raises(ValueError):                                # a budget smaller than one frame
        ops.dense_eval_chunks(3, 20, 37, 464, budget_bytes=20 * 37 * 464 * 4 - 1)
    assert ops.dense_eval_chunks(3, 20, 37, 464, budget_bytes=20 * 37 * 464 * 4) == [(0, 1), (1, 2), (2, 3)]


# ---------------------------------------------------------------- the predicate and the stock forward
def _small():
    torch.manual_seed(5)
    return model.EstimatorDenseNetSmall().eval()


def _with_slope():
    net = _small()
    net.conv_2[1] = torch.nn.LeakyReLU(0.2)
    return net


def _without_bias():
    net = _small()
    old = net.conv_3[0]
    net.conv_3[0] = torch.nn.Conv2d(old.in_channels, old.out_channels, 3, 1, 1, bias=False)
    return net


def _wide():
    torch.manual_seed(6)
    return model.DenseEstimatorBase((32, 160, 8)).eval()


def _early_fusion():
    torch.manual_seed(7)
    return model.EstimatorDenseNetTinyEarlyFusionSum().eval()


DEFECTS = {"leaky-0.2": _with_slope, "no-bias": _without_bias, "width-160": _wide, "early-fusion": _early_fusion}


def _stock(net, x):
    if isinstance(net, model._EarlyFusion):
        m, r = net.conv_0_mv(x[:, :2]), net.conv_0_r(x[:, 2:])
        t = m + r
        for i in (1, 2, 3, 4):
            t = torch.cat((getattr(net, "conv_%d" % i)(t), t), 1)
        return net.predict_flow(t)
    return D.stock_forward(net, x)


def test_structural_part_of_the_predicate():
    """Without a GPU the predicate is False at its first test (a CPU tensor); the structural part (_dense_plan) is checked on its
    own: it accepts the two networks and refuses each defect."""
    for name in NETS:
        net = model._ESTIMATORS[name]().eval()
        assert ops._dense_plan(net) is None                        # CPU parameters: not served
        convs, head = ops._dense_plan(net, on_device=False)
        assert [c.out_channels for c in convs] == list(D.WIDTHS[name]) and head is net.predict_flow
    for what, make in DEFECTS.items():
        assert ops._dense_plan(make(), on_device=False) is None, what
    net = _small()
    net.conv_1[0].padding = (2, 2)
    assert ops._dense_plan(net, on_device=False) is None
    net = _small()
    net.predict_flow = torch.nn.Conv2d(117, 3, 3, 1, 1)
    assert ops._dense_plan(net, on_device=False) is None
    assert ops._dense_plan(_small().double(), on_device=False) is None


@pytest.mark.parametrize("what", ["cpu", "grad", "4-channels"] + sorted(DEFECTS))
def test_unsupported_cases_take_the_stock_forward(what):
    net = DEFECTS[what]() if what in DEFECTS else _small()
    x = D.rnd(1, (2, 4 if what == "4-channels" else 5, 12, 9))
    if what == "4-channels":
        with torch.no_grad():
            assert not ops.dense_eval_supported(net, x)
            with pytest.raises(RuntimeError):                      # the stock modules' own complaint, not a kernel's
                net(x)
            with pytest.raises(_lib.DmcHipError):
                ops.dense_eval(net, x)
        return
    if what == "grad":
        assert torch.is_grad_enabled() and not ops.dense_eval_supported(net, x)
        got, want = net(x), _stock(net, x)
        assert got.requires_grad and torch.equal(got, want)
        return
    with torch.no_grad():
        assert not ops.dense_eval_supported(net, x)
        assert torch.equal(net(x), _stock(net, x))
        with pytest.raises(_lib.DmcHipError):
            ops.dense_eval(net, x)


def test_flag_off_is_the_stock_forward(monkeypatch):
    monkeypatch.setattr(model, "DENSE_EVAL", False)
    monkeypatch.setattr(ops, "dense_eval_supported", lambda net, x: pytest.fail("the predicate is not consulted with the flag off"))
    for name in NETS:
        net = model._ESTIMATORS[name]().eval()
        x = D.rnd(2, (1, 5, 7, 6))
        with torch.no_grad():
            assert torch.equal(net(x), D.stock_forward(net, x))


def test_predicate_refuses_other_inputs():
    net = _small()
    with torch.no_grad():
        for bad in (torch.zeros(2, 5, 8, 8, dtype=torch.float64), torch.zeros(2, 4, 8, 8), torch.zeros(5, 8, 8), torch.zeros(0, 5, 8, 8), None):
            assert not ops.dense_eval_supported(net, bad)


def test_tiny_and_early_fusion_never_reach_the_route(monkeypatch):
    monkeypatch.setattr(ops, "dense_eval", lambda net, x: pytest.fail("dense_eval called"))
    monkeypatch.setattr(ops, "dense_eval_supported", lambda net, x: True)
    assert model.EstimatorDenseNetTiny.forward is not model.DenseEstimatorBase.forward
    assert not issubclass(model._EarlyFusion, model.DenseEstimatorBase)
    net = _early_fusion()
    with torch.no_grad():
        x = D.rnd(4, (1, 5, 6, 6))
        assert torch.equal(net(x), _stock(net, x))


def test_which_class_consults_the_route_by_default(monkeypatch):
    """DMC_DENSE_EVAL unset: EstimatorDenseNet consults the predicate; EstimatorDenseNetSmall (slower on the route) only when the stock
    forward's widest concatenation reaches 4 GiB -- 183 frames of 224 x 224 at its 117 channels -- or with DMC_DENSE_EVAL=1."""
    asked = []
    monkeypatch.setattr(ops, "dense_eval_supported", lambda net, x: (asked.append(type(net).__name__), True)[1])
    monkeypatch.setattr(ops, "dense_eval", lambda net, x: "route")
    monkeypatch.setattr(model, "DENSE_EVAL", True)
    monkeypatch.setattr(model, "DENSE_EVAL_ALL", False)
    big, small = model.EstimatorDenseNet(), model.EstimatorDenseNetSmall()
    assert big.DENSE_EVAL_BY_DEFAULT and not small.DENSE_EVAL_BY_DEFAULT and model.DenseEstimatorBase.DENSE_EVAL_BY_DEFAULT
    x = torch.zeros(1, 5, 6, 6)
    with torch.no_grad():
        assert big(x) == "route" and asked == ["EstimatorDenseNet"]
        assert torch.equal(small(x), D.stock_forward(small, x)) and asked == ["EstimatorDenseNet"]
        for frames, passes in ((182, False), (183, True), (250, True)):
            meta = torch.empty((frames, 5, 224, 224), device="meta")
            assert small._stock_passes_4gib(meta) == passes == (frames * 224 * 224 * 117 * 4 >= 2 ** 32)
        assert small(torch.empty((183, 5, 224, 224), device="meta")) == "route" and asked[-1] == "EstimatorDenseNetSmall"
        monkeypatch.setattr(model, "DENSE_EVAL_ALL", True)
        assert small(x) == "route"
        monkeypatch.setattr(model, "DENSE_EVAL", False)            # =0 wins over everything
        assert torch.equal(small(x), D.stock_forward(small, x)) and torch.equal(big(x), D.stock_forward(big, x))


def test_flag_is_read_from_the_environment_once():
    code = "import sys; sys.path.insert(0, %r); from dmcnet_amd import model; print(int(model.DENSE_EVAL) + 2 * int(model.DENSE_EVAL_ALL))" % ROOT
    for value, want in ((None, "1"), ("0", "0"), ("1", "3")):
        env = dict(os.environ)
        env.pop("DMC_DENSE_EVAL", None)
        if value is not None:
            env["DMC_DENSE_EVAL"] = value
        out = subprocess.run([sys.executable, "-c", code], env=env, stdout=subprocess.PIPE, check=True, universal_newlines=True).stdout
        assert out.strip().splitlines()[-1] == want, (value, out)


# ---------------------------------------------------------------- the C ABI without a GPU
def test_size_and_capability_queries_without_gpu():
    lib = _lib.load()
    for name in NETS:
        ks, rs, ct = D.EXPECTED[name]
        for k, r in zip(ks, rs):
            assert lib.dmc_dense_supported(25, 224, 224, ct, k, r) == 1, (name, k, r)
            assert lib.dmc_dense_wpack_bytes(k, r) == k * r * 9 * 3 * 2
        assert lib.dmc_dense_supported(25, 224, 224, ct, ct, 2) == 1
    assert lib.dmc_dense_supported(92, 224, 224, 464, 432, 32) == 1 and lib.dmc_dense_supported(93, 224, 224, 464, 432, 32) == 0      # 2^31 elements
    assert lib.dmc_dense_supported(31, 448, 448, 176, 144, 32) == 1
    assert lib.dmc_dense_supported(1, 8, 8, 512, 512, 2) == 1 and lib.dmc_dense_supported(1, 8, 8, 528, 528, 2) == 0
    assert lib.dmc_dense_supported(1, 8, 8, 464, 432, 32) == 1 and lib.dmc_dense_supported(1, 8, 8, 464, 448, 32) == 0                # K + R > CT
    assert lib.dmc_dense_supported(1, 8, 8, 464, 464, 2) == 1 and lib.dmc_dense_supported(1, 8, 8, 464, 480, 2) == 0                  # K > CT
    for n, h, w, ct, k, r in ((0, 8, 8, 464, 16, 128), (1, 0, 8, 464, 16, 128), (1, 8, -1, 464, 16, 128), (1, 8, 8, 462, 16, 128),
                              (1, 8, 8, 464, 24, 128), (1, 8, 8, 464, 0, 128), (1, 8, 8, 464, 16, 48), (1, 8, 8, 464, 16, 160),
                              (1, 8, 8, 464, 16, 0), (1, 8, 8, 464, 16, 3), (1, 8, 8, 520, 516, 2), (1, 8, 8, 0, 16, 32), (1, 8, 8, 8, 8, 2)):
        assert lib.dmc_dense_supported(n, h, w, ct, k, r) == 0, (n, h, w, ct, k, r)
    for k, r in ((24, 32), (16, 48), (0, 32), (16, 2), (-16, 32)):
        assert lib.dmc_dense_wpack_bytes(k, r) == 0, (k, r)


def test_refusals_are_loud_and_launch_nothing():
    lib = _lib.load()
    p = _lib.ptr(torch.zeros(16))                                 # any non-null pointer: nothing is launched

    def refused(name, rc):
        assert rc == -1, name
        assert name.encode() in lib.dmc_last_error(), (name, lib.dmc_last_error())

    # null pointers, every position
    for i in range(2):
        a = [p, p]
        a[i] = None
        refused("dmc_dense_pack_weights", lib.dmc_dense_pack_weights(*a, 16, 32, None))
        refused("dmc_dense_ingest", lib.dmc_dense_ingest(*a, 1, 8, 8, 464, None))
    for i in range(3):
        a = [p] * 3
        a[i] = None
        refused("dmc_dense_layer_eval", lib.dmc_dense_layer_eval(*a, 1, 8, 8, 464, 16, 128, None))
    for i in range(4):
        a = [p] * 4
        a[i] = None
        refused("dmc_dense_head_eval", lib.dmc_dense_head_eval(*a, 1, 8, 8, 464, 464, None))
    # K = 24; R = 48; K + R > CT; CT = 462; sizes
    for ct, k, r in ((464, 24, 128), (464, 16, 48), (464, 448, 32), (462, 16, 128), (464, 16, 2)):
        refused("dmc_dense_layer_eval", lib.dmc_dense_layer_eval(p, p, p, 1, 8, 8, ct, k, r, None))
        assert b"unsupported shape" in lib.dmc_last_error()
    for n, h, w in ((0, 8, 8), (1, -2, 8), (93, 224, 224)):
        refused("dmc_dense_layer_eval", lib.dmc_dense_layer_eval(p, p, p, n, h, w, 464, 432, 32, None))
        refused("dmc_dense_ingest", lib.dmc_dense_ingest(p, p, n, h, w, 464, None))
        refused("dmc_dense_head_eval", lib.dmc_dense_head_eval(p, p, p, p, n, h, w, 464, 464, None))
    for k, r in ((24, 32), (16, 48), (0, 32)):
        refused("dmc_dense_pack_weights", lib.dmc_dense_pack_weights(p, p, k, r, None))
    for ct in (462, 12, 0):
        refused("dmc_dense_ingest", lib.dmc_dense_ingest(p, p, 1, 8, 8, ct, None))
    # head: K = 516 (over 512 and no multiple of 16); K > CT; CT = 462; K = 24
    for ct, k in ((520, 516), (464, 480), (462, 16), (464, 24), (528, 528)):
        refused("dmc_dense_head_eval", lib.dmc_dense_head_eval(p, p, p, p, 1, 8, 8, ct, k, None))
        assert b"unsupported shape" in lib.dmc_last_error()
