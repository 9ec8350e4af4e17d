"""GPU: the memory contract of every launching dmc_ef_* entry point (csrc/early_fusion.hip) on the guarded arenas of
tests/abi_arena.py -- buffers of exactly the promised size with a megabyte of fill on both sides, once over 0xFF and once over 0x00:
nothing outside them is touched, inputs stay as they were, every output element is written and does not depend on what the
workspace or the guard bands held, and a refused call writes nothing.  Each case also checks its values against fp64 autograd of
the same convolution in buffer order (3 frames of 33 x 18: 1782 pixels, two runs of partial sums)."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from dmcnet_amd import _lib
from tests import abi_cases
from tests import ef_ref as E
from tests.abi_arena import run_case

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SHAPE = (3, 5, 33, 18)
N, H, W = 3, 33, 18
CAP = 48 << 20
I16 = torch.int16


def rel_err(a, b):
    a, b = a.detach().double().cpu(), torch.as_tensor(b).detach().double().cpu()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))


def nchw(t):
    return t.permute(0, 3, 1, 2)


def oihw(wb):
    """[R, 9, K] buffer order -> [R, K, 3, 3]."""
    r, _, k = wb.shape
    return wb.reshape(r, 3, 3, k).permute(0, 3, 1, 2)


@functools.lru_cache(maxsize=None)
def data(name, li):
    """Everything a case of conv_{li + 1} (li == 4: predict_flow) needs, fp32 on the CPU; never modified: the full feature buffer, the
    weight [R, 9, K] and bias in buffer order, a gradient buffer G and dout."""
    lay = E.layout(name)
    k, r, index = (lay["layers"] + [lay["head"]])[li]
    x, f, _ = E.reference(name, SHAPE)
    full = E.to_buffer(name, f, 5)
    assert not bool(torch.isnan(full).any())
    wt, b = E.params(name)[2 + li]
    return {"k": k, "r": r, "ct": lay["ct"], "x": x, "full": full, "w": E.buffer_weight(wt, k, index), "b": b,
            "G": E.rnd(61 + li, (N, H, W, lay["ct"])), "dout": E.rnd(67, (N, 2, H, W)),
            "signs": sign_plane(f["a"], f["b"])}


def sign_plane(a, b):
    """int16 [N, H, W] (the uint16's bits): bit c = (a_c > 0), bit 8 + c = (b_c > 0)."""
    bits = np.zeros(tuple(a.shape[:1] + a.shape[2:]), np.uint16)
    for c in range(8):
        bits |= (a[:, c] > 0).numpy().astype(np.uint16) << c
        bits |= (b[:, c] > 0).numpy().astype(np.uint16) << (8 + c)
    return torch.from_numpy(bits.view(np.int16).copy())


def first_case(name):
    stack = name == "Stack"

    def fn(a):
        d = data(name, 0)
        (wm, bm), (wr, br) = E.params(name)[:2]
        feat = torch.full((N, H, W, d["ct"]), float("nan"))
        a.call("dmc_ef_first", a.inp("x", d["x"]), a.inp("w_mv", wm), a.inp("b_mv", bm), a.inp("w_r", wr), a.inp("b_r", br),
               a.inout("feat", feat, nan_ok=True), a.out("signs", (N, H, W), dtype=I16), N, H, W, d["ct"], int(stack))

    def check(bufs):
        d = data(name, 0)
        live = 16 if stack else 8
        feat = bufs["feat"].t
        assert rel_err(feat[..., :live], d["full"][..., :live]) < 1e-5 and bool(torch.isnan(feat[..., live:]).all())
        assert float((bufs["signs"].t.cpu() != d["signs"]).double().mean()) < 1e-3     # (fp32 against fp64 next to zero)
    return fn, check


def layer_case(name, li):
    def fn(a):
        d = data(name, li)
        buf = d["full"].clone()
        buf[..., d["k"]:] = float("nan")
        a.call("dmc_ef_layer", a.inout("feat", buf, nan_ok=True), a.inp("w", d["w"]), a.inp("bias", d["b"]), N, H, W, d["ct"], d["k"], d["r"])

    def check(bufs):
        d = data(name, li)
        k, r4 = d["k"], (d["r"] + 3) // 4 * 4
        feat = bufs["feat"].t.cpu()
        assert rel_err(feat[..., k:k + r4], d["full"][..., k:k + r4]) < 1e-5
        assert torch.equal(feat[..., :k], d["full"][..., :k]) and bool(torch.isnan(feat[..., k + r4:]).all())
    return fn, check


def head_case(name):
    def fn(a):
        d = data(name, 4)
        a.call("dmc_ef_head", a.inp("feat", d["full"]), a.inp("w", d["w"]), a.inp("bias", d["b"]), a.out("out", (N, 2, H, W)), N, H, W, d["ct"], d["k"])

    def check(bufs):
        assert rel_err(bufs["out"].t, E.reference(name, SHAPE)[1]["out"]) < 1e-5
    return fn, check


def conv_grads(inp_nhwc, wb, dy_nchw):
    """fp64 autograd of conv2d(inp, w) with the output gradient dy: (d inp NHWC, dw [R, 9, K], db [R])."""
    xi = nchw(inp_nhwc).double().contiguous().requires_grad_(True)
    w = oihw(wb).double().contiguous().requires_grad_(True)
    b = torch.zeros(w.shape[0], dtype=torch.float64, requires_grad=True)
    gx, gw, gb = torch.autograd.grad((F.conv2d(xi, w, b, 1, 1) * dy_nchw.double()).sum(), [xi, w, b])
    return gx.permute(0, 2, 3, 1), gw.permute(0, 2, 3, 1).reshape(w.shape[0], 9, w.shape[1]), gb


def head_dgrad_case(name):
    def fn(a):
        d = data(name, 4)
        a.call("dmc_ef_head_dgrad", a.inp("dout", d["dout"]), a.inp("w", d["w"]), a.out("G", (N, H, W, d["ct"])), N, H, W, d["ct"], d["k"])

    def check(bufs):
        d = data(name, 4)
        assert rel_err(bufs["G"].t, conv_grads(d["full"], d["w"], d["dout"])[0]) < 1e-5
    return fn, check


def head_wgrad_case(name):
    def fn(a):
        d = data(name, 4)
        ws = a.work("workspace", _lib.load().dmc_ef_head_wgrad_workspace_bytes(N, H, W, d["k"]))
        a.call("dmc_ef_head_wgrad", a.inp("dout", d["dout"]), a.inp("feat", d["full"]), a.out("dw", (2, 9, d["k"])), a.out("db", (2,)), ws,
               N, H, W, d["ct"], d["k"])

    def check(bufs):
        d = data(name, 4)
        _, gw, gb = conv_grads(d["full"], d["w"], d["dout"])
        assert rel_err(bufs["dw"].t, gw) < 2e-5 and rel_err(bufs["db"].t, gb) < 2e-5
    return fn, check


def masked(d):
    k, r4 = d["k"], (d["r"] + 3) // 4 * 4
    g, f = d["G"][..., k:k + r4], d["full"][..., k:k + r4]
    return torch.where(f > 0, g, torch.tensor(0.1, dtype=torch.float32) * g)


def mask_case(name, li):
    def fn(a):
        d = data(name, li)
        ws = a.work("workspace", _lib.load().dmc_ef_layer_mask_workspace_bytes(N, H, W, d["r"]))
        a.call("dmc_ef_layer_mask", a.inp("feat", d["full"]), a.inout("G", d["G"]), a.out("db", (d["r"],)), ws, N, H, W, d["ct"], d["k"], d["r"])

    def check(bufs):
        d = data(name, li)
        k, r, r4 = d["k"], d["r"], (d["r"] + 3) // 4 * 4
        G = bufs["G"].t.cpu()
        assert torch.equal(G[..., k:k + r4], masked(d))
        assert torch.equal(G[..., :k], d["G"][..., :k]) and torch.equal(G[..., k + r4:], d["G"][..., k + r4:])
        assert rel_err(bufs["db"].t, masked(d).double().sum((0, 1, 2))[:r]) < 2e-5
    return fn, check


def layer_wgrad_case(name, li):
    def fn(a):
        d = data(name, li)
        ws = a.work("workspace", _lib.load().dmc_ef_layer_wgrad_workspace_bytes(N, H, W, d["k"], d["r"]))
        a.call("dmc_ef_layer_wgrad", a.inp("feat", d["full"]), a.inp("G", d["G"]), a.out("dw", (d["r"], 9, d["k"])), ws, N, H, W, d["ct"], d["k"], d["r"])

    def check(bufs):
        d = data(name, li)
        k, r = d["k"], d["r"]
        _, gw, _ = conv_grads(d["full"][..., :k], d["w"], nchw(d["G"][..., k:k + r]))
        assert rel_err(bufs["dw"].t, gw) < 2e-5
    return fn, check


def layer_dgrad_case(name, li):
    def fn(a):
        d = data(name, li)
        a.call("dmc_ef_layer_dgrad", a.inout("G", d["G"]), a.inp("w", d["w"]), N, H, W, d["ct"], d["k"], d["r"])

    def check(bufs):
        d = data(name, li)
        k, r = d["k"], d["r"]
        gx, _, _ = conv_grads(d["full"][..., :k], d["w"], nchw(d["G"][..., k:k + r]))
        G = bufs["G"].t.cpu()
        assert rel_err(G[..., :k], d["G"][..., :k].double() + gx) < 1e-5
        assert torch.equal(G[..., k:], d["G"][..., k:])
    return fn, check


def first_bwd_case(name):
    stack = name == "Stack"

    def fn(a):
        d = data(name, 0)
        ws = a.work("workspace", _lib.load().dmc_ef_first_bwd_workspace_bytes(N, H, W))
        a.call("dmc_ef_first_bwd", a.inp("G", d["G"]), a.inp("x", d["x"]), None if stack else a.inp("signs", d["signs"]),
               a.inp("feat", d["full"]) if stack else None, a.out("dw_mv", (8, 2, 3, 3)), a.out("db_mv", (8,)), a.out("dw_r", (8, 3, 3, 3)),
               a.out("db_r", (8,)), ws, N, H, W, d["ct"], int(stack))

    def check(bufs):
        d = data(name, 0)
        ps = [(w.requires_grad_(True), b.requires_grad_(True)) for w, b in E.params(name, torch.float64)[:2]]
        x = d["x"].double()
        m = F.leaky_relu(F.conv2d(x[:, :2], ps[0][0], ps[0][1], 1, 1), E.SLOPE)
        r = F.leaky_relu(F.conv2d(x[:, 2:], ps[1][0], ps[1][1], 1, 1), E.SLOPE)
        g = nchw(d["G"]).double()
        loss = (m * g[:, :8]).sum() + (r * (g[:, 8:16] if stack else g[:, :8])).sum()
        want = torch.autograd.grad(loss, [ps[0][0], ps[0][1], ps[1][0], ps[1][1]])
        for key, w_ in zip(("dw_mv", "db_mv", "dw_r", "db_r"), want):
            assert rel_err(bufs[key].t, w_) < 2e-5, key
    return fn, check


def refused_layer(a):           # K + round_up4(R) > CT
    a.call("dmc_ef_layer", a.inout("feat", torch.ones(1, 8, 8, 40)), a.inp("w", torch.zeros(6, 9, 36)), a.inp("bias", torch.zeros(6)), 1, 8, 8, 40, 36, 6)


def refused_head_dgrad(a):      # CT over 64
    a.call("dmc_ef_head_dgrad", a.inp("dout", torch.ones(1, 2, 8, 8)), a.inp("w", torch.zeros(2, 9, 40)), a.out("G", (1, 8, 8, 72)), 1, 8, 8, 72, 40)


def refused_first_bwd(a):       # Sum without its sign plane
    ws = a.work("workspace", _lib.load().dmc_ef_first_bwd_workspace_bytes(1, 8, 8))
    a.call("dmc_ef_first_bwd", a.inp("G", torch.ones(1, 8, 8, 32)), a.inp("x", torch.ones(1, 5, 8, 8)), None, a.inp("feat", torch.ones(1, 8, 8, 32)),
           a.out("dw_mv", (8, 2, 3, 3)), a.out("db_mv", (8,)), a.out("dw_r", (8, 3, 3, 3)), a.out("db_r", (8,)), ws, 1, 8, 8, 32, 0)


def refused_mask(a):            # R = 5
    ws = a.work("workspace", 64)
    a.call("dmc_ef_layer_mask", a.inp("feat", torch.ones(1, 8, 8, 40)), a.inout("G", torch.ones(1, 8, 8, 40)), a.out("db", (8,)), ws, 1, 8, 8, 40, 16, 5)


ARENA_CASES = []


def _add(id, covers, pair, **kw):
    fn, check = pair if isinstance(pair, tuple) else (pair, None)
    ARENA_CASES.append(abi_cases.Case(id, covers, fn, check=check, capacity=CAP, **kw))


for _name in E.NETS:
    _add("dmc_ef_first-" + _name, ["dmc_ef_first"], first_case(_name))
    _add("dmc_ef_head-" + _name, ["dmc_ef_head"], head_case(_name))
    _add("dmc_ef_head_dgrad-" + _name, ["dmc_ef_head_dgrad"], head_dgrad_case(_name))
    _add("dmc_ef_head_wgrad-" + _name, ["dmc_ef_head_wgrad"], head_wgrad_case(_name))
    _add("dmc_ef_first_bwd-" + _name, ["dmc_ef_first_bwd"], first_bwd_case(_name))
    for _li in range(4):
        _add("dmc_ef_layer-%s-conv_%d" % (_name, _li + 1), ["dmc_ef_layer"], layer_case(_name, _li))
        _add("dmc_ef_layer_mask-%s-conv_%d" % (_name, _li + 1), ["dmc_ef_layer_mask"], mask_case(_name, _li))
        _add("dmc_ef_layer_wgrad-%s-conv_%d" % (_name, _li + 1), ["dmc_ef_layer_wgrad"], layer_wgrad_case(_name, _li))
        _add("dmc_ef_layer_dgrad-%s-conv_%d" % (_name, _li + 1), ["dmc_ef_layer_dgrad"], layer_dgrad_case(_name, _li))
_add("dmc_ef_layer-refused-K+R-over-CT", ["dmc_ef_layer"], refused_layer, expect_rc=abi_cases.DMC_E_INVALID)
_add("dmc_ef_head_dgrad-refused-CT-72", ["dmc_ef_head_dgrad"], refused_head_dgrad, expect_rc=abi_cases.DMC_E_INVALID)
_add("dmc_ef_first_bwd-refused-no-signs", ["dmc_ef_first_bwd"], refused_first_bwd, expect_rc=abi_cases.DMC_E_INVALID)
_add("dmc_ef_layer_mask-refused-R-5", ["dmc_ef_layer_mask"], refused_mask, expect_rc=abi_cases.DMC_E_INVALID)
# the shared list: tests/test_abi_arena_cpu.py counts these cases as the dmc_ef_* entry points' coverage and dry-runs them on the CPU
_known = {c.id for c in abi_cases.CASES}
abi_cases.CASES.extend(c for c in ARENA_CASES if c.id not in _known)


@pytest.mark.parametrize("case", ARENA_CASES, ids=[c.id for c in ARENA_CASES])
def test_early_fusion_entries_memory_contract(case):
    try:
        bufs = run_case(case.fn, device=DEV, capacity=case.capacity, expect_rc=case.expect_rc)
        if case.check is not None:
            case.check(bufs)
    except RuntimeError as e:
        if "HIP error" in str(e) or "illegal memory access" in str(e):
            # a faulted device serves nothing more: end the session here instead of launching the remaining cases on it
            pytest.exit("GPU fault in %s: %s" % (case.id, str(e).splitlines()[0]), returncode=3)
        raise


def test_every_launching_entry_point_has_a_case():
    covered = {n for c in ARENA_CASES for n in c.covers}
    launching = {n for n in _lib.SIGNATURES if n.startswith("dmc_ef_") and not n.endswith(("_supported", "_bytes"))}
    assert covered == launching and len(launching) == 9
