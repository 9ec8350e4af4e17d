"""GPU: the eval-mode epilogues of the pre-split forward kernels (dmc_x3s_conv_bn_eval, dmc_x3q_conv_bn_eval) and their dispatch.

The two entry points are compared BIT FOR BIT (torch.equal on the fp32 output and on the slice bytes) with the two-pass route they
replace -- the convolution entry followed by the streaming BatchNorm entries, all through ctypes -- because the epilogue evaluates
the same expression in the same order and the build forbids contraction.  One case per entry is also tied to the stock modules in
fp64 at the bar of this arithmetic (rel_err < 1e-5, tests/test_x3s_gpu.py).  Above the C ABI: a ResidualUnit, a stride-2 block
wired as ResNet wires it, and the whole classifier through evaluate.forward_video / driver.validate with resnet.EVAL_FUSED on and
off (the scores within the existing 1e-4 of the oracle model), the entry points of the fused forward recorded and counted.

Shapes (n, cin, h, w, cout) are the smallest at which the kernels can go wrong: 256-pixel tiles crossing image rows, a ragged last
tile with tiles spanning images (M = 343), H != W, two channel tiles, the 7 x 7 maps of layer4, the 128-pixel two-workgroup
configuration by option; for the pair: one output pixel per image, H != W, 192 channels (three channel tiles), the 28-wide maps.

The arena cases of both entry points are built here and appended to the registry of tests/abi_cases.py at import (the registry's
coverage check, tests/test_abi_arena_cpu.py, then sees the entry points); they are RUN here."""
import copy
import ctypes

import numpy as np
import pytest
import torch

import dmcnet_amd
from dmcnet_amd import _lib, ops, resnet
from oracle import dmc_oracle as O
from tests import abi_cases
from tests.abi_arena import run_case

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CL = torch.channels_last
U8 = torch.uint8
EPS = 1e-5


def rnd(seed, shape, scale=1.0):
    return torch.from_numpy((np.random.RandomState(seed).standard_normal(shape) * scale).astype(np.float32))


def pos(seed, shape):
    return torch.from_numpy(np.random.RandomState(seed).uniform(0.5, 1.5, shape).astype(np.float32))


def rel_err(a, b):
    a, b = a.detach().double().cpu(), torch.as_tensor(b).detach().double().cpu()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))


def P(t):
    return _lib.ptr(t)


def ok(rc, what):
    _lib.check(rc, what)


def bn_params(seed, c, device):
    """(stats = [mean, 1 / sqrt(var + eps)], gamma, beta, mean, var) of a seeded BatchNorm; stats as ops builds them, on ``device``."""
    mean, var = rnd(seed, (c,), 0.3).to(device), pos(seed + 1, (c,)).to(device)
    gamma, beta = pos(seed + 2, (c,)).to(device), rnd(seed + 3, (c,), 0.2).to(device)
    stats = torch.cat([mean, torch.rsqrt(var + EPS)]).contiguous()
    return stats, gamma, beta, mean, var


def f32_out(m, c):
    return torch.full((m, c), float("nan"), dtype=torch.float32, device=DEV)


def slice_out(m, c):
    return torch.full((m * c * 6,), 0xFF, dtype=U8, device=DEV)


def bn_two_pass(y, res, gamma, beta, stats, relu, want_f32, want_sl, s2d_geom=None):
    """The streaming reference pass on y [M][C]: (out fp32 | None, slice bytes | None).  The reference entries take power-of-two
    channel counts; another count (192) is served in 64-channel column blocks -- a chunk plane holds 16 channels, so a block's slice
    tensor is four whole planes of each slice of the full tensor."""
    lib = _lib.load()
    m, c = y.shape
    if c & (c - 1) == 0:
        out, ys = (f32_out(m, c) if want_f32 else None), (slice_out(m, c) if want_sl else None)
        if s2d_geom is not None:
            n, h, w = s2d_geom
            ok(lib.dmc_bn_apply_act_x3q(P(y), P(res), P(gamma), P(beta), P(stats), P(out), P(ys), None, n, h, w, c, relu, ops._stream()),
               "dmc_bn_apply_act_x3q")
        else:
            ok(lib.dmc_bn_apply_act_x3s(P(y), P(res), P(gamma), P(beta), P(stats), P(out), P(ys), None, m, c, relu, ops._stream()),
               "dmc_bn_apply_act_x3s")
        return out, ys
    assert s2d_geom is None and c % 64 == 0
    out = f32_out(m, c) if want_f32 else None
    ys = slice_out(m, c).view(3, c // 16, m * 32) if want_sl else None
    for k in range(c // 64):
        sl = slice(64 * k, 64 * k + 64)
        st = torch.cat([stats[:c][sl], stats[c:][sl]]).contiguous()
        o, s = bn_two_pass(y[:, sl].contiguous(), None if res is None else res[:, sl].contiguous(), gamma[sl].contiguous(),
                           beta[sl].contiguous(), st, relu, want_f32, want_sl)
        if want_f32:
            out[:, sl] = o
        if want_sl:
            ys[:, 4 * k:4 * k + 4] = s.view(3, 4, m * 32)
    return out, (ys.reshape(-1) if want_sl else None)


# ---------------------------------------------------------------------------------------------------------------------
# 1. dmc_x3s_conv_bn_eval, bit for bit
# ---------------------------------------------------------------------------------------------------------------------
X3S_SHAPES = [(2, 64, 56, 56, 64), (7, 64, 7, 7, 64), (2, 64, 10, 14, 64), (3, 64, 28, 28, 128), (1, 128, 14, 14, 64), (5, 512, 7, 7, 512)]
#: (fp32, slices, s2d)
OUTPUT_SETS = [(1, 0, 0), (0, 1, 0), (1, 1, 0), (0, 1, 1), (1, 1, 1)]


def x3s_inputs(shape):
    n, cin, h, w, cout = shape
    x = rnd(501, (n, cin, h, w)).to(DEV).contiguous(memory_format=CL)
    wt = rnd(502, (cout, cin, 3, 3), 0.1).to(DEV).contiguous(memory_format=CL)
    res = rnd(503, (n * h * w, cout)).to(DEV)
    return x, wt, res


def check_x3s_shape(shape, fp64_case=False):
    n, cin, h, w, cout = shape
    m = n * h * w
    lib = _lib.load()
    assert lib.dmc_x3s_conv_supported(n, h, w, cin, cout)
    x, wt, res = x3s_inputs(shape)
    xs = ops.x3s_split(x)
    wf, _ = ops.x3s_pack_weights(wt, forward=True, transposed=False)
    stats, gamma, beta, mean, var = bn_params(510, cout, DEV)
    y = torch.empty((m, cout), dtype=torch.float32, device=DEV)          # the two-pass route's convolution result, once per shape
    ok(lib.dmc_x3s_conv_fwd(P(xs), P(wf), P(y), None, 0, n, h, w, cin, cout, ops._stream()), "dmc_x3s_conv_fwd")
    for relu in (0, 1):
        for with_res in (0, 1):
            r = res if with_res else None
            for f32, sl, s2d in OUTPUT_SETS:
                if s2d and ((h | w) & 1):
                    continue
                want_out, want_ys = bn_two_pass(y, r, gamma, beta, stats, relu, f32, sl, (n, h, w) if s2d else None)
                out, ys = (f32_out(m, cout) if f32 else None), (slice_out(m, cout) if sl else None)
                ok(lib.dmc_x3s_conv_bn_eval(P(xs), P(wf), P(stats), P(gamma), P(beta), P(r), P(out), P(ys), s2d, relu, n, h, w, cin, cout,
                                            ops._stream()), "dmc_x3s_conv_bn_eval")
                what = (shape, relu, with_res, f32, sl, s2d)
                if f32:
                    assert torch.equal(out, want_out), what
                if sl:
                    assert torch.equal(ys, want_ys), what
    if fp64_case:       # against the stock modules in fp64
        conv = torch.nn.Conv2d(cin, cout, 3, padding=1, bias=False).double()
        bn = torch.nn.BatchNorm2d(cout, eps=EPS).double().eval()
        with torch.no_grad():
            conv.weight.copy_(wt.cpu().double()); bn.weight.copy_(gamma.cpu().double()); bn.bias.copy_(beta.cpu().double())
            bn.running_mean.copy_(mean.cpu().double()); bn.running_var.copy_(var.cpu().double())
            ref = torch.relu(bn(conv(x.cpu().double())) + res.cpu().double().view(n, h, w, cout).permute(0, 3, 1, 2))
        out, ys = f32_out(m, cout), slice_out(m, cout)
        ok(lib.dmc_x3s_conv_bn_eval(P(xs), P(wf), P(stats), P(gamma), P(beta), P(res), P(out), P(ys), 0, 1, n, h, w, cin, cout, ops._stream()),
           "dmc_x3s_conv_bn_eval")
        assert rel_err(out.view(n, h, w, cout).permute(0, 3, 1, 2), ref) < 1e-5
        assert torch.equal(ops.x3s_merge(ys, (n, cout, h, w)), out.view(n, h, w, cout).permute(0, 3, 1, 2))


@pytest.mark.parametrize("shape", X3S_SHAPES, ids=["-".join(map(str, s)) for s in X3S_SHAPES])
def test_x3s_conv_bn_eval_equals_two_passes(shape):
    check_x3s_shape(shape, fp64_case=(shape == (3, 64, 28, 28, 128)))


@pytest.mark.parametrize("cfg", [102, 104, 105, 106])
def test_x3s_conv_bn_eval_obeys_conv_cfg(cfg):
    lib = _lib.load()
    old = lib.dmc_get_option(b"conv_cfg")
    try:
        assert lib.dmc_set_option(b"conv_cfg", cfg) == 0
        check_x3s_shape((6, 64, 14, 14, 128))
    finally:
        assert lib.dmc_set_option(b"conv_cfg", old) == 0


# ---------------------------------------------------------------------------------------------------------------------
# 2. dmc_x3q_conv_bn_eval, bit for bit
# ---------------------------------------------------------------------------------------------------------------------
X3Q_SHAPES = [(1, 64, 8, 8, 64), (3, 64, 20, 12, 64), (5, 128, 6, 10, 192), (2, 64, 2, 2, 64), (6, 64, 56, 56, 128)]


@pytest.mark.parametrize("shape", X3Q_SHAPES, ids=["-".join(map(str, s)) for s in X3Q_SHAPES])
def test_x3q_conv_bn_eval_equals_two_passes(shape):
    check_x3q_shape(shape)


@pytest.mark.parametrize("cfg", [201, 202, 203])
@pytest.mark.parametrize("shape", [(3, 64, 20, 12, 64), (6, 64, 56, 56, 128)], ids=["3-64-20-12-64", "6-64-56-56-128"])
def test_x3q_conv_bn_eval_obeys_conv_cfg(shape, cfg):
    """Every kernel variant of the pair (256-pixel tiles / 128-pixel tiles of 32 x 32 wave tiles / two workgroups per CU: the one
    the 250-frame evaluator batch takes) by option, as tests/test_x3q_gpu.py does for the training kernel."""
    lib = _lib.load()
    old = lib.dmc_get_option(b"conv_cfg")
    try:
        assert lib.dmc_set_option(b"conv_cfg", cfg) == 0
        check_x3q_shape(shape)
    finally:
        assert lib.dmc_set_option(b"conv_cfg", old) == 0


def check_x3q_shape(shape):
    n, cin, h, w, cout = shape
    oh, ow = h // 2, w // 2
    mq = n * oh * ow
    lib = _lib.load()
    assert lib.dmc_x3q_supported(n, oh, ow, cin, cout)
    x = rnd(521, (n, cin, h, w)).to(DEV).contiguous(memory_format=CL)
    w3 = rnd(522, (cout, cin, 3, 3), 0.1).to(DEV).contiguous(memory_format=CL)
    w1 = rnd(523, (cout, cin, 1, 1), 0.2).to(DEV).contiguous(memory_format=CL)
    xq = ops.x3q_split(x)
    wf, _ = ops.x3q_pack_weights(w3, w1, forward=True, transposed=False)
    st3, g3, b3, mean3, var3 = bn_params(530, cout, DEV)
    st1, g1, b1, mean1, var1 = bn_params(540, cout, DEV)
    y3, y1 = torch.empty((mq, cout), dtype=torch.float32, device=DEV), torch.empty((mq, cout), dtype=torch.float32, device=DEV)
    ok(lib.dmc_x3q_conv_fwd(P(xq), P(wf), P(y3), P(y1), None, None, 0, n, oh, ow, cin, cout, ops._stream()), "dmc_x3q_conv_fwd")
    if cout & (cout - 1) == 0:
        want1 = f32_out(mq, cout)
        ok(lib.dmc_bn_apply_act_nhwc(P(y1), None, P(g1), P(b1), P(st1), P(want1), None, mq, cout, 0, ops._stream()), "dmc_bn_apply_act_nhwc")
    else:                # (the same expression on 64-channel column blocks: bn_two_pass)
        want1, _ = bn_two_pass(y1, None, g1, b1, st1, 0, 1, 0)
    for f32, sl in ((1, 0), (0, 1), (1, 1)):
        want3, want_ys = bn_two_pass(y3, None, g3, b3, st3, 1, f32, sl)
        out3, ys3, out1 = (f32_out(mq, cout) if f32 else None), (slice_out(mq, cout) if sl else None), f32_out(mq, cout)
        ok(lib.dmc_x3q_conv_bn_eval(P(xq), P(wf), P(st3), P(g3), P(b3), P(st1), P(g1), P(b1), P(out3), P(ys3), P(out1), n, oh, ow, cin, cout,
                                    ops._stream()), "dmc_x3q_conv_bn_eval")
        assert torch.equal(out1, want1), (shape, f32, sl)
        if f32:
            assert torch.equal(out3, want3), (shape, f32, sl)
        if sl:
            assert torch.equal(ys3, want_ys), (shape, f32, sl)
    if shape == (3, 64, 20, 12, 64):      # against the stock modules in fp64
        xd = x.cpu().double()
        ref3 = torch.nn.functional.conv2d(xd, w3.cpu().double(), None, 2, 1)
        ref1 = torch.nn.functional.conv2d(xd, w1.cpu().double(), None, 2, 0)
        bn = lambda t, g, b, mu, v: (t - mu.cpu().double().view(1, -1, 1, 1)) / torch.sqrt(v.cpu().double().view(1, -1, 1, 1) + EPS) \
            * g.cpu().double().view(1, -1, 1, 1) + b.cpu().double().view(1, -1, 1, 1)
        nchw = lambda t: t.view(n, oh, ow, cout).permute(0, 3, 1, 2)
        assert rel_err(nchw(out3), torch.relu(bn(ref3, g3, b3, mean3, var3))) < 1e-5
        assert rel_err(nchw(out1), bn(ref1, g1, b1, mean1, var1)) < 1e-5


# ---------------------------------------------------------------------------------------------------------------------
# 3. / 4. units
# ---------------------------------------------------------------------------------------------------------------------
def seeded_unit(cin, planes, stride, seed):
    u = resnet.ResidualUnit("basic", cin, planes, stride)
    O.seeded_state_fill(u, seed)
    return u.eval()


def fp64_of(*units):
    return torch.nn.Sequential(*[copy.deepcopy(u).cpu().double().eval() for u in units])


class Recorder(object):
    """A stand-in for the loaded library that records the name of every entry point called through it."""

    def __init__(self, lib):
        self._lib, self.calls = lib, []

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if not name.startswith("dmc_"):
            return fn

        def call(*args):
            self.calls.append(name)
            return fn(*args)
        return call


def record_calls(monkeypatch):
    rec = Recorder(_lib.load())
    monkeypatch.setattr(_lib, "load", lambda: rec)
    return rec


def test_identity_unit_fused_equals_two_pass(monkeypatch):
    monkeypatch.setattr(resnet, "OWN_CONV", True)
    u = seeded_unit(64, 64, 1, 601).to(DEV).to(memory_format=CL)
    x = rnd(602, (3, 64, 14, 14))
    xg = x.to(DEV).contiguous(memory_format=CL)
    with torch.no_grad():
        ref = fp64_of(u)(x.double())
        monkeypatch.setattr(resnet, "EVAL_FUSED", True)
        rec = record_calls(monkeypatch)
        on = u(xg)
        assert rec.calls.count("dmc_x3s_conv_bn_eval") == 2 and "dmc_bn_apply_act_x3s" not in rec.calls and "dmc_x3s_conv_fwd" not in rec.calls
        monkeypatch.setattr(resnet, "EVAL_FUSED", False)
        del rec.calls[:]
        off = u(xg)
        assert "dmc_x3s_conv_bn_eval" not in rec.calls and rec.calls.count("dmc_x3s_conv_fwd") == 2
    assert ops.f32_valid(on) and torch.equal(on, off)
    assert rel_err(on, ref) < 1e-5 and rel_err(off, ref) < 1e-5


def test_stride2_block_reads_s2d_slices(monkeypatch):
    monkeypatch.setattr(resnet, "OWN_CONV", True)
    monkeypatch.setattr(resnet, "EVAL_FUSED", True)
    monkeypatch.setattr(resnet, "KEEP_F32_OUTPUTS", False)
    u1, u2 = seeded_unit(64, 64, 1, 611).to(DEV).to(memory_format=CL), seeded_unit(64, 128, 2, 612).to(DEV).to(memory_format=CL)
    u1.next_conv[0], u1.next_identity[0], u1.next_unit[0] = u2.conv1, False, u2          # as ResNet.__init__ wires the chain
    x = rnd(613, (2, 64, 28, 28))
    xg = x.to(DEV).contiguous(memory_format=CL)
    with torch.no_grad():
        ref = fp64_of(u1, u2)(x.double())
        rec = record_calls(monkeypatch)
        mid = u1(xg)
        assert ops.x3q_of(mid) is not None and not ops.f32_valid(mid)
        out = u2(mid)
        assert rec.calls.count("dmc_x3q_conv_bn_eval") == 1 and rec.calls.count("dmc_x3s_conv_bn_eval") == 3
        assert "dmc_x3q_split" not in rec.calls and "dmc_conv_nhwc_fwd" not in rec.calls
        assert rel_err(out, ref) < 1e-5
        handle = u1.register_forward_hook(lambda mod, inp, res: None)      # somebody may read the fp32 form: it is written
        try:
            mid2 = u1(xg)
        finally:
            handle.remove()
        assert ops.f32_valid(mid2) and ops.x3q_of(mid2) is None
        assert torch.equal(ops.x3q_merge(ops.x3q_of(mid), tuple(mid.shape)), mid2)
        assert torch.equal(u2(mid2), out)


# ---------------------------------------------------------------------------------------------------------------------
# 5. the whole classifier
# ---------------------------------------------------------------------------------------------------------------------
def test_whole_model_eval_routes(monkeypatch):
    from dmcnet_amd import driver, evaluate
    monkeypatch.setattr(resnet, "OWN_CONV", True)
    kw = dict(base_model="resnet18", use_databn=0, gen_flow_or_delta=1, arch_estimator="DenseNetTiny")
    o = O.seeded_state_fill(O.OracleModel(51, 3, "mv", **kw), 621).eval()
    m = dmcnet_amd.Model(51, 3, "mv", **kw)
    m.load_state_dict(o.state_dict())
    m.to(DEV).eval()
    flow, mv, res, tgt = O.synthetic_batch(seed=622, batch=2, num_segments=3, num_class=51)
    with torch.no_grad():
        ref = o(mv, res)[0].view(2, 3, 51).mean(1).numpy()
    stock = []
    orig = torch.nn.Conv2d._conv_forward
    monkeypatch.setattr(torch.nn.Conv2d, "_conv_forward", lambda self, x, w, b: (stock.append(tuple(w.shape)), orig(self, x, w, b))[1])
    monkeypatch.setattr(resnet, "EVAL_FUSED", False)
    off = evaluate.forward_video(m, mv.to(DEV), res.to(DEV), 3, 1)
    monkeypatch.setattr(resnet, "EVAL_FUSED", True)
    rec = record_calls(monkeypatch)
    on = evaluate.forward_video(m, mv.to(DEV), res.to(DEV), 3, 1)
    calls = list(rec.calls)
    assert rel_err(torch.from_numpy(on), ref) < 1e-4 and rel_err(torch.from_numpy(off), ref) < 1e-4
    assert calls.count("dmc_x3s_conv_bn_eval") == 13 and calls.count("dmc_x3q_conv_bn_eval") == 3, calls
    for name in ("dmc_x3s_conv_fwd", "dmc_x3q_conv_fwd", "dmc_conv_nhwc_fwd", "dmc_bn_apply_act_x3s"):
        assert name not in calls, name
    assert stock == [], stock
    val = driver.validate([(flow, mv, res, tgt)], m, 3, 1.0, 10.0, DEV, log=None)
    assert np.isfinite(val["loss"]) and 0.0 <= val["top1"] <= 100.0 and stock == []


# ---------------------------------------------------------------------------------------------------------------------
# 6. refusals: non-zero before any launch, outputs untouched
# ---------------------------------------------------------------------------------------------------------------------
def test_refusals_write_nothing():
    lib = _lib.load()
    n, h, w, c = 2, 8, 8, 64
    m = n * h * w
    buf = torch.zeros(1 << 20, dtype=U8, device=DEV)                      # any valid input pointer: nothing is launched
    y, ys, y1 = slice_out(m, c), slice_out(m, c), slice_out(m, c)
    p, s = P(buf), ops._stream()
    x3s = [
        ("xs", lambda: lib.dmc_x3s_conv_bn_eval(None, p, p, p, p, None, P(y), P(ys), 0, 1, n, h, w, c, c, s)),
        ("wpack", lambda: lib.dmc_x3s_conv_bn_eval(p, None, p, p, p, None, P(y), P(ys), 0, 1, n, h, w, c, c, s)),
        ("stats", lambda: lib.dmc_x3s_conv_bn_eval(p, p, None, p, p, None, P(y), P(ys), 0, 1, n, h, w, c, c, s)),
        ("gamma", lambda: lib.dmc_x3s_conv_bn_eval(p, p, p, None, p, None, P(y), P(ys), 0, 1, n, h, w, c, c, s)),
        ("beta", lambda: lib.dmc_x3s_conv_bn_eval(p, p, p, p, None, None, P(y), P(ys), 0, 1, n, h, w, c, c, s)),
        ("no output", lambda: lib.dmc_x3s_conv_bn_eval(p, p, p, p, p, None, None, None, 0, 1, n, h, w, c, c, s)),
        ("s2d odd H", lambda: lib.dmc_x3s_conv_bn_eval(p, p, p, p, p, None, P(y), P(ys), 1, 1, n, 7, w, c, c, s)),
        ("s2d odd W", lambda: lib.dmc_x3s_conv_bn_eval(p, p, p, p, p, None, P(y), P(ys), 1, 1, n, h, 7, c, c, s)),
        ("Cin", lambda: lib.dmc_x3s_conv_bn_eval(p, p, p, p, p, None, P(y), P(ys), 0, 1, n, h, w, 32, c, s)),
        ("Cout", lambda: lib.dmc_x3s_conv_bn_eval(p, p, p, p, p, None, P(y), P(ys), 0, 1, n, h, w, c, 32, s)),
    ]
    oh, ow = h // 2, w // 2
    x3q = [
        ("xq", lambda: lib.dmc_x3q_conv_bn_eval(None, p, p, p, p, p, p, p, P(y), P(ys), P(y1), n, oh, ow, c, c, s)),
        ("wpack", lambda: lib.dmc_x3q_conv_bn_eval(p, None, p, p, p, p, p, p, P(y), P(ys), P(y1), n, oh, ow, c, c, s)),
        ("stats3", lambda: lib.dmc_x3q_conv_bn_eval(p, p, None, p, p, p, p, p, P(y), P(ys), P(y1), n, oh, ow, c, c, s)),
        ("gamma3", lambda: lib.dmc_x3q_conv_bn_eval(p, p, p, None, p, p, p, p, P(y), P(ys), P(y1), n, oh, ow, c, c, s)),
        ("beta3", lambda: lib.dmc_x3q_conv_bn_eval(p, p, p, p, None, p, p, p, P(y), P(ys), P(y1), n, oh, ow, c, c, s)),
        ("stats1", lambda: lib.dmc_x3q_conv_bn_eval(p, p, p, p, p, None, p, p, P(y), P(ys), P(y1), n, oh, ow, c, c, s)),
        ("gamma1", lambda: lib.dmc_x3q_conv_bn_eval(p, p, p, p, p, p, None, p, P(y), P(ys), P(y1), n, oh, ow, c, c, s)),
        ("beta1", lambda: lib.dmc_x3q_conv_bn_eval(p, p, p, p, p, p, p, None, P(y), P(ys), P(y1), n, oh, ow, c, c, s)),
        ("y1", lambda: lib.dmc_x3q_conv_bn_eval(p, p, p, p, p, p, p, p, P(y), P(ys), None, n, oh, ow, c, c, s)),
        ("no main output", lambda: lib.dmc_x3q_conv_bn_eval(p, p, p, p, p, p, p, p, None, None, P(y1), n, oh, ow, c, c, s)),
        ("Cin", lambda: lib.dmc_x3q_conv_bn_eval(p, p, p, p, p, p, p, p, P(y), P(ys), P(y1), n, oh, ow, 32, c, s)),
        ("Cout", lambda: lib.dmc_x3q_conv_bn_eval(p, p, p, p, p, p, p, p, P(y), P(ys), P(y1), n, oh, ow, c, 96, s)),
    ]
    for entry, cases in (("dmc_x3s_conv_bn_eval", x3s), ("dmc_x3q_conv_bn_eval", x3q)):
        for what, call in cases:
            assert call() != 0, (entry, what)
            assert entry.encode() in lib.dmc_last_error(), (entry, what)
    torch.cuda.synchronize()
    for t in (y, ys, y1):
        assert bool((t == 0xFF).all())


# ---------------------------------------------------------------------------------------------------------------------
# 7. memory contract: both entry points in guarded arenas (tests/abi_arena.py); check = bit equality with the ops wrapper
# ---------------------------------------------------------------------------------------------------------------------
def _bn_on(arena, seed, c):
    """The BatchNorm's tensors, the statistics built on the arena's device exactly as ops._bn_eval_stats builds them."""
    return bn_params(seed, c, arena.device)


def x3s_eval_case(shape, f32, sl, s2d, with_res, relu):
    n, cin, h, w, cout = shape
    m = n * h * w

    def fn(a):
        lib = _lib.load()
        x = a.inp("x", abi_cases.nhwc(rnd(701, (n, cin, h, w))))
        xs = a.out("xs", nbytes=lib.dmc_x3s_slices_bytes(m, cin), dtype=U8)
        a.call("dmc_x3s_split", x, xs, m, cin)
        wf = a.out("wpack_f", nbytes=lib.dmc_x3s_wpack_bytes(cin, cout), dtype=U8)
        a.call("dmc_x3s_pack_weights", a.inp("w", abi_cases.nhwc(rnd(702, (cout, cin, 3, 3), 0.1))), wf, None, cin, cout)
        stats, gamma, beta, _, _ = _bn_on(a, 710, cout)
        res = a.inp("residual", rnd(703, (m, cout))) if with_res else None
        y = a.out("y", (m, cout)) if f32 else None
        ys = a.out("ys", nbytes=lib.dmc_x3s_slices_bytes(m, cout), dtype=U8) if sl else None
        a.call("dmc_x3s_conv_bn_eval", xs, wf, a.inp("stats", stats), a.inp("gamma", gamma), a.inp("beta", beta), res, y, ys, s2d, relu,
               n, h, w, cin, cout)

    def check(bufs):
        conv = torch.nn.Conv2d(cin, cout, 3, padding=1, bias=False).to(DEV).to(memory_format=CL)
        bn = torch.nn.BatchNorm2d(cout, eps=EPS).to(DEV).eval()
        _, gamma, beta, mean, var = bn_params(710, cout, DEV)
        with torch.no_grad():
            conv.weight.copy_(rnd(702, (cout, cin, 3, 3), 0.1)); bn.weight.copy_(gamma); bn.bias.copy_(beta)
            bn.running_mean.copy_(mean); bn.running_var.copy_(var)
            x = rnd(701, (n, cin, h, w)).to(DEV).contiguous(memory_format=CL)
            res = rnd(703, (m, cout)).to(DEV).view(n, h, w, cout).permute(0, 3, 1, 2) if with_res else None
            out = ops.conv_bn_act_eval(x, conv, bn, res, bool(relu), want_f32=bool(f32), want_slices=bool(sl), s2d=bool(s2d))
        if f32:
            assert abi_cases.same(bufs["y"], abi_cases.nhwc(out))
        if sl:
            assert torch.equal(bufs["ys"].u8, ops.x3q_of(out) if s2d else ops.x3s_of(out))
    return fn, check


def x3q_eval_case(shape, want_slices):
    n, cin, h, w, cout = shape
    oh, ow = h // 2, w // 2
    mq = n * oh * ow

    def fn(a):
        lib = _lib.load()
        x = a.inp("x", abi_cases.nhwc(rnd(721, (n, cin, h, w))))
        xq = a.out("xq", nbytes=lib.dmc_x3s_slices_bytes(n * h * w, cin), dtype=U8)
        a.call("dmc_x3q_split", x, xq, n, h, w, cin)
        wf = a.out("wpack_f", nbytes=lib.dmc_x3q_wpack_bytes(cin, cout), dtype=U8)
        a.call("dmc_x3q_pack_weights", a.inp("w3", abi_cases.nhwc(rnd(722, (cout, cin, 3, 3), 0.1))), a.inp("w1", rnd(723, (cout, cin), 0.2)), wf, None,
               cin, cout)
        st3, g3, b3, _, _ = _bn_on(a, 730, cout)
        st1, g1, b1, _, _ = _bn_on(a, 740, cout)
        y3 = None if want_slices else a.out("y3", (mq, cout))
        ys3 = a.out("ys3", nbytes=lib.dmc_x3s_slices_bytes(mq, cout), dtype=U8) if want_slices else None
        a.call("dmc_x3q_conv_bn_eval", xq, wf, a.inp("stats3", st3), a.inp("gamma3", g3), a.inp("beta3", b3), a.inp("stats1", st1),
               a.inp("gamma1", g1), a.inp("beta1", b1), y3, ys3, a.out("y1", (mq, cout)), n, oh, ow, cin, cout)

    def check(bufs):
        u = resnet.ResidualUnit("basic", cin, cout, 2).to(DEV).to(memory_format=CL).eval()
        with torch.no_grad():
            u.conv1.weight.copy_(rnd(722, (cout, cin, 3, 3), 0.1)); u.downsample[0].weight.copy_(rnd(723, (cout, cin), 0.2).view(cout, cin, 1, 1))
            for bn, seed in ((u.bn1, 730), (u.downsample[1], 740)):
                _, g, b, mean, var = bn_params(seed, cout, DEV)
                bn.weight.copy_(g); bn.bias.copy_(b); bn.running_mean.copy_(mean); bn.running_var.copy_(var)
            x = rnd(721, (n, cin, h, w)).to(DEV).contiguous(memory_format=CL)
            assert ops.s2_pair_eval_usable(tuple(x.shape), u)
            out3, out1 = ops.conv_bn_s2_pair_eval(x, u, want_slices)
        assert abi_cases.same(bufs["y1"], abi_cases.nhwc(out1))
        if want_slices:
            assert torch.equal(bufs["ys3"].u8, ops.x3s_of(out3))
        else:
            assert abi_cases.same(bufs["y3"], abi_cases.nhwc(out3))
    return fn, check


def refused_case(a):        # a space-to-depth result of a 7 x 7 map: refused, nothing written
    lib = _lib.load()
    n, c, h, w = 1, 64, 7, 7
    m = n * h * w
    stats, gamma, beta, _, _ = _bn_on(a, 752, c)
    a.call("dmc_x3s_conv_bn_eval", a.inp("xs", torch.zeros(lib.dmc_x3s_slices_bytes(m, c), dtype=U8)),
           a.inp("wpack_f", torch.zeros(lib.dmc_x3s_wpack_bytes(c, c), dtype=U8)), a.inp("stats", stats), a.inp("gamma", gamma),
           a.inp("beta", beta), None, a.out("y", (m, c)), a.out("ys", nbytes=lib.dmc_x3s_slices_bytes(m, c), dtype=U8), 1, 1, n, h, w, c, c)


ARENA_CASES = []
_X3S_COVERS = ["dmc_x3s_split", "dmc_x3s_pack_weights", "dmc_x3s_conv_bn_eval"]
for _name, _shape, _args in (("slices", (2, 64, 10, 14, 64), (0, 1, 0, 0, 1)), ("s2d", (2, 64, 10, 14, 64), (0, 1, 1, 0, 1)),
                             ("f32-s2d-res", (2, 64, 10, 14, 64), (1, 1, 1, 1, 0)), ("f32-res", (7, 64, 7, 7, 64), (1, 0, 0, 1, 1)),
                             ("f32-slices-res", (1, 128, 14, 14, 64), (1, 1, 0, 1, 1))):
    _fn, _ck = x3s_eval_case(_shape, *_args)
    ARENA_CASES.append(abi_cases.Case(abi_cases.tag("dmc_x3s_conv_bn_eval", *_shape, _name), _X3S_COVERS, _fn, check=_ck, capacity=48 << 20))
for _shape, _sl in (((3, 64, 20, 12, 64), True), ((3, 64, 20, 12, 64), False), ((5, 128, 6, 10, 192), True), ((2, 64, 2, 2, 64), False)):
    _fn, _ck = x3q_eval_case(_shape, _sl)
    ARENA_CASES.append(abi_cases.Case(abi_cases.tag("dmc_x3q_conv_bn_eval", *_shape, "slices" if _sl else "f32"),
                                      ["dmc_x3q_split", "dmc_x3q_pack_weights", "dmc_x3q_conv_bn_eval"], _fn, check=_ck, capacity=48 << 20))
ARENA_CASES.append(abi_cases.Case("dmc_x3s_conv_bn_eval-refused-s2d-odd", ["dmc_x3s_conv_bn_eval"], refused_case,
                                  expect_rc=abi_cases.DMC_E_INVALID, capacity=48 << 20))
_known = {c.id for c in abi_cases.CASES}
abi_cases.CASES.extend(c for c in ARENA_CASES if c.id not in _known)


@pytest.mark.parametrize("case", ARENA_CASES, ids=[c.id for c in ARENA_CASES])
def test_eval_entries_memory_contract(case):
    try:
        bufs = run_case(case.fn, device=DEV, capacity=case.capacity, expect_rc=case.expect_rc)
        if case.check is not None:
            case.check(bufs)
    except RuntimeError as e:
        if "HIP error" in str(e) or "illegal memory access" in str(e):
            # a faulted device serves nothing more: end the session here instead of launching the remaining cases on it
            pytest.exit("GPU fault in %s: %s" % (case.id, str(e).splitlines()[0]), returncode=3)
        raise
