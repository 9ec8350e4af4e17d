"""GPU: ContextNetwork / ContextNetworkAtt in eval mode on the kernels of csrc/ctx_eval.hip.

Per unit, through the C ABI, against the same unit in fp64 stock modules on the CPU (Conv2d(dilation=d, padding=d, bias=False) ->
BatchNorm2d.eval() -> LeakyReLU(0.1)) at the bar of the bf16x3 arithmetic, rel_err < 1e-5 (tests/test_x3s_gpu.py; the fp32 stock
unit sits at 3-4e-7 on these inputs).  BatchNorm parameters and weights are drawn by oracle.dmc_oracle.seeded_state_fill, inputs
are standard normal (about half of the pre-activations are negative: asserted).  The shapes are the smallest at which the kernels
can go wrong -- see UNIT_SHAPES.  Then: batch isolation and run-to-run bit equality; the whole networks against the reference's
own outputs (golden G2) and against fp64; the dispatch (no stock convolution in the forward-only paths, DMC_CTX_EVAL's module
flag, training / autograd untouched); every launching entry point in a guarded arena (tests/abi_arena.py).

What the 1e-5 bar cannot see in the middle unit's bf16x3 loop -- a lost third-order slice product, a defect in one tap or one
16-channel k-block, a wrong slice plane of dmc_ctx_pack_weights -- is held by tests/test_ctx_products_gpu.py: the unit with
identity statistics, exact cases bit for bit through the LeakyReLU and error tap by tap against the CPU emulation."""
import copy
import functools

import numpy as np
import pytest
import torch

import dmcnet_amd
from dmcnet_amd import _lib, model, ops
from oracle import dmc_oracle as O
from tests import abi_cases
from tests.abi_arena import run_case

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U8 = torch.uint8
SLOPE = 0.1


def rnd(seed, shape, scale=1.0):
    return torch.from_numpy((np.random.RandomState(seed).standard_normal(shape) * scale).astype(np.float32))


def rel_err(a, b):
    a, b = a.detach().double().cpu(), torch.as_tensor(b).detach().double().cpu()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))


def P(t):
    return _lib.ptr(t)


def ok(rc, what):
    _lib.check(rc, what)


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def nchw(t):
    return t.permute(0, 3, 1, 2)


@functools.lru_cache(maxsize=None)
def stock_unit(cin, cout, d, seed):
    u = torch.nn.Sequential(torch.nn.Conv2d(cin, cout, 3, 1, d, d, bias=False), torch.nn.BatchNorm2d(cout), torch.nn.LeakyReLU(SLOPE))
    return O.seeded_state_fill(u, seed).eval()


def bn_tensors(bn, device):
    """(stats, gamma, beta) as ops._bn_eval_stats builds them, on ``device``."""
    bn = copy.deepcopy(bn).to(device)
    return ops._bn_eval_stats(bn).detach(), bn.weight.detach().contiguous(), bn.bias.detach().contiguous()


@functools.lru_cache(maxsize=None)
def unit_case(n, h, w, cin, cout, d, seed=801):
    """(x [N,Cin,H,W] fp32 CPU, the unit, its fp64 result, its fp64 pre-activation): computed once per shape, never modified."""
    x = rnd(seed, (n, cin, h, w))
    u = stock_unit(cin, cout, d, seed + 1)
    u64 = copy.deepcopy(u).double()
    with torch.no_grad():
        pre = u64[1](u64[0](x.double()))
        ref = u64[2](pre.clone())
    return x, u, ref, pre


def run_middle(x_nhwc, u, n, h, w, cin, cout, d):
    """dmc_ctx_pack_weights + dmc_ctx_unit_eval on device tensors; returns y [N,H,W,Cout] (NaN-prefilled)."""
    lib = _lib.load()
    wt = nhwc(u[0].weight.detach()).to(DEV)
    wp = torch.full((lib.dmc_ctx_wpack_bytes(cin, cout),), 0xFF, dtype=U8, device=DEV)
    ok(lib.dmc_ctx_pack_weights(P(wt), P(wp), cin, cout, ops._stream()), "dmc_ctx_pack_weights")
    stats, gamma, beta = bn_tensors(u[1], DEV)
    y = torch.full((n, h, w, cout), float("nan"), dtype=torch.float32, device=DEV)
    ok(lib.dmc_ctx_unit_eval(P(x_nhwc), P(wp), P(stats), P(gamma), P(beta), P(y), n, h, w, cin, cout, d, ops._stream()), "dmc_ctx_unit_eval")
    return y


#: (N, H, W, Cin, Cout, d)
UNIT_SHAPES = [
    (1, 20, 37, 32, 128, 2),      # ragged width; a pixel count no tile divides
    (3, 33, 18, 128, 128, 4),     # tiles span frame boundaries
    (2, 17, 40, 128, 96, 8),      # H < 2d+1: no pixel has both vertical neighbours; Cout 96
    (2, 40, 12, 96, 64, 16),      # W < d: every horizontal side tap is outside the frame (a linearised offset would land in the next row)
    (1, 35, 35, 96, 64, 16),      # the smallest map on which interior pixels see all nine taps at d = 16
    (2, 9, 21, 96, 64, 1),        # the down-sampled plan's unit 5
    (2, 16, 24, 64, 32, 1),       # Cout 32
]
IDS = ["-".join(map(str, s)) for s in UNIT_SHAPES]


@pytest.mark.parametrize("shape", UNIT_SHAPES, ids=IDS)
def test_middle_unit_vs_fp64(shape):
    n, h, w, cin, cout, d = shape
    assert _lib.load().dmc_ctx_unit_supported(*shape) == 1
    x, u, ref, pre = unit_case(*shape)
    neg = float((pre < 0).double().mean())
    assert 0.3 < neg < 0.7, neg                                    # both LeakyReLU branches carry weight
    xg = nhwc(x).to(DEV)
    y = run_middle(xg, u, *shape)
    e = rel_err(nchw(y), ref)
    print("ctx unit %s: rel_err %.3e (negative pre-activations %.2f)" % (shape, e, neg))
    assert not bool(torch.isnan(y).any())
    assert e < 1e-5, e
    assert torch.equal(run_middle(xg, u, *shape), y)               # run to run


def run_first(x, u, n, h, w):
    lib = _lib.load()
    stats, gamma, beta = bn_tensors(u[1], DEV)
    y = torch.full((n, h, w, 32), float("nan"), dtype=torch.float32, device=DEV)
    ok(lib.dmc_ctx_first_eval(P(x), P(u[0].weight.detach().contiguous().to(DEV)), P(stats), P(gamma), P(beta), P(y), n, h, w, ops._stream()),
       "dmc_ctx_first_eval")
    return y


def test_first_unit_vs_fp64():
    n, h, w = 2, 19, 37
    x, u, ref, pre = unit_case(n, h, w, 5, 32, 1)
    neg = float((pre < 0).double().mean())
    assert 0.3 < neg < 0.7, neg
    xg = x.to(DEV)
    y = run_first(xg, u, n, h, w)
    e = rel_err(nchw(y), ref)
    print("ctx first unit: rel_err %.3e" % e)
    assert e < 1e-5, e
    assert torch.equal(run_first(xg, u, n, h, w), y)


def run_heads(x_nhwc, uf, ua, n, h, w):
    lib = _lib.load()
    flow = torch.full((n, 2, h, w), float("nan"), dtype=torch.float32, device=DEV)
    att = torch.full((n, 2, h, w), float("nan"), dtype=torch.float32, device=DEV) if ua is not None else None
    args = []
    for u in (uf, ua):
        if u is None:
            args += [None, None, None, None]
        else:
            args += [nhwc(u[0].weight.detach()).to(DEV)] + list(bn_tensors(u[1], DEV))
    ok(lib.dmc_ctx_heads_eval(P(x_nhwc), *[P(t) for t in args], P(flow), P(att), n, h, w, ops._stream()), "dmc_ctx_heads_eval")
    return flow, att


HEADS = (3, 19, 37)


@functools.lru_cache(maxsize=None)
def heads_case_data():
    """(x, flow unit, attention unit, fp64 flow, fp64 attention BEFORE its ReLU) of the heads' shape; both heads read the same x."""
    n, h, w = HEADS
    x, uf, ref_f, pre_f = unit_case(n, h, w, 32, 2, 1)
    ua = stock_unit(32, 2, 1, 812)
    with torch.no_grad():
        ref_a = copy.deepcopy(ua).double()(x.double())
    return x, uf, ua, ref_f, ref_a


@pytest.mark.parametrize("two", [False, True], ids=["flow", "flow+att"])
def test_heads_vs_fp64(two):
    n, h, w = HEADS
    x, uf, ua, ref_f, ref_a = heads_case_data()
    assert 0.2 < float((ref_f < 0).double().mean()) < 0.8 and 0.2 < float((ref_a < 0).double().mean()) < 0.8
    xg = nhwc(x).to(DEV)
    flow, att = run_heads(xg, uf, ua if two else None, n, h, w)
    e = rel_err(flow, ref_f)
    print("ctx heads: flow rel_err %.3e" % e)
    assert e < 1e-5, e
    flow2, att2 = run_heads(xg, uf, ua if two else None, n, h, w)
    assert torch.equal(flow, flow2)
    if two:
        ea = rel_err(att, torch.relu(ref_a))
        print("ctx heads: att rel_err %.3e" % ea)
        assert ea < 1e-5, ea
        a = att.cpu()
        assert bool((a >= 0).all())                                # never negative
        assert bool((a[ref_a < -1e-6] == 0).all())                 # exactly zero wherever the fp64 value in front of the ReLU is below -1e-6
        assert torch.equal(att, att2)
    else:
        assert att is None


# ---------------------------------------------------------------------------------------------------------------------
# isolation
# ---------------------------------------------------------------------------------------------------------------------
def test_frame_result_is_independent_of_its_batch():
    shape = (3, 33, 18, 128, 128, 4)
    n, h, w, cin, cout, d = shape
    x, u, _, _ = unit_case(*shape)
    xg = nhwc(x).to(DEV)
    y = run_middle(xg, u, *shape)
    alone = run_middle(xg[1:2].contiguous(), u, 1, h, w, cin, cout, d)
    assert torch.equal(y[1:2], alone)


def test_frame_result_ignores_its_neighbour_frame():
    shape = (2, 40, 12, 96, 64, 16)
    n, h, w, cin, cout, d = shape
    x, u, _, _ = unit_case(*shape)
    xg = nhwc(x).to(DEV)
    y = run_middle(xg, u, *shape)
    xb = xg.clone()
    xb[0] = nhwc(rnd(899, (1, cin, h, w), 1e6)).to(DEV)[0]
    yb = run_middle(xb, u, *shape)
    assert torch.equal(y[1], yb[1])
    assert not torch.equal(y[0], yb[0])


def test_byte_offsets_past_4_gib():
    """42 frames of 448 x 448 are 8.4 M pixels: the 128-channel tensor is 4.3 GB, so byte offsets pass 2^32 while N H W 128 stays
    below 2^31 (one launch).  First as the OUTPUT (32 -> 128, d = 2), then as the INPUT (128 -> 32, d = 16): frames at both ends
    and in the middle equal the same frame evaluated alone, bit for bit (a truncated offset lands in another frame), and the last
    frame of the first unit is held to fp64."""
    n, h, w = 42, 448, 448
    assert n * h * w * 128 * 4 > 2 ** 32 and n * h * w * 128 < 2 ** 31
    assert _lib.load().dmc_ctx_unit_supported(n, h, w, 32, 128, 2) == 1 and _lib.load().dmc_ctx_unit_supported(n, h, w, 128, 32, 16) == 1
    g = torch.Generator(device=DEV).manual_seed(77)
    x = torch.randn((n, h, w, 32), generator=g, device=DEV)
    u1, u2 = stock_unit(32, 128, 2, 871), stock_unit(128, 32, 16, 872)
    y = run_middle(x, u1, n, h, w, 32, 128, 2)
    for f in (0, 20, 24, 25, n - 1):                               # the last frame is the one that crosses 2^32 bytes
        assert torch.equal(y[f:f + 1], run_middle(x[f:f + 1].contiguous(), u1, 1, h, w, 32, 128, 2)), f
    with torch.no_grad():
        ref = copy.deepcopy(u1).double()(nchw(x[n - 1:n]).cpu().double())
    assert rel_err(nchw(y[n - 1:n]), ref) < 1e-5
    z = run_middle(y, u2, n, h, w, 128, 32, 16)
    for f in (0, 24, 25, n - 1):
        assert torch.equal(z[f:f + 1], run_middle(y[f:f + 1].contiguous(), u2, 1, h, w, 128, 32, 16)), f


# ---------------------------------------------------------------------------------------------------------------------
# whole networks
# ---------------------------------------------------------------------------------------------------------------------
def build_pair(att, ds, seed=26):
    o = O.seeded_state_fill(O.build_estimator("ContextNetwork", ds, att), seed=seed).eval()
    cls = model.ContextNetworkAtt if att else model.ContextNetwork
    m = cls(5, True, ds)
    assert list(m.state_dict().keys()) == list(o.state_dict().keys())
    m.load_state_dict(o.state_dict())
    return o, m.to(DEV).eval()


def as_tuple(r):
    return tuple(r) if isinstance(r, (tuple, list)) else (r,)


def check_chain(att, ds, x):
    o, m = build_pair(att, ds)
    with torch.no_grad():
        assert ops.context_eval_supported(m, x.to(DEV))
        got = as_tuple(m(x.to(DEV)))
        ref32 = as_tuple(o(x))
        ref64 = as_tuple(copy.deepcopy(o).double()(x.double()))
    assert len(got) == len(ref64) == (2 if att else 1)
    for g, r32, r64 in zip(got, ref32, ref64):
        assert tuple(g.shape) == tuple(r64.shape)
        e = float((g.double().cpu() - r64).abs().max())
        e_ref = float((r32.double() - r64).abs().max())
        top = float(r64.abs().max())
        print("ctx chain att=%d ds=%d %s: e %.3e e_ref %.3e max|y| %.3e" % (att, ds, tuple(x.shape), e, e_ref, top))
        assert e <= max(4 * e_ref, 2e-5 * top), (e, e_ref, top)
    return got


@pytest.mark.parametrize("att", [0, 1])
def test_whole_network_vs_reference_golden(att, golden):
    g = golden("g2_model_eval")
    got = check_chain(att, 0, rnd(24, (2, 5, 48, 48)))
    keys = ["est_ContextNetworkAtt_flow", "est_ContextNetworkAtt_att"] if att else ["est_ContextNetwork"]
    for t, k in zip(got, keys):
        np.testing.assert_allclose(t.cpu().numpy(), g[k], rtol=1e-4, atol=1e-5)
    if att:
        assert bool((got[1] >= 0).all())


@pytest.mark.parametrize("att", [0, 1])
@pytest.mark.parametrize("ds,shape", [(16, (3, 5, 14, 14)), (0, (1, 5, 20, 37)), (0, (3, 5, 33, 18))], ids=["ds16-14x14", "20x37", "33x18"])
def test_whole_network_vs_fp64(att, ds, shape):
    check_chain(att, ds, rnd(31, shape))


def test_chunked_batches_equal_one_launch(monkeypatch):
    """ops.context_eval walks context_eval_chunks: with a small index limit the batch is evaluated in several frame ranges, and
    -- frames being independent of their batch -- the result is bit-identical."""
    o, m = build_pair(1, 0)
    x = rnd(41, (5, 5, 12, 10)).to(DEV)
    with torch.no_grad():
        one = m(x)
        monkeypatch.setattr(ops, "_CTX_MAX_INDEX", 2 * 12 * 10 * 128 + 1)
        assert ops.context_eval_chunks(5, 12, 10) == [(0, 2), (2, 4), (4, 5)]
        many = m(x)
    assert torch.equal(one[0], many[0]) and torch.equal(one[1], many[1])


# ---------------------------------------------------------------------------------------------------------------------
# dispatch
# ---------------------------------------------------------------------------------------------------------------------
class Recorder(object):
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


@pytest.mark.parametrize("att", [0, 1])
def test_forward_only_paths_run_no_stock_convolution(att, monkeypatch):
    from dmcnet_amd import evaluate
    kw = dict(base_model="resnet18", use_databn=0, arch_estimator="ContextNetwork", att=att)
    o = O.seeded_state_fill(O.OracleModel(51, 3, "mv", **kw), 71).eval()
    m = dmcnet_amd.Model(51, 3, "mv", **kw)
    m.load_state_dict(o.state_dict())
    m.to(DEV).eval()
    _, mv, res, _ = O.synthetic_batch(seed=72, batch=2, num_segments=3, num_class=51)
    with torch.no_grad():
        ref = o(mv, res)[0].view(2, 3, 51).mean(1).numpy()
    stock = []
    orig = torch.nn.Conv2d._conv_forward
    monkeypatch.setattr(torch.nn.Conv2d, "_conv_forward", lambda self, x, w, b: (stock.append(tuple(w.shape)), orig(self, x, w, b))[1])
    monkeypatch.setattr(model, "CTX_EVAL", True)
    rec = Recorder(_lib.load())
    monkeypatch.setattr(_lib, "load", lambda: rec)
    on = evaluate.forward_video(m, mv.to(DEV), res.to(DEV), 3, 1)
    assert stock == [], stock
    assert rec.calls.count("dmc_ctx_first_eval") == 1 and rec.calls.count("dmc_ctx_unit_eval") == 5 and rec.calls.count("dmc_ctx_heads_eval") == 1
    assert rel_err(torch.from_numpy(on), ref) < 1e-4
    monkeypatch.setattr(model, "CTX_EVAL", False)                  # DMC_CTX_EVAL=0
    del rec.calls[:]
    off = evaluate.forward_video(m, mv.to(DEV), res.to(DEV), 3, 1)
    assert len(stock) == (8 if att else 7) and all(s[2:] == (3, 3) for s in stock), stock
    assert not any(c.startswith("dmc_ctx_") for c in rec.calls)
    assert rel_err(torch.from_numpy(off), ref) < 1e-4 and rel_err(torch.from_numpy(on), off) < 1e-4


@pytest.mark.parametrize("att", [0, 1])
def test_training_and_autograd_keep_the_stock_modules(att, monkeypatch):
    _, m = build_pair(att, 0)
    x = rnd(51, (2, 5, 21, 17)).to(DEV)
    r = rnd(52, (2, 2, 21, 17)).to(DEV)
    rec = Recorder(_lib.load())
    monkeypatch.setattr(_lib, "load", lambda: rec)

    def stock_forward(net, inp):
        t = net.conv_context(inp)
        return (net.predict_flow(t), net.predict_att(t)) if att else (t,)

    def grads(net, fwd, train):
        net = copy.deepcopy(net)
        net.train(train)
        xi = x.clone().requires_grad_(True)
        outs = as_tuple(fwd(net, xi))
        sum((t * r).sum() for t in outs).backward()
        return [t.detach() for t in outs] + [xi.grad] + [p.grad for p in net.parameters()] + [b for b in net.buffers()]

    # the stock route must reproduce itself for a bit comparison to mean anything: MIOpen is asked for its deterministic solvers
    monkeypatch.setattr(torch.backends.cudnn, "deterministic", True)
    monkeypatch.setattr(torch.backends.cudnn, "benchmark", False)
    for train in (True, False):                                    # train(): never; eval() with autograd on: never
        b = grads(m, stock_forward, train)
        a = grads(m, lambda net, xi: net(xi), train)
        b2 = grads(m, stock_forward, train)
        assert not any(c.startswith("dmc_ctx_") for c in rec.calls), rec.calls
        assert len(a) == len(b) == len(b2)
        same = [torch.equal(s, t) for s, t in zip(a, b)]
        print("train=%s: forward() == stock per tensor %s; stock == stock %s" % (train, same, [torch.equal(s, t) for s, t in zip(b, b2)]))
        assert all(same), (train, [i for i, q in enumerate(same) if not q])
    m.train()
    with torch.no_grad():                                          # train() without autograd: never either
        assert not ops.context_eval_supported(m, x)
    m.eval()
    with torch.no_grad():
        assert ops.context_eval_supported(m, x)
        assert not ops.context_eval_supported(m, x.double()) and not ops.context_eval_supported(m, x[:, :4])
        m(x)
    assert any(c.startswith("dmc_ctx_") for c in rec.calls)


# ---------------------------------------------------------------------------------------------------------------------
# refusals and the memory contract
# ---------------------------------------------------------------------------------------------------------------------
def test_refused_calls_write_nothing():
    lib = _lib.load()
    buf = torch.zeros(1 << 16, dtype=U8, device=DEV)
    y = torch.full((1 << 16,), 0xFF, dtype=U8, device=DEV)
    p, q, s = P(buf), P(y), ops._stream()
    calls = [("dmc_ctx_unit_eval", lambda: lib.dmc_ctx_unit_eval(p, p, p, p, p, q, 1, 8, 8, 32, 128, 3, s)),
             ("dmc_ctx_unit_eval", lambda: lib.dmc_ctx_unit_eval(p, p, None, p, p, q, 1, 8, 8, 32, 128, 2, s)),
             ("dmc_ctx_unit_eval", lambda: lib.dmc_ctx_unit_eval(p, p, p, p, p, q, 1, 8, 8, 5, 32, 1, s)),
             ("dmc_ctx_pack_weights", lambda: lib.dmc_ctx_pack_weights(p, q, 32, 2, s)),
             ("dmc_ctx_first_eval", lambda: lib.dmc_ctx_first_eval(p, None, p, p, p, q, 1, 8, 8, s)),
             ("dmc_ctx_first_eval", lambda: lib.dmc_ctx_first_eval(p, p, p, p, p, q, 335, 224, 224, s)),
             ("dmc_ctx_heads_eval", lambda: lib.dmc_ctx_heads_eval(p, p, p, p, p, p, p, None, p, q, q, 1, 8, 8, s)),
             ("dmc_ctx_heads_eval", lambda: lib.dmc_ctx_heads_eval(p, p, p, p, p, None, None, None, None, q, q, 1, 8, 8, s))]
    for name, call in calls:
        assert call() == -1, name
        assert name.encode() in lib.dmc_last_error(), name
    torch.cuda.synchronize()
    assert bool((y == 0xFF).all())


def middle_case(shape):
    n, h, w, cin, cout, d = shape

    def fn(a):
        lib = _lib.load()
        x, u, _, _ = unit_case(*shape)
        wp = a.out("wpack", nbytes=lib.dmc_ctx_wpack_bytes(cin, cout), dtype=U8)
        a.call("dmc_ctx_pack_weights", a.inp("w", nhwc(u[0].weight.detach())), wp, cin, cout)
        stats, gamma, beta = bn_tensors(u[1], a.device)
        a.call("dmc_ctx_unit_eval", a.inp("x", nhwc(x)), wp, a.inp("stats", stats), a.inp("gamma", gamma), a.inp("beta", beta),
               a.out("y", (n, h, w, cout)), n, h, w, cin, cout, d)
    return fn


def first_case(a):
    n, h, w = 2, 19, 37
    x, u, _, _ = unit_case(n, h, w, 5, 32, 1)
    stats, gamma, beta = bn_tensors(u[1], a.device)
    a.call("dmc_ctx_first_eval", a.inp("x", x), a.inp("w", u[0].weight.detach()), a.inp("stats", stats), a.inp("gamma", gamma),
           a.inp("beta", beta), a.out("y", (n, h, w, 32)), n, h, w)


def heads_case(two):
    n, h, w = HEADS

    def fn(a):
        x, uf, ua, _, _ = heads_case_data()
        args = [a.inp("x", nhwc(x))]
        for tag_, u in (("flow", uf), ("att", ua if two else None)):
            if u is None:
                args += [None, None, None, None]
                continue
            stats, gamma, beta = bn_tensors(u[1], a.device)
            args += [a.inp("w_" + tag_, nhwc(u[0].weight.detach())), a.inp("stats_" + tag_, stats), a.inp("gamma_" + tag_, gamma),
                     a.inp("beta_" + tag_, beta)]
        args += [a.out("flow", (n, 2, h, w)), a.out("att", (n, 2, h, w)) if two else None]
        a.call("dmc_ctx_heads_eval", *args, n, h, w)
    return fn


def refused_unit_case(a):      # dilation 3: refused, nothing written
    lib = _lib.load()
    n, h, w, cin, cout = 1, 8, 8, 32, 128
    a.call("dmc_ctx_unit_eval", a.inp("x", torch.zeros(n, h, w, cin)), a.inp("wpack", torch.zeros(lib.dmc_ctx_wpack_bytes(cin, cout), dtype=U8)),
           a.inp("stats", torch.ones(2 * cout)), a.inp("gamma", torch.ones(cout)), a.inp("beta", torch.zeros(cout)),
           a.out("y", (n, h, w, cout)), n, h, w, cin, cout, 3)


def refused_heads_case(a):     # an attention output without attention weights: refused, nothing written
    n, h, w = 1, 8, 8
    one = torch.ones(4)
    a.call("dmc_ctx_heads_eval", a.inp("x", torch.zeros(n, h, w, 32)), a.inp("w_flow", torch.zeros(2, 3, 3, 32)), a.inp("stats_flow", one),
           a.inp("gamma_flow", one[:2]), a.inp("beta_flow", one[:2]), None, None, None, None, a.out("flow", (n, 2, h, w)),
           a.out("att", (n, 2, h, w)), n, h, w)


def _middle_check(shape):
    def check(bufs):
        assert rel_err(nchw(bufs["y"].t), unit_case(*shape)[2]) < 1e-5
    return check


def _first_check(bufs):
    assert rel_err(nchw(bufs["y"].t), unit_case(2, 19, 37, 5, 32, 1)[2]) < 1e-5


def _heads_check(two):
    def check(bufs):
        _, _, _, ref_f, ref_a = heads_case_data()
        assert rel_err(bufs["flow"].t, ref_f) < 1e-5
        if two:
            assert rel_err(bufs["att"].t, torch.relu(ref_a)) < 1e-5
    return check


ARENA_CASES = []
for _shape in ((1, 20, 37, 32, 128, 2), (2, 17, 40, 128, 96, 8), (2, 40, 12, 96, 64, 16), (2, 16, 24, 64, 32, 1)):
    ARENA_CASES.append(abi_cases.Case(abi_cases.tag("dmc_ctx_unit_eval", *_shape), ["dmc_ctx_pack_weights", "dmc_ctx_unit_eval"],
                                      middle_case(_shape), check=_middle_check(_shape), capacity=32 << 20))
ARENA_CASES.append(abi_cases.Case("dmc_ctx_first_eval-2-19-37", ["dmc_ctx_first_eval"], first_case, check=_first_check, capacity=32 << 20))
ARENA_CASES.append(abi_cases.Case("dmc_ctx_heads_eval-3-19-37-flow", ["dmc_ctx_heads_eval"], heads_case(False), check=_heads_check(False),
                                  capacity=32 << 20))
ARENA_CASES.append(abi_cases.Case("dmc_ctx_heads_eval-3-19-37-flow-att", ["dmc_ctx_heads_eval"], heads_case(True), check=_heads_check(True),
                                  capacity=32 << 20))
ARENA_CASES.append(abi_cases.Case("dmc_ctx_unit_eval-refused-dilation-3", ["dmc_ctx_unit_eval"], refused_unit_case,
                                  expect_rc=abi_cases.DMC_E_INVALID, capacity=32 << 20))
ARENA_CASES.append(abi_cases.Case("dmc_ctx_heads_eval-refused-att-without-weights", ["dmc_ctx_heads_eval"], refused_heads_case,
                                  expect_rc=abi_cases.DMC_E_INVALID, capacity=32 << 20))
_known = {c.id for c in abi_cases.CASES}
abi_cases.CASES.extend(c for c in ARENA_CASES if c.id not in _known)


@pytest.mark.parametrize("case", ARENA_CASES, ids=[c.id for c in ARENA_CASES])
def test_ctx_entries_memory_contract(case):
    try:
        bufs = run_case(case.fn, device=DEV, capacity=case.capacity, expect_rc=case.expect_rc)
        if case.check is not None:
            case.check(bufs)
    except RuntimeError as e:
        if "HIP error" in str(e) or "illegal memory access" in str(e):
            # a faulted device serves nothing more: end the session here instead of launching the remaining cases on it
            pytest.exit("GPU fault in %s: %s" % (case.id, str(e).splitlines()[0]), returncode=3)
        raise
