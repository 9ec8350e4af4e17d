"""GPU: the dilated convolutions of the ContextNetwork training route (csrc/dconv.hip, ops.dilated_conv, model.CTX_TRAIN).

Through the C ABI, against fp64 stock convolutions on the CPU (F.conv2d(dilation=d, padding=d) and its autograd) at the bar of
the bf16x3 arithmetic, rel_err < 1e-5 (tests/test_x3s_gpu.py): the forward, the data gradient (dmc_dconv_fwd on dy with the
transposed pack, Cin and Cout exchanged) and the weight gradient, each run twice and bit-equal.  The shapes are the smallest at
which the kernels can go wrong -- see SHAPES.  Then: batch independence (also past byte offset 2^32); the autograd op (values,
both gradients, which launches a frozen operand saves, grad_output layouts); the whole networks in train() with model.CTX_TRAIN
on against the stock route on the same device and an fp64 stock copy (outputs, x.grad, every parameter gradient, every
BatchNorm buffer; the worst pair measured on an MI355X is in DESIGN 4.22); the dispatch; every launching entry point in a
guarded arena (tests/abi_arena.py).

The 1e-5 bar on dense Gaussian operands cannot see a lost or mis-paired third-order slice product, a defect confined to one tap or
one 16-channel k-block of the weight panel, a wrong slice plane in the pack or a mirrored tap on the wrong panel of the transposed
pack: tests/test_ctx_products_gpu.py holds these kernels (and the packs, bit for bit) to the six-product bars of
tests/test_x3_products_gpu.py on the SHAPES below."""
import copy
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from dmcnet_amd import _lib, model, ops
from oracle import dmc_oracle as O
from tests import abi_cases
from tests.abi_arena import run_case

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U8 = torch.uint8
CL = torch.channels_last


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
def conv_case(n, h, w, cin, cout, d, seed=901):
    """(x [N,Cin,H,W], weight [Cout,Cin,3,3], dy [N,Cout,H,W]) fp32 on the CPU and the fp64 (y, dx, dw) of the stock convolution:
    computed once per shape, never modified."""
    x, wt, dy = rnd(seed, (n, cin, h, w)), rnd(seed + 1, (cout, cin, 3, 3), 0.05), rnd(seed + 2, (n, cout, h, w))
    x64, w64 = x.double().requires_grad_(True), wt.double().requires_grad_(True)
    y = F.conv2d(x64, w64, None, 1, d, d)
    y.backward(dy.double())
    return x, wt, dy, y.detach(), x64.grad, w64.grad


def pack(w_ohwi, cin, cout, transposed):
    lib = _lib.load()
    wp = torch.full((lib.dmc_dconv_wpack_bytes(cin, cout),), 0xFF, dtype=U8, device=DEV)
    ok(lib.dmc_dconv_pack_weights(P(w_ohwi), P(wp), cin, cout, transposed, ops._stream()), "dmc_dconv_pack_weights")
    return wp


def run_fwd(x_nhwc, w_ohwi, n, h, w, cin, cout, d):
    """y [N,H,W,Cout] (NaN-prefilled) = conv(x) through dmc_dconv_pack_weights + dmc_dconv_fwd."""
    y = torch.full((n, h, w, cout), float("nan"), dtype=torch.float32, device=DEV)
    ok(_lib.load().dmc_dconv_fwd(P(x_nhwc), P(pack(w_ohwi, cin, cout, 0)), P(y), n, h, w, cin, cout, d, ops._stream()), "dmc_dconv_fwd")
    return y


def run_dgrad(dy_nhwc, w_ohwi, n, h, w, cin, cout, d):
    """dx [N,H,W,Cin]: the same entry point on dy with the transposed pack, Cin and Cout exchanged."""
    dx = torch.full((n, h, w, cin), float("nan"), dtype=torch.float32, device=DEV)
    ok(_lib.load().dmc_dconv_fwd(P(dy_nhwc), P(pack(w_ohwi, cin, cout, 1)), P(dx), n, h, w, cout, cin, d, ops._stream()), "dmc_dconv_fwd")
    return dx


def run_wgrad(x_nhwc, dy_nhwc, n, h, w, cin, cout, d):
    """dw [Cout,3,3,Cin] (NaN-prefilled), the workspace at exactly the reported size (0xFF-prefilled)."""
    lib = _lib.load()
    ws = torch.full((lib.dmc_dconv_wgrad_workspace_bytes(n, h, w, cin, cout),), 0xFF, dtype=U8, device=DEV)
    dw = torch.full((cout, 3, 3, cin), float("nan"), dtype=torch.float32, device=DEV)
    ok(lib.dmc_dconv_wgrad(P(x_nhwc), P(dy_nhwc), P(dw), P(ws), n, h, w, cin, cout, d, ops._stream()), "dmc_dconv_wgrad")
    return dw


#: (N, H, W, Cin, Cout, d)
SHAPES = [
    (1, 20, 37, 32, 128, 2),      # ragged width, a pixel count no tile divides; the transposed GEMM has TN = 1
    (3, 33, 18, 128, 128, 4),     # tiles and pixel ranges span frame boundaries
    (2, 17, 40, 128, 96, 8),      # H < 2d+1; 96 as Cout forward and as Cin in the transposed pack
    (2, 40, 12, 96, 64, 16),      # W < d: every horizontal side tap is outside, those six dW taps are exactly 0 and written
    (1, 35, 35, 96, 64, 16),      # the smallest map where interior pixels see all nine taps
    (2, 9, 21, 64, 32, 1),        # TN = 1 forward
    (4, 64, 64, 32, 32, 1),       # 16 k pixels of K: several pixel ranges, fp32 accumulation
]
IDS = ["-".join(map(str, s)) for s in SHAPES]


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_conv_dgrad_wgrad_vs_fp64(shape):
    n, h, w, cin, cout, d = shape
    assert _lib.load().dmc_dconv_supported(*shape) == 1
    x, wt, dy, y64, dx64, dw64 = conv_case(*shape)
    xg, dyg, wg = nhwc(x).to(DEV), nhwc(dy).to(DEV), nhwc(wt).to(DEV)
    y = run_fwd(xg, wg, *shape)
    dx = run_dgrad(dyg, wg, *shape)
    dw = run_wgrad(xg, dyg, *shape)
    e = (rel_err(nchw(y), y64), rel_err(nchw(dx), dx64), rel_err(nchw(dw), dw64))
    print("dconv %s: rel_err forward %.3e, data gradient %.3e, weight gradient %.3e" % ((shape,) + e))
    for t in (y, dx, dw):
        assert not bool(torch.isnan(t).any())
    assert e[0] < 1e-5 and e[1] < 1e-5 and e[2] < 1e-5, e
    if w <= d:                                                     # no pixel has a horizontal neighbour at distance d
        assert bool((dw64[:, :, :, 0] == 0).all()) and bool((dw64[:, :, :, 2] == 0).all())
        assert bool((dw[:, :, 0, :] == 0).all()) and bool((dw[:, :, 2, :] == 0).all())
        assert bool((dw[:, :, 1, :] != 0).any())
    assert torch.equal(run_fwd(xg, wg, *shape), y)                 # run to run
    assert torch.equal(run_dgrad(dyg, wg, *shape), dx)
    assert torch.equal(run_wgrad(xg, dyg, *shape), dw)


def test_several_pixel_ranges_are_in_play():
    """The workspace of the 16 k-pixel shape holds more than one range of partial sums (the reduce kernel adds them in order)."""
    lib = _lib.load()
    assert lib.dmc_dconv_wgrad_workspace_bytes(4, 64, 64, 32, 32) >= 2 * 32 * 32 * 9 * 4
    assert lib.dmc_dconv_wgrad_workspace_bytes(1, 1, 1, 32, 32) == 32 * 32 * 9 * 4


# ---------------------------------------------------------------------------------------------------------------------
# batch independence
# ---------------------------------------------------------------------------------------------------------------------
def test_frame_results_are_independent_of_the_batch():
    shape = (3, 33, 18, 128, 128, 4)
    n, h, w, cin, cout, d = shape
    x, wt, dy, _, _, _ = conv_case(*shape)
    xg, dyg, wg = nhwc(x).to(DEV), nhwc(dy).to(DEV), nhwc(wt).to(DEV)
    y, dx = run_fwd(xg, wg, *shape), run_dgrad(dyg, wg, *shape)
    for f in range(n):
        assert torch.equal(y[f:f + 1], run_fwd(xg[f:f + 1].contiguous(), wg, 1, h, w, cin, cout, d)), f
        assert torch.equal(dx[f:f + 1], run_dgrad(dyg[f:f + 1].contiguous(), wg, 1, h, w, cin, cout, d)), f


def last_frame_only(n, h, w, cin, cout, d, seed):
    """x and dy of n frames, zero except the last frame: (the batch's weight gradient, that frame's own, x)."""
    g = torch.Generator(device=DEV).manual_seed(seed)
    x = torch.zeros((n, h, w, cin), dtype=torch.float32, device=DEV)
    dy = torch.zeros((n, h, w, cout), dtype=torch.float32, device=DEV)
    x[n - 1] = torch.randn((h, w, cin), generator=g, device=DEV)
    dy[n - 1] = torch.randn((h, w, cout), generator=g, device=DEV)
    batch = run_wgrad(x, dy, n, h, w, cin, cout, d)
    alone = run_wgrad(x[n - 1:].contiguous(), dy[n - 1:].contiguous(), 1, h, w, cin, cout, d)
    return batch, alone, x


def test_weight_gradient_of_a_batch_whose_last_frame_alone_is_nonzero():
    shape = (3, 33, 18, 128, 128, 4)
    batch, alone, x = last_frame_only(*shape, seed=61)
    e = rel_err(batch, alone)
    print("dconv wgrad, last frame of %s: rel_err to the frame's own gradient %.3e" % (shape, e))
    assert float(alone.abs().max()) > 0 and float(x[:-1].abs().max()) == 0
    assert e < 1e-5, e


def test_weight_gradient_past_4_gib():
    """42 frames of 448 x 448 at 128 channels are 4.3 GB: the nonzero (last) frame of x crosses byte offset 2^32 (it starts at
    4.21e9 and ends at 4.32e9) while N H W 128 stays below 2^31.  A truncated offset reads the zeros of frame 0 instead."""
    n, h, w, cin, cout, d = 42, 448, 448, 128, 32, 2
    assert (n - 1) * h * w * cin * 4 < 2 ** 32 < n * h * w * cin * 4 and n * h * w * 128 < 2 ** 31
    assert _lib.load().dmc_dconv_supported(n, h, w, cin, cout, d) == 1
    need = n * h * w * (cin + 2 * cout) * 4 + (2 << 30)
    free = torch.cuda.mem_get_info(torch.device(DEV))[0]
    if free < need:
        pytest.skip("the device has %.1f GB free; x, dy and y of 42 x 448 x 448 pixels and their slack need %.1f GB" % (free / 1e9, need / 1e9))
    batch, alone, x = last_frame_only(n, h, w, cin, cout, d, seed=62)
    e = rel_err(batch, alone)
    print("dconv wgrad, last of 42 frames of 448 x 448: rel_err to the frame's own gradient %.3e" % e)
    assert float(alone.abs().max()) > 0
    assert e < 1e-5, e
    # the forward reads the same frame: bit-identical to the frame alone
    wg = nhwc(rnd(63, (cout, cin, 3, 3), 0.05)).to(DEV)
    y = run_fwd(x, wg, n, h, w, cin, cout, d)
    assert torch.equal(y[n - 1:], run_fwd(x[n - 1:].contiguous(), wg, 1, h, w, cin, cout, d))
    assert float(y[n - 1].abs().max()) > 0 and float(y[:n - 1].abs().max()) == 0


# ---------------------------------------------------------------------------------------------------------------------
# the autograd op
# ---------------------------------------------------------------------------------------------------------------------
class Recorder(object):
    def __init__(self, lib):
        self._lib, self.calls = lib, []

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if not name.startswith("dmc_"):
            return fn

        def call(*args):
            self.calls.append((name, args))
            return fn(*args)
        return call

    def names(self):
        return [n for n, _ in self.calls]

    def count(self, name):
        return self.names().count(name)


OP_SHAPE = (2, 17, 40, 128, 96, 8)


def test_autograd_op_vs_fp64():
    n, h, w, cin, cout, d = OP_SHAPE
    x, wt, dy, y64, dx64, dw64 = conv_case(*OP_SHAPE)
    xi = x.to(DEV).contiguous(memory_format=CL).requires_grad_(True)
    wi = wt.to(DEV).requires_grad_(True)                           # contiguous (OIHW) weight, as nn.Conv2d stores it
    y = ops.dilated_conv(xi, wi, d)
    assert tuple(y.shape) == (n, cout, h, w) and y.is_contiguous(memory_format=CL)
    y.backward(dy.to(DEV).contiguous(memory_format=CL))
    assert tuple(xi.grad.shape) == tuple(x.shape) and tuple(wi.grad.shape) == tuple(wt.shape)
    assert wi.grad.stride() == wi.stride()                         # in the weight's own memory format
    e = (rel_err(y, y64), rel_err(xi.grad, dx64), rel_err(wi.grad, dw64))
    print("ops.dilated_conv %s: rel_err value %.3e, x.grad %.3e, weight.grad %.3e" % ((OP_SHAPE,) + e))
    assert e[0] < 1e-5 and e[1] < 1e-5 and e[2] < 1e-5, e
    wcl = wt.to(DEV).contiguous(memory_format=CL).requires_grad_(True)
    ops.dilated_conv(xi.detach(), wcl, d).backward(dy.to(DEV).contiguous(memory_format=CL))
    assert wcl.grad.stride() == wcl.stride() and torch.equal(wcl.grad, wi.grad)
    conv = torch.nn.Conv2d(cin, cout, 3, 1, d, d, bias=False).to(DEV)
    assert ops.dilated_conv_supported(xi, conv)
    assert not ops.dilated_conv_supported(xi.cpu(), conv) and not ops.dilated_conv_supported(xi.double(), conv)
    assert not ops.dilated_conv_supported(xi, torch.nn.Conv2d(cin, cout, 3, 1, d, d, bias=True).to(DEV))
    assert not ops.dilated_conv_supported(xi, torch.nn.Conv2d(cin, cout, 3, 1, 3, 3, bias=False).to(DEV))
    assert not ops.dilated_conv_supported(xi, torch.nn.Conv2d(cin, cout, 3, 1, 1, d, bias=False).to(DEV))
    with pytest.raises(_lib.DmcHipError):
        ops.dilated_conv(xi, wi, 3)


def test_autograd_op_launches_only_what_is_needed(monkeypatch):
    n, h, w, cin, cout, d = OP_SHAPE
    x, wt, dy, _, _, _ = conv_case(*OP_SHAPE)
    rec = Recorder(_lib.load())
    monkeypatch.setattr(_lib, "load", lambda: rec)
    dyg = dy.to(DEV).contiguous(memory_format=CL)

    def run(x_grad, w_grad):
        del rec.calls[:]
        xi = x.to(DEV).contiguous(memory_format=CL).requires_grad_(x_grad)
        wi = wt.to(DEV).requires_grad_(w_grad)
        ops.dilated_conv(xi, wi, d).backward(dyg)
        packs = [a[4] for nm, a in rec.calls if nm == "dmc_dconv_pack_weights"]       # the `transposed` argument
        return xi.grad, wi.grad, packs

    gx, gw, packs = run(True, True)
    assert packs == [0, 1] and rec.count("dmc_dconv_fwd") == 2 and rec.count("dmc_dconv_wgrad") == 1
    gx2, gw2, packs = run(False, True)                             # no transposed pack, no second dmc_dconv_fwd
    assert gx2 is None and packs == [0] and rec.count("dmc_dconv_fwd") == 1 and rec.count("dmc_dconv_wgrad") == 1
    assert torch.equal(gw2, gw)
    gx3, gw3, packs = run(True, False)                             # frozen weight: no dmc_dconv_wgrad
    assert gw3 is None and packs == [0, 1] and rec.count("dmc_dconv_fwd") == 2 and rec.count("dmc_dconv_wgrad") == 0
    assert torch.equal(gx3, gx)


def test_contiguous_grad_output_gives_the_same_gradients():
    n, h, w, cin, cout, d = OP_SHAPE
    x, wt, dy, _, _, _ = conv_case(*OP_SHAPE)
    grads = []
    for fmt in (CL, torch.contiguous_format):
        xi = x.to(DEV).contiguous(memory_format=CL).requires_grad_(True)
        wi = wt.to(DEV).requires_grad_(True)
        g = dy.to(DEV).contiguous(memory_format=fmt)
        assert g.is_contiguous(memory_format=fmt)
        ops.dilated_conv(xi, wi, d).backward(g)
        grads.append((xi.grad, wi.grad))
    assert torch.equal(grads[0][0], grads[1][0]) and torch.equal(grads[0][1], grads[1][1])


# ---------------------------------------------------------------------------------------------------------------------
# whole networks
# ---------------------------------------------------------------------------------------------------------------------
def build_net(att, ds, seed=26):
    o = O.seeded_state_fill(O.build_estimator("ContextNetwork", ds, att), seed=seed)
    cls = model.ContextNetworkAtt if att else model.ContextNetwork
    m = cls(5, True, ds)
    assert list(m.state_dict().keys()) == list(o.state_dict().keys())
    m.load_state_dict(o.state_dict())
    return m.train()


def as_tuple(r):
    return tuple(r) if isinstance(r, (tuple, list)) else (r,)


def train_step(net, x, r, margins=None):
    """{name: tensor} of one forward + backward of a copy of ``net`` in train(): outputs, x.grad, parameter gradients, buffers.
    ``margins``: a list that receives min|z| / max|z| of every BatchNorm2d output z (the LeakyReLU's argument)."""
    net = copy.deepcopy(net).train()
    if margins is not None:
        for mod in net.modules():
            if isinstance(mod, torch.nn.BatchNorm2d):
                mod.register_forward_hook(lambda _m, _i, z: margins.append(float(z.detach().abs().min() / z.detach().abs().max())))
    xi = x.clone().requires_grad_(True)
    outs = as_tuple(net(xi))
    sum((t * r).sum() for t in outs).backward()
    got = {"out%d" % i: t.detach() for i, t in enumerate(outs)}
    got["x.grad"] = xi.grad
    got.update({"grad:" + k: p.grad for k, p in net.named_parameters()})
    got.update({"buffer:" + k: b.detach() for k, b in net.named_buffers()})
    return got


#: LeakyReLU (and the attention head's ReLU) has a kink at 0: where a BatchNorm output z is closer to 0 than two fp32 routes can
#: agree, they may land on different sides of it, that element's gradient then differs by the factor 10 between the slopes, and a
#: comparison of gradients measures the kink, not the convolutions (seen on an MI355X: one such element of 171 k in unit 3 at
#: (3, 5, 33, 18) with input seed 51 put 1.2 into a weight gradient whose stock error is 3e-5).  So the inputs are drawn where the
#: fp64 REFERENCE has no such element: the first seed from 51 upwards at which every BatchNorm output of the fp64 stock network
#: keeps min|z| >= 2^-20 max|z| (sixteen fp32 ulps of the largest value).  A property of the reference alone, found by
#: kink_free_seed() on the CPU and asserted by the test on the reference it computes anyway.
KINK_MARGIN = 2.0 ** -20
INPUT_SEEDS = {(att, ds, shape): seed for att in (0, 1)
               for (ds, shape), seed in {(0, (2, 5, 21, 17)): 57, (0, (3, 5, 33, 18)): 199, (16, (3, 5, 14, 14)): 55}.items()}


def kink_free_seed(att, ds, shape, first=51, tries=400):
    net = build_net(att, ds).double()
    for seed in range(first, first + tries):
        margins = []
        with torch.no_grad():
            hooked = copy.deepcopy(net).train()
            for mod in hooked.modules():
                if isinstance(mod, torch.nn.BatchNorm2d):
                    mod.register_forward_hook(lambda _m, _i, z: margins.append(float(z.abs().min() / z.abs().max())))
            hooked(rnd(seed, shape).double())
        if min(margins) >= KINK_MARGIN:
            return seed
    raise AssertionError("no kink-free input among %d seeds" % tries)


@pytest.mark.parametrize("att", [0, 1])
@pytest.mark.parametrize("ds,shape", [(0, (2, 5, 21, 17)), (0, (3, 5, 33, 18)), (16, (3, 5, 14, 14))], ids=["21x17", "33x18", "ds16-14x14"])
def test_whole_network_training_step(att, ds, shape, monkeypatch):
    net = build_net(att, ds)
    x, r = rnd(INPUT_SEEDS[(att, ds, shape)], shape), rnd(52, (shape[0], 2) + tuple(shape[2:]))
    monkeypatch.setattr(model, "CTX_TRAIN", True)
    margins = []
    ref = train_step(copy.deepcopy(net).double(), x.double(), r.double(), margins)    # CPU: the stock modules whatever the flag
    assert len(margins) == (8 if att else 7) and min(margins) >= KINK_MARGIN, margins
    dev = copy.deepcopy(net).to(DEV)
    assert ops.context_train_supported(dev, x.to(DEV))
    ours = train_step(dev, x.to(DEV), r.to(DEV))
    monkeypatch.setattr(model, "CTX_TRAIN", False)
    stock = train_step(dev, x.to(DEV), r.to(DEV))
    assert sorted(ours) == sorted(ref) == sorted(stock) and len(ours) > 40
    assert tuple(ours["out0"].shape) == (shape[0], 2) + tuple(shape[2:])
    worst, bad = None, []
    for k in sorted(ref):
        if ref[k].dtype == torch.int64:                            # num_batches_tracked
            assert int(ours[k]) == int(ref[k]) == int(stock[k]) == 1, k
            continue
        assert tuple(ours[k].shape) == tuple(ref[k].shape), k
        e = float((ours[k].double().cpu() - ref[k]).abs().max())
        e_ref = float((stock[k].double().cpu() - ref[k]).abs().max())
        top = float(ref[k].abs().max())
        print("ctx train att=%d ds=%d %s %-48s e %.3e e_ref %.3e max|ref| %.3e" % (att, ds, tuple(shape), k, e, e_ref, top))
        if worst is None or e / max(top, 1e-30) > worst[1] / max(worst[3], 1e-30):
            worst = (k, e, e_ref, top)
        if not e <= max(4 * e_ref, 2e-5 * top):
            bad.append((k, e, e_ref, top))
    print("ctx train att=%d ds=%d %s worst: %s e %.3e e_ref %.3e max|ref| %.3e" % ((att, ds, tuple(shape)) + worst))
    assert not bad, bad


@pytest.mark.parametrize("att", [0, 1])
def test_routes(att, monkeypatch):
    net = build_net(att, 0).to(DEV)
    x, r = rnd(51, (2, 5, 21, 17)).to(DEV), rnd(52, (2, 2, 21, 17)).to(DEV)
    stock = []
    orig = torch.nn.Conv2d._conv_forward
    monkeypatch.setattr(torch.nn.Conv2d, "_conv_forward", lambda self, x, w, b: (stock.append(tuple(w.shape)), orig(self, x, w, b))[1])
    rec = Recorder(_lib.load())
    monkeypatch.setattr(_lib, "load", lambda: rec)
    monkeypatch.setattr(model, "CTX_TRAIN", True)                  # DMC_CTX_TRAIN=1
    train_step(net, x, r)
    assert rec.count("dmc_dconv_fwd") == 10 and rec.count("dmc_dconv_wgrad") == 5 and rec.count("dmc_dconv_pack_weights") == 10
    assert stock == [(32, 5, 3, 3)] + [(2, 32, 3, 3)] * (2 if att else 1), stock
    assert not any(nm.startswith("dmc_ctx_") for nm in rec.names())
    del rec.calls[:], stock[:]
    ev = copy.deepcopy(net).eval()                                 # eval() + no_grad: the eval route keeps precedence
    with torch.no_grad():
        ev(x)
    assert any(nm.startswith("dmc_ctx_") for nm in rec.names()) and not any(nm.startswith("dmc_dconv_") for nm in rec.names())
    assert stock == []
    monkeypatch.setattr(model, "CTX_TRAIN", False)                 # the default
    del rec.calls[:], stock[:]
    train_step(net, x, r)
    assert not any(nm.startswith("dmc_dconv_") for nm in rec.names()), rec.names()
    assert len(stock) == (8 if att else 7)


def test_refused_calls_write_nothing():
    lib = _lib.load()
    buf = torch.zeros(1 << 16, dtype=U8, device=DEV)
    y = torch.full((1 << 16,), 0xFF, dtype=U8, device=DEV)
    p, q, s = P(buf), P(y), ops._stream()
    calls = [("dmc_dconv_fwd", lambda: lib.dmc_dconv_fwd(p, p, q, 1, 8, 8, 32, 128, 3, s)),
             ("dmc_dconv_fwd", lambda: lib.dmc_dconv_fwd(p, p, q, 1, 8, 8, 48, 128, 2, s)),
             ("dmc_dconv_fwd", lambda: lib.dmc_dconv_fwd(p, None, q, 1, 8, 8, 32, 128, 2, s)),
             ("dmc_dconv_wgrad", lambda: lib.dmc_dconv_wgrad(p, p, q, q, 1, 8, 8, 32, 128, 3, s)),
             ("dmc_dconv_wgrad", lambda: lib.dmc_dconv_wgrad(p, p, q, q, 1, 8, 8, 32, 48, 1, s)),
             ("dmc_dconv_wgrad", lambda: lib.dmc_dconv_wgrad(p, None, q, q, 1, 8, 8, 32, 128, 2, s)),
             ("dmc_dconv_pack_weights", lambda: lib.dmc_dconv_pack_weights(p, q, 48, 32, 0, s)),
             ("dmc_dconv_pack_weights", lambda: lib.dmc_dconv_pack_weights(p, q, 32, 48, 1, s))]
    for name, call in calls:
        assert call() == -1, name
        assert name.encode() in lib.dmc_last_error(), name
    torch.cuda.synchronize()
    assert bool((y == 0xFF).all())


# ---------------------------------------------------------------------------------------------------------------------
# the memory contract
# ---------------------------------------------------------------------------------------------------------------------
def conv_arena_case(shape):
    n, h, w, cin, cout, d = shape

    def fn(a):
        lib = _lib.load()
        x, wt, dy, _, _, _ = conv_case(*shape)
        wb = a.inp("w", nhwc(wt))
        wf = a.out("wpack", nbytes=lib.dmc_dconv_wpack_bytes(cin, cout), dtype=U8)
        wtp = a.out("wpack_t", nbytes=lib.dmc_dconv_wpack_bytes(cin, cout), dtype=U8)
        a.call("dmc_dconv_pack_weights", wb, wf, cin, cout, 0)
        a.call("dmc_dconv_pack_weights", wb, wtp, cin, cout, 1)
        xb, dyb = a.inp("x", nhwc(x)), a.inp("dy", nhwc(dy))
        a.call("dmc_dconv_fwd", xb, wf, a.out("y", (n, h, w, cout)), n, h, w, cin, cout, d)
        a.call("dmc_dconv_fwd", dyb, wtp, a.out("dx", (n, h, w, cin)), n, h, w, cout, cin, d)
        a.call("dmc_dconv_wgrad", xb, dyb, a.out("dw", (cout, 3, 3, cin)), a.work("ws", lib.dmc_dconv_wgrad_workspace_bytes(n, h, w, cin, cout)),
               n, h, w, cin, cout, d)
    return fn


def _conv_arena_check(shape):
    def check(bufs):
        _, _, _, y64, dx64, dw64 = conv_case(*shape)
        assert rel_err(nchw(bufs["y"].t), y64) < 1e-5
        assert rel_err(nchw(bufs["dx"].t), dx64) < 1e-5
        assert rel_err(nchw(bufs["dw"].t), dw64) < 1e-5
    return check


def refused_fwd_case(a):       # dilation 3: refused, nothing written
    lib = _lib.load()
    n, h, w, cin, cout = 1, 8, 8, 32, 128
    a.call("dmc_dconv_fwd", a.inp("x", torch.zeros(n, h, w, cin)), a.inp("wpack", torch.zeros(lib.dmc_dconv_wpack_bytes(cin, cout), dtype=U8)),
           a.out("y", (n, h, w, cout)), n, h, w, cin, cout, 3)


def refused_wgrad_case(a):     # width 48: refused, nothing written (the workspace query returns 0: a caller's own buffer)
    n, h, w, cin, cout = 1, 8, 8, 48, 64
    a.call("dmc_dconv_wgrad", a.inp("x", torch.zeros(n, h, w, cin)), a.inp("dy", torch.zeros(n, h, w, cout)), a.out("dw", (cout, 3, 3, cin)),
           a.work("ws", 1 << 16), n, h, w, cin, cout, 1)


def refused_pack_case(a):      # width 48: refused, nothing written
    a.call("dmc_dconv_pack_weights", a.inp("w", torch.zeros(64, 3, 3, 48)), a.out("wpack", nbytes=64 * 48 * 54, dtype=U8), 48, 64, 1)


ARENA_CASES = []
for _shape in ((1, 20, 37, 32, 128, 2), (2, 40, 12, 96, 64, 16)):
    ARENA_CASES.append(abi_cases.Case(abi_cases.tag("dmc_dconv", *_shape), ["dmc_dconv_pack_weights", "dmc_dconv_fwd", "dmc_dconv_wgrad"],
                                      conv_arena_case(_shape), check=_conv_arena_check(_shape), capacity=48 << 20))
ARENA_CASES.append(abi_cases.Case("dmc_dconv_fwd-refused-dilation-3", ["dmc_dconv_fwd"], refused_fwd_case, expect_rc=abi_cases.DMC_E_INVALID,
                                  capacity=32 << 20))
ARENA_CASES.append(abi_cases.Case("dmc_dconv_wgrad-refused-width-48", ["dmc_dconv_wgrad"], refused_wgrad_case, expect_rc=abi_cases.DMC_E_INVALID,
                                  capacity=32 << 20))
ARENA_CASES.append(abi_cases.Case("dmc_dconv_pack_weights-refused-width-48", ["dmc_dconv_pack_weights"], refused_pack_case,
                                  expect_rc=abi_cases.DMC_E_INVALID, capacity=32 << 20))
_known = {c.id for c in abi_cases.CASES}
abi_cases.CASES.extend(c for c in ARENA_CASES if c.id not in _known)


@pytest.mark.parametrize("case", ARENA_CASES, ids=[c.id for c in ARENA_CASES])
def test_dconv_entries_memory_contract(case):
    try:
        bufs = run_case(case.fn, device=DEV, capacity=case.capacity, expect_rc=case.expect_rc)
        if case.check is not None:
            case.check(bufs)
    except RuntimeError as e:
        if "HIP error" in str(e) or "illegal memory access" in str(e):
            # a faulted device serves nothing more: end the session here instead of launching the remaining cases on it
            pytest.exit("GPU fault in %s: %s" % (case.id, str(e).splitlines()[0]), returncode=3)
        raise
