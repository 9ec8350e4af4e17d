"""GPU parity of the I3D trunk's EVAL path: Unit3Dpy (conv -> BatchNorm3d with RUNNING statistics -> ReLU,
code/dmcnet_I3D/network/i3d.py:390-398 under net.eval() + no_grad) as one convolution launch whose epilogue applies the
BatchNorm as a per-channel affine map (ops.conv_bn_relu3d_eval / dmc_unit3d_bf16_fwd_eval), the stem likewise
(ops.stem3d_bn_relu_eval / dmc_stem3d_bf16_fwd_eval), the dispatch of i3d.Unit3Dpy / Mixed, and the video-level evaluator on the
device.

fp64 references are computed here from the bf16-rounded x and w, as in test_conv3d_gpu.py, whose bf16_close bar (one bf16
rounding plus a little absolute slack for cancellation) applies."""
import copy

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import dmcnet_amd
from dmcnet_amd import evaluate, i3d, ops
from oracle import dmc_oracle as O
from tests.test_conv3d_gpu import CASES, bf16_close, rnd

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CL3 = torch.channels_last_3d


def rel_err(a, b):
    a, b = a.detach().double().cpu(), torch.as_tensor(b).double().cpu()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))


def _bn(cout, seed):
    """BatchNorm3d in eval mode with running statistics that matter: mean != 0, variance spread over 1e-2 .. 1e2, about half of the
    gammas negative (the ReLU clips)."""
    g = torch.Generator().manual_seed(seed)
    bn = torch.nn.BatchNorm3d(cout).eval()
    with torch.no_grad():
        bn.running_mean.copy_(torch.randn(cout, generator=g) * 0.5)
        bn.running_var.copy_(10.0 ** (torch.rand(cout, generator=g) * 4.0 - 2.0))
        bn.weight.copy_(torch.randn(cout, generator=g))
        bn.bias.copy_(torch.randn(cout, generator=g) * 0.3)
    assert float(bn.weight.detach().min()) < 0 < float(bn.weight.detach().max())
    return bn.to(DEV)


def _affine64(y, bn, relu):
    sh = (1, -1, 1, 1, 1)
    m, v, g, b = (t.detach().double().cpu().view(sh) for t in (bn.running_mean, bn.running_var, bn.weight, bn.bias))
    r = (y - m) * g / torch.sqrt(v + bn.eps) + b
    return r.clamp_min(0.0) if relu else r


def _conv(cin, cout, k, wt):
    conv = torch.nn.Conv3d(cin, cout, k, padding=k // 2, bias=False).to(DEV)
    with torch.no_grad():
        conv.weight.copy_(wt.to(DEV))
    return conv


@pytest.fixture
def conv_cfg(request):
    lib = dmcnet_amd._lib.load()
    before = lib.dmc_get_option(b"conv_cfg")
    dmcnet_amd._lib.check(lib.dmc_set_option(b"conv_cfg", int(request.param)), "dmc_set_option")
    yield int(request.param)
    dmcnet_amd._lib.check(lib.dmc_set_option(b"conv_cfg", before), "dmc_set_option")


@pytest.mark.parametrize("case", CASES)
def test_unit_eval_vs_fp64(case):
    """relu?((conv3d(x, w) - mean) * gamma / sqrt(var + eps) + beta) against fp64 on the bf16-rounded operands: 1x1x1 and 3x3x3,
    the odd branch widths, depth 1, ragged tiles, the 56 / 28 / 14 / 7-wide maps of the patch-resident kernel; ReLU on and off.
    The running buffers are left as they were."""
    n, cin, d, h, w, cout, k = case
    x = rnd(301, (n, cin, d, h, w)).bfloat16()
    wt = rnd(302, (cout, cin, k, k, k)) * (2.0 / (cin * k ** 3)) ** 0.5
    y64 = F.conv3d(x.double(), wt.bfloat16().double(), None, 1, k // 2)
    conv, bn = _conv(cin, cout, k, wt), _bn(cout, 303)
    before = [t.clone() for t in (bn.running_mean, bn.running_var, bn.num_batches_tracked)]
    xg = x.to(DEV).contiguous(memory_format=CL3)
    for relu in (True, False):
        with torch.no_grad():
            assert ops.conv_bn_relu3d_eval_supported(xg, conv, bn)
            y = ops.conv_bn_relu3d_eval(xg, conv, bn, relu)
        assert y.dtype == torch.bfloat16 and y.shape == y64.shape and y.is_contiguous(memory_format=CL3)
        bf16_close(y, _affine64(y64, bn, relu), "eval unit relu=%s" % relu)
    for a, b in zip(before, (bn.running_mean, bn.running_var, bn.num_batches_tracked)):
        assert torch.equal(a, b)


@pytest.mark.parametrize("conv_cfg", [1, 2, 3, 4, 5, 6, 7, 8], indirect=True)
def test_unit_eval_every_tile_configuration(conv_cfg):
    """Each forward tile configuration (conv_cfg 1 .. 5 the tap-stepping tiles, 6 their automatic choice, 7 / 8 the
    patch-resident kernel with 128- / 64-position tiles) through the eval epilogue on a shape with ragged pixel and channel edges."""
    n, cin, d, h, w, cout, k = 2, 48, 3, 11, 9, 160, 3
    x = rnd(311, (n, cin, d, h, w)).bfloat16()
    wt = rnd(312, (cout, cin, k, k, k)) * 0.05
    y64 = F.conv3d(x.double(), wt.bfloat16().double(), None, 1, 1)
    conv, bn = _conv(cin, cout, k, wt), _bn(cout, 313)
    with torch.no_grad():
        y = ops.conv_bn_relu3d_eval(x.to(DEV).contiguous(memory_format=CL3), conv, bn, True)
    bf16_close(y, _affine64(y64, bn, True), "eval cfg %d" % conv_cfg)


@pytest.mark.parametrize("case,cfg", [((1, 96, 3, 14, 14, 208, 3), 0), ((2, 48, 3, 11, 9, 160, 3), 1), ((2, 64, 3, 9, 7, 48, 1), 0)])
def test_unit_eval_into_a_channel_slice(case, cfg):
    """`into` = a channel slice of a wider channels_last_3d tensor (an Inception block's output): only the unit's channels change --
    sentinels elsewhere survive -- and they are bit-identical to the dense call (patch-resident and tap-stepping kernels)."""
    n, cin, d, h, w, cout, k = case
    lib = dmcnet_amd._lib.load()
    before = lib.dmc_get_option(b"conv_cfg")
    x = rnd(321, (n, cin, d, h, w)).bfloat16().to(DEV).contiguous(memory_format=CL3)
    conv, bn = _conv(cin, cout, k, rnd(322, (cout, cin, k, k, k)) * 0.05), _bn(cout, 323)
    wide = torch.full((n, 16 + cout + 24, d, h, w), 7.0, device=DEV).bfloat16().contiguous(memory_format=CL3)
    try:
        dmcnet_amd._lib.check(lib.dmc_set_option(b"conv_cfg", cfg), "dmc_set_option")
        with torch.no_grad():
            dense = ops.conv_bn_relu3d_eval(x, conv, bn, True)
            got = ops.conv_bn_relu3d_eval(x, conv, bn, True, into=wide[:, 16:16 + cout])
    finally:
        dmcnet_amd._lib.check(lib.dmc_set_option(b"conv_cfg", before), "dmc_set_option")
    torch.cuda.synchronize()
    assert got.data_ptr() == wide[:, 16:].data_ptr()
    assert torch.equal(wide[:, 16:16 + cout], dense)
    assert bool((wide[:, :16] == 7.0).all()) and bool((wide[:, 16 + cout:] == 7.0).all())


@pytest.mark.parametrize("relu", [True, False])
def test_stem_eval_vs_fp64(relu):
    """The stem unit in eval mode: pad (front 2, back 3) + 7x7x7 / stride 2 convolution + BatchNorm (running statistics) + ReLU
    against fp64, on an odd output depth (5) and a 224-wide plane; the module's dispatch gives the same tensor."""
    torch.manual_seed(41)
    unit = i3d.Unit3Dpy(2, 64, (7, 7, 7), (2, 2, 2)).to(DEV).eval()
    unit.batch3d = _bn(64, 42)
    unit.relu = relu
    x = torch.randn(1, 2, 10, 12, 224, device=DEV)
    w = unit.conv3d.weight.detach()
    ref = F.conv3d(F.pad(x.bfloat16().double(), (2, 3, 2, 3, 2, 3)), w.bfloat16().double(), None, 2, 0).cpu()
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
        assert ops.stem3d_eval_supported(x, unit.conv3d, unit.batch3d)
        y = ops.stem3d_bn_relu_eval(x, unit.conv3d, unit.batch3d, relu)
        y2 = unit(x)
    assert tuple(y.shape) == (1, 64, 5, 6, 112) and y.dtype == torch.bfloat16 and y.is_contiguous(memory_format=CL3)
    bf16_close(y, _affine64(ref, unit.batch3d, relu), "stem eval relu=%s" % relu)
    assert torch.equal(y, y2)


def test_eval_trunk_runs_no_stock_convolution_batchnorm_or_cat(monkeypatch):
    """net.eval() + no_grad on a bf16 trunk (trunk-only I3D fed a 2-channel cue, 1 x 16 frames at 224^2): the only stock
    convolution is the biased head conv3d_0c_1x1; no BatchNorm and no concatenation runs."""
    torch.manual_seed(31)
    net = i3d.I3D(51, modality="flow").to(DEV).eval()
    net.trunk_dtype = torch.bfloat16
    x = torch.randn(1, 2, 16, 224, 224, device=DEV)
    convs, counts = [], {"batch_norm": 0, "cat": 0}
    orig_conv, orig_bn, orig_cat = torch.nn.Conv3d._conv_forward, F.batch_norm, torch.cat

    def bn_spy(*a, **k):
        counts["batch_norm"] += 1
        return orig_bn(*a, **k)

    def cat_spy(*a, **k):
        counts["cat"] += 1
        return orig_cat(*a, **k)
    monkeypatch.setattr(torch.nn.Conv3d, "_conv_forward", lambda self, x, w, b: (convs.append(tuple(w.shape)), orig_conv(self, x, w, b))[1])
    monkeypatch.setattr(F, "batch_norm", bn_spy)
    monkeypatch.setattr(torch, "cat", cat_spy)
    with torch.no_grad():
        out = net(x)
    torch.cuda.synchronize()
    assert convs == [(400, 1024, 1, 1, 1)], convs
    assert counts == {"batch_norm": 0, "cat": 0}, counts
    assert tuple(out.shape) == (1, 51) and bool(torch.isfinite(out).all())


def test_eval_route_vs_reference_golden_g8(golden, monkeypatch):
    """G8 (the reference's own I3D, eval mode, fp32): the bf16 trunk's logits on the eval route within 5e-2, and no worse than 1.5x
    the EVAL_FUSED=0 route (conv3d_bf16 -> stock BatchNorm3d -> ReLU, MIOpen stem, torch.cat) on the same run."""
    g = golden("g8_i3d_eval")
    net = i3d.I3D(51, modality="flow+mp4", dropout_prob=0, arch_estimator="DenseNetTiny", arch_d="Discriminator")
    O.seeded_state_fill(net, seed=81)
    net.to(DEV).eval()
    net.trunk_dtype = torch.bfloat16
    data = rnd(82, (1, 7, 16, 224, 224)).to(DEV)
    errs = {}
    for fused in (True, False):
        monkeypatch.setattr(i3d, "EVAL_FUSED", fused)
        with torch.no_grad():
            errs[fused] = rel_err(net(data[:, :5]), g["logits"])
    print("  G8 logits rel err: eval route %.4e, EVAL_FUSED=0 route %.4e" % (errs[True], errs[False]))
    assert errs[True] < 5e-2 and errs[True] <= 1.5 * errs[False], errs


def test_eval_route_is_deterministic_and_stream_transparent(monkeypatch):
    """Two eval forwards are bit-identical, and so is one with the Inception branches on one stream."""
    torch.manual_seed(33)
    net = i3d.I3D(51, modality="flow").to(DEV).eval()
    O.seeded_state_fill(net, seed=34)
    net.trunk_dtype = torch.bfloat16
    x = torch.randn(2, 2, 16, 224, 224, device=DEV)
    outs = []
    for streams in (True, True, False):
        monkeypatch.setattr(i3d, "BRANCH_STREAMS", streams)
        with torch.no_grad():
            outs.append(net(x))
    torch.cuda.synchronize()
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2])


@pytest.mark.slow
def test_eval_route_at_the_recipe_shape(monkeypatch):
    """The evaluator recipe's batch (code/dmcnet_I3D/test/test.sh: 2 clips x 250 frames at 224^2) on a seeded bf16 trunk: finite
    logits, the eval route within 5e-2 of the EVAL_FUSED=0 route."""
    net = i3d.I3D(51, modality="flow").to(DEV).eval()
    O.seeded_state_fill(net, seed=35)
    net.trunk_dtype = torch.bfloat16
    x = torch.randn(2, 2, 250, 224, 224, device=DEV, generator=torch.Generator(device=DEV).manual_seed(36))
    res = {}
    for fused in (True, False):
        monkeypatch.setattr(i3d, "EVAL_FUSED", fused)
        with torch.no_grad():
            res[fused] = net(x).float()
    assert bool(torch.isfinite(res[True]).all())
    err = rel_err(res[True], res[False])
    print("  2 x 250 frames: eval route vs EVAL_FUSED=0 rel err %.4e" % err)
    assert err < 5e-2, err


def test_evaluate_i3d_on_the_device():
    """evaluate.evaluate_i3d around a small bf16 I3D (DenseNetTiny generator, 2 clips x 16 frames per batch, video names repeating
    across batches): per-clip scores, per-video sums and counts and the three metrics equal a host recomputation from the same
    logits."""
    net = i3d.I3D(51, modality="flow+mp4", dropout_prob=0, arch_estimator="DenseNetTiny")
    O.seeded_state_fill(net, seed=37)
    net.to(DEV)
    net.trunk_dtype = torch.bfloat16
    seen = []

    class Rec(torch.nn.Module):
        def __init__(self, inner):
            super().__init__()
            self.inner = inner

        def forward(self, x):
            y = self.inner(x)
            seen.append(y.detach().float().cpu())
            return y
    names = ["a", "b", "b", "c", "a", "b"]
    tgt = torch.tensor([3, 7, 7, 11, 3, 7])
    batches = [(rnd(40 + i, (2, 7, 16, 224, 224)), tgt[2 * i:2 * i + 2], names[2 * i:2 * i + 2]) for i in range(3)]
    res = evaluate.evaluate_i3d(Rec(net), batches, DEV)
    assert not net.training
    logits = torch.cat(seen, 0).double()
    prob = torch.softmax(logits, 1)
    assert np.abs(res["scores"] - prob.numpy()).max() < 1e-6 and np.array_equal(res["labels"], tgt.view(-1, 1).numpy())
    order = ["a", "b", "c"]
    assert res["videos"] == order and res["video_counts"].tolist() == [2, 3, 1]
    sums = torch.stack([prob[[i for i, n in enumerate(names) if n == v]].sum(0) for v in order])
    assert np.abs(res["video_scores"] - sums.numpy()).max() < 1e-5
    first_batch = {"a": 0, "b": 0, "c": 1}
    loss = [float(F.cross_entropy(logits[2 * b:2 * b + 2], tgt[2 * b:2 * b + 2])) for b in range(3)]
    lab = torch.tensor([3, 7, 11])
    top1 = float((sums.argmax(1) == lab).double().mean())
    top5 = float(np.mean([int(lab[j]) in sums[j].topk(5).indices.tolist() for j in range(3)]))
    m = res["metrics"]
    assert abs(m["loss-ce"] - np.mean([loss[first_batch[v]] for v in order])) < 1e-4
    assert m["top1"] == top1 and m["top5"] == top5, (m, top1, top5)
