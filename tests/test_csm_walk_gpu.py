"""GPU: the persistent small-channel convolutions of conv_small.hip against fp64 at shapes where a wave WALKS several tiles.

Every other unit test of these six kernels gives a wave (or workgroup) at most one tile or tile pair
(tests/test_csm_walk_cpu.py keeps the record), so the prefetch of the next tile, the second half of the register double
buffer, the break in the middle of an iteration, the fp64 statistics and the weight-gradient accumulators carried across
visits, and the partial rows of a capped grid were reached only by the 240-frame GAN step, behind end-to-end bars.  The shapes
of tests/csm_walk_shapes.py give every kernel 2-3 .. 20-21 visits per walker at the smallest size that does.

  (a) forward with the whole epilogue (bias, LeakyReLU, keep mask, statistics) against fp64 at 1e-5, the statistics partials
      against fp64 sums of the kernel's own output (1e-12: the accumulation across visits alone) and of the reference (1e-5);
  (b) data gradient against fp64 at 1e-5;
      a failure of (a) / (b) names the worst tile: image, row, segment and which visit of its wave it was;
  (c) weight gradient against fp64: e_hip <= max(4 e_ref, 1e-5), e_ref = the error of the CPU's fp32 evaluation of the same
      gradient (the factor 4 covers another summation order over 270k .. 1M pixels, the floor is the project's bar);
  (d) integer operands (inputs and gradients in [-4, 4], weights in {-1, 0, 1}): every slice product and partial sum is an
      integer below 2^24, so forward, both gradients and the statistics equal fp64 EXACTLY -- a dropped or doubled tile
      fails whatever the tolerance;
  (e) every run of (a)-(c) twice, bit-identical;
  (f) one whole discriminator block through autograd (conv epilogue -> dmc_conv_nhwc_stats_final -> dmc_bn_apply_nhwc and
      back) at a walking stride-1 shape and at the stride-2 16 -> 32 shape, whose epilogue had no unit test at all.

Buffers the kernels write are pre-filled with NaN: a pixel, a statistics row or a partial slot that is read but never written
shows.  References are computed once per case (module cache, dropped when the module is done)."""
import math

import pytest
import torch
import torch.nn.functional as F

import dmcnet_amd
from dmcnet_amd import ops
from oracle import dmc_oracle as O
from tests.csm_walk_shapes import WALK_CASES, out_map, plans, tile_coords

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CL = torch.channels_last
L = dmcnet_amd._lib
NAN = float("nan")
FWD_CASES = WALK_CASES[:4]

#: weight gradient, (e_hip, e_ref) as this file printed them on an MI355X: max |dw - fp64| / max |fp64| of the kernel and of the
#: CPU's fp32 evaluation; a record, not a bar (the bar is max(4 e_ref, 1e-5))
WORST_MEASURED = {
    (41, 16, 173, 38, 16, 1): (3.381e-07, 2.435e-06),      # csm_wgrad<16>, 3-4 pairs per wave
    (41, 16, 173, 70, 16, 1): (3.924e-07, 3.306e-06),      # csm_wgrad<16>, 5-6
    (81, 32, 173, 38, 32, 1): (6.120e-07, 3.619e-06),      # csm_wgrad<32>, 20-21
    (41, 16, 346, 76, 32, 2): (5.118e-07, 2.822e-06),      # csm_wgrad_s2<16>, 20-21 pairs per workgroup
    (25, 32, 58, 76, 64, 2): (2.448e-07, 1.517e-06),       # csm_wgrad_s2<32>, 4-5
}
# forward / data gradient at the four forward cases: 3.4e-07 .. 6.1e-07 (bar 1e-5); the block through autograd: gradients
# 7e-08 .. 5.4e-06 against e_ref 3e-07 .. 9e-06 (the largest is the convolution's bias gradient in both)

_REF = {}


@pytest.fixture(scope="module", autouse=True)
def bf16x3_arith():
    """conv_small.hip serves these shapes under conv_arith = 1 (the default); the references go when the module is done."""
    lib = L.load()
    before = lib.dmc_get_option(b"conv_arith")
    L.check(lib.dmc_set_option(b"conv_arith", 1), "dmc_set_option")
    yield
    L.check(lib.dmc_set_option(b"conv_arith", before), "dmc_set_option")
    _REF.clear()


def rel_err(a, b):
    a, b = a.detach().double(), b.detach().double().to(a.device)
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))


def cl(t):
    return t.to(DEV).contiguous(memory_format=CL)


def _gen(case, salt):
    return torch.Generator().manual_seed(1000 * WALK_CASES.index(case) + salt)


def reference(case, kind):
    """fp64 F.conv2d and autograd on the CPU, once per (case, kind).  kind "rand": normal operands, bias, keep mask with zeros
    and 1 / 0.75, and the CPU's fp32 weight gradient; kind "int": small integers, no epilogue (results kept as fp32: exact)."""
    key = (case, kind)
    if key in _REF:
        return _REF[key]
    n, cin, h, w, cout, stride = case
    oh, ow = out_map(h, w, stride)
    r = {}
    if kind == "int":
        g = _gen(case, 7)
        r["x"] = torch.randint(-4, 5, (n, cin, h, w), generator=g).float()
        r["w"] = torch.randint(-1, 2, (cout, cin, 3, 3), generator=g).float()
        r["go"] = torch.randint(-4, 5, (n, cout, oh, ow), generator=g).float()
        r["bias"] = r["keep"] = None
    else:
        g = _gen(case, 3)
        r["x"] = torch.randn((n, cin, h, w), generator=g)
        r["w"] = torch.randn((cout, cin, 3, 3), generator=g) * 0.1
        r["go"] = torch.randn((n, cout, oh, ow), generator=g)
        r["bias"] = torch.randn(cout, generator=g) * 0.5
        r["keep"] = (torch.rand((n, cout), generator=g) < 0.75).float() / 0.75
        assert (r["keep"] == 0).any() and (r["keep"] > 1).any()
    xo, wo = r["x"].double().requires_grad_(True), r["w"].double().requires_grad_(True)
    pre = F.conv2d(xo, wo, None, stride, 1)
    (pre * r["go"].double()).sum().backward()
    y = pre.detach()
    if kind == "int":
        assert float(y.abs().max()) < 1 << 24 and float(wo.grad.abs().max()) < 1 << 24
        r["y"], r["dx"], r["dw"] = y.float(), xo.grad.float(), wo.grad.float()
        r["ysum"], r["ysq"] = y.sum((0, 2, 3)), (y * y).sum((0, 2, 3))
    else:
        y = F.leaky_relu(y + r["bias"].double()[None, :, None, None], 0.2) * r["keep"].double()[:, :, None, None]
        r["y"], r["dx"], r["dw"] = y, xo.grad, wo.grad
        w32 = r["w"].clone().requires_grad_(True)
        (F.conv2d(r["x"], w32, None, stride, 1) * r["go"]).sum().backward()
        r["dw32"] = w32.grad
    _REF[key] = r
    return r


def lands_in_conv_small(case, xg, wg, walks=True):
    """The public queries say the launch is conv_small.hip's: supported, the default kernel choice, and (forward / data gradient
    kernels) a statistics row count equal to the restated grid -- at its cap where the case is one that walks."""
    lib = L.load()
    n, cin, h, w, cout, stride = case
    assert ops.conv_nhwc_supported(xg, wg, stride, 1)
    assert lib.dmc_get_option(b"conv_arith") == 1 and lib.dmc_get_option(b"conv_path") == 1 and lib.dmc_get_option(b"conv_cfg") == 0
    p = plans(case)
    if p["fwd"] is not None:
        assert lib.dmc_conv_nhwc_stat_blocks(n, h, w, cin, cout, 3, stride, 1) == p["fwd"].grid
        assert (p["fwd"].grid == p["fwd"].cap) == walks
    return p


def run_fwd(case, xg, wg, bias, keep, act):
    lib = L.load()
    n, cin, h, w, cout, stride = case
    oh, ow = out_map(h, w, stride)
    nblk = lib.dmc_conv_nhwc_stat_blocks(n, h, w, cin, cout, 3, stride, 1)
    y = torch.empty((n, cout, oh, ow), dtype=torch.float32, device=DEV, memory_format=CL).fill_(NAN)
    part = torch.full((nblk + 2, cout, 2), NAN, dtype=torch.float64, device=DEV)        # two guard rows behind the partials
    wpack = ops._floats(lib.dmc_conv_nhwc_wt_bytes(cin, cout, 3, 3), DEV)
    L.check(lib.dmc_conv_nhwc_fwd(L.ptr(xg), L.ptr(wg), L.ptr(wpack), L.ptr(bias), L.ptr(keep), L.ptr(y), L.ptr(part), nblk,
                                  n, h, w, cin, cout, 3, 3, stride, 1, act, ops._stream()), "dmc_conv_nhwc_fwd")
    return y, part, nblk


def run_dgrad(case, gg, wg):
    lib = L.load()
    n, cin, h, w, cout, stride = case
    dx = torch.empty((n, cin, h, w), dtype=torch.float32, device=DEV, memory_format=CL).fill_(NAN)
    wt = ops._floats(lib.dmc_conv_nhwc_wt_bytes(cin, cout, 3, 3), DEV)
    L.check(lib.dmc_conv_nhwc_dgrad(L.ptr(gg), L.ptr(wg), L.ptr(wt), L.ptr(dx), n, h, w, cin, cout, 3, 3, stride, 1,
                                    ops._stream()), "dmc_conv_nhwc_dgrad")
    return dx


def run_wgrad(case, xg, gg):
    lib = L.load()
    n, cin, h, w, cout, stride = case
    dw = torch.empty((cout, cin, 3, 3), dtype=torch.float32, device=DEV, memory_format=CL).fill_(NAN)
    work = ops._floats(lib.dmc_conv_nhwc_wgrad_bytes(n, h, w, cin, cout, 3, 3, stride, 1), DEV).fill_(NAN)
    L.check(lib.dmc_conv_nhwc_wgrad(L.ptr(xg), L.ptr(gg), L.ptr(dw), L.ptr(work), n, h, w, cin, cout, 3, 3, stride, 1,
                                    ops._stream()), "dmc_conv_nhwc_wgrad")
    return dw


def per_tile_error(err, case, of_input):
    """max |error| per 16-pixel tile of the OUTPUT map, [tiles]; err is [N][C][rows][columns] of the output map, or (of_input,
    stride 2) of the input map whose pixels (2 oy + py, 2 ox + px) belong to output position (oy, ox)."""
    n, _, h, w, _, stride = case
    oh, ow = out_map(h, w, stride)
    e = torch.nan_to_num(err, nan=math.inf).amax(1)
    if of_input and stride == 2:
        e = e.reshape(n, oh, 2, ow, 2).amax((2, 4))
    segs = (ow + 15) // 16
    e = F.pad(e, (0, segs * 16 - ow)).reshape(n, oh, segs, 16).amax(3)
    return e.reshape(-1)


def assert_close_by_tile(got, want, case, plan, bar, what, of_input=False):
    """max |got - want| / max |want| < bar; a failure names the worst tile and says which visits of their waves the bad tiles are."""
    want = want.to(DEV)
    err = (got.double() - want.double()).abs()
    scale = float(want.abs().max())
    e = float(err.max()) / scale
    print("%s %s: rel_err %.3e" % (what, case, e))
    if e < bar:
        return e
    tiles = per_tile_error(err, case, of_input)
    walkers = plan.grid * plan.per_group
    visit = torch.arange(tiles.numel(), device=tiles.device) // walkers
    bad = tiles >= bar * scale if bar > 0 else tiles > 0
    worst = int(tiles.argmax())
    img, row, seg = tile_coords(worst, case)
    by_visit = [int((bad & (visit == v)).sum()) for v in range(plan.vmax)]
    pytest.fail("%s %s (%s): rel_err %.3e >= %.0e; worst tile %d = image %d, row %d, segment %d, visit %d of its wave; "
                "%d of %d tiles are bad, per visit %s%s"
                % (what, case, plan.kernel, e, bar, worst, img, row, seg, worst // walkers, int(bad.sum()), tiles.numel(), by_visit,
                   " -- confined to visits >= 1: the tile walk" if by_visit[0] == 0 else ""))


def check_statistics(part, nblk, y, want_sum, want_sq, tol_ref):
    """Exactly nblk finite rows; column sums = fp64 sums of the kernel's own y (the kernel adds the stored fp32 values in fp64:
    only the order differs) and, to tol_ref, of the reference."""
    assert bool(torch.isfinite(part[:nblk]).all()), "a statistics row of the launch was not written"
    assert bool(torch.isnan(part[nblk:]).all()), "the launch wrote behind its statistics rows"
    got = part[:nblk].sum(0)
    yd = y.double()
    own_sum, own_abs, own_sq = yd.sum((0, 2, 3)), yd.abs().sum((0, 2, 3)), (yd * yd).sum((0, 2, 3))
    assert bool(((got[:, 0] - own_sum).abs() <= 1e-12 * own_abs).all()), ((got[:, 0] - own_sum).abs() / own_abs).max()
    assert bool(((got[:, 1] - own_sq).abs() <= 1e-12 * own_sq).all()), ((got[:, 1] - own_sq).abs() / own_sq).max()
    want_sum, want_sq = want_sum.to(DEV), want_sq.to(DEV)
    if tol_ref == 0:
        assert torch.equal(got[:, 0], want_sum) and torch.equal(got[:, 1], want_sq)
    else:
        assert bool(((got[:, 0] - want_sum).abs() <= tol_ref * own_abs).all()), ((got[:, 0] - want_sum).abs() / own_abs).max()
        assert bool(((got[:, 1] - want_sq).abs() <= tol_ref * own_sq).all()), ((got[:, 1] - want_sq).abs() / own_sq).max()


@pytest.mark.parametrize("case", FWD_CASES)
def test_forward_epilogue_and_statistics_vs_fp64(case):
    """(a), (e): conv + bias + LeakyReLU + keep mask and the fp64 statistics partials of a launch whose waves make 2-3 / 4-5 visits."""
    r = reference(case, "rand")
    xg, wg, bias, keep = cl(r["x"]), cl(r["w"]), r["bias"].to(DEV), r["keep"].to(DEV).contiguous()
    p = lands_in_conv_small(case, xg, wg)["fwd"]
    y, part, nblk = run_fwd(case, xg, wg, bias, keep, 1)
    assert nblk == p.grid
    assert_close_by_tile(y, r["y"], case, p, 1e-5, "forward")
    yr = r["y"]
    check_statistics(part, nblk, y, yr.sum((0, 2, 3)), (yr * yr).sum((0, 2, 3)), 1e-5)
    y2, part2, _ = run_fwd(case, xg, wg, bias, keep, 1)
    assert torch.equal(y, y2) and torch.equal(part[:nblk], part2[:nblk])


@pytest.mark.parametrize("case", FWD_CASES)
def test_data_gradient_vs_fp64(case):
    """(b), (e): csm_conv_kernel on dy with the mirrored transposed weights (stride 1), csm_dgrad_s2_kernel (16 -> 32, stride 2)."""
    r = reference(case, "rand")
    xg, wg, gg = cl(r["x"]), cl(r["w"]), cl(r["go"])
    p = lands_in_conv_small(case, xg, wg)["dgrad"]
    dx = run_dgrad(case, gg, wg)
    assert_close_by_tile(dx, r["dx"], case, p, 1e-5, "data gradient", of_input=True)
    assert torch.equal(dx, run_dgrad(case, gg, wg))


@pytest.mark.parametrize("case", WALK_CASES)
def test_weight_gradient_vs_fp64_and_fp32(case):
    """(c), (e): accumulators carried over 3-4 .. 20-21 tile pairs per wave / workgroup, then the fixed-order reductions."""
    r = reference(case, "rand")
    xg, wg, gg = cl(r["x"]), cl(r["w"]), cl(r["go"])
    p = lands_in_conv_small(case, xg, wg)["wgrad"]
    assert p is not None and p.grid == p.cap
    dw = run_wgrad(case, xg, gg)
    assert bool(torch.isfinite(dw).all()), "a partial slot was read but never written"
    e_hip, e_ref = rel_err(dw, r["dw"]), rel_err(r["dw32"], r["dw"])
    print("weight gradient %s (%s): e_hip %.3e, e_ref %.3e" % (case, p.kernel, e_hip, e_ref))
    assert e_hip <= max(4 * e_ref, 1e-5), (e_hip, e_ref)
    assert torch.equal(dw, run_wgrad(case, xg, gg))


@pytest.mark.parametrize("case", WALK_CASES)
def test_integer_operands_exact(case):
    """(d): every product and partial sum is an integer below 2^24, so all three passes and the statistics equal fp64 exactly."""
    r = reference(case, "int")
    xg, wg, gg = cl(r["x"]), cl(r["w"]), cl(r["go"])
    p = lands_in_conv_small(case, xg, wg)
    y, part, nblk = run_fwd(case, xg, wg, None, None, 0)
    if not torch.equal(y, r["y"].to(DEV)):
        assert p["fwd"] is not None, "forward %s differs from fp64" % (case,)
        assert_close_by_tile(y, r["y"], case, p["fwd"], 0.0, "integer forward")
    check_statistics(part, nblk, y, r["ysum"], r["ysq"], 0)
    dx = run_dgrad(case, gg, wg)
    if not torch.equal(dx, r["dx"].to(DEV)):
        assert p["dgrad"] is not None, "data gradient %s differs from fp64" % (case,)
        assert_close_by_tile(dx, r["dx"], case, p["dgrad"], 0.0, "integer data gradient", of_input=True)
    dw = run_wgrad(case, xg, gg)
    want = r["dw"].to(DEV)
    assert torch.equal(dw, want), "weight gradient %s: %d of %d values differ from fp64, largest difference %g" % (
        case, int((dw != want).sum()), dw.numel(), float((dw - want).abs().max()))


def _block_pair(cin, cout, stride, dtype):
    conv, bn = torch.nn.Conv2d(cin, cout, 3, stride, 1), torch.nn.BatchNorm2d(cout, 0.8)
    O.seeded_state_fill(conv, 212)
    O.seeded_state_fill(bn, 213)
    return conv.to(dtype), bn.to(dtype)


def _stock_block(conv, bn, x, keep, r):
    """The stock modules on the CPU in the dtype of conv: output, the five gradients, the running statistics."""
    xo = x.to(conv.weight.dtype).requires_grad_(True)
    yo = bn(F.leaky_relu(conv(xo), 0.2) * keep.to(xo.dtype)[:, :, None, None])
    (yo * r.to(xo.dtype)).sum().backward()
    return dict(y=yo.detach(), grads=[xo.grad, conv.weight.grad, conv.bias.grad, bn.weight.grad, bn.bias.grad],
                running=[bn.running_mean, bn.running_var])


BLOCK_CASES = [  # (N, Cin, H, W, Cout, stride), gradients held to max(4 e_ref, 2e-5) (True) or to 2e-5
    ((41, 16, 173, 38, 16, 1), True),
    ((41, 16, 346, 76, 32, 2), True),      # csm_conv_s2's epilogue feeding dmc_conv_nhwc_stats_final and dmc_bn_apply_nhwc
    ((5, 16, 20, 24, 32, 2), False),       # the same block at one tile per wave, at test_disc_block_unit's own bars
]


@pytest.mark.parametrize("case,walks", BLOCK_CASES)
def test_disc_block_through_autograd_vs_stock_modules(case, walks):
    """(f): ops.disc_block, BatchNorm in training mode, against the stock modules in fp64: output and running statistics at 1e-5,
    the five gradients at max(4 e_ref, 2e-5) with e_ref from the stock modules in fp32 on the CPU (BatchNorm's backward
    cancels over 270k values; 2e-5 is test_disc_block_unit's bar)."""
    n, cin, h, w, cout, stride = case
    oh, ow = out_map(h, w, stride)
    g = torch.Generator().manual_seed(4242 + h)
    x = torch.randn((n, cin, h, w), generator=g)
    r = torch.randn((n, cout, oh, ow), generator=g)
    keep = (torch.rand((n, cout), generator=g) < 0.75).float() / 0.75
    conv_d, bn_d = _block_pair(cin, cout, stride, torch.float64)
    want = _stock_block(conv_d, bn_d, x, keep, r)
    conv_m, bn_m = _block_pair(cin, cout, stride, torch.float32)
    conv_m, bn_m = conv_m.to(DEV).to(memory_format=CL), bn_m.to(DEV)
    xg = cl(x).requires_grad_(True)
    assert ops.disc_block_supported(xg, conv_m, False)
    p = lands_in_conv_small(case, xg, conv_m.weight, walks)
    assert (p["fwd"].vmax >= 3) == walks and (p["wgrad"].vmax >= 3) == walks
    y = ops.disc_block(xg, conv_m, keep.to(DEV), bn_m, True, first=False)
    (y * cl(r)).sum().backward()
    assert rel_err(y, want["y"]) < 1e-5
    assert rel_err(bn_m.running_mean, want["running"][0]) < 1e-5 and rel_err(bn_m.running_var, want["running"][1]) < 1e-5
    assert int(bn_m.num_batches_tracked) == 1
    got = [xg.grad, conv_m.weight.grad, conv_m.bias.grad, bn_m.weight.grad, bn_m.bias.grad]
    e_ref = [0.0] * 5
    if walks:
        f32 = _stock_block(*_block_pair(cin, cout, stride, torch.float32), x, keep, r)
        e_ref = [rel_err(a, b) for a, b in zip(f32["grads"], want["grads"])]
    e_hip = [rel_err(a, b) for a, b in zip(got, want["grads"])]
    print("disc_block %s: e_hip %s, e_ref %s" % (case, ["%.2e" % e for e in e_hip], ["%.2e" % e for e in e_ref]))
    for name, eh, er in zip(("dx", "dw", "db", "dgamma", "dbeta"), e_hip, e_ref):
        assert eh <= max(4 * er, 2e-5), (name, eh, er)
