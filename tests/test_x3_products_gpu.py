"""GPU tests that tell six bf16x3 slice products from five: conv_x3s.hip, conv_x3q.hip, and conv_nhwc.hip /
conv_small.hip under option conv_arith = 1, against tests/x3_ref.py (whose own checks are tests/test_x3_ref_cpu.py).

Exact layer, no tolerance.  Pre-split kernels take crafted slice tensors: small integers (|u| <= 3, half of them zero) live
in ONE slice of an operand, so every product and partial sum is an integer below 2^24 (asserted from B = sum |a||b|, which
bounds the partial sums of any order) and the result must equal the fp64 integers bit for bit.
  * weight gradients: x in slice i, dy in slice j, all nine (i, j): the integer gradient for the six documented pairs,
    all zeros for (1,2) (2,1) (2,2);
  * forward / data gradient: the activation in slice i against fp32 weights whose split is known by construction
    (+-(256 p + q): s2 = 0; +-(65536 p + 256 q + r)), nonzero in one tap and one 64-channel block of the contraction at a
    time.  Slice 0 sees the whole weight, slice 1 sees s0 + s1, slice 2 sees s0 only.  (The second family's values reach
    2^24 - 1, so its activations are one-hot over the channels with |u| = 1: one term per output.)
In-loop-split kernels cannot be handed slices; a one-hot operand (+-1 / +-2) against full 24-bit Gaussian values must return
the other operand's value, scaled, bit for bit: the partial sums of a value's slices are fp32 values, a lost (i, 0) or
(0, j) product is not.  The two 16- / 32-channel shapes reach conv_small.hip: csm_supported (Cin = Cout in {16, 32}, 3 x 3,
stride 1) and csm_fwd_s2 / csm_dgrad_s2 / csm_wgrad_s2_supported (16 -> 32, stride 2, even H and W) are tried first by
dmc_conv_nhwc_fwd / _dgrad / _wgrad whenever conv_arith = 1.

Statistical layer.  Gaussian operands and a wide-range family (per-channel scales 2^-6 .. 2^6, a tenth exact bf16), weights
nonzero in one tap at a time (K = Cin: no other tap dilutes a defect), outputs grouped by tap x 64-wide channel block with
>= 1000 outputs per group.  With B = sum |a||b| in fp64, per group
    rms(got - fp64) / rms(B) <= 3 x the same figure of the CPU emulation on the same operands,
    max(|got - fp64| / B)    <= 4 x the emulation's maximum over the whole tensor.
The bars never look at the kernel; tests/test_x3_ref_cpu.py shows every seeded one-tap / one-chunk defect above them and the
emulation's own order dependence within a third of them.  conv_x3q.hip takes even input sizes: its deepest-K case is the
512-channel 14 x 14 input whose output grid is 7 x 7.  Shapes of conv_nhwc that the fp32 MFMA kernels serve (Cin 32, 48)
are held to the same bars: they must not be worse than the arithmetic that replaced them.

Measured on an MI355X (all 117 cases pass; WORST_MEASURED below has every kernel and pass): no kernel forms a product outside
the six or misses one of them.  Worst kernel / emulation ratios: rms 1.61 (bar 3), max 3.32 (bar 4).  The pre-split and
in-loop-split forward / data-gradient loops sit at 1.3 .. 1.5 x the emulation's rms on K = 64, the weight gradients (long K,
split over workgroups and reduced) at 0.8 .. 1.05 x: the emulation rounds once per 16-term dot product, which the matrix
instruction's internal summation need not do, so a short contraction shows its rounding and a long one averages it out.  The
largest max ratio belongs to a shape the fp32 MFMA kernel serves (Cin 32, stride-2 data gradient, ~1000 live outputs a tap).
Tried once against a library whose x3s_conv_kernel skipped the (1,1) product in the centre tap only: 36 of the 53 x3s cases here
failed (both layers, forward and data gradient), while every 1e-5 case of tests/test_x3s_gpu.py passed."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F
from torch.nn import grad as G

import dmcnet_amd
from dmcnet_amd import ops
from tests import x3_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CL = torch.channels_last
TWO24 = float(1 << 24)
WORST = {}
#: the worst (rms, max) ratios this file printed on an MI355X, per kernel and pass (bars 3 and 4); a record, not a bar
WORST_MEASURED = {
    "x3s-fwd": (1.478, 1.944), "x3s-dgrad": (1.456, 1.982), "x3s-wgrad": (1.050, 0.777),
    "x3q-fwd3": (1.528, 2.317), "x3q-fwd1": (1.388, 1.761), "x3q-dgrad3": (1.481, 2.640), "x3q-dgrad1": (1.398, 1.905),
    "x3q-wgrad3": (0.811, 0.527), "x3q-wgrad1": (0.949, 1.068),
    "nhwc-fwd": (1.398, 1.853), "nhwc-dgrad": (1.570, 3.317), "nhwc-wgrad": (1.610, 1.461),
}


def rs(seed):
    return np.random.RandomState(seed)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(DEV).contiguous(memory_format=CL)


def f64(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64))


def rows(t):
    """[N, C, H, W] tensor -> numpy float64 [N H W, C] (the GEMM's output layout)."""
    return t.detach().double().cpu().permute(0, 2, 3, 1).reshape(-1, t.shape[1]).numpy()


def assert_exact(got, want, what):
    """torch.equal(got, want) in fp64, naming the taps / 64-channel blocks that differ when it does not hold."""
    got, want = got.detach().double().cpu(), torch.as_tensor(want, dtype=torch.float64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    if torch.equal(got, want):
        return
    bad = (got != want).nonzero()
    where = sorted({tuple(int(v) // (64 if d < 2 else 1) for d, v in enumerate(ix)) for ix in bad[:4096]})[:8]
    raise AssertionError("%s: %d of %d values differ; first (dim0 / 64, dim1 / 64, y, x): %s; got %s want %s" %
                         (what, bad.shape[0], got.numel(), where, got[tuple(bad[0])].item(), want[tuple(bad[0])].item()))


def report(what, rms_ratio, max_ratio, extra=""):
    key = what.split(" ")[0]
    for k, v in ((key + " rms", rms_ratio), (key + " max", max_ratio)):
        WORST[k] = max(WORST.get(k, 0.0), v)
    print("  %s  kernel / emulation: rms %.3f (bar 3)  max %.3f (bar 4)  %s" % (what, rms_ratio, max_ratio, extra))
    print("  worst so far: %s" % "  ".join("%s %.3f" % kv for kv in sorted(WORST.items())))
    assert rms_ratio <= 3.0 and max_ratio <= 4.0, (what, rms_ratio, max_ratio)


@pytest.fixture
def conv_arith(request):
    """Option conv_arith for one test: 0 = fp32 MFMA, 1 = bf16x3 (fp32 products from three bf16 slices)."""
    lib = dmcnet_amd._lib.load()
    before = lib.dmc_get_option(b"conv_arith")
    dmcnet_amd._lib.check(lib.dmc_set_option(b"conv_arith", int(request.param)), "dmc_set_option")
    yield int(request.param)
    dmcnet_amd._lib.check(lib.dmc_set_option(b"conv_arith", before), "dmc_set_option")


X3S_SHAPES = [(2, 64, 14, 14, 64), (1, 64, 56, 56, 64), (3, 128, 7, 7, 64), (2, 64, 10, 14, 128)]
X3S_TWO_WG = (37, 64, 14, 14, 64)           # forward only, one tap: the two-workgroup configuration
X3Q_SHAPES = [(1, 64, 8, 8, 64), (3, 64, 20, 12, 64), (2, 128, 28, 28, 64), (1, 64, 56, 56, 64)]
X3Q_WGRAD_SHAPES = X3Q_SHAPES[2:]           # the weight gradient walks whole padded rows of 28 / 14 / 7-wide output grids only
NHWC_SHAPES = [(2, 64, 14, 14, 64, 3, 1), (1, 32, 13, 11, 64, 3, 2), (3, 48, 9, 7, 80, 3, 1), (2, 128, 10, 10, 64, 1, 2),
               (3, 16, 9, 7, 16, 3, 1), (3, 16, 10, 38, 32, 3, 2)]       # the last two: conv_small.hip
DEEP_X3S = (2, 512, 7, 7, 64)
DEEP_X3Q = (2, 512, 14, 14, 64)
DEEP_NHWC = (2, 512, 7, 7, 64, 3, 1)


def x3q_wgrad_ok(shape):
    n, cin, h, w, cout = shape
    return bool(dmcnet_amd._lib.load().dmc_x3q_conv_wgrad_supported(n, h // 2, w // 2, cin, cout))


# ================================================================ exact layer: weight gradients, all nine (i, j)
def int_operands(seed, x_shape, dy_shape):
    r = rs(seed)
    return R.small_ints(r, x_shape), R.small_ints(r, dy_shape)


def dw_fp64(x, dy, wshape, stride, pad):
    return G.conv2d_weight(f64(x), wshape, f64(dy), stride=stride, padding=pad)


@pytest.mark.parametrize("shape", X3S_SHAPES)
def test_x3s_wgrad_forms_the_six_products_and_no_other(shape):
    n, cin, h, w, cout = shape
    assert dmcnet_amd._lib.load().dmc_x3s_conv_wgrad_supported(n, h, w, cin, cout)
    x, dy = int_operands(701, (n, cin, h, w), (n, cout, h, w))
    assert 9.0 * n * h * w < TWO24                               # |x dy| <= 9 per pixel: every partial sum is an exact integer
    want = dw_fp64(x, dy, (cout, cin, 3, 3), 1, 1)
    assert want.abs().max() > 0 and torch.equal(want, want.round())
    xs0, dys0 = ops.x3s_split(dev(x)), ops.x3s_split(dev(dy))
    for i in range(3):
        for j in range(3):
            dw = ops.x3s_conv_wgrad(R.rotate_slices(xs0, i), R.rotate_slices(dys0, j), n, h, w, cin, cout)
            assert_exact(dw, want if (i, j) in R.SIX else torch.zeros_like(want), "x3s wgrad, x slice %d, dy slice %d" % (i, j))


@pytest.mark.parametrize("shape", X3Q_WGRAD_SHAPES)
def test_x3q_wgrad_forms_the_six_products_and_no_other(shape):
    n, cin, h, w, cout = shape
    oh, ow = h // 2, w // 2
    assert x3q_wgrad_ok(shape) and not any(x3q_wgrad_ok(s) for s in X3Q_SHAPES[:2])
    x, dy3 = int_operands(702, (n, cin, h, w), (n, cout, oh, ow))
    dy1 = R.small_ints(rs(703), (n, cout, oh, ow))
    assert 9.0 * n * oh * ow < TWO24
    want3, want1 = dw_fp64(x, dy3, (cout, cin, 3, 3), 2, 1), dw_fp64(x, dy1, (cout, cin, 1, 1), 2, 0)
    assert want3.abs().max() > 0 and want1.abs().max() > 0
    xq0 = ops.x3q_split(dev(x))
    d30, d10 = ops.x3s_split(dev(dy3)), ops.x3s_split(dev(dy1))
    for i in range(3):
        for j in range(3):
            dw3, dw1 = ops.x3q_conv_wgrad(R.rotate_slices(xq0, i), R.rotate_slices(d30, j), R.rotate_slices(d10, j), n, oh, ow, cin, cout)
            six = (i, j) in R.SIX
            assert_exact(dw3, want3 if six else torch.zeros_like(want3), "x3q wgrad dw3, x slice %d, dy slice %d" % (i, j))
            assert_exact(dw1, want1 if six else torch.zeros_like(want1), "x3q wgrad dw1, x slice %d, dy slice %d" % (i, j))


# ================================================================ exact layer: forward / data gradient on crafted slices
def crafted_activation(r, shape, family):
    """family 1: |u| <= 3 integers; family 2 (weights up to 2^24 - 1): one channel per pixel, |u| = 1."""
    return R.small_ints(r, shape) if family == 1 else R.one_hot_channels(r, shape, values=(1.0,))


def tap_block_cases(w, parts, ntaps, nblocks, axis, taps=None):
    """(tap, block, fp32 weight, [weight seen by an activation in slice i]) with the weight zero outside one tap and one
    64-channel block of the contraction axis."""
    for tap in (range(ntaps) if taps is None else taps):
        for blk in range(nblocks):
            b = blk if nblocks > 1 else None
            wt = R.only_tap(w, tap, b, axis=axis)
            seen = [R.only_tap(p, tap, b, axis=axis) for p in parts]
            yield tap, blk, wt, [R.weight_seen_by_slice(seen, i) for i in range(3)]


def check_bound(act, wt, stride, pad, transposed_to=None):
    """max B < 2^24 with B = sum |u||w| per output: every partial sum of every order is an exact fp32 integer."""
    a, b = f64(np.abs(act)), f64(np.abs(wt))
    bound = F.conv2d(a, b, None, stride, pad) if transposed_to is None else G.conv2d_input(transposed_to, b, a, stride=stride, padding=pad)
    assert 0 < float(bound.max()) < TWO24
    return bound


def x3s_fwd_exact(shape, family, taps=None):
    n, cin, h, w, cout = shape
    r = rs(710 + family)
    u = crafted_activation(r, (n, cin, h, w), family)
    wfull, parts = R.weight_family(r, (cout, cin, 3, 3), family)
    xs0 = ops.x3s_split(dev(u))
    xs = [R.rotate_slices(xs0, i) for i in range(3)]
    for tap, blk, wt, seen in tap_block_cases(wfull, parts, 9, cin // 64, 1, taps):
        check_bound(u, wt, 1, 1)
        wf, _ = ops.x3s_pack_weights(dev(wt), transposed=False)
        for i in range(3):
            y, _ = ops.x3s_conv_fwd(xs[i], wf, n, h, w, cin, cout)
            assert_exact(y, F.conv2d(f64(u), f64(seen[i]), None, 1, 1),
                         "x3s fwd, family %d, tap %d, input block %d, activation slice %d" % (family, tap, blk, i))


@pytest.mark.parametrize("family", [1, 2])
@pytest.mark.parametrize("shape", X3S_SHAPES)
def test_x3s_forward_pairs_each_activation_slice_with_its_weight_slices(shape, family):
    x3s_fwd_exact(shape, family)


def test_x3s_forward_two_workgroup_configuration_exact():
    x3s_fwd_exact(X3S_TWO_WG, 1, taps=[5])


@pytest.mark.parametrize("family", [1, 2])
@pytest.mark.parametrize("shape", X3S_SHAPES)
def test_x3s_dgrad_pairs_each_gradient_slice_with_its_weight_slices(shape, family):
    n, cin, h, w, cout = shape
    r = rs(720 + family)
    g = crafted_activation(r, (n, cout, h, w), family)
    wfull, parts = R.weight_family(r, (cout, cin, 3, 3), family)
    d0 = ops.x3s_split(dev(g))
    ds = [R.rotate_slices(d0, i) for i in range(3)]
    for tap, blk, wt, seen in tap_block_cases(wfull, parts, 9, cout // 64, 0):
        check_bound(g, wt, 1, 1, transposed_to=(n, cin, h, w))
        _, wtr = ops.x3s_pack_weights(dev(wt), forward=False)
        for i in range(3):
            dx = ops.x3s_conv_dgrad(ds[i], wtr, n, h, w, cin, cout)
            assert_exact(dx, G.conv2d_input((n, cin, h, w), f64(seen[i]), f64(g), stride=1, padding=1),
                         "x3s dgrad, family %d, tap %d, output block %d, dy slice %d" % (family, tap, blk, i))


def x3q_weight_cases(r, cin, cout, family, axis):
    """Ten cases per block: taps 0 .. 8 of the 3 x 3 weight with a zero shortcut weight, then the 1 x 1 shortcut weight alone."""
    w3, p3 = R.weight_family(r, (cout, cin, 3, 3), family)
    w1, p1 = R.weight_family(r, (cout, cin, 1, 1), family)
    nblocks = (cin if axis == 1 else cout) // 64
    z3, z1 = np.zeros_like(w3), np.zeros_like(w1)
    for tap, blk, wt, seen in tap_block_cases(w3, p3, 9, nblocks, axis):
        yield tap, blk, wt, z1, seen, [z1.astype(np.float64)] * 3
    for _, blk, wt, seen in tap_block_cases(w1, p1, 1, nblocks, axis):
        yield 9, blk, z3, wt, [z3.astype(np.float64)] * 3, seen


@pytest.mark.parametrize("family", [1, 2])
@pytest.mark.parametrize("shape", X3Q_SHAPES)
def test_x3q_forward_pairs_each_activation_slice_with_its_weight_slices(shape, family):
    n, cin, h, w, cout = shape
    oh, ow = h // 2, w // 2
    assert dmcnet_amd._lib.load().dmc_x3q_supported(n, oh, ow, cin, cout)
    r = rs(730 + family)
    u = crafted_activation(r, (n, cin, h, w), family)
    xq0 = ops.x3q_split(dev(u))
    xq = [R.rotate_slices(xq0, i) for i in range(3)]
    for tap, blk, w3, w1, seen3, seen1 in x3q_weight_cases(r, cin, cout, family, 1):
        if tap < 9:
            check_bound(u, w3, 2, 1)
        else:
            check_bound(u, w1, 2, 0)
        wf, _ = ops.x3q_pack_weights(dev(w3), dev(w1), transposed=False)
        for i in range(3):
            y3, y1, _, _ = ops.x3q_conv_fwd(xq[i], wf, n, oh, ow, cin, cout)
            what = "x3q fwd %%s, family %d, tap %d, input block %d, activation slice %d" % (family, tap, blk, i)
            assert_exact(y3, F.conv2d(f64(u), f64(seen3[i]), None, 2, 1), what % "y3")
            assert_exact(y1, F.conv2d(f64(u), f64(seen1[i]), None, 2, 0), what % "y1")


@pytest.mark.parametrize("family", [1, 2])
@pytest.mark.parametrize("shape", X3Q_SHAPES)
def test_x3q_dgrad_pairs_each_gradient_slice_with_its_weight_slices(shape, family):
    n, cin, h, w, cout = shape
    oh, ow = h // 2, w // 2
    r = rs(740 + family)
    g3, g1 = crafted_activation(r, (n, cout, oh, ow), family), crafted_activation(r, (n, cout, oh, ow), family)
    d30, d10 = ops.x3s_split(dev(g3)), ops.x3s_split(dev(g1))
    d3, d1 = [R.rotate_slices(d30, i) for i in range(3)], [R.rotate_slices(d10, i) for i in range(3)]
    size = (n, cin, h, w)
    for tap, blk, w3, w1, seen3, seen1 in x3q_weight_cases(r, cin, cout, family, 0):
        if tap < 9:
            check_bound(g3, w3, 2, 1, transposed_to=size)
        else:
            check_bound(g1, w1, 2, 0, transposed_to=size)
        _, wt = ops.x3q_pack_weights(dev(w3), dev(w1), forward=False)
        for i in range(3):
            dx = ops.x3q_conv_dgrad(d3[i], d1[i], wt, n, oh, ow, cin, cout)
            want = G.conv2d_input(size, f64(seen3[i]), f64(g3), stride=2, padding=1) + \
                G.conv2d_input(size, f64(seen1[i]), f64(g1), stride=2, padding=0)
            assert_exact(dx, want, "x3q dgrad, family %d, tap %d, output block %d, dy slice %d" % (family, tap, blk, i))


# ================================================================ exact layer: in-loop-split kernels, one-hot operands
def lattice(shape, k, r):
    """[N, 1, H, W] mask of the pixels (y, x) = (oy, ox) mod k: any k x k window holds at most one of them."""
    n, _, h, w = shape
    oy, ox = r.randint(k), r.randint(k)
    m = np.zeros((n, 1, h, w), np.float32)
    m[:, :, oy::k, ox::k] = 1.0
    return m


def nhwc_run(x, w, dy, stride, pad, want):
    xg, wg = dev(x).requires_grad_("dx" in want), dev(w).requires_grad_("dw" in want)
    y = ops.conv_nhwc(xg, wg, stride, pad)
    out = {"y": y.detach()}
    if xg.requires_grad or wg.requires_grad:
        y.backward(dev(dy))
        out["dx"], out["dw"] = xg.grad, wg.grad
    return out


@pytest.mark.parametrize("conv_arith", [1], indirect=True)
@pytest.mark.parametrize("case", NHWC_SHAPES)
def test_conv_nhwc_one_hot_operands_come_back_bit_for_bit(case, conv_arith):
    n, cin, h, w, cout, k, stride = case
    pad = k // 2
    r = rs(750)
    oh, ow = R.out_size(h, k, stride, pad), R.out_size(w, k, stride, pad)
    xs, ys, ws = (n, cin, h, w), (n, cout, oh, ow), (cout, cin, k, k)
    gauss = lambda shape, s=1.0: (r.standard_normal(shape) * s).astype(np.float32)
    assert ops.conv_nhwc_supported(dev(np.zeros(xs)), dev(np.zeros(ws)), stride, pad)
    # forward, weight side: one nonzero weight per output channel -> y = x[shifted] * w; pins (1,0) (2,0) of the activation
    x, wt = gauss(xs), R.one_hot_weights(r, cout, cin, k)
    assert_exact(nhwc_run(x, wt, None, stride, pad, "")["y"], F.conv2d(f64(x), f64(wt), None, stride, pad), "fwd, one-hot weights")
    # forward, activation side: one channel per pixel on a k-spaced lattice -> one term per output; pins (0,1) (0,2)
    x, wt = R.one_hot_channels(r, xs) * lattice(xs, k, r), gauss(ws, 0.1)
    want = F.conv2d(f64(x), f64(wt), None, stride, pad)
    assert want.abs().max() > 0
    assert_exact(nhwc_run(x, wt, None, stride, pad, "")["y"], want, "fwd, one-hot activation")
    # data gradient, weight side: one nonzero weight per INPUT channel, dy in the role of x
    dy, wt = gauss(ys), np.ascontiguousarray(R.one_hot_weights(r, cin, cout, k).transpose(1, 0, 2, 3))
    assert_exact(nhwc_run(gauss(xs), wt, dy, stride, pad, ("dx",))["dx"], G.conv2d_input(xs, f64(wt), f64(dy), stride=stride, padding=pad),
                 "dgrad, one-hot weights")
    # data gradient, dy side
    dy, wt = R.one_hot_channels(r, ys) * lattice(ys, k, r), gauss(ws, 0.1)
    want = G.conv2d_input(xs, f64(wt), f64(dy), stride=stride, padding=pad)
    assert want.abs().max() > 0
    assert_exact(nhwc_run(gauss(xs), wt, dy, stride, pad, ("dx",))["dx"], want, "dgrad, one-hot dy")
    # weight gradient: one nonzero pixel per image in dy; output channel co lives in image co mod n, so each dw element is
    # ONE product x * dy (x full 24 bits): pins (1,0) (2,0) of x
    dy = np.zeros(ys, np.float32)
    for img in range(n):
        dy[img, img::n, r.randint(oh), r.randint(ow)] = r.choice([1.0, 2.0], size=len(range(img, cout, n))) * \
            r.choice([-1.0, 1.0], size=len(range(img, cout, n)))
    x = gauss(xs)
    want = dw_fp64(x, dy, ws, stride, pad)
    assert want.abs().max() > 0
    assert_exact(nhwc_run(x, gauss(ws), dy, stride, pad, ("dw",))["dw"], want, "wgrad, one-hot dy")
    # ... and the mirror image: one nonzero pixel per image in x (input channel ci in image ci mod n), dy full: (0,1) (0,2)
    x = np.zeros(xs, np.float32)
    for img in range(n):
        x[img, img::n, r.randint(h), r.randint(w)] = r.choice([1.0, 2.0], size=len(range(img, cin, n))) * \
            r.choice([-1.0, 1.0], size=len(range(img, cin, n)))
    dy = gauss(ys)
    want = dw_fp64(x, dy, ws, stride, pad)
    assert want.abs().max() > 0
    assert_exact(nhwc_run(x, gauss(ws), dy, stride, pad, ("dw",))["dw"], want, "wgrad, one-hot x")


# ================================================================ statistical layer: error tap by tap against the emulation
def operands(family, seed, a_shape, b_shape, a_axis, b_axis, b_scale=0.1):
    """Two fp32 arrays; the wide family scales the channels of axis a_axis / b_axis by 2^-6 .. 2^6 and cuts a tenth to bf16."""
    r = rs(seed)
    if family == "gauss":
        return r.standard_normal(a_shape).astype(np.float32), (r.standard_normal(b_shape) * b_scale).astype(np.float32)
    return R.wide_range(r, a_shape, a_axis), (R.wide_range(r, b_shape, b_axis) * np.float32(b_scale)).astype(np.float32)


def hold_to_emulation(what, got, a, b, order, conv32=None):
    """got [M, C] against the emulation of a [M, K] @ b [K, C], per 64-wide (merged to >= 1000 outputs) block of C."""
    ref, bound = R.fp64_and_bound(a, b)
    emu = R.emulate(a, b, order=order)
    emu_max = R.max_metric(emu, ref, bound)
    worst_rms = worst_max = 0.0
    for c0, c1 in R.channel_groups(ref.shape[1], ref.shape[0]):
        sl = (slice(None), slice(c0, c1))
        assert ref[sl].size >= R.MIN_GROUP
        worst_rms = max(worst_rms, R.rms_metric(got[sl], ref[sl], bound[sl]) / R.rms_metric(emu[sl], ref[sl], bound[sl]))
        worst_max = max(worst_max, R.max_metric(got[sl], ref[sl], bound[sl]) / emu_max)
    extra = "old metric %.2e" % R.old_metric(got, ref)
    if conv32 is not None:
        extra += "  (F.conv2d fp32 on the CPU: rms %.2e, emulation %.2e)" % (R.rms_metric(conv32, ref, bound), R.rms_metric(emu, ref, bound))
    report(what, worst_rms, worst_max, extra)


def tap_columns(tap, c):
    return slice(tap * c, (tap + 1) * c)


def fwd_like_statistics(name, run, act, wt, k, stride, pad, dgrad_to=None, taps=None):
    """One launch pair per tap: ``run(weight with one live tap)`` -> [M, C] rows; the emulation contracts over that tap only."""
    if dgrad_to is None:
        col, mat, cred = R.im2col(act, k, stride, pad), R.weight_matrix(wt), wt.shape[1]
    else:
        col, mat, cred = R.im2col_dgrad(act, k, stride, pad, *dgrad_to), R.weight_matrix_dgrad(wt), wt.shape[0]
    for tap in (range(k * k) if taps is None else taps):
        w1 = R.only_tap(wt, tap)
        got, again = run(w1), run(w1)
        assert torch.equal(got, again)
        conv32 = None
        if dgrad_to is None:
            conv32 = rows(F.conv2d(torch.from_numpy(act), torch.from_numpy(w1), None, stride, pad))
        ks = tap_columns(tap, cred)
        hold_to_emulation("%s tap %d" % (name, tap), rows(got), col[:, ks], mat[ks], R.ORDER_WEIGHT_OUTER, conv32)


def wgrad_statistics(name, dw, x, dy, k, stride, pad, dilation=1):
    """dw [Cout, Cin, k, k] of one launch on dense operands, grouped by tap x 64-wide output-channel block (taps merged where
    a block holds fewer than 1000 outputs); K runs over the pixels.  A group without a single live output (a dilated tap that
    lies outside the frame for every pixel) must be all zeros; every other group must hold >= 1000 LIVE outputs."""
    cout, cin = dw.shape[0], dw.shape[1]
    a, b = R.wgrad_operands(x, dy, k, stride, pad, dilation)
    got = dw.detach().double().cpu().permute(0, 2, 3, 1).reshape(cout, k * k * cin).numpy()
    block = min(64, cout)
    per_tap = block * cin
    tap_groups = R.channel_groups(k * k, per_tap, width=1) if k > 1 else [(0, 1)]
    a_p, b_p = R.pad_k(a, b)
    ref, bound = R.fp64_and_bound(a, b)
    emu = R.six_product(R.split(a_p), R.split(b_p), order=R.ORDER_SMALL_FIRST)
    emu_max = R.max_metric(emu, ref, bound)
    worst_rms = worst_max = 0.0
    for t0, t1 in tap_groups:
        for c0, c1 in R.channel_groups(cout, (t1 - t0) * cin):
            sl = (slice(c0, c1), slice(t0 * cin, t1 * cin))
            assert ref[sl].size >= R.MIN_GROUP
            if not (bound[sl] > 0).any():
                assert not got[sl].any() and not np.isnan(got[sl]).any(), (name, "taps", t0, t1, "is not all zeros")
                continue
            assert int((bound[sl] > 0).sum()) >= R.MIN_GROUP
            worst_rms = max(worst_rms, R.rms_metric(got[sl], ref[sl], bound[sl]) / R.rms_metric(emu[sl], ref[sl], bound[sl]))
            worst_max = max(worst_max, R.max_metric(got[sl], ref[sl], bound[sl]) / emu_max)
    report(name, worst_rms, worst_max, "old metric %.2e" % R.old_metric(got, ref))


@pytest.mark.parametrize("family", ["gauss", "wide"])
@pytest.mark.parametrize("shape", X3S_SHAPES + [DEEP_X3S, X3S_TWO_WG])
def test_x3s_forward_error_tap_by_tap(shape, family):
    n, cin, h, w, cout = shape
    x, wt = operands(family, 801, (n, cin, h, w), (cout, cin, 3, 3), 1, 1)
    xs = ops.x3s_split(dev(x))

    def run(w1):
        wf, _ = ops.x3s_pack_weights(dev(w1), transposed=False)
        return ops.x3s_conv_fwd(xs, wf, n, h, w, cin, cout)[0]
    fwd_like_statistics("x3s-fwd %s %s" % (shape, family), run, x, wt, 3, 1, 1, taps=[5] if shape == X3S_TWO_WG else None)


@pytest.mark.parametrize("family", ["gauss", "wide"])
@pytest.mark.parametrize("shape", X3S_SHAPES + [DEEP_X3S])
def test_x3s_dgrad_error_tap_by_tap(shape, family):
    n, cin, h, w, cout = shape
    g, wt = operands(family, 802, (n, cout, h, w), (cout, cin, 3, 3), 1, 0)
    ds = ops.x3s_split(dev(g))

    def run(w1):
        _, wtr = ops.x3s_pack_weights(dev(w1), forward=False)
        return ops.x3s_conv_dgrad(ds, wtr, n, h, w, cin, cout)
    fwd_like_statistics("x3s-dgrad %s %s" % (shape, family), run, g, wt, 3, 1, 1, dgrad_to=(h, w))


@pytest.mark.parametrize("family", ["gauss", "wide"])
@pytest.mark.parametrize("shape", X3S_SHAPES + [DEEP_X3S])
def test_x3s_wgrad_error_tap_by_tap(shape, family):
    n, cin, h, w, cout = shape
    x, g = operands(family, 803, (n, cin, h, w), (n, cout, h, w), 1, 1, b_scale=1.0)
    xs, ds = ops.x3s_split(dev(x)), ops.x3s_split(dev(g))
    dw = ops.x3s_conv_wgrad(xs, ds, n, h, w, cin, cout)
    assert torch.equal(dw, ops.x3s_conv_wgrad(xs, ds, n, h, w, cin, cout))
    wgrad_statistics("x3s-wgrad %s %s" % (shape, family), dw, x, g, 3, 1, 1)


@pytest.mark.parametrize("family", ["gauss", "wide"])
@pytest.mark.parametrize("shape", X3Q_SHAPES + [DEEP_X3Q])
def test_x3q_forward_error_tap_by_tap(shape, family):
    n, cin, h, w, cout = shape
    oh, ow = h // 2, w // 2
    x, w3 = operands(family, 811, (n, cin, h, w), (cout, cin, 3, 3), 1, 1)
    _, w1 = operands(family, 812, (1,) * 4, (cout, cin, 1, 1), 1, 1, b_scale=0.2)
    xq = ops.x3q_split(dev(x))
    z3, z1 = np.zeros_like(w3), np.zeros_like(w1)

    def run3(wt):
        wf, _ = ops.x3q_pack_weights(dev(wt), dev(z1), transposed=False)
        y3, y1, _, _ = ops.x3q_conv_fwd(xq, wf, n, oh, ow, cin, cout)
        assert not bool(y1.any())
        return y3

    def run1(wt):
        wf, _ = ops.x3q_pack_weights(dev(z3), dev(wt), transposed=False)
        y3, y1, _, _ = ops.x3q_conv_fwd(xq, wf, n, oh, ow, cin, cout)
        assert not bool(y3.any())
        return y1
    fwd_like_statistics("x3q-fwd3 %s %s" % (shape, family), run3, x, w3, 3, 2, 1)
    fwd_like_statistics("x3q-fwd1 %s %s" % (shape, family), run1, x, w1, 1, 2, 0)


@pytest.mark.parametrize("family", ["gauss", "wide"])
@pytest.mark.parametrize("shape", X3Q_SHAPES + [DEEP_X3Q])
def test_x3q_dgrad_error_tap_by_tap(shape, family):
    n, cin, h, w, cout = shape
    oh, ow = h // 2, w // 2
    g3, w3 = operands(family, 821, (n, cout, oh, ow), (cout, cin, 3, 3), 1, 0)
    g1, w1 = operands(family, 822, (n, cout, oh, ow), (cout, cin, 1, 1), 1, 0, b_scale=0.2)
    d3, d1 = ops.x3s_split(dev(g3)), ops.x3s_split(dev(g1))
    z3, z1 = np.zeros_like(w3), np.zeros_like(w1)

    def run3(wt):
        _, wtr = ops.x3q_pack_weights(dev(wt), dev(z1), forward=False)
        return ops.x3q_conv_dgrad(d3, d1, wtr, n, oh, ow, cin, cout)

    def run1(wt):
        _, wtr = ops.x3q_pack_weights(dev(z3), dev(wt), forward=False)
        return ops.x3q_conv_dgrad(d3, d1, wtr, n, oh, ow, cin, cout)
    fwd_like_statistics("x3q-dgrad3 %s %s" % (shape, family), run3, g3, w3, 3, 2, 1, dgrad_to=(h, w))
    fwd_like_statistics("x3q-dgrad1 %s %s" % (shape, family), run1, g1, w1, 1, 2, 0, dgrad_to=(h, w))


@pytest.mark.parametrize("family", ["gauss", "wide"])
@pytest.mark.parametrize("shape", X3Q_WGRAD_SHAPES + [DEEP_X3Q])
def test_x3q_wgrad_error_tap_by_tap(shape, family):
    n, cin, h, w, cout = shape
    oh, ow = h // 2, w // 2
    assert x3q_wgrad_ok(shape)
    x, g3 = operands(family, 831, (n, cin, h, w), (n, cout, oh, ow), 1, 1, b_scale=1.0)
    _, g1 = operands(family, 832, (1,) * 4, (n, cout, oh, ow), 1, 1, b_scale=1.0)
    xq, d3, d1 = ops.x3q_split(dev(x)), ops.x3s_split(dev(g3)), ops.x3s_split(dev(g1))
    dw3, dw1 = ops.x3q_conv_wgrad(xq, d3, d1, n, oh, ow, cin, cout)
    again = ops.x3q_conv_wgrad(xq, d3, d1, n, oh, ow, cin, cout)
    assert torch.equal(dw3, again[0]) and torch.equal(dw1, again[1])
    wgrad_statistics("x3q-wgrad3 %s %s" % (shape, family), dw3, x, g3, 3, 2, 1)
    wgrad_statistics("x3q-wgrad1 %s %s" % (shape, family), dw1, x, g1, 1, 2, 0)


@pytest.mark.parametrize("conv_arith", [1], indirect=True)
@pytest.mark.parametrize("family", ["gauss", "wide"])
@pytest.mark.parametrize("case", NHWC_SHAPES + [DEEP_NHWC])
def test_conv_nhwc_error_tap_by_tap(case, family, conv_arith):
    n, cin, h, w, cout, k, stride = case
    pad = k // 2
    oh, ow = R.out_size(h, k, stride, pad), R.out_size(w, k, stride, pad)
    x, wt = operands(family, 841, (n, cin, h, w), (cout, cin, k, k), 1, 1)
    g, wd = operands(family, 842, (n, cout, oh, ow), (cout, cin, k, k), 1, 0)
    gw = operands(family, 843, (1,) * 4, (n, cout, oh, ow), 1, 1, b_scale=1.0)[1]
    name = "nhwc-%%s %s %s" % (case, family)
    fwd_like_statistics(name % "fwd", lambda w1: nhwc_run(x, w1, None, stride, pad, "")["y"], x, wt, k, stride, pad)
    fwd_like_statistics(name % "dgrad", lambda w1: nhwc_run(x, w1, g, stride, pad, ("dx",))["dx"], g, wd, k, stride, pad, dgrad_to=(h, w))
    dw = nhwc_run(x, wt, gw, stride, pad, ("dw",))["dw"]
    assert torch.equal(dw, nhwc_run(x, wt, gw, stride, pad, ("dw",))["dw"])
    wgrad_statistics(name % "wgrad", dw, x, gw, k, stride, pad)
