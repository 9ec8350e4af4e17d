"""GPU: every tile configuration of conv3_kernel (bf16x3) and conv2_kernel (fp32 MFMA) of conv_nhwc.hip against fp64.

The kernels pick their tile by problem size, and the sizes of the other unit tests pick two configurations each
(tests/test_conv_nhwc_plans_cpu.py keeps the record): the 256-pixel 8-wave tiles, the 192 x 128 tile and the rest -- each with an
epilogue instantiation of its own -- ran only in the B = 40 end-to-end steps, behind bars on logits and losses.  Here the option
conv_cfg forces each configuration in turn on five ragged shapes small enough for an instant fp64 reference
(tests/conv_nhwc_plans.py: CFG_SHAPES, cfg_sweep), and under each:

  (a) forward with the whole epilogue (bias, LeakyReLU, keep mask, statistics partials) into NaN-filled memory against
      keep * leaky_relu(conv64 + bias, 0.2) at 1e-5; the row count of the partials equals the restated ceil(M / BM) -- the launch
      refuses any other, so the forced tile is the one that ran; rows behind the partials stay NaN;
  (b) the partials summed over rows against the fp64 sums and sums of squares of the STORED output at 1e-9;
  (c) the data gradient (one launch per parity class of a stride-2 input map, each with its own tile count) against fp64
      autograd at 1e-5; stride 1 under bf16x3: addend= gives exactly dx + addend;
  (d) a second run, through ops._conv_fwd / ops._conv_dgrad, bit-identical.

A failure names the configuration, the worst pixel tile (pixel // BM), the channel tile and whether the worst pixel lies in the
last, partial tile.  Bar: max |got - ref| <= 1e-5 max |ref|, the project's own for these kernels
(test_conv_nhwc_fwd_dgrad_wgrad_vs_fp64).  Measured on an MI355X over the 89 cases: forward 3.7e-07 .. 1.7e-06, data gradient
5.0e-07 .. 1.6e-06, the same range under either arithmetic.

The statistics of (b) were per-lane fp32 sums (and fp32 squares) until this file was written: 8e-9 of the sum of squares at
M = 297.  The epilogues now add the stored values and their squares in fp64."""
import pytest
import torch
import torch.nn.functional as F

import dmcnet_amd
from dmcnet_amd import ops
from tests import conv_nhwc_plans as P

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CL = torch.channels_last
L = dmcnet_amd._lib
NAN = float("nan")
BAR = 1e-5

_REF = {}


@pytest.fixture(scope="module", autouse=True)
def drop_references():
    yield
    _REF.clear()


@pytest.fixture
def options():
    """set(conv_arith, conv_cfg); both are process-wide and restored when the test is done."""
    lib = L.load()
    before = {name: lib.dmc_get_option(name) for name in (b"conv_arith", b"conv_cfg")}

    def set_options(arith, cfg):
        L.check(lib.dmc_set_option(b"conv_arith", arith), "dmc_set_option")
        L.check(lib.dmc_set_option(b"conv_cfg", cfg), "dmc_set_option")
        return lib

    yield set_options
    for name, value in before.items():
        L.check(lib.dmc_set_option(name, value), "dmc_set_option")


def cl(t):
    return t.to(DEV).contiguous(memory_format=CL)


def reference(shape):
    """fp64 on the CPU, once per shape: y = keep * leaky_relu(conv + bias), dx = the convolution's data gradient for dy = go."""
    if shape in _REF:
        return _REF[shape]
    n, cin, h, w, cout, k, stride = shape
    oh, ow = P.out_map(shape)
    g = torch.Generator().manual_seed(500 + P.CFG_SHAPES.index(shape))
    r = {"x": torch.randn((n, cin, h, w), generator=g), "w": torch.randn((cout, cin, k, k), generator=g) * 0.1,
         "go": torch.randn((n, cout, oh, ow), generator=g), "bias": torch.randn(cout, generator=g) * 0.5,
         "keep": (torch.rand((n, cout), generator=g) < 0.75).float() / 0.75, "add": torch.randn((n, cin, h, w), generator=g)}
    assert (r["keep"] == 0).any() and (r["keep"] > 1).any()
    xo = r["x"].double().requires_grad_(True)
    pre = F.conv2d(xo, r["w"].double(), None, stride, k // 2)
    (pre * r["go"].double()).sum().backward()
    r["y"] = F.leaky_relu(pre.detach() + r["bias"].double()[None, :, None, None], 0.2) * r["keep"].double()[:, :, None, None]
    r["dx"] = xo.grad
    r["dev"] = {name: (cl(r[name]) if r[name].dim() == 4 else r[name].to(DEV).contiguous()) for name in ("x", "w", "go", "bias", "keep", "add")}
    _REF[shape] = r
    return r


def worst_tile(err, choice):
    """err [N][C][rows][columns] of ONE launch's output pixels: where the largest error is, in the launch's tiles."""
    n, c, rows, cols = err.shape
    e = torch.nan_to_num(err, nan=float("inf")).permute(0, 2, 3, 1).reshape(-1, c)
    pix, ch = divmod(int(e.argmax()), c)
    m = e.shape[0]
    assert m == choice.m
    tile, tiles = pix // choice.bm, P.ceil_div(m, choice.bm)
    partial = m % choice.bm != 0 and tile == tiles - 1
    return ("%s configuration %s (%d x %d): worst pixel %d = pixel tile %d of %d, channel %d = channel tile %d; %s"
            % (choice.kernel, choice.cfg, choice.bm, choice.bn, pix, tile, tiles, ch, ch // choice.bn,
               "in the last, partial tile (%d pixels)" % (m % choice.bm) if partial else "in a full tile"))


def assert_close(got, want, what, tag, parts):
    """parts: [(label, slices of the two map axes, Choice)], the launches that wrote got."""
    want = want.to(DEV)
    err = (got.double() - want).abs()
    scale = float(want.abs().max())
    e = float(torch.nan_to_num(err, nan=float("inf")).max()) / scale
    print("%s %s: rel_err %.3e" % (what, tag, e))
    if e <= BAR:
        return
    worst = max(parts, key=lambda p: float(torch.nan_to_num(err[:, :, p[1][0], p[1][1]], nan=float("inf")).max()))
    label, (ys, xs), choice = worst
    pytest.fail("%s %s: rel_err %.3e > %.0e; %s: %s" % (what, tag, e, BAR, label, worst_tile(err[:, :, ys, xs], choice)))


def run_fwd_nan(shape, d, nblk):
    """The forward through the C ABI into NaN-filled memory, two guard rows behind the partials."""
    lib = L.load()
    n, cin, h, w, cout, k, stride = shape
    oh, ow = P.out_map(shape)
    y = torch.empty((n, cout, oh, ow), dtype=torch.float32, device=DEV, memory_format=CL).fill_(NAN)
    part = torch.full((nblk + 2, cout, 2), NAN, dtype=torch.float64, device=DEV)
    wpack = ops._floats(lib.dmc_conv_nhwc_wt_bytes(cin, cout, k, k), DEV)
    L.check(lib.dmc_conv_nhwc_fwd(L.ptr(d["x"]), L.ptr(d["w"]), L.ptr(wpack), L.ptr(d["bias"]), L.ptr(d["keep"]), L.ptr(y),
                                  L.ptr(part), nblk, n, h, w, cin, cout, k, k, stride, k // 2, 1, ops._stream()), "dmc_conv_nhwc_fwd")
    return y, part


def run_dgrad_nan(shape, d):
    lib = L.load()
    n, cin, h, w, cout, k, stride = shape
    dx = torch.empty((n, cin, h, w), dtype=torch.float32, device=DEV, memory_format=CL).fill_(NAN)
    wt = ops._floats(lib.dmc_conv_nhwc_wt_bytes(cin, cout, k, k), DEV)
    L.check(lib.dmc_conv_nhwc_dgrad(L.ptr(d["go"]), L.ptr(d["w"]), L.ptr(wt), L.ptr(dx), n, h, w, cin, cout, k, k, stride, k // 2,
                                    ops._stream()), "dmc_conv_nhwc_dgrad")
    return dx


def check_statistics(part, nblk, y):
    assert bool(torch.isfinite(part[:nblk]).all()), "a statistics row of the launch was not written"
    assert bool(torch.isnan(part[nblk:]).all()), "the launch wrote behind its statistics rows"
    s = part[:nblk].sum(0).cpu()
    yd = y.double().permute(1, 0, 2, 3).reshape(y.shape[1], -1).cpu()
    assert float((s[:, 0] - yd.sum(1)).abs().max()) <= 1e-9 * float(yd.abs().sum(1).max())
    assert float((s[:, 1] - (yd * yd).sum(1)).abs().max()) <= 1e-9 * float((yd * yd).sum(1).max())


def _id(param):
    shape, arith, cfg = param
    return "%s-arith%d-cfg%d" % ("x".join(str(v) for v in shape), arith, cfg)


@pytest.mark.parametrize("param", P.cfg_sweep(), ids=_id)
def test_forced_tile_configuration_vs_fp64(param, options):
    shape, arith, cfg = param
    n, cin, h, w, cout, k, stride = shape
    pad = k // 2
    r = reference(shape)
    d = r["dev"]
    lib = options(arith, cfg)
    tag = "%s conv_arith %d conv_cfg %d" % (shape, arith, cfg)
    full = (slice(None), slice(None))

    # (a), (b) forward
    choice = P.fwd_choice(shape, arith, cfg)
    want_blocks = P.ceil_div(choice.m, choice.bm)
    nblk = lib.dmc_conv_nhwc_stat_blocks(n, h, w, cin, cout, k, stride, pad)
    assert nblk == want_blocks, (tag, choice)
    y, part = run_fwd_nan(shape, d, nblk)
    assert_close(y, r["y"], "forward", tag, [("the launch", full, choice)])
    check_statistics(part, nblk, y)

    # (c) data gradient: the launches of the parity classes
    classes = P.dgrad_choices(shape, arith, cfg)
    assert [t for _, _, t, _ in classes] == ([k * k] if stride == 1 else [1, 2, 2, 4] if k == 3 else [1, 0, 0, 0])
    dx = run_dgrad_nan(shape, d)
    parts = [("parity class (%d, %d) of %d, %d taps" % (py, px, len(classes), t), (slice(py, None, stride), slice(px, None, stride)), c)
             for py, px, t, c in classes]
    assert_close(dx, r["dx"], "data gradient", tag, parts)
    if stride == 1 and arith == 1:
        assert torch.equal(ops._conv_dgrad(d["go"], d["w"], d["x"].shape, stride, pad, addend=d["add"]), dx + d["add"]), tag

    # (d) again, through the wrappers the training path calls
    y2, part2, nblk2 = ops._conv_fwd(d["x"], d["w"], d["bias"], d["keep"], stride, pad, 1, True)
    assert nblk2 == want_blocks and torch.equal(y, y2) and torch.equal(part[:nblk], part2), tag
    assert torch.equal(dx, ops._conv_dgrad(d["go"], d["w"], d["x"].shape, stride, pad)), tag


def test_the_sweep_launches_every_configuration():
    """Every case of launch_conv3 and of launch_conv's conv2 switch is taken by some launch above."""
    swept = P.swept_configurations()
    assert swept["conv3"] == set(P.V3_TILES) and swept["conv2"] == set(P.V2_TILES)
