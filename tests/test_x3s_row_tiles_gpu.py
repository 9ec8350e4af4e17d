"""GPU tests of tile configuration 5 of the pre-split convolutions (dmc-net_amd/csrc/conv_x3s.hip): 512 pixel slots, eight waves
of 64 pixels x 64 channels, tiles that start on image-row boundaries (stride (512 // W) * W pixels).

Option conv_cfg = 107 forces it wherever its patch fits, 108 never takes it (the choice without it).  Every output element sums the
same products in the same order in every tile configuration, so the forward result, the stride-1 data gradient (with and
without addend, with and without the linked BatchNorm-backward sums) and the eval-mode epilogue are compared with torch.equal;
the statistics partials group pixels differently (other rows) and their column sums agree to fp64 rounding,
<= 1e-12 * max|sum| -- the bar of test_x3s_two_workgroups_per_cu_configuration.  The shapes are the smallest that reach the cases: a last
tile of 224 of 504 pixels, tiles crossing images, two column blocks, strides 504 = 36 rows of 14 and 511 = 73 rows of 7 (more
images than rows per tile), the 8 unused slots behind a 504-pixel tile and the one behind 511."""
import contextlib
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import dmcnet_amd
from dmcnet_amd import ops

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CL = torch.channels_last
ROW, PARENT = 107, 108


def rnd(seed, shape):
    return torch.from_numpy(np.random.RandomState(seed).standard_normal(shape).astype(np.float32))


def rel_err(a, b):
    a, b = a.detach().double().cpu(), torch.as_tensor(b).double().cpu()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))


@contextlib.contextmanager
def conv_cfg(value):
    L, lib = dmcnet_amd._lib, dmcnet_amd._lib.load()
    before = lib.dmc_get_option(b"conv_cfg")
    L.check(lib.dmc_set_option(b"conv_cfg", value), "dmc_set_option")
    try:
        yield lib
    finally:
        L.check(lib.dmc_set_option(b"conv_cfg", before), "dmc_set_option")


def stride(w):
    return (512 // w) * w


def blocks(n, h, w):
    return -(-n * h * w // stride(w))


@functools.lru_cache(maxsize=None)
def operands(case):
    """Inputs of one shape, their slice tensors and packed weights (device), made once."""
    n, cin, h, w, cout = case
    x, wt, go = rnd(811, (n, cin, h, w)), rnd(812, (cout, cin, 3, 3)) * 0.1, rnd(813, (n, cout, h, w))
    xs = ops.x3s_split(x.to(DEV).contiguous(memory_format=CL))
    dys = ops.x3s_split(go.to(DEV).contiguous(memory_format=CL))
    wf, wtr = ops.x3s_pack_weights(wt.to(DEV).contiguous(memory_format=CL))
    return x, wt, xs, dys, wf, wtr


CASES = [
    (2, 64, 56, 56, 64),        # tiles cross the image boundary; last tile 224 of 504 pixels
    (3, 128, 56, 56, 128),      # two column blocks; K = 128
    (5, 64, 14, 14, 64),        # stride 504 = 36 rows: a tile spans three images
    (11, 64, 7, 7, 128),        # stride 511: more images than rows per tile
]
WIDE = CASES[0]


@pytest.mark.parametrize("case", CASES)
def test_row_tiles_forward_and_data_gradient_are_bitwise_the_parent_choice(case):
    n, cin, h, w, cout = case
    x, wt, xs, dys, wf, wtr = operands(case)
    out = {}
    for cfg in (ROW, PARENT):
        with conv_cfg(cfg) as lib:
            nblk = lib.dmc_x3s_conv_stat_blocks(n, h, w, cout)
            y, part = ops.x3s_conv_fwd(xs, wf, n, h, w, cin, cout, want_stats=True)
            dx = ops.x3s_conv_dgrad(dys, wtr, n, h, w, cin, cout)
            out[cfg] = (y, dx, part.sum(0), nblk)
    assert out[ROW][3] == blocks(n, h, w) and out[PARENT][3] != out[ROW][3]      # configuration 5 was really taken, and only under 107
    assert torch.equal(out[ROW][0], out[PARENT][0])
    assert torch.equal(out[ROW][1], out[PARENT][1])
    gap, top = float((out[ROW][2] - out[PARENT][2]).abs().max()), float(out[PARENT][2].abs().max())
    print("statistics sums: max gap %.3e, max |sum| %.3e" % (gap, top))
    assert gap <= 1e-12 * top
    err = rel_err(out[ROW][0], F.conv2d(x.double(), wt.double(), None, 1, 1))
    print("forward against fp64: %.3e" % err)
    assert err < 1e-5


def test_row_tiles_data_gradient_with_addend():
    n, cin, h, w, cout = WIDE
    _, _, _, dys, _, wtr = operands(WIDE)
    add = rnd(814, (n, cin, h, w)).to(DEV).contiguous(memory_format=CL)
    dx = {}
    for cfg in (ROW, PARENT):
        with conv_cfg(cfg):
            dx[cfg] = ops.x3s_conv_dgrad(dys, wtr, n, h, w, cin, cout, addend=add)
            plain = ops.x3s_conv_dgrad(dys, wtr, n, h, w, cin, cout)
        assert torch.equal(dx[cfg], plain + add)                # added exactly once, in fp32
    assert torch.equal(dx[ROW], dx[PARENT])


def test_row_tiles_linked_batchnorm_backward_sums():
    """dmc_x3s_conv_dgrad_bnb: dx bitwise, both column sums to fp64 rounding, and exactly dmc_x3s_conv_stat_blocks rows written
    (the buffer has four more, which keep their fill)."""
    L = dmcnet_amd._lib
    n, cin, h, w, cout = WIDE
    m = n * h * w
    _, _, _, dys, _, wtr = operands(WIDE)
    add = rnd(815, (n, cin, h, w)).to(DEV).contiguous(memory_format=CL)
    bn_y = rnd(816, (m, cin)).to(DEV)
    stats = torch.cat([bn_y.mean(0), 1.0 / (bn_y.var(0, unbiased=False) + 1e-5).sqrt()]).contiguous()
    gamma, beta = (rnd(817, (cin,)) * 0.5 + 1).to(DEV), (rnd(818, (cin,)) * 0.2).to(DEV)
    out = {}
    for cfg in (ROW, PARENT):
        with conv_cfg(cfg) as lib:
            nblk = lib.dmc_x3s_conv_stat_blocks(n, h, w, cin)
            part = torch.full((nblk + 4, cin, 2), float("nan"), dtype=torch.float64, device=DEV)
            dx = torch.empty((n, cin, h, w), device=DEV).contiguous(memory_format=CL)
            dgamma, dbeta = torch.empty(cin, device=DEV), torch.empty(cin, device=DEV)
            L.check(lib.dmc_x3s_conv_dgrad_bnb(L.ptr(dys), L.ptr(wtr), L.ptr(add), L.ptr(dx), L.ptr(bn_y), L.ptr(stats), L.ptr(gamma),
                                               L.ptr(beta), None, 1, L.ptr(part), nblk, L.ptr(dgamma), L.ptr(dbeta), n, h, w, cin, cout,
                                               ops._stream()), "dmc_x3s_conv_dgrad_bnb")
            torch.cuda.synchronize()
            assert not bool(torch.isnan(part[:nblk]).any()) and bool(torch.isnan(part[nblk:]).all())
            out[cfg] = (dx, part[:nblk].sum(0), nblk, dgamma, dbeta)
    assert out[ROW][2] == blocks(n, h, w) and out[PARENT][2] != out[ROW][2]
    assert torch.equal(out[ROW][0], out[PARENT][0])
    for col, name in ((0, "sum d"), (1, "sum d xhat")):
        a, b = out[ROW][1][:, col], out[PARENT][1][:, col]
        gap, top = float((a - b).abs().max()), float(b.abs().max())
        print("%s: max gap %.3e, max |sum| %.3e" % (name, gap, top))
        assert gap <= 1e-12 * top
    # the reduced fp32 results are those sums
    assert rel_err(out[ROW][4], out[ROW][1][:, 0]) < 1e-6 and rel_err(out[ROW][3], out[ROW][1][:, 1]) < 1e-6


def test_row_tiles_eval_epilogue_is_bitwise_the_parent_choice():
    L = dmcnet_amd._lib
    n, cin, h, w, cout = WIDE
    m = n * h * w
    _, _, xs, _, wf, _ = operands(WIDE)
    stats = torch.cat([rnd(819, (cout,)) * 0.1, rnd(820, (cout,)).abs() + 0.5]).to(DEV)
    gamma, beta = (rnd(821, (cout,)) * 0.5 + 1).to(DEV), rnd(822, (cout,)).to(DEV)
    res = rnd(823, (m, cout)).to(DEV)
    out = {}
    for cfg in (ROW, PARENT):
        with conv_cfg(cfg) as lib:
            y = torch.empty((m, cout), device=DEV)
            ys = torch.empty(lib.dmc_x3s_slices_bytes(m, cout), dtype=torch.uint8, device=DEV)
            L.check(lib.dmc_x3s_conv_bn_eval(L.ptr(xs), L.ptr(wf), L.ptr(stats), L.ptr(gamma), L.ptr(beta), L.ptr(res), L.ptr(y), L.ptr(ys),
                                             0, 1, n, h, w, cin, cout, ops._stream()), "dmc_x3s_conv_bn_eval")
            out[cfg] = (y, ys)
    assert torch.equal(out[ROW][0], out[PARENT][0]) and torch.equal(out[ROW][1], out[PARENT][1])
    assert float(out[ROW][0].min()) == 0.0 and float(out[ROW][0].max()) > 0.0       # the ReLU was applied to a real result


def test_row_tiles_query_and_launch_agree():
    """dmc_x3s_conv_stat_blocks counts the tiles of the stride; a partials buffer sized under the other option is refused."""
    L = dmcnet_amd._lib
    n, cin, h, w, cout = WIDE
    _, _, xs, _, wf, _ = operands(WIDE)
    y = torch.empty((n, cout, h, w), device=DEV).contiguous(memory_format=CL)
    nblk = {}
    for cfg in (ROW, PARENT):
        with conv_cfg(cfg) as lib:
            nblk[cfg] = lib.dmc_x3s_conv_stat_blocks(n, h, w, cout)
    with conv_cfg(ROW) as lib:
        for frames in (1, 2, 3, 40):
            assert lib.dmc_x3s_conv_stat_blocks(frames, 56, 56, 64) == -(-frames * 3136 // 504)
    assert nblk[ROW] != nblk[PARENT]
    for sized, launched in ((PARENT, ROW), (ROW, PARENT)):
        part = torch.empty((nblk[sized], cout, 2), dtype=torch.float64, device=DEV)
        with conv_cfg(launched) as lib:
            rc = lib.dmc_x3s_conv_fwd(L.ptr(xs), L.ptr(wf), L.ptr(y), L.ptr(part), nblk[sized], n, h, w, cin, cout, ops._stream())
            assert rc != 0 and b"x3s_conv" in lib.dmc_last_error()


def test_default_rule_takes_row_tiles_where_they_save_rounds():
    """56-wide maps, 1.8 x the rounds of 256 CUs of configuration 5 below those of the 256-pixel tiles (the measured frame counts of
    profiles/x3s_row_tiles_ab_frames.txt): 120 frames = 3 rounds against 6 -> taken; 96 = 3 against 5, 83 = 3 against 4 -> not."""
    lib = dmcnet_amd._lib.load()
    for frames, taken in ((24, True), (41, True), (120, True), (240, True), (12, False), (62, False), (83, False), (96, False)):
        with conv_cfg(PARENT):
            parent = lib.dmc_x3s_conv_stat_blocks(frames, 56, 56, 64)
        assert lib.dmc_x3s_conv_stat_blocks(frames, 56, 56, 64) == (blocks(frames, 56, 56) if taken else parent), frames
        assert parent != blocks(frames, 56, 56)


@pytest.mark.parametrize("shape", [(2, 56, 56, 64), (6, 14, 14, 128), (37, 14, 14, 64), (5, 7, 7, 64), (42, 14, 14, 512), (3, 28, 28, 128)])
def test_small_shapes_keep_the_parent_default(shape):
    """The default rule takes configuration 5 only where it was measured faster: the shapes of the other suites do
    not change their tiles."""
    lib = dmcnet_amd._lib.load()
    default = lib.dmc_x3s_conv_stat_blocks(*shape)
    with conv_cfg(PARENT):
        assert lib.dmc_x3s_conv_stat_blocks(*shape) == default
