"""GPU: EstimatorDenseNet / EstimatorDenseNetSmall in eval mode on the kernels of csrc/dense_eval.hip.

Through the C ABI unless stated otherwise; the reference side is tests/dense_ref.py (the fp64 stack with torch.cat, the buffer
builder made from ops.dense_eval_layout's own description) and tests/x3_ref.py (the six-product arithmetic).

  1. dmc_dense_pack_weights against x3_ref.ctx_pack, bit for bit, at every layer shape of EstimatorDenseNet.
  2. dmc_dense_ingest: the 5 values, eleven +0.0, nothing else touched.
  3. dmc_dense_layer_eval against fp64 at max|err| / max|ref| < 1e-5 -- the project's bar for bf16x3 kernels
     (tests/test_context_eval_gpu.py) -- on layers of the two networks (LAYER_SHAPES says why each shape is there), both LeakyReLU
     branches live on the reference, every channel outside [K, K + R) bitwise unchanged, channels >= K + R prefilled with 0xFF
     (NaN: a read past K would surface), every launch twice and bit-equal.
  4. The exact layer, which a 1e-5 bar cannot see (tests/test_ctx_products_gpu.py's docstring): the stride-CT addressing and the
     six slice products of the new main loop.  (a) a one-hot sweep over all 9 K (tap, buffer channel) positions; (b) one-hot in
     both operands with x3_ref.loop_family; (c) hand-built one-slice packs of small integers; (d) the statistical layer with the
     metrics and the bars of tests/test_x3_products_gpu.py, weights live in one tap and one 32-channel block per launch.
  5. dmc_dense_head_eval against fp64.
  6. The whole networks through net(x): against the reference's own golden outputs (G2) and against the fp64 stack within
     max(4 e_ref, 2e-5 max|ref|), e_ref = the stock fp32 forward's own distance from fp64 (the bar of DESIGN.md 4.21).
  7. Isolation: a frame's result does not depend on its batch, its neighbours or the frame ranges.
  8. Byte offsets past 4 GiB in one launch.
  9. Dispatch: no stock convolution and no concatenation on the forward-only paths; autograd / DENSE_EVAL = False keep the stock loop.
 10. Every launching entry point in a guarded arena (tests/abi_arena.py); the feature buffer is an in/out buffer.

Measured on an MI355X: see MEASURED / WORST_MEASURED below (records, not bars)."""
import copy
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import dmcnet_amd
from dmcnet_amd import _lib, model, ops
from oracle import dmc_oracle as O
from tests import abi_cases
from tests import dense_ref as D
from tests import test_x3_products_gpu as XP
from tests import x3_ref as R
from tests.abi_arena import run_case

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U8 = torch.uint8
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TWO24 = float(1 << 24)
SLOPE = np.float32(0.1)
#: the worst (rms, max) kernel / emulation ratios test_error_tap_by_tap_and_k_block_by_k_block printed on an MI355X (bars 3 and 4)
WORST_MEASURED = {"dense-layer": (1.574, 2.112)}
#: printed on an MI355X: max|err| / max|ref| of the fp64 cases (bar 1e-5) by LAYER_SHAPES entry and head, and the worst (e, e_ref) of the
#: whole networks (bar max(4 e_ref, 2e-5 max|ref|), max|ref| 3.3 .. 4.6)
MEASURED = {"layers": (2.43e-7, 1.63e-6, 1.51e-6, 1.50e-6, 8.23e-7, 3.33e-7, 4.84e-7, 9.28e-8), "head-464": 4.94e-7, "head-176": 3.50e-7,
            "DenseNet": (4.71e-6, 1.82e-6), "DenseNetSmall": (2.40e-6, 1.64e-6)}


def P(t):
    return _lib.ptr(t)


def ok(rc, what):
    _lib.check(rc, what)


def rs(seed):
    return np.random.RandomState(seed)


def rel_err(a, b):
    a, b = a.detach().double().cpu(), torch.as_tensor(b).detach().double().cpu()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))


def f64(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64))


def bits(t):
    return t.detach().contiguous().view(torch.int32)


def leaky32(v):
    """LeakyReLU(0.1) as the epilogue computes it, on a numpy float32 array."""
    v = np.asarray(v)
    assert v.dtype == np.float32
    return np.where(v > 0, v, SLOPE * v)


def leaky32_of(v64):
    """The same of an fp64 tensor that holds fp32 values (asserted); fp64 tensor out."""
    v = v64.numpy().astype(np.float32)
    assert np.array_equal(v.astype(np.float64), v64.numpy())
    return f64(leaky32(v))


def ff_buffer(shape):
    """A device fp32 tensor whose every byte is 0xFF (NaN)."""
    n = int(np.prod(shape))
    return torch.full((4 * n,), 0xFF, dtype=U8, device=DEV).view(torch.float32).view(shape)


def is_ff(t):
    return bool((bits(t) == -1).all())


def lib_pack(wb, k, r):
    """dmc_dense_pack_weights of an OHWI [r, 3, 3, k] fp32 tensor over a 0xFF-prefilled destination."""
    lib = _lib.load()
    wg = wb.contiguous().to(DEV)
    assert tuple(wg.shape) == (r, 3, 3, k) and wg.dtype == torch.float32
    wp = torch.full((lib.dmc_dense_wpack_bytes(k, r),), 0xFF, dtype=U8, device=DEV)
    ok(lib.dmc_dense_pack_weights(P(wg), P(wp), k, r, ops._stream()), "dmc_dense_pack_weights")
    return wp


def upload_pack(slices, k, r):
    """A hand-built pack (x3_ref.ctx_pack) of three slice arrays [r, k, 3, 3]."""
    p = R.ctx_pack(slices)
    assert p.shape == (9, k // 16, 3, r, 16) and p.nbytes == _lib.load().dmc_dense_wpack_bytes(k, r)
    return torch.from_numpy(p.view(np.uint8).reshape(-1)).to(DEV)


def ohwi(w):
    """numpy / torch [Cout, Cin, 3, 3] -> torch [Cout, 3, 3, Cin]."""
    return torch.as_tensor(np.asarray(w, np.float32)).permute(0, 2, 3, 1).contiguous()


def run_layer(feat, wp, bias, k, r):
    n, h, w, ct = feat.shape
    ok(_lib.load().dmc_dense_layer_eval(P(feat), P(wp), P(bias), n, h, w, ct, k, r, ops._stream()), "dmc_dense_layer_eval")
    return feat


def prefix_buffer(act_nhwc, ct):
    """[N, H, W, ct] on the device: ``act_nhwc`` [N, H, W, K] in the prefix, 0xFF bytes behind it."""
    feat = ff_buffer(tuple(act_nhwc.shape[:3]) + (ct,))
    feat[..., :act_nhwc.shape[3]] = torch.as_tensor(act_nhwc).to(DEV)
    return feat


def layer_out(act_nhwc, wp, bias, ct, k, r):
    """One launch on a fresh buffer; asserts the prefix and the tail untouched; returns the slot [N, H, W, r] on the device."""
    feat = prefix_buffer(act_nhwc, ct)
    before = feat[..., :k].clone()
    run_layer(feat, wp, bias, k, r)
    assert torch.equal(bits(feat[..., :k]), bits(before)) and is_ff(feat[..., k + r:])
    return feat[..., k:k + r].contiguous()


# =====================================================================================================================
# 1. pack
# =====================================================================================================================
@pytest.mark.parametrize("k,r", [(16, 32), (144, 128), (272, 96), (368, 64), (432, 32)])
def test_pack_equals_the_documented_layout_bit_for_bit(k, r):
    w = (rs(901).standard_normal((r, k, 3, 3)) * 0.05).astype(np.float32)
    w[0, 0, 0, 0], w[1, 1, 1, 1] = 0.0, -0.0
    w[:, 5:16] = 0                                                  # pad columns, as the route's own weights have them
    s = R.split(w)
    assert s[1].any() and s[2].any()
    got = lib_pack(ohwi(w), k, r).cpu().numpy().view(np.uint16).reshape(9, k // 16, 3, r, 16)
    want = R.ctx_pack(s)
    assert got.shape == want.shape
    if not np.array_equal(got, want):
        bad = np.argwhere(got != want)
        raise AssertionError("pack (K %d, R %d): %d of %d elements differ; first (tap, k-block, slice, row, k) %s: got %04x want %04x"
                             % (k, r, len(bad), want.size, tuple(bad[0]), got[tuple(bad[0])], want[tuple(bad[0])]))


# =====================================================================================================================
# 2. ingest
# =====================================================================================================================
@pytest.mark.parametrize("ct", [464, 176])
@pytest.mark.parametrize("shape", [(2, 19, 37), (1, 1, 1)], ids=["2-19-37", "1-1-1"])
def test_ingest_writes_its_slot_and_nothing_else(shape, ct):
    n, h, w = shape
    x = D.rnd(811, (n, 5, h, w)).to(DEV)
    feat = ff_buffer((n, h, w, ct))
    ok(_lib.load().dmc_dense_ingest(P(x), P(feat), n, h, w, ct, ops._stream()), "dmc_dense_ingest")
    assert torch.equal(bits(feat[..., :5]), bits(x.permute(0, 2, 3, 1)))
    assert bool((bits(feat[..., 5:16]) == 0).all())                # +0.0
    assert is_ff(feat[..., 16:])


# =====================================================================================================================
# 3. layer against fp64
# =====================================================================================================================
#: (N, H, W, CT, K, R)
LAYER_SHAPES = [
    (2, 19, 37, 464, 16, 128),    # the first layer: 5 live channels of 16 in the contraction; TN 4; a pixel count no tile divides
    (1, 9, 70, 464, 272, 96),     # TN 3
    (2, 17, 40, 464, 432, 32),    # the longest contraction; TN 1
    (1, 12, 21, 464, 368, 64),    # TN 2
    (3, 5, 7, 176, 112, 32),      # 105 pixels: less than one tile, tiles span frame boundaries
    (1, 1, 257, 176, 48, 32),     # one full 256-pixel tile and one pixel; H = 1: every vertical tap is outside
    (1, 33, 1, 176, 144, 32),     # W = 1: every horizontal tap is outside (a linearised offset would land in the next row)
    (1, 1, 1, 176, 16, 32),       # only the centre tap is inside
]
LAYER_IDS = ["-".join(map(str, s)) for s in LAYER_SHAPES]


@functools.lru_cache(maxsize=None)
def layer_case(n, h, w, ct, k, r):
    """(buffer [N, H, W, CT] fp32 CPU with NaN from channel K on, weight OHWI [R, 3, 3, K], bias [R], fp64 result [N, R, H, W] with zeros
    in the pad channels, fp64 pre-activation of the live channels): layer ``K`` of the network with ``CT`` buffer channels on the fp32
    activations of the fp64 stack in front of it.  Computed once per shape, never modified."""
    name = D.net_of_ct(ct)
    lay = D.layout(name)
    li = D.EXPECTED[name][0].index(k)
    assert lay["layers"][li][:2] == (k, r)
    ps = D.params(name)
    x = D.rnd(D.SEED, (n, 5, h, w))
    _, ys, _ = D.stack(ps, x, upto=li)
    buf = D.to_buffer(lay, x, [y.float() for y in ys])
    assert not bool(torch.isnan(buf[..., :k]).any()) and bool(torch.isnan(buf[..., k:]).all())
    wt, b = ps[li]
    wb, bb = D.buffer_weight(wt, b, k, r, lay["layers"][li][2])
    pre = F.conv2d(D.gather_input(lay, li, buf).double(), wt.double(), b.double(), 1, 1)
    ref = torch.zeros((n, r, h, w), dtype=torch.float64)
    ref[:, :wt.shape[0]] = F.leaky_relu(pre, D.SLOPE)
    return buf, wb, bb, ref, pre


@pytest.mark.parametrize("shape", LAYER_SHAPES, ids=LAYER_IDS)
def test_layer_vs_fp64(shape):
    n, h, w, ct, k, r = shape
    assert _lib.load().dmc_dense_supported(*shape) == 1
    buf, wb, bb, ref, pre = layer_case(*shape)
    neg = float((pre < 0).double().mean())
    assert 0.3 < neg < 0.7, neg                                    # both LeakyReLU branches carry weight
    wp, bias = lib_pack(wb, k, r), bb.to(DEV)
    feat = ff_buffer((n, h, w, ct))
    feat[..., :k] = buf[..., :k].to(DEV)
    before = feat.clone()
    run_layer(feat, wp, bias, k, r)
    slot = feat[..., k:k + r]
    e = rel_err(slot.permute(0, 3, 1, 2), ref)
    print("dense layer %s: rel_err %.3e (negative pre-activations %.3f)" % (shape, e, neg))
    assert not bool(torch.isnan(slot).any())
    assert e < 1e-5, e
    live = pre.shape[1]
    assert bool((bits(slot[..., live:]) == 0).all()) if live < r else True         # pad channels: leaky(0 + 0) = +0.0
    assert torch.equal(bits(feat[..., :k]), bits(before[..., :k])) and is_ff(feat[..., k + r:])
    again = before.clone()
    run_layer(again, wp, bias, k, r)
    assert torch.equal(bits(again), bits(feat))                    # run to run


# =====================================================================================================================
# 4. the exact layer
# =====================================================================================================================
#: (CT, K, R).  K = 432 with R = 128 -- the longest contraction under the widest tile -- does not fit a 464-channel buffer (K + R <= CT is
#: part of dmc_dense_supported), so that pair runs in a 560-channel one, and the network's own last layer (464, 432, 32) runs beside it.
EXACT = [(560, 432, 128), (464, 432, 32), (176, 144, 32)]
EXACT_IDS = ["560-432-128", "464-432-32", "176-144-32"]
FRAME = (1, 7, 9)


def shifted(x_nhwc, tap):
    """[N, H, W, K] numpy -> the tap-shifted activation, zero outside the frame: out[n, y, x] = in[n, y + ky - 1, x + kx - 1]."""
    n, h, w, k = x_nhwc.shape
    xp = np.zeros((n, h + 2, w + 2, k), x_nhwc.dtype)
    xp[:, 1:-1, 1:-1] = x_nhwc
    ky, kx = divmod(tap, 3)
    return xp[:, ky:ky + h, kx:kx + w]


def one_hot_launch(x, positions, values, ct, k, r):
    """Output channel i carries ``values[i]`` at (tap, channel) = divmod(positions[i], k) and nothing else; bias 0.  Returns (got
    [N, H, W, r] numpy float32, the shifted activation each channel must show [N, H, W, r])."""
    wt = np.zeros((r, k, 3, 3), np.float32)
    seen = np.zeros(x.shape[:3] + (r,), x.dtype)
    for i, (p, v) in enumerate(zip(positions, values)):
        tap, ch = divmod(int(p), k)
        wt[i, ch, tap // 3, tap % 3] = v
        seen[..., i] = shifted(x, tap)[..., ch]
    got = layer_out(x, lib_pack(ohwi(wt), k, r), torch.zeros(r, device=DEV), ct, k, r)
    return got.cpu().numpy(), seen


@pytest.mark.parametrize("ct,k,r", EXACT, ids=EXACT_IDS)
def test_one_hot_sweep_over_every_tap_and_buffer_channel(ct, k, r):
    """Every one of the 9 K positions of the contraction, once: the output is the shifted activation times +-1 / +-2 through the
    LeakyReLU, bit for bit, and exactly 0 where the tap falls outside the frame.  A wrong pixel stride, a wrong k-block offset or a
    wrong tap offset shows in the position that uses it."""
    r_ = rs(930)
    n, h, w = FRAME
    x = r_.standard_normal((n, h, w, k)).astype(np.float32)
    total = 9 * k
    covered = np.zeros(total, bool)
    for first in range(0, total, r):
        positions = (first + np.arange(r)) % total
        values = (r_.choice([1.0, 2.0], size=r) * r_.choice([-1.0, 1.0], size=r)).astype(np.float32)
        got, seen = one_hot_launch(x, positions, values, ct, k, r)
        want = leaky32(seen * values)                              # (x times +-1 / +-2 is exact)
        assert np.array_equal(got, want), "positions %d..: %d of %d values differ" % (first, int((got != want).sum()), want.size)
        for i, p in enumerate(positions):                          # outside the frame: exactly zero
            tap = int(p) // k
            dead = shifted(np.ones((n, h, w, 1), np.float32), tap)[..., 0] == 0
            assert dead.any() == (tap != 4) and not got[..., i][dead].any()
        covered[positions] = True
    assert covered.all()


@pytest.mark.parametrize("ct,k,r", EXACT, ids=EXACT_IDS)
def test_one_term_in_both_operands_is_the_six_product_sum(ct, k, r):
    """x3_ref.loop_family on both operands: the one-term six-product sum is exact and is NOT the rounded fp32 product; a lost
    product or a spurious (1,2) / (2,1) changes the bits."""
    r_ = rs(931)
    n, h, w = FRAME
    c = np.float32(R.LOOP_C)
    x, ux = R.loop_family(r_, (n, h, w, k))
    for _ in range(3):
        positions = r_.randint(0, 9 * k, size=r)
        uw = np.exp2(r_.randint(-3, 4, size=r).astype(np.float64)) * r_.choice([-1.0, 1.0], size=r)
        wv = (uw * R.LOOP_C).astype(np.float32)
        assert np.array_equal(wv.astype(np.float64), uw * R.LOOP_C)
        got, _ = one_hot_launch(x, positions, wv, ct, k, r)
        exp64 = np.zeros((n, h, w, r), np.float64)
        for i, p in enumerate(positions):
            tap, ch = divmod(int(p), k)
            exp64[..., i] = shifted(ux, tap)[..., ch] * uw[i] * R.LOOP_CC
        want32 = exp64.astype(np.float32)
        assert np.array_equal(want32.astype(np.float64), exp64)    # exact in fp32
        rounded = np.zeros_like(want32)
        for i, p in enumerate(positions):
            tap, ch = divmod(int(p), k)
            rounded[..., i] = shifted(x, tap)[..., ch] * wv[i]
        assert not np.array_equal(rounded, want32)                 # ... and not what an fp32 multiplication returns
        assert np.array_equal(got, leaky32(want32)), "%d of %d values differ" % (int((got != leaky32(want32)).sum()), want32.size)


@functools.lru_cache(maxsize=None)
def crafted_activation(k, family):
    """(x [N, K, H, W], [what a weight in slice j sees of it, fp64]) -- computed once, never modified."""
    n, h, w = FRAME
    x, parts = R.weight_family(rs(910 + family), (n, k, h, w), family)
    return x, [f64(R.weight_seen_by_slice(parts, j)) for j in range(3)]


@pytest.mark.parametrize("family", [1, 2])
@pytest.mark.parametrize("ct,k,r", EXACT, ids=EXACT_IDS)
def test_crafted_packs_pair_each_weight_slice_with_its_activation_slices(ct, k, r, family):
    """Small integers in slice j ALONE of a hand-built pack (legitimate input once the pack test holds), live in one tap and one
    <= 64-channel block at a time; B = sum |u||x| < 2^24, so every partial sum of every order is an exact integer: slice 0 must see
    all of x, slice 1 s0 + s1, slice 2 s0 only."""
    n, h, w = FRAME
    r_ = rs(920 + family)
    x, seen = crafted_activation(k, family)
    xg, xabs = np.ascontiguousarray(x.transpose(0, 2, 3, 1)), f64(np.abs(x))
    stacked = torch.cat(seen)
    dense = R.small_ints(r_, (r, k, 3, 3))
    zero = np.zeros((r, k, 3, 3), np.float32)
    bias = torch.zeros(r, device=DEV)
    for tap in range(9):
        for blk in range((k + 63) // 64):
            c0, c1 = 64 * blk, min(k, 64 * blk + 64)
            if family == 1:
                u = R.only_tap(dense, tap, blk, axis=1)
            else:                                                  # family 2 reaches 2^24 - 1: one-hot weights with |u| = 1
                u = np.zeros((r, k, 3, 3), np.float32)
                u[np.arange(r), r_.randint(c0, c1, size=r), tap // 3, tap % 3] = r_.choice([-1.0, 1.0], size=r)
            assert np.abs(u).sum() > 0
            bound = F.conv2d(xabs[:, c0:c1], f64(np.abs(u))[:, c0:c1], None, 1, 1)
            assert 0 < float(bound.max()) < TWO24
            wants = F.conv2d(stacked[:, c0:c1], f64(u)[:, c0:c1], None, 1, 1).split(n)
            for j in range(3):
                wp = upload_pack([u if s == j else zero for s in range(3)], k, r)
                got = layer_out(xg, wp, bias, ct, k, r)
                XP.assert_exact(got.permute(0, 3, 1, 2), leaky32_of(wants[j]), "family %d, tap %d, block %d, weight slice %d" % (family, tap, blk, j))
    assert not torch.equal(seen[0], seen[2]) and (family == 1 or not torch.equal(seen[0], seen[1]))      # the cases tell five from six


STAT = [(464, 64, 128), (464, 48, 96), (176, 64, 64), (176, 80, 32)]          # (CT, K, R): TN 4, 3, 2, 1; K = 48, 80 end in a 16-wide block
STAT_FRAME = (2, 7, 9)


def accumulators(act_nhwc, wt, ct, k, r):
    """The raw sums of a layer launch, read back exactly: bias 0, once with the weights as they are (positive results pass the
    LeakyReLU unchanged) and once negated; every launch twice and bit-equal."""
    bias = torch.zeros(r, device=DEV)
    out = []
    for sign in (1.0, -1.0):
        wp = lib_pack(ohwi(wt * np.float32(sign)), k, r)
        y = layer_out(act_nhwc, wp, bias, ct, k, r)
        assert torch.equal(bits(y), bits(layer_out(act_nhwc, wp, bias, ct, k, r)))
        out.append(y)
    pos, neg = out
    assert not bool(torch.isnan(pos).any()) and not bool(((pos > 0) & (neg > 0)).any())
    acc = torch.where(pos > 0, pos, torch.where(neg > 0, -neg, pos * 0))
    return acc.double().cpu().reshape(-1, r).numpy()


@pytest.mark.parametrize("family", ["gauss", "wide"])
@pytest.mark.parametrize("ct,k,r", STAT, ids=["-".join(map(str, s)) for s in STAT])
def test_error_tap_by_tap_and_k_block_by_k_block(ct, k, r, family):
    n, h, w = STAT_FRAME
    act, wt = XP.operands(family, 950, (n, k, h, w), (r, k, 3, 3), 1, 1)
    col, mat = R.im2col(act, 3, 1, 1), R.weight_matrix(wt)
    ag = np.ascontiguousarray(act.transpose(0, 2, 3, 1))
    for tap in range(9):
        for c0 in range(0, k, 32):
            c1 = min(k, c0 + 32)
            w1 = np.zeros_like(wt)
            w1[:, c0:c1, tap // 3, tap % 3] = wt[:, c0:c1, tap // 3, tap % 3]
            got = accumulators(ag, w1, ct, k, r)
            ks = slice(tap * k + c0, tap * k + c1)
            m1 = R.weight_matrix(w1)                               # live in these rows of the contraction and nowhere else
            assert np.array_equal(m1[ks], mat[ks]) and np.count_nonzero(m1) == np.count_nonzero(mat[ks])
            _, bound = R.fp64_and_bound(col[:, ks], mat[ks])
            for g0, g1 in R.channel_groups(bound.shape[1], bound.shape[0]):
                assert int((bound[:, g0:g1] > 0).sum()) >= R.MIN_GROUP, (tap, c0, g0, g1)       # decided by the reference alone
            XP.hold_to_emulation("dense-layer %s %s tap %d channels %d..%d" % ((ct, k, r), family, tap, c0, c1), got, col[:, ks], mat[ks],
                                 R.ORDER_WEIGHT_OUTER)                                          # (dead outputs exactly zero: max_metric)


# =====================================================================================================================
# 5. head against fp64
# =====================================================================================================================
HEAD = (3, 19, 37)


@functools.lru_cache(maxsize=None)
def head_case(ct):
    """(full buffer [N, H, W, CT] fp32 CPU, head weight [2, 3, 3, CT] and bias in buffer order, fp64 result [N, 2, H, W])."""
    name = D.net_of_ct(ct)
    lay = D.layout(name)
    ps = D.params(name)
    n, h, w = HEAD
    x = D.rnd(D.SEED + 1, (n, 5, h, w))
    _, ys, _ = D.stack(ps, x)
    buf = D.to_buffer(lay, x, [y.float() for y in ys])
    assert not bool(torch.isnan(buf).any())
    k, _, index = lay["head"]
    wb, bb = D.buffer_weight(ps[-1][0], ps[-1][1], k, 2, index)
    assert not bool(wb[..., index < 0].any())                      # zero weights in the pad columns
    ref = F.conv2d(D.gather_input(lay, len(ys), buf).double(), ps[-1][0].double(), ps[-1][1].double(), 1, 1)
    return buf, wb, bb, ref


def run_head(feat, wb, bb, k):
    n, h, w, ct = feat.shape
    out = ff_buffer((n, 2, h, w))
    ok(_lib.load().dmc_dense_head_eval(P(feat), P(wb), P(bb), P(out), n, h, w, ct, k, ops._stream()), "dmc_dense_head_eval")
    return out


@pytest.mark.parametrize("ct", [464, 176])
def test_head_vs_fp64(ct):
    assert _lib.load().dmc_dense_supported(*HEAD, ct, ct, 2) == 1
    buf, wb, bb, ref = head_case(ct)
    feat, wg, bg = buf.to(DEV), wb.to(DEV), bb.to(DEV)
    out = run_head(feat, wg, bg, ct)
    e = rel_err(out, ref)
    print("dense head CT %d: rel_err %.3e" % (ct, e))
    assert not bool(torch.isnan(out).any()) and tuple(out.shape) == tuple(ref.shape)
    assert e < 1e-5, e
    assert torch.equal(bits(run_head(feat, wg, bg, ct)), bits(out))
    assert torch.equal(bits(feat), bits(buf.to(DEV)))              # the buffer is read only


# =====================================================================================================================
# 6. whole networks, through net(x)
# =====================================================================================================================
CLS = {"DenseNet": model.EstimatorDenseNet, "DenseNetSmall": model.EstimatorDenseNetSmall}


def route_on(monkeypatch):
    """DMC_DENSE_EVAL=1: the route for every class it serves (EstimatorDenseNetSmall is not on it by default: it measured slower)."""
    monkeypatch.setattr(model, "DENSE_EVAL", True)
    monkeypatch.setattr(model, "DENSE_EVAL_ALL", True)


@functools.lru_cache(maxsize=None)
def seeded_net(name):
    return D.load_into(CLS[name](), name).to(DEV).eval()


@pytest.mark.parametrize("name", ["DenseNet", "DenseNetSmall"])
def test_whole_network_vs_reference_golden(name, golden, monkeypatch):
    g = golden("g2_model_eval")
    route_on(monkeypatch)
    o = O.seeded_state_fill(O.build_estimator(name), seed=25).eval()
    m = CLS[name]()
    assert list(m.state_dict().keys()) == list(o.state_dict().keys())
    m.load_state_dict(o.state_dict())
    m.to(DEV).eval()
    x = D.rnd(24, (2, 5, 48, 48)).to(DEV)                          # (the golden test's rnd(24, ...): the same draw)
    with torch.no_grad():
        assert ops.dense_eval_supported(m, x)
        got = m(x)
    np.testing.assert_allclose(got.cpu().numpy(), g["est_" + name], rtol=1e-4, atol=1e-5)


@pytest.mark.parametrize("shape", [(1, 5, 20, 37), (3, 5, 33, 18), (3, 5, 14, 14)], ids=["20x37", "33x18", "14x14"])
@pytest.mark.parametrize("name", ["DenseNet", "DenseNetSmall"])
def test_whole_network_vs_fp64(name, shape, monkeypatch):
    route_on(monkeypatch)
    m = seeded_net(name)
    ps = D.params(name)
    x = D.rnd(31, shape)
    ref64 = D.stack(ps, x)[2]
    ref32 = D.stack(ps, x, dtype=torch.float32)[2]
    with torch.no_grad():
        assert ops.dense_eval_supported(m, x.to(DEV))
        got = m(x.to(DEV))
    assert tuple(got.shape) == tuple(ref64.shape)
    e = float((got.double().cpu() - ref64).abs().max())
    e_ref = float((ref32.double() - ref64).abs().max())
    top = float(ref64.abs().max())
    print("dense chain %s %s: e %.3e e_ref %.3e max|y| %.3e" % (name, shape, e, e_ref, top))
    assert e <= max(4 * e_ref, 2e-5 * top), (e, e_ref, top)


# =====================================================================================================================
# 7. isolation
# =====================================================================================================================
@pytest.mark.parametrize("name", ["DenseNet", "DenseNetSmall"])
def test_frame_result_is_independent_of_its_batch_and_neighbours(name, monkeypatch):
    route_on(monkeypatch)
    m = seeded_net(name)
    f, g, h2 = (D.rnd(40 + i, (1, 5, 20, 37)).to(DEV) for i in range(3))
    wild = D.rnd(49, (1, 5, 20, 37), 1e6).to(DEV)
    with torch.no_grad():
        alone = m(f)
        first = m(torch.cat((f, g, h2)))
        last = m(torch.cat((g, h2, f)))
        changed = m(torch.cat((f, wild, h2)))
    assert torch.equal(bits(alone[0]), bits(first[0])) and torch.equal(bits(alone[0]), bits(last[2]))
    assert torch.equal(bits(changed[0]), bits(first[0])) and torch.equal(bits(changed[2]), bits(first[2]))
    assert not torch.equal(changed[1], first[1])


@pytest.mark.parametrize("name", ["DenseNet", "DenseNetSmall"])
def test_frame_ranges_equal_one_range(name, monkeypatch):
    route_on(monkeypatch)
    m = seeded_net(name)
    ct = D.EXPECTED[name][2]
    x = D.rnd(41, (5, 5, 20, 37)).to(DEV)
    with torch.no_grad():
        assert ops.dense_eval_chunks(5, 20, 37, ct) == [(0, 5)]
        one = m(x)
        monkeypatch.setattr(ops, "DENSE_EVAL_BUDGET", 2 * 20 * 37 * ct * 4)
        assert ops.dense_eval_chunks(5, 20, 37, ct) == [(0, 2), (2, 4), (4, 5)]
        many = m(x)
    assert torch.equal(bits(one), bits(many))


# =====================================================================================================================
# 8. byte offsets past 4 GiB
# =====================================================================================================================
def test_byte_offsets_past_4_gib():
    """31 frames of 448 x 448 with 176 buffer channels: 4.38 GB, 1.095e9 elements (one launch).  Slot [144, 176) of the first and
    the last frame equals what the same entry point returns on one-frame copies, bit for bit (a truncated offset lands in another
    frame or another pixel)."""
    n, h, w, ct, k, r = 31, 448, 448, 176, 144, 32
    assert n * h * w * ct * 4 > 2 ** 32 and n * h * w * ct < 2 ** 31
    assert _lib.load().dmc_dense_supported(n, h, w, ct, k, r) == 1
    try:
        feat = torch.empty((n, h, w, ct), dtype=torch.float32, device=DEV)
    except RuntimeError as e:                                      # (torch.cuda.OutOfMemoryError is one)
        pytest.skip("cannot allocate the 4.38 GB feature buffer: %s" % str(e).splitlines()[0])
    g = torch.Generator(device=DEV).manual_seed(77)
    for f in range(n):
        feat[f, :, :, :k] = torch.randn((h, w, k), generator=g, device=DEV)
        feat[f, :, :, k:] = float("nan")
    wt = (rs(871).standard_normal((r, k, 3, 3)) * (1.4 / np.sqrt(9.0 * k))).astype(np.float32)
    wp, bias = lib_pack(ohwi(wt), k, r), D.rnd(872, (r,), 0.1).to(DEV)
    singles = {f: feat[f:f + 1].clone() for f in (0, n - 1)}
    run_layer(feat, wp, bias, k, r)
    for f, one in singles.items():
        run_layer(one, wp, bias, k, r)
        assert not bool(torch.isnan(one[..., k:]).any())
        assert torch.equal(bits(feat[f:f + 1, :, :, k:]), bits(one[..., k:])), f
        assert torch.equal(bits(feat[f:f + 1, :, :, :k]), bits(one[..., :k])), f
    ref = F.conv2d(singles[n - 1][:, :8, :8, :k].permute(0, 3, 1, 2).double().cpu(), f64(wt), bias.double().cpu(), 1, 1)[:, :, :7, :7]
    assert rel_err(feat[n - 1:n, :7, :7, k:].permute(0, 3, 1, 2), F.leaky_relu(ref, D.SLOPE)) < 1e-5


# =====================================================================================================================
# 9. dispatch
# =====================================================================================================================
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


def forbid_stock_ops_inside(gen, monkeypatch):
    """Patches F.conv2d, torch.cat and Tensor.cat to raise, but only while ``gen.forward`` runs (the classifier behind the generator
    is not what this file is about)."""
    inner = gen.forward

    def boom(*a, **kw):
        raise AssertionError("a stock convolution or concatenation ran inside the generator")

    def guarded(x):
        with pytest.MonkeyPatch.context() as mp:
            mp.setattr(torch.nn.functional, "conv2d", boom)
            mp.setattr(torch, "cat", boom)
            mp.setattr(torch.Tensor, "cat", boom, raising=False)
            return inner(x)
    monkeypatch.setattr(gen, "forward", guarded)


@pytest.mark.parametrize("name", ["DenseNet", "DenseNetSmall"])
def test_forward_video_runs_no_stock_convolution_or_concatenation(name, monkeypatch):
    from dmcnet_amd import evaluate
    route_on(monkeypatch)
    m = dmcnet_amd.Model(51, 3, "mv", base_model="resnet18", use_databn=0, arch_estimator=name)
    O.seeded_state_fill(m, 71)
    m.to(DEV).eval()
    assert isinstance(m.gen_flow_model, CLS[name])
    _, mv, res, _ = O.synthetic_batch(seed=72, batch=1, num_segments=3, num_class=51)
    rec = Recorder(_lib.load())
    monkeypatch.setattr(_lib, "load", lambda: rec)
    forbid_stock_ops_inside(m.gen_flow_model, monkeypatch)
    with torch.no_grad():
        on = evaluate.forward_video(m, mv.to(DEV), res.to(DEV), 3, 1)
    assert rec.calls.count("dmc_dense_ingest") == 1 and rec.calls.count("dmc_dense_layer_eval") == 5 and rec.calls.count("dmc_dense_head_eval") == 1
    assert rec.calls.count("dmc_dense_pack_weights") == 5
    assert on.shape == (1, 51) and np.isfinite(on).all()          # (the generator's values: the golden and the fp64 cases above)


def test_i3d_generate_runs_no_stock_convolution_or_concatenation(monkeypatch):
    from dmcnet_amd import i3d
    route_on(monkeypatch)
    net = i3d.I3D(51, modality="mv", arch_estimator="DenseNetSmall")
    D.load_into(net.gen_flow_model, "DenseNetSmall")
    gen = net.gen_flow_model.to(DEV).eval()
    inp = D.rnd(73, (1, 5, 4, 24, 20)).to(DEV)
    forbid_stock_ops_inside(gen, monkeypatch)
    with torch.no_grad():
        got = net.generate(inp)
    assert tuple(got.shape) == (1, 2, 4, 24, 20)
    ref = D.stack(D.params("DenseNetSmall"), inp.cpu().transpose(1, 2).reshape(-1, 5, 24, 20))[2]
    assert rel_err(got.transpose(1, 2).reshape(-1, 2, 24, 20), ref) < 1e-5


@pytest.mark.parametrize("name", ["DenseNet", "DenseNetSmall"])
def test_autograd_and_the_flag_keep_the_stock_loop(name, monkeypatch):
    m = seeded_net(name)
    x = D.rnd(51, (2, 5, 21, 17)).to(DEV)
    rec = Recorder(_lib.load())
    monkeypatch.setattr(_lib, "load", lambda: rec)
    # the stock route must reproduce itself for a bit comparison to mean anything: MIOpen is asked for its deterministic solvers
    monkeypatch.setattr(torch.backends.cudnn, "deterministic", True)
    monkeypatch.setattr(torch.backends.cudnn, "benchmark", False)
    route_on(monkeypatch)
    for train in (True, False):                                    # autograd on: never, in train() or in eval()
        m.train(train)
        got, want = m(x), D.stock_forward(m, x)
        assert got.requires_grad and torch.equal(bits(got), bits(want))
    m.eval()
    assert not ops.dense_eval_supported(m, x)
    monkeypatch.setattr(model, "DENSE_EVAL", False)                # DMC_DENSE_EVAL=0
    with torch.no_grad():
        assert torch.equal(bits(m(x)), bits(D.stock_forward(m, x)))
    assert not any(c.startswith("dmc_dense_") for c in rec.calls), rec.calls
    route_on(monkeypatch)
    with torch.no_grad():
        assert ops.dense_eval_supported(m, x)
        assert not ops.dense_eval_supported(m, x.double()) and not ops.dense_eval_supported(m, x[:, :4])
        assert not ops.dense_eval_supported(m.cpu(), x)
        m.to(DEV)
        on = m(x)
    assert any(c.startswith("dmc_dense_") for c in rec.calls)
    assert rel_err(on, D.stock_forward(m, x).detach()) < 1e-5
    monkeypatch.setattr(model, "DENSE_EVAL_ALL", False)            # DMC_DENSE_EVAL unset: by class (the one that measured slower stays stock)
    del rec.calls[:]
    with torch.no_grad():
        m(x)
    assert any(c.startswith("dmc_dense_") for c in rec.calls) == (name == "DenseNet") == m.DENSE_EVAL_BY_DEFAULT


def test_structural_defects_are_refused_on_the_device():
    x = D.rnd(52, (1, 5, 9, 9)).to(DEV)
    good = CLS["DenseNetSmall"]().to(DEV).eval()
    with torch.no_grad():
        assert ops.dense_eval_supported(good, x)
        for what in ("slope", "bias", "wide", "early"):
            net = CLS["DenseNetSmall"]().eval()
            if what == "slope":
                net.conv_2[1] = torch.nn.LeakyReLU(0.2)
            elif what == "bias":
                net.conv_3[0] = torch.nn.Conv2d(net.conv_3[0].in_channels, net.conv_3[0].out_channels, 3, 1, 1, bias=False)
            elif what == "wide":
                net = model.DenseEstimatorBase((32, 160, 8)).eval()
            else:
                net = model.EstimatorDenseNetTinyEarlyFusionSum().eval()
            net.to(DEV)
            assert not ops.dense_eval_supported(net, x), what
            if what != "early":
                assert torch.equal(net(x), D.stock_forward(net, x)), what
            with pytest.raises(_lib.DmcHipError):
                ops.dense_eval(net, x)


CHILD = """
import sys
sys.path.insert(0, %r)
import torch
from dmcnet_amd import model, ops
from tests import dense_ref as D
torch.backends.cudnn.deterministic = True
torch.backends.cudnn.benchmark = False
net = D.load_into(model.EstimatorDenseNetSmall(), "DenseNetSmall").to("cuda:0").eval()
x = D.rnd(53, (2, 5, 13, 11)).to("cuda:0")
calls = []
real = ops.dense_eval
ops.dense_eval = lambda n, t: (calls.append(1), real(n, t))[1]
with torch.no_grad():
    got, want = net(x), D.stock_forward(net, x)
print("RESULT", int(model.DENSE_EVAL), len(calls), int(torch.equal(got, want)))
"""


def test_environment_flag_off_in_a_fresh_process():
    """DMC_DENSE_EVAL is read once, at import: a fresh child process with DMC_DENSE_EVAL=0 runs the stock loop, bit for bit."""
    env = dict(os.environ)
    env["DMC_DENSE_EVAL"] = "0"
    out = subprocess.run([sys.executable, "-c", CHILD % ROOT], env=env, stdout=subprocess.PIPE, check=True, universal_newlines=True, timeout=300).stdout
    line = [ln for ln in out.splitlines() if ln.startswith("RESULT")][-1]
    assert line.split()[1:] == ["0", "0", "1"], out


# =====================================================================================================================
# 10. refusals and the memory contract
# =====================================================================================================================
def test_refused_calls_write_nothing():
    lib = _lib.load()
    buf = torch.zeros(1 << 16, dtype=U8, device=DEV)
    y = torch.full((1 << 16,), 0xFF, dtype=U8, device=DEV)
    p, q, s = P(buf), P(y), ops._stream()
    calls = [("dmc_dense_layer_eval", lambda: lib.dmc_dense_layer_eval(q, p, p, 1, 4, 4, 464, 16, 48, s)),
             ("dmc_dense_layer_eval", lambda: lib.dmc_dense_layer_eval(q, p, p, 1, 4, 4, 464, 448, 32, s)),
             ("dmc_dense_layer_eval", lambda: lib.dmc_dense_layer_eval(q, p, p, 1, 4, 4, 464, 24, 32, s)),
             ("dmc_dense_layer_eval", lambda: lib.dmc_dense_layer_eval(q, p, p, 1, 4, 4, 462, 16, 32, s)),
             ("dmc_dense_layer_eval", lambda: lib.dmc_dense_layer_eval(q, None, p, 1, 4, 4, 464, 16, 32, s)),
             ("dmc_dense_pack_weights", lambda: lib.dmc_dense_pack_weights(p, q, 16, 48, s)),
             ("dmc_dense_pack_weights", lambda: lib.dmc_dense_pack_weights(p, q, 24, 32, s)),
             ("dmc_dense_ingest", lambda: lib.dmc_dense_ingest(p, q, 1, 4, 4, 462, s)),
             ("dmc_dense_ingest", lambda: lib.dmc_dense_ingest(None, q, 1, 4, 4, 464, s)),
             ("dmc_dense_head_eval", lambda: lib.dmc_dense_head_eval(p, p, p, q, 1, 4, 4, 520, 516, s)),
             ("dmc_dense_head_eval", lambda: lib.dmc_dense_head_eval(p, p, None, q, 1, 4, 4, 464, 464, s))]
    for name, call in calls:
        assert call() == -1, name
        assert name.encode() in lib.dmc_last_error(), name
    torch.cuda.synchronize()
    assert bool((y == 0xFF).all())


def layer_arena_case(shape):
    n, h, w, ct, k, r = shape

    def fn(a):
        lib = _lib.load()
        buf, wb, bb, _, _ = layer_case(*shape)
        wp = a.out("wpack", nbytes=lib.dmc_dense_wpack_bytes(k, r), dtype=U8)
        a.call("dmc_dense_pack_weights", a.inp("w", wb), wp, k, r)
        a.call("dmc_dense_layer_eval", a.inout("feat", buf, nan_ok=True), wp, a.inp("bias", bb), n, h, w, ct, k, r)     # (NaN behind K + R: as given)

    def check(bufs):
        buf, _, _, ref, _ = layer_case(*shape)
        feat = bufs["feat"].t
        assert rel_err(feat[..., k:k + r].permute(0, 3, 1, 2), ref) < 1e-5
        assert torch.equal(bits(feat[..., :k]), bits(buf[..., :k].to(feat.device)))
        assert torch.equal(bits(feat[..., k + r:]), bits(buf[..., k + r:].to(feat.device)))
    return fn, check


def ingest_arena_case(a):
    n, h, w, ct = 2, 19, 37, 176
    feat = torch.full((n, h, w, ct), float("nan"))
    a.call("dmc_dense_ingest", a.inp("x", D.rnd(D.SEED, (n, 5, h, w))), a.inout("feat", feat, nan_ok=True), n, h, w, ct)


def _ingest_check(bufs):
    feat = bufs["feat"].t
    x = D.rnd(D.SEED, (2, 5, 19, 37)).to(feat.device)
    assert torch.equal(bits(feat[..., :5]), bits(x.permute(0, 2, 3, 1))) and bool((bits(feat[..., 5:16]) == 0).all())
    assert bool(torch.isnan(feat[..., 16:]).all())


def head_arena_case(ct):
    def fn(a):
        n, h, w = HEAD
        buf, wb, bb, _ = head_case(ct)
        a.call("dmc_dense_head_eval", a.inp("feat", buf), a.inp("w", wb), a.inp("bias", bb), a.out("out", (n, 2, h, w)), n, h, w, ct, ct)

    def check(bufs):
        assert rel_err(bufs["out"].t, head_case(ct)[3]) < 1e-5
    return fn, check


def refused_layer_case(ct, k, r):
    def fn(a):
        n, h, w = 1, 8, 8
        a.call("dmc_dense_layer_eval", a.inout("feat", torch.ones(n, h, w, 464)), a.inp("wpack", torch.zeros(16 * 128 * 54, dtype=U8)),
               a.inp("bias", torch.zeros(128)), n, h, w, ct, k, r)
    return fn


def refused_head_case(a):      # K = 516: over 512 and no multiple of 16
    n, h, w = 1, 8, 8
    a.call("dmc_dense_head_eval", a.inp("feat", torch.ones(n, h, w, 520)), a.inp("w", torch.zeros(2, 3, 3, 516)), a.inp("bias", torch.zeros(2)),
           a.out("out", (n, 2, h, w)), n, h, w, 520, 516)


ARENA_CASES = []
for _shape in ((1, 12, 21, 464, 368, 64), (3, 5, 7, 176, 112, 32)):
    _fn, _ck = layer_arena_case(_shape)
    ARENA_CASES.append(abi_cases.Case(abi_cases.tag("dmc_dense_layer_eval", *_shape), ["dmc_dense_pack_weights", "dmc_dense_layer_eval"], _fn,
                                      check=_ck, capacity=32 << 20))
ARENA_CASES.append(abi_cases.Case("dmc_dense_ingest-2-19-37-176", ["dmc_dense_ingest"], ingest_arena_case, check=_ingest_check, capacity=32 << 20))
_fn, _ck = head_arena_case(176)
ARENA_CASES.append(abi_cases.Case("dmc_dense_head_eval-3-19-37-176", ["dmc_dense_head_eval"], _fn, check=_ck, capacity=32 << 20))
ARENA_CASES.append(abi_cases.Case("dmc_dense_layer_eval-refused-R-48", ["dmc_dense_layer_eval"], refused_layer_case(464, 16, 48),
                                  expect_rc=abi_cases.DMC_E_INVALID, capacity=32 << 20))
ARENA_CASES.append(abi_cases.Case("dmc_dense_layer_eval-refused-K+R-over-CT", ["dmc_dense_layer_eval"], refused_layer_case(464, 448, 32),
                                  expect_rc=abi_cases.DMC_E_INVALID, capacity=32 << 20))
ARENA_CASES.append(abi_cases.Case("dmc_dense_head_eval-refused-K-516", ["dmc_dense_head_eval"], refused_head_case,
                                  expect_rc=abi_cases.DMC_E_INVALID, capacity=32 << 20))
_known = {c.id for c in abi_cases.CASES}
abi_cases.CASES.extend(c for c in ARENA_CASES if c.id not in _known)


@pytest.mark.parametrize("case", ARENA_CASES, ids=[c.id for c in ARENA_CASES])
def test_dense_entries_memory_contract(case):
    try:
        bufs = run_case(case.fn, device=DEV, capacity=case.capacity, expect_rc=case.expect_rc)
        if case.check is not None:
            case.check(bufs)
    except RuntimeError as e:
        if "HIP error" in str(e) or "illegal memory access" in str(e):
            # a faulted device serves nothing more: end the session here instead of launching the remaining cases on it
            pytest.exit("GPU fault in %s: %s" % (case.id, str(e).splitlines()[0]), returncode=3)
        raise
