"""GPU tests that tell six bf16x3 slice products from five in the dilated convolutions of the ContextNetwork:
gather_gemm<TN, TM> of csrc/ctx_common.h -- the main loop of the eval unit (ctx_eval.hip, dmc_ctx_unit_eval), of the training
forward and, with the transposed tap-mirrored pack, of the training data gradient (dconv.hip, dmc_dconv_fwd) -- and the second,
independent six-product loop of dconv_wgrad_kernel.  Everything goes through the C ABI; the reference is tests/x3_ref.py (whose
own checks, the seeded defects at this geometry included, are tests/test_x3_ref_cpu.py); the two layers, the metrics and the bars
are those of tests/test_x3_products_gpu.py.  tests/test_dconv_gpu.py and tests/test_context_eval_gpu.py hold the same kernels to
max|err| / max|ref| < 1e-5 on dense Gaussian operands, which sees neither a lost third-order product, nor a defect confined to
one tap or one 16-channel k-block of the panel, nor a mirrored tap on the wrong panel (it sits under the other eight taps).

Packs.  dmc_dconv_pack_weights (both orientations) and dmc_ctx_pack_weights against x3_ref.ctx_pack, the documented layout
[9][K / 16][3][R][16] built in numpy from x3_ref.split, bit for bit over a 0xFF-prefilled destination.  That makes a hand-built
pack legitimate input for the next layer.

Exact layer, no tolerance.  SHAPES of tests/test_dconv_gpu.py without its 16 k-pixel one: TN = 1 .. 4 in both orientations,
H < 2d + 1, W < d, the 35 x 35 frame at d = 16.  "Side" fwd runs every case through dmc_dconv_fwd AND dmc_ctx_unit_eval (identity
statistics: fmaf((v - 0) * 1, 1, 0) = v, then v > 0 ? v : 0.1f * v in numpy float32), side dgrad through dmc_dconv_fwd with
the transposed panels and Cin, Cout exchanged, against conv2d_input.
  * crafted packs: small integers (|u| <= 3) in slice j ALONE of a hand-built pack, live in one tap and one <= 64-channel block
    of the contraction at a time, against activations whose split is known by construction (x3_ref.weight_family; family 2
    reaches 2^24 - 1, so its weights are one-hot with |u| = 1).  B = sum |u||x| < 2^24 is asserted, so every partial sum of
    every order is an exact integer: slice 0 must see all of x, slice 1 s0 + s1, slice 2 s0 only.  A tap that lies outside the
    frame for every pixel (W <= d, H <= d) must return all zeros.
  * one-hot operands through the library's own packs: one nonzero weight (+-1 / +-2) per output channel against 24-bit Gaussian
    activations; one nonzero channel per pixel on a lattice of period 3d (no dilated window holds two live pixels) against
    Gaussian weights; and both again with x3_ref.loop_family on BOTH operands, whose one-term six-product sum is exact and is
    not the rounded fp32 product -- the only case that excludes a spurious (1,2) / (2,1) where the kernel splits in the loop.
  * weight gradient: one nonzero pixel per image in dy (channel co lives in image co mod n) against dense x, the mirror image,
    and both with loop_family: every dw element is one product, equal to fp64 conv2d_weight(dilation=d) bit for bit (d = 1 .. 16,
    pixel counts that are no multiple of the 32-pixel step).

Statistical layer.  Gaussian and wide-range operands, weights live in one tap and one 32-channel block of the contraction per
launch pair (K = 32 = two MFMA k-blocks: a one-chunk defect is half the sum), the emulation in the loop's own order
(ORDER_WEIGHT_OUTER; ORDER_SMALL_FIRST for the weight gradient, A = dy, B = x), outputs grouped by 64-wide output-channel block
(weight gradient: tap x 64-wide Cout block), >= 1000 LIVE outputs (B > 0) per group -- asserted on the reference alone --
    rms(got - fp64) / rms(B) <= 3 x the emulation's, max(|got - fp64| / B) <= 4 x the emulation's maximum over the tensor,
dead outputs exactly zero, a tap without a live output all zeros, every launch twice and bit-equal.  The eval unit's
accumulators are read back exactly: with gamma = +1 the positive ones pass unchanged, with gamma = -1 the negated negative ones.

Measured on an MI355X (all 115 cases pass, the file takes 11 s; WORST_MEASURED below): no kernel forms a product outside the six
or misses one of them, both packs equal the documented layout.  gather_gemm sits at 1.42 .. 1.43 x the emulation's rms on K = 32
(max 1.77 forward and eval unit -- the same accumulators bit for bit -- and 2.11 data gradient), where conv3_kernel and the x3s
loops sit on K = 64; the weight gradient at 0.23 .. 0.81 x (max 0.43): its pixel ranges carry shorter fp32 sums than the one
sequential accumulator of the emulation, most visibly on the 16 k-pixel shape, so the range split needs no model of its own.
Tried once against a library with two seeded defects -- gather_gemm skipping the (1,1) product in the second 16-channel k-block
of the centre tap, dconv_wgrad_kernel skipping (0,2) in the second 16-pixel block of every step of the centre tap: 97 of the
115 cases here failed (all but the packs, the masked taps and the two coverage checks; every exact and every statistical case
of every pass), while of the fourteen 1e-5 cases of tests/test_dconv_gpu.py::test_conv_dgrad_wgrad_vs_fp64 and
tests/test_context_eval_gpu.py::test_middle_unit_vs_fp64 thirteen passed -- the one that failed is the 35 x 35 frame at d = 16,
where the centre tap is most of the sum, with a weight gradient at 1.07e-5."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F
from torch.nn import grad as G

from dmcnet_amd import _lib, ops
from tests import test_dconv_gpu as DC
from tests import test_x3_products_gpu as XP
from tests import x3_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U8 = torch.uint8
TWO24 = float(1 << 24)
SLOPE = np.float32(0.1)
#: the worst (rms, max) kernel / emulation ratios this file printed on an MI355X, per kernel and pass (bars 3 and 4); a record, not a bar
WORST_MEASURED = {"ctx-fwd": (1.434, 1.767), "ctx-eval": (1.434, 1.767), "ctx-dgrad": (1.416, 2.112), "ctx-wgrad": (0.812, 0.430)}

SHAPES = [s for s in DC.SHAPES if s != (4, 64, 64, 32, 32, 1)]
WGRAD_SHAPES = SHAPES + [(4, 64, 64, 32, 32, 1)]            # 64 pixel ranges whose partials are reduced in order
H_MASKED = (2, 4, 70, 32, 64, 4)                            # H <= d: every vertical side tap is outside (no SHAPES entry has that)
IDS = DC.IDS[:len(SHAPES)]
assert len(SHAPES) == 6 and SHAPES == DC.SHAPES[:6]
PAIRS = [(32, 128), (128, 96), (96, 64), (64, 32)]          # (Cin, Cout): 32 .. 128 on both sides, never equal


def rs(seed):
    return np.random.RandomState(seed)


def f64(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64))


def to_dev(a):
    """numpy [N, C, H, W] -> fp32 device tensor [N, H, W, C]."""
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, np.float32).transpose(0, 2, 3, 1))).to(DEV)


def ohwi(w):
    """numpy [Cout, Cin, 3, 3] -> fp32 device tensor [Cout, 3, 3, Cin]."""
    return to_dev(w)


def nchw(t):
    return t.permute(0, 3, 1, 2)


def tap_is_outside(tap, h, w, d):
    ky, kx = divmod(tap, 3)
    return (w <= d and kx != 1) or (h <= d and ky != 1)


def leaky32(v64):
    """LeakyReLU(0.1) of fp32 values as the eval epilogue computes it, in numpy float32; fp64 tensor in, fp64 tensor out."""
    v = v64.numpy().astype(np.float32)
    assert np.array_equal(v.astype(np.float64), v64.numpy())
    return f64(np.where(v > 0, v, SLOPE * v))


class Pass(object):
    """One route through gather_gemm.  kind 'fwd' / 'eval': activation x [N, Cin, H, W], result [N, Cout, H, W]; kind 'dgrad':
    activation dy [N, Cout, H, W], result dx [N, Cin, H, W].  ca / cr = channels of the activation (the contraction) / the result;
    ``axis`` = the contraction axis of the weight [Cout, Cin, 3, 3]."""

    def __init__(self, kind, shape):
        self.kind, self.shape = kind, shape
        self.n, self.h, self.w, self.cin, self.cout, self.d = shape
        self.ca, self.cr = (self.cout, self.cin) if kind == "dgrad" else (self.cin, self.cout)
        self.axis = 0 if kind == "dgrad" else 1
        self.wshape = (self.cout, self.cin, 3, 3)
        self.act_shape = (self.n, self.ca, self.h, self.w)
        assert _lib.load().dmc_dconv_supported(*shape) == 1 and _lib.load().dmc_ctx_unit_supported(*shape) == 1

    def upload_pack(self, slices):
        """A hand-built pack (x3_ref.ctx_pack) of three slice arrays [Cout, Cin, 3, 3]."""
        p = R.ctx_pack(slices, transposed=self.kind == "dgrad")
        assert p.nbytes == _lib.load().dmc_dconv_wpack_bytes(self.cin, self.cout) == _lib.load().dmc_ctx_wpack_bytes(self.cin, self.cout)
        return torch.from_numpy(p.view(np.uint8).reshape(-1)).to(DEV)

    def library_pack(self, w):
        """The library's own pack of fp32 weights [Cout, Cin, 3, 3] (numpy), over a 0xFF-prefilled destination."""
        lib = _lib.load()
        wg = ohwi(w)
        wp = torch.full((lib.dmc_dconv_wpack_bytes(self.cin, self.cout),), 0xFF, dtype=U8, device=DEV)
        if self.kind == "eval":
            DC.ok(lib.dmc_ctx_pack_weights(DC.P(wg), DC.P(wp), self.cin, self.cout, ops._stream()), "dmc_ctx_pack_weights")
        else:
            DC.ok(lib.dmc_dconv_pack_weights(DC.P(wg), DC.P(wp), self.cin, self.cout, int(self.kind == "dgrad"), ops._stream()),
                  "dmc_dconv_pack_weights")
        return wp

    def launch(self, act, wp, gamma=1.0):
        """act [N, H, W, ca] on the device, wp a pack -> [N, H, W, cr] (NaN-prefilled)."""
        lib = _lib.load()
        y = torch.full((self.n, self.h, self.w, self.cr), float("nan"), dtype=torch.float32, device=DEV)
        if self.kind == "eval":
            stats = torch.cat([torch.zeros(self.cr), torch.ones(self.cr)]).to(DEV)         # mean 0, invstd 1
            gam, bet = torch.full((self.cr,), gamma).to(DEV), torch.zeros(self.cr).to(DEV)
            DC.ok(lib.dmc_ctx_unit_eval(DC.P(act), DC.P(wp), DC.P(stats), DC.P(gam), DC.P(bet), DC.P(y), self.n, self.h, self.w, self.ca, self.cr,
                                        self.d, ops._stream()), "dmc_ctx_unit_eval")
        else:
            assert gamma == 1.0
            DC.ok(lib.dmc_dconv_fwd(DC.P(act), DC.P(wp), DC.P(y), self.n, self.h, self.w, self.ca, self.cr, self.d, ops._stream()), "dmc_dconv_fwd")
        return y

    def accumulators(self, act, wp):
        """The raw convolution result, read twice and bit-equal; the eval unit's through gamma = +1 and gamma = -1."""
        if self.kind != "eval":
            y = self.launch(act, wp)
            assert torch.equal(y, self.launch(act, wp))
            return y
        pos, neg = self.launch(act, wp, 1.0), self.launch(act, wp, -1.0)
        assert torch.equal(pos, self.launch(act, wp, 1.0)) and torch.equal(neg, self.launch(act, wp, -1.0))
        assert not bool(((pos > 0) & (neg > 0)).any())
        return torch.where(pos > 0, pos, torch.where(neg > 0, -neg, pos * 0))

    def ref(self, act, w, c0=None, c1=None):
        """fp64 stock convolution / data gradient of fp64 tensors; [c0, c1) = the only live channels of the contraction."""
        if self.kind == "dgrad":
            size = (act.shape[0], self.cin, self.h, self.w)
            return G.conv2d_input(size, w[c0:c1], act[:, c0:c1], stride=1, padding=self.d, dilation=self.d)
        return F.conv2d(act[:, c0:c1], w[:, c0:c1], None, 1, self.d, self.d)

    def expect(self, want):
        return leaky32(want) if self.kind == "eval" else want

    def one_hot_weights(self, r, values=(1.0, 2.0), tap=None, c0=0, c1=None):
        """[Cout, Cin, 3, 3] with ONE nonzero entry per RESULT channel: contraction channel in [c0, c1), tap ``tap`` (or any)."""
        w = np.zeros(self.wshape, np.float32)
        for ch in range(self.cr):
            k, t = r.randint(c0, self.ca if c1 is None else c1), (r.randint(9) if tap is None else tap)
            co, ci = (k, ch) if self.kind == "dgrad" else (ch, k)
            w[co, ci, t // 3, t % 3] = r.choice(values) * r.choice([-1.0, 1.0])
        return w

    def im2col(self, act):
        """numpy activation -> [M, 9 ca], K = [tap][channel]."""
        return R.im2col_dgrad(act, 3, 1, self.d, self.h, self.w, self.d) if self.kind == "dgrad" else R.im2col(act, 3, 1, self.d, self.d)

    def weight_matrix(self, wt):
        """numpy weight [Cout, Cin, 3, 3] -> [9 ca, cr] in the same K order."""
        return R.weight_matrix_dgrad(wt) if self.kind == "dgrad" else R.weight_matrix(wt)


def passes_of(side, shape):
    return [Pass("fwd", shape), Pass("eval", shape)] if side == "fwd" else [Pass("dgrad", shape)]


def rows(t):
    """[N, H, W, C] device tensor -> numpy float64 [N H W, C] (the GEMM's output layout)."""
    return t.detach().double().cpu().reshape(-1, t.shape[-1]).numpy()


# ================================================================ the packs, bit for bit
def weight_values(kind, r, shape):
    if kind == "gauss":
        return (r.standard_normal(shape) * 0.05).astype(np.float32)
    if kind == "wide":
        return (R.wide_range(r, shape, 1) * np.float32(0.1)).astype(np.float32)
    return R.loop_family(r, shape)[0]


@pytest.mark.parametrize("values", ["gauss", "wide", "loop"])
@pytest.mark.parametrize("cin,cout", PAIRS)
def test_packs_equal_the_documented_layout_bit_for_bit(cin, cout, values):
    w = weight_values(values, rs(901), (cout, cin, 3, 3))
    w[0, 0, 0, 0], w[1, 1, 1, 1] = 0.0, -0.0
    s = R.split(w)
    assert s[1].any() and s[2].any()
    shape = (1, 8, 8, cin, cout, 1)
    for kind in ("fwd", "dgrad", "eval"):
        p = Pass(kind, shape)
        got = p.library_pack(w).cpu().numpy().view(np.uint16).reshape(9, p.ca // 16, 3, p.cr, 16)
        want = R.ctx_pack(s, transposed=kind == "dgrad")
        assert got.shape == want.shape
        if not np.array_equal(got, want):
            bad = np.argwhere(got != want)
            raise AssertionError("%s pack (Cin %d, Cout %d, %s): %d of %d elements differ; first (tap, k-block, slice, row, k) %s: got %04x want %04x"
                                 % (kind, cin, cout, values, len(bad), want.size, tuple(bad[0]), got[tuple(bad[0])], want[tuple(bad[0])]))
    # the transposed panels hold element (t', co, ci) = w[co][8 - t'][ci]
    tr = R.ctx_pack(s, transposed=True)
    b0 = R.bf16_bits(s[0])
    for t, co, ci in ((0, 3, 5), (2, cout - 1, 17), (7, 16, cin - 1)):
        assert tr[t, co // 16, 0, ci, co % 16] == b0[co, ci, (8 - t) // 3, (8 - t) % 3]


# ================================================================ exact layer: crafted packs
@functools.lru_cache(maxsize=None)
def crafted_activation(ca, n, h, w, family):
    """(x, [what a weight in slice j sees of it, fp64]) -- computed once per activation shape, never modified."""
    x, parts = R.weight_family(rs(910 + family), (n, ca, h, w), family)
    return x, [f64(R.weight_seen_by_slice(parts, j)) for j in range(3)]


@pytest.mark.parametrize("family", [1, 2])
@pytest.mark.parametrize("side", ["fwd", "dgrad"])
@pytest.mark.parametrize("shape", SHAPES + [H_MASKED], ids=IDS + ["H-masked"])
def test_crafted_packs_pair_each_weight_slice_with_its_activation_slices(shape, side, family):
    n, h, w, cin, cout, d = shape
    passes = passes_of(side, shape)
    p = passes[0]
    r = rs(920 + family)
    x, seen = crafted_activation(p.ca, n, h, w, family)
    xg, xabs = to_dev(x), f64(np.abs(x))
    stacked = torch.cat(seen)                                   # the three wants of a weight in one stock call
    dense = R.small_ints(r, p.wshape)
    zero = np.zeros(p.wshape, np.float32)
    masked = 0
    for tap in range(9):
        for blk in range((p.ca + 63) // 64):
            c0, c1 = 64 * blk, min(p.ca, 64 * blk + 64)
            u = R.only_tap(dense, tap, blk, axis=p.axis) if family == 1 else p.one_hot_weights(r, (1.0,), tap, c0, c1)
            assert np.abs(u).sum() > 0
            bound = p.ref(xabs, f64(np.abs(u)), c0, c1)
            assert float(bound.max()) < TWO24                   # every partial sum of every order is an exact fp32 integer
            dead = float(bound.max()) == 0
            assert dead == tap_is_outside(tap, h, w, d)
            masked += dead
            wants = p.ref(stacked, f64(u), c0, c1).split(n)
            for j in range(3):
                wp = p.upload_pack([u if s == j else zero for s in range(3)])
                assert dead == (not bool(wants[j].any()))
                for q in passes:
                    XP.assert_exact(nchw(q.launch(xg, wp)), q.expect(wants[j]),
                                    "%s %s, family %d, tap %d, block %d, weight slice %d" % (q.kind, shape, family, tap, blk, j))
    assert masked == sum(tap_is_outside(t, h, w, d) for t in range(9)) * ((p.ca + 63) // 64)
    assert not torch.equal(seen[0], seen[2]) and (family == 1 or not torch.equal(seen[0], seen[1]))      # the cases tell five from six


# ================================================================ exact layer: one-hot operands through the library's packs
def one_hot_activation(r, p):
    """One nonzero channel per pixel (+-1 / +-2) on a lattice of period 3d: no dilated 3 x 3 window holds two live pixels."""
    return R.one_hot_channels(r, p.act_shape) * XP.lattice(p.act_shape, 3 * p.d, r)


@pytest.mark.parametrize("side", ["fwd", "dgrad"])
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_one_hot_operands_come_back_bit_for_bit(shape, side):
    n, h, w, cin, cout, d = shape
    r = rs(930)
    c = np.float32(R.LOOP_C)
    for q in passes_of(side, shape):
        gauss = lambda shp, s=1.0: (r.standard_normal(shp) * s).astype(np.float32)
        # one nonzero weight per result channel: the result is a shifted activation times +-1 / +-2 -- pins (x1, w0) (x2, w0)
        x, wt = gauss(q.act_shape), q.one_hot_weights(r)
        want = q.ref(f64(x), f64(wt))
        assert float(want.abs().max()) > 0
        XP.assert_exact(nchw(q.launch(to_dev(x), q.library_pack(wt))), q.expect(want), "%s %s, one-hot weights" % (q.kind, shape))
        # ... and with the in-loop family on both sides: one term, six products, no (1,2) / (2,1)
        x, ux = R.loop_family(r, q.act_shape)
        uw = q.one_hot_weights(r)
        want = q.ref(f64(ux), f64(uw)) * R.LOOP_CC
        assert float(want.abs().max()) > 0 and not torch.equal(want, q.ref(f64(x), f64(uw * c)))
        XP.assert_exact(nchw(q.launch(to_dev(x), q.library_pack(uw * c))), q.expect(want), "%s %s, one-hot weights, loop family" % (q.kind, shape))
        if d > 4:
            continue
        # one nonzero channel per pixel on the 3d lattice: one term per output -- pins (x0, w1) (x0, w2)
        x, wt = one_hot_activation(r, q), gauss(q.wshape, 0.1)
        want = q.ref(f64(x), f64(wt))
        assert float(want.abs().max()) > 0
        XP.assert_exact(nchw(q.launch(to_dev(x), q.library_pack(wt))), q.expect(want), "%s %s, one-hot activation" % (q.kind, shape))
        ux = one_hot_activation(r, q)
        wt, uw = R.loop_family(r, q.wshape)
        want = q.ref(f64(ux), f64(uw)) * R.LOOP_CC
        assert float(want.abs().max()) > 0
        XP.assert_exact(nchw(q.launch(to_dev(ux * c), q.library_pack(wt))), q.expect(want), "%s %s, one-hot activation, loop family" % (q.kind, shape))


def test_the_lattice_cases_cover_dilations_1_2_4():
    assert sorted({s[5] for s in SHAPES if s[5] <= 4}) == [1, 2, 4]


# ================================================================ exact layer: masked taps
@pytest.mark.parametrize("side", ["fwd", "dgrad"])
@pytest.mark.parametrize("shape", [(2, 40, 12, 96, 64, 16), H_MASKED], ids=["W-masked", "H-masked"])
def test_a_weight_in_a_tap_outside_the_frame_returns_zeros(shape, side):
    n, h, w, cin, cout, d = shape
    r = rs(940)
    outside = [t for t in range(9) if tap_is_outside(t, h, w, d)]
    assert len(outside) == 6
    for q in passes_of(side, shape):
        x = to_dev(r.standard_normal(q.act_shape))
        wt = (r.standard_normal(q.wshape) * 0.1).astype(np.float32)
        for tap in outside:
            y = q.launch(x, q.library_pack(R.only_tap(wt, tap)))
            assert not bool(torch.isnan(y).any()) and not bool(y.any()), (q.kind, tap)
        y = q.launch(x, q.library_pack(R.only_tap(wt, 4)))
        assert not bool(torch.isnan(y).any()) and bool(y.any())


# ================================================================ statistical layer: forward, data gradient, eval unit
def hold_block_to_emulation(what, got, a, b):
    """got [M, C] against the emulation of a [M, 32] @ b [32, C]; a tensor without a live output must be all zeros, any other
    must hold >= MIN_GROUP live outputs per group -- both decided by the fp64 bound alone."""
    _, bound = R.fp64_and_bound(a, b)
    assert not np.isnan(got).any()
    if not (bound > 0).any():
        assert not got.any(), what + ": no live output, yet not all zeros"
        return False
    for c0, c1 in R.channel_groups(bound.shape[1], bound.shape[0]):
        assert int((bound[:, c0:c1] > 0).sum()) >= R.MIN_GROUP, (what, c0, c1)
    XP.hold_to_emulation(what, got, a, b, R.ORDER_WEIGHT_OUTER)
    return True


@pytest.mark.parametrize("family", ["gauss", "wide"])
@pytest.mark.parametrize("kind", ["fwd", "dgrad", "eval"])
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_error_tap_by_tap_and_k_block_by_k_block(shape, kind, family):
    n, h, w, cin, cout, d = shape
    p = Pass(kind, shape)
    act, wt = XP.operands(family, 950, p.act_shape, p.wshape, 1, p.axis)
    col, mat = p.im2col(act), p.weight_matrix(wt)
    ag = to_dev(act)
    live = 0
    for tap in range(9):
        for blk in range(p.ca // 32):
            w1 = R.only_tap(wt, tap, blk, width=32, axis=p.axis)
            got = rows(p.accumulators(ag, p.library_pack(w1)))
            ks = slice(tap * p.ca + 32 * blk, tap * p.ca + 32 * blk + 32)
            m1 = p.weight_matrix(w1)                            # live in these 32 rows of K and nowhere else
            assert np.array_equal(m1[ks], mat[ks]) and np.count_nonzero(m1) == np.count_nonzero(mat[ks])
            alive = hold_block_to_emulation("ctx-%s %s %s tap %d k-block %d" % (kind, shape, family, tap, blk), got, col[:, ks], mat[ks])
            assert alive != tap_is_outside(tap, h, w, d)
            live += alive
    assert live == sum(not tap_is_outside(t, h, w, d) for t in range(9)) * (p.ca // 32)


# ================================================================ weight gradient
def run_wgrad(x, dy, shape):
    """dw [Cout, Cin, 3, 3] (device) of numpy x [N, Cin, H, W], dy [N, Cout, H, W]; run twice, bit-equal."""
    xg, dyg = to_dev(x), to_dev(dy)
    dw = DC.run_wgrad(xg, dyg, *shape)
    assert torch.equal(dw, DC.run_wgrad(xg, dyg, *shape))
    return dw.permute(0, 3, 1, 2)


def dw_fp64(x, dy, shape):
    n, h, w, cin, cout, d = shape
    return G.conv2d_weight(f64(x), (cout, cin, 3, 3), f64(dy), stride=1, padding=d, dilation=d)


def one_pixel_per_image(r, shape):
    """[N, C, H, W]: one nonzero pixel per image, channel c lives in image c mod N, values +-1 / +-2; the pixel is drawn from
    the central third of the frame so that some taps of a dilated window stay inside."""
    n, c, h, w = shape
    out = np.zeros(shape, np.float32)
    for img in range(n):
        k = len(range(img, c, n))
        out[img, img::n, h // 3 + r.randint(h - 2 * (h // 3)), w // 3 + r.randint(w - 2 * (w // 3))] = \
            r.choice([1.0, 2.0], size=k) * r.choice([-1.0, 1.0], size=k)
    return out


@pytest.mark.parametrize("shape", WGRAD_SHAPES, ids=DC.IDS)
def test_wgrad_one_product_per_element_comes_back_bit_for_bit(shape):
    n, h, w, cin, cout, d = shape
    r = rs(960)
    xs, ys = (n, cin, h, w), (n, cout, h, w)
    c = np.float32(R.LOOP_C)
    gauss = lambda shp: r.standard_normal(shp).astype(np.float32)
    # dy sparse, x dense: each dw element is ONE product dy x (x full 24 bits) -- pins (dy0, x1) (dy0, x2)
    x, dy = gauss(xs), one_pixel_per_image(r, ys)
    want = dw_fp64(x, dy, shape)
    assert float(want.abs().max()) > 0
    XP.assert_exact(run_wgrad(x, dy, shape), want, "wgrad %s, one-hot dy" % (shape,))
    # the mirror image -- pins (dy1, x0) (dy2, x0)
    x, dy = one_pixel_per_image(r, xs), gauss(ys)
    want = dw_fp64(x, dy, shape)
    assert float(want.abs().max()) > 0
    XP.assert_exact(run_wgrad(x, dy, shape), want, "wgrad %s, one-hot x" % (shape,))
    # both with the in-loop family on both sides: one term, the six products and no other
    (x, ux), udy = R.loop_family(r, xs), one_pixel_per_image(r, ys)
    want = dw_fp64(ux, udy, shape) * R.LOOP_CC
    assert float(want.abs().max()) > 0 and not torch.equal(want, dw_fp64(x, udy * c, shape))
    XP.assert_exact(run_wgrad(x, udy * c, shape), want, "wgrad %s, one-hot dy, loop family" % (shape,))
    ux, (dy, udy) = one_pixel_per_image(r, xs), R.loop_family(r, ys)
    want = dw_fp64(ux, udy, shape) * R.LOOP_CC
    assert float(want.abs().max()) > 0
    XP.assert_exact(run_wgrad(ux * c, dy, shape), want, "wgrad %s, one-hot x, loop family" % (shape,))
    if w <= d:
        assert not bool(want[:, :, :, 0].any()) and not bool(want[:, :, :, 2].any())


def test_the_wgrad_cases_cover_partial_steps_and_both_ends_of_the_dilations():
    assert {1, 16} <= {s[5] for s in WGRAD_SHAPES}
    assert any((s[0] * s[1] * s[2]) % 32 for s in WGRAD_SHAPES if s[5] == 1) and any((s[0] * s[1] * s[2]) % 32 for s in WGRAD_SHAPES if s[5] == 16)


@pytest.mark.parametrize("family", ["gauss", "wide"])
@pytest.mark.parametrize("shape", WGRAD_SHAPES, ids=DC.IDS)
def test_wgrad_error_tap_by_tap(shape, family):
    n, h, w, cin, cout, d = shape
    x, g = XP.operands(family, 970, (n, cin, h, w), (n, cout, h, w), 1, 1, b_scale=1.0)
    XP.wgrad_statistics("ctx-wgrad %s %s" % (shape, family), run_wgrad(x, g, shape), x, g, 3, 1, d, dilation=d)
