"""CPU tests of tests/x3_ref.py, the reference arithmetic that tests/test_x3_products_gpu.py holds the bf16x3 convolution
kernels to.  Three questions, none of which needs a kernel:

 1. Is the reference right?  The split round-trips bit for bit, the im2col GEMMs are the convolutions (against F.conv2d and
    autograd in fp64), and the emulation returns the expected integers of every kind of exact case the GPU file runs, bit
    for bit out of its fp32 accumulator, with the largest partial sum asserted below 2^24.
 2. Is it fp32 arithmetic?  The correct emulation's rms error stays below 2^-24 of rms(B), B = sum |a||b|: less than one
    fp32 rounding of the bound (the omitted products are below 2^-23 |a||b| each, the accumulator rounds
    once per product and chunk).
 3. Would the GPU file's statistical bars (3 x the emulation's rms per group, 4 x its max) catch the defects this
    arithmetic is prone to?  Each seeded defect must exceed a bar in at least one group, on one-hot-tap operands (K = Cin)
    at Cin 64 and Cin 512, while the suite's older metric, max|err| / max|ref| < 1e-5, printed alongside, passes most of
    them.  Two accumulation orders of the CORRECT emulation must agree to within a third of the bar (the order a kernel
    happens to use is not what the bar measures); read as: |metric(order A) - metric(order B)| <= bar / 3 in every group.

The same three questions for the dilated kernels of the ContextNetwork (tests/test_ctx_products_gpu.py): the dilated im2col
GEMMs against F.conv2d(dilation=d, padding=d) and its gradients, the seeded defects at K = 32 with 32 .. 128 output columns
(the weakest, one product lost in one 16-channel chunk, is 24 x the rms bar), the value family for kernels that split both
operands in the loop, and the numpy weight pack.

Measured here (rms metric, Gaussian operands): correct 1.9e-8 .. 2.2e-8; a third-order product lost in the tap 7e-7 .. 2e-6;
(1,1) lost in one 16-channel chunk 1.0e-6 (Cin 64), 1.4e-7 (Cin 512); the figures are printed by the tests."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import x3_ref as R

TWO24 = float(1 << 24)


def rs(seed):
    return np.random.RandomState(seed)


# ---------------------------------------------------------------- 1. the reference itself
@pytest.mark.parametrize("family", ["normal", "tiny", "huge", "bf16", "zeros", "wide"])
def test_split_round_trips_bit_for_bit(family):
    r = rs(11)
    v = r.standard_normal(4096).astype(np.float32)
    if family == "tiny":
        v *= np.float32(2.0 ** -90)        # normal values whose last slice is still above the subnormal range of bf16
        v[:3] = [1.0e-30, -2.0 ** -100, 2.0 ** -126]
    elif family == "huge":
        v *= np.float32(2.0 ** 120)
        v[:2] = [3.0e38, -3.0e38]
    elif family == "bf16":
        v = R._trunc16(v)
    elif family == "zeros":
        v[::2] = 0.0
        v[1::4] = -0.0
    elif family == "wide":
        v = v * np.exp2(np.round(r.uniform(-40, 40, v.shape) / np.log(2.0))).astype(np.float32)
    s0, s1, s2 = R.split(v)                                   # asserts the round trip
    for s in (s0, s1, s2):
        assert np.array_equal(R._trunc16(s), s)               # each slice is a bf16 value
    m0 = np.abs(s0).astype(np.float64)
    assert np.all(np.abs(s1) <= m0 * 2.0 ** -7) and np.all(np.abs(s2) <= m0 * 2.0 ** -15)
    if family == "bf16":
        assert not s1.any() and not s2.any()
    if family == "zeros":
        neg = np.signbit(v) & (v == 0)
        assert neg.any() and np.all(np.signbit(s0[neg])) and not np.signbit(s1[neg]).any()


@pytest.mark.parametrize("k,stride", [(3, 1), (3, 2), (1, 2)])
def test_im2col_gemms_are_the_convolution_and_its_gradients(k, stride):
    pad = k // 2
    n, cin, h, w, cout = 2, 5, 7, 6, 4
    r = rs(12)
    x, wt = r.standard_normal((n, cin, h, w)), r.standard_normal((cout, cin, k, k))
    xo, wo = torch.from_numpy(x).requires_grad_(True), torch.from_numpy(wt).requires_grad_(True)
    yo = F.conv2d(xo, wo, None, stride, pad)
    oh, ow = yo.shape[2:]
    g = r.standard_normal(tuple(yo.shape))
    (yo * torch.from_numpy(g)).sum().backward()
    y = R.col2nchw(R.im2col(x, k, stride, pad) @ R.weight_matrix(wt), n, oh, ow)
    assert np.abs(y - yo.detach().numpy()).max() < 1e-12
    dx = R.col2nchw(R.im2col_dgrad(g, k, stride, pad, h, w) @ R.weight_matrix_dgrad(wt), n, h, w)
    assert np.abs(dx - xo.grad.numpy()).max() < 1e-12
    a, b = R.wgrad_operands(x, g, k, stride, pad)
    assert np.abs(R.dw_from_matrix(a @ b, cin, k) - wo.grad.numpy()).max() < 1e-12


def test_product_table_of_the_emulation_on_crafted_slices():
    """Integers in slice i of one operand and slice j of the other: the integer GEMM for the six pairs, zero for the other
    three, bit for bit; a mutated ``keep`` is seen."""
    r = rs(13)
    a, b = R.small_ints(r, (48, 96)), R.small_ints(r, (96, 40))
    want = a.astype(np.float64) @ b.astype(np.float64)
    assert np.abs(a).astype(np.float64).sum(1).max() * 3 < TWO24
    zero = np.zeros_like
    for i in range(3):
        for j in range(3):
            A = [a if s == i else zero(a) for s in range(3)]
            B = [b if s == j else zero(b) for s in range(3)]
            got, top = R.six_product(A, B, order=R.ORDER_SMALL_FIRST, peak=True)
            assert top < TWO24
            assert np.array_equal(got, want if (i, j) in R.SIX else zero(want)), (i, j)
            bad = R.six_product(A, B, keep=[p for p in R.SIX if p != (1, 1)])
            assert np.array_equal(bad, want) == ((i, j) in R.SIX and (i, j) != (1, 1))


@pytest.mark.parametrize("family", [1, 2])
@pytest.mark.parametrize("kind", ["fwd", "dgrad"])
def test_weight_family_cases_of_the_emulation(kind, family):
    """The forward / data-gradient exact case: integers in slice i of the activation, weights with a known split, one tap and
    one 64-channel block at a time.  Slice 0 and 1 see the whole weight (family 2: slice 1 loses s2), slice 2 sees s0 only."""
    r = rs(14 + family)
    n, cin, h, w, cout, k = 1, 128, 5, 4, 64, 3
    if kind == "dgrad":
        cin, cout = cout, cin                                  # the contraction runs over Cout
    cred = cin if kind == "fwd" else cout
    wt, parts = R.weight_family(r, (cout, cin, k, k), family)
    act_shape = (n, cin, h, w) if kind == "fwd" else (n, cout, h, w)
    u = R.small_ints(r, act_shape) if family == 1 else R.one_hot_channels(r, act_shape, values=(1.0,))
    for tap in range(k * k):
        for blk in range(cred // 64):
            ax = 1 if kind == "fwd" else 0
            seen = [R.only_tap(p.astype(np.float32).astype(np.float64), tap, blk, axis=ax) for p in parts]
            if kind == "fwd":
                col, mat = R.im2col(u, k, 1, 1), R.weight_matrix
            else:
                col, mat = R.im2col_dgrad(u, k, 1, 1, h, w), R.weight_matrix_dgrad
            B = [mat(s) for s in seen]
            bound = np.abs(col).astype(np.float64) @ np.abs(mat(R.only_tap(wt, tap, blk, axis=ax))).astype(np.float64)
            assert bound.max() < TWO24                         # every partial sum, in any order, is below 2^24
            for i in range(3):
                A = [col if s == i else np.zeros_like(col) for s in range(3)]
                got, top = R.six_product(A, B, order=R.ORDER_WEIGHT_OUTER, peak=True)
                want = col.astype(np.float64) @ mat(R.weight_seen_by_slice(seen, i))
                assert top < TWO24 and np.array_equal(got, want), (tap, blk, i)
                if i == 2 or (i == 1 and family == 2):
                    assert not np.array_equal(want, col.astype(np.float64) @ sum(B))      # the case tells five from six


@pytest.mark.parametrize("k,stride", [(3, 1), (3, 2), (1, 2)])
def test_one_hot_cases_of_the_emulation(k, stride):
    """The in-loop-split exact cases: a one-hot operand (+-1 / +-2) against a full 24-bit operand returns the other operand's
    value times a power of two, bit for bit, because the prefix sums s0, s0 + s1, s0 + s1 + s2 are fp32 values; any lost
    (i, 0) / (0, j) product shows."""
    r = rs(16)
    pad = k // 2
    n, cin, h, w, cout = 2, 32, 7, 6, 16
    x = r.standard_normal((n, cin, h, w)).astype(np.float32)
    wt = R.one_hot_weights(r, cout, cin, k)
    a, b = R.im2col(x, k, stride, pad), R.weight_matrix(wt)
    ref, _ = R.fp64_and_bound(a, b)
    for order in (R.SIX, R.ORDER_SMALL_FIRST, R.ORDER_WEIGHT_OUTER):
        assert np.array_equal(R.emulate(a, b, order=order), ref)
    for lost in ((1, 0), (2, 0)):
        assert not np.array_equal(R.emulate(a, b, keep=[p for p in R.SIX if p != lost]), ref)
    xh = R.one_hot_channels(r, (n, cin, h, w))
    wf = (r.standard_normal((cout, cin, k, k)) * 0.1).astype(np.float32)
    a, b = R.im2col(xh, 1, 1, 0), R.weight_matrix(wf[:, :, :1, :1])           # one term per output: a 1 x 1 tap
    ref, _ = R.fp64_and_bound(a, b)
    assert np.array_equal(R.emulate(a, b), ref)
    for lost in ((0, 1), (0, 2)):
        assert not np.array_equal(R.emulate(a, b, keep=[p for p in R.SIX if p != lost]), ref)


# ---------------------------------------------------------------- 2. and 3.: the bars against seeded defects
def one_tap_operands(cin, seed, m=48, n=128):
    r = rs(seed)
    a = r.standard_normal((m, cin)).astype(np.float32)
    b = (r.standard_normal((cin, n)) * 0.1).astype(np.float32)
    return a, b


def group_metrics(got, ref, bound, width=64):
    groups = R.channel_groups(ref.shape[1], ref.shape[0], width)
    rms = [R.rms_metric(got[:, a:b], ref[:, a:b], bound[:, a:b]) for a, b in groups]
    mx = [R.max_metric(got[:, a:b], ref[:, a:b], bound[:, a:b]) for a, b in groups]
    return np.array(rms), np.array(mx)


def drop(p):
    return [q for q in R.SIX if q != p]


def seeded_defects(a, b, cin):
    """name -> result of a defective emulation of a @ b (K = cin: one tap)."""
    A, B = R.split(a), R.split(b)
    out = {}
    for p in R.SIX[1:]:
        out["%s lost in the tap" % (p,)] = R.six_product(A, B, keep=drop(p))
    out["(1,1) lost in one 16-channel chunk"] = R.six_product(A, B, defect=(16, 32, drop((1, 1))))
    out["(1,2) in place of (0,2)"] = R.six_product(A, B, keep=drop((0, 2)) + [(1, 2)])
    out["s1 rounded, s2 not adjusted"] = R.six_product(R.split_rounded_s1(a), B)
    return out


@pytest.mark.parametrize("cin", [64, 512])
def test_seeded_defects_exceed_the_statistical_bars(cin):
    a, b = one_tap_operands(cin, 21 + cin)
    ref, bound = R.fp64_and_bound(a, b)
    good = R.emulate(a, b)
    rms0, max0 = group_metrics(good, ref, bound)
    assert all(b_ - a_ == 64 for a_, b_ in R.channel_groups(ref.shape[1], ref.shape[0]))
    whole_max = R.max_metric(good, ref, bound)
    print("\nCin %d  correct: rms %s  max %.2e  old metric %.2e" % (cin, rms0, whole_max, R.old_metric(good, ref)))
    assert rms0.max() <= 2.0 ** -24, "the correct emulation is not fp32 arithmetic"
    assert R.old_metric(good, ref) < 1e-5
    room = {}
    for name, got in seeded_defects(a, b, cin).items():
        rms, mx = group_metrics(got, ref, bound)
        over = max(float((rms / (3 * rms0)).max()), float((mx / (4 * whole_max)).max()))
        room[name] = over
        print("  %-38s rms %.2e (x%.1f of the bar)  max x%.1f of the bar  old metric %.2e%s" %
              (name, rms.max(), (rms / (3 * rms0)).max(), (mx / (4 * whole_max)).max(), R.old_metric(got, ref),
               "  <- passes the old 1e-5 bar" if R.old_metric(got, ref) < 1e-5 else ""))
        assert over > 1.0, (name, over)
    if cin == 64:      # third-order losses are what the old bar cannot see
        a9, b9 = one_tap_operands(9 * cin, 5)
        ref9, _ = R.fp64_and_bound(a9, b9)
        lost = R.six_product(R.split(a9), R.split(b9), defect=(0, cin, drop((1, 1))))
        assert R.old_metric(lost, ref9) < 1e-5


@pytest.mark.parametrize("cin", [64, 512])
def test_two_accumulation_orders_agree_within_a_third_of_the_bar(cin):
    a, b = one_tap_operands(cin, 31 + cin)
    ref, bound = R.fp64_and_bound(a, b)
    o1 = R.emulate(a, b, order=R.ORDER_WEIGHT_OUTER)
    o2 = R.emulate(a, b, order=R.ORDER_SMALL_FIRST, reverse=True)
    assert not np.array_equal(o1, o2)
    (r1, m1), (r2, m2) = group_metrics(o1, ref, bound), group_metrics(o2, ref, bound)
    w1, w2 = R.max_metric(o1, ref, bound), R.max_metric(o2, ref, bound)
    print("\nCin %d  rms %s / %s   max %.2e / %.2e" % (cin, r1, r2, w1, w2))
    for ra, rb, wa, ma, mb in ((r1, r2, w1, m1, m2), (r2, r1, w2, m2, m1)):     # the bar taken from either order
        assert np.all(np.abs(ra - rb) <= (3 * ra) / 3)
        assert np.all(np.abs(ma - mb) <= (4 * wa) / 3)
        assert np.all(rb <= 3 * ra) and np.all(mb <= 4 * wa)
    assert max(r1.max(), r2.max()) <= 2.0 ** -24


# ---------------------------------------------------------------- the dilated kernels of the ContextNetwork (tests/test_ctx_products_gpu.py)
@pytest.mark.parametrize("d,h,w", [(1, 7, 6), (2, 7, 6), (2, 5, 2), (16, 35, 35), (16, 20, 12), (16, 9, 40)])
def test_dilated_im2col_gemms_are_the_dilated_convolution_and_its_gradients(d, h, w):
    """padding = dilation = d, 3 x 3, stride 1; the frames include W <= d (every horizontal side tap outside), H <= d and the
    35 x 35 frame in which only the 3 x 3 centre pixels see all nine taps at d = 16."""
    n, cin, cout, k = 2, 3, 4, 3
    r = rs(17)
    x, wt = r.standard_normal((n, cin, h, w)), r.standard_normal((cout, cin, k, k))
    xo, wo = torch.from_numpy(x).requires_grad_(True), torch.from_numpy(wt).requires_grad_(True)
    yo = F.conv2d(xo, wo, None, 1, d, d)
    assert tuple(yo.shape) == (n, cout, h, w)
    g = r.standard_normal(tuple(yo.shape))
    (yo * torch.from_numpy(g)).sum().backward()
    col = R.im2col(x, k, 1, d, d)
    assert np.abs(R.col2nchw(col @ R.weight_matrix(wt), n, h, w) - yo.detach().numpy()).max() < 1e-12
    dx = R.col2nchw(R.im2col_dgrad(g, k, 1, d, h, w, d) @ R.weight_matrix_dgrad(wt), n, h, w)
    assert np.abs(dx - xo.grad.numpy()).max() < 1e-12
    a, b = R.wgrad_operands(x, g, k, 1, d, d)
    assert np.abs(R.dw_from_matrix(a @ b, cin, k) - wo.grad.numpy()).max() < 1e-12
    for tap in range(9):                                       # a tap that lies outside for every pixel is a zero column block
        ky, kx = divmod(tap, 3)
        outside = (w <= d and kx != 1) or (h <= d and ky != 1)
        assert (not col[:, tap * cin:(tap + 1) * cin].any()) == outside, tap
    if d == 16 and h == 35:
        sees_all = (col.reshape(n, h, w, 9, cin) != 0).all(axis=(3, 4))
        assert sees_all.sum() == 9 * n and sees_all[:, 16:19, 16:19].all()


def test_default_dilation_leaves_the_helpers_bit_identical():
    r = rs(18)
    x, g = r.standard_normal((2, 5, 9, 8)).astype(np.float32), r.standard_normal((2, 4, 5, 4)).astype(np.float32)
    assert np.array_equal(R.im2col(x, 3, 2, 1), R.im2col(x, 3, 2, 1, 1))
    assert np.array_equal(R.im2col_dgrad(g, 3, 2, 1, 9, 8), R.im2col_dgrad(g, 3, 2, 1, 9, 8, 1))
    cols = [x[:, :, ky:ky + 7, kx:kx + 6].transpose(0, 2, 3, 1).reshape(-1, 5) for ky in range(3) for kx in range(3)]
    assert np.array_equal(R.im2col(x, 3, 1, 0), np.concatenate(cols, axis=1))                # written out for d = 1, no padding


def ctx_defects(a, b):
    """The seeded defects at the ContextNetwork geometry (K = 32: two 16-chunks)."""
    A, B = R.split(a), R.split(b)
    out = {}
    for p in R.SIX[1:]:
        out["%s lost in the block" % (p,)] = R.six_product(A, B, keep=drop(p), order=R.ORDER_WEIGHT_OUTER)
    for p in ((1, 1), (0, 2)):
        out["%s lost in one 16-channel chunk" % (p,)] = R.six_product(A, B, defect=(16, 32, drop(p)), order=R.ORDER_WEIGHT_OUTER)
    out["(1,2) in place of (0,2)"] = R.six_product(A, B, keep=drop((0, 2)) + [(1, 2)], order=R.ORDER_WEIGHT_OUTER)
    out["s1 rounded, s2 not adjusted"] = R.six_product(R.split_rounded_s1(a), B, order=R.ORDER_WEIGHT_OUTER)
    return out


@pytest.mark.parametrize("cols", [32, 64, 96, 128])
def test_seeded_defects_exceed_the_statistical_bars_at_the_context_geometry(cols):
    """tests/test_ctx_products_gpu.py keeps the weights live in one tap and one 32-channel block of the contraction, so K = 32;
    378 rows are its smallest frame (2 x 9 x 21 pixels), 32 .. 128 columns the output widths, grouped as there (96 columns: a
    64-wide group and the 32-wide tail).  The kernel's order is ORDER_WEIGHT_OUTER; the correct emulation in another order
    (smallest first, chunks reversed) stays within a third of the bars."""
    a, b = one_tap_operands(32, 41 + cols, m=378, n=cols)
    ref, bound = R.fp64_and_bound(a, b)
    good = R.emulate(a, b, order=R.ORDER_WEIGHT_OUTER)
    rms0, _ = group_metrics(good, ref, bound)
    whole_max = R.max_metric(good, ref, bound)
    groups = R.channel_groups(cols, ref.shape[0])
    assert groups == {32: [(0, 32)], 64: [(0, 64)], 96: [(0, 64), (64, 96)], 128: [(0, 64), (64, 128)]}[cols]
    print("\nK 32, %d columns  correct: rms %s  max %.2e  old metric %.2e" % (cols, rms0, whole_max, R.old_metric(good, ref)))
    assert rms0.max() <= 2.0 ** -24 and R.old_metric(good, ref) < 1e-5
    for name, got in ctx_defects(a, b).items():
        rms, mx = group_metrics(got, ref, bound)
        over_rms, over_max = float((rms / (3 * rms0)).max()), float((mx / (4 * whole_max)).max())
        print("  %-38s rms x%.1f of the bar  max x%.1f of the bar  old metric %.2e%s" %
              (name, over_rms, over_max, R.old_metric(got, ref), "  <- passes the old 1e-5 bar" if R.old_metric(got, ref) < 1e-5 else ""))
        assert max(over_rms, over_max) > 1.0, (name, over_rms, over_max)
    other = R.emulate(a, b, order=R.ORDER_SMALL_FIRST, reverse=True)
    assert not np.array_equal(other, good)
    rms1, max1 = group_metrics(other, ref, bound)
    _, max0 = group_metrics(good, ref, bound)
    assert np.all(np.abs(rms1 - rms0) <= (3 * rms0) / 3) and np.all(np.abs(max1 - max0) <= (4 * whole_max) / 3)
    assert np.all(rms1 <= 3 * rms0) and np.all(max1 <= 4 * whole_max)


def test_loop_family_tells_the_six_products_from_any_other_set():
    """One term a b of the in-loop family (x3_ref.loop_family): the six-product sum is unit_a unit_b LOOP_CC bit for bit in both
    issue orders; dropping any one of the six changes the bits; an extra (1,2) or (2,1) changes them at EVERY position of both
    orders; an extra (2,2) changes them at none (below fp32 resolution)."""
    r = rs(19)
    n = 64
    a, ua = R.loop_family(r, (n, 1))
    b, ub = R.loop_family(r, (1, n))
    assert len(np.unique(ua)) > 8 and (ua < 0).any() and (ua > 0).any()
    want = ua @ ub * R.LOOP_CC                                  # [n, n]: every pair of scales and signs
    assert np.array_equal(want.astype(np.float32).astype(np.float64), want)
    assert not np.array_equal(want, (a.astype(np.float64) @ b.astype(np.float64)).astype(np.float32).astype(np.float64))
    A = [np.concatenate([s, np.zeros((n, 15), np.float32)], axis=1) for s in R.split(a)]     # K = 16 with one live k
    B = [np.concatenate([s, np.zeros((15, n), np.float32)], axis=0) for s in R.split(b)]
    for order in (R.ORDER_SMALL_FIRST, R.ORDER_WEIGHT_OUTER):
        assert np.array_equal(R.six_product(A, B, order=order), want)
        for lost in R.SIX:
            assert not (R.six_product(A, B, keep=drop(lost), order=order) == want).any(), (order, lost)
        for extra in ((1, 2), (2, 1), (2, 2)):
            for pos in range(7):
                seq = list(order[:pos]) + [extra] + list(order[pos:])
                got = R.six_product(A, B, keep=seq, order=seq)
                if extra == (2, 2):
                    assert np.array_equal(got, want), (order, pos)
                else:
                    assert not (got == want).any(), (order, extra, pos)


def test_ctx_pack_layout():
    """x3_ref.ctx_pack against the element formulas of csrc/ctx_common.h, written out as loops."""
    r = rs(20)
    cin, cout = 32, 48
    w = r.standard_normal((cout, cin, 3, 3)).astype(np.float32)
    s = R.split(w)
    fwd, tr = R.ctx_pack(s), R.ctx_pack(s, transposed=True)
    assert fwd.shape == (9, cin // 16, 3, cout, 16) and tr.shape == (9, cout // 16, 3, cin, 16) and fwd.dtype == np.uint16
    bits = [R.bf16_bits(p) for p in s]
    for _ in range(2000):
        co, ci, t, sl = r.randint(cout), r.randint(cin), r.randint(9), r.randint(3)
        assert fwd[t, ci // 16, sl, co, ci % 16] == bits[sl][co, ci, t // 3, t % 3]
        assert tr[t, co // 16, sl, ci, co % 16] == bits[sl][co, ci, (8 - t) // 3, (8 - t) % 3]
