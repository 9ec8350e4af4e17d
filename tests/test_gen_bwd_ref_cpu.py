"""CPU checks of tests/gen_bwd_ref.py, the reference and the checks that tests/test_gen_bwd_products_gpu.py holds the generator's
backward (dmc_gen_tiny_bwd) to.

  * backward64 is the backward of the oracle's dense estimator: with the oracle's own features as ``saved`` it equals
    tests/gen_conditioned.forced_fp64 to 1e-12, parameter by parameter.
  * The checks can see what they are for.  An emulation of the operator on x3_ref.six_product (strips of 32 columns, fragments
    shifted one pixel with an edge pixel per 8, a left column per strip, a plane of ones for the bias) passes every check when
    clean and fails at least one with each seeded defect: a lost (1,1) product in one tap, slice 2 / slice 1 of the edge
    pixel 8 kq - 1 dropped for the shifted taps, a strip's left column from the wrong row, the LeakyReLU branch read from the
    neighbouring pixel, the ones missing in one strip.
  * The clean emulation in another summation order (chunks reversed, products in another order) stays within a third of the
    statistical bars, tap by tap.

Measured here: the one-hot families catch the edge-pixel, left-column and bias defects bit for bit, the branch family the
neighbour's branch; a lost (1,1) product has no term in a one-hot or small-integer operand (their slices 1 and 2 are zero) and
is seen by the statistical layer alone: rms ratio 21 .. 26 and max ratio 24 .. 45 at (2, 3, 36), 6.7 .. 8.4 and 6.4 .. 8.3 at
(1, 30, 64) (bars 3 and 4) -- the emulation's own error grows with the length of the contraction, so the margin is widest on the
small frames."""
import copy

import numpy as np
import pytest
import torch

from oracle import dmc_oracle as O
from tests import gen_bwd_ref as B
from tests import x3_ref as R
from tests.gen_conditioned import forced_fp64, oracle_features

SHAPES = [(2, 3, 36), (1, 30, 64)]


def test_channel_maps():
    for k in range(B.NL):
        idx = B.phys_index(k)
        assert sorted(idx) == list(range(B.cin_of(k)))
        # logical order: y_{k-1}, .., y_0, mv, res
        logical = []
        for j in range(k - 1, -1, -1):
            logical += list(range(B.yoff(j), B.yoff(j) + B.cout_of(j)))
        logical += list(range(B.NIN))
        assert [logical[idx[p]] for p in range(B.cin_of(k))] == list(range(B.cin_of(k)))
    assert B.cin_of(5) == 33 and sum(B.cout_of(k) * B.cin_of(k) for k in range(B.NL)) == 506


@pytest.mark.parametrize("shape", [(2, 5, 7, 9), (1, 5, 1, 5)])
def test_backward64_is_the_oracles_backward(shape):
    o64 = copy.deepcopy(O.seeded_state_fill(O.build_estimator("DenseNetTiny"), 23)).double()
    r = np.random.RandomState(5)
    x64 = torch.from_numpy(r.standard_normal(shape))
    r64 = torch.from_numpy(r.standard_normal((shape[0], 2) + shape[2:]))
    feats = oracle_features(o64, x64)
    assert all((f > 0).any() and (f < 0).any() for f in feats)
    _, want = forced_fp64(o64, x64, r64, [f > 0 for f in feats])
    ws = [getattr(o64, "conv_%d" % k)[0].weight.detach().numpy() for k in range(5)] + [o64.predict_flow.weight.detach().numpy()]
    g, dw, db = B.backward64(x64[:, :2].numpy(), x64[:, 2:].numpy(), torch.cat(feats, 1).numpy(), ws, r64.numpy())
    assert [t.shape[1] for t in g] == list(B.WIDTHS)
    for k in range(B.NL):
        for got, ref in ((dw[k], want[2 * k]), (db[k], want[2 * k + 1])):
            ref = ref.numpy()
            assert got.shape == ref.shape
            assert np.abs(got - ref).max() <= 1e-12 * np.abs(ref).max(), k


def test_wino_bound_covers_the_transform():
    """The absolute-value bound is at least the direct sum |f||d| and at most 81 x it (per axis the rows of |G| sum to <= 1.5,
    those of |B^T| to 2, those of |A^T| to 3), and an integer filter's transform is a multiple of 1/4."""
    r = np.random.RandomState(3)
    d, f = np.abs(R.small_ints(r, (1, 3, 5, 8))).astype(np.float64), np.abs(R.small_ints(r, (2, 3, 3, 3), amax=2)).astype(np.float64)
    direct = float(torch.nn.functional.conv2d(torch.from_numpy(d), torch.from_numpy(f), padding=1).max())
    wb = B.wino_bound(d, f)
    assert direct <= wb <= 81 * direct
    U = np.einsum("ia,dcab,jb->dcij", B.WINO_G, f, B.WINO_G)
    assert np.array_equal(U * 4, np.round(U * 4))


def emu_run(defect=None, **kw):
    return lambda *ops: B.emulate_backward(*ops, defect=defect, **kw)


def all_checks(run, shape):
    """Every check of tests/test_gen_bwd_products_gpu.py against ``run``; returns the names of those that fail."""
    failed = []

    def stat(family):
        rms, mx, _ = B.statistics(run, shape, family, 700)
        assert rms <= 3.0 and mx <= 4.0, (rms, mx)
    checks = [("integer", lambda: B.check_integer(run, B.integer_operands(shape, 11))),
              ("branch", lambda: B.check_branch(run, shape, 21)),
              ("g one-hot", lambda: B.check_g_one_hot(run, shape, 31)),
              ("inputs one-hot", lambda: B.check_in_one_hot(run, shape, 41)),
              ("statistics gauss", lambda: stat("gauss")), ("statistics wide", lambda: stat("wide"))]
    for name, fn in checks:
        try:
            fn()
        except AssertionError as e:
            failed.append((name, str(e)[:160]))
    return failed


@pytest.mark.parametrize("shape", SHAPES)
def test_clean_emulation_passes_every_check(shape):
    assert all_checks(emu_run(), shape) == []


DEFECTS = {
    "(1,1) lost in layer 1, tap 3": B.Defect(lost11=(1, 3)),
    "(1,1) lost in layer 2, tap 8": B.Defect(lost11=(2, 8)),
    "slice 2 of the edge pixel dropped": B.Defect(edge_drop=2),
    "slice 1 of the edge pixel dropped": B.Defect(edge_drop=1),
    "left column of strip 1 from the wrong row": B.Defect(left_row=1),
    "branch from the neighbouring pixel": B.Defect(branch_shift=True),
    "ones missing in strip 1": B.Defect(ones_missing=1),
}


@pytest.mark.parametrize("name", sorted(DEFECTS))
@pytest.mark.parametrize("shape", SHAPES)
def test_every_seeded_defect_fails_a_check(shape, name):
    failed = all_checks(emu_run(DEFECTS[name]), shape)
    print("\n%s %s: fails %s" % (shape, name, [f[0] for f in failed]))
    assert failed, name


@pytest.mark.parametrize("family", ["gauss", "wide"])
@pytest.mark.parametrize("shape", SHAPES + [(1, 2, 4)])
def test_two_summation_orders_agree_within_a_third_of_the_bars(shape, family):
    _, _, (r1, e1, m1, w1) = B.statistics(emu_run(), shape, family, 700)
    _, _, (r2, e2, m2, w2) = B.statistics(emu_run(order=R.ORDER_WEIGHT_OUTER, reverse=True), shape, family, 700)
    assert np.array_equal(e1, e2) and w1 == w2                     # the bars' reference is the same
    assert not np.array_equal(r1, r2)
    print("\n%s %s  rms / emulation %s | %s   max / emulation max %s | %s" %
          (shape, family, np.round(r1 / e1, 3), np.round(r2 / e1, 3), np.round(m1 / w1, 3), np.round(m2 / w1, 3)))
    assert np.all(np.abs(r1 - r2) <= (3 * e1) / 3)
    assert np.all(np.abs(m1 - m2) <= (4 * w1) / 3)
