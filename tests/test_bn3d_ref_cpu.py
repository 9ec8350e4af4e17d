"""The bounds of tests/bn3d_ref.py against themselves, without a GPU: an fp32 emulation that follows bn3d_bf16.hip's
rounding points and blockwise partials must sit well inside every bound, and each of a list of seeded defects must
break at least one -- otherwise the GPU tests that use these bounds (test_unit3d_chain_gpu.py) could not tell a wrong
kernel from a right one.

Headroom: the emulation has to stay within fmt + arith / 4 (bn3d_ref.Bound).  The fmt part is the single rounding of the
stored value into fp32 or bf16, which a correct kernel attains exactly (an element just above a power of two errs by
the whole 2^-8 |ref|), so only the accumulated part can be asked for headroom."""
import numpy as np
import pytest
import torch

from tests import bn3d_ref as R

EPS, MOM = 1e-5, 0.1
HEADROOM = 4.0
_CACHE = {}


def operands(M, C, spread):
    key = (M, C, spread)
    if key not in _CACHE:
        case = R.bn_case(M, C, 1000 + C, spread)
        case["part"] = R.make_partials(case["y"])
        case["stats"] = R.Stats(case["y"], EPS, R.TEST_PART_CHAIN)
        _CACHE[key] = case
    return _CACHE[key]


def npf(t):
    return t.float().numpy()


def ratios(case, relu, part=None, fwd_defect=None, bwd_defect=None, headroom=1.0):
    """Every checked quantity's worst error / bound for the emulation (optionally with a seeded defect)."""
    st, y, dout = case["stats"], case["y"], case["dout"]
    part = case["part"] if part is None else part
    f = R.emulate_forward(npf(y), part.numpy(), npf(case["gamma"]), npf(case["beta"]), npf(case["rm"]), npf(case["rv"]),
                          EPS, MOM, relu, fwd_defect)
    out = torch.from_numpy(f["out"])
    (rm, b_rm), (rv, b_rv) = st.running(case["rm"], case["rv"], MOM)
    ref_out, b_out = R.forward_ref(y, st, case["gamma"], case["beta"], relu)
    res = dict(mean=R.ratio(f["mean"], st.mean, st.b_mean, headroom), invstd=R.ratio(f["invstd"], st.invstd, st.b_invstd, headroom),
               rm=R.ratio(f["rm"], rm, b_rm, headroom), rv=R.ratio(f["rv"], rv, b_rv, headroom),
               out=R.ratio(out, ref_out, b_out, headroom))
    if np.isfinite(f["invstd"]).all():
        b = R.emulate_backward(npf(dout), npf(y), f["mean"], f["invstd"], npf(case["gamma"]), npf(case["beta"]), relu, bwd_defect)
        ref = R.backward_ref(dout, y, out, st, case["gamma"], relu, R.bn3_bwd_chain(*y.shape))
        for k in ("dy", "dgamma", "dbeta"):
            res[k] = R.ratio(b[k], ref[k][0], ref[k][1], headroom)
    return res


@pytest.mark.parametrize("relu", [0, 1])
@pytest.mark.parametrize("shape", R.BN_SHAPES)
def test_faithful_emulation_keeps_every_bound_with_headroom(shape, relu):
    case = operands(*shape)
    assert float(case["stats"].var[3]) == 0.0 and float(case["gamma"][2]) == 0.0 and float(case["gamma"][1]) < 0
    res = ratios(case, relu, headroom=HEADROOM)
    print("  emulation M=%d C=%d relu=%d  error / (fmt + arith / %g): %s  (cond max %.1f)" % (
        shape[0], shape[1], relu, HEADROOM, "  ".join("%s %.3f" % kv for kv in res.items()), float(case["stats"].cond[[0, 1, 2] + list(range(4, shape[1]))].max())))
    assert all(v <= 1.0 for v in res.values()), res


def test_geometry_of_the_shapes():
    """The shapes reach what they are there for (bn3_blocks of bn3d_bf16.hip mirrored in bn3_geometry)."""
    assert R.bn3_geometry(333, 208) == (9, 19, 2)
    assert R.bn3_geometry(2500, 2048) == (1, 1024, 3)
    assert R.bn3_geometry(2 * 1024 * 256 + 77, 8) == (256, 1024, 3)
    assert R.bn3_geometry(2, 8) == (256, 1, 1) and R.bn3_geometry(2500, 64) == (32, 40, 2)


def broken(res):
    return sorted(k for k, v in res.items() if not v <= 1.0)


@pytest.mark.parametrize("shape", [(333, 208, False), (600, 24, False)])
def test_a_pixel_left_out_of_the_sums_is_seen(shape):
    case = operands(*shape)
    y = case["y"].clone()
    y[shape[0] // 2] = 0                                         # the sums skip one pixel; M stays
    assert "mean" in broken(ratios(case, 1, part=R.make_partials(y)))


@pytest.mark.parametrize("shape", [(2500, 64, True), (2500, 2048, False)])
def test_biased_variance_in_the_running_update_is_seen(shape):
    assert broken(ratios(operands(*shape), 1, fwd_defect="biased")) == ["rv"]


@pytest.mark.parametrize("shape", R.BN_SHAPES[:5])
def test_a_flipped_relu_mask_element_is_seen(shape):
    case = operands(*shape)
    m = int((case["dout"][:, 0].float().abs() - 0.67).abs().argmin())     # a gradient of typical size (the median of |N(0, 1)|)
    assert "dy" in broken(ratios(case, 1, bwd_defect=("flip", m, 0)))


@pytest.mark.parametrize("shape", R.BN_SHAPES[:5])
def test_dgamma_summed_without_the_mask_is_seen(shape):
    assert "dgamma" in broken(ratios(operands(*shape), 1, bwd_defect="nomask_dgamma"))


@pytest.mark.parametrize("shape", R.BN_SHAPES[:5])
def test_momentum_the_wrong_way_round_is_seen(shape):
    assert broken(ratios(operands(*shape), 1, fwd_defect="momentum")) == ["rm", "rv"]


@pytest.mark.parametrize("shape", R.BN_SHAPES[:5])
def test_eps_dropped_on_the_constant_channel_is_seen(shape):
    assert {"invstd", "out"} <= set(broken(ratios(operands(*shape), 0, fwd_defect="noeps")))
