"""The bounds of tests/bn2d_ref.py against themselves, without a GPU: an fp32 emulation that follows bn_act.hip's rounding
points and summation order must sit well inside every bound, and each of a list of seeded defects must break at least one
-- otherwise test_bn2d_fp64_gpu.py, which uses these bounds, could not tell a wrong kernel from a right one.

Headroom: the emulation has to stay within fmt + arith / 4 (bn3d_ref.Bound), the rule of test_bn3d_ref_cpu.py: only the
accumulated part of a bound can be asked for headroom (what counts as accumulated for an fp32 result: bn2d_ref's docstring).
For every defect the old metric of the suite (rel_err = max |a - b| / max |b| over the whole tensor, bars 1e-5 for y and the
running statistics, 1e-4 for dx, dgamma, dbeta) is printed next to the new ratio; the old metric is taken on the data the
older tests present (N(0, 1) in every channel, bn2d_case(kind="plain")) with the same defect at the same shape."""
import numpy as np
import pytest
import torch

from tests import bn2d_ref as R

EPS, MOM = 1e-5, 0.1
HEADROOM = 4.0
OLD_BARS = dict(y=1e-5, rm=1e-5, rv=1e-5, dx=1e-4, dgamma=1e-4, dbeta=1e-4, dres=1e-5)
_CACHE = {}

CPU_SHAPES = [s for s in R.BN_SHAPES if R.rows_of(s) * s[1] <= 1 << 20]
EMPTY_WG = (161, 1024, 1, 1)                                    # M = 161, split 20, per 9: two empty workgroups


def case_of(shape, kind="normal"):
    key = (shape, kind)
    if key not in _CACHE:
        _CACHE[key] = R.bn2d_case(shape, seed=2000 + shape[1] + shape[0], kind=kind)
    return _CACHE[key]


def npf(t):
    return t.numpy()


def old_metric(got, ref):
    got, ref = torch.as_tensor(got).double(), ref.double()
    if not bool(torch.isfinite(got).all()):
        return float("inf")
    return float((got - ref).abs().max() / ref.abs().max().clamp_min(1e-30))


def emulate(case, res, relu, use_mask, partials64=None, defect=None, keep=None, slope=0.0):
    """The training step of one unit in the emulation; returns numpy outputs."""
    x, M, C = npf(case["x"]), case["M"], case["C"]
    if partials64 is None:
        p0, p1 = R.emu_partials(x, x, x, M, C, R.split_of(M, C), empty_fill=float("nan") if defect == "empty_uninit" else 0.0)
    else:
        part = R.make_partials64(case["x"], partials64).numpy()
        p0, p1 = part[:, :, 0], part[:, :, 1]
    st = R.emu_stats_final(p0, p1, M, npf(case["rm"]), npf(case["rv"]), EPS, MOM, defect)
    r = npf(case["res"]) if res else None
    y, mask = R.emu_apply_fwd(x, st["mean"], st["invstd"], npf(case["gamma"]), npf(case["beta"]), r, relu, defect)
    out = dict(st, y=y, mask=mask)
    if np.isfinite(st["invstd"]).all() and np.isfinite(st["mean"]).all():
        b = R.emu_backward(x, npf(case["dy"]), st["mean"], st["invstd"], npf(case["gamma"]), npf(case["beta"]), r, relu,
                           mask if use_mask else None, keep=keep, hw=case["hw"], slope=slope, defect=defect)
        out.update(b)
    return out


def judge(case, got, res, relu, n_stats, headroom=1.0, keep=None, slope=0.0):
    """error / bound of every output of emulate() (bn2d_ref.unit_ratios), and the old metric of the same outputs against a
    full fp64 evaluation."""
    x = case["x"]
    t = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a))
    got = {k: t(v) for k, v in got.items()}
    kp = t(keep)
    new = R.unit_ratios(case, got, res, relu, n_stats, headroom, keep=kp, slope=slope, eps=EPS, momentum=MOM)
    new.pop("cond", None), new.pop("dx_arith", None)
    st = R.Stats(x, EPS, 0)
    (rm, _), (rv, _) = st.running(case["rm"], case["rv"], MOM)
    old = dict(rm=old_metric(got["rm"], rm), rv=old_metric(got["rv"], rv))
    if "y" in new:
        full = R.forward_ref(x, st.mean, st.invstd, case["gamma"], case["beta"], case["res"] if res else None, relu)[0]
        old["y"] = old_metric(got["y"], full)
        if "dx" in got:
            fullb = R.backward_ref(x, case["dy"], st.mean, st.invstd, case["gamma"], 0, keep_mask=(full > 0) if relu else None,
                                   keep=kp, hw=case["hw"], slope=slope)
            for k in ("dx", "dgamma", "dbeta"):
                old[k] = old_metric(got[k], fullb[k][0])
    return new, old


def broken(new):
    return sorted(k for k, v in new.items() if not v <= 1.0)


def show(tag, new, old):
    print("  %s\n    new (error / bound): %s\n    old (rel_err / bar):  %s   -> old suite %s" % (
        tag, "  ".join("%s %.3g" % kv for kv in new.items()), "  ".join("%s %.3g" % (k, v / OLD_BARS[k]) for k, v in old.items()),
        "SEES it" if any(v > OLD_BARS[k] for k, v in old.items()) else "passes"))


# ------------------------------------------------------------------------------------------ the case itself
@pytest.mark.parametrize("kind", ["normal", "dyadic"])
def test_every_regime_is_present(kind):
    case = case_of((4, 64, 56, 56), kind)
    x, g, b = case["x"].double(), case["gamma"], case["beta"]
    st = R.Stats(case["x"], EPS, 9)
    ratio_ = (st.mean.abs() / st.var.sqrt().clamp_min(1e-300))
    assert float(x[:, 1].var(unbiased=False)) == 0.0 and float(x[0, 1]) == R.CONST_VALUE          # constant channel
    assert float(g[2]) == 0.0 and bool((g > 0).any()) and bool((g < 0).any())
    assert float(b[10]) >= 12.0 and float(b[11]) <= -12.0
    assert bool((x[:, 10].sub(st.mean[10]).mul(st.invstd[10] * g[10].double()).add(12.0) > 0).all())
    assert bool((x[:, 11].sub(st.mean[11]).mul(st.invstd[11] * g[11].double()).sub(12.0) < 0).all())
    if kind == "normal":
        for want in (8.0, 64.0, 128.0):
            assert bool(((ratio_ - want).abs() < 0.05 * want).any()), want
        assert bool((st.mean < -50 * st.var.sqrt()).any()) and bool((st.mean > 50 * st.var.sqrt()).any())
        assert float(st.var[8]) < 0.2 * R.f32(EPS) and float(st.var[9]) > 2.0 ** 19               # var << eps, scale 2^10
        cond = st.cond.clone()
        cond[1::16] = 0                                         # (the constant channels: mean^2 / eps, and exact all the same)
        assert 1.0e4 < float(cond.max()) < 3.0e4, float(cond.max())
        assert not bool(R.exact_sums(case["x"])[0])
    else:
        ex = R.exact_sums(case["x"])
        assert bool(ex[0]) and bool(ex[1]) and int(ex.sum()) >= 24, int(ex.sum())                # exact partial sums, proved
        assert float(g.abs()[g != 0].min()) >= 0.25 and bool((g[::3][g[::3] != 0] < 0).all())
    assert bool(R.exact_sums(case["x"])[1])


def test_geometry_of_the_shapes():
    geo = lambda s: R.geometry(R.rows_of(s), s[1])
    want = {(1, 4, 1, 1): (1, 1, 0), (2, 16, 5, 7): (1, 2, 0), (1, 1024, 3, 3): (1, 9, 0), (5, 512, 7, 7): (15, 9, 0),
            (977, 64, 1, 1): (7, 9, 0), (3, 256, 37, 61): (211, 9, 5), (4, 64, 56, 56): (98, 8, 0), (32717, 64, 1, 1): (255, 9, 1),
            (32769, 64, 1, 1): (256, 9, 1), (32996, 64, 1, 1): (257, 9, 1), (131004, 64, 1, 1): (1023, 9, 7),
            (3, 64, 210, 210): (1024, 9, 6), (6, 512, 53, 53): (1024, 9, 32), (6, 64, 210, 210): (1024, 17, 2)}
    for s in R.BN_SHAPES:
        g = geo(s)
        assert (g["split"], g["iters"], g["empty"]) == want[s], (s, g)
    wraps = [s for s in R.BN_SHAPES if R.stream_wraps(R.rows_of(s), s[1], 4)]
    assert wraps == [(3, 64, 210, 210), (6, 512, 53, 53), (6, 64, 210, 210)]
    assert [s for s in R.BN_SHAPES if R.stream_wraps(R.rows_of(s), s[1], 8)] == [(6, 64, 210, 210)]
    assert R.geometry(161, 1024)["empty"] == 2
    assert R.pool_blocks(3, 112, 112) == 147 and R.pool_tiles(2, 129, 127) == 2 * 9 * 8 and R.pool_blocks(120, 112, 112) == 1024


# ------------------------------------------------------------------------------------------ the faithful emulation
@pytest.mark.parametrize("res,relu,use_mask", [(0, 0, 0), (0, 1, 0), (1, 1, 1), (1, 1, 0), (1, 0, 0)])
@pytest.mark.parametrize("shape", CPU_SHAPES, ids=str)
def test_faithful_emulation_keeps_every_bound_with_headroom(shape, res, relu, use_mask):
    case = case_of(shape)
    got = emulate(case, res, relu, use_mask)
    new, _ = judge(case, got, res, relu, R.chain_of(case["x"], case["M"], case["C"]), headroom=HEADROOM)
    print("  emulation %s res=%d relu=%d mask=%d  error / (fmt + arith / %g): %s" % (
        shape, res, relu, use_mask, HEADROOM, "  ".join("%s %.3f" % kv for kv in new.items())))
    assert not broken(new), new
    if case["M"] > 1:                                           # the constant channel: exact, whatever its conditioning
        c = 1
        assert float(got["mean"][c]) == R.CONST_VALUE and float(got["invstd"][c]) == float(np.float32(1.0 / np.sqrt(np.float64(np.float32(EPS)))))
        if not res:
            want = max(float(case["beta"][c]), 0.0) if relu else float(case["beta"][c])
            assert bool((got["y"][:, c] == np.float32(want)).all())


@pytest.mark.parametrize("nblk", [1, 255, 257])
def test_faithful_emulation_with_fp64_partials(nblk):
    """The conv_stats_final_kernel path (n = 0): nothing but the stored values' own roundings is allowed."""
    case = case_of((4, 64, 56, 56))
    got = emulate(case, 1, 1, 1, partials64=nblk)
    new, _ = judge(case, got, 1, 1, 0, headroom=HEADROOM)
    print("  fp64 partials nblk=%d: %s" % (nblk, "  ".join("%s %.3f" % kv for kv in new.items())))
    assert not broken(new), new


def test_faithful_emulation_of_the_keep_and_slope_tail():
    case = case_of((5, 512, 7, 7))
    keep = np.random.RandomState(5).choice([0.0, 1.0, 2.0, 0.5], (5, 512)).astype(np.float32)
    got = emulate(case, 0, 0, 0, keep=keep, slope=0.2)
    new, _ = judge(case, got, 0, 0, R.chain_of(case["x"], 245, 512), headroom=HEADROOM, keep=keep, slope=0.2)
    assert not broken(new), new


# ------------------------------------------------------------------------------------------ seeded defects
def defect_case(shape, defect, res=1, relu=1, use_mask=1, partials64=None, keep=None, slope=0.0, kind="normal"):
    case = case_of(shape, kind)
    got = emulate(case, res, relu, use_mask, partials64=partials64, defect=defect, keep=keep, slope=slope)
    n = 0 if partials64 else R.chain_of(case["x"], case["M"], case["C"])
    new, _ = judge(case, got, res, relu, n, keep=keep, slope=slope)
    plain = case_of(shape, "plain")                             # the old metric on the data the old tests present
    _, old = judge(plain, emulate(plain, res, relu, use_mask, partials64=partials64, defect=defect, keep=keep, slope=slope),
                   res, relu, n if partials64 else R.geometry(plain["M"], plain["C"])["iters"], keep=keep, slope=slope)
    show("%s at %s" % (defect, shape), new, old)
    return broken(new)


def test_defect_biased_running_variance():
    """M = 12,544: the bias is 0.1 var / M = 8e-6 var, below the old bar."""
    assert defect_case((4, 64, 56, 56), "biased") == ["rv"]


def test_defect_tail_partial_dropped():
    assert R.geometry(245, 512)["split"] % 32 != 0
    assert {"mean", "invstd"} <= set(defect_case((5, 512, 7, 7), "tail_partial"))


def test_defect_empty_workgroup_partial_uninitialised():
    assert "mean" in defect_case(EMPTY_WG, "empty_uninit")


def test_defect_empty_workgroup_partial_uninitialised_backward():
    case = case_of(EMPTY_WG)
    good = emulate(case, 1, 1, 1)
    bad = R.emu_backward(npf(case["x"]), npf(case["dy"]), good["mean"], good["invstd"], npf(case["gamma"]), npf(case["beta"]),
                         npf(case["res"]), 1, good["mask"], defect="empty_uninit")
    new, _ = judge(case, dict(good, **bad), 1, 1, R.chain_of(case["x"], 161, 1024))
    old = dict(dx=float("inf"), dgamma=float("inf"), dbeta=float("inf"))          # (NaN in any data)
    show("empty_uninit (backward) at %s" % (EMPTY_WG,), new, old)
    assert {"dgamma", "dbeta", "dx"} <= set(broken(new))


def test_defect_mean_rounded_before_it_is_squared():
    """fp64-partials path: squaring the fp32 mean costs cond u / 2 in invstd -- the channels with |mean| = 64 .. 128 deviations
    show it, the tensor-wide metric on y does not."""
    assert "invstd" in defect_case((4, 64, 56, 56), "mean32_sq", partials64=257)


def test_defect_relu_sign_recomputed_without_the_residual():
    assert {"dx", "dres"} <= set(defect_case((2, 16, 5, 7), "relu_no_res", use_mask=0))


def test_defect_mask_bits_reversed():
    assert "mask" in defect_case((977, 64, 1, 1), "mask_reversed")


def test_defect_dgamma_and_dbeta_exchanged():
    assert {"dgamma", "dbeta"} <= set(defect_case((1, 1024, 3, 3), "swap"))


def test_defect_keep_indexed_by_row():
    keep = np.random.RandomState(5).choice([0.0, 1.0, 2.0, 0.5], (5, 512)).astype(np.float32)
    assert defect_case((5, 512, 7, 7), "keep_row", res=0, relu=0, use_mask=0, keep=keep, slope=0.2) == ["dx"]


# ------------------------------------------------------------------------------------------ the stem tail
def pool_case(shape):
    key = ("pool", shape)
    if key not in _CACHE:
        n, c, h, w = shape
        case = R.bn2d_case(shape, seed=2000 + c + n, kind="dyadic")        # (the GPU file's cases)
        x = case["x"]
        st = R.emu_stats_final(*R.emu_partials(npf(x), npf(x), npf(x), case["M"], c, R.split_of(case["M"], c)), case["M"],
                               npf(case["rm"]), npf(case["rv"]), EPS, MOM)
        case["mean"], case["inv"] = torch.from_numpy(st["mean"]), torch.from_numpy(st["invstd"])
        case["x4"] = x.view(n, h, w, c)
        case["ref"] = R.pool_ref(case["x4"], case["mean"], case["inv"], case["gamma"], case["beta"])
        ph, pw = R.pool_dims(h, w)
        case["dpool"] = torch.from_numpy(np.random.RandomState(7).standard_normal((n, ph, pw, c)).astype(np.float32))
        _CACHE[key] = case
    return _CACHE[key]


@pytest.mark.parametrize("shape", R.POOL_SHAPES, ids=str)
def test_pool_reference_alone_decides_the_dyadic_windows(shape):
    """The GPU file's condition is: undecided share <= 1e-4 and every decided window exact.  The reference alone has to meet
    the cap, or the condition would be empty."""
    ref = pool_case(shape)["ref"]
    print("  pool %s: %d undecided of %d windows" % (shape, ref["n_undecided"], ref["windows"]))
    assert ref["undecided"] <= 1e-4


def pool_judge(case, fwd, bwd, shape, tile=False, headroom=1.0):
    n, c, h, w = shape
    ref = case["ref"]
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a))
    dec = ref["decided"]
    new = dict(y=R.ratio(t(fwd["y"])[dec], ref["y"][dec], R.Bound(ref["b_y"].fmt[dec], ref["b_y"].arith[dec])),
               code=0.0 if torch.equal(t(fwd["code"])[dec], ref["code"][dec]) else float("inf"),
               xmax=0.0 if torch.equal(t(fwd["xmax"])[dec], ref["xmax"][dec]) else float("inf"))
    old = {}
    if bwd is not None and int(t(fwd["code"]).max()) <= 8:
        ph, pw = R.pool_dims(h, w)
        try:
            back = R.pool_backward_ref(case["x4"], case["dpool"], t(fwd["code"]), case["mean"], case["inv"], case["gamma"], case["beta"],
                                       R.pool_tile_chain(n, h, w, c) if tile else R.geometry(n * ph * pw, c)["iters"], 3 if tile else 0)
        except AssertionError:
            new["route"] = float("inf")
            return new, old
        for k in ("dx", "dgamma", "dbeta"):
            got = t(bwd[k]).reshape(back[k][0].shape)
            new[k] = R.ratio(got, back[k][0], back[k][1], headroom)
            old[k] = old_metric(got, back[k][0])
    return new, old


@pytest.mark.parametrize("shape", [s for s in R.POOL_SHAPES if R.rows_of(s) * s[1] <= 1 << 20], ids=str)
def test_pool_emulation_keeps_every_bound(shape):
    case = pool_case(shape)
    a = (npf(case["x4"]), npf(case["mean"]), npf(case["inv"]), npf(case["gamma"]), npf(case["beta"]))
    fwd = R.emu_pool_fwd(*a)
    bwd = R.emu_pool_bwd_arg(a[0], npf(case["dpool"]), fwd["code"], fwd["xmax"], *a[1:])
    new, _ = pool_judge(case, fwd, bwd, shape, headroom=HEADROOM)
    tile, _ = pool_judge(case, fwd, R.emu_pool_bwd_tile(a[0], npf(case["dpool"]), fwd["code"], *a[1:]), shape, tile=True, headroom=HEADROOM)
    new.update({"tile_" + k: tile[k] for k in ("dx", "dgamma", "dbeta")})
    print("  pool emulation %s: %s" % (shape, "  ".join("%s %.3f" % kv for kv in new.items())))
    assert not broken(new), new


@pytest.mark.parametrize("defect,shape,seen", [("tie_last", (2, 64, 17, 23), "code"), ("clamped_wins", (2, 64, 30, 31), "code"),
                                               ("inv_count_pooled", (2, 128, 8, 8), "dx")])
def test_pool_defects(defect, shape, seen):
    case = pool_case(shape)
    a = (npf(case["x4"]), npf(case["mean"]), npf(case["inv"]), npf(case["gamma"]), npf(case["beta"]))
    fwd = R.emu_pool_fwd(*a, defect=defect)
    good = R.emu_pool_fwd(*a)
    bwd = R.emu_pool_bwd_arg(a[0], npf(case["dpool"]), good["code"], good["xmax"], *a[1:], defect=defect)
    new, old = pool_judge(case, fwd, bwd, shape)
    old["y"] = old_metric(fwd["y"], case["ref"]["y"])
    show("%s at %s" % (defect, shape), new, old)
    assert seen in broken(new)
