"""The classifier's fp32 BatchNorm2d kernels (csrc/bn_act.hip, conv_stats_final_kernel of csrc/conv_nhwc.hip) held to fp64 per
element and per channel, through the C ABI.

Every tolerance is a bound derived in tests/bn2d_ref.py from the kernels' arithmetic (checked against an emulation and against
seeded defects in test_bn2d_ref_cpu.py); a result passes when error / bound <= 1 for EVERY element -- one wrong channel of 512, or
a channel whose scale is 2^-10 of the largest, fails it.  Each stage is judged on the operands it really had (the stored
statistics, the kernel's own ReLU decision, the kernel's arg-max codes).  Output buffers are NaN-filled before each call, every
call runs twice and must repeat bit for bit.  The data have per-channel regimes (bn2d_ref.bn2d_case): means of up to 128
deviations (cond up to 2 10^4), scales 2^-10 and 2^10, a constant channel, gamma of both signs and 0.

Shapes (geometry from bn2d_ref.geometry, asserted in test_bn2d_ref_cpu.py):
    (N, C, H, W)          M       split  iters  reaches
    (1, 4, 1, 1)          1       1      1      count == 1, one float4 column
    (2, 16, 5, 7)         70      1      2      smallest slice-kernel C
    (1, 1024, 3, 3)       9       1      9      256 float4 columns, one thread row
    (5, 512, 7, 7)        245     15     9      layer4, two thread rows
    (977, 64, 1, 1)       977     7      9      ragged rows
    (3, 256, 37, 61)      6771    211    9      5 empty workgroups
    (4, 64, 56, 56)       12544   98     8      layer1 tile
    (32717 / 32769 / 32996 / 131004, 64, 1, 1)  split 255 / 256 / 257 / 1023: bn_bwd_final_kernel's 4-per-thread tail,
                                                reduce_partials' 32-lane tail
    (3, 64, 210, 210)     132300  1024   9      split capped, 6 empty workgroups; the 4-channel kernels wrap
    (6, 512, 53, 53)      16854   1024   9      32 empty workgroups; wrap at C = 512
    (6, 64, 210, 210)     264600  1024   17     the 8-channel slice kernels wrap

Measured on an MI355X (error / bound, worst over all cases): mean 0.993, invstd 0.998, running mean / var 0.72 / 0.70, y 0.999 (each its
own roundings: fmt), dx 0.68 (0.025 of its accumulated part), dgamma 0.20, dbeta 0.23, dx from slices only 0.92, pool: pooled map 0.93,
codes / xmax exact, 0 undecided windows of 1.18 M, dx 0.46, dgamma 0.51, dbeta 0.94; eval-mode invstd 0.42.  DESIGN.md section 4.6."""
import numpy as np
import pytest
import torch

import dmcnet_amd
from dmcnet_amd import ops
from tests import bn2d_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
L = dmcnet_amd._lib
EPS, MOM = 1e-5, 0.1
NAN = float("nan")
WORST = {}
_CASES = {}

#: (residual, relu, mask bytes): the unit forms of the ResNet, and both ways the backward learns the ReLU decision
COMBOS = [(0, 0, 0), (0, 1, 0), (1, 1, 1), (1, 1, 0), (1, 0, 0)]
SLICE_SHAPES = [s for s in R.BN_SHAPES if s[1] % 16 == 0]


def case_of(shape, kind="normal"):
    key = (shape, kind)
    if key not in _CASES:
        if len(_CASES) > 3:                                      # (the large cases are 34 and 68 MB a tensor)
            _CASES.clear()
        c = R.bn2d_case(shape, seed=2000 + shape[1] + shape[0], kind=kind)
        _CASES[key] = {k: (v.to(DEV) if torch.is_tensor(v) else v) for k, v in c.items()}
    return _CASES[key]


def nanf(*shape):
    return torch.full(shape, NAN, dtype=torch.float32, device=DEV)


def report(what, res):
    info = {k: res.pop(k) for k in ("cond", "dx_arith", "undecided") if k in res}
    for k, v in res.items():
        WORST[k] = max(WORST.get(k, 0.0), v)
    for k, v in info.items():
        WORST["(" + k + ")"] = max(WORST.get("(" + k + ")", 0.0), v)
    print("  %s  error / bound: %s  %s" % (what, "  ".join("%s %.3f" % kv for kv in res.items()), "  ".join("%s=%.4g" % kv for kv in info.items())))
    print("  worst so far: %s" % "  ".join("%s %.4g" % kv for kv in sorted(WORST.items())))
    assert all(v <= 1.0 for v in res.values()), (what, res)


def twice(fn):
    """Every call runs twice on fresh NaN-filled buffers and must repeat bit for bit."""
    a, b = fn(), fn()
    torch.cuda.synchronize()
    for k in a:
        if a[k] is not None:
            assert R.same_bits(a[k], b[k]), "%s differs between two runs" % k
    return a


def scratch_of(C):
    lib = L.load()
    return torch.full((lib.dmc_bn_act_scratch_bytes(C) // 8,), NAN, dtype=torch.float64, device=DEV)


def run_fwd(case, res, relu, use_mask, training=1):
    lib = L.load()
    M, C = case["M"], case["C"]
    y, stats = nanf(M, C), nanf(2 * C)
    rm, rv = case["rm"].clone(), case["rv"].clone()
    mask = torch.full((M * C // 4,), 0xAA, dtype=torch.uint8, device=DEV) if (relu and use_mask) else None
    scratch = scratch_of(C)
    L.check(lib.dmc_bn_act_fwd(L.ptr(case["x"]), L.ptr(case["res"]) if res else None, L.ptr(case["gamma"]), L.ptr(case["beta"]), L.ptr(rm),
                               L.ptr(rv), L.ptr(y), L.ptr(stats), L.ptr(scratch), L.ptr(mask), M, C, relu, training, EPS, MOM, None),
            "dmc_bn_act_fwd")
    return dict(mean=stats[:C], invstd=stats[C:], rm=rm, rv=rv, y=y, mask=mask)


def run_bwd(case, f, res, relu, entry="dmc_bn_act_bwd", want_dx=True, want_dxs=False, given=None):
    """dmc_bn_act_bwd / dmc_bn_act_bwd_x3s / dmc_bn_act_bwd_x3s_apply on the forward's statistics and mask."""
    lib = L.load()
    M, C = case["M"], case["C"]
    stats = torch.cat([f["mean"], f["invstd"]]).contiguous()
    mask = f.get("mask")
    rr = case["res"] if (res and relu and mask is None) else None            # re-read only to recompute the sign
    dx = nanf(M, C) if want_dx else None
    dres = nanf(M, C) if (res and relu) else None
    dxs = torch.full((lib.dmc_x3s_slices_bytes(M, C),), 0xFF, dtype=torch.uint8, device=DEV) if want_dxs else None
    if given is None:
        dg, db = nanf(C), nanf(C)
    else:
        dg, db = given[0].clone(), given[1].clone()
    a = (L.ptr(case["x"]), L.ptr(rr), L.ptr(case["gamma"]), L.ptr(case["beta"]), L.ptr(stats))
    scratch = scratch_of(C)
    if entry == "dmc_bn_act_bwd":
        L.check(lib.dmc_bn_act_bwd(*a, L.ptr(scratch), L.ptr(case["dy"]), L.ptr(dx), L.ptr(dres), L.ptr(dg), L.ptr(db), L.ptr(mask),
                                   M, C, relu, None), entry)
    elif entry == "dmc_bn_act_bwd_x3s":
        L.check(lib.dmc_bn_act_bwd_x3s(*a, L.ptr(scratch), L.ptr(case["dy"]), L.ptr(dx), L.ptr(dxs), L.ptr(dres), L.ptr(dg), L.ptr(db),
                                       L.ptr(mask), M, C, relu, None), entry)
    else:
        L.check(lib.dmc_bn_act_bwd_x3s_apply(*a, L.ptr(case["dy"]), L.ptr(dx), L.ptr(dxs), L.ptr(dres), L.ptr(dg), L.ptr(db), L.ptr(mask),
                                             M, C, relu, None), entry)
    out = dict(dx=dx, dgamma=dg, dbeta=db, dres=dres, dxs=dxs)
    if want_dxs:
        merged = nanf(M, C)
        L.check(lib.dmc_x3s_merge(L.ptr(dxs), L.ptr(merged), M, C, None), "dmc_x3s_merge")
        out["dx_merged"] = merged
    return out


def exactness_of_the_constant_channel(case, f, res, relu):
    """Exact sums: mean = c, var' = 0, invstd = fl(eps^-1/2), y = relu?(beta) exactly."""
    if case["M"] == 1 or case["C"] < 2:
        return
    assert float(f["mean"][1]) == R.CONST_VALUE
    assert float(f["invstd"][1]) == float(np.float32(1.0 / np.sqrt(np.float64(np.float32(EPS)))))
    if not res:
        b = float(case["beta"][1])
        assert bool((f["y"][:, 1] == (max(b, 0.0) if relu else b)).all())


# ------------------------------------------------------------------------------------------ dmc_bn_act_fwd / dmc_bn_act_bwd
@pytest.mark.parametrize("res,relu,use_mask", COMBOS)
@pytest.mark.parametrize("shape", R.BN_SHAPES, ids=str)
def test_bn_act_training_vs_fp64(shape, res, relu, use_mask):
    case = case_of(shape)
    f = twice(lambda: run_fwd(case, res, relu, use_mask))
    b = twice(lambda: run_bwd(case, f, res, relu))
    exactness_of_the_constant_channel(case, f, res, relu)
    got = dict(f, **{k: b[k] for k in ("dx", "dgamma", "dbeta", "dres")})
    report("bn_act %s res=%d relu=%d mask=%d" % (shape, res, relu, use_mask),
           R.unit_ratios(case, got, res, relu, R.chain_of(case["x"], case["M"], case["C"]), eps=EPS, momentum=MOM))


@pytest.mark.parametrize("shape", R.BN_SHAPES, ids=str)
def test_bn_act_eval_vs_fp64(shape):
    """Eval mode: the mean is the running mean bit for bit, invstd = rsqrtf(running_var + eps) within its own bound, the running
    statistics are left alone; y from the stored statistics."""
    case = case_of(shape)
    f = twice(lambda: run_fwd(case, 1, 1, 1, training=0))
    report("bn_act eval %s" % (shape,), R.unit_ratios(case, f, 1, 1, eps=EPS, momentum=MOM, training=False))


@pytest.mark.parametrize("shape", [(2, 16, 5, 7), (4, 64, 56, 56)], ids=str)
def test_bn_act_dyadic_data_has_exact_sums(shape):
    """Data on a grid: where bn2d_ref.exact_sums proves every fp32 partial sum exact, the statistics get the chain-free bound
    (one fp32 rounding of the stored value)."""
    case = case_of(shape, "dyadic")
    n = R.chain_of(case["x"], case["M"], case["C"])
    assert int((n == 0).sum()) >= case["C"] // 4
    f = twice(lambda: run_fwd(case, 0, 1, 0))
    report("bn_act dyadic %s" % (shape,), R.unit_ratios(case, f, 0, 1, n, eps=EPS, momentum=MOM))


# ------------------------------------------------------------------------------------------ statistics from fp64 partials, the apply kernels
def run_conv_stats(case, nblk):
    lib = L.load()
    M, C = case["M"], case["C"]
    part = R.make_partials64(case["x"], nblk)
    stats = nanf(2 * C)
    rm, rv = case["rm"].clone(), case["rv"].clone()
    L.check(lib.dmc_conv_nhwc_stats_final(L.ptr(part), nblk, C, M, L.ptr(stats), L.ptr(rm), L.ptr(rv), EPS, MOM, None), "dmc_conv_nhwc_stats_final")
    return dict(mean=stats[:C], invstd=stats[C:], rm=rm, rv=rv, stats=stats)


def run_apply(case, stats, res, relu, entry, shape=None):
    lib = L.load()
    M, C = case["M"], case["C"]
    y = nanf(M, C)
    mask = torch.full((M * C // 4,), 0xAA, dtype=torch.uint8, device=DEV) if relu else None
    a = (L.ptr(case["x"]), L.ptr(case["res"]) if res else None, L.ptr(case["gamma"]), L.ptr(case["beta"]), L.ptr(stats))
    out = dict(y=y, mask=mask)
    if entry == "nhwc":
        L.check(lib.dmc_bn_apply_act_nhwc(*a, L.ptr(y), L.ptr(mask), M, C, relu, None), entry)
        return out
    ys = torch.full((lib.dmc_x3s_slices_bytes(M, C),), 0xFF, dtype=torch.uint8, device=DEV)
    merged = nanf(M, C)
    if entry == "x3s":
        L.check(lib.dmc_bn_apply_act_x3s(*a, L.ptr(y), L.ptr(ys), L.ptr(mask), M, C, relu, None), entry)
        L.check(lib.dmc_x3s_merge(L.ptr(ys), L.ptr(merged), M, C, None), "dmc_x3s_merge")
    else:
        n, c, h, w = shape
        L.check(lib.dmc_bn_apply_act_x3q(*a, L.ptr(y), L.ptr(ys), L.ptr(mask), n, h, w, c, relu, None), entry)
        L.check(lib.dmc_x3q_merge(L.ptr(ys), L.ptr(merged), n, h, w, c, None), "dmc_x3q_merge")
    out["merged"] = merged
    return out


@pytest.mark.parametrize("nblk", [1, 255, 256, 257, 12000])
@pytest.mark.parametrize("shape", [(5, 512, 7, 7), (4, 64, 56, 56)], ids=str)
def test_conv_stats_final_and_the_apply_kernels_vs_fp64(shape, nblk):
    """dmc_conv_nhwc_stats_final on fp64 partials the test makes (n = 0: the stored values' own rounding is all there is), then
    dmc_bn_apply_act_nhwc / _x3s / _x3q on those statistics; the merged slices equal the fp32 result bit for bit."""
    case = case_of(shape)
    nblk = min(nblk, case["M"]) if nblk == 12000 else nblk
    st = twice(lambda: run_conv_stats(case, nblk))
    res = R.unit_ratios(case, st, 0, 0, 0, eps=EPS, momentum=MOM)
    entries = ("nhwc", "x3s", "x3q") if shape[2] % 2 == 0 and shape[3] % 2 == 0 else ("nhwc", "x3s")      # (space-to-depth: even maps)
    for r_, relu in ((1, 1), (0, 1), (1, 0)):
        outs = {e: twice(lambda: run_apply(case, st["stats"], r_, relu, e, shape)) for e in entries}
        for e in entries[1:]:
            assert R.same_bits(outs[e]["y"], outs["nhwc"]["y"]), e
            assert outs[e]["mask"] is None or torch.equal(outs[e]["mask"], outs["nhwc"]["mask"]), e
            assert torch.equal(outs[e]["merged"], outs["nhwc"]["y"]), e + ": merged slices"
        got = dict(st, **outs["nhwc"])
        for k, v in R.unit_ratios(case, got, r_, relu, None, eps=EPS, momentum=MOM).items():
            res["%s_r%dq%d" % (k, r_, relu)] = v
    report("conv_stats_final + apply %s nblk=%d" % (shape, nblk), res)


@pytest.mark.parametrize("shape", [(3, 64, 210, 210), (6, 64, 210, 210)], ids=str)
def test_apply_kernels_where_the_streams_wrap(shape):
    """The second grid-stride pass of the 4- and the 8-channel apply kernels, slices and space-to-depth slices included."""
    case = case_of(shape)
    st = run_conv_stats(case, 257)
    outs = {e: twice(lambda: run_apply(case, st["stats"], 1, 1, e, shape)) for e in ("nhwc", "x3s", "x3q")}
    for e in ("x3s", "x3q"):
        assert R.same_bits(outs[e]["y"], outs["nhwc"]["y"]) and torch.equal(outs[e]["mask"], outs["nhwc"]["mask"]), e
        assert torch.equal(outs[e]["merged"], outs["nhwc"]["y"]), e + ": merged slices"
    res = R.unit_ratios(case, dict(st, **outs["nhwc"]), 1, 1, 0, eps=EPS, momentum=MOM)
    report("apply, wrapped %s" % (shape,), res)


# ------------------------------------------------------------------------------------------ the hot-path backward: slices only
@pytest.mark.parametrize("res,relu,use_mask", [(0, 1, 0), (1, 1, 1), (1, 0, 0)])
@pytest.mark.parametrize("shape", SLICE_SHAPES, ids=str)
def test_bn_act_bwd_slices_only_vs_fp64(shape, res, relu, use_mask):
    """dmc_bn_act_bwd_x3s with dx = NULL, as _ConvBnAct.backward calls it: the gradient leaves as slices only, and their merge is
    held to the bound of dx.  Then dmc_bn_act_bwd_x3s_apply with that call's dgamma / dbeta as inputs."""
    case = case_of(shape)
    f = run_fwd(case, res, relu, use_mask)
    b = twice(lambda: run_bwd(case, f, res, relu, "dmc_bn_act_bwd_x3s", want_dx=False, want_dxs=True))
    got = dict(mean=f["mean"], invstd=f["invstd"], y=f["y"], mask=f["mask"], dx=b["dx_merged"], dgamma=b["dgamma"], dbeta=b["dbeta"], dres=b["dres"])
    out = R.unit_ratios(case, got, res, relu, None, eps=EPS, momentum=MOM)
    given = (b["dgamma"], b["dbeta"])
    a = twice(lambda: run_bwd(case, f, res, relu, "dmc_bn_act_bwd_x3s_apply", want_dx=True, want_dxs=True, given=given))
    assert R.same_bits(a["dgamma"], b["dgamma"]) and R.same_bits(a["dbeta"], b["dbeta"])              # inputs: left alone
    assert torch.equal(a["dx"], a["dx_merged"]) and torch.equal(a["dx"], b["dx_merged"])
    got2 = dict(got, dx=a["dx"], dres=a["dres"])
    for k, v in R.unit_ratios(case, got2, res, relu, None, eps=EPS, momentum=MOM, given=given).items():
        if k in ("dx", "dres", "dx_arith"):
            out["apply_" + k] = v
    out.pop("apply_dx_arith", None)
    report("bwd slices %s res=%d relu=%d mask=%d" % (shape, res, relu, use_mask), out)


# ------------------------------------------------------------------------------------------ the keep / LeakyReLU tail
def run_bwd_act(case, f, keep, slope, with_bn):
    lib = L.load()
    M, C = case["M"], case["C"]
    stats = torch.cat([f["mean"], f["invstd"]]).contiguous()
    dx, dg, db, scratch = nanf(M, C), nanf(C), nanf(C), scratch_of(C)
    if with_bn:
        L.check(lib.dmc_bn_bwd_act_nhwc(L.ptr(case["x"]), L.ptr(case["gamma"]), L.ptr(case["beta"]), L.ptr(stats), L.ptr(scratch),
                                        L.ptr(case["dy"]), L.ptr(dx), L.ptr(dg), L.ptr(db), L.ptr(keep), case["hw"], slope, M, C, None), "dmc_bn_bwd_act_nhwc")
        return dict(dx=dx, dgamma=dg, dbeta=db)
    L.check(lib.dmc_bn_bwd_act_nhwc(L.ptr(case["x"]), None, None, None, None, L.ptr(case["dy"]), L.ptr(dx), None, None, L.ptr(keep), case["hw"],
                                    slope, M, C, None), "dmc_bn_bwd_act_nhwc")
    return dict(dx=dx)


@pytest.mark.parametrize("shape", [(2, 16, 5, 7), (5, 512, 7, 7), (3, 256, 37, 61), (3, 64, 210, 210)], ids=str)
def test_bn_bwd_act_keep_and_slope_vs_fp64(shape):
    """dmc_bn_bwd_act_nhwc: keep[n][c] with zeros and non-unit values, slope 0.2, frames of hw = 35 / 49 / 2257 / 44100 pixels (a frame
    boundary falls inside a workgroup's run of float4 columns), with gamma and with gamma == NULL (act_mask_bwd_kernel)."""
    case = case_of(shape)
    n = shape[0]
    keep = torch.from_numpy(np.random.RandomState(5).choice([0.0, 1.0, 2.0, 0.5], (n, shape[1])).astype(np.float32)).to(DEV)
    f = run_fwd(case, 0, 0, 0)
    res = {}
    for kp in (keep, None):
        b = twice(lambda: run_bwd_act(case, f, kp, 0.2, True))
        got = dict(mean=f["mean"], invstd=f["invstd"], **b)
        for k, v in R.unit_ratios(case, got, 0, 0, None, keep=kp, slope=0.2, eps=EPS, momentum=MOM).items():
            res[k + ("" if kp is not None else "_nokeep")] = v
        a = twice(lambda: run_bwd_act(case, f, kp, 0.2, False))
        ref, bd = R.act_mask_ref(case["x"], case["dy"], kp, case["hw"], 0.2)
        res["act_only" + ("" if kp is not None else "_nokeep")] = R.ratio(a["dx"], ref, bd)
    res.pop("dx_arith_nokeep", None)
    report("bn_bwd_act %s" % (shape,), res)


@pytest.mark.parametrize("shape", R.BN_SHAPES, ids=str)
def test_channel_sum_vs_fp64(shape):
    lib = L.load()
    case = case_of(shape)
    M, C = case["M"], case["C"]

    def run():
        out, scratch = nanf(C), scratch_of(C)
        L.check(lib.dmc_channel_sum_nhwc(L.ptr(case["x"]), L.ptr(scratch), L.ptr(out), M, C, None), "dmc_channel_sum_nhwc")
        return dict(out=out)
    st = R.Stats(case["x"], EPS, R.chain_of(case["x"], M, C))
    b = R.Bound(R.U32 * st.s1.abs(), st.b_s1.arith)
    report("channel_sum %s" % (shape,), dict(channel_sum=R.ratio(twice(run)["out"], st.s1, b)))


# ------------------------------------------------------------------------------------------ the stem tail
def pool_case(shape):
    case = case_of(shape, "dyadic")
    if "dpool" not in case:
        n, c, h, w = shape
        ph, pw = R.pool_dims(h, w)
        case["x4"] = case["x"].view(n, h, w, c)
        case["dpool"] = torch.from_numpy(np.random.RandomState(7).standard_normal((n, ph, pw, c)).astype(np.float32)).to(DEV)
    return case


def run_pool_fwd(case, shape, entry, codes=True, stat_split=0):
    lib = L.load()
    n, c, h, w = shape
    ph, pw = R.pool_dims(h, w)
    y, stats = nanf(n, ph, pw, c), nanf(2 * c)
    rm, rv = case["rm"].clone(), case["rv"].clone()
    scratch = scratch_of(c) if stat_split == 0 else R.make_partials64(case["x"], stat_split, layout="bn")
    a = (L.ptr(case["x"]), L.ptr(case["gamma"]), L.ptr(case["beta"]), L.ptr(rm), L.ptr(rv), L.ptr(y))
    out = dict(mean=stats[:c], invstd=stats[c:], rm=rm, rv=rv, ypool=y)
    if entry == "fwd":
        L.check(lib.dmc_bn_relu_pool_fwd(*a, L.ptr(stats), L.ptr(scratch), n, h, w, c, 1, EPS, MOM, None), "dmc_bn_relu_pool_fwd")
        return out
    cd = torch.full((n, ph, pw, c), 0xFF, dtype=torch.uint8, device=DEV) if codes else None
    xm = nanf(n, ph, pw, c) if codes else None
    ys = torch.full((lib.dmc_x3s_slices_bytes(n * ph * pw, c),), 0xFF, dtype=torch.uint8, device=DEV)
    L.check(lib.dmc_bn_relu_pool_fwd_arg(*a, L.ptr(ys), L.ptr(cd), L.ptr(xm), L.ptr(stats), L.ptr(scratch), stat_split, n, h, w, c, 1, EPS, MOM, None),
            "dmc_bn_relu_pool_fwd_arg")
    merged = nanf(n, ph, pw, c)
    L.check(lib.dmc_x3s_merge(L.ptr(ys), L.ptr(merged), n * ph * pw, c, None), "dmc_x3s_merge")
    out.update(code=cd, xmax=xm, merged=merged)
    return out


def run_pool_bwd(case, shape, f, entry):
    lib = L.load()
    n, c, h, w = shape
    stats = torch.cat([f["mean"], f["invstd"]]).contiguous()
    dx, dg, db, scratch = nanf(n, h, w, c), nanf(c), nanf(c), scratch_of(c)
    a = (L.ptr(case["x"]), L.ptr(case["gamma"]), L.ptr(case["beta"]), L.ptr(stats), L.ptr(scratch), L.ptr(case["dpool"]))
    if entry == "bwd_arg":
        L.check(lib.dmc_bn_relu_pool_bwd_arg(*a, L.ptr(f["code"]), L.ptr(f["xmax"]), L.ptr(dx), L.ptr(dg), L.ptr(db), n, h, w, c, None), entry)
        return dict(dx=dx, dgamma=dg, dbeta=db)
    cd = torch.full_like(f["code"], 0xFF) if entry == "bwd_codes" else None
    L.check(lib.dmc_bn_relu_pool_bwd(*a, L.ptr(dx), L.ptr(dg), L.ptr(db), L.ptr(cd), n, h, w, c, None), entry)
    return dict(dx=dx, dgamma=dg, dbeta=db, code=cd)


@pytest.mark.parametrize("shape", R.POOL_SHAPES, ids=str)
def test_bn_relu_pool_vs_fp64(shape):
    """The four pool entry points on dyadic inputs (exact ties inside windows): statistics, the pooled map, codes and xmax exact on
    every decided window (undecided share <= 1e-4; the reference alone leaves none, test_bn2d_ref_cpu.py), dx routed through the
    kernel's codes, dgamma / dbeta with the chain of the pass that made them."""
    n, c, h, w = shape
    ph, pw = R.pool_dims(h, w)
    case = pool_case(shape)
    n_stats = R.chain_of(case["x"], case["M"], c)
    plain = twice(lambda: run_pool_fwd(case, shape, "fwd"))
    res = {k: v for k, v in R.unit_ratios(case, plain, 0, 1, n_stats, eps=EPS, momentum=MOM).items()}
    ref = R.pool_ref(case["x4"], plain["mean"], plain["invstd"], case["gamma"], case["beta"])
    dec = ref["decided"]
    res["undecided"] = ref["undecided"]
    assert ref["undecided"] <= 1e-4
    b_y = R.Bound(ref["b_y"].fmt[dec], ref["b_y"].arith[dec])
    res["ypool"] = R.ratio(plain["ypool"][dec], ref["y"][dec], b_y)
    if c % 16 != 0:
        return report("pool %s" % (shape,), res)
    arg = twice(lambda: run_pool_fwd(case, shape, "fwd_arg"))
    noc = twice(lambda: run_pool_fwd(case, shape, "fwd_arg", codes=False))
    for k in ("mean", "invstd", "rm", "rv", "ypool"):
        assert R.same_bits(arg[k], plain[k]) and R.same_bits(noc[k], plain[k]), k
    assert torch.equal(arg["merged"], plain["ypool"]) and torch.equal(noc["merged"], plain["ypool"])
    res["code"] = R.flag(torch.equal(arg["code"][dec], ref["code"][dec]))
    res["xmax"] = R.flag(R.same_bits(arg["xmax"][dec], ref["xmax"][dec]))
    assert int(arg["code"].max()) <= 8
    # backward, three ways
    for entry, n_b, ex in (("bwd_arg", R.geometry(n * ph * pw, c)["iters"], 0), ("bwd", R.pool_tile_chain(n, h, w, c), 3),
                           ("bwd_codes", R.pool_tile_chain(n, h, w, c), 3)):
        b = twice(lambda: run_pool_bwd(case, shape, arg, entry))
        if entry == "bwd_codes":
            assert torch.equal(b["code"], arg["code"])                                   # the tile pass' own record = the forward's
        back = R.pool_backward_ref(case["x4"], case["dpool"], arg["code"], plain["mean"], plain["invstd"], case["gamma"], case["beta"], n_b, ex)
        assert back["undecided_relu"] == 0
        for k in ("dx", "dgamma", "dbeta"):
            res["%s_%s" % (entry, k)] = R.ratio(b[k].reshape(back[k][0].shape), back[k][0], back[k][1])
    report("pool %s" % (shape,), res)


@pytest.mark.parametrize("stat_split", [1, 31, 32, 33, 1024])
def test_bn_relu_pool_statistics_from_given_partials(stat_split):
    """stat_split > 0: the producer left that many fp64 partial pairs per channel in [C][1024][2] layout (the rest of the scratch is
    NaN here): reduce_partials' 32-lane tail at every count."""
    shape = (2, 64, 30, 31)
    case = pool_case(shape)
    f = twice(lambda: run_pool_fwd(case, shape, "fwd_arg", stat_split=stat_split))
    res = R.unit_ratios(case, f, 0, 1, 0, eps=EPS, momentum=MOM)
    ref = R.pool_ref(case["x4"], f["mean"], f["invstd"], case["gamma"], case["beta"])
    res["code"] = R.flag(torch.equal(f["code"][ref["decided"]], ref["code"][ref["decided"]]))
    report("pool stat_split=%d" % stat_split, res)


# ------------------------------------------------------------------------------------------ the unit as the model runs it
@pytest.mark.parametrize("res,relu", [(0, 0), (0, 1), (1, 0), (1, 1)])
@pytest.mark.parametrize("shape", [(5, 512, 7, 7), (4, 64, 56, 56)], ids=str)
def test_conv_bn_act_chain_vs_fp64(shape, res, relu, monkeypatch):
    """ops.conv_bn_act with ops.X3S on, forward and backward: the BatchNorm stages are referenced from the convolution output the
    op saved (statistics from the convolution epilogue's fp64 partials: n = 0), dgamma / dbeta / the residual's gradient from the
    kernel's own mask; the BatchNorm's dx leaves as slices into the data gradient and is held by the slices-only test above."""
    monkeypatch.setattr(ops, "X3S", True)
    n, c, h, w = shape
    base = case_of(shape)
    g = torch.Generator(device="cpu").manual_seed(77)
    conv = torch.nn.Conv2d(c, c, 3, 1, 1, bias=False)
    with torch.no_grad():
        conv.weight.copy_(torch.randn(conv.weight.shape, generator=g) * (2.0 / (9 * c)) ** 0.5)
    conv = conv.to(DEV)
    bn = torch.nn.BatchNorm2d(c, eps=EPS, momentum=MOM).to(DEV).train()
    with torch.no_grad():
        bn.weight.copy_(base["gamma"]); bn.bias.copy_(base["beta"].clamp(-1, 1))
        bn.running_mean.copy_(base["rm"]); bn.running_var.copy_(base["rv"])
    cl = lambda t: t.view(n, h, w, c).permute(0, 3, 1, 2)                                # [M][C] memory as a channels_last NCHW tensor
    x = cl(torch.randn((n * h * w, c), generator=g).to(DEV)).requires_grad_(True)
    r = cl(base["res"].clone()).requires_grad_(True) if res else None
    assert ops.x3s_usable(n, h, w, conv)
    out = ops.conv_bn_act(x, conv, bn, r, bool(relu))
    _, _, y, gamma, beta, stats, mask = out.grad_fn.saved_tensors
    out.backward(cl(base["dy"]))
    torch.cuda.synchronize()
    M = n * h * w
    flat = lambda t: t.permute(0, 2, 3, 1).reshape(M, c)
    case = dict(base, x=flat(y).contiguous(), beta=beta.detach())
    got = dict(mean=stats[:c], invstd=stats[c:2 * c], rm=bn.running_mean, rv=bn.running_var, y=flat(out.detach()).contiguous(), mask=mask,
               dgamma=bn.weight.grad, dbeta=bn.bias.grad, dres=flat(r.grad).contiguous() if (res and relu) else None)
    if res and not relu:
        assert torch.equal(flat(r.grad), base["dy"])
    report("conv_bn_act chain %s res=%d relu=%d" % (shape, res, relu), R.unit_ratios(case, got, res, relu, 0, eps=EPS, momentum=MOM))
