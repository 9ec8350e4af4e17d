"""The I3D trunk's conv -> BatchNorm3d -> ReLU unit held to fp64 stage by stage, on the path the trunk really takes
(csrc/unit3d.hip: dmc_unit3d_bf16_fwd_into / dmc_unit3d_bf16_bwd -- both weight layouts packed by one launch, forward and
data gradient on the packed workspace, BatchNorm sums from the convolution's epilogue, one workspace per direction).

Three layers of tests, each through the C ABI:
  * the statistics rows the convolution writes, for every tile configuration: all rows written, nothing behind them, and their
    fp64 sum against the sums of the y the same call wrote;
  * the BatchNorm kernels alone (csrc/bn3d_bf16.hip) at the shapes where their launch geometry changes;
  * the fused unit as a chain: every stage against an fp64 evaluation of that stage on the PREVIOUS stage's actual bf16 output,
    so a defect shows in the stage that has it.

Every BatchNorm tolerance is a bound derived in tests/bn3d_ref.py from the kernels' arithmetic (a function of fp64 quantities,
checked against an emulation and against seeded defects in test_bn3d_ref_cpu.py); convolution outputs use the project's
bf16_close and the weight gradient its 2e-5 fp32-accumulation bar.  The ReLU mask of every backward reference is read from the
kernel's own `out`, as it is, while the kernel recomputes it from y: a disagreement between the two fails the dy check.
Each test prints error / bound per stage (headroom, not a target); out_arith / dy_arith are the share of the accumulated part
of the bound that is used once the bf16 rounding itself is taken off (bn3d_ref.excess)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import dmcnet_amd
from tests import bn3d_ref as R
from tests.test_conv3d_gpu import CASES, bf16_close, rnd

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
L = dmcnet_amd._lib
EPS, MOM = 1e-5, 0.1                                       # nn.BatchNorm3d's defaults, as Unit3Dpy builds it
NAN = float("nan")
WORST = {}


@pytest.fixture
def conv_cfg(request):
    lib = L.load()
    before = lib.dmc_get_option(b"conv_cfg")
    try:
        L.check(lib.dmc_set_option(b"conv_cfg", int(request.param)), "dmc_set_option")
        yield int(request.param)
    finally:
        L.check(lib.dmc_set_option(b"conv_cfg", before), "dmc_set_option")


def report(what, res):
    for k, v in res.items():
        WORST[k] = max(WORST.get(k, 0.0), v)
    print("  %s  error / bound: %s" % (what, "  ".join("%s %.3f" % kv for kv in res.items())))
    print("  worst so far: %s" % "  ".join("%s %.3f" % kv for kv in sorted(WORST.items())))
    assert all(v <= 1.0 for v in res.values()), (what, res)


def ndhwc(t):
    """[N][C][D][H][W] -> [N D H W][C]"""
    return t.permute(0, 2, 3, 4, 1).reshape(-1, t.shape[1])


def pattern(rows, cols):
    """bf16 [rows][cols] of small distinct integers: what a kernel must leave alone outside its channel slice"""
    return ((torch.arange(rows * cols, device=DEV) % 251) - 125).to(torch.bfloat16).view(rows, cols)


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and bool((a.contiguous().view(torch.uint8) == b.contiguous().view(torch.uint8)).all())


def conv_ref(x, wt, k):
    """fp64 convolution on the CPU of the bf16-rounded operands, as leaves: (x [N,C,D,H,W], w, y)"""
    xo = x.double().cpu().requires_grad_(True)
    wo = wt.bfloat16().double().cpu().requires_grad_(True)
    return xo, wo, F.conv3d(xo, wo, None, 1, k // 2)


# ------------------------------------------------------------------------------------------ 2. statistics rows
def check_conv_stat_rows(n, cin, d, h, w, cout, k, expect_nblk=None):
    lib = L.load()
    M, T = n * d * h * w, k ** 3
    x = rnd(401, (n, cin, d, h, w)).bfloat16()
    wt = rnd(402, (cout, cin, k, k, k)) * (2.0 / (cin * T)) ** 0.5
    xg, wg = ndhwc(x.to(DEV)).contiguous(), wt.to(DEV).contiguous()
    nblk = lib.dmc_conv3d_bf16_stat_blocks_k(n, d, h, w, cin, cout, k, k, k)      # (after the option is set)
    if expect_nblk is not None:
        assert nblk == expect_nblk, (nblk, expect_nblk)
    assert 0 < nblk < 10 ** 6
    rows = nblk * cout * 2
    buf = torch.full((2 * rows,), NAN, dtype=torch.float32, device=DEV)           # the rows and a tail of the same size
    y = torch.full((M, cout), NAN, dtype=torch.bfloat16, device=DEV)
    wpack = torch.empty(lib.dmc_conv3d_bf16_wpack_bytes(cin, cout, k, k, k), dtype=torch.uint8, device=DEV)
    L.check(lib.dmc_conv3d_bf16_fwd(L.ptr(xg), L.ptr(wg), cin * T, T, 1, L.ptr(wpack), L.ptr(y), L.ptr(buf), n, d, h, w, cin, cout,
                                    k, k, k, None), "dmc_conv3d_bf16_fwd")
    torch.cuda.synchronize()
    assert bool(torch.isfinite(buf[:rows]).all()), "%d floats of the statistics rows not written" % int((~torch.isfinite(buf[:rows])).sum())
    assert bool(torch.isnan(buf[rows:]).all()), "%d floats written behind the statistics rows" % int((~torch.isnan(buf[rows:])).sum())
    if k == 1:
        yo = x.double().permute(0, 2, 3, 4, 1).reshape(M, cin) @ wt.bfloat16().double().view(cout, cin).t()
    else:
        yo = ndhwc(conv_ref(x, wt, k)[2].detach())
    bf16_close(y, yo, "forward")
    st = R.Stats(y, EPS, R.CONV_STAT_CHAIN)
    got = buf[:rows].view(nblk, cout, 2).double().sum(0)
    report("conv rows %s nblk=%d" % ((n, cin, d, h, w, cout, k), nblk),
           dict(conv_sum=R.ratio(got[:, 0], st.s1, st.b_s1), conv_sumsq=R.ratio(got[:, 1], st.s2, st.b_s2)))


@pytest.mark.parametrize("conv_cfg", [0, 1, 2, 3, 4, 5, 6, 7, 8], indirect=True)
@pytest.mark.parametrize("shape", [(2, 48, 3, 11, 9, 160), (1, 24, 2, 5, 6, 40)])
def test_conv_statistics_rows_3x3x3_every_tile(shape, conv_cfg):
    """conv_cfg 1 .. 5: the tap-stepping tiles (128x128, 128x64 and 256x128 reduce across waves through LDS), 6: their automatic
    choice, 0 / 7 / 8: the patch-resident kernel, whose waves share a job's rows in three ways."""
    check_conv_stat_rows(*shape, 3)


def test_conv_statistics_rows_3x3x3_narrow_map_falls_back():
    """W + 2 < 6: the patch-resident kernel does not serve the map; the row count follows the tap-stepping choice."""
    check_conv_stat_rows(2, 144, 2, 3, 3, 288, 3)


@pytest.mark.parametrize("conv_cfg", [0, 1, 2, 3, 4, 5, 6], indirect=True)
@pytest.mark.parametrize("shape", [(1, 208, 5, 4, 3, 48), (2, 40, 3, 7, 9, 136)])
def test_conv_statistics_rows_1x1x1_every_tile(shape, conv_cfg):
    check_conv_stat_rows(*shape, 1)


@pytest.mark.parametrize("cout,dhw,nblk", [(64, (5, 116, 113), 513),      # 128 x 64
                                            (208, (3, 104, 105), 256),     # 128 x 128
                                            (256, (5, 116, 113), 257)])    # 256 x 128
def test_conv_statistics_rows_automatic_tile_choice(cout, dhw, nblk):
    """The smallest pixel counts at which the automatic choice takes each large tile, with a ragged last one; the expected row count
    pins the choice and the rows together."""
    check_conv_stat_rows(1, 16, *dhw, cout, 1, expect_nblk=nblk)


# ------------------------------------------------------------------------------------------ 3. BatchNorm alone
def run_bn(case, relu, wide, running):
    lib = L.load()
    y, gamma, beta, part = case["y"], case["gamma"], case["beta"], case["part"]
    M, C = y.shape
    ld, off = (C + 40, 16) if wide else (C, 0)
    out_buf, dout_buf = pattern(M, ld), pattern(M, ld)
    dout_buf[:, off:off + C] = case["dout"]
    dout_before = dout_buf.clone()
    out, dout = out_buf[:, off:off + C], dout_buf[:, off:off + C]
    stats = torch.full((2 * C,), NAN, dtype=torch.float32, device=DEV)
    rm, rv = (case["rm"].clone(), case["rv"].clone()) if running else (None, None)
    L.check(lib.dmc_bn3d_bf16_fwd_ld(L.ptr(y), L.ptr(part), part.shape[0], L.ptr(gamma), L.ptr(beta), L.ptr(stats), L.ptr(rm), L.ptr(rv),
                                     L.ptr(out), ld, M, C, relu, EPS, MOM, None), "dmc_bn3d_bf16_fwd_ld")
    scratch = torch.empty(lib.dmc_bn3d_bf16_scratch_bytes(C), dtype=torch.uint8, device=DEV)
    dy = torch.full((M, C), NAN, dtype=torch.bfloat16, device=DEV)
    dgamma, dbeta = torch.full((C,), NAN, device=DEV), torch.full((C,), NAN, device=DEV)
    L.check(lib.dmc_bn3d_bf16_bwd(L.ptr(dout), ld, L.ptr(y), L.ptr(stats), L.ptr(gamma), L.ptr(beta), L.ptr(scratch), L.ptr(dy),
                                  L.ptr(dgamma), L.ptr(dbeta), M, C, relu, None), "dmc_bn3d_bf16_bwd")
    torch.cuda.synchronize()
    if wide:                                                # columns outside the slice: untouched, bit for bit
        fresh = pattern(M, ld)
        assert same_bits(out_buf[:, :off], fresh[:, :off]) and same_bits(out_buf[:, off + C:], fresh[:, off + C:])
    assert same_bits(dout_buf, dout_before)
    res = dict(stats=stats, out=out.contiguous(), dy=dy, dgamma=dgamma, dbeta=dbeta)
    if running:
        res.update(rm=rm, rv=rv)
    return res


def bn_ratios(got, y, dout, gamma, beta, rm0, rv0, relu, n_stats):
    """error / bound of every BatchNorm output against fp64 on the kernel's operands (the mask from the kernel's out)"""
    C = y.shape[1]
    st = R.Stats(y, EPS, n_stats)
    res = dict(mean=R.ratio(got["stats"][:C], st.mean, st.b_mean), invstd=R.ratio(got["stats"][C:], st.invstd, st.b_invstd))
    if "rm" in got:
        (rm, b_rm), (rv, b_rv) = st.running(rm0, rv0, MOM)
        res.update(running_mean=R.ratio(got["rm"], rm, b_rm), running_var=R.ratio(got["rv"], rv, b_rv))
    ref, b = R.forward_ref(y, st, gamma, beta, relu)
    res["out"], res["out_arith"] = R.ratio(got["out"], ref, b), R.excess(got["out"], ref, b)
    back = R.backward_ref(dout, y, got["out"], st, gamma, relu, R.bn3_bwd_chain(*y.shape))
    for k in ("dy", "dgamma", "dbeta"):
        res[k] = R.ratio(got[k], back[k][0], back[k][1])
    res["dy_arith"] = R.excess(got["dy"], *back["dy"])
    return res


_BN_CASES = {}


def bn_operands(M, C, spread):
    if (M, C) not in _BN_CASES:
        case = {k: v.to(DEV) for k, v in R.bn_case(M, C, 1000 + C, spread).items()}
        case["part"] = R.make_partials(case["y"])
        _BN_CASES[(M, C)] = case
    return _BN_CASES[(M, C)]


@pytest.mark.parametrize("relu", [0, 1])
@pytest.mark.parametrize("shape", R.BN_SHAPES)
def test_bn3d_kernels_alone_vs_fp64(shape, relu):
    """dmc_bn3d_bf16_fwd_ld / dmc_bn3d_bf16_bwd on partial rows the test makes (fp64 sums per 128 pixels, rounded to fp32): dense with
    running statistics, and as a channel slice (ld = C + 40, offset 16) without; a negative and a zero gamma, a constant channel;
    each call twice, bit for bit."""
    case = bn_operands(*shape)
    assert float(case["y"][:, 3].double().var(unbiased=False)) == 0.0
    for wide, running in ((False, True), (True, False)):
        got, again = run_bn(case, relu, wide, running), run_bn(case, relu, wide, running)
        for k in got:
            assert same_bits(got[k], again[k]), k
        report("bn M=%d C=%d relu=%d ld=%s running=%d" % (shape[0], shape[1], relu, "C+40" if wide else "C", running),
               bn_ratios(got, case["y"], case["dout"], case["gamma"], case["beta"], case["rm"], case["rv"], relu, R.TEST_PART_CHAIN))


# ------------------------------------------------------------------------------------------ 4. the fused unit as a chain
def up256(b):
    return (b + 255) // 256 * 256


def run_unit(case, idx, ops_):
    """One forward + backward of the fused unit on buffers the test owns; even idx: `out` is a channel slice, odd: `dout` is."""
    lib = L.load()
    n, cin, d, h, w, cout, k = case
    geom = (n, d, h, w, cin, cout, k, k, k)
    M = n * d * h * w
    relu = 0 if idx % 5 == 4 else 1
    ld_o, off_o = (cout + 40, 16) if idx % 2 == 0 else (cout, 0)
    ld_g, off_g = (cout + 40, 16) if idx % 2 == 1 else (cout, 0)
    out_buf, dout_buf = pattern(M, ld_o), pattern(M, ld_g)
    dout_buf[:, off_g:off_g + cout] = ops_["dout"]
    out, dout = out_buf[:, off_o:off_o + cout], dout_buf[:, off_g:off_g + cout]
    fws = torch.empty(lib.dmc_unit3d_bf16_fwd_workspace_bytes(*geom), dtype=torch.uint8, device=DEV)
    bws = torch.empty(lib.dmc_unit3d_bf16_bwd_workspace_bytes(*geom), dtype=torch.uint8, device=DEV)
    y = torch.full((M, cout), NAN, dtype=torch.bfloat16, device=DEV)
    dy, dx = torch.full_like(y, NAN), torch.full((M, cin), NAN, dtype=torch.bfloat16, device=DEV)
    dw = torch.full((cout, cin, k, k, k), NAN, device=DEV)
    dgamma, dbeta = torch.full((cout,), NAN, device=DEV), torch.full((cout,), NAN, device=DEV)
    rm, rv = ops_["rm"].clone(), ops_["rv"].clone()
    L.check(lib.dmc_unit3d_bf16_fwd_into(L.ptr(ops_["x"]), L.ptr(ops_["w"]), L.ptr(ops_["gamma"]), L.ptr(ops_["beta"]), L.ptr(rm), L.ptr(rv),
                                         L.ptr(fws), L.ptr(y), L.ptr(out), ld_o, *geom, relu, EPS, MOM, None), "dmc_unit3d_bf16_fwd_into")
    L.check(lib.dmc_unit3d_bf16_bwd(L.ptr(dout), ld_g, L.ptr(ops_["x"]), L.ptr(y), L.ptr(fws), L.ptr(ops_["gamma"]), L.ptr(ops_["beta"]),
                                    L.ptr(bws), L.ptr(dy), L.ptr(dx), L.ptr(dw), L.ptr(dgamma), L.ptr(dbeta), *geom, relu, None),
            "dmc_unit3d_bf16_bwd")
    torch.cuda.synchronize()
    fresh = pattern(M, ld_o)
    assert same_bits(out_buf[:, :off_o], fresh[:, :off_o]) and same_bits(out_buf[:, off_o + cout:], fresh[:, off_o + cout:])
    # (mean, invstd): the last region of the forward workspace (FwdLayout of csrc/unit3d.hip), kept there for the backward
    stats = fws[fws.numel() - up256(8 * cout):][:8 * cout].view(torch.float32).clone()
    return relu, dict(y=y, stats=stats, out=out.contiguous(), rm=rm, rv=rv, dy=dy, dgamma=dgamma, dbeta=dbeta, dx=dx, dw=dw)


def check_unit_chain(case, idx):
    n, cin, d, h, w, cout, k = case
    M = n * d * h * w
    x = rnd(411, (n, cin, d, h, w)).bfloat16()
    wt = rnd(412, (cout, cin, k, k, k)) * (2.0 / (cin * k ** 3)) ** 0.5
    r = np.random.RandomState(413)
    gamma = r.uniform(0.5, 1.5, cout)
    gamma[1] = -gamma[1]
    f = lambda a: torch.from_numpy(np.asarray(a, dtype=np.float32)).to(DEV)
    ops_ = dict(x=ndhwc(x.to(DEV)).contiguous(), w=wt.to(DEV).contiguous(), gamma=f(gamma), beta=f(r.uniform(-0.5, 0.5, cout)),
                rm=f(r.uniform(-1.0, 1.0, cout)), rv=f(r.uniform(0.5, 2.0, cout)), dout=rnd(414, (M, cout)).bfloat16().to(DEV))
    relu, got = run_unit(case, idx, ops_)
    _, again = run_unit(case, idx, ops_)
    for name in got:
        assert same_bits(got[name], again[name]), name
    # convolution: y against fp64 on bf16(x), bf16(w)
    xo, wo, yo = conv_ref(x, wt, k)
    bf16_close(got["y"], ndhwc(yo.detach()), "y")
    # BatchNorm forward and backward: fp64 on the kernel's y, dout and out
    res = bn_ratios(got, got["y"], ops_["dout"], ops_["gamma"], ops_["beta"], ops_["rm"], ops_["rv"], relu, R.CONV_STAT_CHAIN)
    # convolution gradients: fp64 from the kernel's dy
    yo.backward(got["dy"].double().cpu().view(n, d, h, w, cout).permute(0, 4, 1, 2, 3))
    bf16_close(got["dx"], ndhwc(xo.grad), "dx")
    res["dw_over_2e-5"] = float((got["dw"].double().cpu() - wo.grad).abs().max() / wo.grad.abs().max()) / 2e-5
    report("unit %s relu=%d %s" % (case, relu, "out slice" if idx % 2 == 0 else "dout slice"), res)


CHAIN_CASES = [c for c in CASES if c[0] * c[2] * c[3] * c[4] <= 4000]
assert (1, 96, 3, 14, 14, 208, 3) in CHAIN_CASES


@pytest.mark.parametrize("idx", range(len(CHAIN_CASES)), ids=["%d-%d-%d-%d-%d-%d-k%d" % c for c in CHAIN_CASES])
def test_unit3d_chain_vs_fp64(idx):
    check_unit_chain(CHAIN_CASES[idx], idx)


@pytest.mark.parametrize("conv_cfg", [1, 2, 3, 4, 5, 6, 7, 8], indirect=True)
def test_unit3d_chain_3x3x3_every_tile(conv_cfg):
    """(the option stays as it is between the forward and its backward, which recomputes the workspace layout)"""
    check_unit_chain((2, 48, 3, 11, 9, 160, 3), conv_cfg)


@pytest.mark.parametrize("conv_cfg", [1, 2, 3, 4, 5], indirect=True)
def test_unit3d_chain_1x1x1_every_tile(conv_cfg):
    check_unit_chain((2, 40, 3, 7, 9, 136, 1), conv_cfg)
