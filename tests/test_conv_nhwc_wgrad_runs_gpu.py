"""GPU: the row-walking weight-gradient kernels of conv_nhwc.hip (conv_wgrad3_kernel<1 / 2>, conv_wgrad2_kernel<3,1 / 3,2 / 1,1 /
1,2>) against fp64 where a workgroup makes a RUN of three to eight steps.

Every other unit test gives a workgroup one step, in a few cases two (tests/test_conv_nhwc_plans_cpu.py keeps the record), so the
double-buffered step loop -- set_step(step + 1, buf ^ 1), the interleaved issue_slot, the buffer parity from the third step on,
steps that move to the next image inside one workgroup, a last group shorter than the others -- ran only in the B = 40 end-to-end
steps.  The cases of tests/conv_nhwc_plans.py (WGRAD_RUN_SWEEP) are the smallest that give each kernel such runs: R = 1 and
R > 1, even and odd run lengths, last groups of 1 .. 7 steps.

  (a) weight gradient against fp64 autograd of F.conv2d at 1e-5 of max |ref|; a case that sums tens of thousands of pixels in
      fp32 might have needed max(4 e_ref, 1e-5) instead, e_ref = the error of the CPU's own fp32 F.conv2d weight gradient;
      none does (WORST_MEASURED: e_hip 1.8e-07 .. 7.9e-07, below e_ref everywhere), so every case is held to 1e-5;
  (b) integer operands (x and dy in [-4, 4]): every product and partial sum is an integer below 2^24, exact in fp32 and in
      bf16x3, so the result equals fp64 EXACTLY -- a dropped or doubled step fails whatever the tolerance;
  (c) every run twice, bit-identical; workspace and result start as NaN, so a partial that is read but never written shows;
  (d) a failure names (co, tap, ci) of the worst element;
  (e) the generic conv_wgrad_kernel with three slices and conv_wgrad_reduce_kernel behind it; forward and data gradient at
      M = 32768, where conv_nhwc_kernel<128, 64, 16, ..> runs; the forward at 48 output channels with statistics, whose row
      count the library once sized for another tile than it launched."""
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

#: (e_hip under conv_arith = 1, e_hip under conv_arith = 0 or None where the case does not run there, e_ref) as this file printed
#: them on an MI355X: max |dw - fp64| / max |fp64| of the kernel and of the CPU's fp32 evaluation; a record, not a bar
WORST_MEASURED = {
    (11, 512, 7, 7, 512, 3, 1): (2.669e-07, 3.152e-07, 8.707e-07),
    (25, 256, 14, 14, 256, 3, 1): (3.981e-07, 4.508e-07, 2.823e-06),
    (10, 64, 56, 56, 64, 3, 1): (2.752e-07, 2.655e-07, 9.067e-07),
    (21, 128, 28, 28, 128, 3, 1): (3.102e-07, 3.850e-07, 1.551e-06),
    (10, 64, 56, 56, 128, 3, 2): (1.927e-07, 1.980e-07, 1.065e-06),
    (9, 256, 14, 14, 512, 3, 2): (1.920e-07, 2.909e-07, 8.937e-07),
    (55, 64, 28, 28, 128, 3, 2): (1.827e-07, 1.961e-07, 2.018e-06),
    (20, 128, 28, 28, 256, 1, 2): (2.657e-07, None, 3.126e-07),
    (3, 256, 13, 10, 512, 1, 1): (1.949e-07, None, 3.366e-07),
    (20, 256, 14, 14, 512, 3, 2): (None, 3.192e-07, 1.349e-06),
    (3, 48, 28, 28, 80, 3, 1): (7.949e-07, 7.949e-07, 2.041e-06),       # the generic kernel: one arithmetic
}
# forward / data gradient of test_first_generation_tiles_vs_fp64: 6.5e-07 .. 7.9e-07 / 5.3e-07 .. 1.4e-06

_REF = {}


@pytest.fixture(scope="module", autouse=True)
def drop_references():
    yield
    _REF.clear()


@pytest.fixture
def conv_arith(request):
    lib = L.load()
    before = {name: lib.dmc_get_option(name) for name in (b"conv_arith", b"conv_cfg")}
    L.check(lib.dmc_set_option(b"conv_arith", int(request.param)), "dmc_set_option")
    L.check(lib.dmc_set_option(b"conv_cfg", 0), "dmc_set_option")
    yield int(request.param)
    for name, value in before.items():
        L.check(lib.dmc_set_option(name, value), "dmc_set_option")


def cl(t):
    return t.to(DEV).contiguous(memory_format=CL)


def rel_err(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float(torch.nan_to_num(a - b, nan=float("inf")).abs().max() / b.abs().max().clamp_min(1e-30))


def _wgrad_of(x, go, case):
    """The weight gradient of F.conv2d in the dtype of x, by autograd on the CPU (the input needs no gradient)."""
    n, cin, h, w, cout, k, stride = case
    wt = torch.zeros((cout, cin, k, k), dtype=x.dtype, requires_grad=True)
    (F.conv2d(x, wt, None, stride, k // 2) * go).sum().backward()
    return wt.grad


def reference(case, kind):
    """Once per (case, kind), shared by both arithmetics.  "rand": normal operands, dw in fp64 and in the CPU's fp32; "int": small
    integers, dw exact (kept as fp32)."""
    key = (case, kind)
    if key in _REF:
        return _REF[key]
    n, cin, h, w, cout, k, stride = case
    oh, ow = P.out_map(case)
    g = torch.Generator().manual_seed(7000 + 10 * sum(case) + (kind == "int"))
    r = {}
    if kind == "int":
        r["x"] = torch.randint(-4, 5, (n, cin, h, w), generator=g).float()
        r["go"] = torch.randint(-4, 5, (n, cout, oh, ow), generator=g).float()
        dw = _wgrad_of(r["x"].double(), r["go"].double(), case)
        assert float(dw.abs().max()) < 1 << 24 and 16 * n * oh * ow < 1 << 24
        r["dw"] = dw.float()
    else:
        r["x"] = torch.randn((n, cin, h, w), generator=g)
        r["go"] = torch.randn((n, cout, oh, ow), generator=g)
        r["dw"] = _wgrad_of(r["x"].double(), r["go"].double(), case)
        r["dw32"] = _wgrad_of(r["x"], r["go"], case)
    r["xg"], r["gg"] = cl(r["x"]), cl(r["go"])
    _REF[key] = r
    return r


def run_wgrad(case, xg, gg):
    """dmc_conv_nhwc_wgrad through the C ABI: result and workspace start as NaN."""
    lib = L.load()
    n, cin, h, w, cout, k, stride = case
    dw = torch.empty((cout, cin, k, k), dtype=torch.float32, device=DEV).contiguous(memory_format=CL).fill_(NAN)
    work = ops._floats(lib.dmc_conv_nhwc_wgrad_bytes(n, h, w, cin, cout, k, k, stride, k // 2), DEV).fill_(NAN)
    L.check(lib.dmc_conv_nhwc_wgrad(L.ptr(xg), L.ptr(gg), L.ptr(dw), L.ptr(work), n, h, w, cin, cout, k, k, stride, k // 2,
                                    ops._stream()), "dmc_conv_nhwc_wgrad")
    return dw


def worst_element(dw, want, case):
    n, cin, h, w, cout, k, stride = case
    err = torch.nan_to_num(dw.double().cpu() - want.double().cpu(), nan=float("inf")).abs()       # [co][ci][ky][kx]
    idx = int(err.argmax())
    co, rest = divmod(idx, cin * k * k)
    ci, tap = divmod(rest, k * k)
    bad = int((err > 1e-5 * float(want.abs().max())).sum())
    return "worst element (co %d, tap %d, ci %d) = block (%d, %d) of 64 x 64: got %r, want %r; %d of %d elements are off by more than 1e-5" % (
        co, tap, ci, co // 64, ci // 64, float(dw[co, ci, tap // k, tap % k]), float(want[co, ci, tap // k, tap % k]), bad, err.numel())


def _id(param):
    return "x".join(str(v) for v in param) if isinstance(param, tuple) else "arith%d" % param


#: every run case under bf16x3, the 3 x 3 ones again under fp32 MFMA with the sibling of 20 images (the 1 x 1 kernels are the same
#: launch in either arithmetic); the generic split-K kernel in both
SWEEP = P.WGRAD_RUN_SWEEP + [(P.GENERIC_SPLIT_CASE, 1), (P.GENERIC_SPLIT_CASE, 0)]


@pytest.mark.parametrize("case,conv_arith", SWEEP, indirect=["conv_arith"], ids=_id)
def test_weight_gradient_runs_vs_fp64(case, conv_arith):
    """(a), (c), (d)."""
    p = P.wgrad_plan(case, conv_arith)
    assert L.load().dmc_conv_nhwc_wgrad_bytes(case[0], case[2], case[3], case[1], case[4], case[5], case[5], case[6], case[5] // 2) \
        == P.wgrad_bytes(case, conv_arith)
    r = reference(case, "rand")
    dw = run_wgrad(case, r["xg"], r["gg"])
    e_hip, e_ref = rel_err(dw, r["dw"]), rel_err(r["dw32"], r["dw"])
    print("weight gradient %s conv_arith %d (%s, %s steps in %s groups of %s, last %s): e_hip %.3e, e_ref %.3e"
          % (case, conv_arith, p.kernel, p.steps, p.groups, p.per_group, p.last, e_hip, e_ref))
    assert e_hip <= 1e-5, "%s %s: e_hip %.3e (e_ref %.3e); %s" % (case, p.kernel, e_hip, e_ref, worst_element(dw, r["dw"], case))
    assert torch.equal(dw, run_wgrad(case, r["xg"], r["gg"]))
    assert torch.equal(dw, ops._conv_wgrad(r["xg"], r["gg"], dw, case[6], case[5] // 2))


@pytest.mark.parametrize("case,conv_arith", SWEEP, indirect=["conv_arith"], ids=_id)
def test_weight_gradient_runs_integer_operands_exact(case, conv_arith):
    """(b), (c)."""
    p = P.wgrad_plan(case, conv_arith)
    r = reference(case, "int")
    dw = run_wgrad(case, r["xg"], r["gg"])
    want = r["dw"].to(DEV)
    assert torch.equal(dw, want), "%s %s: %d of %d values differ from fp64; %s" % (
        case, p.kernel, int((dw != want).sum()), dw.numel(), worst_element(dw, r["dw"], case))
    assert torch.equal(dw, run_wgrad(case, r["xg"], r["gg"]))


# ---- (e) code that no other test reaches -------------------------------------------------------------------------------------------

def _fwd_nan(case, xg, wg, bias, keep, nblk, act):
    lib = L.load()
    n, cin, h, w, cout, k, stride = case
    oh, ow = P.out_map(case)
    y = torch.empty((n, cout, oh, ow), dtype=torch.float32, device=DEV, memory_format=CL).fill_(NAN)
    part = torch.full((nblk + 2, cout, 2), NAN, dtype=torch.float64, device=DEV)
    wpack = ops._floats(lib.dmc_conv_nhwc_wt_bytes(cin, cout, k, k), DEV)
    L.check(lib.dmc_conv_nhwc_fwd(L.ptr(xg), L.ptr(wg), L.ptr(wpack), L.ptr(bias), L.ptr(keep), L.ptr(y), L.ptr(part), nblk,
                                  n, h, w, cin, cout, k, k, stride, k // 2, act, ops._stream()), "dmc_conv_nhwc_fwd")
    return y, part


def _check_statistics(part, nblk, y):
    assert bool(torch.isfinite(part[:nblk]).all()), "a statistics row of the launch was not written"
    assert bool(torch.isnan(part[nblk:]).all()), "the launch wrote behind its statistics rows"
    s = part[:nblk].sum(0).cpu()
    yd = y.double().permute(1, 0, 2, 3).reshape(y.shape[1], -1).cpu()
    assert float((s[:, 0] - yd.sum(1)).abs().max()) <= 1e-9 * float(yd.abs().sum(1).max())
    assert float((s[:, 1] - (yd * yd).sum(1)).abs().max()) <= 1e-9 * float((yd * yd).sum(1).max())


@pytest.mark.parametrize("conv_arith", [1, 0], indirect=True)
@pytest.mark.parametrize("case", [P.V1_LARGE_CASE, P.V1_48_CASE], ids=_id)
def test_first_generation_tiles_vs_fp64(case, conv_arith):
    """conv_nhwc_kernel<128, 64, 16, ..> (80 output channels at M = 32768; its data gradient, 48 channels, on <128, 32, 16, ..>) and
    the forward at 48 output channels: whole epilogue and statistics partials, forward and data gradient against fp64 at 1e-5."""
    n, cin, h, w, cout, k, stride = case
    c = P.fwd_choice(case, conv_arith)
    assert c.kernel == "conv_nhwc" and c.bm == 128 and c.bn == (64 if cout >= 64 else 32)
    g = torch.Generator().manual_seed(900 + cout)
    x, wt = torch.randn((n, cin, h, w), generator=g), torch.randn((cout, cin, k, k), generator=g) * 0.1
    go, bias = torch.randn((n, cout, h, w), generator=g), torch.randn(cout, generator=g) * 0.5
    keep = (torch.arange(n * cout).reshape(n, cout) % 4 != 1).float() / 0.75
    xo = x.double().requires_grad_(True)
    pre = F.conv2d(xo, wt.double(), None, stride, 1)
    (pre * go.double()).sum().backward()
    yo = F.leaky_relu(pre.detach() + bias.double()[None, :, None, None], 0.2) * keep.double()[:, :, None, None]
    xg, wg, gg = cl(x), cl(wt), cl(go)
    nblk = L.load().dmc_conv_nhwc_stat_blocks(n, h, w, cin, cout, k, stride, 1)
    assert nblk == P.ceil_div(n * h * w, 128)
    y, part = _fwd_nan(case, xg, wg, bias.to(DEV), keep.to(DEV).contiguous(), nblk, 1)
    e_fwd = rel_err(y, yo)
    _check_statistics(part, nblk, y)
    dx = ops._conv_dgrad(gg, wg, xg.shape, stride, 1)
    e_dx = rel_err(dx, xo.grad)
    print("first-generation tiles %s conv_arith %d: forward %.3e, data gradient %.3e" % (case, conv_arith, e_fwd, e_dx))
    assert e_fwd <= 1e-5 and e_dx <= 1e-5, (e_fwd, e_dx)
    y2, part2, nblk2 = ops._conv_fwd(xg, wg, bias.to(DEV), keep.to(DEV).contiguous(), stride, 1, 1, True)
    assert nblk2 == nblk and torch.equal(y, y2) and torch.equal(part[:nblk], part2)
    assert torch.equal(dx, ops._conv_dgrad(gg, wg, xg.shape, stride, 1))
