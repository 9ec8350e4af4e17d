"""GPU: the kernels of the first discriminator block (disc_first.hip) called directly, against fp64.

dmc_disc_first_fwd has two forms: disc_first_fwd_lds_kernel (Cout 16, W % 4 == 0, W <= 512: the production form, a workgroup
stages nine input rows for four output rows) and the one-thread-per-pixel kernel for everything else.  test_disc_block_unit
runs the block at W = 43 only -- the fallback -- and the whole-discriminator tests reach the LDS form at 224 x 224 alone, so
here it gets shapes of its own: one row, one column quad, an odd height with a partial last strip, the widest row, and its
fallback neighbours on either side of each condition; both forms on the same input agree to 1e-6.  The weight gradient is
run where a wave's run of pixel quads exceeds its 16-quad floor and where a workgroup has waves without work; the data
gradient at the same shapes, odd sizes included.  Reference: F.conv2d(2 -> Cout, 3, stride 2, padding 1) + LeakyReLU(0.2) +
keep mask and autograd in fp64; bars as test_disc_block_unit: 1e-5 forward, 2e-5 gradients.  Outputs and the workspace are
pre-filled with NaN."""
import pytest
import torch
import torch.nn.functional as F

import dmcnet_amd
from dmcnet_amd import ops

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
L = dmcnet_amd._lib
NAN = float("nan")

LDS_SHAPES = [(3, 1, 4), (2, 7, 8), (2, 40, 44), (1, 9, 512), (2, 33, 224)]          # (N, H, W), Cout 16
FALLBACK_SHAPES = [((1, 10, 516), 16), ((2, 40, 43), 16), ((2, 40, 44), 8)]            # W > 512; W % 4 != 0; Cout 8
# (12, 224, 224): 37,632 pixel quads = 19 per wave of the weight gradient, above its 16-quad floor; (1, 3, 5): 6 pixels = one wave with
# work in a workgroup of four -- the final kernel reads the partial slots of the three that had none
GRAD_SHAPES = [(s, 16) for s in LDS_SHAPES] + FALLBACK_SHAPES + [((1, 3, 5), 16), ((2, 9, 7), 8), ((12, 224, 224), 16)]

_REF = {}


@pytest.fixture(scope="module", autouse=True)
def _drop_references():
    yield
    _REF.clear()


def rel_err(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))


def takes_lds_form(shape, cout):
    return cout == 16 and shape[2] % 4 == 0 and shape[2] <= 512


def reference(shape, cout):
    """Operands and the fp64 results, once per (shape, Cout): z with and without (bias, keep), the gradients of the plain conv."""
    key = (shape, cout)
    if key in _REF:
        return _REF[key]
    n, h, w = shape
    oh, ow = (h - 1) // 2 + 1, (w - 1) // 2 + 1
    g = torch.Generator().manual_seed(h * 1000 + w + cout)
    r = dict(x=torch.randn((n, 2, h, w), generator=g), w=torch.randn((cout, 2, 3, 3), generator=g) * 0.3,
             bias=torch.randn(cout, generator=g) * 0.5, keep=(torch.rand((n, cout), generator=g) < 0.75).float() / 0.75,
             go=torch.randn((n, cout, oh, ow), generator=g))
    xo, wo = r["x"].double().requires_grad_(True), r["w"].double().requires_grad_(True)
    pre = F.conv2d(xo, wo, None, 2, 1)
    (pre * r["go"].double()).sum().backward()
    pre = pre.detach()
    r["z_plain"] = F.leaky_relu(pre, 0.2)
    r["z_full"] = F.leaky_relu(pre + r["bias"].double()[None, :, None, None], 0.2) * r["keep"].double()[:, :, None, None]
    r["dx"], r["dw"], r["db"] = xo.grad, wo.grad, r["go"].double().sum((0, 2, 3))
    _REF[key] = r
    return r


def run_fwd(r, shape, cout, full):
    """z as an NCHW view of the NHWC result."""
    lib = L.load()
    n, h, w = shape
    oh, ow = (h - 1) // 2 + 1, (w - 1) // 2 + 1
    x, wt = r["x"].to(DEV), r["w"].to(DEV)
    bias = r["bias"].to(DEV) if full else None
    keep = r["keep"].to(DEV).contiguous() if full else None
    z = torch.full((n, oh, ow, cout), NAN, dtype=torch.float32, device=DEV)
    L.check(lib.dmc_disc_first_fwd(L.ptr(x), L.ptr(wt), L.ptr(bias), L.ptr(keep), L.ptr(z), n, h, w, cout, 1, ops._stream()),
            "dmc_disc_first_fwd")
    return z.permute(0, 3, 1, 2)


@pytest.fixture
def conv_cfg():
    """Set option conv_cfg inside a test; the fixture puts the old value back."""
    lib = L.load()
    before = lib.dmc_get_option(b"conv_cfg")

    def put(value):
        L.check(lib.dmc_set_option(b"conv_cfg", value), "dmc_set_option")
    yield put
    put(before)


@pytest.mark.parametrize("full", [True, False], ids=["bias_mask", "plain"])
@pytest.mark.parametrize("shape,cout", [(s, 16) for s in LDS_SHAPES] + FALLBACK_SHAPES)
def test_forward_both_forms_vs_fp64(shape, cout, full, conv_cfg):
    assert L.load().dmc_disc_first_supported(cout) == 1 and L.load().dmc_get_option(b"conv_cfg") == 0
    r = reference(shape, cout)
    want = r["z_full"] if full else r["z_plain"]
    z = run_fwd(r, shape, cout, full)
    assert rel_err(z, want) < 1e-5
    assert torch.equal(z, run_fwd(r, shape, cout, full))
    if takes_lds_form(shape, cout):
        conv_cfg(305)                       # the one-thread-per-pixel form on the same input
        try:
            zf = run_fwd(r, shape, cout, full)
        finally:
            conv_cfg(0)
        assert rel_err(zf, want) < 1e-5
        assert rel_err(z, zf) < 1e-6        # the same 18 products and bias per value in both forms


@pytest.mark.parametrize("shape,cout", GRAD_SHAPES)
def test_data_gradient_vs_fp64(shape, cout):
    lib = L.load()
    n, h, w = shape
    r = reference(shape, cout)
    g = r["go"].to(DEV).permute(0, 2, 3, 1).contiguous()             # [N][OH][OW][Cout]
    dx = torch.full((n, 2, h, w), NAN, dtype=torch.float32, device=DEV)
    L.check(lib.dmc_disc_first_dgrad(L.ptr(g), L.ptr(r["w"].to(DEV)), L.ptr(dx), n, h, w, cout, ops._stream()), "dmc_disc_first_dgrad")
    assert rel_err(dx, r["dx"]) < 2e-5


def run_wgrad(r, shape, cout):
    lib = L.load()
    n, h, w = shape
    x = r["x"].to(DEV)
    g = r["go"].to(DEV).permute(0, 2, 3, 1).contiguous()
    dw = torch.full((cout, 2, 3, 3), NAN, dtype=torch.float32, device=DEV)
    db = torch.full((cout,), NAN, dtype=torch.float32, device=DEV)
    work = ops._floats(lib.dmc_disc_first_wgrad_bytes(cout), DEV).fill_(NAN)
    L.check(lib.dmc_disc_first_wgrad(L.ptr(x), L.ptr(g), L.ptr(dw), L.ptr(db), L.ptr(work), n, h, w, cout, ops._stream()),
            "dmc_disc_first_wgrad")
    return dw, db


@pytest.mark.parametrize("shape,cout", GRAD_SHAPES)
def test_weight_and_bias_gradient_vs_fp64(shape, cout):
    r = reference(shape, cout)
    dw, db = run_wgrad(r, shape, cout)
    assert bool(torch.isfinite(dw).all()) and bool(torch.isfinite(db).all()), "a partial slot was read but never written"
    assert rel_err(dw, r["dw"]) < 2e-5
    assert rel_err(db, r["db"]) < 2e-5
    dw2, db2 = run_wgrad(r, shape, cout)
    assert torch.equal(dw, dw2) and torch.equal(db, db2)


def test_weight_gradient_shapes_cover_both_ends():
    def waves(n, h, w):
        quads = (n * ((h - 1) // 2 + 1) * ((w - 1) // 2 + 1) + 3) // 4
        per = max(-(-quads // 2048), 16)
        return quads, per, -(-quads // per)
    quads, per, nw = waves(12, 224, 224)
    assert quads == 37632 and per > 16 and nw > 4
    quads, per, nw = waves(1, 3, 5)
    assert per == 16 and nw == 1                                      # a workgroup of four waves, one with work
