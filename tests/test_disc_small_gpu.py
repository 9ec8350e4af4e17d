"""GPU: the kernels of csrc/disc_c8.hip (Discriminator4's 8 -> 16, stride-2 block) and csrc/disc_head.hip (adv_layer on the NHWC
activation) through the C ABI, against fp64 references computed on the CPU (tests/disc_small_ref.py).

Bars (derived, not tuned): an fp32 sum of K products is within (K + 2) * 2^-24 * S of the fp64 value, S the same contraction of
absolute values; K = 72 + 1 (block forward / data gradient), N * OH * OW (block weight gradient), C * H * W (head forward), M
(head dweight / dbias), 2 (head dx).  The fp64 statistic partials, summed, equal the fp64 sums of the kernel's own z and z^2 to
n * 2^-53 * sum |.|.  One-hot operands come back bit for bit; two runs give the same bits.  Every case prints its worst
error / bar."""
import pytest
import torch

from dmcnet_amd import _lib, ops
from tests import disc_small_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
INVALID = -1


def call(name, *args):
    lib = _lib.load()
    conv = [_lib.ptr(a) if (a is None or isinstance(a, torch.Tensor)) else a for a in args]
    rc = getattr(lib, name)(*(conv + [ops._stream()]))
    torch.cuda.synchronize()
    return rc


def dev(t):
    return None if t is None else t.to(DEV).contiguous()


def empty(shape, dtype=torch.float32):
    return torch.full(shape, float("nan"), dtype=dtype, device=DEV)


def c8_fwd(shape, x, w, bias, keep, act, stats):
    n, h, wd = shape
    oh, ow = R.out_hw(h, wd)
    z = empty((n, oh, ow, 16))
    nblk = _lib.load().dmc_disc_c8_stat_blocks(n, h, wd)
    part = empty((nblk, 16, 2), torch.float64) if stats else None
    rc = call("dmc_disc_c8_fwd", dev(x), dev(w), dev(bias), dev(keep), z, part, nblk if stats else 0, n, h, wd, int(act))
    return rc, z, part


def c8_dgrad(shape, g, w):
    n, h, wd = shape
    dx = empty((n, h, wd, 8))
    return call("dmc_disc_c8_dgrad", dev(g), dev(w), dx, n, h, wd), dx


def c8_wgrad(shape, x, g, with_db=True, work_fill=None):
    n, h, wd = shape
    dw, db = empty((16, 3, 3, 8)), (empty((16,)) if with_db else None)
    work = torch.empty(max(_lib.load().dmc_disc_c8_wgrad_bytes(n, h, wd), 4) // 4, dtype=torch.float32, device=DEV)
    if work_fill is not None:
        work.fill_(work_fill)
    return call("dmc_disc_c8_wgrad", dev(x), dev(g), dw, db, work, n, h, wd), dw, db


OPTIONS = [(True, True, 1, True), (False, False, 0, False), (True, False, 1, False), (False, True, 0, True), (False, True, 1, False)]


def check_c8(shape):
    d = R.c8_inputs(shape)
    worst = {}
    for with_bias, with_keep, act, stats in OPTIONS:
        rc, z, part = c8_fwd(shape, d["x"], d["w"], d["bias"] if with_bias else None, d["keep"] if with_keep else None, act, stats)
        assert rc == 0
        z64, bar = R.c8_forward(shape, with_bias, with_keep, act)
        worst["fwd"] = max(worst.get("fwd", 0.0), R.ratio(z, z64, bar))
        if stats:
            zd = z.double().cpu().reshape(-1, 16)
            cnt = zd.shape[0]
            got = part.cpu().sum(0)
            for k, v in ((0, zd), (1, zd * zd)):
                sbar = cnt * 2.0 ** -53 * v.abs().sum(0)
                worst["stats"] = max(worst.get("stats", 0.0), R.ratio(got[:, k], v.sum(0), sbar))
    g = R.c8_grads(shape)
    rc, dx = c8_dgrad(shape, d["g"], d["w"])
    assert rc == 0
    worst["dgrad"] = R.ratio(dx, g["dx"], g["dx_bar"])
    rc, dw, db = c8_wgrad(shape, d["x"], d["g"])
    assert rc == 0
    worst["wgrad"] = max(R.ratio(dw, g["dw"], g["dw_bar"]), R.ratio(db, g["db"], g["db_bar"]))
    rc, dw2, _ = c8_wgrad(shape, d["x"], d["g"], with_db=False, work_fill=float("nan"))
    assert rc == 0 and torch.equal(dw, dw2)                      # no db; nothing depends on what the workspace held
    print("disc_c8 %s: worst error / bar %s" % (R.sid(shape), ", ".join("%s %.3f" % kv for kv in sorted(worst.items()))))
    for k, v in worst.items():
        assert v <= 1.0, (k, v)


@pytest.mark.parametrize("shape", R.C8_SHAPES, ids=R.sid)
def test_c8_block_within_the_fp32_bars(shape):
    """(1, 112, 112) is the real geometry and gives the weight gradient six full runs of 512 output pixels and a partial one;
    (2, 18, 34) has a ragged last forward workgroup and a pixel count that is no multiple of 64."""
    assert _lib.load().dmc_disc_c8_supported(*shape) == 1
    check_c8(shape)


@pytest.mark.parametrize("shape", R.C8_ODD_SHAPES, ids=R.sid)
def test_c8_block_odd_sizes_are_served_within_the_bars_or_refused_untouched(shape):
    lib = _lib.load()
    if lib.dmc_disc_c8_supported(*shape):
        check_c8(shape)
        return
    d = R.c8_inputs(shape)
    assert lib.dmc_disc_c8_stat_blocks(*shape) == 0 and lib.dmc_disc_c8_wgrad_bytes(*shape) == 0
    rc, z, _ = c8_fwd(shape, d["x"], d["w"], d["bias"], d["keep"], 1, False)
    assert rc == INVALID and bool(torch.isnan(z).all())
    rc, dx = c8_dgrad(shape, d["g"], d["w"])
    assert rc == INVALID and bool(torch.isnan(dx).all())
    rc, dw, db = c8_wgrad(shape, d["x"], d["g"])
    assert rc == INVALID and bool(torch.isnan(dw).all()) and bool(torch.isnan(db).all())


def test_c8_one_hot_operands_come_back_bit_for_bit():
    """One-hot x (forward) or g (data / weight gradient) against random operands: every output is one product (or zero), which
    the fp64 evaluation rounded to fp32 gives exactly."""
    shape = (3, 12, 20)
    d = R.c8_inputs(shape)
    x = torch.zeros_like(d["x"])
    for n, y, xx, c in ((0, 0, 0, 0), (1, 5, 8, 3), (2, 11, 19, 7)):
        x[n, y, xx, c] = 1.5
    rc, z, _ = c8_fwd(shape, x, d["w"], None, None, 0, False)
    want = R.nhwc(torch.nn.functional.conv2d(R.nchw(x).double(), d["w"].permute(0, 3, 1, 2).double(), None, 2, 1)).float()
    assert rc == 0 and int((want != 0).sum()) >= 16 * (1 + 2 + 1) and torch.equal(z.cpu(), want)
    for shp, hot in ((shape, (1, 2, 7, 5)), ((1, 112, 112), (0, 30, 5, 11)), ((1, 112, 112), (0, 55, 55, 0))):
        dd = R.c8_inputs(shp)
        g = torch.zeros_like(dd["g"])
        g[hot] = 1.5
        xr = R.nchw(dd["x"]).double().contiguous().requires_grad_(True)
        wr = dd["w"].permute(0, 3, 1, 2).double().contiguous().requires_grad_(True)
        gx, gw = torch.autograd.grad((torch.nn.functional.conv2d(xr, wr, None, 2, 1) * R.nchw(g).double()).sum(), [xr, wr])
        rc, dx = c8_dgrad(shp, g, dd["w"])
        assert rc == 0 and torch.equal(dx.cpu(), R.nhwc(gx).float())
        rc, dw, db = c8_wgrad(shp, dd["x"], g)
        want_db = torch.zeros(16)
        want_db[hot[3]] = 1.5
        assert rc == 0 and torch.equal(dw.cpu(), gw.permute(0, 2, 3, 1).float()) and torch.equal(db.cpu(), want_db)


def test_c8_is_deterministic():
    shape = (1, 112, 112)
    d = R.c8_inputs(shape)
    a = (c8_fwd(shape, d["x"], d["w"], d["bias"], d["keep"], 1, True)[1:], c8_dgrad(shape, d["g"], d["w"])[1], c8_wgrad(shape, d["x"], d["g"])[1:])
    b = (c8_fwd(shape, d["x"], d["w"], d["bias"], d["keep"], 1, True)[1:], c8_dgrad(shape, d["g"], d["w"])[1], c8_wgrad(shape, d["x"], d["g"])[1:])
    assert torch.equal(a[0][0], b[0][0]) and torch.equal(a[0][1], b[0][1]) and torch.equal(a[1], b[1])
    assert torch.equal(a[2][0], b[2][0]) and torch.equal(a[2][1], b[2][1])


def test_c8_refuses_a_wrong_stat_blocks_without_writing():
    shape = (2, 18, 34)
    n, h, w = shape
    d = R.c8_inputs(shape)
    nblk = _lib.load().dmc_disc_c8_stat_blocks(*shape)
    assert nblk == 2
    for wrong in (nblk - 1, nblk + 1, 0):
        z, part = empty((n, 9, 17, 16)), empty((nblk + 1, 16, 2), torch.float64)
        rc = call("dmc_disc_c8_fwd", dev(d["x"]), dev(d["w"]), None, None, z, part, wrong, n, h, w, 1)
        assert rc == INVALID and bool(torch.isnan(z).all()) and bool(torch.isnan(part).all())


# ---------------------------------------------------------------------------------------------------------------- head

def head_fwd(shape, x, weight, bias):
    m, c, h, w = shape
    v = empty((m, 2))
    return call("dmc_disc_head_fwd", dev(x), dev(weight), dev(bias), v, m, c, h, w), v


def head_bwd(shape, x, weight, dv, want, work_fill=None):
    """``want``: a subset of "xwb".  Only what the call needs is passed: a dx-only call gets neither x nor a workspace."""
    m, c, h, w = shape
    dx = empty((m, h, w, c)) if "x" in want else None
    dw = empty((2, c * h * w)) if "w" in want else None
    db = empty((2,)) if "b" in want else None
    work = None
    if "w" in want:
        work = torch.empty(_lib.load().dmc_disc_head_bwd_bytes(m, c, h, w) // 4, dtype=torch.float32, device=DEV)
        if work_fill is not None:
            work.fill_(work_fill)
    rc = call("dmc_disc_head_bwd", dev(x) if "w" in want else None, dev(weight) if "x" in want else None, dev(dv), dx, dw, db, work, m, c, h, w)
    return rc, dx, dw, db


@pytest.mark.parametrize("shape", R.HEAD_SHAPES, ids=R.sid)
def test_head_within_the_fp32_bars(shape):
    assert _lib.load().dmc_disc_head_supported(*shape) == 1
    d, ref = R.head_inputs(shape), R.head_ref(shape)
    rc, v = head_fwd(shape, d["x"], d["weight"], d["bias"])
    assert rc == 0
    worst = {"fwd": R.ratio(v, ref["v"], ref["v_bar"])}
    full = None
    for want in ("xwb", "x", "wb"):
        rc, dx, dw, db = head_bwd(shape, d["x"], d["weight"], d["dv"], want, work_fill=float("nan") if want == "wb" else None)
        assert rc == 0
        if "x" in want:
            worst["dx"] = max(worst.get("dx", 0.0), R.ratio(dx, ref["dx"], ref["dx_bar"]))
        if "w" in want:
            worst["dweight"] = max(worst.get("dweight", 0.0), R.ratio(dw, ref["dw"], ref["dw_bar"]))
            worst["dbias"] = max(worst.get("dbias", 0.0), R.ratio(db, ref["db"], ref["db_bar"]))
        if full is None:
            full = (dx, dw, db)
        else:           # the partial calls give the bits of the full one
            for a, b in zip(full, (dx, dw, db)):
                assert b is None or torch.equal(a, b)
    print("disc_head %s: worst error / bar %s" % (R.sid(shape), ", ".join("%s %.3f" % kv for kv in sorted(worst.items()))))
    for k, val in worst.items():
        assert val <= 1.0, (k, val)


def test_head_one_hot_operands_come_back_bit_for_bit():
    shape = (5, 128, 14, 14)
    m, c, h, w = shape
    d = R.head_inputs(shape)
    m0, h0, w0, c0 = 3, 9, 13, 77
    col = c0 * h * w + h0 * w + w0
    x = torch.zeros_like(d["x"])
    x[m0, h0, w0, c0] = 2.0
    rc, v = head_fwd(shape, x, d["weight"], d["bias"])
    want = d["bias"].repeat(m, 1)
    want[m0] = d["bias"] + 2.0 * d["weight"][:, col]             # one exact product, one fp32 addition
    assert rc == 0 and torch.equal(v.cpu(), want)
    # dweight: one-hot x against random dvalidity -> one product per row of the weight
    x[m0, h0, w0, c0] = 1.5
    rc, _, dw, db = head_bwd(shape, x, d["weight"], d["dv"], "wb")
    want = torch.zeros(2, c * h * w)
    want[:, col] = (d["dv"][m0].double() * 1.5).float()
    assert rc == 0 and torch.equal(dw.cpu(), want)
    # dx: one-hot dvalidity against the random weight -> a scaled copy of one weight row in the frame's NHWC order
    for j in (0, 1):
        dv = torch.zeros(m, 2)
        dv[m0, j] = 1.5
        rc, dx, _, _ = head_bwd(shape, None, d["weight"], dv, "x")
        want = torch.zeros(m, h, w, c)
        want[m0] = (d["weight"][j].double() * 1.5).float().reshape(c, h, w).permute(1, 2, 0)
        assert rc == 0 and torch.equal(dx.cpu(), want)


def test_head_is_deterministic():
    shape = (12, 128, 14, 14)
    d = R.head_inputs(shape)
    runs = [(head_fwd(shape, d["x"], d["weight"], d["bias"])[1],) + head_bwd(shape, d["x"], d["weight"], d["dv"], "xwb")[1:] for _ in range(2)]
    for a, b in zip(*runs):
        assert torch.equal(a, b)


def test_head_refusals_write_nothing():
    lib = _lib.load()
    assert lib.dmc_disc_head_supported(1, 24, 2, 2) == 0 and lib.dmc_disc_head_bwd_bytes(1, 24, 2, 2) == 0      # C no multiple of 16
    assert lib.dmc_disc_head_supported(32768, 16, 64, 64) == 0 and lib.dmc_disc_head_supported(32767, 16, 64, 64) == 1    # 2^31 elements
    shape = (2, 24, 2, 2)
    x, wt, b, dv = R.rnd(1, (2, 2, 2, 24)), R.rnd(2, (2, 96)), R.rnd(3, (2,)), R.rnd(4, (2, 2))
    rc, v = head_fwd(shape, x, wt, b)
    assert rc == INVALID and bool(torch.isnan(v).all())
    rc, dx, dw, db = head_bwd(shape, x, wt, dv, "xb")
    assert rc == INVALID and bool(torch.isnan(dx).all()) and bool(torch.isnan(db).all())
    good = (1, 16, 2, 3)
    d = R.head_inputs(good)
    v = empty((1, 2))
    assert call("dmc_disc_head_fwd", dev(d["x"]), None, dev(d["bias"]), v, *good) == INVALID and bool(torch.isnan(v).all())
    dw = empty((2, 96))
    assert call("dmc_disc_head_bwd", None, None, dev(d["dv"]), None, dw, None, None, *good) == INVALID and bool(torch.isnan(dw).all())
