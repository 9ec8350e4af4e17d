"""GPU: the early-fusion estimators on their own kernels (csrc/early_fusion.hip, ops.early_fusion_eval / early_fusion_train).

  1. each forward entry point alone against fp64 (tests/ef_ref.py), with the bytes it must not touch pre-filled with 0xFF;
  2. the one-hot sweep: every (tap, buffer channel) of every layer returns its weight exactly;
  3. whole networks: the reference's own golden, fp64 under the project's criterion e <= max(4 e_ref, 2e-5 max|y|), isolation of a
     frame, frame ranges, byte offsets past 4 GiB;
  4. dispatch: the evaluator runs 1 + 4 + 1 launches per range and nothing stock; everything else is the stock loop bit for bit;
  5. training: the fourteen parameter gradients against fp64 autograd, the two LeakyReLU branches of Sum, the optimizer step.

Tolerance of the single-entry cases: a sum of at most 9 * 36 = 324 fp32 FMAs has a statistical error of about sqrt(324) * 2^-24 = 1e-6
of its terms' magnitude and these layers' outputs are of their terms' magnitude; the bar is the 1e-5 max|ref| that the dense
estimators' head, the same kind of kernel with a longer sum, is held to (tests/test_dense_eval_gpu.py)."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import dmcnet_amd
from dmcnet_amd import _lib, model, ops
from oracle import dmc_oracle as O
from tests import ef_ref as E

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U8 = torch.uint8
ALL_SHAPES = E.MAIN_SHAPES + E.DEGENERATE_SHAPES


def P(t):
    return _lib.ptr(t)


def ok(rc, what):
    _lib.check(rc, what)


def bits(t):
    return t.detach().contiguous().view(torch.int32)


def rel_err(a, b):
    a, b = a.detach().double().cpu(), torch.as_tensor(b).detach().double().cpu()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))


def ff_buffer(shape):
    """A device fp32 tensor whose every byte is 0xFF (NaN)."""
    n = int(np.prod(shape))
    return torch.full((4 * n,), 0xFF, dtype=U8, device=DEV).view(torch.float32).view(shape)


def is_ff(t):
    return bool((bits(t) == -1).all())


def route_on(monkeypatch):
    """DMC_EF_EVAL=1: the eval route for both classes, whatever their default."""
    monkeypatch.setattr(model, "EF_EVAL", True)
    monkeypatch.setattr(model, "EF_EVAL_ALL", True)


@functools.lru_cache(maxsize=None)
def seeded_net(name):
    return E.net(name, DEV).eval()


class Recorder(object):
    def __init__(self, lib):
        self._lib, self.calls = lib, []

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if not name.startswith("dmc_"):
            return fn

        def call(*args):
            self.calls.append(name)
            return fn(*args)
        return call

    def launches(self):
        return [c for c in self.calls if c.startswith("dmc_ef_") and not c.endswith(("_supported", "_bytes"))]


# =====================================================================================================================
# 1. the forward entry points alone
# =====================================================================================================================
def run_first(name, x, ct, stack, want_signs=True, ps=None):
    """dmc_ef_first on the seeded parameters of ``name`` (or on ``ps`` = [(w_mv, b_mv), (w_r, b_r)]) -> (feat, signs)."""
    n, _, h, w = x.shape
    (wm, bm), (wr, br) = [(a.detach().to(DEV).contiguous(), b.detach().to(DEV).contiguous()) for a, b in (ps or E.params(name)[:2])]
    feat = ff_buffer((n, h, w, ct))
    signs = torch.full((n, h, w), -1, dtype=torch.int16, device=DEV) if want_signs else None
    ok(_lib.load().dmc_ef_first(P(x), P(wm), P(bm), P(wr), P(br), P(feat), P(signs), n, h, w, ct, int(stack), ops._stream()), "dmc_ef_first")
    return feat, signs


@pytest.mark.parametrize("shape", ALL_SHAPES, ids=E.sid)
@pytest.mark.parametrize("name", E.NETS)
def test_first_vs_fp64(name, shape):
    x, f, _ = E.reference(name, shape)
    stack = name == "Stack"
    ct = E.layout(name)["ct"]
    feat, signs = run_first(name, x.to(DEV), ct, stack)
    live = 16 if stack else 8
    want = torch.cat((f["m"], f["r"]), 1) if stack else f["base"]
    e = rel_err(feat[..., :live].permute(0, 3, 1, 2), want)
    print("ef first %s %s: rel_err %.3e" % (name, shape, e))
    assert e < 1e-5, e
    assert is_ff(feat[..., live:])                                          # nothing else is written
    # the sign plane: bit c = (a_c > 0), bit 8 + c = (b_c > 0), wherever fp32 cannot be on the other side of zero
    s = signs.cpu().to(torch.int32) & 0xFFFF
    for half, pre in ((0, f["a"]), (8, f["b"])):
        for c in range(8):
            got = ((s >> (half + c)) & 1).bool()
            sure = pre[:, c].abs() > 1e-4
            assert torch.equal(got[sure], (pre[:, c] > 0)[sure]), (half, c)
    # both flags see the same a and b bits: the other flag's launch on the same weights gives the same sign plane, and Sum's value
    # is the fp32 sum of Stack's two slots
    other, signs2 = run_first(name, x.to(DEV), 40, not stack)
    assert torch.equal(signs, signs2)
    st, sm = (feat, other) if stack else (other, feat)
    assert torch.equal(bits(st[..., :8] + st[..., 8:16]), bits(sm[..., :8]))
    again, signs3 = run_first(name, x.to(DEV), ct, stack)
    assert torch.equal(bits(again), bits(feat)) and torch.equal(signs, signs3)      # run to run
    quiet, none = run_first(name, x.to(DEV), ct, stack, want_signs=False)           # signs is optional
    assert none is None and torch.equal(bits(quiet), bits(feat))


@functools.lru_cache(maxsize=None)
def layer_case(name, li, shape):
    """(buffer [N, H, W, CT] fp32 CPU with NaN from channel K on, weight [R, 9, K], bias [R], fp64 result [N, R, H, W]) of conv_{li + 1}
    (li == 4: predict_flow, no activation) on the fp32 activations of the fp64 forward in front of it.  Never modified."""
    lay = E.layout(name)
    k, r, index = (lay["layers"] + [lay["head"]])[li]
    _, f, _ = E.reference(name, shape)
    buf = E.to_buffer(name, f, li + 1)
    assert not bool(torch.isnan(buf[..., :k]).any()) and bool(torch.isnan(buf[..., k:]).all())
    wt, b = E.params(name)[2 + li]
    pre = F.conv2d(E.gather_input(index, buf[..., :k]).double(), wt.double(), b.double(), 1, 1)
    return buf, E.buffer_weight(wt, k, index), b, (pre if li == 4 else F.leaky_relu(pre, E.SLOPE))


def run_layer(feat, wb, bias, k, r):
    n, h, w, ct = feat.shape
    ok(_lib.load().dmc_ef_layer(P(feat), P(wb), P(bias), n, h, w, ct, k, r, ops._stream()), "dmc_ef_layer")


@pytest.mark.parametrize("shape", ALL_SHAPES, ids=E.sid)
@pytest.mark.parametrize("li", [0, 1, 2, 3])
@pytest.mark.parametrize("name", E.NETS)
def test_layer_vs_fp64(name, li, shape):
    buf, wb, b, ref = layer_case(name, li, shape)
    k, r = wb.shape[2], wb.shape[0]
    r4 = (r + 3) // 4 * 4
    assert _lib.load().dmc_ef_supported(buf.shape[0], buf.shape[1], buf.shape[2], buf.shape[3], k, r) == 1
    feat = ff_buffer(tuple(buf.shape))
    feat[..., :k] = buf[..., :k].to(DEV)
    before = feat.clone()
    wd, bd = wb.to(DEV), b.to(DEV)
    run_layer(feat, wd, bd, k, r)
    e = rel_err(feat[..., k:k + r].permute(0, 3, 1, 2), ref)
    print("ef layer %s conv_%d %s: rel_err %.3e" % (name, li + 1, shape, e))
    assert e < 1e-5, e
    assert bool((bits(feat[..., k + r:k + r4]) == 0).all())                 # pad channels: +0.0
    assert torch.equal(bits(feat[..., :k]), bits(before[..., :k])) and is_ff(feat[..., k + r4:])
    again = before.clone()
    run_layer(again, wd, bd, k, r)
    assert torch.equal(bits(again), bits(feat))                             # run to run


@pytest.mark.parametrize("shape", ALL_SHAPES, ids=E.sid)
@pytest.mark.parametrize("name", E.NETS)
def test_head_vs_fp64(name, shape):
    buf, wb, b, ref = layer_case(name, 4, shape)
    n, h, w, ct = buf.shape
    k = wb.shape[2]
    feat = buf.to(DEV)
    before = feat.clone()
    outs = []
    wd, bd = wb.to(DEV), b.to(DEV)
    for _ in range(2):
        out = ff_buffer((n, 2, h, w))
        ok(_lib.load().dmc_ef_head(P(feat), P(wd), P(bd), P(out), n, h, w, ct, k, ops._stream()), "dmc_ef_head")
        outs.append(out)
    e = rel_err(outs[0], ref)
    print("ef head %s %s: rel_err %.3e" % (name, shape, e))
    assert e < 1e-5, e
    assert torch.equal(bits(feat), bits(before))                            # the buffer is read only
    assert torch.equal(bits(outs[0]), bits(outs[1]))


# =====================================================================================================================
# 2. one-hot sweep
# =====================================================================================================================
HOT = [(1, 1), (0, 0), (0, 2), (2, 0), (2, 2), (0, 1)]      # the centre of a 3 x 3 frame sees all nine taps, corners and an edge lose some


@pytest.mark.parametrize("li", [0, 1, 2, 3, 4])
@pytest.mark.parametrize("name", E.NETS)
def test_one_hot_sweep_over_every_tap_and_buffer_channel(name, li):
    """One frame per (buffer channel, position of the 1.0): the output at pixel p - o(t) is w[r][t][c] bit for bit (positive
    weights: the LeakyReLU passes them as they are; zero bias) and exactly 0 everywhere else -- a tap outside the frame has no
    pixel to land on.  A wrong channel permutation, pixel stride or tap offset shows at the position that uses it."""
    lay = E.layout(name)
    k, r, _ = (lay["layers"] + [lay["head"]])[li]
    ct = lay["ct"]
    rs = np.random.RandomState(930 + li)
    wt = torch.from_numpy((0.5 + rs.random_sample((r, k, 3, 3))).astype(np.float32))        # [R, K, 3, 3], buffer order
    x = torch.zeros((k * len(HOT), k, 3, 3))
    for c in range(k):
        for j, (py, px) in enumerate(HOT):
            x[c * len(HOT) + j, c, py, px] = 1.0
    want = F.conv2d(x.double(), wt.double(), None, 1, 1)                                   # one term each: exact
    assert torch.equal(want.float().double(), want) and int((want != 0).sum()) == k * r * (9 + 4 * 4 + 6)
    wb = wt.permute(0, 2, 3, 1).reshape(r, 9, k).contiguous().to(DEV)
    feat = ff_buffer((x.shape[0], 3, 3, ct))
    feat[..., :k] = x.permute(0, 2, 3, 1).to(DEV)
    zero = torch.zeros(r, device=DEV)
    n = x.shape[0]
    if li == 4:
        got = ff_buffer((n, 2, 3, 3))
        ok(_lib.load().dmc_ef_head(P(feat), P(wb), P(zero), P(got), n, 3, 3, ct, k, ops._stream()), "dmc_ef_head")
    else:
        run_layer(feat, wb, zero, k, r)
        got = feat[..., k:k + r].permute(0, 3, 1, 2)
    assert torch.equal(bits(got.cpu()), bits(want.float())), "%d of %d values differ" % (int((got.cpu() != want.float()).sum()), want.numel())


# =====================================================================================================================
# 3. whole networks
# =====================================================================================================================
@pytest.mark.parametrize("name", E.NETS)
def test_whole_network_vs_reference_golden(name, golden, monkeypatch):
    g = golden("g2_model_eval")
    route_on(monkeypatch)
    m = seeded_net(name)
    x = E.rnd(24, (2, 5, 48, 48)).to(DEV)                          # (the golden's rnd(24, ...): the same draw)
    rec = Recorder(_lib.load())
    monkeypatch.setattr(_lib, "load", lambda: rec)
    with torch.no_grad():
        assert ops.early_fusion_supported(m, x)
        got = m(x)
    assert rec.launches() == ["dmc_ef_first"] + ["dmc_ef_layer"] * 4 + ["dmc_ef_head"]
    np.testing.assert_allclose(got.cpu().numpy(), g["est_" + E.ARCH[name]], rtol=1e-4, atol=1e-5)


@pytest.mark.parametrize("shape", E.MAIN_SHAPES + [E.ROW_SHAPE], ids=E.sid)
@pytest.mark.parametrize("name", E.NETS)
def test_whole_network_vs_fp64(name, shape, monkeypatch):
    route_on(monkeypatch)
    m = seeded_net(name)
    x, f, ref32 = E.reference(name, shape)
    ref64 = f["out"]
    with torch.no_grad():
        assert ops.early_fusion_supported(m, x.to(DEV))
        got = m(x.to(DEV))
    assert tuple(got.shape) == tuple(ref64.shape)
    e = float((got.double().cpu() - ref64).abs().max())
    e_ref = float((ref32.double() - ref64).abs().max())
    top = float(ref64.abs().max())
    print("ef chain %s %s: e %.3e e_ref %.3e max|y| %.3e" % (name, shape, e, e_ref, top))
    assert e <= max(4 * e_ref, 2e-5 * top), (e, e_ref, top)


@pytest.mark.parametrize("name", E.NETS)
def test_frame_result_is_independent_of_its_batch_and_neighbours(name, monkeypatch):
    route_on(monkeypatch)
    m = seeded_net(name)
    f, g, h2 = (E.rnd(40 + i, (1, 5, 20, 37)).to(DEV) for i in range(3))
    wild = E.rnd(49, (1, 5, 20, 37), 1e6).to(DEV)
    with torch.no_grad():
        alone = m(f)
        first = m(torch.cat((f, g, h2)))
        last = m(torch.cat((g, h2, f)))
        changed = m(torch.cat((f, wild, h2)))
    assert torch.equal(bits(alone[0]), bits(first[0])) and torch.equal(bits(alone[0]), bits(last[2]))
    assert torch.equal(bits(changed[0]), bits(first[0])) and torch.equal(bits(changed[2]), bits(first[2]))
    assert not torch.equal(changed[1], first[1])


@pytest.mark.parametrize("name", E.NETS)
def test_frame_ranges_equal_one_range(name, monkeypatch):
    route_on(monkeypatch)
    m = seeded_net(name)
    ct = E.layout(name)["ct"]
    x = E.rnd(41, (5, 5, 20, 37)).to(DEV)
    rec = Recorder(_lib.load())
    monkeypatch.setattr(_lib, "load", lambda: rec)
    with torch.no_grad():
        assert ops.dense_eval_chunks(5, 20, 37, ct) == [(0, 5)]
        one = m(x)
        monkeypatch.setattr(ops, "DENSE_EVAL_BUDGET", 2 * 20 * 37 * ct * 4)
        assert ops.dense_eval_chunks(5, 20, 37, ct) == [(0, 2), (2, 4), (4, 5)]
        del rec.calls[:]
        many = m(x)
    assert rec.launches() == (["dmc_ef_first"] + ["dmc_ef_layer"] * 4 + ["dmc_ef_head"]) * 3
    assert torch.equal(bits(one), bits(many))


def test_byte_offsets_past_4_gib():
    """540 frames of 224 x 224 with 40 buffer channels: 4.33 GB, 1.084e9 elements (one launch).  Stack's conv_1 (K 16, R 8): the slot of
    the first and of the last frame equals what the same entry point returns on one-frame copies, bit for bit (a truncated offset
    lands in another frame or another pixel)."""
    n, h, w, ct, k, r = 540, 224, 224, 40, 16, 8
    assert n * h * w * ct * 4 > 2 ** 32 and n * h * w * ct < 2 ** 31
    assert _lib.load().dmc_ef_supported(n, h, w, ct, k, r) == 1
    try:
        feat = torch.empty((n, h, w, ct), dtype=torch.float32, device=DEV)
    except RuntimeError as e:                                      # (torch.cuda.OutOfMemoryError is one)
        pytest.skip("cannot allocate the 4.33 GB feature buffer: %s" % str(e).splitlines()[0])
    feat.normal_(generator=torch.Generator(device=DEV).manual_seed(77))
    lay = E.layout("Stack")
    wt, b = E.params("Stack")[2]
    wb, bias = E.buffer_weight(wt, k, lay["layers"][0][2]).to(DEV), b.to(DEV)
    singles = {f: feat[f:f + 1].clone() for f in (0, n - 1)}
    run_layer(feat, wb, bias, k, r)
    for f, one in singles.items():
        before = one.clone()
        run_layer(one, wb, bias, k, r)
        assert not torch.equal(bits(one[..., k:k + r]), bits(before[..., k:k + r]))
        assert torch.equal(bits(feat[f:f + 1]), bits(one)), f
    ref = F.conv2d(singles[n - 1][:, :8, :8, :k].permute(0, 3, 1, 2).double().cpu(), wt.double(), b.double(), 1, 1)[:, :, :7, :7]
    assert rel_err(feat[n - 1:n, :7, :7, k:k + r].permute(0, 3, 1, 2), F.leaky_relu(ref, E.SLOPE)) < 1e-5


# =====================================================================================================================
# 4. dispatch
# =====================================================================================================================
def forbid_stock_ops_inside(gen, monkeypatch):
    """Patches F.conv2d, torch.cat and Tensor.cat to raise, but only while ``gen.forward`` runs (the classifier behind the generator
    is not what this file is about)."""
    inner = gen.forward

    def boom(*a, **kw):
        raise AssertionError("a stock convolution or concatenation ran inside the generator")

    def guarded(x):
        with pytest.MonkeyPatch.context() as mp:
            mp.setattr(torch.nn.functional, "conv2d", boom)
            mp.setattr(torch, "cat", boom)
            mp.setattr(torch.Tensor, "cat", boom, raising=False)
            return inner(x)
    monkeypatch.setattr(gen, "forward", guarded)


@pytest.mark.parametrize("name", E.NETS)
def test_forward_video_runs_no_stock_convolution_or_concatenation(name, monkeypatch):
    from dmcnet_amd import evaluate
    route_on(monkeypatch)
    m = dmcnet_amd.Model(51, 3, "mv", base_model="resnet18", use_databn=0, arch_estimator=E.ARCH[name])
    O.seeded_state_fill(m, 71)
    m.to(DEV).eval()
    assert isinstance(m.gen_flow_model, E.CLS[name])
    _, mv, res, _ = O.synthetic_batch(seed=72, batch=1, num_segments=3, num_class=51)
    rec = Recorder(_lib.load())
    monkeypatch.setattr(_lib, "load", lambda: rec)
    forbid_stock_ops_inside(m.gen_flow_model, monkeypatch)
    with torch.no_grad():
        on = evaluate.forward_video(m, mv.to(DEV), res.to(DEV), 3, 1)
    assert rec.launches() == ["dmc_ef_first"] + ["dmc_ef_layer"] * 4 + ["dmc_ef_head"]
    assert on.shape == (1, 51) and np.isfinite(on).all()          # (the generator's values: the golden and the fp64 cases above)


def outcome(fn):
    try:
        return fn()
    except Exception as e:                                          # what the stock modules raise on an input they do not take
        return type(e)


def same(a, b):
    return torch.equal(bits(a), bits(b)) if torch.is_tensor(a) and torch.is_tensor(b) else (a is b and isinstance(a, type))


@pytest.mark.parametrize("name", E.NETS)
def test_everything_else_is_the_stock_loop_bit_for_bit(name, monkeypatch):
    m = seeded_net(name)
    x = E.rnd(51, (2, 5, 21, 17)).to(DEV)
    rec = Recorder(_lib.load())
    monkeypatch.setattr(_lib, "load", lambda: rec)
    # the stock route must reproduce itself for a bit comparison to mean anything: MIOpen is asked for its deterministic solvers
    monkeypatch.setattr(torch.backends.cudnn, "deterministic", True)
    monkeypatch.setattr(torch.backends.cudnn, "benchmark", False)
    route_on(monkeypatch)
    monkeypatch.setattr(model, "EF_TRAIN", False)
    for train in (True, False):                                     # autograd on without DMC_EF_TRAIN: never, in train() or in eval()
        m.train(train)
        got, want = m(x), E.stock_forward(m, x)
        assert got.requires_grad and same(got, want)
    m.eval()
    monkeypatch.setattr(model, "EF_EVAL", False)                    # DMC_EF_EVAL=0
    with torch.no_grad():
        assert same(m(x), E.stock_forward(m, x))
    route_on(monkeypatch)
    cpu = E.net(name).eval()
    with torch.no_grad():
        for net_, t in ((m, x.double()), (m, x[:, :4]), (cpu, x.cpu()), (cpu, x)):         # fp64 input, 4 channels, a CPU module
            assert not ops.early_fusion_supported(net_, t)
            assert same(outcome(lambda: net_(t)), outcome(lambda: E.stock_forward(net_, t)))
    assert rec.launches() == [], rec.calls
    with torch.no_grad():
        assert ops.early_fusion_supported(m, x)
        on = m(x)
    assert len(rec.launches()) == 6
    assert rel_err(on, E.stock_forward(m, x).detach()) < 1e-5
    monkeypatch.setattr(model, "EF_EVAL_ALL", False)                # DMC_EF_EVAL unset: by class
    del rec.calls[:]
    with torch.no_grad():
        m(x)
    assert bool(rec.launches()) == m.EF_EVAL_BY_DEFAULT


# =====================================================================================================================
# 5. training
# =====================================================================================================================
def train_on(monkeypatch):
    monkeypatch.setattr(model, "EF_TRAIN", True)


def grads_of(m, x, r):
    m.zero_grad(set_to_none=True)
    out = m(x)
    (out * r).sum().backward()
    return out.detach(), [p.grad.detach().clone() for p in m.parameters()]


def check_gradients(tag, got, name, x, r, state=None):
    """The project's criterion per tensor: e <= max(4 e_ref, 2e-5 max|g|), e_ref the fp32 CPU autograd's distance from fp64."""
    _, g64 = (E.gradients(name, x, r, torch.float64) if state is None else state(torch.float64))
    _, g32 = (E.gradients(name, x, r, torch.float32) if state is None else state(torch.float32))
    for pname, g, a64, a32 in zip(E.PARAM_NAMES, got, g64, g32):
        assert g.shape == a64.shape, pname
        e = float((g.double().cpu() - a64).abs().max())
        e_ref = float((a32.double() - a64).abs().max())
        top = float(a64.abs().max())
        print("ef grad %s %s: e %.3e e_ref %.3e max|g| %.3e" % (tag, pname, e, e_ref, top))
        assert e <= max(4 * e_ref, 2e-5 * top), (pname, e, e_ref, top)


@pytest.mark.parametrize("shape", E.MAIN_SHAPES + [E.ROW_SHAPE], ids=E.sid)
@pytest.mark.parametrize("name", E.NETS)
def test_parameter_gradients_vs_fp64(name, shape, monkeypatch):
    train_on(monkeypatch)
    route_on(monkeypatch)
    m = E.net(name, DEV).train()
    x = E.rnd(31, shape)
    r = E.rnd(33, (shape[0], 2) + shape[2:])
    xd, rd = x.to(DEV), r.to(DEV)
    assert ops.early_fusion_train_supported(m, xd)
    rec = Recorder(_lib.load())
    monkeypatch.setattr(_lib, "load", lambda: rec)
    out, got = grads_of(m, xd, rd)
    assert rec.launches() == (["dmc_ef_first"] + ["dmc_ef_layer"] * 4 + ["dmc_ef_head", "dmc_ef_head_dgrad", "dmc_ef_head_wgrad"]
                              + ["dmc_ef_layer_mask", "dmc_ef_layer_wgrad", "dmc_ef_layer_dgrad"] * 4 + ["dmc_ef_first_bwd"])
    assert list(dict(m.named_parameters())) == E.PARAM_NAMES
    check_gradients("%s %s" % (name, shape), got, name, x, r)
    with torch.no_grad():
        assert torch.equal(bits(out), bits(m(xd)))                 # the forward is the eval route's, bit for bit
    out2, again = grads_of(m, xd, rd)
    assert torch.equal(bits(out), bits(out2)) and all(torch.equal(bits(a), bits(b)) for a, b in zip(got, again))      # run to run


def test_sum_follows_the_two_first_branches_separately(monkeypatch):
    """Sum with conv_0_r = -conv_0_mv on a residual that repeats the motion vectors: b = -a bit for bit, so wherever a is not 0 the
    two LeakyReLUs take opposite branches at the same place.  The sign plane says so, and the gradients of both convolutions are
    fp64's under the criterion -- one shared branch would be off by a factor of 10 at every place."""
    train_on(monkeypatch)
    shape = (3, 5, 14, 14)
    m = E.net("Sum", DEV).train()
    with torch.no_grad():
        m.conv_0_r[0].weight.zero_()
        m.conv_0_r[0].weight[:, :2] = -m.conv_0_mv[0].weight
        m.conv_0_r[0].bias.copy_(-m.conv_0_mv[0].bias)
    x = E.rnd(31, shape)
    x[:, 2:4] = x[:, :2]
    r = E.rnd(33, (3, 2, 14, 14))
    st = {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}

    def reference(dtype):
        ps = [(st[u + ".weight"].to(dtype).requires_grad_(True), st[u + ".bias"].to(dtype).requires_grad_(True)) for u in E.UNITS]
        f = E.forward(ps, x.to(dtype), False)
        if dtype == torch.float64:
            assert bool(((f["a"] > 0) != (f["b"] > 0)).all()) and bool((f["a"] != 0).all()) and bool((f["b"] != 0).all())
        return f["out"].detach(), list(torch.autograd.grad((f["out"] * r.to(dtype)).sum(), [t for pair in ps for t in pair]))

    _, signs = run_first("Sum", x.to(DEV), 32, False, ps=[(m.conv_0_mv[0].weight, m.conv_0_mv[0].bias), (m.conv_0_r[0].weight, m.conv_0_r[0].bias)])
    s = signs.to(torch.int32) & 0xFFFF
    assert bool(((s & 0xFF) ^ (s >> 8) == 0xFF).all())              # bit c and bit 8 + c differ at every place
    assert ops.early_fusion_train_supported(m, x.to(DEV))
    _, got = grads_of(m, x.to(DEV), r.to(DEV))
    check_gradients("Sum opposite", got, "Sum", x, r, state=reference)


@pytest.mark.parametrize("name", E.NETS)
def test_an_input_that_requires_a_gradient_takes_the_stock_route(name, monkeypatch):
    train_on(monkeypatch)
    m = E.net(name, DEV).train()
    x = E.rnd(31, (2, 5, 11, 9)).to(DEV).requires_grad_(True)
    assert not ops.early_fusion_train_supported(m, x) and ops.early_fusion_train_supported(m, x.detach())
    rec = Recorder(_lib.load())
    monkeypatch.setattr(_lib, "load", lambda: rec)
    monkeypatch.setattr(torch.backends.cudnn, "deterministic", True)
    monkeypatch.setattr(torch.backends.cudnn, "benchmark", False)
    out = m(x)
    assert torch.equal(bits(out), bits(E.stock_forward(m, x)))
    out.sum().backward()
    assert rec.launches() == []
    assert x.grad is not None and tuple(x.grad.shape) == tuple(x.shape) and bool(x.grad.abs().sum() > 0)


@pytest.mark.parametrize("name", E.NETS)
def test_one_adam_step_moves_every_generator_parameter(name, monkeypatch):
    from dmcnet_amd import train
    train_on(monkeypatch)
    m = dmcnet_amd.Model(51, 3, "mv", base_model="resnet18", use_databn=0, arch_estimator=E.ARCH[name])
    O.seeded_state_fill(m, 71)
    m.to(DEV).train()
    flow, mv, res, _ = O.synthetic_batch(seed=72, batch=1, num_segments=3, num_class=51)
    _, og = train.make_optimizers(m, 0.01, 1e-4, 0.01, 1.0)
    before = {k: v.detach().clone() for k, v in m.gen_flow_model.named_parameters()}
    rec = Recorder(_lib.load())
    monkeypatch.setattr(_lib, "load", lambda: rec)
    out = m(mv.to(DEV), res.to(DEV))
    gen_flow = out[1]
    loss = F.mse_loss(gen_flow, flow.to(DEV).reshape(gen_flow.shape))
    og.zero_grad()
    loss.backward()
    assert "dmc_ef_first_bwd" in rec.launches() and rec.launches().count("dmc_ef_layer_dgrad") == 4
    og.step()
    assert len(before) == 14
    for k, v in m.gen_flow_model.named_parameters():
        assert v.grad is not None and bool(torch.isfinite(v.grad).all()), k
        assert not torch.equal(v.detach(), before[k]), k
