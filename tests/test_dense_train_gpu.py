"""GPU: EstimatorDenseNet / EstimatorDenseNetSmall in training on the kernels of csrc/dense_train.hip (backward) and
csrc/dense_eval.hip (forward).

Through the C ABI unless stated otherwise; the reference side is tests/dense_ref.py (the fp64 stack with torch autograd, the buffer
builder) and tests/dense_train_ref.py (the gradients of one layer in buffer order, tap by tap, which tests/test_dense_train_cpu.py
holds against autograd).  Bars: max|err| / max|ref| < 1e-5 for a bf16x3 kernel against fp64 (tests/test_dconv_gpu.py) and
max(4 e_ref, 2e-5 max|ref|) for whole networks, e_ref = the stock fp32 stack's own distance from fp64 on the same inputs.

  1. mask pass: bitwise against where(f > 0, g, g * float32(0.1)) with +0.0, -0.0 and denormals in the feature slot; every other
     channel of G untouched; the bias sums against fp64.
  2. layer data gradient against fp64 on every channel triple at 3 x 33 x 18 and on every geometry at two triples: the result is
     the prefill plus the gradient, the slot [K, K + R) is unchanged bitwise, channels >= K + R (NaN) are still NaN.
  3. layer weight gradient against fp64 on the same grid, feat NaN from K + R on; one case beyond the 256-step range cap.
  4. exact cases (small integers: every product and partial sum exact): both gradients bit for bit; one-hot sweeps over (tap, r)
     for the data gradient and (tap, block-boundary channel) for the weight gradient.
  5. head backward against fp64; every float of a NaN-prefilled G written.
  6. whole networks through net(x) with model.DENSE_TRAIN on: output bitwise equal to ops.dense_eval, the thirteen gradients
     within the whole-network bar; frame ranges; determinism.
  7. dispatch: flag off = the stock loop bit for bit and no entry point of dense_train.hip; flag on = no stock convolution,
     concatenation or LeakyReLU in the generator, forward or backward; the environment flag; no_grad keeps the eval route; one
     Model forward + backward at 224 x 224.
  8. every new launching entry point in a guarded arena (tests/abi_arena.py), G and feat as in/out buffers, workspaces of exactly
     the queried size.

Measured on an MI355X: see MEASURED below (records, not bars)."""
import copy
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import dmcnet_amd
from dmcnet_amd import _lib, model, ops
from oracle import dmc_oracle as O
from tests import abi_cases
from tests import dense_ref as D
from tests import dense_train_ref as TR
from tests.abi_arena import run_case

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U8 = torch.uint8
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
#: printed on an MI355X: (smallest, largest) max|err| / max|ref| over the cases of a group (bar 1e-5), and the largest e / bar of
#: the whole-network gradients (bar max(4 e_ref, 2e-5 max|ref|))
MEASURED = {"dgrad": (1.6e-7, 1.3e-6), "wgrad": (8.3e-8, 3.4e-7), "wgrad-beyond-cap": 2.5e-6, "mask-bias": (0.0, 2.8e-7), "head-G": (3.3e-8, 2.1e-7),
            "head-dW": (1.1e-8, 2.7e-7), "head-db": (0.0, 3.1e-7), "DenseNet": 0.11, "DenseNetSmall": 0.04, "model-224-on-vs-off": (1.25e-6, 1.10)}

GEOMS = [(1, 1, 1), (1, 1, 37), (1, 29, 1), (2, 5, 7), (1, 16, 16), (1, 1, 257), (3, 33, 18)]
TRIPLES = [(464, 432, 32), (464, 368, 64), (464, 272, 96), (464, 144, 128), (464, 16, 128), (176, 144, 32), (176, 16, 32), (560, 432, 128)]
GRID = [GEOMS[-1] + t for t in TRIPLES] + [g + t for g in GEOMS[:-1] for t in ((464, 272, 96), (176, 144, 32))]
GRID_IDS = ["-".join(map(str, s)) for s in GRID]
EXACT = [(560, 432, 128), (464, 432, 32), (176, 144, 32)]
EXACT_IDS = ["-".join(map(str, s)) for s in EXACT]
CLS = {"DenseNet": model.EstimatorDenseNet, "DenseNetSmall": model.EstimatorDenseNetSmall}


def P(t):
    return _lib.ptr(t)


def ok(rc, what):
    _lib.check(rc, what)


def rs(seed):
    return np.random.RandomState(seed)


def rel_err(a, b):
    a, b = a.detach().double().cpu(), torch.as_tensor(b).detach().double().cpu()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))


def bits(t):
    return t.detach().contiguous().view(torch.int32)


def ff_buffer(shape):
    """A device fp32 tensor whose every byte is 0xFF (NaN)."""
    n = int(np.prod(shape))
    return torch.full((4 * n,), 0xFF, dtype=U8, device=DEV).view(torch.float32).view(shape)


def ff_bytes(nbytes):
    return torch.full((max(int(nbytes), 1),), 0xFF, dtype=U8, device=DEV)


# ---------------------------------------------------------------- launches
def run_mask(feat, G, k, r):
    lib = _lib.load()
    n, h, w, ct = G.shape
    db = ff_buffer((r,))
    work = ff_bytes(lib.dmc_densetrain_mask_workspace_bytes(n, h, w, r))
    ok(lib.dmc_densetrain_mask(P(feat), P(G), P(db), P(work), n, h, w, ct, k, r, ops._stream()), "dmc_densetrain_mask")
    return db


def run_dgrad(G, wb, k, r):
    """The layer's data gradient in place, block by block, on the packs the route itself builds (ops._dense_dgrad_packs)."""
    lib = _lib.load()
    n, h, w, ct = G.shape
    assert tuple(wb.shape) == (r, 3, 3, k)
    for c0, cb, pack in ops._dense_dgrad_packs(wb.contiguous().to(DEV), k, r):
        ok(lib.dmc_densetrain_layer_dgrad(P(G), P(pack), n, h, w, ct, k, r, c0, cb, ops._stream()), "dmc_densetrain_layer_dgrad")
    return G


def run_wgrad(feat, G, k, r):
    lib = _lib.load()
    n, h, w, ct = G.shape
    dw = ff_buffer((r, 3, 3, k))
    work = ff_bytes(lib.dmc_densetrain_wgrad_workspace_bytes(n, h, w, k, r))
    ok(lib.dmc_densetrain_layer_wgrad(P(feat), P(G), P(dw), P(work), n, h, w, ct, k, r, ops._stream()), "dmc_densetrain_layer_wgrad")
    return dw


def run_head(dout, feat, wb):
    lib = _lib.load()
    n, h, w, ct = feat.shape
    G, dw, db = ff_buffer((n, h, w, ct)), ff_buffer((2, 3, 3, ct)), ff_buffer((2,))
    ok(lib.dmc_densetrain_head_dgrad(P(dout), P(wb), P(G), n, h, w, ct, ops._stream()), "dmc_densetrain_head_dgrad")
    work = ff_bytes(lib.dmc_densetrain_head_workspace_bytes(n, h, w, ct))
    ok(lib.dmc_densetrain_head_wgrad(P(dout), P(feat), P(dw), P(db), P(work), n, h, w, ct, ops._stream()), "dmc_densetrain_head_wgrad")
    return G, dw, db


# ---------------------------------------------------------------- one layer's operands and fp64 gradients
@functools.lru_cache(maxsize=None)
def layer_case(n, h, w, ct, k, r, ints=False):
    """(feat [N, H, W, CT], G [N, H, W, CT], weight OHWI [R, 3, 3, K], fp64 data gradient [N, H, W, K], fp64 weight gradient
    [R, 3, 3, K]) on the CPU.  feat: activations in [0, K + R), NaN behind; G: a known prefill in [0, K), the slot's gradient dz in
    [K, K + R), NaN behind.  ``ints``: every operand a small integer, |v| <= 4.  Computed once per shape, never modified."""
    r_ = rs(1000 + 131 * n + 17 * h + 7 * w + k + r)
    if ints:
        draw = lambda shape, scale=1.0: r_.randint(-4, 5, size=shape).astype(np.float32)
    else:
        draw = lambda shape, scale=1.0: (r_.standard_normal(shape) * scale).astype(np.float32)
    feat = torch.full((n, h, w, ct), float("nan"))
    G = torch.full((n, h, w, ct), float("nan"))
    feat[..., :k + r] = torch.from_numpy(draw((n, h, w, k + r)))
    G[..., :k] = torch.from_numpy(draw((n, h, w, k), 0.5))
    G[..., k:k + r] = torch.from_numpy(draw((n, h, w, r)))
    wb = torch.from_numpy(draw((r, 3, 3, k), 1.4 / np.sqrt(9.0 * k)))
    dz = G[..., k:k + r].double()
    return feat, G, wb, TR.dgrad(dz, wb.double()), TR.wgrad(dz, feat[..., :k].double())


# =====================================================================================================================
# 1. mask pass
# =====================================================================================================================
MASK_SHAPES = [(3, 33, 18, 464, 432, 32), (3, 33, 18, 464, 272, 96), (3, 33, 18, 464, 16, 128), (3, 33, 18, 176, 144, 32), (2, 5, 7, 464, 368, 64),
               (1, 1, 1, 176, 16, 32)]


@pytest.mark.parametrize("shape", MASK_SHAPES, ids=["-".join(map(str, s)) for s in MASK_SHAPES])
def test_mask_pass_bitwise_and_bias_sums(shape):
    n, h, w, ct, k, r = shape
    r_ = rs(1100 + k + r)
    special = np.array([0.0, -0.0, 1e-40, -1e-40, 1.4e-45, -1.4e-45, 1.0, -1.0], np.float32)
    assert (special[2:6] != 0).all() and (np.abs(special[2:6]) < np.finfo(np.float32).tiny).all()     # denormals of both signs
    f = r_.standard_normal((n, h, w, ct)).astype(np.float32)
    pick = r_.randint(0, 3 * len(special), size=(n, h, w, r))
    slot = np.where(pick < len(special), special[pick % len(special)], f[..., k:k + r])
    flat = slot.reshape(-1)
    flat[:min(flat.size, len(special))] = special[:min(flat.size, len(special))]       # every special value at least once
    f[..., k:k + r] = slot
    g = r_.standard_normal((n, h, w, ct)).astype(np.float32)
    want = g.copy()
    want[..., k:k + r] = TR.mask(f[..., k:k + r], g[..., k:k + r])
    feat, G = torch.from_numpy(f).to(DEV), torch.from_numpy(g).to(DEV)
    db = run_mask(feat, G, k, r)
    assert torch.equal(bits(G), bits(torch.from_numpy(want)).to(DEV)), "%d values differ" % int((bits(G).cpu() != bits(torch.from_numpy(want))).sum())
    assert torch.equal(bits(feat), bits(torch.from_numpy(f)).to(DEV))                # feat is read only
    ref = want[..., k:k + r].astype(np.float64).reshape(-1, r).sum(0)
    e = rel_err(db, ref)
    print("dense mask %s: bias rel_err %.3e" % (shape, e))
    assert e < 1e-5, e
    G2 = torch.from_numpy(g).to(DEV)
    assert torch.equal(bits(run_mask(feat, G2, k, r)), bits(db)) and torch.equal(bits(G2), bits(G))          # run to run


# =====================================================================================================================
# 2. layer data gradient against fp64
# =====================================================================================================================
@pytest.mark.parametrize("shape", GRID, ids=GRID_IDS)
def test_layer_data_gradient_vs_fp64(shape):
    n, h, w, ct, k, r = shape
    assert _lib.load().dmc_densetrain_supported(*shape) == 1
    _, G0, wb, dg, _ = layer_case(*shape)
    G = G0.to(DEV)
    run_dgrad(G, wb, k, r)
    want = G0[..., :k].double() + dg                               # the prefill plus the gradient
    e = float((G[..., :k].double().cpu() - want).abs().max() / dg.abs().max().clamp_min(1e-30))
    print("dense dgrad %s: rel_err %.3e" % (shape, e))
    assert not bool(torch.isnan(G[..., :k]).any())
    assert e < 1e-5, e
    assert torch.equal(bits(G[..., k:k + r]), bits(G0[..., k:k + r]).to(DEV))        # the slot: read, never written
    assert bool(torch.isnan(G[..., k + r:]).all()) and torch.equal(bits(G[..., k + r:]), bits(G0[..., k + r:]).to(DEV))
    again = run_dgrad(G0.to(DEV), wb, k, r)
    assert torch.equal(bits(again), bits(G))                       # run to run


# =====================================================================================================================
# 3. layer weight gradient against fp64
# =====================================================================================================================
@pytest.mark.parametrize("shape", GRID, ids=GRID_IDS)
def test_layer_weight_gradient_vs_fp64(shape):
    n, h, w, ct, k, r = shape
    feat0, G0, _, _, dwref = layer_case(*shape)
    assert bool(torch.isnan(feat0[..., k + r:]).all())             # nothing past the slots in use may reach a live column
    feat, G = feat0.to(DEV), G0.to(DEV)
    dw = run_wgrad(feat, G, k, r)
    e = rel_err(dw, dwref)
    print("dense wgrad %s: rel_err %.3e" % (shape, e))
    assert not bool(torch.isnan(dw).any())
    assert e < 1e-5, e
    assert torch.equal(bits(feat), bits(feat0).to(DEV)) and torch.equal(bits(G), bits(G0).to(DEV))       # both read only
    assert torch.equal(bits(run_wgrad(feat, G, k, r)), bits(dw))   # run to run


def test_weight_gradient_beyond_the_range_cap():
    """11 x 224 x 224 with (CT, K, R) = (48, 16, 32): 17248 steps of 32 pixels are more than 64 ranges of 256 steps, so the cap
    binds (68 ranges of at most 8 k pixels).  The fp64 reference is computed on the device."""
    n, h, w, ct, k, r = 11, 224, 224, 48, 16, 32
    lib = _lib.load()
    assert n * h * w > 64 * 256 * 32 and lib.dmc_densetrain_wgrad_workspace_bytes(n, h, w, k, r) == 68 * r * 9 * k * 4
    g = torch.Generator(device=DEV).manual_seed(79)
    feat = torch.randn((n, h, w, ct), generator=g, device=DEV)
    G = torch.randn((n, h, w, ct), generator=g, device=DEV)
    dw = run_wgrad(feat, G, k, r)
    ref = TR.wgrad(G[..., k:].double(), feat[..., :k].double())
    e = rel_err(dw, ref)
    print("dense wgrad beyond the cap: rel_err %.3e" % e)
    assert e < 1e-5, e


# =====================================================================================================================
# 4. exact cases
# =====================================================================================================================
EXACT_FRAME = (2, 9, 11)


def boundary_channels(k):
    return sorted({0, 15, 16, 127, 128, k - 17, k - 16, k - 1} & set(range(k)))


@pytest.mark.parametrize("ct,k,r", EXACT, ids=EXACT_IDS)
def test_small_integers_give_both_gradients_bit_for_bit(ct, k, r):
    """|dz|, |w|, |feat|, |prefill| <= 4 on 198 pixels: every product, every partial sum (at most 9 * 128 * 16 in the data gradient,
    198 * 16 in the weight gradient) and every bf16 slice split is exact, whatever the order."""
    n, h, w = EXACT_FRAME
    feat0, G0, wb, dg, dwref = layer_case(n, h, w, ct, k, r, True)
    assert float(dg.abs().max()) < 2 ** 24 and float(dwref.abs().max()) < 2 ** 24 and float(dg.abs().max()) > 0
    feat, G = feat0.to(DEV), G0.to(DEV)
    dw = run_wgrad(feat, G, k, r)
    want = dwref.float()
    assert torch.equal(want.double(), dwref)
    assert torch.equal(bits(dw), bits(want).to(DEV)), "wgrad: %d of %d values differ" % (int((dw.cpu() != want).sum()), want.numel())
    run_dgrad(G, wb, k, r)
    want = (G0[..., :k].double() + dg).float()
    assert torch.equal(bits(G[..., :k]), bits(want).to(DEV)), "dgrad: %d of %d values differ" % (int((G[..., :k].cpu() != want).sum()), want.numel())


@pytest.mark.parametrize("ct,k,r", EXACT, ids=EXACT_IDS)
def test_data_gradient_one_hot_sweep_over_tap_and_r(ct, k, r):
    """Per tap one launch: w[r][tap][c_r] = +-1 / +-2 with distinct c_r and nothing else.  Then G[m][c_r] = dz[m - o(tap)][r] times
    that value, exactly, zero where the tap leaves the frame, and every other channel below K stays at its (zero) prefill: each
    (tap, r) shows in exactly one output channel.  A mirrored tap, a transposed pack or a wrong block offset shows here."""
    n, h, w = 1, 7, 9
    r_ = rs(1400 + k + r)
    dz = r_.randint(-4, 5, size=(n, h, w, r)).astype(np.float32)
    dz[dz == 0] = 3.0                                              # (every position visible)
    bnd = boundary_channels(k)
    for tap in range(9):
        perm = r_.permutation(k)
        if tap % 3 == 0:                                           # the block-boundary channels among the targets
            perm = np.array(bnd + [c for c in perm.tolist() if c not in bnd])
        cs = perm[:r]
        assert len(set(cs.tolist())) == r
        vals = (r_.choice([1.0, 2.0], size=len(cs)) * r_.choice([-1.0, 1.0], size=len(cs))).astype(np.float32)
        wb = np.zeros((r, 3, 3, k), np.float32)
        wb[np.arange(len(cs)), tap // 3, tap % 3, cs] = vals
        G0 = torch.full((n, h, w, ct), float("nan"))
        G0[..., :k] = 0
        G0[..., k:k + r] = torch.from_numpy(dz)
        G = run_dgrad(G0.to(DEV), torch.from_numpy(wb), k, r).cpu().numpy()
        want = np.zeros((n, h, w, k), np.float32)
        shifted = TR.shift(torch.from_numpy(dz), -(tap // 3 - 1), -(tap % 3 - 1)).numpy()
        for i, c in enumerate(cs):
            want[..., c] = shifted[..., i] * vals[i]
        assert np.array_equal(G[..., :k], want), "tap %d: %d values differ" % (tap, int((G[..., :k] != want).sum()))
        assert int((G[..., :k] != 0).any(axis=(0, 1, 2)).sum()) == r       # each (tap, r) in exactly one channel


@pytest.mark.parametrize("ct,k,r", EXACT, ids=EXACT_IDS)
def test_weight_gradient_one_hot_sweep_over_tap_and_block_boundaries(ct, k, r):
    """dz lives at one pixel p and one channel r0, feat at the pixel p + o(tap) in the block-boundary channels: dW has exactly
    those entries [r0][tap][c], with the products as values, and zeros everywhere else."""
    n, h, w = 1, 5, 6
    py, px = 2, 3
    cs = boundary_channels(k)
    assert {0, 15, 16, 127, 128, k - 17, k - 16, k - 1} == set(cs)
    for tap in range(9):
        r0 = (7 * tap + 3) % r
        feat0 = torch.full((n, h, w, ct), float("nan"))
        feat0[..., :k + r] = 0
        G0 = torch.full((n, h, w, ct), float("nan"))
        G0[..., :k + r] = 0
        G0[0, py, px, k + r0] = 2.0
        vals = np.arange(1, len(cs) + 1, dtype=np.float32) * np.where(np.arange(len(cs)) % 2, -1.0, 1.0).astype(np.float32)
        feat0[0, py + tap // 3 - 1, px + tap % 3 - 1, cs] = torch.from_numpy(vals)
        dw = run_wgrad(feat0.to(DEV), G0.to(DEV), k, r).cpu().numpy()
        want = np.zeros((r, 3, 3, k), np.float32)
        want[r0, tap // 3, tap % 3, cs] = 2.0 * vals
        assert np.array_equal(dw, want), "tap %d: %d values differ, %d nonzero (want %d)" % (tap, int((dw != want).sum()), int((dw != 0).sum()), len(cs))


# =====================================================================================================================
# 5. head backward
# =====================================================================================================================
HEAD_SHAPES = [(3, 19, 37), (2, 5, 7), (1, 1, 1)]


@functools.lru_cache(maxsize=None)
def head_case(ct, shape):
    """(full buffer [N, H, W, CT], head weight [2, 3, 3, CT] in buffer order, dout [N, 2, H, W], fp64 G, dW, db)."""
    name = D.net_of_ct(ct)
    lay = D.layout(name)
    ps = D.params(name)
    n, h, w = shape
    x = D.rnd(D.SEED + 2, (n, 5, h, w))
    _, ys, _ = D.stack(ps, x)
    buf = D.to_buffer(lay, x, [y.float() for y in ys])
    k, _, index = lay["head"]
    wb, _ = D.buffer_weight(ps[-1][0], ps[-1][1], k, 2, index)
    dout = D.rnd(D.SEED + 3, (n, 2, h, w))
    dz = dout.permute(0, 2, 3, 1).double()
    return buf, wb, dout, TR.dgrad(dz, wb.double()), TR.wgrad(dz, buf.double()), dz.reshape(-1, 2).sum(0)


@pytest.mark.parametrize("shape", HEAD_SHAPES, ids=["3-19-37", "2-5-7", "1-1-1"])
@pytest.mark.parametrize("ct", [464, 176])
def test_head_backward_vs_fp64(ct, shape):
    assert _lib.load().dmc_densetrain_supported(*shape, ct, ct, 2) == 1
    buf, wb, dout, gref, dwref, dbref = head_case(ct, shape)
    feat, wg, dg = buf.to(DEV), wb.to(DEV), dout.to(DEV)
    G, dw, db = run_head(dg, feat, wg)
    assert not bool(torch.isnan(G).any()) and not bool(torch.isnan(dw).any()) and not bool(torch.isnan(db).any())     # every float written
    eg, ew, eb = rel_err(G, gref), rel_err(dw, dwref), rel_err(db, dbref)
    print("dense head backward CT %d %s: G %.3e dW %.3e db %.3e" % (ct, shape, eg, ew, eb))
    assert eg < 1e-5 and ew < 1e-5 and eb < 1e-5, (eg, ew, eb)
    index = D.layout(D.net_of_ct(ct))["head"][2]
    assert not bool(G[..., index < 0].any())                       # pad channels: zero weights, zero gradient
    assert torch.equal(bits(feat), bits(buf).to(DEV))
    G2, dw2, db2 = run_head(dg, feat, wg)
    assert torch.equal(bits(G2), bits(G)) and torch.equal(bits(dw2), bits(dw)) and torch.equal(bits(db2), bits(db))


def test_export_writes_the_five_live_channels():
    n, h, w, ct = 2, 5, 7, 176
    G = D.rnd(61, (n, h, w, ct)).to(DEV)
    dx = ff_buffer((n, 5, h, w))
    ok(_lib.load().dmc_densetrain_export(P(G), P(dx), n, h, w, ct, ops._stream()), "dmc_densetrain_export")
    assert torch.equal(bits(dx), bits(G[..., :5].permute(0, 3, 1, 2)))


# =====================================================================================================================
# 6. whole networks, through net(x)
# =====================================================================================================================
NET_SHAPES = [(1, 5, 20, 37), (3, 5, 33, 18), (3, 5, 14, 14)]
NET_IDS = ["20x37", "33x18", "14x14"]
#: (network, input shape) -> the seed of x: see net_input
NET_SEEDS = {("DenseNet", (1, 5, 20, 37)): 33, ("DenseNet", (3, 5, 33, 18)): 117, ("DenseNet", (3, 5, 14, 14)): 32, ("DenseNet", (2, 5, 21, 17)): 40,
             ("DenseNetSmall", (1, 5, 20, 37)): 31, ("DenseNetSmall", (3, 5, 33, 18)): 31, ("DenseNetSmall", (3, 5, 14, 14)): 32,
             ("DenseNetSmall", (2, 5, 21, 17)): 32}
NAMES = ["w0", "b0", "w1", "b1", "w2", "b2", "w3", "b3", "w4", "b4", "w_head", "b_head", "x"]


def train_on(monkeypatch):
    monkeypatch.setattr(model, "DENSE_TRAIN", True)


def fresh_net(name):
    return D.load_into(CLS[name](), name).to(DEV).train()


def parameters_in_order(net):
    out = []
    for i in range(net.depth):
        conv = getattr(net, "conv_%d" % i)[0]
        out += [conv.weight, conv.bias]
    return out + [net.predict_flow.weight, net.predict_flow.bias]


@functools.lru_cache(maxsize=None)
def net_input(name, shape):
    """x = D.rnd(seed, shape) for the first seed from 31 on (NET_SEEDS, found by a search on the CPU; the condition is asserted here) at which NO pre-activation of the fp64 stack lies within 4 e_ref of zero,
    e_ref = the largest distance of the stock fp32 stack's pre-activations of that layer from fp64.  The gradient of a LeakyReLU
    jumps by 0.9 g where its argument crosses zero, so a gradient can be held to a tolerance only on inputs where every route that
    meets the forward bar (4 e_ref) takes the branches fp64 takes; at seed 31, 3 x 14 x 14, EstimatorDenseNet has pre-activations
    of 1.2e-6 and 1.05e-6 in layers 3 and 4 under an e_ref of 2.2e-6, the stock fp32 stack itself takes the other branch at one of
    them and its w_0 gradient is then 3.8e-2 off.  Decided by the two references alone, never by a kernel's result."""
    seed = NET_SEEDS[name, shape]
    ps = D.params(name)
    x = D.rnd(seed, shape)
    p64, p32 = D.stack(ps, x)[0], D.stack(ps, x, dtype=torch.float32)[0]
    for k, (a, b) in enumerate(zip(p64, p32)):
        assert float(a.abs().min()) > 4 * float((b.double() - a).abs().max()), (name, shape, seed, k)
    return x


@functools.lru_cache(maxsize=None)
def net_reference(name, shape):
    """(x, r, fp64 gradients of the twelve parameters and of x, the stock fp32 stack's) for the loss sum(out * r); computed once."""
    x = net_input(name, shape)
    r = D.rnd(32, (shape[0], 2) + tuple(shape[2:]))
    _, g64, dx64 = TR.network_grads(name, x, r, torch.float64)
    _, g32, dx32 = TR.network_grads(name, x, r, torch.float32)
    return x, r, g64 + [dx64], g32 + [dx32]


def step(net, x, r, x_grad=True):
    """One forward + backward of ``net`` on the device; (out, the thirteen gradients -- x's None without x_grad)."""
    net.zero_grad(set_to_none=True)
    xg = x.to(DEV).requires_grad_(x_grad)
    out = net(xg)
    (out * r.to(DEV)).sum().backward()
    return out.detach(), [p.grad for p in parameters_in_order(net)] + [xg.grad]


def hold_to_bar(what, got, g64, g32):
    for name, a, b, c in zip(NAMES, got, g64, g32):
        e = float((a.double().cpu() - b).abs().max())
        e_ref = float((c.double() - b).abs().max())
        top = float(b.abs().max())
        print("dense train %s %s: e %.3e e_ref %.3e max|ref| %.3e" % (what, name, e, e_ref, top))
        assert tuple(a.shape) == tuple(b.shape) and e <= max(4 * e_ref, 2e-5 * top), (what, name, e, e_ref, top)


@pytest.mark.parametrize("shape", NET_SHAPES, ids=NET_IDS)
@pytest.mark.parametrize("name", ["DenseNet", "DenseNetSmall"])
def test_whole_network_gradients_vs_fp64(name, shape, monkeypatch):
    train_on(monkeypatch)
    net = fresh_net(name)
    x, r, g64, g32 = net_reference(name, shape)
    assert ops.dense_train_supported(net, x.to(DEV))
    out, grads = step(net, x, r)
    with torch.no_grad():
        assert torch.equal(bits(out), bits(ops.dense_eval(net, x.to(DEV))))          # the forward IS the eval route's launches
    hold_to_bar("%s %s" % (name, shape), grads, g64, g32)
    out2, grads2 = step(net, x, r)                                 # determinism: bitwise, every gradient
    assert torch.equal(bits(out2), bits(out))
    for what, a, b in zip(NAMES, grads, grads2):
        assert torch.equal(bits(a), bits(b)), what


@pytest.mark.parametrize("name", ["DenseNet", "DenseNetSmall"])
def test_frame_ranges(name, monkeypatch):
    """3 frames as 3 ranges: output and dx bitwise equal to the one-range run (frames are independent); the parameter gradients, whose
    three per-range parts are added in range order, within the fp64 bar."""
    train_on(monkeypatch)
    net = fresh_net(name)
    shape = NET_SHAPES[1]
    x, r, g64, g32 = net_reference(name, shape)
    ct = D.EXPECTED[name][2]
    assert ops._dense_train_chunks(3, 33, 18, ct) == [(0, 3)]
    one_out, one = step(net, x, r)
    monkeypatch.setattr(ops, "DENSE_TRAIN_BUDGET", 33 * 18 * ct * 4)
    assert ops._dense_train_chunks(3, 33, 18, ct) == [(0, 1), (1, 2), (2, 3)]
    many_out, many = step(net, x, r)
    assert torch.equal(bits(many_out), bits(one_out)) and torch.equal(bits(many[-1]), bits(one[-1]))
    hold_to_bar("%s in 3 ranges" % name, many, g64, g32)


# =====================================================================================================================
# 7. dispatch
# =====================================================================================================================
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


def forbid_stock_ops_inside(gen, monkeypatch):
    """F.conv2d, torch.cat, Tensor.cat and the LeakyReLUs raise while ``gen.forward`` runs."""
    inner = gen.forward

    def boom(*a, **kw):
        raise AssertionError("a stock convolution, concatenation or LeakyReLU ran inside the generator")

    def guarded(x):
        with pytest.MonkeyPatch.context() as mp:
            mp.setattr(torch.nn.functional, "conv2d", boom)
            mp.setattr(torch.nn.functional, "leaky_relu", boom)
            mp.setattr(torch, "cat", boom)
            mp.setattr(torch.Tensor, "cat", boom, raising=False)
            return inner(x)
    monkeypatch.setattr(gen, "forward", guarded)


def backward_nodes(t):
    """Names of every node of the autograd graph behind ``t``."""
    seen, todo, names = set(), [t.grad_fn], []
    while todo:
        f = todo.pop()
        if f is None or f in seen:
            continue
        seen.add(f)
        names.append(type(f).__name__)
        todo += [g for g, _ in f.next_functions]
    return names


@pytest.mark.parametrize("name", ["DenseNet", "DenseNetSmall"])
def test_flag_off_is_the_stock_loop_and_flag_on_runs_no_stock_op(name, monkeypatch):
    net = fresh_net(name)
    x, r = net_input(name, (2, 5, 21, 17)), D.rnd(52, (2, 2, 21, 17))
    rec = Recorder(_lib.load())
    monkeypatch.setattr(_lib, "load", lambda: rec)
    monkeypatch.setattr(torch.backends.cudnn, "deterministic", True)
    monkeypatch.setattr(torch.backends.cudnn, "benchmark", False)
    assert model.DENSE_TRAIN is False or os.environ.get("DMC_DENSE_TRAIN") == "1"
    monkeypatch.setattr(model, "DENSE_TRAIN", False)               # the default
    off, off_grads = step(net, x, r)
    assert torch.equal(bits(off), bits(D.stock_forward(net, x.to(DEV))))
    assert not any(c.startswith("dmc_densetrain_") or c.startswith("dmc_dense_") for c in rec.calls), rec.calls
    train_on(monkeypatch)
    forbid_stock_ops_inside(net, monkeypatch)
    xg = x.to(DEV).requires_grad_(True)
    out = net(xg)
    nodes = backward_nodes(out)
    assert "_DenseTrainBackward" in nodes, nodes
    assert not any(("Convolution" in n) or ("Cat" in n) or ("LeakyRelu" in n) for n in nodes), nodes
    assert set(nodes) <= {"_DenseTrainBackward", "AccumulateGrad"}, nodes
    net.zero_grad(set_to_none=True)
    del rec.calls[:]
    (out * r.to(DEV)).sum().backward()
    blocks = sum(len(ops._dense_dgrad_blocks(k)) for k in D.EXPECTED[name][0])
    assert rec.calls.count("dmc_densetrain_head_dgrad") == 1 and rec.calls.count("dmc_densetrain_head_wgrad") == 1
    assert rec.calls.count("dmc_densetrain_mask") == 5 and rec.calls.count("dmc_densetrain_layer_wgrad") == 5
    assert rec.calls.count("dmc_densetrain_layer_dgrad") == blocks and rec.calls.count("dmc_densetrain_export") == 1
    for what, a, b in zip(NAMES, [p.grad for p in parameters_in_order(net)] + [xg.grad], off_grads):
        assert rel_err(a, b) < 1e-4, what                          # (the fp64 bars: section 6; here only that nothing is misplaced)
    # an input that needs no gradient: layer 0's data gradient and the export are not launched
    del rec.calls[:]
    net.zero_grad(set_to_none=True)
    xn = x.to(DEV)
    (net(xn) * r.to(DEV)).sum().backward()
    assert xn.grad is None and rec.calls.count("dmc_densetrain_export") == 0
    assert rec.calls.count("dmc_densetrain_layer_dgrad") == blocks - len(ops._dense_dgrad_blocks(16))
    # torch.no_grad() with the flag on: the eval route
    del rec.calls[:]
    monkeypatch.setattr(model, "DENSE_EVAL", True)
    monkeypatch.setattr(model, "DENSE_EVAL_ALL", True)
    with torch.no_grad():
        y = net(xn)
    assert not y.requires_grad and rec.calls.count("dmc_dense_layer_eval") == 5
    assert not any(c.startswith("dmc_densetrain_") for c in rec.calls), rec.calls
    assert torch.equal(bits(y), bits(out))


def test_refused_networks_raise_and_fall_back_to_the_stock_loop(monkeypatch):
    train_on(monkeypatch)
    x = D.rnd(53, (1, 5, 9, 9)).to(DEV)
    good = CLS["DenseNetSmall"]().to(DEV)
    assert ops.dense_train_supported(good, x)
    bad = CLS["DenseNetSmall"]()
    bad.conv_2[1] = torch.nn.LeakyReLU(0.2)
    bad.to(DEV)
    tiny = model.EstimatorDenseNetTiny().to(DEV)
    for net in (bad, tiny, CLS["DenseNetSmall"]()):                # a wrong slope, Tiny, CPU parameters
        assert not ops.dense_train_supported(net, x)
        with pytest.raises(_lib.DmcHipError):
            ops.dense_train(net, x)
    assert torch.equal(bad(x), D.stock_forward(bad, x))


CHILD = """
import sys
sys.path.insert(0, %r)
import torch
from dmcnet_amd import model, ops
from tests import dense_ref as D
net = D.load_into(model.EstimatorDenseNetSmall(), "DenseNetSmall").to("cuda:0")
x = D.rnd(53, (2, 5, 13, 11)).to("cuda:0")
calls = []
real = ops.dense_train
ops.dense_train = lambda n, t: (calls.append(1), real(n, t))[1]
out = net(x)
out.sum().backward()
print("RESULT", int(model.DENSE_TRAIN), len(calls), int(all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in net.parameters())))
"""


def test_environment_flag_on_in_a_fresh_process():
    """DMC_DENSE_TRAIN is read once, at import: a fresh child process with DMC_DENSE_TRAIN=1 takes the route."""
    env = dict(os.environ)
    env["DMC_DENSE_TRAIN"] = "1"
    out = subprocess.run([sys.executable, "-c", CHILD % ROOT], env=env, stdout=subprocess.PIPE, check=True, universal_newlines=True, timeout=300).stdout
    line = [ln for ln in out.splitlines() if ln.startswith("RESULT")][-1]
    assert line.split()[1:] == ["1", "1", "1"], out


def test_model_forward_and_backward_at_224(monkeypatch):
    """One Model(arch_estimator="DenseNet") step at 1 clip x 1 segment x 224 x 224 through Model.forward: every gen_flow_model
    parameter gets a finite gradient; gen_flow equals the flag-off run within 2e-5 max|ref| -- the second term of the whole-network
    bar alone (the first, 4 e_ref, would need an fp64 run of this size and could only widen the bar)."""
    m = dmcnet_amd.Model(51, 1, "mv", base_model="resnet18", use_databn=0, arch_estimator="DenseNet")
    O.seeded_state_fill(m, 71)
    m.to(DEV).train()
    assert isinstance(m.gen_flow_model, CLS["DenseNet"])
    _, mv, res, _ = O.synthetic_batch(seed=72, batch=1, num_segments=1, num_class=51)
    mv, res = mv.to(DEV), res.to(DEV)
    r = D.rnd(73, (1, 2, 224, 224)).to(DEV)
    monkeypatch.setattr(model, "DENSE_TRAIN", False)
    off = copy.deepcopy(m)(mv, res)[1].detach()
    train_on(monkeypatch)
    rec = Recorder(_lib.load())
    monkeypatch.setattr(_lib, "load", lambda: rec)
    forbid_stock_ops_inside(m.gen_flow_model, monkeypatch)
    base_out, gen_flow = m(mv, res)
    assert rec.calls.count("dmc_dense_layer_eval") == 5
    ((gen_flow * r).sum() + base_out.sum()).backward()
    assert rec.calls.count("dmc_densetrain_layer_wgrad") == 5
    for name, p in m.gen_flow_model.named_parameters():
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()) and bool(p.grad.any()), name
    e, top = float((gen_flow.detach() - off).abs().max()), float(off.abs().max())
    print("dense train Model 224: |on - off| %.3e max|off| %.3e" % (e, top))
    assert tuple(gen_flow.shape) == (1, 2, 224, 224) and bool(torch.isfinite(base_out).all())
    assert e <= 2e-5 * top, (e, top)


# =====================================================================================================================
# 8. the memory contract
# =====================================================================================================================
ARENA_LAYER = (2, 5, 7, 176, 144, 32)
ARENA_HEAD = (176, (2, 5, 7))


def mask_arena_case(a):
    n, h, w, ct, k, r = ARENA_LAYER
    feat, G, _, _, _ = layer_case(*ARENA_LAYER)
    lib = _lib.load()
    a.call("dmc_densetrain_mask", a.inp("feat", feat, nan_ok=True), a.inout("G", G, nan_ok=True), a.out("db", (r,)),
           a.work("workspace", lib.dmc_densetrain_mask_workspace_bytes(n, h, w, r)), n, h, w, ct, k, r)


def _mask_check(bufs):
    n, h, w, ct, k, r = ARENA_LAYER
    feat, G, _, _, _ = layer_case(*ARENA_LAYER)
    want = TR.mask(feat[..., k:k + r].numpy(), G[..., k:k + r].numpy())
    got = bufs["G"].t
    assert torch.equal(bits(got[..., k:k + r]), bits(torch.from_numpy(want)).to(got.device))
    assert torch.equal(bits(got[..., :k]), bits(G[..., :k]).to(got.device)) and torch.equal(bits(got[..., k + r:]), bits(G[..., k + r:]).to(got.device))
    assert rel_err(bufs["db"].t, want.astype(np.float64).reshape(-1, r).sum(0)) < 1e-5


def wgrad_arena_case(a):
    n, h, w, ct, k, r = ARENA_LAYER
    feat, G, _, _, _ = layer_case(*ARENA_LAYER)
    lib = _lib.load()
    a.call("dmc_densetrain_layer_wgrad", a.inp("feat", feat, nan_ok=True), a.inp("G", G, nan_ok=True), a.out("dw", (r, 3, 3, k)),
           a.work("workspace", lib.dmc_densetrain_wgrad_workspace_bytes(n, h, w, k, r)), n, h, w, ct, k, r)


def _wgrad_check(bufs):
    assert rel_err(bufs["dw"].t, layer_case(*ARENA_LAYER)[4]) < 1e-5


def dgrad_arena_case(a):
    n, h, w, ct, k, r = ARENA_LAYER
    _, G, wb, _, _ = layer_case(*ARENA_LAYER)
    lib = _lib.load()
    g = a.inout("G", G, nan_ok=True)
    for c0, cb in ops._dense_dgrad_blocks(k):
        blk = torch.zeros((r, 3, 3, cb))
        live = min(cb, k - c0)
        blk[..., :live] = wb[..., c0:c0 + live]
        pack = a.out("wpack%d" % c0, nbytes=lib.dmc_dconv_wpack_bytes(cb, r), dtype=U8)
        a.call("dmc_dconv_pack_weights", a.inp("w%d" % c0, blk), pack, cb, r, 1)
        a.call("dmc_densetrain_layer_dgrad", g, pack, n, h, w, ct, k, r, c0, cb)


def _dgrad_check(bufs):
    n, h, w, ct, k, r = ARENA_LAYER
    _, G, _, dg, _ = layer_case(*ARENA_LAYER)
    got = bufs["G"].t
    e = float((got[..., :k].double().cpu() - (G[..., :k].double() + dg)).abs().max() / dg.abs().max())
    assert e < 1e-5, e
    assert torch.equal(bits(got[..., k:]), bits(G[..., k:]).to(got.device))


def head_arena_case(a):
    ct, (n, h, w) = ARENA_HEAD
    buf, wb, dout, _, _, _ = head_case(*ARENA_HEAD)
    lib = _lib.load()
    d, f = a.inp("dout", dout), a.inp("feat", buf)
    a.call("dmc_densetrain_head_dgrad", d, a.inp("w", wb), a.out("G", (n, h, w, ct)), n, h, w, ct)
    a.call("dmc_densetrain_head_wgrad", d, f, a.out("dw", (2, 3, 3, ct)), a.out("db", (2,)),
           a.work("workspace", lib.dmc_densetrain_head_workspace_bytes(n, h, w, ct)), n, h, w, ct)
    a.call("dmc_densetrain_export", a.inp("Gx", buf), a.out("dx", (n, 5, h, w)), n, h, w, ct)


def _head_check(bufs):
    buf, _, _, gref, dwref, dbref = head_case(*ARENA_HEAD)
    assert rel_err(bufs["G"].t, gref) < 1e-5 and rel_err(bufs["dw"].t, dwref) < 1e-5 and rel_err(bufs["db"].t, dbref) < 1e-5
    assert torch.equal(bits(bufs["dx"].t), bits(buf[..., :5].permute(0, 3, 1, 2)).to(bufs["dx"].t.device))


def refused_dgrad_case(a):     # c0 + cb > K + 16
    n, h, w, ct, k, r = ARENA_LAYER
    a.call("dmc_densetrain_layer_dgrad", a.inout("G", torch.ones(n, h, w, ct)), a.inp("wpack", torch.zeros(128 * 32 * 54, dtype=U8)), n, h, w, ct, k, r, 128, 64)


def refused_mask_case(a):      # K + R > CT
    n, h, w, ct, k, r = ARENA_LAYER
    a.call("dmc_densetrain_mask", a.inp("feat", torch.ones(n, h, w, ct)), a.inout("G", torch.ones(n, h, w, ct)), a.out("db", (64,)),
           a.work("workspace", 4096), n, h, w, ct, k, 64)


ARENA_CASES = [
    abi_cases.Case(abi_cases.tag("dmc_densetrain_mask", *ARENA_LAYER), ["dmc_densetrain_mask"], mask_arena_case, check=_mask_check, capacity=32 << 20),
    abi_cases.Case(abi_cases.tag("dmc_densetrain_layer_wgrad", *ARENA_LAYER), ["dmc_densetrain_layer_wgrad"], wgrad_arena_case, check=_wgrad_check,
                   capacity=32 << 20),
    abi_cases.Case(abi_cases.tag("dmc_densetrain_layer_dgrad", *ARENA_LAYER), ["dmc_dconv_pack_weights", "dmc_densetrain_layer_dgrad"], dgrad_arena_case,
                   check=_dgrad_check, capacity=32 << 20),
    abi_cases.Case("dmc_densetrain_head-2-5-7-176", ["dmc_densetrain_head_dgrad", "dmc_densetrain_head_wgrad", "dmc_densetrain_export"], head_arena_case,
                   check=_head_check, capacity=32 << 20),
    abi_cases.Case("dmc_densetrain_layer_dgrad-refused-block", ["dmc_densetrain_layer_dgrad"], refused_dgrad_case,
                   expect_rc=abi_cases.DMC_E_INVALID, capacity=32 << 20),
    abi_cases.Case("dmc_densetrain_mask-refused-K+R-over-CT", ["dmc_densetrain_mask"], refused_mask_case,
                   expect_rc=abi_cases.DMC_E_INVALID, capacity=32 << 20),
]
_known = {c.id for c in abi_cases.CASES}
abi_cases.CASES.extend(c for c in ARENA_CASES if c.id not in _known)


@pytest.mark.parametrize("case", ARENA_CASES, ids=[c.id for c in ARENA_CASES])
def test_dense_train_entries_memory_contract(case):
    try:
        bufs = run_case(case.fn, device=DEV, capacity=case.capacity, expect_rc=case.expect_rc)
        if case.check is not None:
            case.check(bufs)
    except RuntimeError as e:
        if "HIP error" in str(e) or "illegal memory access" in str(e):
            # a faulted device serves nothing more: end the session here instead of launching the remaining cases on it
            pytest.exit("GPU fault in %s: %s" % (case.id, str(e).splitlines()[0]), returncode=3)
        raise
