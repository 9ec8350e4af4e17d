"""The ContextNetwork's dilated convolutions (csrc/dconv.hip) and the dense estimators' layers (csrc/dense_eval.hip,
csrc/dense_train.hip) run ONE main loop (gather_gemm, csrc/ctx_common.h), and their weight-gradient kernels the same loop in
two copies with one plan of pixel ranges and one reduce (csrc/ctx_wgrad.h): at shapes both families accept, the two give the
same bits, so a change to one side that the other does not get shows here.

Through the C ABI only.  The dense side works inside feature buffers [M][CT] with CT = K + R + 16, so its pixel stride differs
from every width and a tail of 16 channels exists behind the slot; the dconv side gets contiguous copies of the same values.
Operands are seeded Gaussians, outputs and every channel a launch must not read or write are prefilled with NaN bytes, workspaces
have exactly the reported size, every launch runs twice and must repeat its bits.  Equality is torch.equal (-0 equals +0: the
dense data gradient adds its sum to a zero).

Pixel shapes: (2, 11, 13) = 286 pixels: two 256-pixel workgroups, the second partly empty, an image boundary inside a tile, nine
weight-gradient ranges of one step; for the weight gradient also (3, 27, 29) = 2349 pixels: 74 steps in 37 ranges of two, the
last step 13 pixels.  (K, R) puts TN = 1 .. 4 on both sides."""
import functools

import numpy as np
import pytest
import torch

from dmcnet_amd import _lib, ops

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U8 = torch.uint8
SLOPE = np.float32(0.1)

FRAME = (2, 11, 13)
WGRAD_FRAMES = [FRAME, (3, 27, 29)]
CHANNELS = [(32, 128), (64, 96), (96, 32), (128, 64)]           # (K, R)
CH_IDS = ["%d-%d" % c for c in CHANNELS]

P = _lib.ptr


def ok(rc, what):
    _lib.check(rc, what)


def nan_bytes(nbytes):
    return torch.full((max(int(nbytes), 1),), 0xFF, dtype=U8, device=DEV)


def nan_buffer(shape):
    return nan_bytes(4 * int(np.prod(shape))).view(torch.float32).view(shape)


def bits(t):
    return t.contiguous().view(torch.int32)


def twice(launch):
    """The launch's result, produced twice from fresh outputs and bit-equal."""
    a, b = launch(), launch()
    assert torch.equal(bits(a), bits(b))
    return a


def leaky32(v):
    """v > 0 ? v : 0.1f * v in numpy float32 (the layer's epilogue), device tensor in and out."""
    a = v.cpu().numpy()
    return torch.from_numpy(np.where(a > 0, a, SLOPE * a).astype(np.float32)).to(DEV)


@functools.lru_cache(maxsize=None)
def operands(frame, k, r):
    """(feat [N, H, W, CT], G [N, H, W, CT], weight OHWI [R, 3, 3, K]) on the device, never modified.  feat: Gaussians in [0, K),
    NaN bytes behind; G: NaN bytes except Gaussians in the slot [K, K + R)."""
    n, h, w = frame
    ct = k + r + 16
    g = np.random.RandomState(7000 + 97 * n * h * w + 3 * k + r)
    feat, G = nan_buffer((n, h, w, ct)), nan_buffer((n, h, w, ct))
    feat[..., :k] = torch.from_numpy(g.standard_normal((n, h, w, k)).astype(np.float32)).to(DEV)
    G[..., k:k + r] = torch.from_numpy(g.standard_normal((n, h, w, r)).astype(np.float32)).to(DEV)
    wt = torch.from_numpy((g.standard_normal((r, 3, 3, k)) * (1.4 / np.sqrt(9.0 * k))).astype(np.float32)).to(DEV)
    return feat, G, wt


def dconv_pack(wt, k, r, transposed):
    lib = _lib.load()
    wp = nan_bytes(lib.dmc_dconv_wpack_bytes(k, r))
    ok(lib.dmc_dconv_pack_weights(P(wt), P(wp), k, r, transposed, ops._stream()), "dmc_dconv_pack_weights")
    return wp


def dense_pack(wt, k, r):
    lib = _lib.load()
    wp = nan_bytes(lib.dmc_dense_wpack_bytes(k, r))
    ok(lib.dmc_dense_pack_weights(P(wt), P(wp), k, r, ops._stream()), "dmc_dense_pack_weights")
    return wp


def dconv_fwd(x, wp, cin, cout):
    lib = _lib.load()
    n, h, w, _ = x.shape
    assert x.is_contiguous() and x.shape[3] == cin
    y = nan_buffer((n, h, w, cout))
    ok(lib.dmc_dconv_fwd(P(x), P(wp), P(y), n, h, w, cin, cout, 1, ops._stream()), "dmc_dconv_fwd")
    return y


@pytest.mark.parametrize("k,r", CHANNELS, ids=CH_IDS)
def test_packs_are_the_same_bytes(k, r):
    lib = _lib.load()
    wt = operands(FRAME, k, r)[2]
    assert lib.dmc_dense_wpack_bytes(k, r) == lib.dmc_dconv_wpack_bytes(k, r) == k * r * 9 * 3 * 2
    assert torch.equal(twice(lambda: dense_pack(wt, k, r)), twice(lambda: dconv_pack(wt, k, r, 0)))


@pytest.mark.parametrize("k,r", CHANNELS, ids=CH_IDS)
def test_layer_forward_is_the_dilated_forward(k, r):
    lib = _lib.load()
    feat0, _, wt = operands(FRAME, k, r)
    n, h, w, ct = feat0.shape
    wp_dense, wp_dconv = dense_pack(wt, k, r), dconv_pack(wt, k, r, 0)
    bias = torch.zeros(r, device=DEV)

    def dense():
        feat = feat0.clone()
        ok(lib.dmc_dense_layer_eval(P(feat), P(wp_dense), P(bias), n, h, w, ct, k, r, ops._stream()), "dmc_dense_layer_eval")
        return feat

    feat = twice(dense)
    want = leaky32(twice(lambda: dconv_fwd(feat0[..., :k].contiguous(), wp_dconv, k, r)))
    assert torch.equal(feat[..., k:k + r], want)
    assert torch.equal(bits(feat[..., :k]), bits(feat0[..., :k]))
    assert torch.equal(bits(feat[..., k + r:]), bits(feat0[..., k + r:]))


@pytest.mark.parametrize("k,r", CHANNELS, ids=CH_IDS)
def test_layer_data_gradient_is_the_dilated_forward_on_the_transposed_pack(k, r):
    lib = _lib.load()
    _, G0, wt = operands(FRAME, k, r)
    n, h, w, ct = G0.shape
    wpt = dconv_pack(wt, k, r, 1)

    def dense():
        G = G0.clone()
        G[..., :k] = 0
        ok(lib.dmc_densetrain_layer_dgrad(P(G), P(wpt), n, h, w, ct, k, r, 0, k, ops._stream()), "dmc_densetrain_layer_dgrad")
        return G

    G = twice(dense)
    want = twice(lambda: dconv_fwd(G0[..., k:k + r].contiguous(), wpt, r, k))
    assert torch.equal(G[..., :k], want)
    assert torch.equal(bits(G[..., k:]), bits(G0[..., k:]))


@pytest.mark.parametrize("k,r", CHANNELS, ids=CH_IDS)
@pytest.mark.parametrize("frame", WGRAD_FRAMES, ids=["2-11-13", "3-27-29"])
def test_layer_weight_gradient_is_the_dilated_weight_gradient(frame, k, r):
    lib = _lib.load()
    feat, G, _ = operands(frame, k, r)
    n, h, w, ct = feat.shape
    nbytes = lib.dmc_densetrain_wgrad_workspace_bytes(n, h, w, k, r)
    assert nbytes == lib.dmc_dconv_wgrad_workspace_bytes(n, h, w, k, r) > 0
    x, dy = feat[..., :k].contiguous(), G[..., k:k + r].contiguous()

    def dense():
        dw, work = nan_buffer((r, 3, 3, k)), nan_bytes(nbytes)
        ok(lib.dmc_densetrain_layer_wgrad(P(feat), P(G), P(dw), P(work), n, h, w, ct, k, r, ops._stream()), "dmc_densetrain_layer_wgrad")
        return dw

    def dconv():
        dw, work = nan_buffer((r, 3, 3, k)), nan_bytes(nbytes)
        ok(lib.dmc_dconv_wgrad(P(x), P(dy), P(dw), P(work), n, h, w, k, r, 1, ops._stream()), "dmc_dconv_wgrad")
        return dw

    assert torch.equal(twice(dense), twice(dconv))
