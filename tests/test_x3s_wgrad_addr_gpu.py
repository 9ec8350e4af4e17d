"""GPU: the transfer addressing of the weight-gradient kernels (x3s_wgrad_kernel in conv_x3s.hip, x3q_wgrad_kernel in
conv_x3q.hip) where a slip would hide.  The kernels fetch padded image rows: pad rows, the columns left and right of the
image, the group in front of the first image and the groups behind the last one must arrive as ZEROS, which only an explicit
out-of-range offset produces (the buffer descriptors span 2 GB).  Per shape (tests/wgrad_addr_shapes.py: every width, N = 1,
odd N, H != W, ragged last groups, several ci / co tiles):
  * dw against an fp64 torch convolution weight gradient on random inputs, <= 1e-5 relative as tests/test_x3s_gpu.py -- a
    lane that reads a wrong pixel INSIDE the tensor shows here;
  * two runs bit for bit;
  * the same call with the slice tensors in the middle of allocations filled with NaN bit patterns: the result must be the
    same bits (hence free of NaN) -- a lane that reads OUTSIDE the tensor where it should have received zeros shows here.
Only the split and the weight-gradient entry points are called."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import dmcnet_amd
from dmcnet_amd import ops
from tests.wgrad_addr_shapes import X3Q_ADDR_CASES, X3S_ADDR_CASES

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CL = torch.channels_last
MARGIN = 1 << 20          # bytes of NaN patterns on each side: far more than the rows a group can reach beyond a tensor


def rnd(seed, shape):
    return torch.from_numpy(np.random.RandomState(seed).standard_normal(shape).astype(np.float32))


def rel_err(a, b):
    a, b = a.detach().double().cpu(), torch.as_tensor(b).double().cpu()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))


def amid_nan(t):
    """A copy of the byte tensor ``t`` whose surroundings, MARGIN bytes on each side, read as NaN in bf16 and in fp32."""
    nbytes = (t.numel() + 255) // 256 * 256
    big = torch.empty(2 * MARGIN + nbytes, dtype=torch.uint8, device=t.device)
    big.view(torch.int16).fill_(0x7FC0)
    assert bool(torch.isnan(big.view(torch.bfloat16)).all()) and bool(torch.isnan(big.view(torch.float32)).all())
    mid = big[MARGIN:MARGIN + t.numel()]
    mid.copy_(t)
    assert mid.data_ptr() % 256 == 0
    return mid


@pytest.mark.parametrize("case", X3S_ADDR_CASES)
def test_x3s_wgrad_addresses(case):
    n, cin, h, w, cout = case
    assert dmcnet_amd._lib.load().dmc_x3s_conv_wgrad_supported(n, h, w, cin, cout)
    x, go = rnd(301, (n, cin, h, w)), rnd(303, (n, cout, h, w))
    wo = torch.zeros((cout, cin, 3, 3), dtype=torch.float64, requires_grad=True)
    (F.conv2d(x.double(), wo, None, 1, 1) * go.double()).sum().backward()
    xs = ops.x3s_split(x.to(DEV).contiguous(memory_format=CL))
    dys = ops.x3s_split(go.to(DEV).contiguous(memory_format=CL))
    dw = ops.x3s_conv_wgrad(xs, dys, n, h, w, cin, cout)
    err = rel_err(dw, wo.grad)
    print("x3s wgrad %s: rel err %.3e" % (case, err))
    assert err < 1e-5
    assert torch.equal(dw, ops.x3s_conv_wgrad(xs, dys, n, h, w, cin, cout))
    guarded = ops.x3s_conv_wgrad(amid_nan(xs), amid_nan(dys), n, h, w, cin, cout)
    assert not bool(torch.isnan(guarded).any())
    assert torch.equal(dw, guarded)


@pytest.mark.parametrize("case", X3Q_ADDR_CASES)
def test_x3q_wgrad_addresses(case):
    n, cin, h, w, cout = case
    oh, ow = h // 2, w // 2
    assert dmcnet_amd._lib.load().dmc_x3q_conv_wgrad_supported(n, oh, ow, cin, cout)
    x = rnd(631, (n, cin, h, w))
    g3, g1 = rnd(634, (n, cout, oh, ow)), rnd(635, (n, cout, oh, ow))
    w3 = torch.zeros((cout, cin, 3, 3), dtype=torch.float64, requires_grad=True)
    w1 = torch.zeros((cout, cin, 1, 1), dtype=torch.float64, requires_grad=True)
    (F.conv2d(x.double(), w3, None, 2, 1) * g3.double()).sum().backward()
    (F.conv2d(x.double(), w1, None, 2, 0) * g1.double()).sum().backward()
    xq = ops.x3q_split(x.to(DEV).contiguous(memory_format=CL))
    dys3 = ops.x3s_split(g3.to(DEV).contiguous(memory_format=CL))
    dys1 = ops.x3s_split(g1.to(DEV).contiguous(memory_format=CL))
    dw3, dw1 = ops.x3q_conv_wgrad(xq, dys3, dys1, n, oh, ow, cin, cout)
    e3, e1 = rel_err(dw3, w3.grad), rel_err(dw1, w1.grad)
    print("x3q wgrad %s: rel err %.3e (3x3) %.3e (1x1)" % (case, e3, e1))
    assert e3 < 1e-5 and e1 < 1e-5
    dw3b, dw1b = ops.x3q_conv_wgrad(xq, dys3, dys1, n, oh, ow, cin, cout)
    assert torch.equal(dw3, dw3b) and torch.equal(dw1, dw1b)
    g3w, g1w = ops.x3q_conv_wgrad(amid_nan(xq), amid_nan(dys3), amid_nan(dys1), n, oh, ow, cin, cout)
    assert not bool(torch.isnan(g3w).any()) and not bool(torch.isnan(g1w).any())
    assert torch.equal(dw3, g3w) and torch.equal(dw1, g1w)
