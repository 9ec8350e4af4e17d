"""Reference side of the dense-estimator training route (csrc/dense_train.hip, ops.dense_train*), in plain torch / numpy.

In buffer order (NHWC, OHWI), tap by tap, as matrix products -- a formulation that shares nothing with the kernels and that
tests/test_dense_train_cpu.py holds against torch autograd of F.conv2d:

  * dgrad(dz, w)   dL/dx [N, H, W, K] of y = conv3x3(x, w) given dz = dL/dy [N, H, W, R]:  sum_t dz[m - o(t)] @ w[:, t, :]
  * wgrad(dz, x)   dL/dw [R, 3, 3, K]:                                                     dz[m]^T @ x[m + o(t)] per tap
  * mask(f, g)     where(f > 0, g, g * float32(0.1)) in float32, as the mask pass defines it
  * network_grads  fp64 / fp32 gradients of the whole stack (tests/dense_ref.stack with torch autograd) for the loss sum(out * r)

Works on any device and dtype (the big weight-gradient case runs it in fp64 on the GPU).  Nothing here reads a kernel's result."""
import numpy as np
import torch

from tests import dense_ref as D


def shift(t, dy, dx):
    """out[n, y, x] = t[n, y + dy, x + dx], zero outside the frame; t [N, H, W, C]."""
    n, h, w, c = t.shape
    p = torch.zeros((n, h + 2, w + 2, c), dtype=t.dtype, device=t.device)
    p[:, 1:-1, 1:-1] = t
    return p[:, 1 + dy:1 + dy + h, 1 + dx:1 + dx + w]


def dgrad(dz, w):
    """dz [N, H, W, R], w OHWI [R, 3, 3, K] -> [N, H, W, K]."""
    out = torch.zeros(tuple(dz.shape[:3]) + (w.shape[3],), dtype=dz.dtype, device=dz.device)
    for t in range(9):
        ky, kx = divmod(t, 3)
        out += shift(dz, -(ky - 1), -(kx - 1)) @ w[:, ky, kx, :]
    return out


def wgrad(dz, x):
    """dz [N, H, W, R], x [N, H, W, K] -> OHWI [R, 3, 3, K]."""
    r, k = dz.shape[3], x.shape[3]
    out = torch.zeros((r, 3, 3, k), dtype=dz.dtype, device=dz.device)
    a = dz.reshape(-1, r).t()
    for t in range(9):
        ky, kx = divmod(t, 3)
        out[:, ky, kx, :] = a @ shift(x, ky - 1, kx - 1).reshape(-1, k)
    return out


def mask(f, g):
    """numpy float32 arrays -> the masked gradient, float32."""
    f, g = np.asarray(f), np.asarray(g)
    assert f.dtype == np.float32 and g.dtype == np.float32
    return np.where(f > 0, g, g * np.float32(0.1))


def network_grads(name, x, r, dtype):
    """(out, [dw_0, db_0, ..., dw_head, db_head], dx) of the stack D.params(name) on ``x`` for the loss sum(out * r), in ``dtype``."""
    ps = [(w.detach().clone().to(dtype).requires_grad_(True), b.detach().clone().to(dtype).requires_grad_(True)) for w, b in D.params(name)]
    xx = x.detach().clone().to(dtype).requires_grad_(True)                      # (clones: the shared inputs stay leaves without a gradient)
    out = D.stack(ps, xx, dtype=dtype)[2]
    (out * r.to(dtype)).sum().backward()
    grads = []
    for w, b in ps:
        grads += [w.grad, b.grad]
    return out.detach(), grads, xx.grad
