"""Plain-numpy restatement of the reference's interpolated flow upsampling (code/dmcnet/dataset.py:236-246:
``scipy.interpolate.interp1d(linspace(0, 1, n), means, kind="linear", axis)(linspace(0, 1, n * factor))`` along H and then
along W).  No scipy import here: the GPU tests compare the device path against this module, and
tests/test_device_prep_cpu.py ties it to ``dataset.blockify(..., upsample_interp=True)`` (scipy) bit for bit.

scipy's linear kernel is ``idx = clip(searchsorted(x, xn), 1, n - 1); lo = idx - 1;
y = ((y[idx] - y[lo]) / (x[idx] - x[lo])) * (xn - x[lo]) + y[lo]`` in fp64.  searchsorted is left-sided, so an ``xn`` that
equals a knot is evaluated in the interval to its left."""
import numpy as np


def taps(n, factor):
    """(lo int64, dx float64, t float64), each [n * factor], of one axis with ``n`` blocks."""
    if n < 2:
        raise ValueError("interpolation needs at least two blocks on an axis (got %d)" % n)
    x, xn = np.linspace(0, 1, n), np.linspace(0, 1, n * factor)
    idx = np.clip(np.searchsorted(x, xn), 1, n - 1)
    lo = idx - 1
    return lo, x[idx] - x[lo], xn - x[lo]


def block_means(flow, factor):
    """[..., H, W] integers -> fp64 means over factor x factor blocks, ragged edges zero-padded."""
    h, w = flow.shape[-2:]
    nh, nw = -(-h // factor), -(-w // factor)
    x = np.zeros(flow.shape[:-2] + (nh * factor, nw * factor), np.int64)
    x[..., :h, :w] = flow
    sums = x.reshape(flow.shape[:-2] + (nh, factor, nw, factor)).sum(axis=(-3, -1))
    return sums.astype(np.float64) / np.float64(factor * factor)


def blockify_interp(flow, factor):
    """== ``dataset.blockify(flow, factor, upsample_interp=True)``: fp64 [..., H, W]."""
    h, w = flow.shape[-2:]
    y = block_means(np.asarray(flow), factor)
    lo, dx, t = taps(y.shape[-2], factor)
    y_lo, y_hi = y[..., lo, :], y[..., lo + 1, :]
    y = ((y_hi - y_lo) / dx[:, None]) * t[:, None] + y_lo
    lo, dx, t = taps(y.shape[-1], factor)
    y_lo, y_hi = y[..., lo], y[..., lo + 1]
    y = ((y_hi - y_lo) / dx) * t + y_lo
    return y[..., :h, :w]


def flow_tensor(frames, factor):
    """The flow tensor ``dataset.to_tensors(frames [S,7,H,W], factor, upsample_interp=True)[0]`` returns."""
    import torch
    from dmcnet_amd import dataset
    f = torch.from_numpy(np.ascontiguousarray(blockify_interp(np.asarray(frames)[:, 0:2], factor))).float() / 255.0
    std = torch.tensor(dataset._STD, dtype=torch.float32).reshape(1, 3, 1, 1)
    return (f - 0.5) / torch.mean(std)
