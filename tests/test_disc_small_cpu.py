"""CPU: the host side of csrc/disc_c8.hip and csrc/disc_head.hip.

The header declares the ten dmc_disc_c8_* / dmc_disc_head_* entry points with the signatures _lib.SIGNATURES binds and the
library exports them; the queries run (host code); every refusal comes from the argument checks in front of the first launch; the
two switches of model.py are read from the environment and leave CPU tensors on the stock path; the references of
tests/disc_small_ref.py agree with autograd of the stock modules."""
import ctypes
import os
import re
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as F

from dmcnet_amd import _lib, model, ops
from tests import disc_small_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
I, P, Z = ctypes.c_int, ctypes.c_void_p, ctypes.c_size_t
NEW = {
    "dmc_disc_c8_supported": (I, [I] * 3),
    "dmc_disc_c8_stat_blocks": (I, [I] * 3),
    "dmc_disc_c8_fwd": (I, [P] * 6 + [I] * 5 + [P]),
    "dmc_disc_c8_dgrad": (I, [P] * 3 + [I] * 3 + [P]),
    "dmc_disc_c8_wgrad_bytes": (Z, [I] * 3),
    "dmc_disc_c8_wgrad": (I, [P] * 5 + [I] * 3 + [P]),
    "dmc_disc_head_supported": (I, [I] * 4),
    "dmc_disc_head_fwd": (I, [P] * 4 + [I] * 4 + [P]),
    "dmc_disc_head_bwd_bytes": (Z, [I] * 4),
    "dmc_disc_head_bwd": (I, [P] * 7 + [I] * 4 + [P]),
}


def test_entry_points_are_declared_bound_and_built():
    text = open(os.path.join(ROOT, "include", "dmcnet_hip.h")).read()
    lib = _lib.load()
    for name, sig in NEW.items():
        m = re.search(r"\b(int|size_t)\s+%s\(([^;]*)\);" % name, text)
        assert m, name + " is not declared in include/dmcnet_hip.h"
        args = [a.strip() for a in m.group(2).split(",")]
        kinds = [P if ("*" in a or a.startswith("dmc_stream_t")) else I for a in args]
        assert (Z if m.group(1) == "size_t" else I, kinds) == sig, name
        assert _lib.SIGNATURES[name] == sig and hasattr(lib, name)
    assert sorted(n for n in _lib.SIGNATURES if n.startswith(("dmc_disc_c8_", "dmc_disc_head_"))) == sorted(NEW)
    build = __import__("dmcnet_amd.build", fromlist=["SOURCES"])
    assert "disc_c8.hip" in build.SOURCES and "disc_head.hip" in build.SOURCES
    assert "code/dmcnet_GAN/model.py:254-265" in text and ":369-385" in text and "code/dmcnet_GAN/model.py:290,297-298" in text


def test_queries():
    lib = _lib.load()
    for shape in R.C8_SHAPES + [(240, 112, 112)]:
        n, h, w = shape
        px = n * (h // 2) * (w // 2)
        assert lib.dmc_disc_c8_supported(n, h, w) == 1
        assert lib.dmc_disc_c8_stat_blocks(n, h, w) == (px + 255) // 256
        assert lib.dmc_disc_c8_wgrad_bytes(n, h, w) == (px + 511) // 512 * 1168 * 4
    for shape in R.C8_ODD_SHAPES + [(0, 4, 4), (1, 0, 4), (1, 4, -2)]:
        assert lib.dmc_disc_c8_supported(*shape) == 0 and lib.dmc_disc_c8_stat_blocks(*shape) == 0 and lib.dmc_disc_c8_wgrad_bytes(*shape) == 0
    # x reaches 2^31 bytes at N H W = 2^26
    assert lib.dmc_disc_c8_supported(1024, 256, 256) == 0 and lib.dmc_disc_c8_supported(1023, 256, 256) == 1
    assert lib.dmc_disc_c8_supported(2 ** 31 - 2, 2 ** 31 - 2, 2 ** 31 - 2) == 0
    for shape in R.HEAD_SHAPES + [(384, 128, 14, 14), (240, 32, 28, 28)]:
        m, c, h, w = shape
        assert lib.dmc_disc_head_supported(*shape) == 1
        assert lib.dmc_disc_head_bwd_bytes(*shape) == (m + 15) // 16 * 2 * c * h * w * 4
    for shape in [(1, 24, 2, 2), (1, 8, 4, 4), (0, 16, 2, 2), (1, 16, 0, 2), (32768, 16, 64, 64), (2 ** 31 - 1, 2 ** 31 - 16, 2 ** 31 - 1, 2 ** 31 - 1)]:
        assert lib.dmc_disc_head_supported(*shape) == 0 and lib.dmc_disc_head_bwd_bytes(*shape) == 0
    assert lib.dmc_disc_head_supported(32767, 16, 64, 64) == 1


def test_refusals_come_before_any_launch():
    """(No GPU here: a call that got as far as a launch would not return DMC_E_INVALID.)"""
    lib = _lib.load()
    buf = torch.zeros(1 << 16)
    p, null, s0 = _lib.ptr(buf), _lib.ptr(None), P(0)
    inv = -1
    assert lib.dmc_disc_c8_fwd(null, p, p, p, p, null, 0, 1, 4, 6, 1, s0) == inv and b"null" in lib.dmc_last_error()
    assert lib.dmc_disc_c8_fwd(p, p, null, null, null, null, 0, 1, 4, 6, 1, s0) == inv
    assert lib.dmc_disc_c8_fwd(p, p, null, null, p, p, 2, 1, 4, 6, 1, s0) == inv and b"statistics" in lib.dmc_last_error()
    assert lib.dmc_disc_c8_fwd(p, p, null, null, p, null, 0, 1, 7, 9, 1, s0) == inv and b"unsupported" in lib.dmc_last_error()
    assert lib.dmc_disc_c8_dgrad(p, p, null, 1, 4, 6, s0) == inv
    assert lib.dmc_disc_c8_dgrad(p, p, p, 1024, 256, 256, s0) == inv
    assert lib.dmc_disc_c8_wgrad(p, p, p, p, null, 1, 4, 6, s0) == inv
    assert lib.dmc_disc_c8_wgrad(p, p, p, null, p, 2, 5, 12, s0) == inv
    assert lib.dmc_disc_head_fwd(p, p, null, p, 1, 16, 2, 3, s0) == inv
    assert lib.dmc_disc_head_fwd(p, p, p, p, 1, 24, 2, 2, s0) == inv
    assert lib.dmc_disc_head_bwd(p, p, null, p, p, p, p, 1, 16, 2, 3, s0) == inv
    assert lib.dmc_disc_head_bwd(p, null, p, p, null, null, null, 1, 16, 2, 3, s0) == inv          # dx without the weight
    assert lib.dmc_disc_head_bwd(null, p, p, null, p, null, p, 1, 16, 2, 3, s0) == inv             # dweight without x
    assert lib.dmc_disc_head_bwd(p, p, p, null, p, null, null, 1, 16, 2, 3, s0) == inv             # dweight without the workspace
    assert lib.dmc_disc_head_bwd(p, p, p, null, null, null, p, 1, 16, 2, 3, s0) == inv             # nothing asked for
    assert lib.dmc_disc_head_bwd(p, p, p, p, p, p, p, 32768, 16, 64, 64, s0) == inv
    assert not bool(buf.any())


def test_references_agree_with_autograd_of_the_stock_modules():
    """tests/disc_small_ref.py restates Conv2d(8, 16, 3, 2, 1) -> LeakyReLU(0.2) -> mask and Linear on the (c, h, w) flattening: its
    fp64 values are those of the stock fp32 modules to fp32 rounding, its bars are positive and small."""
    shape = (3, 12, 20)
    d = R.c8_inputs(shape)
    z64, bar = R.c8_forward(shape, True, True, 1)
    x = R.nchw(d["x"]).contiguous().requires_grad_(True)
    w = d["w"].permute(0, 3, 1, 2).contiguous().requires_grad_(True)
    b = d["bias"].clone().requires_grad_(True)
    z = F.leaky_relu(F.conv2d(x, w, b, 2, 1), 0.2) * d["keep"][:, :, None, None]
    assert R.ratio(R.nhwc(z), z64, bar) <= 1.0 and float(bar.max()) < 1e-4
    g = R.c8_grads(shape)
    gx, gw, gb = torch.autograd.grad((F.conv2d(x, w, b, 2, 1) * R.nchw(d["g"])).sum(), [x, w, b])
    assert R.ratio(R.nhwc(gx), g["dx"], g["dx_bar"]) <= 1.0
    assert R.ratio(gw.permute(0, 2, 3, 1), g["dw"], g["dw_bar"]) <= 1.0 and R.ratio(gb, g["db"], g["db_bar"]) <= 1.0
    hs = (3, 32, 28, 28)
    hd, ref = R.head_inputs(hs), R.head_ref(hs)
    xf = R.head_flat(hd["x"]).contiguous().requires_grad_(True)
    wt, bb = hd["weight"].clone().requires_grad_(True), hd["bias"].clone().requires_grad_(True)
    v = F.linear(xf, wt, bb)
    gxf, gwt, gbb = torch.autograd.grad(v, [xf, wt, bb], hd["dv"])
    assert R.ratio(v, ref["v"], ref["v_bar"]) <= 1.0 and R.ratio(gwt, ref["dw"], ref["dw_bar"]) <= 1.0
    assert R.ratio(R.nhwc(gxf.reshape(3, 32, 28, 28)), ref["dx"], ref["dx_bar"]) <= 1.0 and R.ratio(gbb, ref["db"], ref["db_bar"]) <= 1.0


def test_switches_follow_the_environment():
    code = "from dmcnet_amd import model; print(int(model.DISC_C8), int(model.DISC_HEAD))"
    for value, want in ((None, "%d %d" % (model.DISC_C8_BY_DEFAULT, model.DISC_HEAD_BY_DEFAULT)), ("0", "0 0"), ("1", "1 1")):
        env = dict(os.environ)
        for k in ("DMC_DISC_C8", "DMC_DISC_HEAD"):
            env.pop(k, None)
            if value is not None:
                env[k] = value
        out = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, capture_output=True, text=True, check=True).stdout
        assert out.split() == want.split()


def test_cpu_tensors_are_not_taken_by_either_route():
    """The predicates refuse CPU tensors (and a head without a bias, or of another width) whatever the switches say: forward then
    takes the branch it took before."""
    m = model._DISCRIMINATORS["Discriminator4"](2)
    conv = m.discriminator_block_2[0]
    assert (conv.in_channels, conv.out_channels, conv.stride) == (8, 16, (2, 2))
    x = torch.zeros(1, 8, 32, 32).contiguous(memory_format=torch.channels_last)
    assert not ops.disc_block_supported(x, conv, False, c8=True) and not ops.disc_block_supported(x, conv, False)
    a = torch.zeros(1, 32, 28, 28).contiguous(memory_format=torch.channels_last)
    assert tuple(m.adv_layer.weight.shape) == (2, 32 * 28 * 28) and not ops.disc_head_supported(a, m.adv_layer)
    assert not ops.disc_head_supported(a, torch.nn.Linear(32 * 28 * 28, 2, bias=False))
