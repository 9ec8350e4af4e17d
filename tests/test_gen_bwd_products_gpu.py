"""The backward of EstimatorDenseNetTiny (dmc_gen_tiny_bwd: the data gradient of csrc/gen_tiny.hip, the weight gradients of
csrc/gen_wgrad.hip and gen_bwd_weight_pc_kernel) held to the two layers of tests/test_x3_products_gpu.py: exact cases that tell
six bf16x3 slice products from five and one pixel from its neighbour, and the error tap by tap against the CPU emulation.

The operator is called at the C ABI: it takes the saved features as an input, derives the LeakyReLU branches from their sign,
leaves the pre-activation gradients in the caller's gbuf and reads them back for the weight gradient.  So the tests hand it
features of their own (no forward runs) and read back the operand the weight gradient consumed.  dw, db, gbuf and partials
are filled with 0xFF bytes before every call.  The reference, the operand families, the checks and the reasoning behind every
exactness premise are in tests/gen_bwd_ref.py; tests/test_gen_bwd_ref_cpu.py shows each check failing on a seeded defect.

  (a) integers everywhere, every slope 1: gbuf, six dw, six db equal the fp64 backward bit for bit (bounds on every partial sum
      asserted, the Winograd transforms' factor 4 included); also with the frames processed two at a time (gen_frames);
  (b) the layers above k silenced, saved_k with both signs and exact zeros: gbuf is G_k or the fp32 product 0.1f G_k, pixel by
      pixel -- which pixel's sign a gradient takes;
  (c) one term per output, the other operand with all three slices: A, g one-hot against 24-bit inputs; B, inputs one-hot
      against 24-bit gradients; the hot pixels on both sides of every seam of the row-sliding kernel (columns 7 | 8,
      31 | 32 | 33, W - 1; rows 0 | 1, 27 | 28, H - 1; first, middle and last frame);
  (d) Gaussian and wide-range operands: rms and max error per tap against x3_ref.emulate on the operands the kernel read, bars
      3 and 4 (test_x3_products_gpu.report).

Options: gen_wgrad_path 5 (row-sliding kernel where W % 4 == 0 and H >= 2) and 4; gen_wino 0 (direct data gradient), 768 (the
default: groups 0 and 1 on the Winograd kernel where 64 <= W <= 224, W % 4 == 0) and 0x1F00 (all five groups).

Measured on an MI355X (all 445 cases pass, the file takes 35 s): no case of (a), (b) or (c) differs in a single bit under either
weight-gradient path and any of the three Winograd settings.  Statistical layer, worst kernel / emulation ratios: rms 1.29 (bar
3), max 1.27 (bar 4), both at (1, 2, 4), where a contraction is 8 pixels and both paths give the same figures; from (1, 30, 64)
upwards the row-sliding kernel sits at 0.17 .. 0.83 of the emulation's rms and path 4 at 0.16 .. 0.43: the emulation rounds its
one accumulator after every 16-pixel dot product, the kernels keep one accumulator per workgroup and sum those in a tree, so
the longer the contraction the further they stay below it."""
import contextlib
import time

import numpy as np
import pytest
import torch

import dmcnet_amd
from tests import gen_bwd_ref as B
from tests.test_x3_products_gpu import report

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

#: the worst (rms, max) kernel / emulation ratios this file printed on an MI355X per weight-gradient path (bars 3 and 4); a
#: record, not a bar
WORST_MEASURED = {"gen-wgrad-path5": (1.288, 1.274), "gen-wgrad-path4": (1.288, 1.274)}

SHAPES = [(1, 2, 4),          # the smallest
          (2, 3, 36),         # odd height; a 32-column strip and a 4-column one: a left-column hand-over
          (1, 30, 64),        # two bands (28 + 2 rows), two full strips
          (3, 9, 100),        # four strips, the last one partial
          (1, 5, 224),        # the widest width the ring kernels serve
          (1, 6, 228),        # wider than that
          (130, 2, 64),       # 260 segments on <= 256 workgroups: ranges that begin at strip 1 fill the cache from memory
          (1, 1, 64),         # H = 1: the tile kernel even under path 5
          (1, 7, 33),         # W % 4 != 0: the VALU kernels
          (1, 9, 68), (2, 3, 64), (1, 33, 128)]      # Winograd data gradient (64 <= W, W % 4 == 0), tile edges
FRAMES_SHAPE = (5, 3, 64)
PATHS = [5, 4]
WINOS = [0, 768, 0x1F00]
_TIMES = {}


@contextlib.contextmanager
def options(**kw):
    lib = dmcnet_amd._lib.load()
    before = {k: lib.dmc_get_option(k.encode()) for k in kw}
    try:
        for k, v in kw.items():
            dmcnet_amd._lib.check(lib.dmc_set_option(k.encode(), int(v)), "dmc_set_option")
        yield
    finally:
        for k, v in before.items():
            dmcnet_amd._lib.check(lib.dmc_set_option(k.encode(), v), "dmc_set_option")


def _ff(nbytes):
    assert nbytes % 4 == 0
    return torch.full((nbytes,), 255, dtype=torch.uint8, device=DEV).view(torch.float32)


def run(mv, res, saved, ws, gout):
    """dmc_gen_tiny_bwd through ctypes -> (gbuf [N, 28, H, W], dw[6], db[6]) as numpy fp32."""
    L, lib = dmcnet_amd._lib, dmcnet_amd._lib.load()
    n, _, h, w = mv.shape
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(DEV).contiguous()      # noqa: E731
    mv_d, res_d, saved_d, gout_d = d(mv), d(res), d(saved), d(gout)
    ws_d = [d(x) for x in ws]
    assert [tuple(x.shape) for x in ws_d] == [B.wshape(k) for k in range(B.NL)]
    dws = [_ff(4 * x.numel()).view(x.shape) for x in ws_d]
    dbs = [_ff(4 * B.cout_of(k)) for k in range(B.NL)]
    assert lib.dmc_gen_tiny_gbuf_bytes(n, h, w) == lib.dmc_gen_tiny_saved_bytes(n, h, w) == 4 * saved_d.numel()
    gbuf, partials = _ff(lib.dmc_gen_tiny_gbuf_bytes(n, h, w)), _ff(lib.dmc_gen_tiny_partials_bytes(n, h, w))
    work = torch.empty(lib.dmc_gen_tiny_workspace_bytes() // 4, device=DEV)
    L.check(lib.dmc_gen_tiny_bwd(L.ptr(mv_d), L.ptr(res_d), L.ptr_array(ws_d), L.ptr(saved_d), L.ptr(gout_d), L.ptr_array(dws),
                                 L.ptr_array(dbs), L.ptr(gbuf), L.ptr(partials), L.ptr(work), n, h, w,
                                 torch.cuda.current_stream().cuda_stream), "dmc_gen_tiny_bwd")
    torch.cuda.synchronize()
    return gbuf.view(n, B.NFEAT, h, w).cpu().numpy(), [x.cpu().numpy() for x in dws], [x.cpu().numpy() for x in dbs]


@pytest.fixture(autouse=True)
def _wall_time(request):
    t0 = time.time()
    yield
    _TIMES[request.node.name] = time.time() - t0
    print("  wall time of this file so far: %.1f s over %d cases" % (sum(_TIMES.values()), len(_TIMES)))


_INT_CASES = {}


def int_case(shape):
    """The integer operands and their fp64 reference, computed once per shape and shared by every option combination."""
    if shape not in _INT_CASES:
        _INT_CASES[shape] = B.integer_operands(shape, 11)
    return _INT_CASES[shape]


def test_options_are_the_documented_defaults():
    lib = dmcnet_amd._lib.load()
    assert lib.dmc_get_option(b"gen_wgrad_path") == 5 and lib.dmc_get_option(b"gen_wino") == 768
    assert lib.dmc_get_option(b"gen_frames") == 0


# ================================================================ (a) integers: everything exact
@pytest.mark.parametrize("wino", WINOS)
@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("shape", SHAPES)
def test_integer_operands_come_back_bit_for_bit(shape, path, wino):
    with options(gen_wgrad_path=path, gen_wino=wino):
        B.check_integer(run, int_case(shape))


@pytest.mark.parametrize("frames", [0, 2])
@pytest.mark.parametrize("wino", WINOS)
@pytest.mark.parametrize("path", PATHS)
def test_integer_operands_frames_per_pass(path, wino, frames):
    """N = 5 frames in one pass and in passes of 2, 2 and 1."""
    with options(gen_wgrad_path=path, gen_wino=wino, gen_frames=frames):
        B.check_integer(run, int_case(FRAMES_SHAPE))


# ================================================================ (b) which pixel's sign a gradient takes
@pytest.mark.parametrize("wino", WINOS)
@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("shape", SHAPES)
def test_branch_is_taken_from_the_pixels_own_feature(shape, path, wino):
    with options(gen_wgrad_path=path, gen_wino=wino):
        B.check_branch(run, shape, 21)


# ================================================================ (c) one term per output
@pytest.mark.parametrize("wino", WINOS)
@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("shape", SHAPES)
def test_one_hot_gradient_returns_the_inputs_bit_for_bit(shape, path, wino):
    with options(gen_wgrad_path=path, gen_wino=wino):
        B.check_g_one_hot(run, shape, 31)


@pytest.mark.parametrize("wino", WINOS)
@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("shape", SHAPES)
def test_one_hot_inputs_return_the_gradient_bit_for_bit(shape, path, wino):
    with options(gen_wgrad_path=path, gen_wino=wino):
        B.check_in_one_hot(run, shape, 41)


# ================================================================ (d) error tap by tap against the emulation
@pytest.mark.parametrize("family", ["gauss", "wide"])
@pytest.mark.parametrize("wino", WINOS)
@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("shape", SHAPES)
def test_weight_gradient_error_tap_by_tap(shape, path, wino, family):
    with options(gen_wgrad_path=path, gen_wino=wino):
        rms, mx, _ = B.statistics(run, shape, family, 700)
    report("gen-wgrad-path%d %s wino %#x %s" % (path, shape, wino, family), rms, mx)
