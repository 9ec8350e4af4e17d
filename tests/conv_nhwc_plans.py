"""The kernel selection of dmc-net_amd/csrc/conv_nhwc.hip restated in plain Python (no torch), and the shapes at which its tile
configurations and the multi-step runs of its row-walking weight-gradient kernels are tested.

conv_nhwc.hip picks a kernel by problem size: use_v2 / use_v3, v3_choice (conv3_kernel, bf16x3), v2_choice (conv2_kernel, fp32
MFMA), block_pixels_v1 (conv_nhwc_kernel), wgrad3_plan / wgrad2_plan (rows per step, steps per workgroup) and wgrad_slices (the
generic split-K weight gradient).  tests/test_conv_nhwc_plans_cpu.py checks this restatement against the library's host queries
and records which configurations the older unit tests reach; tests/test_conv_nhwc_cfgs_gpu.py and
tests/test_conv_nhwc_wgrad_runs_gpu.py run the cases below on the GPU.

A "case" is (N, Cin, H, W, Cout, k, stride), padding k // 2, as in CONV_CASES of tests/test_hip_parity.py.  arith is the option
conv_arith (0 = fp32 MFMA, 1 = bf16x3), cfg the option conv_cfg (0 = automatic); conv_path is taken as 1 (its default)."""
from collections import namedtuple


def ceil_div(a, b):
    return -(-a // b)


def out_map(case):
    n, cin, h, w, cout, k, stride = case
    pad = k // 2
    return (h + 2 * pad - k) // stride + 1, (w + 2 * pad - k) // stride + 1


# ---- forward / data gradient: which kernel, which tile ---------------------------------------------------------------------------

def use_v2(cin, cout):
    return cin % 32 == 0 and cout % 32 == 0


def use_v3(cin, cout, arith):
    return arith == 1 and cin % 64 == 0 and cout % 64 == 0


#: conv3_kernel<BM, BN, WM, WN> of launch_conv3 by configuration (10 = 384 x 128 was removed and falls to the default, 128 x 64)
V3_TILES = {0: (256, 128, 8, 1), 1: (256, 64, 8, 1), 2: (128, 128, 4, 2), 3: (128, 256, 4, 2), 4: (64, 128, 2, 2),
            5: (128, 64, 4, 1), 6: (128, 128, 4, 1), 7: (64, 128, 2, 1), 8: (256, 128, 4, 1), 9: (128, 128, 2, 1),
            11: (192, 128, 2, 2), 12: (96, 128, 3, 1)}
#: conv2_kernel<BM, BN, WM, WN> of launch_conv by configuration
V2_TILES = {0: (128, 32, 4, 1), 1: (128, 64, 2, 2), 2: (64, 64, 2, 2), 3: (256, 64, 4, 1), 4: (128, 128, 2, 2),
            5: (64, 128, 1, 4), 6: (128, 128, 2, 4), 7: (256, 64, 4, 2), 8: (128, 64, 4, 2)}


def v3_honoured(cfg, cout):
    """Does v3_choice obey conv_cfg = cfg (1 + configuration) for this channel count?  11 (c == 10) never."""
    if not 1 <= cfg <= 13:
        return False
    c = cfg - 1
    if c == 10:
        return False
    return c in (1, 5) or (cout % 256 == 0 if c == 3 else cout % 128 == 0)


def v3_choice(cout, m, cfg=0):
    if v3_honoured(cfg, cout):
        return cfg - 1
    need = 512
    if cout % 128 == 0 and ceil_div(m, 256) * (cout // 128) >= need:
        return 0
    if cout % 128 == 0 and ceil_div(m, 128) * (cout // 128) >= need:
        return 2
    if cout % 128 != 0:
        return 1 if ceil_div(m, 256) * (cout // 64) >= need else 5
    if ceil_div(m, 192) * (cout // 128) >= 200:
        return 11
    return 6


def v2_honoured(cfg, cout):
    if cout % 64 != 0:
        return False
    if cfg in (1, 2, 3, 7, 8):
        return True
    return cfg in (4, 5, 6) and cout % 128 == 0


def v2_choice(cout, m, cfg=0):
    if cout % 64 != 0:
        return 0
    if v2_honoured(cfg, cout):
        return cfg
    need = 640
    if cout % 128 == 0 and ceil_div(m, 128) * (cout // 128) >= need:
        return 6
    if ceil_div(m, 256) * (cout // 64) >= need:
        return 3
    if ceil_div(m, 128) * (cout // 64) >= need:
        return 8
    return 2


def block_pixels_v1(cout, m):
    if cout >= 64:
        return 128 if m >= 32768 else 64
    return 128 if cout >= 32 else 256          # launch_conv: 128 x 32 tiles for 32 and 48 channels, 256 x 16 for 16


def _csm_s1(case, arith, cfg):
    n, cin, h, w, cout, k, stride = case
    return arith == 1 and cfg != 301 and cin == cout and cin in (16, 32) and k == 3 and stride == 1


def _csm_s2(case, arith, cfg):
    n, cin, h, w, cout, k, stride = case
    return arith == 1 and cfg not in (301, 303) and (cin, cout) == (16, 32) and k == 3 and stride == 2 and h % 2 == 0 and w % 2 == 0


#: kernel: "conv3" | "conv2" | "conv_nhwc" (first generation) | "conv_small" (another file: no configuration);
#: cfg: the configuration chosen (None outside conv3 / conv2); bm, bn: the tile; m: pixels of the launch
Choice = namedtuple("Choice", "kernel cfg bm bn m")


def gemm_choice(cin, cout, m, arith, cfg=0):
    """The launch of launch_conv3 / launch_conv for a GEMM that contracts over cin and produces cout channels at m pixels."""
    if use_v3(cin, cout, arith):
        c = v3_choice(cout, m, cfg)
        bm, bn = V3_TILES.get(c, V3_TILES[5])[:2]
        return Choice("conv3", c, bm, bn, m)
    if use_v2(cin, cout):
        c = v2_choice(cout, m, cfg)
        bm, bn = V2_TILES[c][:2]
        return Choice("conv2", c, bm, bn, m)
    bm = block_pixels_v1(cout, m)
    return Choice("conv_nhwc", None, bm, 64 if cout >= 64 else 32 if cout >= 32 else 16, m)


def fwd_choice(case, arith, cfg=0):
    n, cin, h, w, cout, k, stride = case
    oh, ow = out_map(case)
    if _csm_s1(case, arith, cfg) or _csm_s2(case, arith, cfg):
        return Choice("conv_small", None, 16, cout, n * oh * ow)
    return gemm_choice(cin, cout, n * oh * ow, arith, cfg)


def stat_blocks(case, arith, cfg=0):
    """dmc_conv_nhwc_stat_blocks for the shapes that conv_nhwc.hip serves: one row of partials per pixel tile."""
    c = fwd_choice(case, arith, cfg)
    assert c.kernel != "conv_small", case
    return ceil_div(c.m, c.bm)


def dgrad_choices(case, arith, cfg=0):
    """One launch per parity class (py, px) of the input map: the GEMM contracts over Cout and produces Cin channels.
    [(py, px, taps, Choice)]"""
    n, cin, h, w, cout, k, stride = case
    pad = k // 2
    if _csm_s1(case, arith, cfg) or (_csm_s2(case, arith, cfg) and cfg != 304):
        return [(0, 0, k * k, Choice("conv_small", None, 16, cin, n * h * w))]
    res = []
    for py in range(stride):
        for px in range(stride):
            ohs, ows = ceil_div(h - py, stride), ceil_div(w - px, stride)
            taps = sum(1 for ky in range(k) for kx in range(k) if (py + pad - ky) % stride == 0 and (px + pad - kx) % stride == 0)
            res.append((py, px, taps, gemm_choice(cout, cin, n * ohs * ows, arith, cfg)))
    return res


# ---- weight gradient ---------------------------------------------------------------------------------------------------------------

#: kernel: "wgrad3<s>" | "wgrad2<k,s>" | "generic" | "small" | "conv_small"; r: output rows per step; gpi: steps per image;
#: steps = n * gpi; tiles: 64 x 64 blocks of dw (generic: x taps); groups: workgroups along the pixels (generic: slices);
#: per_group: steps per workgroup; last: steps of the last workgroup
WgradPlan = namedtuple("WgradPlan", "kernel r gpi steps tiles groups per_group last")


def _run_plan(kernel, n, oh, r, cin, cout):
    gpi = ceil_div(oh, r)
    steps = n * gpi
    tiles = (cout // 64) * (cin // 64)
    groups = min(max(256 // tiles, 1), steps)
    per_group = ceil_div(steps, groups)
    groups = ceil_div(steps, per_group)
    return WgradPlan(kernel, r, gpi, steps, tiles, groups, per_group, steps - (groups - 1) * per_group)


def wgrad3_plan(n, oh, ow, cin, cout, stride):
    owp = (ow + 7) & ~7
    xc = (owp - 1) * stride + 3

    def nbytes(r):
        g = r * owp // 8
        dyrows, xr = 16 * ((g + 1) // 2), (r - 1) * stride + 3
        return 2 * (dyrows // 4 + (xr * xc + 3) // 4) * 1024

    r = 1
    for cand in range(1, oh + 1):
        if oh % cand == 0 and cand * owp <= 128 and nbytes(cand) <= 150 * 1024:
            r = cand
    return _run_plan("wgrad3<%d>" % stride, n, oh, r, cin, cout)


def wgrad2_plan(n, oh, ow, cin, cout, k, stride):
    xc = (ow - 1) * stride + k

    def nbytes(r):
        ppad, xr = (r * ow + 3) & ~3, (r - 1) * stride + k
        return 2 * ((ppad + 3) // 4 + (xr * xc + 3) // 4) * 256 * 4

    r = 1
    for cand in range(1, oh + 1):
        if oh % cand == 0 and cand * ow <= 128 and nbytes(cand) <= 150 * 1024:
            r = cand
    return _run_plan("wgrad2<%d,%d>" % (k, stride), n, oh, r, cin, cout)


def wgrad_slices(m, tiles):
    return max(min(ceil_div(768, tiles), ceil_div(m, 1024)), 1)


def wgrad_plan(case, arith, cfg=0):
    """The kernel dmc_conv_nhwc_wgrad launches and its plan."""
    n, cin, h, w, cout, k, stride = case
    oh, ow = out_map(case)
    if _csm_s1(case, arith, cfg) and cfg != 302:
        return WgradPlan("conv_small", None, None, None, None, None, None, None)
    if arith == 1 and cfg not in (301, 302) and cin in (16, 32) and cout == 2 * cin and k == 3 and stride == 2 and h % 2 == 0 and w % 2 == 0:
        return WgradPlan("conv_small", None, None, None, None, None, None, None)
    if cin in (16, 32) and k == 3:
        return WgradPlan("small", None, None, None, None, None, None, None)
    if arith == 1 and cin % 64 == 0 and cout % 64 == 0 and k == 3:
        return wgrad3_plan(n, oh, ow, cin, cout, stride)
    if cin % 64 == 0 and cout % 64 == 0 and ow >= 2:
        return wgrad2_plan(n, oh, ow, cin, cout, k, stride)
    tiles = ceil_div(cout, 64) * ceil_div(cin, 64) * k * k
    ns = wgrad_slices(n * oh * ow, tiles)
    return WgradPlan("generic", None, None, None, tiles, ns, None, None)


def wgrad_bytes(case, arith, cfg=0):
    """dmc_conv_nhwc_wgrad_bytes for the shapes of the row-walking and the generic kernels: the partials of `groups` workgroups
    (none where one workgroup writes dw itself) plus 16 bytes."""
    n, cin, h, w, cout, k, stride = case
    p = wgrad_plan(case, arith, cfg)
    assert p.kernel not in ("conv_small", "small"), case
    return (p.groups if p.groups > 1 else 0) * cout * k * k * cin * 4 + 16


def crosses_images(p):
    """How many workgroups' runs of consecutive steps pass from one image (step // gpi) to the next."""
    runs = [(g * p.per_group, min((g + 1) * p.per_group, p.steps) - 1) for g in range(p.groups)]
    return sum(1 for first, last in runs if first // p.gpi != last // p.gpi)


# ---- the cases ---------------------------------------------------------------------------------------------------------------------

#: ragged shapes of the tile-configuration sweep: M = 297 (two 256-pixel tiles, the second with 41 pixels; five 64-pixel tiles;
#: tiles crossing rows and images; Cout % 256 == 0, so configuration 3 is accepted), M = 70 with four data-gradient parity classes
#: of 1, 2, 2 and 4 taps, a 1 x 1 / stride-2 convolution, 64 output channels, where only configurations 1 and 5 are honoured,
#: and 32 input channels, which conv3_kernel does not take
CFG_SHAPES = [
    (3, 256, 11, 9, 256, 3, 1),
    (2, 256, 13, 10, 256, 3, 2),
    (2, 128, 9, 7, 256, 1, 2),
    (3, 128, 11, 9, 64, 3, 1),
    (5, 32, 15, 14, 64, 3, 2),          # the 32 -> 64 / 2 discriminator block: conv2_kernel in BOTH arithmetics (M = 280), and its
]                                       # data gradient, 32 output channels, on conv2 configuration 0
V3_FORCED = [c for c in range(1, 14) if c != 11]           # conv_arith = 1
V2_FORCED = list(range(1, 9))                               # conv_arith = 0


def launches(shape, arith, cfg=0):
    """Every launch of the forward and of the data gradient: [Choice]"""
    return [fwd_choice(shape, arith, cfg)] + [c for _, _, _, c in dgrad_choices(shape, arith, cfg)]


def cfg_sweep():
    """[(shape, arith, cfg)]: the automatic choice of every shape, and every forced value (1 .. 13 without 11 under bf16x3, 1 .. 8
    under fp32 MFMA) that changes a launch of the forward or the data gradient; a value that changes none -- not honoured for
    either channel count, or equal to the automatic choice -- would run the automatic launches again."""
    res = []
    for shape in CFG_SHAPES:
        for arith, forced in ((1, V3_FORCED), (0, V2_FORCED)):
            res.append((shape, arith, 0))
            res += [(shape, arith, c) for c in forced if launches(shape, arith, c) != launches(shape, arith, 0)]
    return res


def swept_configurations():
    """{"conv3" | "conv2": configurations that some forward or data-gradient launch of the sweep takes}"""
    seen = {"conv3": set(), "conv2": set(), "conv_nhwc": set()}
    for shape, arith, cfg in cfg_sweep():
        for c in launches(shape, arith, cfg):
            seen[c.kernel].add(c.cfg)
    return seen


#: weight-gradient runs of several steps: case -> (kernel under conv_arith = 1, steps, groups, per_group, steps of the last group)
WGRAD_RUNS = {
    (11, 512, 7, 7, 512, 3, 1): ("wgrad3<1>", 11, 4, 3, 2),
    (25, 256, 14, 14, 256, 3, 1): ("wgrad3<1>", 50, 13, 4, 2),          # every run crosses images
    (10, 64, 56, 56, 64, 3, 1): ("wgrad3<1>", 560, 187, 3, 2),          # R = 1
    (21, 128, 28, 28, 128, 3, 1): ("wgrad3<1>", 294, 59, 5, 4),         # R = 2
    (10, 64, 56, 56, 128, 3, 2): ("wgrad3<2>", 280, 94, 3, 1),
    (9, 256, 14, 14, 512, 3, 2): ("wgrad3<2>", 63, 8, 8, 7),            # R = 1
    (55, 64, 28, 28, 128, 3, 2): ("wgrad3<2>", 385, 97, 4, 1),          # R = 2, as the 240-frame discriminator block
    (20, 128, 28, 28, 256, 1, 2): ("wgrad2<1,2>", 140, 28, 5, 5),
    (3, 256, 13, 10, 512, 1, 1): ("wgrad2<1,1>", 39, 8, 5, 4),          # the 1 x 1 / stride-1 kernel, R = 1
}
WGRAD_RUN_CASES = list(WGRAD_RUNS)
#: the 3 x 3 cases run again under conv_arith = 0: conv_wgrad2_kernel<3,1> and <3,2>, whose plans differ (no padding of the row to
#: eight pixels: R = 4 at 28 x 28, R = 7 on the 7 x 7 output of the 14 x 14 stride-2 case).  That last case comes to 9 steps in
#: 5 groups of 2 there, so it has a sibling of 20 images: 20 steps of 7 rows in 7 groups of 3, the last of 2
WGRAD2_S2_R7_CASE = (20, 256, 14, 14, 512, 3, 2)
WGRAD_RUN_SWEEP = [(c, 1) for c in WGRAD_RUN_CASES] + [(c, 0) for c in WGRAD_RUN_CASES if c[5] == 3] + [(WGRAD2_S2_R7_CASE, 0)]

#: code no other test reaches: the generic conv_wgrad_kernel with three slices and its reduce; M = 32768, where forward and data
#: gradient take conv_nhwc_kernel<128, 64, 16, ..>
GENERIC_SPLIT_CASE = (3, 48, 28, 28, 80, 3, 1)
V1_LARGE_CASE = (1, 48, 128, 256, 80, 3, 1)
#: 48 output channels: the first-generation 128 x 32 tile with a statistics row per tile (M = 297: three rows)
V1_48_CASE = (3, 48, 11, 9, 48, 3, 1)

#: production: the discriminator's NHWC blocks at 240 frames and the classifier's (ResNet-18) convolutions at 120 frames
PRODUCTION_DISC = [
    (240, 32, 56, 56, 64, 3, 2),
    (240, 64, 28, 28, 64, 3, 1),
    (240, 64, 28, 28, 128, 3, 2),
    (240, 128, 14, 14, 128, 3, 1),
]
PRODUCTION_CLS = [
    (120, 64, 56, 56, 64, 3, 1),        # layer1
    (120, 64, 56, 56, 128, 3, 2),       # layer2.0.conv1
    (120, 64, 56, 56, 128, 1, 2),       # layer2.0.downsample
    (120, 128, 28, 28, 128, 3, 1),
    (120, 256, 14, 14, 256, 3, 1),
    (120, 512, 7, 7, 512, 3, 1),
    (120, 256, 14, 14, 512, 3, 2),
    (120, 128, 28, 28, 256, 1, 2),      # layer3.0.downsample
]
PRODUCTION = PRODUCTION_DISC + PRODUCTION_CLS
