"""Shapes at which the persistent small-channel kernels of conv_small.hip WALK: a wave (or workgroup) visits several 16-pixel
tiles, so the register double buffer, its prefetch, the mid-iteration break and the accumulation across visits all run
(tests/test_csm_walk_gpu.py).  With a plain restatement of the launch geometry of conv_small.hip (csm_stat_blocks,
csm_fwd_s2_stat_blocks, the csm_dgrad_s2 grid, csm_wgrad_groups, csm_wgrad_s2_groups), so that what each shape reaches can be
checked without a GPU (tests/test_csm_walk_cpu.py)."""
from collections import namedtuple

# (N, Cin, H, W, Cout, stride) of a 3x3 / padding-1 convolution.  Every tile count is odd (the last tile pair of the weight
# gradients is half empty), every row ends in a partial 16-pixel segment, and the images are short and many: the image index
# (and with it the keep-mask row) changes between the visits of one wave.
WALK_CASES = [
    (41, 16, 173, 38, 16, 1),     # 21,279 tiles: 2-3 per wave forward, 3-4 pairs per wave in the weight gradient
    (41, 16, 173, 70, 16, 1),     # 35,465 tiles: 4-5 per wave (two full rounds of the double buffer), 5-6 pairs
    (81, 32, 173, 38, 32, 1),     # 42,039 tiles: 2-3 per wave (eight waves per workgroup), 20-21 pairs
    (41, 16, 346, 76, 32, 2),     # 21,279 output tiles: 2-3 per wave (csm_conv_s2, csm_dgrad_s2), 20-21 pairs per workgroup
    (25, 32, 58, 76, 64, 2),      # 2,175 output tiles: generic forward / data gradient, 4-5 pairs per workgroup (csm_wgrad_s2<32>)
]

# the visits the table of DESIGN promises per case: (forward / data gradient, weight gradient); None = not a conv_small.hip kernel
WALK_VISITS = {
    WALK_CASES[0]: ((2, 3), (3, 4)),
    WALK_CASES[1]: ((4, 5), (5, 6)),
    WALK_CASES[2]: ((2, 3), (20, 21)),
    WALK_CASES[3]: ((2, 3), (20, 21)),
    WALK_CASES[4]: (None, (4, 5)),
}

# kernel: name in conv_small.hip; units: tiles (forward, data gradient) or tile pairs (weight gradient); grid: workgroups;
# cap: the largest grid the launch takes; per_group: walkers per workgroup (waves, or 1 where a whole workgroup walks);
# vmin, vmax: fewest / most units one walker visits
Plan = namedtuple("Plan", "kernel tiles units grid cap per_group vmin vmax")


def out_map(h, w, stride):
    """(OH, OW) of the 3x3 / padding-1 convolution."""
    return (h + 2 - 3) // stride + 1, (w + 2 - 3) // stride + 1


def tile_count(n, h, w, stride=1):
    """16-pixel row segments of the OUTPUT map (the stride-2 kernels tile the output)."""
    oh, ow = out_map(h, w, stride)
    return n * oh * ((ow + 15) // 16)


def _plan(kernel, tiles, units, cap, per_group):
    grid = min(max(-(-units // per_group), 1), cap)
    walkers = grid * per_group
    # walker i takes units i, i + walkers, ..: the first units % walkers walkers make one visit more
    return Plan(kernel, tiles, units, grid, cap, per_group, units // walkers, -(-units // walkers))


def _s1(cin, cout, stride):
    return stride == 1 and cin == cout and cin in (16, 32)


def _s2_even(h, w, stride):
    return stride == 2 and h % 2 == 0 and w % 2 == 0


def fwd_plan(case):
    """csm_conv_kernel<C> (csm_stat_blocks) or csm_conv_s2_kernel (csm_fwd_s2_stat_blocks); None: another file's kernel."""
    n, cin, h, w, cout, stride = case
    tiles = tile_count(n, h, w, stride)
    if _s1(cin, cout, stride):
        return _plan("csm_conv<%d>" % cin, tiles, tiles, 2048, 4 if cin == 16 else 8)
    if _s2_even(h, w, stride) and (cin, cout) == (16, 32):
        return _plan("csm_conv_s2", tiles, tiles, 2048, 4)
    return None


def dgrad_plan(case):
    """csm_conv_kernel<C> on dy (stride 1: the map of dy is the map of x) or csm_dgrad_s2_kernel (tiles of the dy map)."""
    n, cin, h, w, cout, stride = case
    tiles = tile_count(n, h, w, stride)
    if _s1(cin, cout, stride):
        return _plan("csm_conv<%d>" % cin, tiles, tiles, 2048, 4 if cin == 16 else 8)
    if _s2_even(h, w, stride) and (cin, cout) == (16, 32):
        return _plan("csm_dgrad_s2", tiles, tiles, 2048, 4)
    return None


def wgrad_plan(case):
    """csm_wgrad_kernel<C> (csm_wgrad_groups: four waves walk pairs) or csm_wgrad_s2_kernel<Cin> (csm_wgrad_s2_groups: a
    workgroup walks pairs)."""
    n, cin, h, w, cout, stride = case
    tiles = tile_count(n, h, w, stride)
    pairs = (tiles + 1) // 2
    if _s1(cin, cout, stride):
        return _plan("csm_wgrad<%d>" % cin, tiles, pairs, 768 if cin == 16 else 256, 4)
    if _s2_even(h, w, stride) and cin in (16, 32) and cout == 2 * cin:
        return _plan("csm_wgrad_s2<%d>" % cin, tiles, pairs, 512 if cin == 16 else 256, 1)
    return None


def plans(case):
    """{"fwd" | "dgrad" | "wgrad": Plan or None}"""
    return {"fwd": fwd_plan(case), "dgrad": dgrad_plan(case), "wgrad": wgrad_plan(case)}


def wgrad_workspace_bytes(case):
    """dmc_conv_nhwc_wgrad_bytes for the small-channel 3x3 shapes: room for 512 partials of the fp32-MFMA form or for the
    stride-1 bf16x3 kernel's groups on the INPUT map, whichever is more, plus 16 bytes."""
    n, cin, h, w, cout, _ = case
    pairs = (n * h * ((w + 15) // 16) + 1) // 2
    groups = min(max(-(-pairs // 4), 1), 768 if cin == 16 else 256)
    return max(512, groups) * cout * 9 * cin * 4 + 16


def visit_of(tile, plan):
    """Which visit of its walker a tile (forward, data gradient) is: 0 = the tile the prologue loaded."""
    return tile // (plan.grid * plan.per_group)


def tile_coords(tile, case):
    """(image, row, segment) of an output tile."""
    n, _, h, w, _, stride = case
    oh, ow = out_map(h, w, stride)
    segs = (ow + 15) // 16
    row, seg = divmod(tile, segs)
    img, y = divmod(row, oh)
    return img, y, seg
