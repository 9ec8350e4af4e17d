"""Shapes for the transfer-address tests of the weight-gradient kernels (tests/test_x3s_wgrad_addr_gpu.py), with a plain
restatement of the launch plans of conv_x3s.hip (x3s_wgrad_plan) and conv_x3q.hip (q_wgrad_plan), so that what each shape
covers can be checked without a GPU (tests/test_x3s_wgrad_addr_cpu.py)."""

# (n, cin, h, w, cout) of a 3x3 / stride-1 / padding-1 convolution.  The kernels walk padded image rows (h + 2 per image) in
# groups of R rows: R = 1 / 2 / 4 / 9 for w = 56 / 28 / 14 / 7, (h + 2) % R == 0, w = 7 only with h = 7.
X3S_ADDR_CASES = [
    # w = 56
    (1, 64, 3, 56, 64),          # one image of three rows: every step touches a pad row
    (1, 64, 56, 56, 64),
    (3, 64, 56, 56, 128),        # odd N, two co tiles
    (5, 64, 55, 56, 64),         # 285 steps in 143 groups: the last group runs one step
    (2, 128, 8, 56, 64),         # two ci tiles
    # w = 28
    (1, 64, 28, 28, 64),
    (7, 64, 10, 28, 64),         # odd N, H != W
    (2, 64, 30, 28, 64),         # H > W
    (3, 128, 28, 28, 192),       # 2 x 3 tiles, 45 steps in 23 groups
    # w = 14
    (1, 64, 14, 14, 64),
    (2, 64, 10, 14, 64),
    (3, 64, 6, 14, 64),          # images of two groups
    (1, 64, 2, 14, 64),          # an image is ONE group: pad row, two rows, pad row
    (5, 256, 14, 14, 128),       # 4 x 2 tiles
    (43, 128, 14, 14, 128),      # 172 steps in 58 groups of three: the last group runs one step
    # w = 7: a group is a whole padded image
    (1, 64, 7, 7, 64),
    (3, 64, 7, 7, 64),
    (7, 64, 7, 7, 128),
    (5, 512, 7, 7, 512),         # 5 steps in 3 groups
    (41, 256, 7, 7, 128),        # 41 steps in 21 groups
]

# (n, cin, h, w, cout) of the stride-2 block pairs of layer2.0 / layer3.0 / layer4.0 (3x3 / stride 2 + 1x1 / stride 2 shortcut)
X3Q_ADDR_CASES = [(n, cin, hw, hw, 2 * cin) for cin, hw in ((64, 56), (128, 28), (256, 14)) for n in (1, 3, 7)]


def x3s_plan(n, h, w, cin, cout):
    """dict(R, steps, tiles, groups, per_group) of x3s_wgrad_plan, or None where it refuses the shape."""
    r = {56: 1, 28: 2, 14: 4, 7: 9}.get(w, 0)
    if not r or (h + 2) % r or (w == 7 and h != 7) or cin % 64 or cout % 64:
        return None
    steps = n * (h + 2) // r
    tiles = (cout // 64) * (cin // 64)
    groups = min(max(256 // tiles, 1), steps)
    per_group = -(-steps // groups)
    return dict(R=r, steps=steps, tiles=tiles, groups=-(-steps // per_group), per_group=per_group)


def x3q_plan(n, oh, ow, cin, cout):
    """The 3x3 part of q_wgrad_plan (the shortcut's plain GEMM has no row addressing)."""
    geo = {(28, 28): (1, 29), (14, 14): (2, 16), (7, 7): (4, 8)}.get((oh, ow))
    if geo is None or cin % 64 or cout % 64 or n <= 0:
        return None
    r, hp = geo
    steps = n * hp // r
    tiles = (cout // 64) * (cin // 64)
    groups = min(max(256 // tiles, 1), steps)
    per_group = -(-steps // groups)
    return dict(R=r, HP=hp, steps=steps, tiles=tiles, groups=-(-steps // per_group), per_group=per_group)
