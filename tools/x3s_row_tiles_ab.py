#!/usr/bin/env python3
"""A/B of tile configuration 5 of the pre-split convolutions (row-aligned 512-slot tiles, option conv_cfg = 107) against the
choice without it (108) on the ResNet-18 stride-1 shapes: forward with statistics and data gradient, HIP events, the two options
alternating in ONE process, ROUNDS rounds of ITERS launches each.  Prints per shape the median and minimum of both.

    python tools/x3s_row_tiles_ab.py [frames [shape ...]] > profiles/x3s_row_tiles_ab.txt
"""
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import dmcnet_amd
from dmcnet_amd import ops

DEV = "cuda:0"
FRAMES = int(sys.argv[1]) if len(sys.argv) > 1 else 120
SHAPES = [("layer1", 64, 56, 64), ("layer2", 128, 28, 128), ("layer3", 256, 14, 256), ("layer4", 512, 7, 512)]
if len(sys.argv) > 2:                          # only the named shapes
    SHAPES = [s for s in SHAPES if s[0] in sys.argv[2:]]
ROUNDS, ITERS = 7, 20
L, lib = dmcnet_amd._lib, dmcnet_amd._lib.load()


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(ITERS):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / ITERS * 1e3


print("frames %d, %d rounds x %d launches, us per launch: median (min)" % (FRAMES, ROUNDS, ITERS))
print("%-8s %-6s %6s %6s | %18s | %18s | %s" % ("shape", "pass", "wg107", "wg108", "conv_cfg=107", "conv_cfg=108", "107/108"))
for name, cin, hw, cout in SHAPES:
    n = FRAMES
    x = torch.randn(n, cin, hw, hw, device=DEV).contiguous(memory_format=torch.channels_last)
    dy = torch.randn(n, cout, hw, hw, device=DEV).contiguous(memory_format=torch.channels_last)
    w = (torch.randn(cout, cin, 3, 3, device=DEV) * 0.05).contiguous(memory_format=torch.channels_last)
    xs, dys = ops.x3s_split(x), ops.x3s_split(dy)
    wf, wt = ops.x3s_pack_weights(w)
    passes = {"fwd": lambda: ops.x3s_conv_fwd(xs, wf, n, hw, hw, cin, cout, want_stats=True),
              "dgrad": lambda: ops.x3s_conv_dgrad(dys, wt, n, hw, hw, cin, cout)}
    for pname, fn in passes.items():
        t, wgs = {107: [], 108: []}, {}
        for cfg in (107, 108):
            L.check(lib.dmc_set_option(b"conv_cfg", cfg), "dmc_set_option")
            wgs[cfg] = lib.dmc_x3s_conv_stat_blocks(n, hw, hw, cout) * (cout // 64)
            timed(fn)
        for _ in range(ROUNDS):
            for cfg in (107, 108):
                L.check(lib.dmc_set_option(b"conv_cfg", cfg), "dmc_set_option")
                t[cfg].append(timed(fn))
        L.check(lib.dmc_set_option(b"conv_cfg", 0), "dmc_set_option")
        ma, mb = statistics.median(t[107]), statistics.median(t[108])
        print("%-8s %-6s %6d %6d | %8.1f (%7.1f) | %8.1f (%7.1f) | %.3f" % (name, pname, wgs[107], wgs[108], ma, min(t[107]), mb, min(t[108]), ma / mb))
