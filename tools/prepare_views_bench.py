#!/usr/bin/env python3
"""Times the device input preparation's entry points on bench.bench_prepare's shape (120 frames 256 x 340 x 7 uint8 ->
224 x 224 fp32 planes, the copy-crop + flip plans), one HIP-event pair per call, 10 warm-up + 60 timed calls, median:

  * repeat path (flow_ds_factor 16) and copy path (0) through dmc_prepare_inputs_crop  -- the guard for the kernels the
    new entry points share with it; with --ab PARENT_LIB the same lines from a library built from the parent commit, in
    fresh processes alternating A / B / A / B;
  * the same two through dmc_prepare_inputs_views (identity views), and the interpolated path (factor 16) next to them;
  * ten views of 12 frames (120 outputs from 12 uploaded frames) against the crop entry on 120 replicated frames.

    python tools/prepare_views_bench.py [--lib libdmcnet_hip.so] [--ab parent/libdmcnet_hip.so] [--out profiles/r8_prepare_views.json]

One JSON object per line: label, ms (median), min / max ms, GB/s over 7 B per sampled source pixel + 28 B per output pixel,
the sha256 of csrc/prepare.hip the running tree holds and of the library measured."""
import argparse
import ctypes
import hashlib
import json
import os
import random
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
WARMUP, TIMED = 10, 60


def _sha(path):
    with open(path, "rb") as f:
        return hashlib.sha256(f.read()).hexdigest()


def measure(lib_path, tag):
    """Prints and returns the JSON lines of one library."""
    import torch
    from dmcnet_amd import _lib, ops, transforms
    dev = torch.device("cuda", 0)
    lib = ctypes.CDLL(lib_path)
    have_views = hasattr(lib, "dmc_prepare_inputs_views")
    for name in ("dmc_prepare_crop_workspace_bytes", "dmc_prepare_inputs_crop") + \
            (("dmc_prepare_views_workspace_bytes", "dmc_prepare_inputs_views") if have_views else ()):
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = _lib.SIGNATURES[name]
    lib.dmc_last_error.restype = ctypes.c_char_p
    g = torch.Generator(device=dev).manual_seed(7)
    n = 120
    frames = ops.u8_frames_buffer((n, 256, 340, 7), dev)
    frames.copy_(torch.randint(0, 256, frames.shape, generator=g, device=dev, dtype=torch.uint8))
    pipe = transforms.Compose([transforms.GroupCenterCrop(224), transforms.GroupRandomHorizontalFlip()])
    random.seed(11)
    plans, flips = [], []
    for _ in range(n):
        plan, _size, flip = transforms.geometry_plan(pipe, (256, 340))
        plans.append(plan); flips.append(int(flip))
    boxes = torch.tensor(plans, dtype=torch.int32, device=dev)
    fl = torch.tensor(flips, dtype=torch.uint8, device=dev)
    outs = [torch.empty((n, c, 224, 224), dtype=torch.float32, device=dev) for c in (2, 2, 3)]
    work = torch.empty(1 << 20, dtype=torch.float32, device=dev)
    std = torch.tensor(ops._STD, dtype=torch.float64).float()
    std4 = (ctypes.c_float * 4)(float(torch.mean(std)), float(std[0]), float(std[1]), float(std[2]))
    stdp = ctypes.cast(std4, ctypes.c_void_p)
    p = _lib.ptr
    stream = _lib._P(torch.cuda.current_stream().cuda_stream)
    lines = []
    hashes = {"tree_prepare_hip_sha256": _sha(os.path.join(ROOT, "dmc-net_amd", "csrc", "prepare.hip")), "library_sha256": _sha(lib_path),
              "library": tag}

    def crop(fr, bx, flp, factor):
        return lambda: lib.dmc_prepare_inputs_crop(p(fr), p(bx), p(flp), p(outs[0]), p(outs[1]), p(outs[2]), p(work), n, 256, 340,
                                                   224, 224, factor, stdp, stream)

    def views(fr, src, bx, flp, n_src, factor, interp):
        return lambda: lib.dmc_prepare_inputs_views(p(fr), p(src), p(bx), p(flp), p(outs[0]), p(outs[1]), p(outs[2]), p(work), n_src, n,
                                                    256, 340, 224, 224, factor, interp, stdp, stream)

    def run(label, call, src_px):
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(TIMED)]
        for _ in range(WARMUP):
            assert call() == 0, lib.dmc_last_error()
        torch.cuda.synchronize()
        for a, b in ev:
            a.record()
            rc = call()
            b.record()
            assert rc == 0, lib.dmc_last_error()
        torch.cuda.synchronize()
        ms = sorted(a.elapsed_time(b) for a, b in ev)
        med = ms[len(ms) // 2]
        nbytes = 7 * src_px + 28 * n * 224 * 224
        line = dict(label=label, ms=round(med, 4), ms_min=round(ms[0], 4), ms_max=round(ms[-1], 4),
                    GBps=round(nbytes / (med * 1e-3) / 1e9, 1), calls=TIMED, **hashes)
        lines.append(json.dumps(line))
        print(lines[-1], flush=True)

    px = n * 224 * 224
    run("crop_entry_repeat_f16", crop(frames, boxes, fl, 16), px)
    run("crop_entry_copy_f0", crop(frames, boxes, fl, 0), px)
    if not have_views:
        return lines
    run("views_entry_repeat_f16", views(frames, None, boxes, fl, n, 16, 0), px)
    run("views_entry_copy_f0", views(frames, None, boxes, fl, n, 0, 0), px)
    run("views_entry_interp_f16", views(frames, None, boxes, fl, n, 16, 1), px)
    # ten views (GroupOverSample(224, None) on 256 x 340: copies) of 12 frames, in DevicePrep's order, against the crop entry on
    # the same 120 plans over replicated frames.  (One 25-segment video alone -- 250 outputs of 25 frames -- runs ~0.1 ms: too
    # short to time; 12 frames x 10 views fill the same 120 outputs as the lines above.)
    vplans, _out, vflips = transforms.oversample_plans(transforms.GroupOverSample(224, None), (256, 340))
    s = 12
    j = torch.arange(10 * s)
    view, seg = (j // (2 * s)) * 2 + j % 2, (j // 2) % s
    vb = torch.tensor(vplans, dtype=torch.int32)[view].to(dev)
    vf = torch.tensor([int(f) for f in vflips], dtype=torch.uint8)[view].to(dev)
    src = seg.to(torch.int32).to(dev)
    replicated = ops.u8_frames_buffer((n, 256, 340, 7), dev)
    replicated.copy_(frames[:s][seg.to(dev)])
    run("views_10x12_frames_f0", views(frames, src, vb, vf, s, 0, 0), px)
    run("crop_entry_120_replicated_f0", crop(replicated, vb, vf, 0), px)
    run("views_10x12_frames_interp_f16", views(frames, src, vb, vf, s, 16, 1), px)
    run("crop_entry_120_replicated_repeat_f16", crop(replicated, vb, vf, 16), px)
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", default=os.path.join(ROOT, "dmc-net_amd", "libdmcnet_hip.so"))
    ap.add_argument("--ab", default=None, help="a library built from the parent commit: alternate with --lib, twice each")
    ap.add_argument("--out", default=None, help="also write the lines to this file")
    ap.add_argument("--tag", default="this", help=argparse.SUPPRESS)
    args = ap.parse_args()
    lines = []
    if args.ab is None:
        lines = measure(args.lib, args.tag)
    for tag, path in ((("parent", args.ab), ("this", args.lib)) * 2 if args.ab else ()):     # A / B / A / B, a fresh process each
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--lib", path, "--tag", tag], stdout=subprocess.PIPE,
                           text=True, timeout=300)
        sys.stdout.write(r.stdout)
        sys.stdout.flush()
        if r.returncode != 0:
            sys.exit("measurement of %s failed (exit %d); nothing more is started" % (tag, r.returncode))
        lines += [l for l in r.stdout.splitlines() if l.startswith("{")]
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
