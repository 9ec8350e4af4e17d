#!/usr/bin/env python3
"""Times the I3D clip preparation (dmc_prepare_clip) at the recipe's micro-batch -- B = 3 clips, T = 64 frames, decoded at
256 x 340, output 224 x 224 -- in its two forms: training (random crop, flips, flow_ds_factor 16) and validation (centre crop,
no flip, flow_ds_factor 1).

    python tools/clip_prep_bench.py [--out profiles/clip_prep_bench.json] [--pairs 5]

Per form, in ONE process, alternating kernel / stock / kernel / stock ... for ``--pairs`` pairs (each side: warm-up calls, then
one HIP-event pair per call, the median):

  * ``kernel_ms``: ops.prepare_clip into a preallocated output; ``hbm_fraction`` = (7 + 28) * B * T * OH * OW bytes over that
    time, as a fraction of the 8 TB/s HBM peak (for orientation: the 2-D prepare paths sit at 0.63 (copy) and 0.35 (resize));
  * ``stock_ms``: the same transform written in stock PyTorch ops on the same uploaded uint8 tensor (slice, flip, 256 - v,
    permute, padded block sums, float, divide, normalise) -- checked once to give the kernel's tensor bit for bit;
  * ``kernel_below_stock_in_every_pair``: the acceptance condition;
  * end to end, recorded and not gated: pinned uint8 upload + kernel (``e2e_u8_upload_kernel_ms``) against the upload of the
    host-prepared fp32 batch (``e2e_fp32_upload_ms``).

One JSON object per line; ``--out`` also writes them to a file.  Needs a GPU: there is no fallback."""
import argparse
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM_PEAK = 8.0e12


def _sha(path):
    with open(path, "rb") as f:
        return hashlib.sha256(f.read()).hexdigest()


def stock_prepare(clips, plans, size, f, mean, std, out):
    """dmc_prepare_clip's tensor from stock torch ops on the device-resident uint8 clips [B,H0,W0,T*7]."""
    import torch
    oh, ow = size
    t = clips.shape[3] // 7
    m = torch.tensor(mean, dtype=torch.float32, device=clips.device).view(-1, 1, 1, 1)
    s = torch.tensor(std, dtype=torch.float32, device=clips.device).view(-1, 1, 1, 1)
    for b, (y1, x1, flip) in enumerate(plans):
        d = clips[b, y1:y1 + oh, x1:x1 + ow].view(oh, ow, t, 7)
        if flip:
            d = d.flip(1)
            d[..., 0] = (256 - d[..., 0].to(torch.int16)).to(torch.uint8)
            d[..., 2] = (256 - d[..., 2].to(torch.int16)).to(torch.uint8)
        x = d.permute(3, 2, 0, 1)                                    # [7, T, OH, OW]
        o = out[b]
        torch.div(x.float(), 255.0, out=o)
        if f >= 2:
            ph, pw = (-oh) % f, (-ow) % f
            flow = torch.nn.functional.pad(x[:2].to(torch.int32), (0, pw, 0, ph))
            sums = flow.view(2, t, (oh + ph) // f, f, (ow + pw) // f, f).sum(dim=(3, 5))
            means = torch.div(sums, f * f, rounding_mode="floor")
            rep = means.repeat_interleave(f, 2).repeat_interleave(f, 3)[:, :, :oh, :ow]
            torch.div(rep.float(), 255.0, out=o[:2])
        n = len(mean)
        o[:n].sub_(m).div_(s)
    return out


def timed(call, warmup, calls):
    import torch
    for _ in range(warmup):
        call()
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(calls)]
    for a, b in ev:
        a.record()
        call()
        b.record()
    torch.cuda.synchronize()
    ms = sorted(a.elapsed_time(b) for a, b in ev)
    return ms[len(ms) // 2], ms[0], ms[-1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--pairs", type=int, default=5)
    ap.add_argument("--batch", type=int, default=3)
    ap.add_argument("--frames", type=int, default=64)
    args = ap.parse_args()
    import numpy as np
    import torch
    from dmcnet_amd import _lib, i3d_data as D, ops
    if not torch.cuda.is_available():
        sys.exit("clip_prep_bench needs a GPU")
    dev = torch.device("cuda", 0)
    B, T, H0, W0, OH, OW = args.batch, args.frames, 256, 340, 224, 224
    g = torch.Generator(device=dev).manual_seed(7)
    clips = ops.u8_frames_buffer((B, H0, W0, T * 7), dev)
    clips.copy_(torch.randint(0, 256, clips.shape, generator=g, device=dev, dtype=torch.uint8))
    out = torch.empty((B, 7, T, OH, OW), dtype=torch.float32, device=dev)
    out_stock = torch.empty_like(out)
    host_u8 = torch.empty(clips.shape, dtype=torch.uint8).pin_memory()
    host_u8.copy_(clips)
    host_f32 = torch.empty(out.shape, dtype=torch.float32).pin_memory()
    nbytes = 35 * B * T * OH * OW
    hashes = {"clip_prep_hip_sha256": _sha(os.path.join(ROOT, "dmc-net_amd", "csrc", "clip_prep.hip")), "library_sha256": _sha(_lib.LIB_PATH)}
    lines = []
    forms = []
    tf = D.ClipTransform((OH, OW), True, 16, aug_seed=1)
    forms.append(("train_f16", 16, [tf.plan((H0, W0)) for _ in range(B)]))
    tv = D.ClipTransform((OH, OW), False, 1)
    forms.append(("val_f1_centre", 1, [tv.plan((H0, W0)) for _ in range(B)]))
    for label, f, plans in forms:
        plans_dev = torch.tensor(plans, dtype=torch.int32, device=dev)
        kernel = lambda: ops.prepare_clip(clips, plans_dev, (OH, OW), f, D.MEAN, D.STD, out=out)
        stock = lambda: stock_prepare(clips, plans, (OH, OW), f, D.MEAN, D.STD, out_stock)
        kernel()
        stock()
        torch.cuda.synchronize()
        same = bool(torch.equal(out, out_stock))
        pairs = []
        for _ in range(args.pairs):
            k = timed(kernel, 5, 30)
            s = timed(stock, 2, 10)
            pairs.append({"kernel_ms": round(k[0], 4), "kernel_ms_min": round(k[1], 4), "kernel_ms_max": round(k[2], 4),
                          "stock_ms": round(s[0], 4), "stock_ms_min": round(s[1], 4), "stock_ms_max": round(s[2], 4)})
        kmed = sorted(p["kernel_ms"] for p in pairs)[len(pairs) // 2]
        smed = sorted(p["stock_ms"] for p in pairs)[len(pairs) // 2]
        # end to end: what crosses the host link and when the batch is ready on the device
        host_f32.copy_(out)

        def e2e_u8():
            clips.copy_(host_u8, non_blocking=True)
            kernel()

        def e2e_f32():
            out_stock.copy_(host_f32, non_blocking=True)
        eu = timed(e2e_u8, 2, 7)
        ef = timed(e2e_f32, 2, 7)
        line = dict(label=label, B=B, T=T, src=[H0, W0], out=[OH, OW], flow_ds_factor=f, plans=[list(p) for p in plans],
                    kernel_ms=round(kmed, 4), stock_ms=round(smed, 4), stock_over_kernel=round(smed / kmed, 2),
                    hbm_bytes=nbytes, hbm_fraction=round(nbytes / (kmed * 1e-3) / HBM_PEAK, 3),
                    GBps=round(nbytes / (kmed * 1e-3) / 1e9, 1), stock_equals_kernel=same,
                    kernel_below_stock_in_every_pair=all(p["kernel_ms"] < p["stock_ms"] for p in pairs), pairs=pairs,
                    e2e_u8_upload_kernel_ms=round(eu[0], 3), e2e_fp32_upload_ms=round(ef[0], 3),
                    upload_bytes_u8=int(host_u8.numel()), upload_bytes_fp32=int(host_f32.numel() * 4), **hashes)
        lines.append(json.dumps(line))
        print(lines[-1], flush=True)
    if args.out:
        with open(args.out, "w") as fo:
            fo.write("\n".join(lines) + "\n")
    ok = all(json.loads(l)["kernel_below_stock_in_every_pair"] and json.loads(l)["stock_equals_kernel"] for l in lines)
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
