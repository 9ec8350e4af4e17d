"""The discriminators' two small kernels against the stock route they replace, as alternating A/B pairs in one process.

  head   adv_layer = Linear(C * H * W -> 2) on the NHWC activation (code/dmcnet_GAN/model.py:290,297-298): ``ops.disc_head``
         (csrc/disc_head.hip) against F.linear on a permuted view of the weight (the lines of _DiscriminatorBase.forward with
         model.DISC_HEAD off), at M = 120, 240, 384 frames for (C, H, W) = (128, 14, 14) and (32, 28, 28): forward, forward +
         backward with all three gradients, and forward + backward with the parameters as constants (the G step: dx only).  Each
         time is also given as a rate over the M * C * H * W * 4 bytes it must read (forward), read and write (forward + backward:
         three passes; dx only: two), and as a fraction of ``--hbm-gbps``.
  c8     Discriminator4's Conv2d(8, 16, 3, 2, 1) block at 112 x 112 with its BatchNorm in train mode, forward + backward, M = 120
         and 240: ``ops.disc_block(..., c8=True)`` (csrc/disc_c8.hip) against F.conv2d + ``ops.disc_tail`` with the two layout
         flips the stock route costs around it (NHWC -> NCHW behind the convolution, NCHW -> NHWC in front of the next block).

Seeded inputs; warm-up first (MIOpen's search, the allocator's growth), then ``--pairs`` alternating pairs of ``--iters`` calls per
route, timed with device events; every pair is reported.  "faster_in_every_pair" is what decides model.DISC_HEAD_BY_DEFAULT /
model.DISC_C8_BY_DEFAULT.  Prints ONE JSON line (``--out FILE`` also writes it).

    python tools/disc_head_bench.py [--warmup 3] [--iters 20] [--pairs 3] [--hbm-gbps 8000] [--commit ID] [--out FILE]"""
import argparse
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HEAD_FRAMES = (120, 240, 384)
HEAD_GEOMETRIES = ((128, 14, 14), (32, 28, 28))
C8_FRAMES = (120, 240)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--pairs", type=int, default=3)
    ap.add_argument("--hbm-gbps", type=float, default=8000.0, help="the HBM rate the fractions are taken of")
    ap.add_argument("--commit", default=None, help="the commit the sources were taken from (recorded as given)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import numpy as np
    import torch
    import torch.nn.functional as F
    if not torch.cuda.is_available():
        raise SystemExit("disc_head_bench: needs a GPU (no CPU timing)")
    from dmcnet_amd import build, model, ops
    dev = torch.device("cuda", 0)
    CL = torch.channels_last

    def timed(fn, reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) / reps

    def ab(ours_fn, stock_fn):
        for _ in range(args.warmup):
            ours_fn(), stock_fn()
        torch.cuda.synchronize()
        ours, stock = [], []
        for p in range(args.pairs):
            for which in ((True, False) if p % 2 == 0 else (False, True)):
                (ours if which else stock).append(timed(ours_fn if which else stock_fn, args.iters))
        return ours, stock

    def row(kind, what, frames, geometry, ours, stock, passes, nbytes):
        o, s = float(np.median(ours)), float(np.median(stock))
        r = {"kernel": kind, "workload": what, "frames": frames, "geometry": list(geometry), "ours_ms": round(o, 4), "stock_ms": round(s, 4),
             "stock_over_ours": round(s / o, 3), "ours_ms_pairs": [round(v, 4) for v in ours], "stock_ms_pairs": [round(v, 4) for v in stock],
             "faster_in_every_pair": bool(all(a < b for a, b in zip(ours, stock)))}
        if nbytes:
            r["floor_bytes"] = int(passes * nbytes)
            for tag, t in (("ours", o), ("stock", s)):
                gbps = passes * nbytes / (t * 1e-3) / 1e9
                r[tag + "_gbps"] = round(gbps, 1)
                r[tag + "_fraction_of_hbm"] = round(gbps / args.hbm_gbps, 4)
        print("# %s" % json.dumps(r, sort_keys=True), flush=True)
        return r

    rows = []
    gen = torch.Generator(device=dev).manual_seed(7)
    # ---- head
    for c, h, w in HEAD_GEOMETRIES:
        lin = torch.nn.Linear(c * h * w, 2).to(dev)
        for m in HEAD_FRAMES:
            x = torch.randn((m, h, w, c), generator=gen, device=dev).permute(0, 3, 1, 2).requires_grad_(True)     # channels_last memory
            dv = torch.randn((m, 2), generator=gen, device=dev)
            assert ops.disc_head_supported(x, lin)

            def stock_head():
                n = x.shape[0]
                wp = lin.weight.view(-1, c, h, w).permute(0, 2, 3, 1).reshape(lin.out_features, -1)
                return F.linear(x.permute(0, 2, 3, 1).reshape(n, -1), wp, lin.bias)

            def own_head():
                return ops.disc_head(x, lin.weight, lin.bias)

            def fwd(fn):
                def run():
                    with torch.no_grad():
                        fn()
                return run

            def fwd_bwd(fn, params):
                def run():
                    for p in lin.parameters():
                        p.requires_grad_(params)
                    x.grad = None
                    lin.zero_grad(set_to_none=True)
                    fn().backward(dv)
                return run
            nbytes = m * c * h * w * 4
            for what, mk, passes in (("forward", fwd, 1), ("forward+backward", lambda f: fwd_bwd(f, True), 3),
                                     ("forward+backward dx only", lambda f: fwd_bwd(f, False), 2)):
                ours, stock = ab(mk(own_head), mk(stock_head))
                rows.append(row("head", what, m, (c, h, w), ours, stock, passes, nbytes))
            for p in lin.parameters():
                p.requires_grad_(True)
            del x, dv
    # ---- the 8 -> 16 block
    d4 = model.Discriminator4(2).to(dev).train()
    blk = d4.discriminator_block_2
    conv, bn = blk[0], blk[3]
    for m in C8_FRAMES:
        x = torch.randn((m, 112, 112, 8), generator=gen, device=dev).permute(0, 3, 1, 2).requires_grad_(True)
        keep = (torch.rand((m, 16), generator=gen, device=dev) >= 0.25).float() / 0.75
        dy = torch.randn((m, 56, 56, 16), generator=gen, device=dev).permute(0, 3, 1, 2)
        assert ops.disc_block_supported(x, conv, False, c8=True)

        def own_block():
            return ops.disc_block(x, conv, keep, bn, True, c8=True)

        def stock_block():
            y = F.conv2d(x, conv.weight, conv.bias, conv.stride, conv.padding)
            y = ops.disc_tail(y.contiguous(), keep, bn, True)
            return y.contiguous(memory_format=CL)                     # what the next (NHWC) block does to its input

        def fwd_bwd(fn):
            def run():
                x.grad = None
                d4.zero_grad(set_to_none=True)
                fn().backward(dy)
            return run
        ours, stock = ab(fwd_bwd(own_block), fwd_bwd(stock_block))
        rows.append(row("c8", "block forward+backward", m, (8, 112, 112), ours, stock, 0, 0))
        del x, keep, dy
    digest = hashlib.sha256(json.dumps(build.source_hashes(), sort_keys=True).encode()).hexdigest()
    res = {"tool": "disc_head_bench", "device": torch.cuda.get_device_name(0), "warmup": args.warmup, "iters": args.iters, "pairs": args.pairs,
           "hbm_gbps": args.hbm_gbps, "commit": args.commit, "library_sources_sha256": digest, "rows": rows}
    line = json.dumps(res, sort_keys=True)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
