"""EstimatorDenseNet / EstimatorDenseNetSmall (code/dmcnet/model.py:122-170) in TRAINING, whole-network forward + backward on 224^2
frames at 24 and at 6 frames: this package's route (DMC_DENSE_TRAIN=1: ops.dense_train -- the forward of csrc/dense_eval.hip with the
feature buffer kept, the backward of csrc/dense_train.hip in a second buffer) against the stock PyTorch-ROCm modules
(DMC_DENSE_TRAIN=0: six convolutions, five concatenations and autograd's saved tensors -- the route of the parent commit), as
alternating pairs in one process; torch.cuda.max_memory_allocated of a step of either route; then every launch of the route's
backward on its own.  The stock side at 48 frames and beyond is not measured (its concatenation passes 4 GiB).

Seeded Gaussian weights (tests/dense_ref.py), seeded standard-normal inputs and output gradients; the input requires a gradient.
Warm-up first, then ``--pairs`` alternating pairs of ``--iters`` steps per route, timed with device events; the median over the
pairs is reported.  Whole-network times include the route's per-call weight permutation, packs and the gradient map.  Per
launch: ms and, for the matrix-core launches, TFLOP/s fp32-equivalent of the PADDED shape (2 x 9 K R per pixel) and its fraction of
the bf16x3 bound (2,500 / 6 = 416.7 TFLOP/s).  Prints ONE JSON line (``--out FILE`` also writes it).

    python tools/dense_train_bench.py [--frames 24,6] [--warmup 2] [--iters 2] [--pairs 5] [--out FILE]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

BOUND = 2500.0 / 6.0          # TFLOP/s of fp32-equivalent work at six bf16 MFMAs per product


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", default="24,6")
    ap.add_argument("--size", type=int, default=224)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--iters", type=int, default=2)
    ap.add_argument("--pairs", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import numpy as np
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("dense_train_bench: needs a GPU (no CPU timing)")
    from dmcnet_amd import _lib, model, ops
    from tests import dense_ref as D
    dev = torch.device("cuda", 0)
    lib = _lib.load()
    h = w = args.size

    def timed(fn, reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) / reps

    def step(net, x, dout, on):
        model.DENSE_TRAIN = on
        net.zero_grad(set_to_none=True)
        x.grad = None
        out = net(x)
        out.backward(dout)
        return out

    def grads(net, x):
        return [p.grad.detach().clone() for p in net.parameters()] + [x.grad.detach().clone()]

    rows = []
    for name, cls in (("DenseNet", model.EstimatorDenseNet), ("DenseNetSmall", model.EstimatorDenseNetSmall)):
        net = D.load_into(cls(), name).to(dev).train()
        macs = 9 * sum(c.in_channels * c.out_channels for c in [getattr(net, "conv_%d" % i)[0] for i in range(net.depth)] + [net.predict_flow])
        for frames in [int(f) for f in args.frames.split(",")]:
            gen = torch.Generator(device=dev).manual_seed(5)
            x = torch.randn((frames, 5, h, w), generator=gen, device=dev).requires_grad_(True)
            dout = torch.randn((frames, 2, h, w), generator=gen, device=dev)
            row = {"network": name, "what": "whole network, forward + backward", "frames": frames}
            if frames >= 48:
                step(net, x, dout, True)
                row.update({"ours_ms": round(timed(lambda: step(net, x, dout, True), args.iters), 3), "stock_ms": "not measured (past 4 GiB)"})
                rows.append(row)
                continue
            peak = {}
            got = {}
            for on in (True, False):
                step(net, x, dout, on)                             # (first call: MIOpen's search, the allocator's growth)
                torch.cuda.synchronize()
                torch.cuda.reset_peak_memory_stats()
                base = torch.cuda.memory_allocated()
                y = step(net, x, dout, on)
                torch.cuda.synchronize()
                peak[on] = torch.cuda.max_memory_allocated() - base
                got[on] = [y.detach().clone()] + grads(net, x)
            agree = max(float((a - b).abs().max() / b.abs().max().clamp_min(1e-30)) for a, b in zip(got[True], got[False]))
            del got
            for _ in range(args.warmup):
                step(net, x, dout, True), step(net, x, dout, False)
            torch.cuda.synchronize()
            ours, stock = [], []
            for p in range(args.pairs):
                for which in ((True, False) if p % 2 == 0 else (False, True)):
                    (ours if which else stock).append(timed(lambda: step(net, x, dout, which), args.iters))
            flop = 3 * 2.0 * macs * frames * h * w                 # forward, data gradient, weight gradient
            o, s = float(np.median(ours)), float(np.median(stock))
            row.update({"gflop": round(flop / 1e9, 1), "ours_ms": round(o, 3), "stock_ms": round(s, 3), "stock_over_ours": round(s / o, 3),
                        "ours_ms_all": [round(v, 3) for v in ours], "stock_ms_all": [round(v, 3) for v in stock],
                        "ours_tflops": round(flop / o / 1e9, 1), "stock_tflops": round(flop / s / 1e9, 1),
                        "ours_peak_bytes_above_start": int(peak[True]), "stock_peak_bytes_above_start": int(peak[False]),
                        "worst_rel_err_ours_vs_stock": agree})
            rows.append(row)
            net.zero_grad(set_to_none=True)
            del x, dout
            torch.cuda.empty_cache()
        # every launch of the route's backward, on the first batch size
        model.DENSE_TRAIN = False
        frames = int(args.frames.split(",")[0])
        lay = ops.dense_eval_layout(D.WIDTHS[name])
        ct = lay["ct"]
        convs, head = ops._dense_plan(net)
        st = ops._stream()
        px = frames * h * w
        with torch.no_grad():
            feat = torch.randn((frames, h, w, ct), device=dev)
            G = torch.empty((frames, h, w, ct), device=dev)
            dout = torch.randn((frames, 2, h, w), device=dev)
            dx = torch.empty((frames, 5, h, w), device=dev)

        def launch_row(what, k, r, fn, mfma=False):
            _lib.check(fn(), what)
            ms = timed(fn, 5)
            r_ = {"network": name, "what": what, "frames": frames, "K": k, "R": r, "ours_ms": round(ms, 4)}
            if mfma:
                tf = 2.0 * 9 * k * r * px / (ms * 1e-3) / 1e12
                r_["ours_tflops_padded"] = round(tf, 1)
                r_["share_of_bf16x3_bound"] = round(tf / BOUND, 4)
            rows.append(r_)

        hk, _, hindex = lay["head"]
        hw_, _ = ops._dense_weight(head, hk, 2, hindex)
        dwh, dbh = torch.empty((2, 3, 3, ct), device=dev), torch.empty((2,), device=dev)
        launch_row("head dgrad", hk, 2, lambda: lib.dmc_densetrain_head_dgrad(_lib.ptr(dout), _lib.ptr(hw_), _lib.ptr(G), frames, h, w, ct, st))
        work = torch.empty(lib.dmc_densetrain_head_workspace_bytes(frames, h, w, ct), dtype=torch.uint8, device=dev)
        launch_row("head wgrad", hk, 2, lambda: lib.dmc_densetrain_head_wgrad(_lib.ptr(dout), _lib.ptr(feat), _lib.ptr(dwh), _lib.ptr(dbh), _lib.ptr(work),
                                                                               frames, h, w, ct, st))
        for conv, (k, r, index) in reversed(list(zip(convs, lay["layers"]))):
            wp, _ = ops._dense_weight(conv, k, r, index)
            db, dw = torch.empty((r,), device=dev), torch.empty((r, 3, 3, k), device=dev)
            work = torch.empty(lib.dmc_densetrain_mask_workspace_bytes(frames, h, w, r), dtype=torch.uint8, device=dev)
            launch_row("mask", k, r, lambda: lib.dmc_densetrain_mask(_lib.ptr(feat), _lib.ptr(G), _lib.ptr(db), _lib.ptr(work), frames, h, w, ct, k, r, st))
            work = torch.empty(lib.dmc_densetrain_wgrad_workspace_bytes(frames, h, w, k, r), dtype=torch.uint8, device=dev)
            launch_row("layer wgrad", k, r, lambda: lib.dmc_densetrain_layer_wgrad(_lib.ptr(feat), _lib.ptr(G), _lib.ptr(dw), _lib.ptr(work), frames, h, w,
                                                                                    ct, k, r, st), mfma=True)
            rows[-1]["workspace_bytes"] = int(work.numel())
            packs = ops._dense_dgrad_packs(wp, k, r)

            def dgrad():
                rc = 0
                for c0, cb, pack in packs:
                    rc = rc or lib.dmc_densetrain_layer_dgrad(_lib.ptr(G), _lib.ptr(pack), frames, h, w, ct, k, r, c0, cb, st)
                return rc
            launch_row("layer dgrad (%d blocks)" % len(packs), k, r, dgrad, mfma=True)
            del work, dw
        launch_row("export", 0, 0, lambda: lib.dmc_densetrain_export(_lib.ptr(G), _lib.ptr(dx), frames, h, w, ct, st))
        del feat, G, dout, dx
        torch.cuda.empty_cache()
    res = {"tool": "dense_train_bench", "device": torch.cuda.get_device_name(0), "size": args.size, "bf16x3_bound_tflops": round(BOUND, 1),
           "warmup": args.warmup, "iters": args.iters, "pairs": args.pairs, "rows": rows}
    line = json.dumps(res, sort_keys=True)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
