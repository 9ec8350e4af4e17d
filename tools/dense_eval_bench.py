"""Eval-mode EstimatorDenseNet / EstimatorDenseNetSmall (code/dmcnet/model.py:122-170; model.eval() + no_grad) on the evaluator's
batch (25 frames at 224^2) and on a 6-frame batch: this package's route (DMC_DENSE_EVAL=1: one feature buffer, one launch per layer,
csrc/dense_eval.hip) against the stock PyTorch-ROCm modules (DMC_DENSE_EVAL=0: six convolutions and five concatenations -- the route
of the parent commit), as alternating pairs in one process; then every launch of the route on its own, and the route alone on the
10-crop batch of 250 frames (EstimatorDenseNet; the stock route's concatenation passes 4 GiB there and is not timed).

Seeded Gaussian weights (tests/dense_ref.py), seeded standard-normal inputs.  Warm-up first, then ``--pairs`` alternating pairs of
``--iters`` runs per route, timed with device events; the median over the pairs is reported.  Whole-network times include the
route's per-call weight permutation and split.  Per launch: ms, TFLOP/s fp32-equivalent of the PADDED shape (2 x 9 K R per pixel)
and its fraction of the bf16x3 bound (2,500 / 6 = 416.7 TFLOP/s).  Prints ONE JSON line (``--out FILE`` also writes it).

    python tools/dense_eval_bench.py [--frames 25,6] [--warmup 3] [--iters 3] [--pairs 5] [--out FILE]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

BOUND = 2500.0 / 6.0          # TFLOP/s of fp32-equivalent work at six bf16 MFMAs per product


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", default="25,6")
    ap.add_argument("--size", type=int, default=224)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--pairs", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import numpy as np
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("dense_eval_bench: needs a GPU (no CPU timing)")
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

    def run(net, x, on):
        model.DENSE_EVAL, model.DENSE_EVAL_ALL = on, on
        with torch.no_grad():
            return net(x)

    rows = []
    for name, cls in (("DenseNet", model.EstimatorDenseNet), ("DenseNetSmall", model.EstimatorDenseNetSmall)):
        net = D.load_into(cls(), name).to(dev).eval()
        macs = 9 * sum(c.in_channels * c.out_channels for c in [getattr(net, "conv_%d" % i)[0] for i in range(net.depth)] + [net.predict_flow])
        for frames in [int(f) for f in args.frames.split(",")]:
            x = torch.randn((frames, 5, h, w), generator=torch.Generator(device=dev).manual_seed(5), device=dev)
            y_ours, y_stock = run(net, x, True), run(net, x, False)
            agree = float((y_ours - y_stock).abs().max() / y_stock.abs().max())
            for _ in range(args.warmup):
                run(net, x, True), run(net, x, False)
            torch.cuda.synchronize()
            ours, stock = [], []
            for p in range(args.pairs):
                for which in ((True, False) if p % 2 == 0 else (False, True)):
                    (ours if which else stock).append(timed(lambda: run(net, x, which), args.iters))
            flop = 2.0 * macs * frames * h * w
            o, s = float(np.median(ours)), float(np.median(stock))
            rows.append({"network": name, "what": "whole network", "frames": frames, "gflop": round(flop / 1e9, 1), "ours_ms": round(o, 3),
                         "stock_ms": round(s, 3), "stock_over_ours": round(s / o, 3), "ours_ms_all": [round(v, 3) for v in ours],
                         "stock_ms_all": [round(v, 3) for v in stock], "ours_tflops": round(flop / o / 1e9, 1), "stock_tflops": round(flop / s / 1e9, 1),
                         "rel_err_ours_vs_stock": agree})
            del x
        # every launch of the route, on the first batch size
        frames = int(args.frames.split(",")[0])
        lay = ops.dense_eval_layout(D.WIDTHS[name])
        ct = lay["ct"]
        convs, head = ops._dense_plan(net)
        st = ops._stream()
        px = frames * h * w
        x = torch.randn((frames, 5, h, w), device=dev)
        feat = torch.empty((frames, h, w, ct), device=dev)
        out = torch.empty((frames, 2, h, w), device=dev)

        def launch_row(what, k, r, fn):
            _lib.check(fn(), what)
            ms = timed(fn, 10)
            r_ = {"network": name, "what": what, "frames": frames, "K": k, "R": r, "ours_ms": round(ms, 4)}
            if what in ("layer", "head"):                          # (the pack and the ingest do no per-pixel arithmetic to rate)
                tf = 2.0 * 9 * k * r * px / (ms * 1e-3) / 1e12
                r_["ours_tflops_padded"] = round(tf, 1)
                if what == "layer":
                    r_["share_of_bf16x3_bound"] = round(tf / BOUND, 4)
            rows.append(r_)

        launch_row("ingest", 0, 0, lambda: lib.dmc_dense_ingest(_lib.ptr(x), _lib.ptr(feat), frames, h, w, ct, st))
        for conv, (k, r, index) in zip(convs, lay["layers"]):
            wp, bp = ops._dense_weight(conv, k, r, index)
            pack = torch.empty(lib.dmc_dense_wpack_bytes(k, r), dtype=torch.uint8, device=dev)
            launch_row("pack", k, r, lambda: lib.dmc_dense_pack_weights(_lib.ptr(wp), _lib.ptr(pack), k, r, st))
            launch_row("layer", k, r, lambda: lib.dmc_dense_layer_eval(_lib.ptr(feat), _lib.ptr(pack), _lib.ptr(bp), frames, h, w, ct, k, r, st))
        hk, _, hindex = lay["head"]
        hw_, hb = ops._dense_weight(head, hk, 2, hindex)
        launch_row("head", hk, 2, lambda: lib.dmc_dense_head_eval(_lib.ptr(feat), _lib.ptr(hw_), _lib.ptr(hb), _lib.ptr(out), frames, h, w, ct, hk, st))
        del x, feat, out
        if name == "DenseNet":
            x = torch.randn((250, 5, h, w), device=dev)
            run(net, x, True)
            ms = timed(lambda: run(net, x, True), 2)
            rows.append({"network": name, "what": "whole network, route only", "frames": 250, "ours_ms": round(ms, 2),
                         "frame_ranges": len(ops.dense_eval_chunks(250, h, w, ct))})
            del x
        torch.cuda.empty_cache()
    res = {"tool": "dense_eval_bench", "device": torch.cuda.get_device_name(0), "size": args.size, "bf16x3_bound_tflops": round(BOUND, 1),
           "warmup": args.warmup, "iters": args.iters, "pairs": args.pairs, "rows": rows}
    line = json.dumps(res, sort_keys=True)
    print(line, flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
