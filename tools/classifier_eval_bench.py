"""Eval-mode DMC-Net classifier on the reference evaluator's recipe batch (code/dmcnet/test.py:139-198: one video = 25 segments x
10 crops = 250 frames at 224^2; DenseNetTiny generator + ResNet-18, 51 classes, model.eval() + no_grad) through
evaluate.forward_video: the one-launch eval route (resnet.EVAL_FUSED = True: BatchNorm, shortcut and ReLU in the epilogue of
every pre-split convolution, the stride-2 pairs on the space-to-depth kernel) against EVAL_FUSED = False (convolution, then a
streaming BatchNorm pass; stride-2 blocks on the in-loop-split kernel) -- the route of the parent commit --, as alternating pairs
in one process.

Seeded weights incl. the running statistics (oracle.dmc_oracle.seeded_state_fill) and seeded inputs.  Per route: warm-up
batches, then `--iters` batches timed with device events per pair.  Prints ONE JSON line: ms per batch and frames/s per route
and pair, the ratio per pair, the fp32 convolution-result traffic the fused route removes (from the shapes) and the time that
traffic would take at the HBM peak, the FLOPs of the 3x3 / 1x1 convolutions of layers 1-4 per batch and the time they take at the
bf16x3 bound (2,500 / 6 TFLOP/s, the roofline arithmetic of bench.py --full), the two routes' score agreement, a sha256 of the sources.
``--routes fused`` runs the eval route only (for a rocprofv3 --kernel-trace --stats run, which also gives the launch count).

    python tools/classifier_eval_bench.py [--frames 250] [--warmup 3] [--iters 20] [--pairs 3] [--out FILE]"""
import argparse
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

BF16X3_PEAK = 2500.0e12 / 6      # fp32-equivalent FLOP/s of six bf16 MFMAs per product block (bench.classifier_conv_roofline)
HBM_PEAK = 8000.0e9


def conv_shapes(hw=224):
    """(outputs per frame of the layer1-4 convolutions whose fp32 result the two-pass route writes and reads back, their MACs)."""
    outs, macs, cin, res = 0, 0, 64, hw // 4
    for i, cout in enumerate((64, 128, 256, 512)):
        if i:
            res //= 2
            macs += res * res * cout * cin * (9 + 1) + 3 * res * res * cout * cout * 9
            outs += 5 * res * res * cout                              # conv1, downsample, conv2, and the second unit's two
        else:
            macs += 4 * res * res * cout * cin * 9
            outs += 4 * res * res * cout
        cin = cout
    return outs, macs


def source_sha():
    import importlib.util
    spec = importlib.util.spec_from_file_location("_dmc_build", os.path.join(ROOT, "dmc-net_amd", "build.py"))
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    h = hashlib.sha256()
    for k, v in sorted(b.source_hashes().items()):
        h.update(("%s %s\n" % (k, v)).encode())
    for f in ("ops.py", "resnet.py", "evaluate.py", "model.py"):
        with open(os.path.join(ROOT, "dmc-net_amd", f), "rb") as fh:
            h.update(hashlib.sha256(fh.read()).hexdigest().encode())
    return h.hexdigest()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=250, help="frames per batch: 25 segments x 10 crops of one video")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--pairs", type=int, default=3)
    ap.add_argument("--routes", default="both", choices=["both", "fused"])
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    args = ap.parse_args()

    import torch
    if not torch.cuda.is_available():
        raise SystemExit("classifier_eval_bench: needs a GPU (no CPU timing)")
    import dmcnet_amd
    from dmcnet_amd import dataset, evaluate, resnet
    from oracle import dmc_oracle as O
    dev = torch.device("cuda", 0)
    m = dmcnet_amd.Model(51, 25, "mv", base_model="resnet18", use_databn=0, gen_flow_or_delta=1, arch_estimator="DenseNetTiny")
    O.seeded_state_fill(m, seed=91)
    m.to(dev).eval()
    inputs = [dataset.synthetic_batch_on_device(92 + k, 1, args.frames, 51, dev)[1:3] for k in range(2)]
    routes = [True, False] if args.routes == "both" else [True]

    def run(fused, k):
        resnet.EVAL_FUSED = fused
        mv, res = inputs[k % 2]
        return evaluate.forward_video(m, mv, res, args.frames, 1)     # [1, frames, C, H, W]: one video, segments x crops

    for fused in routes:                                              # warm-up of every shape of both routes
        for k in range(args.warmup):
            run(fused, k)
    torch.cuda.synchronize()
    pairs, last = [], {}
    for p in range(args.pairs):
        row = {}
        for fused in (routes if p % 2 == 0 else routes[::-1]):       # alternate the order inside the pairs
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for k in range(args.iters):
                out = run(fused, k)
            e1.record()
            torch.cuda.synchronize()
            ms = e0.elapsed_time(e1) / args.iters
            row["fused" if fused else "two_pass"] = {"ms_per_batch": round(ms, 3), "frames_per_s": round(args.frames * 1e3 / ms, 1)}
            last[fused] = out
        if len(routes) == 2:
            row["ratio_two_pass_over_fused"] = round(row["two_pass"]["ms_per_batch"] / row["fused"]["ms_per_batch"], 4)
        pairs.append(row)
    resnet.EVAL_FUSED = True
    outs, macs = conv_shapes()
    removed = 8 * outs * args.frames                                  # one fp32 write and one fp32 read of every convolution output
    flop = 2.0 * macs * args.frames
    best = min(r["fused"]["ms_per_batch"] for r in pairs)
    res = {"tool": "classifier_eval_bench", "source_sha256": source_sha(), "device": torch.cuda.get_device_name(0),
           "workload": {"frames": args.frames, "size": 224, "generator": "DenseNetTiny", "backbone": "resnet18", "classes": 51,
                        "mode": "eval + no_grad, evaluate.forward_video", "warmup_batches": args.warmup,
                        "timed_batches_per_route_and_pair": args.iters},
           "pairs": pairs, "fused_best_ms": best,
           "removed_fp32_conv_result_bytes_per_batch": removed, "removed_traffic_ms_at_hbm_peak": round(removed / HBM_PEAK * 1e3, 3),
           "conv_gflop_per_batch": round(flop / 1e9, 1), "conv_ms_at_bf16x3_bound": round(flop / BF16X3_PEAK * 1e3, 3),
           "whole_forward_share_of_bf16x3_bound_at_best": round(flop / BF16X3_PEAK * 1e3 / best, 4)}
    if len(routes) == 2:
        import numpy as np
        a, b = last[True], last[False]
        res["two_pass_best_ms"] = min(r["two_pass"]["ms_per_batch"] for r in pairs)
        res["saved_ms_at_best"] = round(res["two_pass_best_ms"] - best, 3)
        res["fused_not_slower_on_every_pair"] = all(r["fused"]["ms_per_batch"] <= r["two_pass"]["ms_per_batch"] for r in pairs)
        res["scores_rel_err_fused_vs_two_pass"] = float(np.abs(a - b).max() / max(float(np.abs(b).max()), 1e-30))
        res["scores_finite"] = bool(np.isfinite(a).all() and np.isfinite(b).all())
    line = json.dumps(res, sort_keys=True)
    print(line, flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
