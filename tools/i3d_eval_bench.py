"""Eval-mode I3D on the reference evaluator's recipe batch (code/dmcnet_I3D/test/test.sh: 2 clips x 250 frames at 224^2,
DenseNetTiny generator, node='logit', no_grad, net.eval()) with a bf16 trunk: the eval route (i3d.EVAL_FUSED = True: every unit
one convolution launch with the BatchNorm's running statistics in its epilogue, Inception blocks joined in place) against
EVAL_FUSED = False (conv3d_bf16 -> stock BatchNorm3d -> ReLU, MIOpen stem, torch.cat), as alternating pairs in one process.

Seeded weights incl. the running statistics (oracle.dmc_oracle.seeded_state_fill) and seeded inputs.  Per route: warm-up
batches, then `--iters` batches timed with device events per pair.  Prints ONE JSON line: ms per batch and clips/s per route and
pair, the trunk's FLOPs per batch (from the layer shapes, counted below) and that rate's share of the 2.5 PFLOP/s dense bf16
peak, the two routes' logits agreement on the timed inputs, and a sha256 of the sources.
``--routes fused`` runs the eval route only (for a rocprofv3 --kernel-trace --stats run).

    python tools/i3d_eval_bench.py [--frames 250] [--batch 2] [--warmup 3] [--iters 10] [--pairs 3] [--out FILE]"""
import argparse
import hashlib
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PEAK_BF16 = 2.5e15          # dense bf16 FLOP/s of the MI355X


def trunk_macs(frames, size=224):
    """Multiply-adds of the I3D trunk per clip (every Unit3Dpy convolution incl. the head conv3d_0c_1x1), from the shapes:
    stem 7x7x7 / s2 on 2 channels, TF-"SAME" pools with ceil division (dmcnet_amd.i3d.I3D, code/dmcnet_I3D/network/i3d.py:458-601)."""
    from dmcnet_amd.i3d import _MIXED

    def up(a, b):
        return -(-a // b)
    d, h = up(frames, 2), up(size, 2)
    macs = d * h * h * 64 * 2 * 343                                   # conv3d_1a_7x7
    h = up(h, 2)                                                      # maxPool3d_2a (1,3,3)/(1,2,2)
    macs += d * h * h * (64 * 64 + 64 * 192 * 27)                     # conv3d_2b_1x1, conv3d_2c_3x3
    h = up(h, 2)                                                      # maxPool3d_3a

    def mixed(cin, o, p):
        return p * (cin * o[0] + cin * o[1] + o[1] * o[2] * 27 + cin * o[3] + o[3] * o[4] * 27 + cin * o[5])
    for nm, cin, o in _MIXED:
        if nm == "mixed_4b":
            d, h = up(d, 2), up(h, 2)                                 # maxPool3d_4a (3,3,3)/(2,2,2)
        if nm == "mixed_5b":
            d, h = up(d, 2), up(h, 2)                                 # maxPool3d_5a (2,2,2)/(2,2,2)
        macs += mixed(cin, o, d * h * h)
    macs += max(d - 1, 1) * 1024 * 400                                # avg_pool (2,7,7) -> conv3d_0c_1x1
    return macs


def source_sha():
    """sha256 over the library's sources (build.source_hashes) and the Python modules of the eval path."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("_dmc_build", os.path.join(ROOT, "dmc-net_amd", "build.py"))
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    h = hashlib.sha256()
    for k, v in sorted(b.source_hashes().items()):
        h.update(("%s %s\n" % (k, v)).encode())
    for f in ("ops.py", "i3d.py", "evaluate.py", "model.py"):
        with open(os.path.join(ROOT, "dmc-net_amd", f), "rb") as fh:
            h.update(hashlib.sha256(fh.read()).hexdigest().encode())
    return h.hexdigest()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=250)
    ap.add_argument("--batch", type=int, default=2)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--pairs", type=int, default=3)
    ap.add_argument("--routes", default="both", choices=["both", "fused"])
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    args = ap.parse_args()

    import torch
    if not torch.cuda.is_available():
        raise SystemExit("i3d_eval_bench: needs a GPU (no CPU timing)")
    import dmcnet_amd
    from dmcnet_amd import i3d, miopen
    from oracle import dmc_oracle as O
    miopen.enable_find()
    dev = "cuda:0"
    net = i3d.I3D(51, modality="flow+mp4", dropout_prob=0, arch_estimator="DenseNetTiny")
    O.seeded_state_fill(net, seed=71)
    net.to(dev).eval()
    net.trunk_dtype = torch.bfloat16
    gen = torch.Generator(device=dev).manual_seed(72)
    inputs = [torch.randn(args.batch, 5, args.frames, 224, 224, device=dev, generator=gen) for _ in range(2)]
    routes = [True, False] if args.routes == "both" else [True]

    def run(fused, k):
        i3d.EVAL_FUSED = fused
        with torch.no_grad():
            return net(inputs[k % 2])

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
            row["fused" if fused else "stock"] = {"ms_per_batch": round(ms, 3), "clips_per_s": round(args.batch * 1e3 / ms, 3)}
            last[fused] = out.float()
        if len(routes) == 2:
            row["ratio_stock_over_fused"] = round(row["stock"]["ms_per_batch"] / row["fused"]["ms_per_batch"], 4)
        pairs.append(row)
    i3d.EVAL_FUSED = True
    flops = 2 * trunk_macs(args.frames) * args.batch
    best = min(r["fused"]["ms_per_batch"] for r in pairs)
    res = {"tool": "i3d_eval_bench", "source_sha256": source_sha(), "device": torch.cuda.get_device_name(0),
           "workload": {"clips": args.batch, "frames": args.frames, "size": 224, "generator": "DenseNetTiny", "trunk": "bf16",
                        "mode": "eval + no_grad", "warmup_batches": args.warmup, "timed_batches_per_route_and_pair": args.iters},
           "trunk_flop_per_batch": flops, "pairs": pairs,
           "fused_best_ms": best, "fused_trunk_share_of_bf16_peak_at_best": round(flops / (best * 1e-3) / PEAK_BF16, 4)}
    if len(routes) == 2:
        a, b = last[True], last[False]
        res["stock_best_ms"] = min(r["stock"]["ms_per_batch"] for r in pairs)
        res["fused_not_slower_on_every_pair"] = all(r["fused"]["ms_per_batch"] <= r["stock"]["ms_per_batch"] for r in pairs)
        res["logits_rel_err_fused_vs_stock"] = float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))
        res["logits_finite"] = bool(torch.isfinite(a).all() and torch.isfinite(b).all())
    line = json.dumps(res, sort_keys=True)
    print(line, flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
