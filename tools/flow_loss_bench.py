"""The reconstruction criteria on the device (dmc_flow_loss_fwd / _bwd, dmc_gen_tiny_fwd_loss) against the stock PyTorch-ROCm
route they replace (F.mse_loss / F.smooth_l1_loss / F.l1_loss, with `att * gen` and `att * flow` materialised for the attention
form -- train.flow_loss before these kernels existed).

1. Stand-alone: forward and forward + backward of ops.flow_loss per kind, plain and attention-weighted, on 120 x 2 x 224 x 224
   elements; device events; GB/s from the bytes the pass must move (forward: 2 or 3 arrays read; backward: the same read, 1 or 2
   written) against the 8 TB/s HBM peak; beside it the stock route's time for the same loss on the same tensors.
2. Training step of bench.py's default configuration (B = 40, S = 3, 224 x 224, resnet18 + DenseNetTiny, flow_ds_factor 16) with
   loss_mse = SmoothL1Loss and L1: DmcnetTrainStep (the loss in the generator's one-launch forward) against the step the trainer
   took before (model(), then the stock criterion on gen_flow), alternating pairs in one process.

Prints ONE JSON line (and writes it to --out).

    python tools/flow_loss_bench.py [--iters 50] [--steps 20] [--pairs 3] [--batch 40] [--out profiles/flow_loss_bench.json]"""
import argparse
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK = 8000.0e9
KINDS = ("MSELoss", "SmoothL1Loss", "L1")


def source_sha():
    import importlib.util
    spec = importlib.util.spec_from_file_location("_dmc_build", os.path.join(ROOT, "dmc-net_amd", "build.py"))
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    h = hashlib.sha256()
    for k, v in sorted(b.source_hashes().items()):
        h.update(("%s %s\n" % (k, v)).encode())
    for f in ("ops.py", "train.py", "model.py"):
        with open(os.path.join(ROOT, "dmc-net_amd", f), "rb") as fh:
            h.update(hashlib.sha256(fh.read()).hexdigest().encode())
    return h.hexdigest()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=120)
    ap.add_argument("--iters", type=int, default=50, help="timed repetitions of each stand-alone pass")
    ap.add_argument("--steps", type=int, default=20, help="timed training steps per route and pair")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--pairs", type=int, default=3)
    ap.add_argument("--batch", type=int, default=40)
    ap.add_argument("--no-step", action="store_true", help="stand-alone part only")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch
    import torch.nn.functional as F
    if not torch.cuda.is_available():
        raise SystemExit("flow_loss_bench: needs a GPU (no CPU timing)")
    import dmcnet_amd
    from dmcnet_amd import dataset, ops, train
    dev = torch.device("cuda", 0)
    stock = {"MSELoss": F.mse_loss, "SmoothL1Loss": F.smooth_l1_loss, "L1": F.l1_loss}

    def timed(fn, iters):
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / iters

    # ---- 1. stand-alone
    g = torch.Generator(device=dev).manual_seed(7)
    shape = (args.frames, 2, 224, 224)
    numel = args.frames * 2 * 224 * 224
    gen = (torch.randn(shape, generator=g, device=dev) * 1.5).requires_grad_(True)
    flow = torch.randn(shape, generator=g, device=dev) * 1.5
    att = torch.relu(torch.randn(shape, generator=g, device=dev)).requires_grad_(True)
    standalone = []
    for kind in KINDS:
        for with_att in (False, True):
            a = att if with_att else None

            def ours_fwd():
                with torch.no_grad():
                    return ops.flow_loss(kind, gen, flow, a)

            def ours_fb():
                gen.grad = None
                att.grad = None
                ops.flow_loss(kind, gen, flow, a).backward()

            def stock_loss():
                return stock[kind](gen, flow) if a is None else stock[kind](a * gen, a * flow)

            def stock_fwd():
                with torch.no_grad():
                    return stock_loss()

            def stock_fb():
                gen.grad = None
                att.grad = None
                stock_loss().backward()

            f_ms, fb_ms = timed(ours_fwd, args.iters), timed(ours_fb, args.iters)
            sf_ms, sfb_ms = timed(stock_fwd, args.iters), timed(stock_fb, args.iters)
            b_ms = fb_ms - f_ms
            f_bytes = (3 if with_att else 2) * 4 * numel
            b_bytes = (5 if with_att else 3) * 4 * numel
            with torch.no_grad():
                lo, ls = float(ours_fwd()), float(stock_fwd())
            standalone.append({"kind": kind, "att": with_att, "fwd_ms": round(f_ms, 4), "fwd_bwd_ms": round(fb_ms, 4),
                               "fwd_gb_s": round(f_bytes / f_ms / 1e6, 1), "fwd_frac_hbm_peak": round(f_bytes / (f_ms * 1e-3) / HBM_PEAK, 3),
                               "bwd_ms": round(b_ms, 4), "bwd_gb_s": round(b_bytes / b_ms / 1e6, 1),
                               "bwd_frac_hbm_peak": round(b_bytes / (b_ms * 1e-3) / HBM_PEAK, 3),
                               "stock_fwd_ms": round(sf_ms, 4), "stock_fwd_bwd_ms": round(sfb_ms, 4),
                               "fwd_bwd_ratio_stock_over_ours": round(sfb_ms / fb_ms, 3), "loss": lo, "loss_stock": ls})
    res = {"tool": "flow_loss_bench", "source_sha256": source_sha(), "device": torch.cuda.get_device_name(0),
           "standalone_workload": {"numel": numel, "shape": list(shape), "iters": args.iters,
                                   "note": "bwd_ms = (forward + backward) - forward, autograd and allocator time included in both routes"},
           "standalone": standalone}

    # ---- 2. the training step
    if not args.no_step:
        HP = dict(lr=0.01, weight_decay=1e-4, lr_cls_mult=0.01, lr_mse_mult=1.0)      # bench.py's
        S = 3
        batch = dataset.synthetic_batch_on_device(1234, args.batch, S, 51, dev, flow_ds_factor=16)
        steps = {}
        for kind in ("SmoothL1Loss", "L1"):
            torch.manual_seed(0)
            model = dmcnet_amd.Model(51, S, "mv", base_model="resnet18", use_databn=0, gen_flow_or_delta=1,
                                     arch_estimator="DenseNetTiny").to(dev).train()
            st = train.DmcnetTrainStep(model, S, 1.0, 10.0, loss_mse=kind, **HP)

            def before(st=st, kind=kind):
                """The step DmcnetTrainStep took for this criterion before the device loss existed."""
                input_flow, input_mv, input_residual, target = batch
                fl = input_flow.reshape((-1,) + tuple(input_mv.shape[-3:]))
                st.optimizer_cls.zero_grad(set_to_none=True)
                st.optimizer_gf.zero_grad(set_to_none=True)
                output, gen_flow = st.model(input_mv, input_residual)
                loss_cls, _ = ops.consensus_ce(output, target, S)
                loss = loss_cls * st.lr_cls + stock[kind](gen_flow, fl) * st.lr_mse
                with ops.wgrad_side_stream():
                    loss.backward()
                st.optimizer_cls.step()
                st.optimizer_gf.step()

            routes = {"device_loss": lambda st=st: st.step(batch), "stock_loss": before}
            for fn in routes.values():
                for _ in range(args.warmup):
                    fn()
            train.settle_host()
            pairs = []
            for p in range(args.pairs):
                row = {}
                for name in (sorted(routes) if p % 2 == 0 else sorted(routes)[::-1]):
                    torch.cuda.synchronize()
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    for _ in range(args.steps):
                        routes[name]()
                    e1.record()
                    torch.cuda.synchronize()
                    row[name + "_ms_per_step"] = round(e0.elapsed_time(e1) / args.steps, 3)
                row["ratio_stock_over_device"] = round(row["stock_loss_ms_per_step"] / row["device_loss_ms_per_step"], 4)
                pairs.append(row)
            steps[kind] = pairs
        res["train_step_workload"] = {"batch": args.batch, "segments": S, "size": 224, "flow_ds_factor": 16, "backbone": "resnet18",
                                      "generator": "DenseNetTiny", "steps_per_route_and_pair": args.steps, "warmup": args.warmup}
        res["train_step"] = steps
    line = json.dumps(res, sort_keys=True)
    print(line, flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
