"""Eval-mode ContextNetwork / ContextNetworkAtt (code/dmcnet/model.py:45-104; model.eval() + no_grad) on the evaluator's batch
(25 frames at 224^2, as code/dmcnet/test.py runs it) and on 250 frames: this package's route (model.CTX_EVAL = True, one launch
per dilated conv + BatchNorm + LeakyReLU unit, csrc/ctx_eval.hip) against the stock PyTorch-ROCm modules (CTX_EVAL = False, what
DMC_CTX_EVAL=0 selects -- the route of the parent commit), as alternating pairs in one process.

Seeded weights incl. the running statistics (oracle.dmc_oracle.seeded_state_fill), seeded standard-normal inputs.  Warm-up first,
then `--iters` runs per route and pair, timed with device events.  Per unit (each route on its own layout: NHWC through the C ABI
with the weights packed beforehand / the stock Sequential on NCHW) and for the whole network (ops.context_eval incl. its weight
split and BatchNorm statistics / net.conv_context).  Prints ONE JSON line: ms, TFLOP/s fp32-equivalent (2 x MACs / time) and the
fraction of the bf16x3 bound (2,500 / 6 = 416.7 TFLOP/s) per unit and batch, the ratio stock / ours, the two routes' agreement;
``--table`` also prints the rows as a Markdown table.

    python tools/context_eval_bench.py [--frames 25,250] [--att 0] [--warmup 2] [--iters 5] [--pairs 3] [--table] [--out FILE]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

BF16X3_PEAK = 2500.0e12 / 6
FP32_PEAK = 157.3e12


def timed(fn, iters):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        out = fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters, out


def alternate(ours, stock, warmup, iters, pairs):
    """Best-of-pairs ms of both routes (order alternates inside the pairs) and their last results."""
    for _ in range(warmup):
        ours(); stock()
    best, last = {"ours": float("inf"), "stock": float("inf")}, {}
    for p in range(pairs):
        for name in (("ours", "stock") if p % 2 == 0 else ("stock", "ours")):
            ms, last[name] = timed(ours if name == "ours" else stock, iters)
            best[name] = min(best[name], ms)
    return best, last


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", default="25,250")
    ap.add_argument("--size", type=int, default=224)
    ap.add_argument("--att", type=int, default=0)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--pairs", type=int, default=3)
    ap.add_argument("--table", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch
    if not torch.cuda.is_available():
        raise SystemExit("context_eval_bench: needs a GPU (no CPU timing)")
    from dmcnet_amd import _lib, model, ops
    from oracle import dmc_oracle as O
    dev = torch.device("cuda", 0)
    lib = _lib.load()
    cls = model.ContextNetworkAtt if args.att else model.ContextNetwork
    net = O.seeded_state_fill(cls(5, True, 0), seed=26).to(dev).eval()
    h = w = args.size
    rows = []

    def rel(a, b):
        return float((a.double() - b.double()).abs().max() / b.double().abs().max().clamp_min(1e-30))

    def row(name, frames, macs_per_pixel, best, agree):
        flop = 2.0 * macs_per_pixel * frames * h * w
        r = {"unit": name, "frames": frames, "gflop": round(flop / 1e9, 2), "ours_ms": round(best["ours"], 4), "stock_ms": round(best["stock"], 4),
             "stock_over_ours": round(best["stock"] / best["ours"], 3), "ours_tflops": round(flop / best["ours"] / 1e9, 1),
             "stock_tflops": round(flop / best["stock"] / 1e9, 1), "ours_share_of_bf16x3_bound": round(flop / BF16X3_PEAK * 1e3 / best["ours"], 4),
             "rel_err_ours_vs_stock": agree}
        rows.append(r)
        return r

    with torch.no_grad():
        for frames in [int(f) for f in args.frames.split(",")]:
            g = torch.Generator(device=dev).manual_seed(24 + frames)
            s = ops._stream()
            units = list(net.conv_context) + ([net.predict_flow] if args.att else [])
            total_macs = 0
            for i, unit in enumerate(units):
                conv, bn = unit[0], unit[1]
                cin, cout, d = conv.in_channels, conv.out_channels, conv.dilation[0]
                macs = cin * cout * 9 * (2 if (args.att and cout == 2) else 1)
                total_macs += macs
                x = torch.randn((frames, cin, h, w), generator=g, device=dev)
                stats, gam, bet = ops._bn_eval_stats(bn), bn.weight.detach().contiguous(), bn.bias.detach().contiguous()
                if cin == 5:
                    y = torch.empty((frames, h, w, cout), device=dev)
                    wt = conv.weight.detach().contiguous()
                    ours = lambda: (_lib.check(lib.dmc_ctx_first_eval(_lib.ptr(x), _lib.ptr(wt), _lib.ptr(stats), _lib.ptr(gam), _lib.ptr(bet),
                                                                      _lib.ptr(y), frames, h, w, s), "dmc_ctx_first_eval"), y.permute(0, 3, 1, 2))[1]
                    stock = lambda: unit(x)
                elif cout == 2:
                    xn = x.permute(0, 2, 3, 1).contiguous()
                    heads = [unit] + ([net.predict_att[0]] if args.att else [])
                    hp = []
                    for u in heads:
                        hp += [u[0].weight.detach().permute(0, 2, 3, 1).contiguous(), ops._bn_eval_stats(u[1]), u[1].weight.detach().contiguous(),
                               u[1].bias.detach().contiguous()]
                    hp += [None] * (8 - len(hp))
                    flow = torch.empty((frames, 2, h, w), device=dev)
                    att = torch.empty((frames, 2, h, w), device=dev) if args.att else None
                    ours = lambda: (_lib.check(lib.dmc_ctx_heads_eval(_lib.ptr(xn), *[_lib.ptr(t) for t in hp], _lib.ptr(flow), _lib.ptr(att),
                                                                      frames, h, w, s), "dmc_ctx_heads_eval"), flow)[1]
                    stock = (lambda: (net.predict_flow(x), net.predict_att(x))[0]) if args.att else (lambda: unit(x))
                else:
                    xn = x.permute(0, 2, 3, 1).contiguous()
                    y = torch.empty((frames, h, w, cout), device=dev)
                    wp = torch.empty(lib.dmc_ctx_wpack_bytes(cin, cout), dtype=torch.uint8, device=dev)
                    _lib.check(lib.dmc_ctx_pack_weights(_lib.ptr(conv.weight.detach().permute(0, 2, 3, 1).contiguous()), _lib.ptr(wp), cin, cout, s),
                               "dmc_ctx_pack_weights")
                    ours = lambda: (_lib.check(lib.dmc_ctx_unit_eval(_lib.ptr(xn), _lib.ptr(wp), _lib.ptr(stats), _lib.ptr(gam), _lib.ptr(bet),
                                                                     _lib.ptr(y), frames, h, w, cin, cout, d, s), "dmc_ctx_unit_eval"), y.permute(0, 3, 1, 2))[1]
                    stock = lambda: unit(x)
                best, last = alternate(ours, stock, args.warmup, args.iters, args.pairs)
                row("%d: %d->%d d=%d%s" % (i, cin, cout, d, " (both heads)" if args.att and cout == 2 else ""), frames, macs, best,
                    rel(last["ours"], last["stock"]))
                del x, last
                torch.cuda.empty_cache()
            x = torch.randn((frames, 5, h, w), generator=g, device=dev)

            def whole(on):
                model.CTX_EVAL = on
                try:
                    out = net(x)
                finally:
                    model.CTX_EVAL = True
                return out[0] if isinstance(out, tuple) else out
            best, last = alternate(lambda: whole(True), lambda: whole(False), args.warmup, args.iters, args.pairs)
            row("whole network", frames, total_macs, best, rel(last["ours"], last["stock"]))
            del x, last
            torch.cuda.empty_cache()
    res = {"tool": "context_eval_bench", "device": torch.cuda.get_device_name(0), "network": cls.__name__, "size": args.size,
           "bf16x3_bound_tflops": round(BF16X3_PEAK / 1e12, 1), "fp32_mfma_bound_tflops": round(FP32_PEAK / 1e12, 1),
           "warmup": args.warmup, "iters": args.iters, "pairs": args.pairs, "rows": rows}
    line = json.dumps(res, sort_keys=True)
    print(line, flush=True)
    if args.table:
        print("| frames | unit | GFLOP | ours ms | stock ms | stock / ours | ours TFLOP/s | stock TFLOP/s | of 416.7 | ours vs stock |")
        print("|---|---|---|---|---|---|---|---|---|---|")
        for r in rows:
            print("| %d | %s | %.1f | %.3f | %.3f | %.2f | %.1f | %.1f | %.1f %% | %.1e |" % (
                r["frames"], r["unit"], r["gflop"], r["ours_ms"], r["stock_ms"], r["stock_over_ours"], r["ours_tflops"], r["stock_tflops"],
                100 * r["ours_share_of_bf16x3_bound"], r["rel_err_ours_vs_stock"]))
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
