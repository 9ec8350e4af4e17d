"""Training of ContextNetwork / ContextNetworkAtt (code/dmcnet/model.py:45-104): the dilated convolutions of the five middle
units on csrc/dconv.hip (model.CTX_TRAIN = True, what DMC_CTX_TRAIN=1 selects) against the stock PyTorch-ROCm route
(CTX_TRAIN = False, the default), as alternating pairs in one process.

Seeded weights (oracle.dmc_oracle.seeded_state_fill), seeded standard-normal inputs, 224^2, 24 frames (8 clips x 3 segments)
unless told otherwise.  Warm-up first, then `--iters` runs per route and pair, timed with device events.
  * per middle unit: the convolution's forward, data gradient and weight gradient, each on its own -- ours through the C ABI on
    NHWC tensors with the weights packed beforehand (dmc_dconv_fwd, dmc_dconv_fwd on dy with the transposed pack,
    dmc_dconv_wgrad incl. its reduction), the stock route as F.conv2d on channels_last tensors and torch.autograd.grad of it
    towards the input / the weight alone;
  * the whole network: forward + backward of a training step (loss = sum(out * r)) through net(x) with model.CTX_TRAIN on / off,
    i.e. including the weight packs, the BatchNorms, the first unit, the heads and the host side.
Prints ONE JSON line: ms, TFLOP/s fp32-equivalent (2 x MACs / time; a training step counts three convolutions' worth) and the
share of the bf16x3 bound (2,500 / 6 = 416.7 TFLOP/s), the ratio stock / ours, the two routes' agreement, and the sha256 over the
library's source hashes; ``--table`` also prints the rows as a Markdown table.

    python tools/context_train_bench.py [--frames 24] [--size 224] [--warmup 2] [--iters 5] [--pairs 3] [--table] [--out FILE]"""
import argparse
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

BF16X3_PEAK = 2500.0e12 / 6


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


def sources_hash():
    from dmcnet_amd import build
    return hashlib.sha256(json.dumps(build.source_hashes(), sort_keys=True).encode()).hexdigest()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=24)
    ap.add_argument("--size", type=int, default=224)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--pairs", type=int, default=3)
    ap.add_argument("--nets", default="0,1", help="att values of the whole-network rows: 0 = ContextNetwork, 1 = ContextNetworkAtt")
    ap.add_argument("--table", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch
    import torch.nn.functional as F
    if not torch.cuda.is_available():
        raise SystemExit("context_train_bench: needs a GPU (no CPU timing)")
    from dmcnet_amd import _lib, model, ops
    from oracle import dmc_oracle as O
    dev = torch.device("cuda", 0)
    lib = _lib.load()
    CL = torch.channels_last
    n, h, w = args.frames, args.size, args.size
    rows = []

    def rel(a, b):
        return float((a.double() - b.double()).abs().max() / b.double().abs().max().clamp_min(1e-30))

    def row(name, what, flop, best, agree):
        r = {"unit": name, "pass": what, "frames": n, "gflop": round(flop / 1e9, 2), "ours_ms": round(best["ours"], 4),
             "stock_ms": round(best["stock"], 4), "stock_over_ours": round(best["stock"] / best["ours"], 3),
             "ours_tflops": round(flop / best["ours"] / 1e9, 1), "stock_tflops": round(flop / best["stock"] / 1e9, 1),
             "ours_share_of_bf16x3_bound": round(flop / BF16X3_PEAK * 1e3 / best["ours"], 4), "rel_err_ours_vs_stock": agree}
        rows.append(r)
        print("# %s %s: ours %.3f ms, stock %.3f ms" % (name, what, best["ours"], best["stock"]), file=sys.stderr, flush=True)
        return r

    net0 = O.seeded_state_fill(model.ContextNetwork(5, True, 0), seed=26).to(dev).train()
    g = torch.Generator(device=dev).manual_seed(24 + n)
    s = ops._stream()
    for i, unit in list(enumerate(net0.conv_context))[1:6]:
        conv = unit[0]
        cin, cout, d = conv.in_channels, conv.out_channels, conv.dilation[0]
        flop = 2.0 * cin * cout * 9 * n * h * w
        name = "%d: %d->%d d=%d" % (i, cin, cout, d)
        x = torch.randn((n, cin, h, w), generator=g, device=dev).contiguous(memory_format=CL)
        dy = torch.randn((n, cout, h, w), generator=g, device=dev).contiguous(memory_format=CL)
        wt = conv.weight.detach().contiguous(memory_format=CL)
        wf = torch.empty(lib.dmc_dconv_wpack_bytes(cin, cout), dtype=torch.uint8, device=dev)
        wtr = torch.empty_like(wf)
        _lib.check(lib.dmc_dconv_pack_weights(_lib.ptr(wt), _lib.ptr(wf), cin, cout, 0, s), "dmc_dconv_pack_weights")
        _lib.check(lib.dmc_dconv_pack_weights(_lib.ptr(wt), _lib.ptr(wtr), cin, cout, 1, s), "dmc_dconv_pack_weights")
        y = torch.empty((n, cout, h, w), device=dev, memory_format=CL)
        dx = torch.empty((n, cin, h, w), device=dev, memory_format=CL)
        dw = torch.empty((cout, cin, 3, 3), device=dev, memory_format=CL)
        work = torch.empty(lib.dmc_dconv_wgrad_workspace_bytes(n, h, w, cin, cout), dtype=torch.uint8, device=dev)
        xs, ws = x.clone().requires_grad_(True), wt.clone().requires_grad_(True)
        ys = F.conv2d(xs, ws, None, 1, d, d)                       # the graph both stock gradients are taken from

        def ours_fwd():
            _lib.check(lib.dmc_dconv_fwd(_lib.ptr(x), _lib.ptr(wf), _lib.ptr(y), n, h, w, cin, cout, d, s), "dmc_dconv_fwd")
            return y

        def ours_dgrad():
            _lib.check(lib.dmc_dconv_fwd(_lib.ptr(dy), _lib.ptr(wtr), _lib.ptr(dx), n, h, w, cout, cin, d, s), "dmc_dconv_fwd")
            return dx

        def ours_wgrad():
            _lib.check(lib.dmc_dconv_wgrad(_lib.ptr(x), _lib.ptr(dy), _lib.ptr(dw), _lib.ptr(work), n, h, w, cin, cout, d, s), "dmc_dconv_wgrad")
            return dw

        with torch.no_grad():
            best, last = alternate(ours_fwd, lambda: F.conv2d(x, wt, None, 1, d, d), args.warmup, args.iters, args.pairs)
        row(name, "forward", flop, best, rel(last["ours"], last["stock"]))
        best, last = alternate(ours_dgrad, lambda: torch.autograd.grad(ys, xs, dy, retain_graph=True)[0], args.warmup, args.iters, args.pairs)
        row(name, "data gradient", flop, best, rel(last["ours"], last["stock"]))
        best, last = alternate(ours_wgrad, lambda: torch.autograd.grad(ys, ws, dy, retain_graph=True)[0], args.warmup, args.iters, args.pairs)
        row(name, "weight gradient", flop, best, rel(last["ours"], last["stock"]))
        del x, dy, y, dx, xs, ws, ys, last, work
        torch.cuda.empty_cache()

    for att in [int(a) for a in args.nets.split(",") if a != ""]:
        cls = model.ContextNetworkAtt if att else model.ContextNetwork
        net = O.seeded_state_fill(cls(5, True, 0), seed=26).to(dev).train()
        convs = [u[0] for u in net.conv_context] + ([net.predict_flow[0], net.predict_att[0][0]] if att else [])
        macs = sum(c.in_channels * c.out_channels * 9 for c in convs)
        x = torch.randn((n, 5, h, w), generator=g, device=dev)
        r = torch.randn((n, 2, h, w), generator=g, device=dev)

        def step(on):
            model.CTX_TRAIN = on
            try:
                for p in net.parameters():
                    p.grad = None
                xi = x.clone().requires_grad_(True)
                out = net(xi)
                outs = out if isinstance(out, tuple) else (out,)
                sum((t * r).sum() for t in outs).backward()
            finally:
                model.CTX_TRAIN = False
            return torch.cat([xi.grad.reshape(-1)] + [p.grad.reshape(-1) for p in net.parameters()])

        best, last = alternate(lambda: step(True), lambda: step(False), args.warmup, args.iters, args.pairs)
        row(cls.__name__, "training step (forward + backward)", 3 * 2.0 * macs * n * h * w, best, rel(last["ours"], last["stock"]))
        del x, r, last, net
        torch.cuda.empty_cache()

    res = {"tool": "context_train_bench", "device": torch.cuda.get_device_name(0), "size": args.size, "frames": n,
           "bf16x3_bound_tflops": round(BF16X3_PEAK / 1e12, 1), "warmup": args.warmup, "iters": args.iters, "pairs": args.pairs,
           "sources_sha256": sources_hash(), "rows": rows}
    line = json.dumps(res, sort_keys=True)
    print(line, flush=True)
    if args.table:
        print("| unit | pass | GFLOP | ours ms | stock ms | stock / ours | ours TFLOP/s | stock TFLOP/s | of 416.7 | ours vs stock |")
        print("|---|---|---|---|---|---|---|---|---|---|")
        for r in rows:
            print("| %s | %s | %.1f | %.3f | %.3f | %.2f | %.1f | %.1f | %.1f %% | %.1e |" % (
                r["unit"], r["pass"], r["gflop"], r["ours_ms"], r["stock_ms"], r["stock_over_ours"], r["ours_tflops"], r["stock_tflops"],
                100 * r["ours_share_of_bf16x3_bound"], r["rel_err_ours_vs_stock"]))
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
