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
``--bn`` prints the BatchNorm + LeakyReLU table instead (bn_table below: ops.bn_leaky per unit width, and the whole step on the
three routes stock / CTX_TRAIN / CTX_TRAIN + CTX_TRAIN_BN; recorded in profiles/context_train_bn_bench.json).
``--ends`` prints the table of the two ends instead (ends_table below: the first unit's and the heads' convolution passes and the
heads' BatchNorm through the C ABI, and the whole step on four routes, the last with CTX_TRAIN_ENDS as well; recorded in
profiles/context_train_ends_bench.json with the sources' sha256).

    python tools/context_train_bench.py [--bn | --ends] [--frames 24] [--size 224] [--warmup 2] [--iters 5] [--pairs 3] [--table] [--out FILE]"""
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


HBM_ACHIEVABLE_TBS = 6.3      # MI355X: 8 TB/s peak, about 6.3 TB/s achievable


def bn_table(args):
    """--bn: ops.bn_leaky (csrc/ctx_bn.hip, what DMC_CTX_TRAIN_BN=1 adds to the DMC_CTX_TRAIN=1 route) against the stock
    BatchNorm2d + in-place LeakyReLU.
      * per unit width: forward and backward through the C ABI on [M][C] tensors against the stock modules on channels_last tensors
        (the backward as torch.autograd.grad of their graph), bytes from the shapes (3 M C 4 forward, 5 M C 4 backward) as TB/s;
      * the whole training step of both networks on three routes in one process: stock, CTX_TRAIN, CTX_TRAIN + CTX_TRAIN_BN; every
        pair's times are kept, the order rotates from pair to pair."""
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("context_train_bench: needs a GPU (no CPU timing)")
    from dmcnet_amd import _lib, model, ops
    from oracle import dmc_oracle as O
    dev = torch.device("cuda", 0)
    lib = _lib.load()
    CL = torch.channels_last
    n, h, w = args.frames, args.size, args.size
    M = n * h * w
    g = torch.Generator(device=dev).manual_seed(24 + n)
    s = ops._stream()
    slope, eps, mom = 0.1, 1e-5, 0.1
    units, steps = [], []

    def rel(a, b):
        return float((a.double() - b.double()).abs().max() / b.double().abs().max().clamp_min(1e-30))

    net0 = O.seeded_state_fill(model.ContextNetwork(5, True, 0), seed=26).to(dev).train()
    widths = {}
    for i, unit in list(enumerate(net0.conv_context))[:6]:
        widths.setdefault(unit[1].num_features, []).append(i)
    for c, where in sorted(widths.items()):
        bn = net0.conv_context[where[0]][1]
        act = torch.nn.LeakyReLU(slope, inplace=True)
        z = torch.randn((n, c, h, w), generator=g, device=dev).contiguous(memory_format=CL)
        dy = torch.randn((n, c, h, w), generator=g, device=dev).contiguous(memory_format=CL)
        gamma, beta = bn.weight.detach(), bn.bias.detach()
        rm, rv = bn.running_mean.clone(), bn.running_var.clone()
        y, dz = torch.empty_like(z), torch.empty_like(z)
        stats, dgamma, dbeta = torch.empty(2 * c, device=dev), torch.empty(c, device=dev), torch.empty(c, device=dev)
        scratch = torch.empty(lib.dmc_bnlrelu_scratch_bytes(M, c), dtype=torch.uint8, device=dev)

        def ours_fwd():
            _lib.check(lib.dmc_bnlrelu_fwd(_lib.ptr(z), _lib.ptr(gamma), _lib.ptr(beta), _lib.ptr(rm), _lib.ptr(rv), _lib.ptr(y), _lib.ptr(stats),
                                           _lib.ptr(scratch), M, c, slope, eps, mom, s), "dmc_bnlrelu_fwd")
            return y

        def ours_bwd():
            _lib.check(lib.dmc_bnlrelu_bwd(_lib.ptr(z), _lib.ptr(dy), _lib.ptr(gamma), _lib.ptr(beta), _lib.ptr(stats), _lib.ptr(scratch), _lib.ptr(dz),
                                           _lib.ptr(dgamma), _lib.ptr(dbeta), M, c, slope, s), "dmc_bnlrelu_bwd")
            return dz

        with torch.no_grad():
            best_f, last_f = alternate(ours_fwd, lambda: act(bn(z)), args.warmup, args.iters, args.pairs)
        agree_f = rel(last_f["ours"], last_f["stock"])
        del last_f
        zs = z.clone().requires_grad_(True)
        ys = act(bn(zs))                                           # the graph the stock gradients are taken from
        best_b, last_b = alternate(ours_bwd, lambda: torch.autograd.grad(ys, (zs, bn.weight, bn.bias), dy, retain_graph=True)[0],
                                   args.warmup, args.iters, args.pairs)
        agree_b = rel(last_b["ours"], last_b["stock"])
        for what, best, nbytes, agree in (("forward", best_f, 3.0 * M * c * 4, agree_f), ("backward", best_b, 5.0 * M * c * 4, agree_b)):
            tbs = nbytes / best["ours"] / 1e9
            units.append({"units": where, "channels": c, "rows": M, "pass": what, "ours_ms": round(best["ours"], 4), "stock_ms": round(best["stock"], 4),
                          "stock_over_ours": round(best["stock"] / best["ours"], 3), "mbytes": round(nbytes / 1e6, 1), "ours_tbs": round(tbs, 3),
                          "ours_share_of_achievable": round(tbs / HBM_ACHIEVABLE_TBS, 3), "rel_err_ours_vs_stock": agree})
            print("# C=%d %s: ours %.3f ms (%.2f TB/s), stock %.3f ms" % (c, what, best["ours"], tbs, best["stock"]), file=sys.stderr, flush=True)
        del z, dy, y, dz, zs, ys, last_b, scratch
        torch.cuda.empty_cache()

    routes = (("stock", False, False), ("ctx_train", True, False), ("ctx_train_bn", True, True))
    for att in [int(a) for a in args.nets.split(",") if a != ""]:
        cls = model.ContextNetworkAtt if att else model.ContextNetwork
        net = O.seeded_state_fill(cls(5, True, 0), seed=26).to(dev).train()
        x = torch.randn((n, 5, h, w), generator=g, device=dev)
        r = torch.randn((n, 2, h, w), generator=g, device=dev)

        def step(train, bn_on):
            model.CTX_TRAIN, model.CTX_TRAIN_BN = train, bn_on
            try:
                for p in net.parameters():
                    p.grad = None
                xi = x.clone().requires_grad_(True)
                out = net(xi)
                outs = out if isinstance(out, tuple) else (out,)
                sum((t * r).sum() for t in outs).backward()
            finally:
                model.CTX_TRAIN, model.CTX_TRAIN_BN = False, False
            return torch.cat([xi.grad.reshape(-1)] + [p.grad.reshape(-1) for p in net.parameters()])

        for _ in range(args.warmup):
            for _, a, b in routes:
                step(a, b)
        per_pair, last = [], {}
        for p in range(args.pairs):
            order = routes[p % 3:] + routes[:p % 3]
            ms = {}
            for name, a, b in order:
                ms[name], last[name] = timed(lambda: step(a, b), args.iters)
            per_pair.append({k: round(v, 3) for k, v in ms.items()})
        res = {"network": cls.__name__, "frames": n, "pairs": per_pair,
               "best_ms": {name: min(p[name] for p in per_pair) for name, _, _ in routes},
               "bn_faster_than_ctx_train_in_every_pair": all(p["ctx_train_bn"] < p["ctx_train"] for p in per_pair),
               "rel_err_bn_vs_stock": rel(last["ctx_train_bn"], last["stock"]), "rel_err_ctx_train_vs_stock": rel(last["ctx_train"], last["stock"])}
        steps.append(res)
        print("# %s: %s" % (cls.__name__, per_pair), file=sys.stderr, flush=True)
        del x, r, last, net
        torch.cuda.empty_cache()

    res = {"tool": "context_train_bench --bn", "device": torch.cuda.get_device_name(0), "size": args.size, "frames": n,
           "hbm_achievable_tbs": HBM_ACHIEVABLE_TBS, "warmup": args.warmup, "iters": args.iters, "pairs": args.pairs,
           "sources_sha256": sources_hash(), "units": units, "steps": steps}
    line = json.dumps(res, sort_keys=True)
    print(line, flush=True)
    if args.table:
        print("| units | C | pass | MB | ours ms | stock ms | stock / ours | ours TB/s | of %.1f | ours vs stock |" % HBM_ACHIEVABLE_TBS)
        print("|---|---|---|---|---|---|---|---|---|---|")
        for u in units:
            print("| %s | %d | %s | %.0f | %.3f | %.3f | %.2f | %.2f | %.0f %% | %.1e |" % (
                ",".join(map(str, u["units"])), u["channels"], u["pass"], u["mbytes"], u["ours_ms"], u["stock_ms"], u["stock_over_ours"], u["ours_tbs"],
                100 * u["ours_share_of_achievable"], u["rel_err_ours_vs_stock"]))
        print("| network | pair | stock ms | CTX_TRAIN ms | CTX_TRAIN + CTX_TRAIN_BN ms |")
        print("|---|---|---|---|---|")
        for st in steps:
            for i, p in enumerate(st["pairs"]):
                print("| %s | %d | %.2f | %.2f | %.2f |" % (st["network"], i + 1, p["stock"], p["ctx_train"], p["ctx_train_bn"]))
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


def ends_table(args):
    """--ends: the two ends (csrc/ctx_ends.hip, what DMC_CTX_TRAIN_ENDS=1 adds) against the stock modules.
      * per pass: ours through the C ABI against the stock convolution(s) / BatchNorm2d(2) + LeakyReLU on channels_last tensors (the
        gradients as torch.autograd.grad of their graph; ContextNetworkAtt's stock heads count both heads and the gradient add),
        bytes from the shapes as TB/s;
      * the whole training step of both networks on four routes in one process: stock, CTX_TRAIN, + CTX_TRAIN_BN,
        + CTX_TRAIN_BN + CTX_TRAIN_ENDS; every pair's times are kept, the order rotates from pair to pair."""
    import torch
    import torch.nn.functional as F
    if not torch.cuda.is_available():
        raise SystemExit("context_train_bench: needs a GPU (no CPU timing)")
    from dmcnet_amd import _lib, model, ops
    from oracle import dmc_oracle as O
    dev = torch.device("cuda", 0)
    lib = _lib.load()
    CL = torch.channels_last
    P = _lib.ptr
    n, h, w = args.frames, args.size, args.size
    M = n * h * w
    g = torch.Generator(device=dev).manual_seed(24 + n)
    s = ops._stream()
    slope, eps, mom = 0.1, 1e-5, 0.1
    passes, steps = [], []

    def rel(a, b):
        return float((a.double() - b.double()).abs().max() / b.double().abs().max().clamp_min(1e-30))

    def row(name, floats_per_pixel, ours, stock, cmp):
        best, last = alternate(ours, stock, args.warmup, args.iters, args.pairs)
        nbytes = 4.0 * M * floats_per_pixel
        tbs = nbytes / best["ours"] / 1e9
        passes.append({"pass": name, "ours_ms": round(best["ours"], 4), "stock_ms": round(best["stock"], 4),
                       "stock_over_ours": round(best["stock"] / best["ours"], 3), "mbytes": round(nbytes / 1e6, 1), "ours_tbs": round(tbs, 3),
                       "ours_share_of_achievable": round(tbs / HBM_ACHIEVABLE_TBS, 3), "rel_err_ours_vs_stock": cmp(last["ours"], last["stock"])})
        print("# %s: ours %.3f ms (%.2f TB/s), stock %.3f ms" % (name, best["ours"], tbs, best["stock"]), file=sys.stderr, flush=True)

    net0 = O.seeded_state_fill(model.ContextNetworkAtt(5, True, 0), seed=26).to(dev).train()
    # ---- the first unit's convolution
    w1 = net0.conv_context[0][0].weight.detach().contiguous()
    x = torch.randn((n, 5, h, w), generator=g, device=dev)
    dz = torch.randn((n, 32, h, w), generator=g, device=dev).contiguous(memory_format=CL)
    z = torch.empty((n, 32, h, w), device=dev, memory_format=CL)
    dx, dw1 = torch.empty_like(x), torch.empty_like(w1)
    work = torch.empty(lib.dmc_ctxends_wgrad_workspace_bytes(n, h, w, 5), dtype=torch.uint8, device=dev)
    xs, ws = x.contiguous(memory_format=CL).requires_grad_(True), w1.contiguous(memory_format=CL).requires_grad_(True)
    zs = F.conv2d(xs, ws, None, 1, 1, 1)

    def first_fwd():
        _lib.check(lib.dmc_ctxends_first_fwd(P(x), P(w1), P(z), n, h, w, s), "dmc_ctxends_first_fwd")
        return z

    def first_dgrad():
        _lib.check(lib.dmc_ctxends_first_dgrad(P(dz), P(w1), P(dx), n, h, w, s), "dmc_ctxends_first_dgrad")
        return dx

    def first_wgrad():
        _lib.check(lib.dmc_ctxends_first_wgrad(P(x), P(dz), P(dw1), P(work), n, h, w, s), "dmc_ctxends_first_wgrad")
        return dw1

    with torch.no_grad():
        row("first 5->32 forward", 37, first_fwd, lambda: F.conv2d(xs, ws, None, 1, 1, 1), rel)
    row("first 5->32 data gradient", 37, first_dgrad, lambda: torch.autograd.grad(zs, xs, dz, retain_graph=True)[0], rel)
    row("first 5->32 weight gradient", 37, first_wgrad, lambda: torch.autograd.grad(zs, ws, dz, retain_graph=True)[0], rel)
    del x, dz, z, dx, xs, zs, work
    torch.cuda.empty_cache()
    # ---- the heads' convolutions (ContextNetworkAtt: both heads)
    wh = [net0.predict_flow[0].weight.detach().contiguous(memory_format=CL), net0.predict_att[0][0].weight.detach().contiguous(memory_format=CL)]
    t = torch.randn((n, 32, h, w), generator=g, device=dev).contiguous(memory_format=CL)
    dzh = [torch.randn((n, 2, h, w), generator=g, device=dev) for _ in range(2)]
    dzh_cl = [d.contiguous(memory_format=CL) for d in dzh]
    zh = [torch.empty((n, 2, h, w), device=dev) for _ in range(2)]
    dt = torch.empty_like(t)
    dwh = [torch.empty_like(wt) for wt in wh]
    work = torch.empty(lib.dmc_ctxends_wgrad_workspace_bytes(n, h, w, 4), dtype=torch.uint8, device=dev)
    ts, whs = t.clone().requires_grad_(True), [wt.clone().requires_grad_(True) for wt in wh]
    zhs = [F.conv2d(ts, wt, None, 1, 1, 1) for wt in whs]

    def heads_fwd():
        _lib.check(lib.dmc_ctxends_heads_fwd(P(t), P(wh[0]), P(wh[1]), P(zh[0]), P(zh[1]), n, h, w, s), "dmc_ctxends_heads_fwd")
        return torch.cat(zh)

    def heads_dgrad():
        _lib.check(lib.dmc_ctxends_heads_dgrad(P(dzh[0]), P(dzh[1]), P(wh[0]), P(wh[1]), P(dt), n, h, w, s), "dmc_ctxends_heads_dgrad")
        return dt

    def heads_wgrad():
        _lib.check(lib.dmc_ctxends_heads_wgrad(P(t), P(dzh[0]), P(dzh[1]), P(dwh[0]), P(dwh[1]), P(work), n, h, w, s), "dmc_ctxends_heads_wgrad")
        return torch.cat(dwh)

    with torch.no_grad():
        row("heads 32->2 x2 forward", 36, heads_fwd, lambda: torch.cat([F.conv2d(t, wt, None, 1, 1, 1) for wt in wh]), rel)
    row("heads 32->2 x2 data gradient (+ add)", 36, heads_dgrad, lambda: torch.autograd.grad(zhs, ts, dzh_cl, retain_graph=True)[0], rel)
    row("heads 32->2 x2 weight gradient", 36, heads_wgrad, lambda: torch.cat(torch.autograd.grad(zhs, whs, dzh_cl, retain_graph=True)), rel)
    del t, dt, ts, zhs, work
    torch.cuda.empty_cache()
    # ---- one head's BatchNorm2d(2) + LeakyReLU
    bn, act = net0.predict_flow[1], torch.nn.LeakyReLU(slope, inplace=True)
    zb, dyb = dzh[0], dzh[1]
    zb_cl, dyb_cl = dzh_cl[0], dzh_cl[1]
    gamma, beta = bn.weight.detach(), bn.bias.detach()
    rm, rv = bn.running_mean.clone(), bn.running_var.clone()
    yb, dzb = torch.empty_like(zb), torch.empty_like(zb)
    stats, dgamma, dbeta = torch.empty(4, device=dev), torch.empty(2, device=dev), torch.empty(2, device=dev)
    scratch = torch.empty(lib.dmc_ctxends_bn_scratch_bytes(n, h, w), dtype=torch.uint8, device=dev)

    def bn_fwd():
        _lib.check(lib.dmc_ctxends_bn_fwd(P(zb), P(gamma), P(beta), P(rm), P(rv), P(yb), P(stats), P(scratch), n, h, w, slope, eps, mom, 0, s),
                   "dmc_ctxends_bn_fwd")
        return yb

    def bn_bwd():
        _lib.check(lib.dmc_ctxends_bn_bwd(P(zb), P(dyb), P(gamma), P(beta), P(stats), P(scratch), P(dzb), P(dgamma), P(dbeta), n, h, w, slope, 0, s),
                   "dmc_ctxends_bn_bwd")
        return dzb

    with torch.no_grad():
        row("head BatchNorm(2) + LeakyReLU forward", 6, bn_fwd, lambda: act(bn(zb_cl)), rel)
    zbs = zb_cl.clone().requires_grad_(True)
    ybs = act(bn(zbs))
    row("head BatchNorm(2) + LeakyReLU backward", 10, bn_bwd, lambda: torch.autograd.grad(ybs, (zbs, bn.weight, bn.bias), dyb_cl, retain_graph=True)[0], rel)
    del zbs, ybs, dzh, dzh_cl
    torch.cuda.empty_cache()

    routes = (("stock", False, False, False), ("ctx_train", True, False, False), ("ctx_train_bn", True, True, False),
              ("ctx_train_bn_ends", True, True, True))
    for att in [int(a) for a in args.nets.split(",") if a != ""]:
        cls = model.ContextNetworkAtt if att else model.ContextNetwork
        net = O.seeded_state_fill(cls(5, True, 0), seed=26).to(dev).train()
        x = torch.randn((n, 5, h, w), generator=g, device=dev)
        r = torch.randn((n, 2, h, w), generator=g, device=dev)

        def step(train, bn_on, ends_on):
            model.CTX_TRAIN, model.CTX_TRAIN_BN, model.CTX_TRAIN_ENDS = train, bn_on, ends_on
            try:
                for p in net.parameters():
                    p.grad = None
                xi = x.clone().requires_grad_(True)
                out = net(xi)
                outs = out if isinstance(out, tuple) else (out,)
                sum((t * r).sum() for t in outs).backward()
            finally:
                model.CTX_TRAIN, model.CTX_TRAIN_BN, model.CTX_TRAIN_ENDS = False, False, False
            return torch.cat([xi.grad.reshape(-1)] + [p.grad.reshape(-1) for p in net.parameters()])

        for _ in range(args.warmup):
            for _, a, b, c in routes:
                step(a, b, c)
        per_pair, last = [], {}
        for p in range(args.pairs):
            order = routes[p % 4:] + routes[:p % 4]
            ms = {}
            for name, a, b, c in order:
                ms[name], last[name] = timed(lambda: step(a, b, c), args.iters)
            per_pair.append({k: round(v, 3) for k, v in ms.items()})
        res = {"network": cls.__name__, "frames": n, "pairs": per_pair,
               "best_ms": {name: min(p[name] for p in per_pair) for name, _, _, _ in routes},
               "ends_faster_than_ctx_train_bn_in_every_pair": all(p["ctx_train_bn_ends"] < p["ctx_train_bn"] for p in per_pair),
               "rel_err_ends_vs_stock": rel(last["ctx_train_bn_ends"], last["stock"]), "rel_err_bn_vs_stock": rel(last["ctx_train_bn"], last["stock"])}
        steps.append(res)
        print("# %s: %s" % (cls.__name__, per_pair), file=sys.stderr, flush=True)
        del x, r, last, net
        torch.cuda.empty_cache()

    res = {"tool": "context_train_bench --ends", "device": torch.cuda.get_device_name(0), "size": args.size, "frames": n,
           "hbm_achievable_tbs": HBM_ACHIEVABLE_TBS, "warmup": args.warmup, "iters": args.iters, "pairs": args.pairs,
           "sources_sha256": sources_hash(), "sources": __import__("dmcnet_amd.build", fromlist=["source_hashes"]).source_hashes(),
           "passes": passes, "steps": steps}
    line = json.dumps(res, sort_keys=True)
    print(line, flush=True)
    if args.table:
        print("| pass | MB | ours ms | stock ms | stock / ours | ours TB/s | of %.1f | ours vs stock |" % HBM_ACHIEVABLE_TBS)
        print("|---|---|---|---|---|---|---|---|")
        for u in passes:
            print("| %s | %.0f | %.3f | %.3f | %.2f | %.2f | %.0f %% | %.1e |" % (
                u["pass"], u["mbytes"], u["ours_ms"], u["stock_ms"], u["stock_over_ours"], u["ours_tbs"], 100 * u["ours_share_of_achievable"],
                u["rel_err_ours_vs_stock"]))
        print("| network | pair | stock ms | CTX_TRAIN ms | + BN ms | + BN + ENDS ms |")
        print("|---|---|---|---|---|---|")
        for st in steps:
            for i, p in enumerate(st["pairs"]):
                print("| %s | %d | %.2f | %.2f | %.2f | %.2f |" % (st["network"], i + 1, p["stock"], p["ctx_train"], p["ctx_train_bn"], p["ctx_train_bn_ends"]))
    out = args.out or os.path.join(ROOT, "profiles", "context_train_ends_bench.json")
    with open(out, "w") as f:
        f.write(line + "\n")


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
    ap.add_argument("--bn", action="store_true", help="the BatchNorm + LeakyReLU table (ops.bn_leaky, CTX_TRAIN_BN) instead of the convolutions'")
    ap.add_argument("--ends", action="store_true", help="the first unit's and the heads' table (csrc/ctx_ends.hip, CTX_TRAIN_ENDS); writes "
                                                        "profiles/context_train_ends_bench.json unless --out says otherwise")
    args = ap.parse_args()
    if args.bn:
        return bn_table(args)
    if args.ends:
        return ends_table(args)

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
