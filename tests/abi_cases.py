"""The registry of guarded-arena cases (tests/abi_arena.py): one entry per variant of every launching entry point of
include/dmcnet_hip.h, driven through ctypes as a foreign caller would.  A case carves its buffers -- exactly the promised
size, the size queries' values for workspaces -- copies seeded inputs in and calls the library; where an entry point
needs the product of another one (saved activations, statistics, packed weights, slice tensors) the producer is called
first inside the same arena, so every byte any kernel touches lies in guarded memory.  ``check`` (optional) ties the
outputs to a reference: the ops.py wrapper that makes the same call (bit for bit -- the kernels are deterministic) or,
an independent fp64 torch evaluation (the C oracle for the integer kernels) at the tolerance of the kernel's own unit test --
which of the two each group uses is said in its ``check``.

Importable without a GPU (tests/test_abi_arena_cpu.py reads ``covers``); nothing here runs at import time.
Shapes: the smallest at which each kernel still has a ragged tile, a halo, a second strip or a second channel tile, taken
from the unit tests of the kernels (see each group)."""
import numpy as np
import torch
import torch.nn.functional as F

from dmcnet_amd import _lib
from tests.abi_arena import DMC_OK

DEV = "cuda:0"
CL = torch.channels_last
BF = torch.bfloat16
U8 = torch.uint8
F64 = torch.float64
I32 = torch.int32
DMC_E_INVALID = -1


class Case(object):
    def __init__(self, id, covers, fn, check=None, expect_rc=DMC_OK, options=None, capacity=192 << 20):
        self.id, self.covers, self.fn, self.check, self.expect_rc = id, tuple(covers), fn, check, expect_rc
        self.options, self.capacity = dict(options or {}), capacity


CASES = []


def add(id, covers, fn, **kw):
    CASES.append(Case(id, covers, fn, **kw))


def L():
    return _lib.load()


def rnd(seed, shape, scale=1.0):
    return torch.from_numpy((np.random.RandomState(seed).standard_normal(shape) * scale).astype(np.float32))


def pos(seed, shape, lo=0.5, hi=1.5):
    return torch.from_numpy(np.random.RandomState(seed).uniform(lo, hi, shape).astype(np.float32))


def nhwc(t):
    """The memory of a channels_last tensor, as a contiguous [N][H][W][C] array."""
    return t.permute(0, 2, 3, 1).contiguous()


def ndhwc(t):
    return t.permute(0, 2, 3, 4, 1).contiguous()


def rel_err(a, b):
    a, b = a.detach().double().cpu(), torch.as_tensor(b).detach().double().cpu()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))


def bf16_close(a, ref):
    """Within one bf16 rounding of the reference (the tolerance of tests/test_conv3d_gpu.py: |ref| 2^-8 + 1e-3)."""
    a, ref = a.float().cpu(), ref.float().cpu()
    return bool(((a - ref).abs() <= ref.abs() * 2.0 ** -8 + 1e-3).all())


def same(buf, t):
    """The buffer's bytes equal tensor ``t``'s (a device tensor in the buffer's layout)."""
    return torch.equal(buf.t.reshape(-1), t.detach().reshape(-1).to(buf.t.dtype))


def slices_sum(u8, c, m):
    """fp32 [M][C] from a slice tensor bf16 [3][C / 16][M][16]: (s0 + s1) + s2 is exact in fp32."""
    s = u8.view(BF).view(3, c // 16, m, 16).float()
    return ((s[0] + s[1]) + s[2]).permute(1, 0, 2).reshape(m, c)


def opt_work(a, name, nbytes):
    """A workspace of exactly the queried size; a query that returns 0 means no buffer (NULL)."""
    return a.work(name, nbytes) if nbytes else None


def same_t(a, t):
    return torch.equal(a, t.detach().to(a.dtype).reshape(a.shape))


def tag(*xs):
    return "-".join(str(x) for x in xs)


# =====================================================================================================================
# Generator and losses (gen_fused, gen_tiny, gen_x3, gen_wgrad, losses.hip) [test_hip_parity edge shapes]
# =====================================================================================================================
GEN_CH = [(8, 5), (8, 13), (6, 21), (4, 27), (2, 31), (2, 33)]
GEN_SHAPES = [(2, 9, 120), (2, 7, 12), (1, 3, 5)]


def gen_inputs(n, h, w):
    ws = [rnd(40 + i, (co, ci, 3, 3), 0.2) for i, (co, ci) in enumerate(GEN_CH)]
    bs = [rnd(50 + i, (co,), 0.1) for i, (co, _) in enumerate(GEN_CH)]
    return rnd(1, (n, 2, h, w)), rnd(2, (n, 3, h, w)), ws, bs


def gen_fwd(n, h, w, add_mv, with_saved, mse):
    def fn(a):
        mv, res, ws, bs = gen_inputs(n, h, w)
        mv, res = a.inp("mv", mv), a.inp("res", res)
        ws = [a.inp("w%d" % i, t) for i, t in enumerate(ws)]
        bs = [a.inp("b%d" % i, t) for i, t in enumerate(bs)]
        out = a.out("out", (n, 2, h, w))
        saved = a.out("saved", nbytes=L().dmc_gen_tiny_saved_bytes(n, h, w)) if with_saved else None
        work = a.work("workspace", L().dmc_gen_tiny_workspace_bytes())
        if mse:
            flow, loss = a.inp("flow", rnd(3, (n, 2, h, w))), a.out("loss", (1,))
            part = a.work("mse_partials", L().dmc_gen_tiny_mse_partials_bytes())
            a.call("dmc_gen_tiny_fwd_mse", mv, res, ws, bs, flow, out, saved, work, loss, part, n, h, w, add_mv)
        else:
            a.call("dmc_gen_tiny_fwd", mv, res, ws, bs, out, saved, work, n, h, w, add_mv)
    return fn


def gen_fwd_check(n, h, w, add_mv, mse, with_saved):
    def check(bufs):
        from dmcnet_amd import ops
        mv, res, ws, bs = gen_inputs(n, h, w)
        mv, res, ws, bs = mv.to(DEV), res.to(DEV), [t.to(DEV).requires_grad_(True) for t in ws], [t.to(DEV).requires_grad_(True) for t in bs]
        if mse and with_saved:
            out, loss = ops.gen_tiny_mse(mv, res, rnd(3, (n, 2, h, w)).to(DEV), ws, bs, add_mv=bool(add_mv))
            assert same(bufs["loss"], loss), "loss differs from ops.gen_tiny_mse"
        elif with_saved:
            out = ops.gen_tiny(mv, res, ws, bs, add_mv=bool(add_mv))
        else:
            with torch.no_grad():       # the wrapper's inference call: saved == NULL
                out = ops.gen_tiny(mv, res, ws, bs, add_mv=bool(add_mv))
        assert same(bufs["out"], out), "out differs from the ops wrapper's"
        if mse and not with_saved:      # no wrapper passes saved == NULL to the fused loss: fp64, 1e-5 as test_hip_parity's losses
            ref = ((out.double().cpu() - rnd(3, (n, 2, h, w)).double()) ** 2).mean()
            assert rel_err(bufs["loss"].t, ref.reshape(1)) < 1e-5
    return check


def gen_bwd(n, h, w):
    def fn(a):
        mv, res, ws, bs = gen_inputs(n, h, w)
        mv, res = a.inp("mv", mv), a.inp("res", res)
        wsb = [a.inp("w%d" % i, t) for i, t in enumerate(ws)]
        bsb = [a.inp("b%d" % i, t) for i, t in enumerate(bs)]
        out = a.out("out", (n, 2, h, w))
        saved = a.out("saved", nbytes=L().dmc_gen_tiny_saved_bytes(n, h, w))
        a.call("dmc_gen_tiny_fwd", mv, res, wsb, bsb, out, saved, a.work("workspace_f", L().dmc_gen_tiny_workspace_bytes()), n, h, w, 1)
        go = a.inp("grad_out", rnd(4, (n, 2, h, w)))
        dws = [a.out("dw%d" % i, tuple(t.shape)) for i, t in enumerate(ws)]
        dbs = [a.out("db%d" % i, tuple(t.shape)) for i, t in enumerate(bs)]
        gbuf = a.work("gbuf", L().dmc_gen_tiny_gbuf_bytes(n, h, w))
        part = a.work("partials", L().dmc_gen_tiny_partials_bytes(n, h, w))
        a.call("dmc_gen_tiny_bwd", mv, res, wsb, saved, go, dws, dbs, gbuf, part, a.work("workspace_b", L().dmc_gen_tiny_workspace_bytes()), n, h, w)

    def check(bufs):
        from dmcnet_amd import ops
        mv, res, ws, bs = gen_inputs(n, h, w)
        ws, bs = [t.to(DEV).requires_grad_(True) for t in ws], [t.to(DEV).requires_grad_(True) for t in bs]
        out = ops.gen_tiny(mv.to(DEV), res.to(DEV), ws, bs, add_mv=True)
        out.backward(rnd(4, (n, 2, h, w)).to(DEV))
        for i in range(6):
            assert same(bufs["dw%d" % i], ws[i].grad) and same(bufs["db%d" % i], bs[i].grad), "gradient %d differs from the ops wrapper's" % i
    return fn, check


for _n, _h, _w in GEN_SHAPES:
    for _add in (0, 1):
        for _mse in (0, 1):
            _name = "dmc_gen_tiny_fwd_mse" if _mse else "dmc_gen_tiny_fwd"
            add(tag(_name, _n, _h, _w, "add%d" % _add, "saved"), [_name], gen_fwd(_n, _h, _w, _add, True, _mse),
                check=gen_fwd_check(_n, _h, _w, _add, _mse, True))
            if _w % 4 == 0:          # inference: nothing kept (the one-launch forward serves the shape)
                add(tag(_name, _n, _h, _w, "add%d" % _add, "nosaved"), [_name], gen_fwd(_n, _h, _w, _add, False, _mse),
                    check=gen_fwd_check(_n, _h, _w, _add, _mse, False))
            else:
                # W % 4 != 0 on the layer-by-layer path (option gen_fused 0, which is also what serves W > 224): the kernels pass the
                # features through `saved`, so saved == NULL is refused and nothing is written; with `saved` the path is served
                add(tag(_name, _n, _h, _w, "add%d" % _add, "layers-nosaved-refused"), [_name], gen_fwd(_n, _h, _w, _add, False, _mse),
                    expect_rc=DMC_E_INVALID, options={"gen_fused": 0})
                add(tag(_name, _n, _h, _w, "add%d" % _add, "layers-saved"), [_name], gen_fwd(_n, _h, _w, _add, True, _mse),
                    check=gen_fwd_check(_n, _h, _w, _add, _mse, True), options={"gen_fused": 0})
                # the one-launch forward (the default) serves any W <= 224 and keeps nothing
                add(tag(_name, _n, _h, _w, "add%d" % _add, "nosaved"), [_name], gen_fwd(_n, _h, _w, _add, False, _mse),
                    check=gen_fwd_check(_n, _h, _w, _add, _mse, False))
    _fn, _ck = gen_bwd(_n, _h, _w)
    add(tag("dmc_gen_tiny_bwd", _n, _h, _w), ["dmc_gen_tiny_fwd", "dmc_gen_tiny_bwd"], _fn, check=_ck)


def flow_mse(numel):
    def fn(a):
        g, f = a.inp("gen_flow", rnd(5, (numel,))), a.inp("flow", rnd(6, (numel,)))
        loss = a.out("loss", (1,))
        a.call("dmc_flow_mse_fwd", g, f, loss, a.work("partials", L().dmc_flow_mse_partials_bytes()), numel)
        gl = a.inp("grad_loss", torch.tensor([0.75]))
        a.call("dmc_flow_mse_bwd", g, f, gl, a.out("grad_gen", (numel,)), numel)

    def check(bufs):
        from dmcnet_amd import ops
        g = rnd(5, (numel,)).to(DEV).requires_grad_(True)
        loss = ops.flow_mse(g, rnd(6, (numel,)).to(DEV))
        (loss * 0.75).backward()
        assert same(bufs["loss"], loss) and same(bufs["grad_gen"], g.grad)
    return fn, check


for _numel in (1, 7, 4099):
    _fn, _ck = flow_mse(_numel)
    add(tag("dmc_flow_mse", _numel), ["dmc_flow_mse_fwd", "dmc_flow_mse_bwd"], _fn, check=_ck)


def ce_logits(b, s, c, peak=None):
    x = rnd(7, (b * s, c))
    return x if peak is None else x * (peak / float(x.abs().max()))


def ce_fn(b, s, c, labels, with_grad, peak=None, nan_ok=False):
    def fn(a):
        lg = a.inp("logits", ce_logits(b, s, c, peak))
        tg = a.inp("target", torch.tensor(labels, dtype=torch.int64))
        cons, loss = a.out("consensus", (b, c)), a.out("loss", (1,), nan_ok=nan_ok)
        grad = a.out("grad_logits", (b * s, c), nan_ok=nan_ok) if with_grad else None
        a.call("dmc_consensus_ce_fwd_bwd", lg, tg, cons, loss, grad, b, s, c)
    return fn


def ce_ref64(b, s, c, labels, peak=None):
    x = ce_logits(b, s, c, peak).double().requires_grad_(True)
    cons = x.view(b, s, c).mean(1)
    loss = F.cross_entropy(cons, torch.tensor(labels))
    loss.backward()
    return cons.detach(), loss.detach(), x.grad


def ce_labels(b, c):
    return [(5 * i + 3) % c for i in range(b)]


def ce_check(b, s, c, with_grad):
    def check(bufs):
        from dmcnet_amd import ops
        labels = ce_labels(b, c)
        cons, loss, grad = ce_ref64(b, s, c, labels)
        if with_grad:       # the wrapper makes this very call
            lg = ce_logits(b, s, c).to(DEV).requires_grad_(True)
            l2, c2 = ops.consensus_ce(lg, torch.tensor(labels, device=DEV), s)
            l2.backward()
            assert same(bufs["loss"], l2) and same(bufs["consensus"], c2) and same(bufs["grad_logits"], lg.grad)
        # grad_logits == NULL is reached by no wrapper call that is compared anywhere: fp64, 1e-5 as test_hip_parity's losses
        assert rel_err(bufs["loss"].t, loss.reshape(1)) < 1e-5 and rel_err(bufs["consensus"].t, cons) < 1e-5
        if with_grad:
            assert rel_err(bufs["grad_logits"].t, grad) < 1e-5
    return check


for _b, _s, _c in [(2, 3, 51), (1, 25, 101), (5, 1, 2)]:
    for _g in (1, 0):
        add(tag("dmc_consensus_ce", _b, _s, _c, "grad" if _g else "nograd"), ["dmc_consensus_ce_fwd_bwd"],
            ce_fn(_b, _s, _c, ce_labels(_b, _c), _g), check=ce_check(_b, _s, _c, _g))


def ce_bad_label_check(bufs):
    """Labels [-1, C, 3] (B = 3, S = 3, C = 51): the loss and the gradient rows of clips 0 and 1 are NaN, clip 2's rows are,
    bit for bit, the rows it gets in a batch of valid labels."""
    from tests.abi_arena import run_case
    b, s, c = 3, 3, 51
    good = run_case(ce_fn(b, s, c, [0, 1, 3], 1), device=DEV)
    g, gg = bufs["grad_logits"].t, good["grad_logits"].t
    assert bool(torch.isnan(bufs["loss"].t).all())
    assert bool(torch.isnan(g[:2 * s]).all()), "gradient rows of the clips with out-of-range labels must be NaN"
    assert not bool(torch.isnan(g[2 * s:]).any()) and torch.equal(g[2 * s:], gg[2 * s:])
    assert torch.equal(bufs["consensus"].t, good["consensus"].t)


add("dmc_consensus_ce-labels-out-of-range", ["dmc_consensus_ce_fwd_bwd"], ce_fn(3, 3, 51, [-1, 51, 3], 1, nan_ok=True),
    check=ce_bad_label_check)


def ce_peak80_check(bufs):
    """|x| reaches 80: the kernel must stay within max(4 x, 1e-6) of the error torch's own fp32 cross entropy makes against
    fp64 on the same inputs (the rule of test_generator_full_batch_vs_oracle); both figures are printed."""
    b, s, c = 4, 3, 51
    labels = ce_labels(b, c)
    cons, loss, grad = ce_ref64(b, s, c, labels, 80.0)
    x = ce_logits(b, s, c, 80.0).requires_grad_(True)
    l32 = F.cross_entropy(x.view(b, s, c).mean(1), torch.tensor(labels))
    l32.backward()
    for name, got, ref32, ref in (("loss", bufs["loss"].t.cpu().reshape(()), l32.detach(), loss), ("grad_logits", bufs["grad_logits"].t.cpu(), x.grad, grad)):
        scale = float(ref.abs().max())
        e_hip = float((got.double() - ref).abs().max()) / scale
        e_ref = float((ref32.double() - ref).abs().max()) / scale
        print("consensus_ce |x| <= 80 %s: kernel %.3e  torch fp32 %.3e (relative to the fp64 value's largest element)" % (name, e_hip, e_ref))
        assert e_hip <= max(4 * e_ref, 1e-6), (name, e_hip, e_ref)
    assert rel_err(bufs["consensus"].t, cons) < 1e-6


add("dmc_consensus_ce-logits-to-80", ["dmc_consensus_ce_fwd_bwd"], ce_fn(4, 3, 51, ce_labels(4, 51), 1, peak=80.0), check=ce_peak80_check)


# =====================================================================================================================
# Discriminator (disc_first, conv_small, conv_nhwc, disc_tail, bn_act.hip) [CONV_CASES, test_disc_tail_unit, test_disc_block_unit]
# =====================================================================================================================
def disc_first(cout, with_keep, with_db):
    m, h, w = 2, 9, 7
    oh, ow = (h - 1) // 2 + 1, (w - 1) // 2 + 1

    def fn(a):
        x, wt = a.inp("x", rnd(60, (m, 2, h, w))), a.inp("w", rnd(61, (cout, 2, 3, 3), 0.3))
        bias = a.inp("bias", rnd(62, (cout,), 0.1))
        keep = a.inp("keep", (pos(63, (m, cout), 0, 1) > 0.25).float() / 0.75) if with_keep else None
        z = a.out("z", (m, oh, ow, cout))
        a.call("dmc_disc_first_fwd", x, wt, bias, keep, z, m, h, w, cout, 1)
        g = a.inp("g", rnd(64, (m, oh, ow, cout)))
        a.call("dmc_disc_first_dgrad", g, wt, a.out("dx", (m, 2, h, w)), m, h, w, cout)
        dw = a.out("dw", (cout, 2, 3, 3))
        db = a.out("db", (cout,)) if with_db else None
        a.call("dmc_disc_first_wgrad", x, g, dw, db, a.work("workspace", L().dmc_disc_first_wgrad_bytes(cout)), m, h, w, cout)

    def check(bufs):
        x, wt, bias, g = rnd(60, (m, 2, h, w)).double(), rnd(61, (cout, 2, 3, 3), 0.3).double(), rnd(62, (cout,), 0.1).double(), rnd(64, (m, oh, ow, cout)).double()
        z = F.leaky_relu(F.conv2d(x, wt, bias, 2, 1), 0.2)
        if with_keep:
            z = z * ((pos(63, (m, cout), 0, 1) > 0.25).double() / 0.75)[:, :, None, None]
        assert rel_err(bufs["z"].t, nhwc(z)) < 1e-5
        xr, wr = x.clone().requires_grad_(True), wt.clone().requires_grad_(True)
        (F.conv2d(xr, wr, None, 2, 1) * g.permute(0, 3, 1, 2)).sum().backward()
        assert rel_err(bufs["dx"].t, xr.grad) < 1e-5 and rel_err(bufs["dw"].t, wr.grad) < 1e-5
        if with_db:
            assert rel_err(bufs["db"].t, g.sum((0, 1, 2))) < 1e-5
    return fn, check


for _cout in (16, 8):
    for _keep, _db in ((1, 1), (1, 0), (0, 1), (0, 0)):
        _fn, _ck = disc_first(_cout, _keep, _db)
        add(tag("dmc_disc_first", _cout, "keep" if _keep else "nokeep", "db" if _db else "nodb"),
            ["dmc_disc_first_fwd", "dmc_disc_first_dgrad", "dmc_disc_first_wgrad"], _fn, check=_ck)

CONV_SHAPES = [(3, 16, 9, 7, 16, 3, 1), (3, 16, 10, 38, 32, 3, 2), (1, 32, 13, 11, 64, 3, 2), (3, 48, 9, 7, 80, 3, 1), (2, 64, 5, 3, 64, 3, 1),
               (1, 128, 6, 2, 64, 1, 1)]


def conv_nhwc(shape, full):
    n, cin, h, w, cout, k, stride = shape
    pad = k // 2
    oh, ow = (h + 2 * pad - k) // stride + 1, (w + 2 * pad - k) // stride + 1
    geom = (n, h, w, cin, cout, k, k, stride, pad)

    def fn(a):
        lib = L()
        assert lib.dmc_conv_nhwc_supported(*geom)
        x = a.inp("x", nhwc(rnd(70, (n, cin, h, w))))
        wt = a.inp("w", nhwc(rnd(71, (cout, cin, k, k), 0.1)))
        wtb = lib.dmc_conv_nhwc_wt_bytes(cin, cout, k, k)
        y = a.out("y", (n, oh, ow, cout))
        if not full:
            a.call("dmc_conv_nhwc_fwd", x, wt, a.work("wpack", wtb), None, None, y, None, 0, *geom, 0)
            return
        bias = a.inp("bias", rnd(72, (cout,), 0.1))
        keep = a.inp("keep", (pos(73, (n, cout), 0, 1) > 0.25).float() / 0.75)
        nblk = lib.dmc_conv_nhwc_stat_blocks(n, h, w, cin, cout, k, stride, pad)
        part = a.out("stat_partials", (nblk, cout, 2), dtype=F64)
        a.call("dmc_conv_nhwc_fwd", x, wt, a.work("wpack", wtb), bias, keep, y, part, nblk, *geom, 1)
        stats = a.out("stats", (2 * cout,))
        rm, rv = a.inout("running_mean", rnd(74, (cout,), 0.1)), a.inout("running_var", pos(75, (cout,)))
        a.call("dmc_conv_nhwc_stats_final", part, nblk, cout, n * oh * ow, stats, rm, rv, 0.8, 0.1)
        dy = a.inp("dy", nhwc(rnd(76, (n, cout, oh, ow))))
        a.call("dmc_conv_nhwc_dgrad", dy, wt, a.work("wt", wtb), a.out("dx", (n, h, w, cin)), *geom)
        a.call("dmc_conv_nhwc_wgrad", x, dy, a.out("dw", (cout, k, k, cin)), opt_work(a, "wgrad_workspace", lib.dmc_conv_nhwc_wgrad_bytes(*geom)), *geom)
        if lib.dmc_conv_nhwc_presplit_supported(cin, cout):
            wf, wtt = a.work("wpack_f", wtb), a.work("wpack_t", wtb)
            a.call("dmc_conv_nhwc_split", wt, wf, wtt, cin, cout, k, k)
            a.call("dmc_conv_nhwc_fwd", x, None, wf, None, None, a.out("y_presplit", (n, oh, ow, cout)), None, 0, *geom, 0)
            a.call("dmc_conv_nhwc_dgrad", dy, None, wtt, a.out("dx_presplit", (n, h, w, cin)), *geom)
            if stride == 1:
                addend = a.inp("addend", nhwc(rnd(77, (n, cin, h, w))))
                a.call("dmc_conv_nhwc_dgrad_add", dy, None, wtt, addend, a.out("dx_add", (n, h, w, cin)), *geom)

    def check(bufs):
        from dmcnet_amd import ops
        x, wt = rnd(70, (n, cin, h, w)).double(), rnd(71, (cout, cin, k, k), 0.1).double()
        ref = F.conv2d(x, wt, None, stride, pad)
        # the wrappers' own calls (ops._conv_fwd / _conv_dgrad / _conv_wgrad) on the same inputs: bit for bit
        xd, wd = x.float().to(DEV).contiguous(memory_format=CL), wt.float().to(DEV).contiguous(memory_format=CL)
        if not full:
            assert same(bufs["y"], nhwc(ops._conv_fwd(xd, wd, None, None, stride, pad, 0, False)[0]))
            assert rel_err(bufs["y"].t, nhwc(ref)) < 1e-5
            return
        keep_d = ((pos(73, (n, cout), 0, 1) > 0.25).float() / 0.75).to(DEV)
        y_w, part_w, _ = ops._conv_fwd(xd, wd, rnd(72, (cout,), 0.1).to(DEV), keep_d, stride, pad, 1, True)
        assert same(bufs["y"], nhwc(y_w)) and torch.equal(bufs["stat_partials"].t, part_w)
        dy_d = rnd(76, (n, cout, oh, ow)).to(DEV).contiguous(memory_format=CL)
        assert same(bufs["dx"], nhwc(ops._conv_dgrad(dy_d, wd, (n, cin, h, w), stride, pad)))
        assert same(bufs["dw"], nhwc(ops._conv_wgrad(xd, dy_d, wd, stride, pad)))
        z = F.leaky_relu(ref + rnd(72, (cout,), 0.1).double()[None, :, None, None], 0.2)
        z = z * ((pos(73, (n, cout), 0, 1) > 0.25).double() / 0.75)[:, :, None, None]
        assert rel_err(bufs["y"].t, nhwc(z)) < 1e-5
        yd = bufs["y"].t.double().cpu()
        s = bufs["stat_partials"].t.sum(0).cpu()
        # (sum, sum of squares) per workgroup row are reduced from fp32 values in fp32 before they are stored as doubles:
        # <= 256 pixels per row, so 256 x 2^-24 = 1.5e-5 bounds the relative error of a row sum; the statistics they feed are fp32
        e0, e1 = rel_err(s[:, 0], yd.sum((0, 1, 2))), rel_err(s[:, 1], (yd * yd).sum((0, 1, 2)))
        print("conv_nhwc %s statistics partials: sum %.3e, sum of squares %.3e" % (shape, e0, e1))
        assert e0 < 1.5e-5 and e1 < 1.5e-5
        mean, var = yd.mean((0, 1, 2)), yd.var((0, 1, 2), unbiased=False)
        st = bufs["stats"].t.cpu().double()
        assert rel_err(st[:cout], mean) < 1e-5 and rel_err(st[cout:], (var + 0.8).rsqrt()) < 1e-5
        assert rel_err(bufs["running_mean"].t, 0.9 * rnd(74, (cout,), 0.1).double() + 0.1 * mean) < 1e-5
        g = rnd(76, (n, cout, oh, ow)).double()
        xr, wr = x.clone().requires_grad_(True), wt.clone().requires_grad_(True)
        (F.conv2d(xr, wr, None, stride, pad) * g).sum().backward()
        assert rel_err(bufs["dx"].t, nhwc(xr.grad)) < 1e-5 and rel_err(bufs["dw"].t, nhwc(wr.grad)) < 1e-5
        if "y_presplit" in bufs:
            assert rel_err(bufs["y_presplit"].t, nhwc(ref)) < 1e-5 and torch.equal(bufs["dx_presplit"].t, bufs["dx"].t)
        if "dx_add" in bufs:
            assert rel_err(bufs["dx_add"].t, nhwc(xr.grad + rnd(77, (n, cin, h, w)).double())) < 1e-5
    return fn, check


for _shape in CONV_SHAPES:
    for _arith in (1, 0):
        for _full in (1, 0):
            _fn, _ck = conv_nhwc(_shape, _full)
            _cov = ["dmc_conv_nhwc_fwd"] + (["dmc_conv_nhwc_stats_final", "dmc_conv_nhwc_split", "dmc_conv_nhwc_dgrad", "dmc_conv_nhwc_dgrad_add",
                                             "dmc_conv_nhwc_wgrad"] if _full else [])
            add(tag("dmc_conv_nhwc", *_shape, "arith%d" % _arith, "full" if _full else "plain"), _cov, _fn, check=_ck, options={"conv_arith": _arith})


def bn_stats_of(x2d, eps=1e-5):
    """(mean, invstd) [2 C] of an [M][C] array, in fp32 as a producer's epilogue would leave them."""
    d = x2d.double()
    return torch.cat([d.mean(0), (d.var(0, unbiased=False) + eps).rsqrt()]).float()


def disc_bn(m, c, n, with_gamma):
    hw = m // n

    def fn(a):
        lib = L()
        assert lib.dmc_bn_act_supported(m, c)
        zt = rnd(80, (m, c))
        z = a.inp("z", zt)
        st = a.inp("stats", bn_stats_of(zt, 0.8))
        gamma, beta = a.inp("gamma", pos(81, (c,))), a.inp("beta", rnd(82, (c,), 0.2))
        a.call("dmc_bn_apply_nhwc", z, gamma, beta, st, a.out("y", (m, c)), m, c)
        res = a.inp("residual", rnd(83, (m, c)))
        mask = a.out("relu_mask", (m * c // 4,), dtype=U8)
        a.call("dmc_bn_apply_act_nhwc", z, res, gamma, beta, st, a.out("y_act", (m, c)), mask, m, c, 1)
        a.call("dmc_bn_apply_act_nhwc", z, None, gamma, beta, st, a.out("y_plain", (m, c)), None, m, c, 0)
        dy = a.inp("dy", rnd(84, (m, c)))
        keep = a.inp("keep", (pos(85, (n, c), 0, 1) > 0.25).float() / 0.75)
        scratch = a.work("scratch", lib.dmc_bn_act_scratch_bytes(c))
        if with_gamma:
            a.call("dmc_bn_bwd_act_nhwc", z, gamma, beta, st, scratch, dy, a.out("dpre", (m, c)), a.out("dgamma", (c,)), a.out("dbeta", (c,)),
                   keep, hw, 0.2, m, c)
        else:           # first block: no BatchNorm
            a.call("dmc_bn_bwd_act_nhwc", z, None, None, None, scratch, dy, a.out("dpre", (m, c)), None, None, keep, hw, 0.2, m, c)
        a.call("dmc_channel_sum_nhwc", dy, a.work("scratch_sum", lib.dmc_bn_act_scratch_bytes(c)), a.out("sum", (c,)), m, c)

    def check(bufs):
        z, dy = rnd(80, (m, c)).double(), rnd(84, (m, c)).double()
        st = bn_stats_of(rnd(80, (m, c)), 0.8).double()
        gamma, beta = pos(81, (c,)).double(), rnd(82, (c,), 0.2).double()
        y = (z - st[:c]) * st[c:] * gamma + beta
        assert rel_err(bufs["y"].t, y) < 1e-5 and torch.equal(bufs["y_plain"].t, bufs["y"].t)
        assert rel_err(bufs["y_act"].t, torch.relu(y + rnd(83, (m, c)).double())) < 1e-5
        assert rel_err(bufs["sum"].t, dy.sum(0)) < 1e-5
        # d(pre) = dz * keep * LeakyReLU'(pre) with z = keep * lrelu(pre) (the sign of z is the sign of pre), dz = the BatchNorm
        # backward of dy (dy itself without a BatchNorm); fp64, 1e-4 as the gradients of test_disc_block_unit
        keep = ((pos(85, (n, c), 0, 1) > 0.25).double() / 0.75).repeat_interleave(hw, 0)
        slope = torch.where(z < 0, torch.full_like(z, 0.2), torch.ones_like(z))
        if with_gamma:
            zr, gr, br = z.clone().requires_grad_(True), gamma.clone().requires_grad_(True), beta.clone().requires_grad_(True)
            F.batch_norm(zr, None, None, gr, br, True, 0.0, 0.8).backward(dy)
            assert rel_err(bufs["dpre"].t, zr.grad * keep * slope) < 1e-4
            assert rel_err(bufs["dgamma"].t, gr.grad) < 1e-4 and rel_err(bufs["dbeta"].t, br.grad) < 1e-4
        else:
            assert rel_err(bufs["dpre"].t, dy * keep * slope) < 1e-5
    return fn, check


for _m, _c, _n in ((189, 16, 3), (143, 64, 11)):
    for _g in (1, 0):
        _fn, _ck = disc_bn(_m, _c, _n, _g)
        add(tag("dmc_bn_nhwc", _m, _c, "gamma" if _g else "nogamma"),
            ["dmc_bn_apply_nhwc", "dmc_bn_apply_act_nhwc", "dmc_bn_bwd_act_nhwc", "dmc_channel_sum_nhwc"], _fn, check=_ck)


def disc_tail(shape, use_bn):
    n, c, h, w = shape

    def fn(a):
        x = a.inp("x", rnd(90, shape))
        keep = a.inp("keep", (pos(91, (n, c), 0, 1) > 0.25).float() / 0.75)
        gamma = beta = rm = rv = stats = None
        if use_bn:
            gamma, beta = a.inp("gamma", pos(92, (c,))), a.inp("beta", rnd(93, (c,), 0.2))
            rm, rv = a.inout("running_mean", rnd(94, (c,), 0.1)), a.inout("running_var", pos(95, (c,)))
            stats = a.work("stats", L().dmc_disc_tail_stats_bytes(c))
        a.call("dmc_disc_tail_fwd", x, keep, gamma, beta, rm, rv, a.out("y", shape), stats, n, c, h, w, use_bn, 1, 0.8, 0.1)
        dy = a.inp("dy", rnd(96, shape))
        dg, db = (a.out("dgamma", (c,)), a.out("dbeta", (c,))) if use_bn else (None, None)
        a.call("dmc_disc_tail_bwd", x, keep, gamma, stats, dy, a.out("dx", shape), dg, db, n, c, h, w, use_bn)

    def check(bufs):
        from dmcnet_amd import ops
        x = rnd(90, shape).to(DEV).requires_grad_(True)
        keep = ((pos(91, (n, c), 0, 1) > 0.25).float() / 0.75).to(DEV)
        bn = None
        if use_bn:
            bn = torch.nn.BatchNorm2d(c, 0.8).to(DEV).train()
            with torch.no_grad():
                bn.weight.copy_(pos(92, (c,))); bn.bias.copy_(rnd(93, (c,), 0.2)); bn.running_mean.copy_(rnd(94, (c,), 0.1)); bn.running_var.copy_(pos(95, (c,)))
        y = ops.disc_tail(x, keep, bn, True)
        y.backward(rnd(96, shape).to(DEV))
        assert same(bufs["y"], y) and same(bufs["dx"], x.grad)
        if use_bn:
            assert same(bufs["dgamma"], bn.weight.grad) and same(bufs["dbeta"], bn.bias.grad)
            assert same(bufs["running_mean"], bn.running_mean) and same(bufs["running_var"], bn.running_var)
    return fn, check


for _shape in ((3, 5, 7, 9), (2, 16, 6, 6)):
    for _bn in (1, 0):
        _fn, _ck = disc_tail(_shape, _bn)
        add(tag("dmc_disc_tail", *_shape, "bn%d" % _bn), ["dmc_disc_tail_fwd", "dmc_disc_tail_bwd"], _fn, check=_ck)


# =====================================================================================================================
# Classifier (stem, bn_act, conv_x3s, conv_x3q) [test_x3s_gpu, test_x3q_gpu, wgrad_addr_shapes]
# =====================================================================================================================
def stem(n, h, w, cl_weight):
    oh, ow = (h + 1) // 2, (w + 1) // 2

    def wt_and_strides():
        wt = rnd(101, (64, 2, 7, 7), 0.1)
        return (nhwc(wt), (98, 1, 14, 2)) if cl_weight else (wt, (98, 49, 7, 1))

    def fn(a):
        lib = L()
        x = a.inp("x", rnd(100, (n, 2, h, w)))
        wt, st = wt_and_strides()
        wt = a.inp("w", wt)
        a.call("dmc_stem_fwd", x, wt, *st, a.out("y", (n, oh, ow, 64)), n, h, w)
        a.call("dmc_stem_fwd_x3", x, wt, *st, a.work("workspace_x3", lib.dmc_stem_fwd_x3_workspace_bytes(n, h, w)), a.out("y_x3", (n, oh, ow, 64)), n, h, w)
        y3 = a.out("y_x3_stats", (n, oh, ow, 64))
        stat = a.work("stat_scratch", lib.dmc_bn_act_scratch_bytes(64))
        a.call("dmc_stem_fwd_x3_stats", x, wt, *st, a.work("workspace_x3s", lib.dmc_stem_fwd_x3_workspace_bytes(n, h, w)), y3, stat, n, h, w)
        a.call("dmc_stem_fwd_x3_stats", x, wt, *st, a.work("workspace_x3n", lib.dmc_stem_fwd_x3_workspace_bytes(n, h, w)), a.out("y_x3_nostats", (n, oh, ow, 64)),
               None, n, h, w)
        if lib.dmc_bn_relu_pool_supported(n, oh, ow, 64):       # the consumer of the partial sums: its results show whether they are well defined
            ph, pw = (oh - 1) // 2 + 1, (ow - 1) // 2 + 1
            a.call("dmc_bn_relu_pool_fwd_arg", y3, a.inp("gamma", pos(102, (64,))), a.inp("beta", rnd(103, (64,), 0.2)),
                   a.inout("running_mean", rnd(105, (64,), 0.1)), a.inout("running_var", pos(106, (64,))), a.out("y_pool", (n, ph, pw, 64)), a.out("ys", nbytes=lib.dmc_x3s_slices_bytes(n * ph * pw, 64), dtype=U8), None, None,
                   a.out("bn_stats", nbytes=lib.dmc_bn_act_stats_bytes(64)), stat, lib.dmc_stem_fwd_x3_stat_blocks(n, h, w), n, oh, ow, 64, 1, 1e-5, 0.1)
        dy = a.inp("dy", rnd(104, (n, oh, ow, 64)))
        if lib.dmc_stem_wgrad_supported(h, w):
            a.call("dmc_stem_wgrad", x, dy, a.out("dw", (64, 2, 7, 7)), a.work("partials", lib.dmc_stem_wgrad_partials_bytes(n, h, w)), n, h, w)
        else:
            assert w % 4 != 0
        assert lib.dmc_stem_dgrad_supported(h, w)
        a.call("dmc_stem_dgrad", dy, wt, *st, a.work("dgrad_workspace", lib.dmc_stem_dgrad_workspace_bytes()), a.out("dx", (n, 2, h, w)), n, h, w)

    def check(bufs):
        x, wt, g = rnd(100, (n, 2, h, w)).double(), rnd(101, (64, 2, 7, 7), 0.1).double(), rnd(104, (n, oh, ow, 64)).double().permute(0, 3, 1, 2)
        ref = nhwc(F.conv2d(x, wt, None, 2, 3))
        for name in ("y", "y_x3", "y_x3_stats"):
            assert rel_err(bufs[name].t, ref) < 1e-5, name
        assert torch.equal(bufs["y_x3_nostats"].t, bufs["y_x3"].t)
        # the wrapper (ops.stem_conv and its autograd) makes the bf16x3 forward, the weight- and the data-gradient call
        from dmcnet_amd import ops
        assert L().dmc_get_option(b"conv_arith") == 1
        xg = rnd(100, (n, 2, h, w)).to(DEV).requires_grad_(True)
        wg = rnd(101, (64, 2, 7, 7), 0.1).to(DEV)
        wg = (wg.contiguous(memory_format=CL) if cl_weight else wg).requires_grad_(True)
        yw = ops.stem_conv(xg, wg)
        yw.backward(rnd(104, (n, oh, ow, 64)).to(DEV).permute(0, 3, 1, 2))
        assert same(bufs["y_x3"], nhwc(yw)) and same(bufs["dx"], xg.grad)
        if "dw" in bufs:
            assert same(bufs["dw"], wg.grad.contiguous())
        xr, wr = x.clone().requires_grad_(True), wt.clone().requires_grad_(True)
        (F.conv2d(xr, wr, None, 2, 3) * g).sum().backward()
        assert rel_err(bufs["dx"].t, xr.grad) < 1e-5
        if "dw" in bufs:
            assert rel_err(bufs["dw"].t, wr.grad) < 1e-5
        if "y_pool" in bufs:
            y = bufs["y_x3_stats"].t.double().cpu().permute(0, 3, 1, 2)
            bn = F.batch_norm(y, None, None, pos(102, (64,)).double(), rnd(103, (64,), 0.2).double(), True, 0.1, 1e-5)
            assert rel_err(bufs["y_pool"].t, nhwc(F.max_pool2d(torch.relu(bn), 3, 2, 1))) < 1e-5
    return fn, check


for _n, _h, _w in ((1, 8, 8), (2, 37, 44), (1, 9, 36)):
    for _cl in (0, 1):
        _fn, _ck = stem(_n, _h, _w, _cl)
        add(tag("dmc_stem", _n, _h, _w, "channels_last_w" if _cl else "contiguous_w"),
            ["dmc_stem_fwd", "dmc_stem_fwd_x3", "dmc_stem_fwd_x3_stats", "dmc_stem_wgrad", "dmc_stem_dgrad", "dmc_bn_relu_pool_fwd_arg"], _fn, check=_ck)


def bn_relu_pool(shape, training, with_codes):
    n, c, h, w = shape
    ph, pw = (h - 1) // 2 + 1, (w - 1) // 2 + 1

    def fn(a):
        lib = L()
        assert lib.dmc_bn_relu_pool_supported(n, h, w, c)
        x = a.inp("x", rnd(110, (n, h, w, c)))
        gamma, beta = a.inp("gamma", pos(111, (c,))), a.inp("beta", rnd(112, (c,), 0.2))
        rm, rv = a.inout("running_mean", rnd(113, (c,), 0.1)), a.inout("running_var", pos(114, (c,)))
        sb, cb = lib.dmc_bn_act_stats_bytes(c), lib.dmc_bn_act_scratch_bytes(c)
        role_stats = a.out if training else a.work          # eval mode normalises with the running statistics: nothing to keep
        stats = role_stats("stats", nbytes=sb)
        scratch = lambda name: a.work(name, cb) if training else None
        a.call("dmc_bn_relu_pool_fwd", x, gamma, beta, rm, rv, a.out("y_pool", (n, ph, pw, c)), stats, scratch("scratch"), n, h, w, c, training, 1e-5, 0.1)
        slices = lib.dmc_x3s_slices_bytes(n * ph * pw, c)
        rm2, rv2 = a.inout("running_mean2", rnd(113, (c,), 0.1)), a.inout("running_var2", pos(114, (c,)))
        a.call("dmc_bn_relu_pool_fwd_x3s", x, gamma, beta, rm2, rv2, a.out("y_pool_x3s", (n, ph, pw, c)), a.out("ys", nbytes=slices, dtype=U8),
               role_stats("stats2", nbytes=sb), scratch("scratch2"), n, h, w, c, training, 1e-5, 0.1)
        rm3, rv3 = a.inout("running_mean3", rnd(113, (c,), 0.1)), a.inout("running_var3", pos(114, (c,)))
        codes = a.work("codes", lib.dmc_bn_relu_pool_codes_bytes(n, h, w, c)) if with_codes else None
        xmax = a.out("xmax", (n, ph, pw, c)) if with_codes else None
        a.call("dmc_bn_relu_pool_fwd_arg", x, gamma, beta, rm3, rv3, a.out("y_pool_arg", (n, ph, pw, c)), a.out("ys_arg", nbytes=slices, dtype=U8),
               codes, xmax, role_stats("stats3", nbytes=sb), scratch("scratch3"), 0, n, h, w, c, training, 1e-5, 0.1)
        if not training:
            return
        dp = a.inp("d_pool", rnd(115, (n, ph, pw, c)))
        codes_b = a.work("codes_bwd", lib.dmc_bn_relu_pool_codes_bytes(n, h, w, c)) if with_codes else None
        a.call("dmc_bn_relu_pool_bwd", x, gamma, beta, stats, a.work("scratch_b", cb), dp, a.out("dx", (n, h, w, c)), a.out("dgamma", (c,)),
               a.out("dbeta", (c,)), codes_b, n, h, w, c)
        if with_codes:
            a.call("dmc_bn_relu_pool_bwd_arg", x, gamma, beta, stats, a.work("scratch_ba", cb), dp, codes, xmax, a.out("dx_arg", (n, h, w, c)),
                   a.out("dgamma_arg", (c,)), a.out("dbeta_arg", (c,)), n, h, w, c)

    def check(bufs):
        x = rnd(110, (n, h, w, c)).double().permute(0, 3, 1, 2).clone().requires_grad_(True)
        gamma, beta = pos(111, (c,)).double().requires_grad_(True), rnd(112, (c,), 0.2).double().requires_grad_(True)
        rm, rv = rnd(113, (c,), 0.1).double(), pos(114, (c,)).double()
        y = F.max_pool2d(torch.relu(F.batch_norm(x, rm, rv, gamma, beta, bool(training), 0.1, 1e-5)), 3, 2, 1)
        assert rel_err(bufs["y_pool"].t, nhwc(y)) < 1e-5
        assert torch.equal(bufs["y_pool_x3s"].t, bufs["y_pool"].t) and torch.equal(bufs["y_pool_arg"].t, bufs["y_pool"].t)
        assert torch.equal(bufs["ys"].u8, bufs["ys_arg"].u8)
        yp = bufs["y_pool"].t
        assert torch.equal(slices_sum(bufs["ys"].u8, c, n * ph * pw), yp.reshape(n * ph * pw, c))     # the three slices sum to the value exactly
        if training:
            assert rel_err(bufs["running_mean"].t, rm) < 1e-5 and rel_err(bufs["running_var"].t, rv) < 1e-5
            assert torch.equal(bufs["running_mean3"].t, bufs["running_mean"].t) and torch.equal(bufs["running_var2"].t, bufs["running_var"].t)
            y.backward(rnd(115, (n, ph, pw, c)).double().permute(0, 3, 1, 2))
            assert rel_err(bufs["dx"].t, nhwc(x.grad)) < 1e-4 and rel_err(bufs["dgamma"].t, gamma.grad) < 1e-4 and rel_err(bufs["dbeta"].t, beta.grad) < 1e-4
            if with_codes:
                assert rel_err(bufs["dx_arg"].t, nhwc(x.grad)) < 1e-4 and rel_err(bufs["dgamma_arg"].t, gamma.grad) < 1e-4
                assert rel_err(bufs["dbeta_arg"].t, beta.grad) < 1e-4
        else:
            assert torch.equal(bufs["running_mean"].t.cpu(), rnd(113, (c,), 0.1)) and torch.equal(bufs["running_var3"].t.cpu(), pos(114, (c,)))
    return fn, check


for _shape in ((2, 64, 17, 23), (1, 64, 1, 5)):
    for _tr in (1, 0):
        for _codes in (1, 0):
            _fn, _ck = bn_relu_pool(_shape, _tr, _codes)
            add(tag("dmc_bn_relu_pool", *_shape, "train" if _tr else "eval", "codes" if _codes else "nocodes"),
                ["dmc_bn_relu_pool_fwd", "dmc_bn_relu_pool_fwd_x3s", "dmc_bn_relu_pool_fwd_arg", "dmc_bn_relu_pool_bwd", "dmc_bn_relu_pool_bwd_arg"], _fn, check=_ck)


def bn_act(m, c, with_res, relu, with_mask):
    """dmc_bn_act_fwd / _bwd and the slice-producing forms on one [M][C] activation: residual, relu and relu_mask as the header
    allows them (a mask is written when there is a residual and a ReLU; a backward given the mask may drop the residual)."""
    def fn(a):
        lib = L()
        assert lib.dmc_bn_act_supported(m, c)
        xt = rnd(120, (m, c))
        x = a.inp("x", xt)
        res = a.inp("residual", rnd(121, (m, c))) if with_res else None
        gamma, beta = a.inp("gamma", pos(122, (c,))), a.inp("beta", rnd(123, (c,), 0.2))
        rm, rv = a.inout("running_mean", rnd(124, (c,), 0.1)), a.inout("running_var", pos(125, (c,)))
        sb, cb, slb = lib.dmc_bn_act_stats_bytes(c), lib.dmc_bn_act_scratch_bytes(c), lib.dmc_x3s_slices_bytes(m, c)
        stats = a.out("stats", nbytes=sb)
        mask = a.out("relu_mask", (m * c // 4,), dtype=U8) if with_mask else None
        a.call("dmc_bn_act_fwd", x, res, gamma, beta, rm, rv, a.out("y", (m, c)), stats, a.work("scratch", cb), mask, m, c, relu, 1, 1e-5, 0.1)
        # eval mode: running statistics, no reduction (scratch NULL)
        rm_e, rv_e = a.inout("running_mean_eval", rnd(124, (c,), 0.1)), a.inout("running_var_eval", pos(125, (c,)))
        a.call("dmc_bn_act_fwd", x, res, gamma, beta, rm_e, rv_e, a.out("y_eval", (m, c)), a.work("stats_eval", sb), None, None, m, c, relu, 0, 1e-5, 0.1)
        # the apply pass with given statistics: fp32 only, slices only, both
        mask_s = a.out("relu_mask_x3s", (m * c // 4,), dtype=U8) if with_mask else None
        a.call("dmc_bn_apply_act_x3s", x, res, gamma, beta, stats, a.out("y_f32", (m, c)), None, mask_s, m, c, relu)
        a.call("dmc_bn_apply_act_x3s", x, res, gamma, beta, stats, None, a.out("ys_only", nbytes=slb, dtype=U8), None, m, c, relu)
        a.call("dmc_bn_apply_act_x3s", x, res, gamma, beta, stats, a.out("y_both", (m, c)), a.out("ys_both", nbytes=slb, dtype=U8), None, m, c, relu)
        dy = a.inp("dy", rnd(126, (m, c)))
        dres = (lambda name: a.out(name, (m, c))) if (with_res and relu) else (lambda name: None)
        # a backward given the mask reads it instead of the residual
        res_b = None if with_mask else res
        a.call("dmc_bn_act_bwd", x, res_b, gamma, beta, stats, a.work("scratch_b", cb), dy, a.out("dx", (m, c)), dres("dresidual"),
               a.out("dgamma", (c,)), a.out("dbeta", (c,)), mask, m, c, relu)
        a.call("dmc_bn_act_bwd_x3s", x, res_b, gamma, beta, stats, a.work("scratch_s", cb), dy, a.out("dx_f32", (m, c)), None, dres("dresidual_s"),
               a.out("dgamma_s", (c,)), a.out("dbeta_s", (c,)), mask, m, c, relu)
        dg, db = a.out("dgamma_s2", (c,)), a.out("dbeta_s2", (c,))
        a.call("dmc_bn_act_bwd_x3s", x, res_b, gamma, beta, stats, a.work("scratch_s2", cb), dy, None, a.out("dxs_only", nbytes=slb, dtype=U8), None,
               dg, db, mask, m, c, relu)
        a.call("dmc_bn_act_bwd_x3s", x, res_b, gamma, beta, stats, a.work("scratch_s3", cb), dy, a.out("dx_both", (m, c)), a.out("dxs_both", nbytes=slb, dtype=U8),
               dres("dresidual_s3"), a.out("dgamma_s3", (c,)), a.out("dbeta_s3", (c,)), mask, m, c, relu)
        a.call("dmc_bn_act_bwd_x3s_apply", x, res_b, gamma, beta, stats, dy, a.out("dx_apply", (m, c)), a.out("dxs_apply", nbytes=slb, dtype=U8),
               dres("dresidual_apply"), dg, db, mask, m, c, relu)
        a.call("dmc_bn_act_bwd_x3s_apply", x, res_b, gamma, beta, stats, dy, a.out("dx_apply_f32", (m, c)), None, dres("dresidual_apply_f32"), dg, db, mask, m, c, relu)
        a.call("dmc_bn_act_bwd_x3s_apply", x, res_b, gamma, beta, stats, dy, None, a.out("dxs_apply_only", nbytes=slb, dtype=U8), None, dg, db, mask, m, c, relu)

    def check(bufs):
        x = rnd(120, (m, c)).double().requires_grad_(True)
        res = rnd(121, (m, c)).double().requires_grad_(True) if with_res else None
        gamma, beta = pos(122, (c,)).double().requires_grad_(True), rnd(123, (c,), 0.2).double().requires_grad_(True)
        rm, rv = rnd(124, (c,), 0.1).double(), pos(125, (c,)).double()
        act = (lambda t: torch.relu(t)) if relu else (lambda t: t)
        y_eval = act(F.batch_norm(x, rm.clone(), rv.clone(), gamma, beta, False, 0.1, 1e-5) + (res if with_res else 0))
        y = act(F.batch_norm(x, rm, rv, gamma, beta, True, 0.1, 1e-5) + (res if with_res else 0))
        assert rel_err(bufs["y"].t, y) < 1e-5 and rel_err(bufs["y_eval"].t, y_eval) < 1e-5
        assert rel_err(bufs["running_mean"].t, rm) < 1e-5 and rel_err(bufs["running_var"].t, rv) < 1e-5
        assert torch.equal(bufs["running_mean_eval"].t.cpu(), rnd(124, (c,), 0.1)), "eval mode must not touch the running statistics"
        for name in ("y_f32", "y_both"):
            assert torch.equal(bufs[name].t, bufs["y"].t), name
        assert torch.equal(bufs["ys_only"].u8, bufs["ys_both"].u8)
        assert torch.equal(slices_sum(bufs["ys_only"].u8, c, m), bufs["y"].t)
        if with_mask:
            assert torch.equal(bufs["relu_mask"].t, bufs["relu_mask_x3s"].t)
        y.backward(rnd(126, (m, c)).double())
        for name in ("dx", "dx_f32", "dx_both", "dx_apply", "dx_apply_f32"):
            assert rel_err(bufs[name].t, x.grad) < 1e-4, name
        for name in ("dgamma", "dgamma_s", "dgamma_s2", "dgamma_s3"):
            assert rel_err(bufs[name].t, gamma.grad) < 1e-4, name
        for name in ("dbeta", "dbeta_s", "dbeta_s2", "dbeta_s3"):
            assert rel_err(bufs[name].t, beta.grad) < 1e-4, name
        # fp32 only, slices only and both give the same bits; the three slices sum to the fp32 value exactly
        assert torch.equal(bufs["dx_both"].t, bufs["dx_f32"].t) and torch.equal(bufs["dxs_both"].u8, bufs["dxs_only"].u8)
        assert torch.equal(bufs["dx_apply_f32"].t, bufs["dx_apply"].t) and torch.equal(bufs["dxs_apply_only"].u8, bufs["dxs_apply"].u8)
        assert torch.equal(bufs["dxs_only"].u8, bufs["dxs_apply"].u8) and torch.equal(bufs["dx_apply"].t, bufs["dx_f32"].t)
        assert torch.equal(slices_sum(bufs["dxs_both"].u8, c, m), bufs["dx_both"].t)
        if with_res and relu:
            for name in ("dresidual", "dresidual_s", "dresidual_s3", "dresidual_apply", "dresidual_apply_f32"):
                assert rel_err(bufs[name].t, res.grad) < 1e-4, name
        if with_res and relu and not with_mask:
            return          # the wrapper always keeps a sign mask for a rectified residual sum: it does not make this call
        # ops.bn_act and its autograd make the dmc_bn_act_fwd / dmc_bn_act_bwd calls of this case: bit for bit
        from dmcnet_amd import ops
        as4 = lambda t: t.to(DEV).view(1, m, 1, c).permute(0, 3, 1, 2)       # [M][C] memory as a channels_last [1, C, M, 1] tensor
        bn = torch.nn.BatchNorm2d(c).to(DEV).train()
        with torch.no_grad():
            bn.weight.copy_(pos(122, (c,))); bn.bias.copy_(rnd(123, (c,), 0.2)); bn.running_mean.copy_(rnd(124, (c,), 0.1)); bn.running_var.copy_(pos(125, (c,)))
        x4 = as4(rnd(120, (m, c))).requires_grad_(True)
        r4 = as4(rnd(121, (m, c))).requires_grad_(True) if with_res else None
        assert ops.bn_act_supported(x4)
        y4 = ops.bn_act(x4, bn, r4, bool(relu))
        y4.backward(as4(rnd(126, (m, c))))
        flat = lambda t: t.permute(0, 2, 3, 1).reshape(m, c)
        assert same(bufs["y"], flat(y4)) and same(bufs["running_mean"], bn.running_mean) and same(bufs["running_var"], bn.running_var)
        assert same(bufs["dx"], flat(x4.grad)) and same(bufs["dgamma"], bn.weight.grad) and same(bufs["dbeta"], bn.bias.grad)
        if with_res and relu:
            assert same(bufs["dresidual"], flat(r4.grad))
    return fn, check


for _m, _c in ((977, 64), (245, 512)):
    for _res, _relu, _mask in ((0, 0, 0), (0, 1, 0), (1, 0, 0), (1, 1, 0), (1, 1, 1)):
        _fn, _ck = bn_act(_m, _c, _res, _relu, _mask)
        add(tag("dmc_bn_act", _m, _c, "res%d" % _res, "relu%d" % _relu, "mask%d" % _mask),
            ["dmc_bn_act_fwd", "dmc_bn_act_bwd", "dmc_bn_apply_act_x3s", "dmc_bn_act_bwd_x3s", "dmc_bn_act_bwd_x3s_apply"], _fn, check=_ck)


def bn_apply_x3q(with_res, relu, f32, slices):
    n, h, w, c = 1, 6, 10, 64
    m = n * h * w

    def fn(a):
        xt = rnd(130, (m, c))
        x, st = a.inp("x", xt), a.inp("stats", bn_stats_of(xt))
        res = a.inp("residual", rnd(131, (m, c))) if with_res else None
        gamma, beta = a.inp("gamma", pos(132, (c,))), a.inp("beta", rnd(133, (c,), 0.2))
        y = a.out("y", (m, c)) if f32 else None
        yq = a.out("yq", nbytes=L().dmc_x3s_slices_bytes(m, c), dtype=U8) if slices else None
        mask = a.out("relu_mask", (m * c // 4,), dtype=U8) if (with_res and relu) else None
        a.call("dmc_bn_apply_act_x3q", x, res, gamma, beta, st, y, yq, mask, n, h, w, c, relu)
        if slices:
            a.call("dmc_x3q_merge", yq, a.out("merged", (m, c)), n, h, w, c)

    def check(bufs):
        x = rnd(130, (m, c)).double()
        st = bn_stats_of(rnd(130, (m, c))).double()
        y = (x - st[:c]) * st[c:] * pos(132, (c,)).double() + rnd(133, (c,), 0.2).double()
        if with_res:
            y = y + rnd(131, (m, c)).double()
        y = torch.relu(y) if relu else y
        for name in ("y", "merged"):
            if name in bufs:
                assert rel_err(bufs[name].t, y) < 1e-5, name
        if f32 and slices:
            assert torch.equal(bufs["y"].t, bufs["merged"].t)
    return fn, check


for _res, _relu in ((0, 0), (0, 1), (1, 0), (1, 1)):
    for _f32, _sl in ((0, 1), (1, 1)):          # the s2d slice output is what this entry point is for: only y is nullable
        _fn, _ck = bn_apply_x3q(_res, _relu, _f32, _sl)
        add(tag("dmc_bn_apply_act_x3q", "res%d" % _res, "relu%d" % _relu, "f32" if _f32 else "", "slices" if _sl else ""),
            ["dmc_bn_apply_act_x3q"] + (["dmc_x3q_merge"] if _sl else []), _fn, check=_ck)


def x3s(shape, variant):
    """variant "a": statistics, addend, both weight images; "b": no statistics, no addend, one weight image per pack call."""
    n, cin, h, w, cout = shape
    m = n * h * w

    def fn(a):
        lib = L()
        assert lib.dmc_x3s_conv_supported(n, h, w, cin, cout) and (h > 2 or lib.dmc_x3s_conv_wgrad_supported(n, h, w, cin, cout))
        x = a.inp("x", nhwc(rnd(140, (n, cin, h, w))))
        xs = a.out("xs", nbytes=lib.dmc_x3s_slices_bytes(m, cin), dtype=U8)
        a.call("dmc_x3s_split", x, xs, m, cin)
        a.call("dmc_x3s_merge", xs, a.out("x_merged", (n, h, w, cin)), m, cin)
        wt = a.inp("w", nhwc(rnd(141, (cout, cin, 3, 3), 0.1)))
        wb = lib.dmc_x3s_wpack_bytes(cin, cout)
        wf, wtt = a.out("wpack_f", nbytes=wb, dtype=U8), a.out("wpack_t", nbytes=wb, dtype=U8)
        if variant == "a":
            a.call("dmc_x3s_pack_weights", wt, wf, wtt, cin, cout)
        else:
            a.call("dmc_x3s_pack_weights", wt, wf, None, cin, cout)
            a.call("dmc_x3s_pack_weights", wt, None, wtt, cin, cout)
        y = a.out("y", (n, h, w, cout))
        if variant == "a":
            nblk = lib.dmc_x3s_conv_stat_blocks(n, h, w, cout)
            a.call("dmc_x3s_conv_fwd", xs, wf, y, a.out("stat_partials", (nblk, cout, 2), dtype=F64), nblk, n, h, w, cin, cout)
        else:
            a.call("dmc_x3s_conv_fwd", xs, wf, y, None, 0, n, h, w, cin, cout)
        dy = a.inp("dy", nhwc(rnd(142, (n, cout, h, w))))
        dys = a.out("dys", nbytes=lib.dmc_x3s_slices_bytes(m, cout), dtype=U8)
        a.call("dmc_x3s_split", dy, dys, m, cout)
        addend = a.inp("addend", nhwc(rnd(143, (n, cin, h, w)))) if variant == "a" else None
        a.call("dmc_x3s_conv_dgrad", dys, wtt, addend, a.out("dx", (n, h, w, cin)), n, h, w, cin, cout)
        # the data gradient that also reduces the BatchNorm-backward sums of the unit whose output gradient it writes
        bn_y = a.inp("bn_y", nhwc(rnd(144, (n, cin, h, w))))
        bn_stats = a.inp("bn_stats", bn_stats_of(nhwc(rnd(144, (n, cin, h, w))).reshape(m, cin)))
        bn_gamma, bn_beta = a.inp("bn_gamma", pos(145, (cin,))), a.inp("bn_beta", rnd(146, (cin,), 0.2))
        nb2 = lib.dmc_x3s_conv_stat_blocks(n, h, w, cin)
        # variant "a": that unit closed a residual block -- its ReLU signs come from the mask its forward pass wrote
        bn_mask = None
        if variant == "a":
            bn_mask = a.out("bn_relu_mask", (m * cin // 4,), dtype=U8)
            a.call("dmc_bn_apply_act_x3s", bn_y, a.inp("bn_residual", nhwc(rnd(147, (n, cin, h, w)))), bn_gamma, bn_beta, bn_stats,
                   a.out("bn_out", (n, h, w, cin)), None, bn_mask, m, cin, 1)
        # (no size query for the partials: the header gives [dmc_x3s_conv_stat_blocks(N, H, W, Cin)][Cin][2] doubles)
        a.call("dmc_x3s_conv_dgrad_bnb", dys, wtt, addend, a.out("dx_bnb", (n, h, w, cin)), bn_y, bn_stats, bn_gamma, bn_beta, bn_mask, 1,
               a.work("bnb_partials", nb2 * cin * 2 * 8), nb2, a.out("bnb_dgamma", (cin,)), a.out("bnb_dbeta", (cin,)), n, h, w, cin, cout)
        if lib.dmc_x3s_conv_wgrad_supported(n, h, w, cin, cout):
            a.call("dmc_x3s_conv_wgrad", xs, dys, a.out("dw", (cout, 3, 3, cin)), opt_work(a, "wgrad_workspace", lib.dmc_x3s_conv_wgrad_bytes(n, h, w, cin, cout)),
                   n, h, w, cin, cout)

    def check(bufs):
        from dmcnet_amd import ops
        x = rnd(140, (n, cin, h, w)).to(DEV).contiguous(memory_format=CL)
        wt = rnd(141, (cout, cin, 3, 3), 0.1).to(DEV).contiguous(memory_format=CL)
        dy = rnd(142, (n, cout, h, w)).to(DEV).contiguous(memory_format=CL)
        xs, dys = ops.x3s_split(x), ops.x3s_split(dy)
        wf, wtt = ops.x3s_pack_weights(wt)
        assert torch.equal(bufs["xs"].u8, xs) and torch.equal(bufs["wpack_f"].u8, wf) and torch.equal(bufs["wpack_t"].u8, wtt)
        assert same(bufs["x_merged"], nhwc(x))
        y, part = ops.x3s_conv_fwd(xs, wf, n, h, w, cin, cout, want_stats=(variant == "a"))
        assert same(bufs["y"], nhwc(y))
        if variant == "a":
            assert torch.equal(bufs["stat_partials"].t, part)
        addend = rnd(143, (n, cin, h, w)).to(DEV).contiguous(memory_format=CL) if variant == "a" else None
        dx = ops.x3s_conv_dgrad(dys, wtt, n, h, w, cin, cout, addend=addend)
        assert same(bufs["dx"], nhwc(dx)) and torch.equal(bufs["dx_bnb"].t, bufs["dx"].t)
        # the BatchNorm-backward sums against fp64: d = dx where the unit's ReLU was on, xhat from (y, stats)
        by = nhwc(rnd(144, (n, cin, h, w))).reshape(m, cin).double()
        st = bn_stats_of(by.float()).double()
        gm, bt = pos(145, (cin,)).double(), rnd(146, (cin,), 0.2).double()
        xhat = (by - st[:cin]) * st[cin:]
        on = (bufs["bn_out"].t.reshape(m, cin).cpu() > 0) if variant == "a" else ((xhat * gm + bt) > 0)     # "a": the signs the unit's forward stored
        if variant == "a":
            ref_out = torch.relu(xhat * gm + bt + nhwc(rnd(147, (n, cin, h, w))).reshape(m, cin).double())
            assert rel_err(bufs["bn_out"].t.reshape(m, cin), ref_out) < 1e-5
        d = bufs["dx"].t.reshape(m, cin).double().cpu() * on
        assert rel_err(bufs["bnb_dbeta"].t, d.sum(0)) < 1e-4 and rel_err(bufs["bnb_dgamma"].t, (d * xhat).sum(0)) < 1e-4
        if "dw" in bufs:
            assert same(bufs["dw"], nhwc(ops.x3s_conv_wgrad(xs, dys, n, h, w, cin, cout)))
    return fn, check


for _shape in ((2, 64, 10, 14, 64), (7, 64, 7, 7, 64), (1, 128, 14, 14, 64), (1, 64, 2, 14, 64)):
    for _v in ("a", "b"):
        _fn, _ck = x3s(_shape, _v)
        add(tag("dmc_x3s", *_shape, _v), ["dmc_x3s_split", "dmc_x3s_merge", "dmc_x3s_pack_weights", "dmc_x3s_conv_fwd", "dmc_x3s_conv_dgrad",
                                           "dmc_x3s_conv_dgrad_bnb", "dmc_x3s_conv_wgrad", "dmc_bn_apply_act_x3s"], _fn, check=_ck)


def x3s_s2():
    n, cin, oh, ow, cout = 2, 64, 7, 7, 128
    h, w = 2 * oh, 2 * ow

    def fn(a):
        lib = L()
        assert lib.dmc_x3s_conv_dgrad_s2_supported(n, oh, ow, cin, cout)
        wt = a.inp("w", nhwc(rnd(150, (cout, cin, 3, 3), 0.1)))
        wt2 = a.out("wpack_t2", nbytes=lib.dmc_x3s_wpack_bytes(cin, cout), dtype=U8)
        a.call("dmc_x3s_pack_weights_s2", wt, wt2, cin, cout)
        dy = a.inp("dy", nhwc(rnd(151, (n, cout, oh, ow))))
        dys = a.out("dys", nbytes=lib.dmc_x3s_slices_bytes(n * oh * ow, cout), dtype=U8)
        a.call("dmc_x3s_split", dy, dys, n * oh * ow, cout)
        a.call("dmc_x3s_conv_dgrad_s2", dys, wt2, a.out("dx", (n, h, w, cin)), n, oh, ow, cin, cout)

    def check(bufs):
        xr = torch.zeros((n, cin, h, w), dtype=F64, requires_grad=True)
        (F.conv2d(xr, rnd(150, (cout, cin, 3, 3), 0.1).double(), None, 2, 1) * rnd(151, (n, cout, oh, ow)).double()).sum().backward()
        assert rel_err(bufs["dx"].t, nhwc(xr.grad)) < 1e-5
    return fn, check


_fn, _ck = x3s_s2()
add("dmc_x3s_conv_dgrad_s2-2-64-7-7-128", ["dmc_x3s_pack_weights_s2", "dmc_x3s_split", "dmc_x3s_conv_dgrad_s2"], _fn, check=_ck)


def x3q(shape, variant):
    n, cin, h, w, cout = shape
    oh, ow = h // 2, w // 2
    m, mq = n * h * w, n * oh * ow

    def fn(a):
        lib = L()
        assert lib.dmc_x3q_supported(n, oh, ow, cin, cout)
        x = a.inp("x", nhwc(rnd(160, (n, cin, h, w))))
        xq = a.out("xq", nbytes=lib.dmc_x3s_slices_bytes(m, cin), dtype=U8)
        a.call("dmc_x3q_split", x, xq, n, h, w, cin)
        a.call("dmc_x3q_merge", xq, a.out("x_merged", (n, h, w, cin)), n, h, w, cin)
        w3, w1 = a.inp("w3", nhwc(rnd(161, (cout, cin, 3, 3), 0.1))), a.inp("w1", rnd(162, (cout, cin), 0.2))
        wb = lib.dmc_x3q_wpack_bytes(cin, cout)
        wf, wtt = a.out("wpack_f", nbytes=wb, dtype=U8), a.out("wpack_t", nbytes=wb, dtype=U8)
        if variant == "a":
            a.call("dmc_x3q_pack_weights", w3, w1, wf, wtt, cin, cout)
        else:
            a.call("dmc_x3q_pack_weights", w3, w1, wf, None, cin, cout)
            a.call("dmc_x3q_pack_weights", w3, w1, None, wtt, cin, cout)
        y3, y1 = a.out("y3", (n, oh, ow, cout)), a.out("y1", (n, oh, ow, cout))
        if variant == "a":
            nblk = lib.dmc_x3q_stat_blocks(n, oh, ow, cout)
            a.call("dmc_x3q_conv_fwd", xq, wf, y3, y1, a.out("stat_partials3", (nblk, cout, 2), dtype=F64), a.out("stat_partials1", (nblk, cout, 2), dtype=F64),
                   nblk, n, oh, ow, cin, cout)
        else:
            a.call("dmc_x3q_conv_fwd", xq, wf, y3, y1, None, None, 0, n, oh, ow, cin, cout)
        slb = lib.dmc_x3s_slices_bytes(mq, cout)
        dys3, dys1 = a.out("dys3", nbytes=slb, dtype=U8), a.out("dys1", nbytes=slb, dtype=U8)
        a.call("dmc_x3s_split", a.inp("dy3", nhwc(rnd(163, (n, cout, oh, ow)))), dys3, mq, cout)
        a.call("dmc_x3s_split", a.inp("dy1", nhwc(rnd(164, (n, cout, oh, ow)))), dys1, mq, cout)
        a.call("dmc_x3q_conv_dgrad", dys3, dys1, wtt, a.out("dx", (n, h, w, cin)), n, oh, ow, cin, cout)
        if lib.dmc_x3q_conv_wgrad_supported(n, oh, ow, cin, cout):
            a.call("dmc_x3q_conv_wgrad", xq, dys3, dys1, a.out("dw3", (cout, 3, 3, cin)), a.out("dw1", (cout, cin)),
                   opt_work(a, "wgrad_workspace", lib.dmc_x3q_conv_wgrad_bytes(n, oh, ow, cin, cout)), n, oh, ow, cin, cout)

    def check(bufs):
        from dmcnet_amd import ops
        x = rnd(160, (n, cin, h, w)).to(DEV).contiguous(memory_format=CL)
        w3 = rnd(161, (cout, cin, 3, 3), 0.1).to(DEV).contiguous(memory_format=CL)
        w1 = rnd(162, (cout, cin), 0.2).view(cout, cin, 1, 1).to(DEV).contiguous(memory_format=CL)
        xq = ops.x3q_split(x)
        wf, wtt = ops.x3q_pack_weights(w3, w1)
        assert torch.equal(bufs["xq"].u8, xq) and torch.equal(bufs["wpack_f"].u8, wf) and torch.equal(bufs["wpack_t"].u8, wtt)
        assert same(bufs["x_merged"], nhwc(x))
        y3, y1, p3, p1 = ops.x3q_conv_fwd(xq, wf, n, oh, ow, cin, cout, want_stats=(variant == "a"))
        assert same(bufs["y3"], nhwc(y3)) and same(bufs["y1"], nhwc(y1))
        if variant == "a":
            assert torch.equal(bufs["stat_partials3"].t, p3) and torch.equal(bufs["stat_partials1"].t, p1)
        dys3 = ops.x3s_split(rnd(163, (n, cout, oh, ow)).to(DEV).contiguous(memory_format=CL))
        dys1 = ops.x3s_split(rnd(164, (n, cout, oh, ow)).to(DEV).contiguous(memory_format=CL))
        assert same(bufs["dx"], nhwc(ops.x3q_conv_dgrad(dys3, dys1, wtt, n, oh, ow, cin, cout)))
        if "dw3" in bufs:
            d3, d1 = ops.x3q_conv_wgrad(xq, dys3, dys1, n, oh, ow, cin, cout)
            assert same(bufs["dw3"], nhwc(d3)) and same(bufs["dw1"], d1.reshape(cout, cin))
    return fn, check


for _shape in ((2, 64, 2, 2, 64), (3, 64, 20, 12, 64), (5, 128, 6, 10, 192), (2, 128, 14, 14, 64), (1, 64, 56, 56, 64)):
    for _v in ("a", "b"):
        _fn, _ck = x3q(_shape, _v)
        add(tag("dmc_x3q", *_shape, _v), ["dmc_x3q_split", "dmc_x3q_merge", "dmc_x3q_pack_weights", "dmc_x3q_conv_fwd", "dmc_x3q_conv_dgrad",
                                           "dmc_x3q_conv_wgrad", "dmc_x3s_split"], _fn, check=_ck)


# =====================================================================================================================
# Data side (prepare.hip, coviar_post.hip) [test_hip_parity prepare cases, test_coviar_post_gpu]
# =====================================================================================================================
def std4():
    std = torch.tensor((0.229, 0.224, 0.225), dtype=F64).float()
    return torch.tensor([float(torch.mean(std)), float(std[0]), float(std[1]), float(std[2])], dtype=torch.float32)


def frames_u8(seed, shape):
    return torch.from_numpy(np.random.RandomState(seed).randint(0, 256, shape).astype(np.uint8))


def prepare(size, factor, optional, interp):
    """``optional``: flip, boxes and src_index given (the frames are then larger than the output and two outputs share a frame)."""
    oh = ow = size
    n_src = 2
    n_out = 3 if optional else n_src
    h0, w0 = (size + 14, size + 9) if optional else (size, size)

    def plans():
        flip = torch.tensor([1, 0, 1][:n_out], dtype=U8)
        boxes = torch.tensor([[3, 2, size + 5, size + 4, size + 2, size + 3, 1, 2], [0, 0, h0, w0, size, size, 0, 0], [7, 4, size, size, size, size, 0, 0]][:n_out],
                             dtype=I32)
        return flip, boxes, torch.tensor([1, 0, 1][:n_out], dtype=I32)

    def fn(a):
        lib = L()
        fr = a.inp("frames_u8", frames_u8(170, (n_src, h0, w0, 7)), slack=16)
        flip = boxes = src = None
        if optional:
            flip, boxes, src = plans()
            flip, boxes, src = a.inp("flip", flip), a.inp("boxes", boxes), a.inp("src_index", src)
        s4 = std4()
        if not optional and not interp:
            a.call("dmc_prepare_inputs", a.inp("frames_plain", frames_u8(170, (n_src, h0, w0, 7))), None, a.out("flow0", (n_src, 2, oh, ow)), a.out("mv0", (n_src, 2, oh, ow)),
                   a.out("res0", (n_src, 3, oh, ow)), opt_work(a, "workspace0", lib.dmc_prepare_inputs_workspace_bytes(n_src, oh, ow, factor)), n_src, oh, ow, factor, s4)
            # the same entry point with the mirror flags (its own kernel: the crop / views cases do not reach it)
            a.call("dmc_prepare_inputs", a.inp("frames_plain_f", frames_u8(170, (n_src, h0, w0, 7))), a.inp("flip_plain", torch.tensor([1, 0], dtype=U8)),
                   a.out("flow0f", (n_src, 2, oh, ow)), a.out("mv0f", (n_src, 2, oh, ow)), a.out("res0f", (n_src, 3, oh, ow)),
                   opt_work(a, "workspace0f", lib.dmc_prepare_inputs_workspace_bytes(n_src, oh, ow, factor)), n_src, oh, ow, factor, s4)
        if not interp:
            # (plans over a shared frame need src_index: the crop entry takes one plan per frame)
            nb = n_src
            a.call("dmc_prepare_inputs_crop", fr, a.inp("boxes_crop", plans()[1][:nb]) if optional else None, a.inp("flip_crop", plans()[0][:nb]) if optional else None,
                   a.out("flow_c", (nb, 2, oh, ow)), a.out("mv_c", (nb, 2, oh, ow)), a.out("res_c", (nb, 3, oh, ow)),
                   opt_work(a, "workspace_c", lib.dmc_prepare_crop_workspace_bytes(nb, oh, ow, factor)), nb, h0, w0, oh, ow, factor, s4)
        a.call("dmc_prepare_inputs_views", fr, src, boxes, flip, a.out("flow_v", (n_out, 2, oh, ow)), a.out("mv_v", (n_out, 2, oh, ow)), a.out("res_v", (n_out, 3, oh, ow)),
               opt_work(a, "workspace_v", lib.dmc_prepare_views_workspace_bytes(n_out, oh, ow, factor, interp)), n_src, n_out, h0, w0, oh, ow, factor, interp, s4)

    def check(bufs):
        from dmcnet_amd import ops
        fr = frames_u8(170, (n_src, h0, w0, 7)).to(DEV)
        flip = boxes = src = None
        if optional:
            flip, boxes, src = (t.to(DEV) for t in plans())
        f, mv, res = ops.prepare_inputs(fr, flip, factor, boxes, (oh, ow), upsample_interp=bool(interp), src_index=src if (optional or interp) else None)
        assert same(bufs["flow_v"], f) and same(bufs["mv_v"], mv) and same(bufs["res_v"], res)
        if "flow_c" in bufs:
            f, mv, res = ops.prepare_inputs(fr, flip[:n_src] if optional else None, factor, boxes[:n_src] if optional else None, (oh, ow))
            assert same(bufs["flow_c"], f) and same(bufs["mv_c"], mv) and same(bufs["res_c"], res)
        if "flow0f" in bufs:       # bit-identical to the reference's loader, hence to the crop entry the wrapper calls with the same flags
            f, mv, res = ops.prepare_inputs(fr, torch.tensor([1, 0], dtype=U8, device=DEV), factor)
            assert same(bufs["flow0f"], f) and same(bufs["mv0f"], mv) and same(bufs["res0f"], res)
            assert not torch.equal(bufs["mv0f"].t[0], bufs["mv0"].t[0]) and torch.equal(bufs["mv0f"].t[1], bufs["mv0"].t[1])
        if "flow0" in bufs:
            assert torch.equal(bufs["flow0"].t, bufs["flow_c"].t) and torch.equal(bufs["mv0"].t, bufs["mv_c"].t) and torch.equal(bufs["res0"].t, bufs["res_c"].t)
    return fn, check


for _size, _factor in ((37, 0), (50, 16)):
    for _opt in (0, 1):
        for _interp in ((0, 1) if _factor else (0,)):
            _fn, _ck = prepare(_size, _factor, _opt, _interp)
            _cov = ["dmc_prepare_inputs_views"] + ([] if _interp else ["dmc_prepare_inputs_crop"]) + (["dmc_prepare_inputs"] if not _opt and not _interp else [])
            add(tag("dmc_prepare", _size, "factor%d" % _factor, "plans" if _opt else "whole", "interp" if _interp else "repeat"), _cov, _fn, check=_ck)


def mv_post(hw, stride, optional):
    """``optional``: emit and bad_source given."""
    H, W = hw

    def data():
        from tests import coviar_post_ref as R
        rs = np.random.RandomState(H * 1000 + W + stride)
        dt = R.AVMV40 if stride == 40 else R.AVMV24
        frames = [np.ascontiguousarray(R.synthetic_mvs(rs, H, W, dt)) for _ in range(3)]
        pics = rs.randint(0, 256, (2, H, W, 3)).astype(np.uint8)
        as_u8 = lambda f: torch.from_numpy(f.view(np.uint8).reshape(-1).copy())
        return frames, [as_u8(f) for f in frames], torch.from_numpy(pics)

    def fn(a):
        lib = L()
        frames, raw, pics = data()
        n0 = len(frames[0])
        mv0 = a.inp("mvs0", raw[0]) if n0 else a.inp("mvs0", torch.zeros(stride, dtype=U8))
        owner = a.work("owner_ws", lib.dmc_mv_owner_bytes(1, H, W))
        bad = a.inout("bad_source", torch.zeros(1, dtype=I32)) if optional else None
        mv_out = a.inout("mv_plane", torch.full((H, W, 2), 7, dtype=I32))         # uncovered pixels keep their value
        a.call("dmc_mv_rasterise", mv0, stride, n0, owner, mv_out, bad, H, W)
        accu = a.out("accu0", (W, H, 2), dtype=I32)
        a.call("dmc_mv_accu_init", accu, H, W)
        accu1 = a.out("accu1", (W, H, 2), dtype=I32)
        a.call("dmc_mv_accumulate", mv0, stride, n0, a.work("owner_ws2", lib.dmc_mv_owner_bytes(1, H, W)), accu, accu1, bad, H, W)
        a.call("dmc_mv_from_accu", accu1, a.out("mv_from_accu", (H, W, 2), dtype=I32), H, W)
        ref, cur = a.inp("bgr_ref", pics[0]), a.inp("bgr_cur", pics[1])
        a.call("dmc_residual", ref, cur, accu1, None, a.out("res_accu", (H, W, 3), dtype=I32), H, W)
        # the non-accumulating residual reads the reference at (x, y) - mv: the plane must be a rasterised one (zero where no
        # vector covers the pixel, as the reference's zero-initialised array), or the source leaves the frame
        mv_zero = a.inout("mv_plane_from_zeros", torch.zeros((H, W, 2), dtype=I32))
        a.call("dmc_mv_rasterise", mv0, stride, n0, a.work("owner_ws3", lib.dmc_mv_owner_bytes(1, H, W)), mv_zero, None, H, W)
        a.call("dmc_residual", ref, cur, None, mv_zero, a.out("res_mv", (H, W, 3), dtype=I32), H, W)
        # two chains (frames 0..1 and frame 2); with `emit` the second chain's outputs stay untouched (INOUT)
        allmv = a.inp("mvs_all", torch.cat(raw) if sum(len(f) for f in frames) else torch.zeros(stride, dtype=U8))
        off = np.cumsum([0] + [len(f) for f in frames]).astype(np.int32)
        d_off, d_chain = a.inp("frame_off", torch.from_numpy(off)), a.inp("chain_off", torch.tensor([0, 2, 3], dtype=I32))
        emit = a.inp("emit", torch.tensor([1, 0], dtype=I32)) if optional else None
        owners = a.work("owners", lib.dmc_mv_owner_bytes(3, H, W))
        refs, curs = a.inp("bgr_ref2", torch.stack([pics[0], pics[1]])), a.inp("bgr_cur2", torch.stack([pics[1], pics[0]]))
        mk = (lambda name, shape: a.inout(name, torch.full(shape, 5, dtype=I32))) if optional else (lambda name, shape: a.out(name, shape, dtype=I32))
        a.call("dmc_mv_gop_batch", allmv, stride, int(off[-1]), d_off, 3, d_chain, 2, emit, owners, refs, curs, mk("accu_b", (2, W, H, 2)), mk("mv_b", (2, H, W, 2)),
               mk("res_b", (2, H, W, 3)), bad, H, W)
        a.call("dmc_mv_gop_batch", allmv, stride, int(off[-1]), d_off, 3, d_chain, 2, emit, a.work("owners2", lib.dmc_mv_owner_bytes(3, H, W)), None, None, None,
               mk("mv_only", (2, H, W, 2)), None, None, H, W)

    def check(bufs):
        from tests import coviar_post_ref as R
        frames, _, pics = data()
        pics = pics.numpy()
        want = np.full((H, W, 2), 7, np.int32)
        R.c_call(frames[0], None, want, None, 1, 0, R.MV, None, None, W, H, 1)
        assert np.array_equal(bufs["mv_plane"].t.cpu().numpy(), want)
        assert np.array_equal(bufs["accu0"].t.cpu().numpy(), R.c_accu_init(H, W))
        mv_z, res_z = np.zeros((H, W, 2), np.int32), np.zeros((H, W, 3), np.int32)
        R.c_call(frames[0], pics, mv_z, res_z, 4, 0, R.RESIDUAL, None, None, W, H, 4)
        assert np.array_equal(bufs["mv_plane_from_zeros"].t.cpu().numpy(), mv_z) and np.array_equal(bufs["res_mv"].t.cpu().numpy(), res_z)
        # one frame through the step API (dmc_mv_accumulate from the identity, dmc_mv_from_accu, dmc_residual with accu)
        a_old = R.c_accu_init(H, W)
        a_src = a_old.copy()
        mv1, res1 = np.zeros((H, W, 2), np.int32), np.zeros((H, W, 3), np.int32)
        R.c_call(frames[0], pics, mv1, None, 1, 1, R.MV, a_src, a_old, W, H, 1)
        R.c_call(np.zeros(0, frames[0].dtype), pics, mv1.copy(), res1, 1, 1, R.RESIDUAL, a_src, a_old, W, H, 1)
        assert np.array_equal(bufs["accu1"].t.cpu().numpy(), a_src) and np.array_equal(bufs["mv_from_accu"].t.cpu().numpy(), mv1)
        assert np.array_equal(bufs["res_accu"].t.cpu().numpy(), res1)
        if optional:
            assert int(bufs["bad_source"].t[0]) == 0
            for name in ("accu_b", "mv_b", "res_b", "mv_only"):
                assert bool((bufs[name].t[1] == 5).all()), "%s: the chain with emit == 0 must stay untouched" % name
        # chain 0 of the batch = two calls of the step API from the identity
        accu_old = R.c_accu_init(H, W)
        accu_src = accu_old.copy()
        mv_want, res_want = np.zeros((H, W, 2), np.int32), np.zeros((H, W, 3), np.int32)
        for t in range(2):
            R.c_call(frames[t], pics, mv_want, None, t + 1, 1, R.MV, accu_src, accu_old, W, H, 2)
        R.c_call(np.zeros(0, frames[0].dtype), pics, mv_want.copy(), res_want, 2, 1, R.RESIDUAL, accu_src, accu_old, W, H, 2)
        assert np.array_equal(bufs["accu_b"].t[0].cpu().numpy(), accu_src) and np.array_equal(bufs["mv_b"].t[0].cpu().numpy(), mv_want)
        assert np.array_equal(bufs["res_b"].t[0].cpu().numpy(), res_want) and torch.equal(bufs["mv_only"].t[0], bufs["mv_b"].t[0])
    return fn, check


for _hw in ((17, 23), (1, 1)):
    for _stride in (40, 24):
        for _opt in (1, 0):
            _fn, _ck = mv_post(_hw, _stride, _opt)
            add(tag("dmc_mv", *_hw, "stride%d" % _stride, "emit-bad" if _opt else "noemit-nobad"),
                ["dmc_mv_accu_init", "dmc_mv_rasterise", "dmc_mv_accumulate", "dmc_mv_from_accu", "dmc_residual", "dmc_mv_gop_batch"], _fn, check=_ck)


# =====================================================================================================================
# I3D (conv3d_bf16, stem3d_bf16, bn3d_bf16, pool3d_bf16, unit3d) [test_conv3d_gpu CASES, POOLS]
# =====================================================================================================================
def conv3d(shape):
    n, cin, d, h, w, cout, k = shape
    t = k ** 3
    geom = (n, d, h, w, cin, cout, k, k, k)
    m = n * d * h * w

    def fn(a):
        lib = L()
        assert lib.dmc_conv3d_bf16_supported(*geom)
        x = a.inp("x", ndhwc(rnd(180, (n, cin, d, h, w))).to(BF))
        wt = a.inp("w", rnd(181, (cout, cin, k, k, k), 0.1))
        wb = lib.dmc_conv3d_bf16_wpack_bytes(cin, cout, k, k, k)
        wf, wbk = a.work("wpack_f", wb), a.work("wpack_b", wb)
        a.call("dmc_conv3d_bf16_pack", wt, cin * t, t, 1, wf, wbk, cin, cout, k, k, k)
        nblk = lib.dmc_conv3d_bf16_stat_blocks_k(*geom)
        a.call("dmc_conv3d_bf16_fwd", x, None, cin * t, t, 1, wf, a.out("y_packed", (m, cout), dtype=BF), a.out("stat_partials", (nblk, cout, 2)), *geom)
        a.call("dmc_conv3d_bf16_fwd", x, wt, cin * t, t, 1, a.work("wpack", wb), a.out("y", (m, cout), dtype=BF), None, *geom)
        dy = a.inp("dy", ndhwc(rnd(182, (n, cout, d, h, w))).to(BF))
        a.call("dmc_conv3d_bf16_dgrad", dy, None, cin * t, t, 1, wbk, a.out("dx_packed", (m, cin), dtype=BF), *geom)
        a.call("dmc_conv3d_bf16_dgrad", dy, wt, cin * t, t, 1, a.work("wpack_d", wb), a.out("dx", (m, cin), dtype=BF), *geom)
        a.call("dmc_conv3d_bf16_wgrad", x, dy, a.out("dw", (cout, cin, k, k, k)), opt_work(a, "wgrad_workspace", lib.dmc_conv3d_bf16_wgrad_bytes(*geom)), *geom)

    def check(bufs):
        from dmcnet_amd import ops
        x = rnd(180, (n, cin, d, h, w)).to(BF).to(DEV).contiguous(memory_format=torch.channels_last_3d).requires_grad_(True)
        wt = rnd(181, (cout, cin, k, k, k), 0.1).to(DEV).requires_grad_(True)
        y = ops.conv3d_bf16(x, wt)
        y.backward(rnd(182, (n, cout, d, h, w)).to(BF).to(DEV))
        assert same(bufs["y"], ndhwc(y)) and torch.equal(bufs["y_packed"].t, bufs["y"].t)
        assert same(bufs["dx"], ndhwc(x.grad)) and torch.equal(bufs["dx_packed"].t, bufs["dx"].t) and same(bufs["dw"], wt.grad)
        yd = bufs["y"].t.double().cpu()
        s = bufs["stat_partials"].t.double().sum(0).cpu()
        assert rel_err(s[:, 0], yd.sum(0)) < 1e-4 and rel_err(s[:, 1], (yd * yd).sum(0)) < 1e-4
    return fn, check


for _shape in ((1, 24, 3, 5, 6, 64, 3), (1, 208, 5, 4, 3, 48, 1), (1, 32, 3, 5, 28, 40, 3)):
    _fn, _ck = conv3d(_shape)
    add(tag("dmc_conv3d_bf16", *_shape), ["dmc_conv3d_bf16_pack", "dmc_conv3d_bf16_fwd", "dmc_conv3d_bf16_dgrad", "dmc_conv3d_bf16_wgrad"], _fn, check=_ck)

POOLS = [((3, 3, 3), (1, 1, 1), (2, 16, 1, 3, 2)), ((3, 3, 3), (1, 1, 1), (1, 24, 2, 5, 11)), ((1, 3, 3), (1, 3, 3), (1, 8, 2, 9, 13))]


def maxpool(kernel, stride, shape):
    n, c, d, h, w = shape

    def out_shape():
        import ctypes
        od, oh, ow = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
        assert L().dmc_maxpool3d_tf_out_shape(d, h, w, c, *kernel, *stride, ctypes.byref(od), ctypes.byref(oh), ctypes.byref(ow)) == 1
        return od.value, oh.value, ow.value

    def fn(a):
        od, oh, ow = out_shape()
        x = a.inp("x", ndhwc(torch.relu(rnd(190, shape))).to(BF))
        y, code = a.out("y", (n, od, oh, ow, c), dtype=BF), a.out("code", (n * od * oh * ow * c,), dtype=U8)
        a.call("dmc_maxpool3d_tf_bf16_fwd", x, y, code, n, d, h, w, c, *kernel, *stride)
        dy = a.inp("dy", ndhwc(rnd(191, (n, c, od, oh, ow))).to(BF))
        a.call("dmc_maxpool3d_tf_bf16_bwd", dy, code, a.out("dx", (n, d, h, w, c), dtype=BF), n, d, h, w, c, *kernel, *stride)

    def check(bufs):
        from dmcnet_amd import ops
        od, oh, ow = out_shape()
        x = torch.relu(rnd(190, shape)).to(BF).to(DEV).contiguous(memory_format=torch.channels_last_3d).requires_grad_(True)
        y = ops.maxpool3d_tf(x, kernel, stride)
        y.backward(rnd(191, (n, c, od, oh, ow)).to(BF).to(DEV))
        assert same(bufs["y"], ndhwc(y)) and same(bufs["dx"], ndhwc(x.grad))
    return fn, check


for _k, _s, _shape in POOLS:
    _fn, _ck = maxpool(_k, _s, _shape)
    add(tag("dmc_maxpool3d_tf_bf16", *_k, *_s, *_shape), ["dmc_maxpool3d_tf_bf16_fwd", "dmc_maxpool3d_tf_bf16_bwd"], _fn, check=_ck)


def bn3d(running):
    m, c, ld, c0 = 90, 48, 88, 16

    def tensors():
        y = rnd(200, (m, c)).to(BF)
        yd = y.double()
        part = torch.stack([yd.sum(0), (yd * yd).sum(0)], 1).float().reshape(1, c, 2)       # one block of (sum, sum of squares)
        return y, part, rnd(203, (m, ld)).to(BF), rnd(204, (m, ld)).to(BF)

    def fn(a):
        yt, part, wide, dwide = tensors()
        y, part = a.inp("y", yt), a.inp("partials", part)
        gamma, beta = a.inp("gamma", pos(201, (c,))), a.inp("beta", rnd(202, (c,), 0.2))
        rm = a.inout("running_mean", rnd(205, (c,), 0.1)) if running else None
        rv = a.inout("running_var", pos(206, (c,))) if running else None
        stats = a.out("stats", (2 * c,))
        a.call("dmc_bn3d_bf16_fwd", y, part, 1, gamma, beta, stats, rm, rv, a.out("out", (m, c), dtype=BF), m, c, 1, 1e-3, 0.1)
        # a channel slice (columns 16 .. 63) of an 88-wide tensor: the columns around it must survive
        wide = a.inout("out_wide", wide)
        rm2 = a.inout("running_mean2", rnd(205, (c,), 0.1)) if running else None
        rv2 = a.inout("running_var2", pos(206, (c,))) if running else None
        a.call("dmc_bn3d_bf16_fwd_ld", y, part, 1, gamma, beta, a.out("stats2", (2 * c,)), rm2, rv2, wide.at(2 * c0), ld, m, c, 1, 1e-3, 0.1)
        dout = a.inp("dout_wide", dwide)
        a.call("dmc_bn3d_bf16_bwd", dout.at(2 * c0), ld, y, stats, gamma, beta, a.work("scratch", L().dmc_bn3d_bf16_scratch_bytes(c)),
               a.out("dy", (m, c), dtype=BF), a.out("dgamma", (c,)), a.out("dbeta", (c,)), m, c, 1)

    def check(bufs):
        yt, _, wide, dwide = tensors()
        got = bufs["out_wide"].t.cpu()
        assert torch.equal(got[:, :c0], wide[:, :c0]) and torch.equal(got[:, c0 + c:], wide[:, c0 + c:]), "columns outside the slice were written"
        assert torch.equal(got[:, c0:c0 + c], bufs["out"].t.cpu()) and torch.equal(bufs["stats"].t, bufs["stats2"].t)
        y = yt.double().requires_grad_(True)
        gamma, beta = pos(201, (c,)).double().requires_grad_(True), rnd(202, (c,), 0.2).double().requires_grad_(True)
        rm, rv = rnd(205, (c,), 0.1).double(), pos(206, (c,)).double()
        ref = torch.relu(F.batch_norm(y, rm, rv, gamma, beta, True, 0.1, 1e-3))
        assert bf16_close(bufs["out"].t, ref.detach())
        if running:
            assert rel_err(bufs["running_mean"].t, rm) < 1e-5 and rel_err(bufs["running_var"].t, rv) < 1e-5
            assert torch.equal(bufs["running_var2"].t, bufs["running_var"].t)
        ref.backward(dwide[:, c0:c0 + c].double())
        assert bf16_close(bufs["dy"].t, y.grad)
        assert rel_err(bufs["dgamma"].t, gamma.grad) < 2e-3 and rel_err(bufs["dbeta"].t, beta.grad) < 2e-3
    return fn, check


for _r in (1, 0):
    _fn, _ck = bn3d(_r)
    add(tag("dmc_bn3d_bf16-90-48-ld88", "running" if _r else "norunning"), ["dmc_bn3d_bf16_fwd", "dmc_bn3d_bf16_fwd_ld", "dmc_bn3d_bf16_bwd"], _fn, check=_ck)


def add4(n):
    def fn(a):
        ins = [a.inp("abcd"[i], rnd(210 + i, (n,)).to(BF)) for i in range(4)]
        a.call("dmc_add4_bf16", *ins, a.out("out", (n,), dtype=BF), n)

    def check(bufs):
        t = [rnd(210 + i, (n,)).to(BF) for i in range(4)]
        assert torch.equal(bufs["out"].t.cpu(), ((t[0] + t[1]) + t[2]) + t[3])
    return fn, check


for _n in (8, 4104):
    _fn, _ck = add4(_n)
    add(tag("dmc_add4_bf16", _n), ["dmc_add4_bf16"], _fn, check=_ck)


def unit3d(null):
    """``null``: which of the backward's nullable gradients is dropped ("", "dx", "dw")."""
    n, cin, d, h, w, cout, k = 2, 32, 3, 6, 5, 48, 3
    geom = (n, d, h, w, cin, cout, k, k, k)
    m, ld, c0 = n * d * h * w, 88, 16

    def fn(a):
        lib = L()
        x = a.inp("x", ndhwc(rnd(220, (n, cin, d, h, w))).to(BF))
        wt = a.inp("w", rnd(221, (cout, cin, k, k, k), 0.1))
        gamma, beta = a.inp("gamma", pos(222, (cout,))), a.inp("beta", rnd(223, (cout,), 0.2))
        rm, rv = a.inout("running_mean", rnd(224, (cout,), 0.1)), a.inout("running_var", pos(225, (cout,)))
        fws = a.work("fwd_workspace", lib.dmc_unit3d_bf16_fwd_workspace_bytes(*geom))
        y = a.out("y", (m, cout), dtype=BF)
        a.call("dmc_unit3d_bf16_fwd", x, wt, gamma, beta, rm, rv, fws, y, a.out("out", (m, cout), dtype=BF), *geom, 1, 1e-5, 0.1)
        rm2, rv2 = a.inout("running_mean2", rnd(224, (cout,), 0.1)), a.inout("running_var2", pos(225, (cout,)))
        wide = a.inout("out_wide", rnd(226, (m, ld)).to(BF))
        a.call("dmc_unit3d_bf16_fwd_into", x, wt, gamma, beta, rm2, rv2, a.work("fwd_workspace2", lib.dmc_unit3d_bf16_fwd_workspace_bytes(*geom)),
               a.out("y2", (m, cout), dtype=BF), wide.at(2 * c0), ld, *geom, 1, 1e-5, 0.1)
        wide_e = a.inout("eval_wide", rnd(226, (m, ld)).to(BF))
        a.call("dmc_unit3d_bf16_fwd_eval", x, wt, gamma, beta, a.inp("rm_eval", rnd(224, (cout,), 0.1)), a.inp("rv_eval", pos(225, (cout,))), 1e-3,
               a.work("eval_workspace", lib.dmc_unit3d_bf16_eval_workspace_bytes(*geom)), wide_e.at(2 * c0), ld, *geom, 1)
        dout = a.inp("dout_wide", rnd(227, (m, ld)).to(BF))
        dx = None if null == "dx" else a.out("dx", (m, cin), dtype=BF)
        dw = None if null == "dw" else a.out("dw", (cout, cin, k, k, k))
        a.call("dmc_unit3d_bf16_bwd", dout.at(2 * c0), ld, x, y, fws, gamma, beta, a.work("bwd_workspace", lib.dmc_unit3d_bf16_bwd_workspace_bytes(*geom)),
               a.out("dy", (m, cout), dtype=BF), dx, dw, a.out("dgamma", (cout,)), a.out("dbeta", (cout,)), *geom, 1)

    def check(bufs):
        from dmcnet_amd import ops
        wide0 = rnd(226, (m, ld)).to(BF)
        for name in ("out_wide", "eval_wide"):
            got = bufs[name].t.cpu()
            assert torch.equal(got[:, :c0], wide0[:, :c0]) and torch.equal(got[:, c0 + cout:], wide0[:, c0 + cout:]), name
        assert torch.equal(bufs["out_wide"].t[:, c0:c0 + cout], bufs["out"].t) and torch.equal(bufs["y2"].t, bufs["y"].t)
        assert torch.equal(bufs["running_mean2"].t, bufs["running_mean"].t)
        # the wrapper makes the same calls (dmc_unit3d_bf16_fwd_into with a dense output, dmc_unit3d_bf16_bwd on a slice gradient)
        conv, bn = torch.nn.Conv3d(cin, cout, k, padding=k // 2, bias=False).to(DEV), torch.nn.BatchNorm3d(cout).to(DEV).train()
        with torch.no_grad():
            conv.weight.copy_(rnd(221, (cout, cin, k, k, k), 0.1)); bn.weight.copy_(pos(222, (cout,))); bn.bias.copy_(rnd(223, (cout,), 0.2))
            bn.running_mean.copy_(rnd(224, (cout,), 0.1)); bn.running_var.copy_(pos(225, (cout,)))
        assert bn.eps == 1e-5 and bn.momentum == 0.1
        x = rnd(220, (n, cin, d, h, w)).to(BF).to(DEV).contiguous(memory_format=torch.channels_last_3d).requires_grad_(True)
        out = ops.conv_bn_relu3d(x, conv, bn, True)
        gw = rnd(227, (m, ld)).to(BF).to(DEV).view(n, d, h, w, ld).permute(0, 4, 1, 2, 3)
        out.backward(gw[:, c0:c0 + cout])
        assert same(bufs["out"], ndhwc(out)) and same(bufs["running_var"], bn.running_var)
        assert same(bufs["dgamma"], bn.weight.grad) and same(bufs["dbeta"], bn.bias.grad)
        if "dx" in bufs:
            assert same(bufs["dx"], ndhwc(x.grad))
        if "dw" in bufs:
            assert same(bufs["dw"], conv.weight.grad)
        # dy (the gradient handed to the convolution) is internal to the wrapper: the ReLU + BatchNorm backward of the slice
        # gradient through the SAME bf16 convolution output, in fp64, within one bf16 rounding (as test_conv3d_gpu does)
        yr = bufs["y"].t.double().cpu().requires_grad_(True)
        torch.relu(F.batch_norm(yr, None, None, pos(222, (cout,)).double(), rnd(223, (cout,), 0.2).double(), True, 0.1, 1e-5)).backward(
            rnd(227, (m, ld)).to(BF)[:, c0:c0 + cout].double())
        assert bf16_close(bufs["dy"].t, yr.grad)
        # eval mode: ops.conv_bn_relu3d_eval makes the same call (running statistics as the case gave them: the initial ones)
        bn_e = torch.nn.BatchNorm3d(cout).to(DEV).eval()
        with torch.no_grad():
            bn_e.weight.copy_(pos(222, (cout,))); bn_e.bias.copy_(rnd(223, (cout,), 0.2))
            bn_e.running_mean.copy_(rnd(224, (cout,), 0.1)); bn_e.running_var.copy_(pos(225, (cout,)))
            bn_e.eps = 1e-3
            ev = ops.conv_bn_relu3d_eval(x.detach(), conv, bn_e, True)
        assert same_t(bufs["eval_wide"].t[:, c0:c0 + cout], ndhwc(ev).reshape(m, cout))
    return fn, check


for _null in ("", "dx", "dw"):
    _fn, _ck = unit3d(_null)
    add(tag("dmc_unit3d_bf16-2-32-3-6-5-48-3", "no" + _null if _null else "all"),
        ["dmc_unit3d_bf16_fwd", "dmc_unit3d_bf16_fwd_into", "dmc_unit3d_bf16_fwd_eval", "dmc_unit3d_bf16_bwd"], _fn, check=_ck)


def stem3d(shape):
    n, _, t, h, w = shape
    od, oh, ow = (t - 2) // 2 + 1, (h - 2) // 2 + 1, (w - 2) // 2 + 1
    m = n * od * oh * ow

    def fn(a):
        lib = L()
        x, wt = a.inp("x", rnd(230, shape)), a.inp("w", rnd(231, (64, 2, 7, 7, 7), 0.05))
        nblk = lib.dmc_stem3d_bf16_stat_blocks(n, t, h, w)
        a.call("dmc_stem3d_bf16_fwd", x, wt, a.work("workspace", lib.dmc_stem3d_bf16_workspace_bytes(n, t, h, w)), a.out("y", (m, 64), dtype=BF),
               a.out("stat_partials", (nblk, 64, 2)), n, t, h, w)
        a.call("dmc_stem3d_bf16_fwd", x, wt, a.work("workspace2", lib.dmc_stem3d_bf16_workspace_bytes(n, t, h, w)), a.out("y_nostats", (m, 64), dtype=BF),
               None, n, t, h, w)
        a.call("dmc_stem3d_bf16_fwd_eval", x, wt, a.inp("gamma", pos(232, (64,))), a.inp("beta", rnd(233, (64,), 0.2)), a.inp("running_mean", rnd(234, (64,), 0.1)),
               a.inp("running_var", pos(235, (64,))), 1e-3, a.work("eval_workspace", lib.dmc_stem3d_bf16_eval_workspace_bytes(n, t, h, w)),
               a.out("y_eval", (m, 64), dtype=BF), n, t, h, w, 1)
        dy = a.inp("dy", rnd(236, (m, 64)).to(BF))
        a.call("dmc_stem3d_bf16_wgrad", x, dy, a.out("dw", (64, 2, 7, 7, 7)), opt_work(a, "wgrad_workspace", lib.dmc_stem3d_bf16_wgrad_workspace_bytes(n, t, h, w)), n, t, h, w)
        a.call("dmc_stem3d_bf16_dgrad", dy, wt, a.out("dx", shape), a.work("dgrad_workspace", lib.dmc_stem3d_bf16_dgrad_workspace_bytes()), n, t, h, w)

    def check(bufs):
        x = rnd(230, shape).to(BF).double().requires_grad_(True)
        wt = rnd(231, (64, 2, 7, 7, 7), 0.05).to(BF).double().requires_grad_(True)
        y = F.conv3d(F.pad(x, (2, 3, 2, 3, 2, 3)), wt, None, 2, 0)
        ref = ndhwc(y.detach()).reshape(m, 64)
        assert bf16_close(bufs["y"].t, ref) and torch.equal(bufs["y_nostats"].t, bufs["y"].t)
        yd = bufs["y"].t.double().cpu()
        s = bufs["stat_partials"].t.double().sum(0).cpu()
        assert rel_err(s[:, 0], yd.sum(0)) < 1e-4 and rel_err(s[:, 1], (yd * yd).sum(0)) < 1e-4
        scale = pos(232, (64,)).double() / (pos(235, (64,)).double() + 1e-3).sqrt()
        shift = rnd(233, (64,), 0.2).double() - rnd(234, (64,), 0.1).double() * scale
        assert bf16_close(bufs["y_eval"].t, torch.relu(ref * scale + shift))
        g = rnd(236, (m, 64)).to(BF).double().view(n, od, oh, ow, 64).permute(0, 4, 1, 2, 3)
        (y * g).sum().backward()
        assert rel_err(bufs["dw"].t, wt.grad) < 2e-5 and rel_err(bufs["dx"].t, x.grad) < 2e-5
    return fn, check


for _shape in ((1, 2, 6, 10, 24), (1, 2, 5, 9, 250)):
    _fn, _ck = stem3d(_shape)
    add(tag("dmc_stem3d_bf16", *_shape), ["dmc_stem3d_bf16_fwd", "dmc_stem3d_bf16_fwd_eval", "dmc_stem3d_bf16_wgrad", "dmc_stem3d_bf16_dgrad"], _fn, check=_ck)
