"""torch.autograd bindings of the HIP kernels (device memory and streams are PyTorch's; the
arithmetic is libdmcnet_hip.so's).  Every op requires contiguous fp32 CUDA tensors and raises
otherwise -- there is no CPU path."""
import torch

from . import _lib

__all__ = ["gen_tiny", "flow_mse", "flow_loss", "gen_tiny_loss", "FLOW_LOSS_KINDS", "consensus_ce", "disc_tail", "bn_act", "bn_act_supported", "prepare_inputs",
           "u8_frames_buffer", "conv_nhwc", "conv_nhwc_supported", "disc_block", "disc_block_supported", "disc_head", "disc_head_supported"]


class EventProbe(object):
    """HIP-event timing of individual C-ABI calls on the stream they are launched on (PyTorch's
    current stream).  bench.py installs one over the timed region to obtain the generator
    kernels' average duration; ``summary()`` synchronises."""

    def __init__(self, only=None):
        self.pairs = {}
        self.only = None if only is None else frozenset(only)   # restrict to these span names (fewer event records)

    def span(self, name):
        return _Span(self, name)

    def summary(self):
        torch.cuda.synchronize()
        return {k: (sum(a.elapsed_time(b) for a, b in v) / len(v), len(v))
                for k, v in self.pairs.items() if v}


class _Span(object):
    def __init__(self, probe, name):
        self.probe, self.name = probe, name

    def __enter__(self):
        self.a = torch.cuda.Event(enable_timing=True)
        self.b = torch.cuda.Event(enable_timing=True)
        self.a.record()

    def __exit__(self, *exc):
        self.b.record()
        self.probe.pairs.setdefault(self.name, []).append((self.a, self.b))


class _NoSpan(object):
    def __enter__(self):
        return None

    def __exit__(self, *exc):
        return False


PROBE = None          # set to an EventProbe to time the calls below
#: test hook: a list that receives every discriminator block's z = keep * LeakyReLU(conv + bias) (the
#: tensor whose sign pattern decides the LeakyReLU branches), in call order; None = off
DEBUG_DISC_Z = None


def _span(name):
    if PROBE is None or (PROBE.only is not None and name not in PROBE.only):
        return _NoSpan()
    return PROBE.span(name)


_RAW_STREAM = getattr(torch._C, "_cuda_getCurrentRawStream", None)
_CUR_DEVICE = getattr(torch._C, "_cuda_getDevice", None)


def _stream():
    """The HIP stream PyTorch is launching on (every C-ABI call takes it).  Through the raw getter: 0.3 us instead of the
    9 us of ``torch.cuda.current_stream()`` (a Stream object per call) -- at 2-3 calls per op that was ~2 ms of host time
    per I3D micro-step, which is launch-bound."""
    if _RAW_STREAM is not None and _CUR_DEVICE is not None:
        return _lib._P(_RAW_STREAM(_CUR_DEVICE()))
    return _lib._P(torch.cuda.current_stream().cuda_stream)


def profile_mark():
    """Bracket a region in a rocprofv3 kernel trace (see tools/rocprof_region.py)."""
    _lib.check(_lib.load().dmc_profile_mark(_stream()), "dmc_profile_mark")


def _need_cuda(*tensors):
    for t in tensors:
        if t is None:
            continue
        if not t.is_cuda:
            raise _lib.DmcHipError("the DMC-Net hot path runs on the HIP extension only: got a %s "
                                   "tensor (no CPU fallback)" % t.device)
        if t.dtype not in (torch.float32, torch.int64):
            raise _lib.DmcHipError("expected fp32 tensors, got %s" % t.dtype)


def _floats(nbytes, device):
    return torch.empty((nbytes + 3) // 4, dtype=torch.float32, device=device)


class _GenTiny(torch.autograd.Function):
    """EstimatorDenseNetTiny(cat(mv, res)) [+ mv]; reference code/dmcnet/model.py:187-194,341-346."""

    @staticmethod
    def forward(ctx, mv, res, add_mv, grad_mode, *params):
        lib = _lib.load()
        _need_cuda(mv, res, *params)
        if ctx.needs_input_grad[0] or ctx.needs_input_grad[1]:
            raise NotImplementedError("gradients w.r.t. the MV/residual inputs are not produced "
                                      "(the reference never requests them)")
        mv, res = mv.contiguous(), res.contiguous()
        ws, bs = [p.contiguous() for p in params[:6]], [p.contiguous() for p in params[6:]]
        n, _, h, w = mv.shape
        out = torch.empty((n, 2, h, w), dtype=torch.float32, device=mv.device)
        # inference (no parameter wants a gradient, or torch.no_grad()): the one-launch forward keeps no features -- 8 instead
        # of 120 B/px written.  needs_input_grad reflects the tensors' requires_grad only, NOT the grad mode (it reads True
        # under no_grad, and torch.is_grad_enabled() is always False in here): the caller passes the mode, `grad_mode`.
        keep = (grad_mode and any(ctx.needs_input_grad[4:])) or not ((lib.dmc_get_option(b"gen_fused") & 1) and w <= 224)
        saved = _floats(lib.dmc_gen_tiny_saved_bytes(n, h, w), mv.device) if keep else None
        work = _floats(lib.dmc_gen_tiny_workspace_bytes(), mv.device)
        with _span("gen_tiny_fwd"):
            _lib.check(lib.dmc_gen_tiny_fwd(_lib.ptr(mv), _lib.ptr(res), _lib.ptr_array(ws),
                                            _lib.ptr_array(bs), _lib.ptr(out), _lib.ptr(saved) if keep else None,
                                            _lib.ptr(work), n, h, w, int(add_mv), _stream()),
                       "dmc_gen_tiny_fwd")
        if not keep:
            return out
        ctx.save_for_backward(mv, res, saved, *ws)
        ctx.bias_like = [(b.shape, b.dtype) for b in bs]
        return out

    @staticmethod
    def backward(ctx, grad_out):
        lib = _lib.load()
        mv, res, saved = ctx.saved_tensors[:3]
        ws = list(ctx.saved_tensors[3:])
        grad_out = grad_out.contiguous()
        n, _, h, w = mv.shape
        dws = [torch.empty_like(x) for x in ws]
        dbs = [torch.empty(s, dtype=d, device=mv.device) for s, d in ctx.bias_like]
        gbuf = _floats(lib.dmc_gen_tiny_gbuf_bytes(n, h, w), mv.device)
        partials = _floats(lib.dmc_gen_tiny_partials_bytes(n, h, w), mv.device)
        work = _floats(lib.dmc_gen_tiny_workspace_bytes(), mv.device)
        with _span("gen_tiny_bwd"):
            _lib.check(lib.dmc_gen_tiny_bwd(_lib.ptr(mv), _lib.ptr(res), _lib.ptr_array(ws),
                                            _lib.ptr(saved), _lib.ptr(grad_out), _lib.ptr_array(dws),
                                            _lib.ptr_array(dbs), _lib.ptr(gbuf), _lib.ptr(partials),
                                            _lib.ptr(work), n, h, w, _stream()),
                       "dmc_gen_tiny_bwd")
        return (None, None, None, None) + tuple(dws) + tuple(dbs)


class _GenTinyMSE(torch.autograd.Function):
    """(gen_flow, MSELoss(gen_flow, flow)) with the loss reduced in the epilogue of the kernel that writes
    gen_flow: EstimatorDenseNetTiny(cat(mv, res)) [+ mv] (code/dmcnet/model.py:187-194,341-346) followed by
    ``criterion_mse(gen_flow, input_flow)`` (code/dmcnet/train.py:167,245).  Backward = the flow-MSE gradient
    (plus whatever else reaches gen_flow) through the generator's backward, as with the separate ops."""

    @staticmethod
    def forward(ctx, mv, res, flow, add_mv, *params):
        lib = _lib.load()
        _need_cuda(mv, res, flow, *params)
        if ctx.needs_input_grad[0] or ctx.needs_input_grad[1] or ctx.needs_input_grad[2]:
            raise NotImplementedError("no gradients w.r.t. the MV / residual / flow inputs")
        mv, res, flow = mv.contiguous(), res.contiguous(), flow.contiguous()
        ws, bs = [p.contiguous() for p in params[:6]], [p.contiguous() for p in params[6:]]
        n, _, h, w = mv.shape
        if tuple(flow.shape) != (n, 2, h, w):
            raise ValueError("flow target %s does not match the generator output %s" % (tuple(flow.shape), (n, 2, h, w)))
        out = torch.empty((n, 2, h, w), dtype=torch.float32, device=mv.device)
        loss = torch.empty((), dtype=torch.float32, device=mv.device)
        saved = _floats(lib.dmc_gen_tiny_saved_bytes(n, h, w), mv.device)
        work = _floats(lib.dmc_gen_tiny_workspace_bytes(), mv.device)
        part = _floats(lib.dmc_gen_tiny_mse_partials_bytes(), mv.device)
        with _span("gen_tiny_fwd"):
            _lib.check(lib.dmc_gen_tiny_fwd_mse(_lib.ptr(mv), _lib.ptr(res), _lib.ptr_array(ws), _lib.ptr_array(bs),
                                                _lib.ptr(flow), _lib.ptr(out), _lib.ptr(saved), _lib.ptr(work),
                                                _lib.ptr(loss), _lib.ptr(part), n, h, w, int(add_mv), _stream()),
                       "dmc_gen_tiny_fwd_mse")
        ctx.save_for_backward(mv, res, saved, out, flow, *ws)
        ctx.bias_like = [(b.shape, b.dtype) for b in bs]
        ctx.set_materialize_grads(False)
        return out, loss

    @staticmethod
    def backward(ctx, grad_out, grad_loss):
        lib = _lib.load()
        mv, res, saved, out, flow = ctx.saved_tensors[:5]
        ws = list(ctx.saved_tensors[5:])
        n, _, h, w = mv.shape
        g = None
        if grad_loss is not None:
            g = torch.empty_like(out)
            with _span("flow_mse_bwd"):
                _lib.check(lib.dmc_flow_mse_bwd(_lib.ptr(out), _lib.ptr(flow), _lib.ptr(grad_loss.contiguous().float()),
                                                _lib.ptr(g), out.numel(), _stream()), "dmc_flow_mse_bwd")
        if grad_out is not None:
            g = grad_out.contiguous() if g is None else g.add_(grad_out)
        if g is None:
            return (None,) * (4 + 12)
        dws = [torch.empty_like(x) for x in ws]
        dbs = [torch.empty(s, dtype=d, device=mv.device) for s, d in ctx.bias_like]
        gbuf = _floats(lib.dmc_gen_tiny_gbuf_bytes(n, h, w), mv.device)
        partials = _floats(lib.dmc_gen_tiny_partials_bytes(n, h, w), mv.device)
        work = _floats(lib.dmc_gen_tiny_workspace_bytes(), mv.device)
        with _span("gen_tiny_bwd"):
            _lib.check(lib.dmc_gen_tiny_bwd(_lib.ptr(mv), _lib.ptr(res), _lib.ptr_array(ws), _lib.ptr(saved),
                                            _lib.ptr(g), _lib.ptr_array(dws), _lib.ptr_array(dbs), _lib.ptr(gbuf),
                                            _lib.ptr(partials), _lib.ptr(work), n, h, w, _stream()),
                       "dmc_gen_tiny_bwd")
        return (None, None, None, None) + tuple(dws) + tuple(dbs)


def gen_tiny_mse(mv, res, flow, weights, biases, add_mv=False):
    """(gen_flow [N,2,H,W], mean((gen_flow - flow)^2)) in one forward launch sequence (see _GenTinyMSE)."""
    return _GenTinyMSE.apply(mv, res, flow, bool(add_mv), *weights, *biases)


#: ``--loss-mse`` name (code/dmcnet/train.py:166-172) -> the C ABI's loss kind
FLOW_LOSS_KINDS = {"MSELoss": 0, "SmoothL1Loss": 1, "L1": 2}


def _loss_kind(kind_name):
    if kind_name not in FLOW_LOSS_KINDS:
        raise ValueError("flow loss must be one of %s, got %r" % (tuple(FLOW_LOSS_KINDS), kind_name))
    return FLOW_LOSS_KINDS[kind_name]


class _GenTinyLoss(torch.autograd.Function):
    """_GenTinyMSE with the criterion chosen: (gen_flow, criterion_mse(gen_flow, flow)) for ``--loss-mse`` MSELoss /
    SmoothL1Loss / L1 (code/dmcnet/train.py:166-172,245), the loss reduced in the epilogue of the kernel that writes
    gen_flow (dmc_gen_tiny_fwd_loss).  Backward = dmc_flow_loss_bwd's gradient (plus whatever else reaches gen_flow)
    through the generator's backward."""

    @staticmethod
    def forward(ctx, kind, mv, res, flow, add_mv, *params):
        lib = _lib.load()
        _need_cuda(mv, res, flow, *params)
        if ctx.needs_input_grad[1] or ctx.needs_input_grad[2] or ctx.needs_input_grad[3]:
            raise NotImplementedError("no gradients w.r.t. the MV / residual / flow inputs")
        mv, res, flow = mv.contiguous(), res.contiguous(), flow.contiguous()
        ws, bs = [p.contiguous() for p in params[:6]], [p.contiguous() for p in params[6:]]
        n, _, h, w = mv.shape
        if tuple(flow.shape) != (n, 2, h, w):
            raise ValueError("flow target %s does not match the generator output %s" % (tuple(flow.shape), (n, 2, h, w)))
        out = torch.empty((n, 2, h, w), dtype=torch.float32, device=mv.device)
        loss = torch.empty((), dtype=torch.float32, device=mv.device)
        saved = _floats(lib.dmc_gen_tiny_saved_bytes(n, h, w), mv.device)
        work = _floats(lib.dmc_gen_tiny_workspace_bytes(), mv.device)
        part = _floats(lib.dmc_gen_tiny_mse_partials_bytes(), mv.device)
        with _span("gen_tiny_fwd"):
            _lib.check(lib.dmc_gen_tiny_fwd_loss(kind, _lib.ptr(mv), _lib.ptr(res), _lib.ptr_array(ws), _lib.ptr_array(bs),
                                                 _lib.ptr(flow), _lib.ptr(out), _lib.ptr(saved), _lib.ptr(work),
                                                 _lib.ptr(loss), _lib.ptr(part), n, h, w, int(add_mv), _stream()),
                       "dmc_gen_tiny_fwd_loss")
        ctx.kind = kind
        ctx.save_for_backward(mv, res, saved, out, flow, *ws)
        ctx.bias_like = [(b.shape, b.dtype) for b in bs]
        ctx.set_materialize_grads(False)
        return out, loss

    @staticmethod
    def backward(ctx, grad_out, grad_loss):
        lib = _lib.load()
        mv, res, saved, out, flow = ctx.saved_tensors[:5]
        ws = list(ctx.saved_tensors[5:])
        n, _, h, w = mv.shape
        g = None
        if grad_loss is not None:
            g = torch.empty_like(out)
            with _span("flow_loss_bwd"):
                _lib.check(lib.dmc_flow_loss_bwd(ctx.kind, _lib.ptr(out), _lib.ptr(flow), None,
                                                 _lib.ptr(grad_loss.contiguous().float()), _lib.ptr(g), None, out.numel(),
                                                 _stream()), "dmc_flow_loss_bwd")
        if grad_out is not None:
            g = grad_out.contiguous() if g is None else g.add_(grad_out)
        if g is None:
            return (None,) * (5 + 12)
        dws = [torch.empty_like(x) for x in ws]
        dbs = [torch.empty(s, dtype=d, device=mv.device) for s, d in ctx.bias_like]
        gbuf = _floats(lib.dmc_gen_tiny_gbuf_bytes(n, h, w), mv.device)
        partials = _floats(lib.dmc_gen_tiny_partials_bytes(n, h, w), mv.device)
        work = _floats(lib.dmc_gen_tiny_workspace_bytes(), mv.device)
        with _span("gen_tiny_bwd"):
            _lib.check(lib.dmc_gen_tiny_bwd(_lib.ptr(mv), _lib.ptr(res), _lib.ptr_array(ws), _lib.ptr(saved),
                                            _lib.ptr(g), _lib.ptr_array(dws), _lib.ptr_array(dbs), _lib.ptr(gbuf),
                                            _lib.ptr(partials), _lib.ptr(work), n, h, w, _stream()),
                       "dmc_gen_tiny_bwd")
        return (None, None, None, None, None) + tuple(dws) + tuple(dbs)


def gen_tiny_loss(kind_name, mv, res, flow, weights, biases, add_mv=False):
    """(gen_flow [N,2,H,W], criterion(gen_flow, flow)) in one forward launch sequence; kind_name: "MSELoss" (what
    gen_tiny_mse gives, bit for bit), "SmoothL1Loss" or "L1" (see _GenTinyLoss)."""
    return _GenTinyLoss.apply(_loss_kind(kind_name), mv, res, flow, bool(add_mv), *weights, *biases)


def gen_tiny(mv, res, weights, biases, add_mv=False):
    """mv [N,2,H,W], res [N,3,H,W], 6 weights + 6 biases (reference layout) -> [N,2,H,W]."""
    return _GenTiny.apply(mv, res, bool(add_mv), torch.is_grad_enabled(), *weights, *biases)


class _FlowMSE(torch.autograd.Function):
    """nn.MSELoss()(gen_flow, input_flow); reference code/dmcnet/train.py:167,245."""

    @staticmethod
    def forward(ctx, gen_flow, flow):
        lib = _lib.load()
        _need_cuda(gen_flow, flow)
        if ctx.needs_input_grad[1]:
            raise NotImplementedError("no gradient w.r.t. the flow target")
        if gen_flow.shape != flow.shape:
            raise ValueError("shape mismatch %s vs %s" % (tuple(gen_flow.shape), tuple(flow.shape)))
        gen_flow, flow = gen_flow.contiguous(), flow.contiguous()
        loss = torch.empty((), dtype=torch.float32, device=gen_flow.device)
        partials = _floats(lib.dmc_flow_mse_partials_bytes(), gen_flow.device)
        with _span("flow_mse_fwd"):
            _lib.check(lib.dmc_flow_mse_fwd(_lib.ptr(gen_flow), _lib.ptr(flow), _lib.ptr(loss),
                                            _lib.ptr(partials), gen_flow.numel(), _stream()),
                       "dmc_flow_mse_fwd")
        ctx.save_for_backward(gen_flow, flow)
        return loss

    @staticmethod
    def backward(ctx, grad_loss):
        lib = _lib.load()
        gen_flow, flow = ctx.saved_tensors
        grad_loss = grad_loss.contiguous().float()
        grad = torch.empty_like(gen_flow)
        with _span("flow_mse_bwd"):
            _lib.check(lib.dmc_flow_mse_bwd(_lib.ptr(gen_flow), _lib.ptr(flow), _lib.ptr(grad_loss),
                                            _lib.ptr(grad), gen_flow.numel(), _stream()),
                       "dmc_flow_mse_bwd")
        return grad, None


def flow_mse(gen_flow, flow):
    return _FlowMSE.apply(gen_flow, flow)


class _FlowLoss(torch.autograd.Function):
    """criterion_mse(gen_flow, input_flow) for nn.MSELoss / nn.SmoothL1Loss / nn.L1Loss (code/dmcnet/train.py:166-172,245)
    and its attention-weighted form criterion_mse(att * gen_flow, att * input_flow) (code/dmcnet/train.py:335,
    code/dmcnet_GAN/train.py:352): one pass forward, one pass backward, the two products never materialised."""

    @staticmethod
    def forward(ctx, kind, gen_flow, flow, att):
        lib = _lib.load()
        _need_cuda(gen_flow, flow, att)
        if ctx.needs_input_grad[2]:
            raise NotImplementedError("no gradient w.r.t. the flow target")
        if gen_flow.shape != flow.shape or (att is not None and att.shape != gen_flow.shape):
            raise ValueError("shape mismatch %s vs %s%s" % (tuple(gen_flow.shape), tuple(flow.shape),
                                                            "" if att is None else " vs att %s" % (tuple(att.shape),)))
        for t in (gen_flow, flow, att):
            if t is not None and t.dtype != torch.float32:
                raise _lib.DmcHipError("expected fp32 tensors, got %s" % t.dtype)
        gen_flow, flow = gen_flow.contiguous(), flow.contiguous()
        att = None if att is None else att.contiguous()
        loss = torch.empty((), dtype=torch.float32, device=gen_flow.device)
        partials = _floats(lib.dmc_flow_loss_partials_bytes(), gen_flow.device)
        with _span("flow_loss_fwd"):
            _lib.check(lib.dmc_flow_loss_fwd(kind, _lib.ptr(gen_flow), _lib.ptr(flow), _lib.ptr(att), _lib.ptr(loss),
                                             _lib.ptr(partials), gen_flow.numel(), _stream()),
                       "dmc_flow_loss_fwd")
        ctx.kind, ctx.has_att = kind, att is not None
        ctx.want_att = att is not None and ctx.needs_input_grad[3]
        ctx.save_for_backward(*((gen_flow, flow) + ((att,) if att is not None else ())))
        return loss

    @staticmethod
    def backward(ctx, grad_loss):
        lib = _lib.load()
        gen_flow, flow = ctx.saved_tensors[:2]
        att = ctx.saved_tensors[2] if ctx.has_att else None
        grad_loss = grad_loss.contiguous().float()
        grad = torch.empty_like(gen_flow)
        grad_att = torch.empty_like(att) if ctx.want_att else None
        with _span("flow_loss_bwd"):
            _lib.check(lib.dmc_flow_loss_bwd(ctx.kind, _lib.ptr(gen_flow), _lib.ptr(flow), _lib.ptr(att), _lib.ptr(grad_loss),
                                             _lib.ptr(grad), _lib.ptr(grad_att), gen_flow.numel(), _stream()),
                       "dmc_flow_loss_bwd")
        return None, grad, None, grad_att


def flow_loss(kind_name, gen_flow, flow, att=None):
    """The reference's reconstruction criterion on the device: kind_name "MSELoss" | "SmoothL1Loss" | "L1"; att (optional,
    the shape of gen_flow) weights both arguments.  Gradients to gen_flow and att, none to flow."""
    return _FlowLoss.apply(_loss_kind(kind_name), gen_flow, flow, att)


class _ConsensusCE(torch.autograd.Function):
    """view(-1,S,C).mean(1) + CrossEntropyLoss; reference code/dmcnet/train.py:239-241."""

    @staticmethod
    def forward(ctx, logits, target, num_segments):
        lib = _lib.load()
        _need_cuda(logits, target)
        if logits.dtype != torch.float32 or target.dtype != torch.int64:
            raise _lib.DmcHipError("consensus_ce expects fp32 logits and int64 class labels, got %s / %s"
                                   % (logits.dtype, target.dtype))
        logits, target = logits.contiguous(), target.contiguous()
        n, c = logits.shape
        if n % num_segments != 0 or target.numel() * num_segments != n:
            raise ValueError("logits %s do not match %d targets x %d segments"
                             % (tuple(logits.shape), target.numel(), num_segments))
        b = n // num_segments
        consensus = torch.empty((b, c), dtype=torch.float32, device=logits.device)
        loss = torch.empty((), dtype=torch.float32, device=logits.device)
        grad = torch.empty_like(logits) if ctx.needs_input_grad[0] else None
        _lib.check(lib.dmc_consensus_ce_fwd_bwd(_lib.ptr(logits), _lib.ptr(target),
                                                _lib.ptr(consensus), _lib.ptr(loss), _lib.ptr(grad),
                                                b, num_segments, c, _stream()),
                   "dmc_consensus_ce_fwd_bwd")
        ctx.save_for_backward(grad)
        ctx.mark_non_differentiable(consensus)
        return loss, consensus

    @staticmethod
    def backward(ctx, grad_loss, _grad_consensus):
        (grad,) = ctx.saved_tensors
        return grad * grad_loss, None, None


def consensus_ce(logits, target, num_segments):
    """Returns (loss, consensus logits [B, C])."""
    return _ConsensusCE.apply(logits, target, num_segments)


class _DiscTail(torch.autograd.Function):
    """LeakyReLU(0.2) -> Dropout2d keep-mask -> BatchNorm2d; reference
    code/dmcnet_GAN/model.py:254-279."""

    @staticmethod
    def forward(ctx, x, keep, gamma, beta, running_mean, running_var, training, eps, momentum):
        lib = _lib.load()
        _need_cuda(x, keep, gamma, beta)
        x = x.contiguous()
        n, c, h, w = x.shape
        use_bn = gamma is not None
        keep = keep.contiguous() if keep is not None else None
        y = torch.empty_like(x)
        stats = _floats(lib.dmc_disc_tail_stats_bytes(c), x.device) if use_bn else None
        _lib.check(lib.dmc_disc_tail_fwd(_lib.ptr(x), _lib.ptr(keep), _lib.ptr(gamma), _lib.ptr(beta),
                                         _lib.ptr(running_mean), _lib.ptr(running_var), _lib.ptr(y),
                                         _lib.ptr(stats), n, c, h, w, int(use_bn), int(training),
                                         float(eps), float(momentum), _stream()),
                   "dmc_disc_tail_fwd")
        ctx.save_for_backward(x, keep, gamma, stats)
        ctx.use_bn = use_bn
        ctx.training = bool(training)
        return y

    @staticmethod
    def backward(ctx, dy):
        lib = _lib.load()
        x, keep, gamma, stats = ctx.saved_tensors
        if ctx.use_bn and not ctx.training:
            raise NotImplementedError("backward through eval-mode BatchNorm is not implemented")
        dy = dy.contiguous()
        n, c, h, w = x.shape
        dx = torch.empty_like(x)
        dgamma = torch.empty_like(gamma) if ctx.use_bn else None
        dbeta = torch.empty_like(gamma) if ctx.use_bn else None
        _lib.check(lib.dmc_disc_tail_bwd(_lib.ptr(x), _lib.ptr(keep), _lib.ptr(gamma), _lib.ptr(stats),
                                         _lib.ptr(dy), _lib.ptr(dx), _lib.ptr(dgamma), _lib.ptr(dbeta),
                                         n, c, h, w, int(ctx.use_bn), _stream()),
                   "dmc_disc_tail_bwd")
        return dx, None, dgamma, dbeta, None, None, None, None, None


def disc_tail(x, keep, bn, training):
    """x: conv output; keep: [N,C] mask/(1-p) or None; bn: nn.BatchNorm2d or None."""
    if bn is None:
        return _DiscTail.apply(x, keep, None, None, None, None, training, 0.0, 0.0)
    if training and bn.num_batches_tracked is not None:
        bn.num_batches_tracked.add_(1)
    return _DiscTail.apply(x, keep, bn.weight, bn.bias, bn.running_mean, bn.running_var, training,
                           bn.eps, bn.momentum)


class _BnAct(torch.autograd.Function):
    """act(BatchNorm2d(x) [+ residual]) on channels_last tensors; reference: the BatchNorm /
    ReLU / residual-add modules of torchvision's ResNet (code/dmcnet/model.py:305,352)."""

    @staticmethod
    def forward(ctx, x, residual, gamma, beta, running_mean, running_var, relu, training, eps,
                momentum):
        lib = _lib.load()
        _need_cuda(x, residual, gamma, beta)
        n, c, h, w = x.shape
        m = n * h * w
        y = torch.empty_like(x)           # keeps the channels_last strides
        stats = _floats(lib.dmc_bn_act_stats_bytes(c), x.device)      # (mean, invstd): kept for backward
        # reduction workspace (16 KB x C): transient -- training forwards only, never saved
        scratch = _floats(lib.dmc_bn_act_scratch_bytes(c), x.device) if training else None
        # with a residual the ReLU sign depends on it: keep 4 sign bits per float4 (1/16 of the
        # residual's size) so that the backward neither re-reads nor even keeps the residual
        mask = None
        if relu and training and residual is not None:
            mask = torch.empty(m * (c // 4), dtype=torch.uint8, device=x.device)
        with _span("bn_act_fwd"):
            _lib.check(lib.dmc_bn_act_fwd(_lib.ptr(x), _lib.ptr(residual), _lib.ptr(gamma),
                                          _lib.ptr(beta), _lib.ptr(running_mean),
                                          _lib.ptr(running_var), _lib.ptr(y), _lib.ptr(stats),
                                          _lib.ptr(scratch), _lib.ptr(mask), m, c, int(relu), int(training), float(eps),
                                          float(momentum), _stream()), "dmc_bn_act_fwd")
        ctx.save_for_backward(x, residual if (relu and mask is None) else None, gamma, beta, stats, mask)
        ctx.relu, ctx.training, ctx.has_res = bool(relu), bool(training), residual is not None
        return y

    @staticmethod
    def backward(ctx, dy):
        lib = _lib.load()
        x, residual, gamma, beta, stats, mask = ctx.saved_tensors
        if not ctx.training:
            raise NotImplementedError("backward through eval-mode BatchNorm is not implemented")
        n, c, h, w = x.shape
        dy = dy.contiguous(memory_format=torch.channels_last)
        dx = torch.empty_like(x)
        want_dres = ctx.has_res and ctx.needs_input_grad[1]
        # without ReLU the residual's gradient is dy itself
        dres = torch.empty_like(x) if (want_dres and ctx.relu) else None
        dgamma, dbeta = torch.empty_like(gamma), torch.empty_like(gamma)
        scratch = _floats(lib.dmc_bn_act_scratch_bytes(c), x.device)
        with _span("bn_act_bwd"):
            _lib.check(lib.dmc_bn_act_bwd(_lib.ptr(x), _lib.ptr(residual), _lib.ptr(gamma),
                                          _lib.ptr(beta), _lib.ptr(stats), _lib.ptr(scratch), _lib.ptr(dy), _lib.ptr(dx),
                                          _lib.ptr(dres), _lib.ptr(dgamma), _lib.ptr(dbeta), _lib.ptr(mask),
                                          n * h * w, c, int(ctx.relu), _stream()), "dmc_bn_act_bwd")
        if want_dres and not ctx.relu:
            dres = dy
        return dx, dres, dgamma, dbeta, None, None, None, None, None, None


def bn_act_supported(x):
    """True if the fused NHWC kernel handles this activation (else use the stock modules)."""
    if not (x.is_cuda and x.dtype == torch.float32 and x.dim() == 4):
        return False
    if not x.is_contiguous(memory_format=torch.channels_last):
        return False
    n, c, h, w = x.shape
    return bool(_lib.load().dmc_bn_act_supported(n * h * w, c))


_PENDING_COUNTERS = None


class batched_bn_counters:
    """Context manager: inside it ``bn_act`` defers ``num_batches_tracked += 1`` and one
    multi-tensor add bumps every counter on exit (20 launches per ResNet-18 forward otherwise)."""

    def __enter__(self):
        global _PENDING_COUNTERS
        self._outer = _PENDING_COUNTERS
        _PENDING_COUNTERS = []
        return self

    def __exit__(self, *exc):
        global _PENDING_COUNTERS
        pending, _PENDING_COUNTERS = _PENDING_COUNTERS, self._outer
        if pending and exc[0] is None:
            torch._foreach_add_(pending, 1)
        return False


def bn_act(x, bn, residual=None, relu=True):
    """relu?(bn(x) [+ residual]) for a channels_last ``x`` and an ``nn.BatchNorm2d`` ``bn``."""
    training = bn.training
    if training and bn.num_batches_tracked is not None:
        if _PENDING_COUNTERS is not None:
            _PENDING_COUNTERS.append(bn.num_batches_tracked)
        else:
            bn.num_batches_tracked.add_(1)
    if residual is not None:
        residual = residual.contiguous(memory_format=torch.channels_last)
    return _BnAct.apply(x, residual, bn.weight, bn.bias, bn.running_mean, bn.running_var, relu,
                        training, bn.eps, bn.momentum if bn.momentum is not None else 0.1)


#: True (default): the stem tail's forward records each pooling window's arg-max (position + raw input value, +120 MB at
#: 120 frames) and the backward's BatchNorm sums stream over that record (dmc_bn_relu_pool_bwd_arg); DMC_POOL_ARGMAX=0:
#: the backward recomputes the arg-max from the input (dmc_bn_relu_pool_bwd)
POOL_ARGMAX = __import__("os").environ.get("DMC_POOL_ARGMAX", "1") != "0"


class _BnReluPool(torch.autograd.Function):
    """maxpool3x3s2p1(relu(bn(x))) of the ResNet stem (torchvision's bn1 / relu / maxpool behind
    code/dmcnet/model.py:305,352) on a channels_last ``x``; the rectified tensor is never stored."""

    @staticmethod
    def forward(ctx, x, gamma, beta, running_mean, running_var, training, eps, momentum, want_slices=False, stat_partials=None):
        lib = _lib.load()
        _need_cuda(x, gamma, beta)
        ctx.set_materialize_grads(False)
        n, c, h, w = x.shape
        ph, pw = (h - 1) // 2 + 1, (w - 1) // 2 + 1
        y = torch.empty((n, c, ph, pw), dtype=x.dtype, device=x.device,
                        memory_format=torch.channels_last)
        stats = _floats(lib.dmc_bn_act_stats_bytes(c), x.device)
        stat_split = 0
        if training and stat_partials is not None and want_slices and c % 16 == 0:
            scratch, stat_split = stat_partials     # reduced by x's producer (dmc_stem_fwd_x3_stats)
        else:
            scratch = _floats(lib.dmc_bn_act_scratch_bytes(c), x.device) if training else None
        ys = codes = xmax = None
        with _span("bn_relu_pool_fwd"):
            if want_slices and c % 16 == 0:     # the pooled map also as a bf16x3 slice tensor (layer1's first convolution)
                ys = torch.empty(lib.dmc_x3s_slices_bytes(n * ph * pw, c), dtype=torch.uint8, device=x.device)
                if training and POOL_ARGMAX and any(ctx.needs_input_grad[:3]):
                    # arg-max record for the backward: its BatchNorm sums then stream over pooled-size tensors
                    codes = _floats(lib.dmc_bn_relu_pool_codes_bytes(n, h, w, c), x.device)
                    xmax = torch.empty_like(y)
                _lib.check(lib.dmc_bn_relu_pool_fwd_arg(_lib.ptr(x), _lib.ptr(gamma), _lib.ptr(beta), _lib.ptr(running_mean),
                                                        _lib.ptr(running_var), _lib.ptr(y), _lib.ptr(ys), _lib.ptr(codes),
                                                        _lib.ptr(xmax), _lib.ptr(stats), _lib.ptr(scratch), int(stat_split), n, h, w, c,
                                                        int(training), float(eps), float(momentum), _stream()),
                           "dmc_bn_relu_pool_fwd_arg")
            else:
                _lib.check(lib.dmc_bn_relu_pool_fwd(_lib.ptr(x), _lib.ptr(gamma), _lib.ptr(beta),
                                                    _lib.ptr(running_mean), _lib.ptr(running_var),
                                                    _lib.ptr(y), _lib.ptr(stats), _lib.ptr(scratch), n, h, w, c, int(training),
                                                    float(eps), float(momentum), _stream()),
                           "dmc_bn_relu_pool_fwd")
        if codes is not None:
            ctx.save_for_backward(x, gamma, beta, stats, codes, xmax)
        else:
            ctx.save_for_backward(x, gamma, beta, stats)
        ctx.training = bool(training)
        if ys is None:
            ys = torch.empty(0, dtype=torch.uint8, device=x.device)
        ctx.mark_non_differentiable(ys)
        return y, ys

    @staticmethod
    def backward(ctx, dy, _dys):
        lib = _lib.load()
        x, gamma, beta, stats = ctx.saved_tensors[:4]
        if dy is None:
            return (None,) * 10
        if not ctx.training:
            raise NotImplementedError("backward through eval-mode BatchNorm is not implemented")
        n, c, h, w = x.shape
        dy = dy.contiguous(memory_format=torch.channels_last)
        dx = torch.empty_like(x)
        dgamma, dbeta = torch.empty_like(gamma), torch.empty_like(gamma)
        scratch = _floats(lib.dmc_bn_act_scratch_bytes(c), x.device)
        with _span("bn_relu_pool_bwd"):
            if len(ctx.saved_tensors) == 6:
                codes, xmax = ctx.saved_tensors[4:]
                _lib.check(lib.dmc_bn_relu_pool_bwd_arg(_lib.ptr(x), _lib.ptr(gamma), _lib.ptr(beta), _lib.ptr(stats),
                                                        _lib.ptr(scratch), _lib.ptr(dy), _lib.ptr(codes), _lib.ptr(xmax),
                                                        _lib.ptr(dx), _lib.ptr(dgamma), _lib.ptr(dbeta), n, h, w, c, _stream()),
                           "dmc_bn_relu_pool_bwd_arg")
            else:
                codes = _floats(lib.dmc_bn_relu_pool_codes_bytes(n, h, w, c), x.device)
                _lib.check(lib.dmc_bn_relu_pool_bwd(_lib.ptr(x), _lib.ptr(gamma), _lib.ptr(beta),
                                                    _lib.ptr(stats), _lib.ptr(scratch), _lib.ptr(dy), _lib.ptr(dx),
                                                    _lib.ptr(dgamma), _lib.ptr(dbeta), _lib.ptr(codes),
                                                    n, h, w, c, _stream()), "dmc_bn_relu_pool_bwd")
        return dx, dgamma, dbeta, None, None, None, None, None, None, None


def bn_relu_pool_supported(x):
    """True if the fused stem kernel handles this activation (channels_last fp32 on the GPU)."""
    if not (x.is_cuda and x.dtype == torch.float32 and x.dim() == 4):
        return False
    if not x.is_contiguous(memory_format=torch.channels_last):
        return False
    n, c, h, w = x.shape
    return bool(_lib.load().dmc_bn_relu_pool_supported(n, h, w, c))


def bn_relu_pool(x, bn, want_slices=False):
    """maxpool(3, 2, 1)(relu(bn(x))) for a channels_last ``x`` and an ``nn.BatchNorm2d`` ``bn``; ``want_slices``: the
    pooled map's bf16x3 slice tensor is attached to the result (x3s_of) for a pre-split convolution."""
    training = bn.training
    if training and bn.num_batches_tracked is not None:
        if _PENDING_COUNTERS is not None:
            _PENDING_COUNTERS.append(bn.num_batches_tracked)
        else:
            bn.num_batches_tracked.add_(1)
    y, ys = _BnReluPool.apply(x, bn.weight, bn.bias, bn.running_mean, bn.running_var, training, bn.eps,
                              bn.momentum if bn.momentum is not None else 0.1, bool(want_slices),
                              getattr(x, "_dmc_stat_partials", None))
    if ys.numel():
        y._dmc_x3s = ys
        y._dmc_f32 = True
    return y


#: True (default): conv1's forward on dmc_stem_fwd (exact fp32 MFMA, no LDS); False = F.conv2d (MIOpen)
STEM_FWD_HIP = __import__("os").environ.get("DMC_STEM_FWD", "1") != "0"


#: True (default): conv1's data gradient (GAN variant) on dmc_stem_dgrad; DMC_STEM_DGRAD=0: library GEMM + col2im
STEM_DGRAD_HIP = __import__("os").environ.get("DMC_STEM_DGRAD", "1") != "0"


class _StemConv(torch.autograd.Function):
    """conv1 of the classifier for the 2-channel flow input (code/dmcnet/model.py:285-294): the
    forward convolution is dmc_stem_fwd (fp32 MFMA with the weights resident in registers); with 2 input
    channels MIOpen's implicit-GEMM *gradients* degenerate (weight gradient 0.80 ms, data gradient 2.1 ms at
    120 frames), so
      * the weight gradient is dmc_stem_wgrad (0.24 ms, deterministic);
      * the data gradient (needed only by the GAN variant, whose classifier loss reaches the
        generator) is dmc_stem_dgrad (one wave per input row: a [OW x 14] row GEMM over the 3-4 window rows that
        reach it, in bf16x3 arithmetic, and a 1-D fold); frames wider than 256 fall back to a batched GEMM
        W^T[98,64] x dy[64, OH*OW] followed by ``fold`` (col2im)."""

    @staticmethod
    def forward(ctx, x, weight, want_stats=False):
        xc = x.detach().contiguous()
        stat = None
        if STEM_FWD_HIP:
            n, _, h, w = xc.shape
            y = torch.empty((n, 64, (h + 1) // 2, (w + 1) // 2), dtype=torch.float32, device=x.device,
                            memory_format=torch.channels_last)
            so, si, sy, sx = weight.stride()
            lib = _lib.load()
            with _span("stem_fwd"):
                if lib.dmc_get_option(b"conv_arith") == 1:         # bf16x3 arithmetic, as the other classifier convolutions
                    work = _floats(lib.dmc_stem_fwd_x3_workspace_bytes(n, h, w), x.device)
                    if want_stats:      # bn1's batch statistics from the accumulators: partial sums for the stem tail
                        stat = _floats(lib.dmc_bn_act_scratch_bytes(64), x.device)
                    _lib.check(lib.dmc_stem_fwd_x3_stats(_lib.ptr(xc), _lib.ptr(weight), so, si, sy, sx, _lib.ptr(work), _lib.ptr(y),
                                                         _lib.ptr(stat), n, h, w, _stream()), "dmc_stem_fwd_x3_stats")
                else:
                    _lib.check(lib.dmc_stem_fwd(_lib.ptr(xc), _lib.ptr(weight), so, si, sy, sx, _lib.ptr(y), n, h, w,
                                                _stream()), "dmc_stem_fwd")
        else:
            y = torch.nn.functional.conv2d(x, weight, None, 2, 3)
        ctx.save_for_backward(xc, weight)
        if stat is None:
            stat = torch.empty(0, dtype=torch.float32, device=x.device)
        ctx.mark_non_differentiable(stat)
        return y, stat

    @staticmethod
    def backward(ctx, dy, _dstat=None):
        lib = _lib.load()
        x, weight = ctx.saved_tensors
        n, _, h, w = x.shape
        dy = dy.contiguous(memory_format=torch.channels_last)
        dw = dx = None
        if ctx.needs_input_grad[1]:
            def launch():
                dw = torch.empty((64, 2, 7, 7), dtype=torch.float32, device=x.device)
                partials = _floats(lib.dmc_stem_wgrad_partials_bytes(n, h, w), x.device)
                _lib.check(lib.dmc_stem_wgrad(_lib.ptr(x), _lib.ptr(dy), _lib.ptr(dw), _lib.ptr(partials),
                                              n, h, w, _stream()), "dmc_stem_wgrad")
                if weight.is_contiguous(memory_format=torch.channels_last) and not weight.is_contiguous():
                    dw = dw.contiguous(memory_format=torch.channels_last)
                return dw
            with _span("stem_wgrad"):
                dw = _on_wgrad_stream(weight, (x, dy), launch)
        if ctx.needs_input_grad[0]:
            if STEM_DGRAD_HIP and dy.dtype == torch.float32 and lib.dmc_stem_dgrad_supported(h, w):
                # row GEMM + 1-D fold in one kernel, bf16x3 arithmetic (dmc_stem_dgrad): no [pixels][98] column matrix
                dx = torch.empty((n, 2, h, w), dtype=torch.float32, device=x.device)
                work = _floats(lib.dmc_stem_dgrad_workspace_bytes(), x.device)
                so, si, sy, sx = weight.stride()
                with _span("stem_dgrad"):
                    _lib.check(lib.dmc_stem_dgrad(_lib.ptr(dy), _lib.ptr(weight), so, si, sy, sx, _lib.ptr(work), _lib.ptr(dx),
                                                  n, h, w, _stream()), "dmc_stem_dgrad")
            else:
                oh, ow = dy.shape[2], dy.shape[3]
                g = dy.permute(0, 2, 3, 1).reshape(n, oh * ow, 64)            # a view of the NHWC storage
                cols = torch.matmul(weight.reshape(64, 98).t(), g.transpose(1, 2))   # [N, 98, OH*OW]
                dx = torch.nn.functional.fold(cols, (h, w), kernel_size=7, padding=3, stride=2)
        return dx, dw, None


def stem_conv_supported(x, weight):
    """True when ``conv2d(x, weight, stride 2, padding 3)`` can take the HIP weight gradient."""
    return (x.is_cuda and x.dim() == 4 and x.dtype == torch.float32
            and tuple(weight.shape) == (64, 2, 7, 7) and weight.dtype == torch.float32
            and x.shape[1] == 2
            and bool(_lib.load().dmc_stem_wgrad_supported(int(x.shape[2]), int(x.shape[3]))))


#: True (default): conv1's forward also reduces bn1's batch statistics from its accumulators (dmc_stem_fwd_x3_stats)
STEM_STATS = __import__("os").environ.get("DMC_STEM_STATS", "1") != "0"


def stem_conv(x, weight, want_stats=False):
    """conv1(x) for ``x`` [N,2,H,W] and ``weight`` [64,2,7,7].  ``want_stats``: the batch statistics' partial sums of the
    result are attached to it for ``bn_relu_pool`` (training mode: the BatchNorm pass over the convolution output goes)."""
    _need_cuda(x, weight)
    y, stat = _StemConv.apply(x, weight, bool(want_stats) and STEM_STATS)
    if stat.numel():
        lib = _lib.load()
        y._dmc_stat_partials = (stat, lib.dmc_stem_fwd_x3_stat_blocks(int(x.shape[0]), int(x.shape[2]), int(x.shape[3])))
    return y


# ------------------------------------------------------------------ NHWC convolutions (conv_nhwc.hip)
_CL = torch.channels_last


def _is_cl(t):
    return t.dim() == 4 and t.is_contiguous(memory_format=_CL)


def conv_nhwc_supported(x, weight, stride, padding):
    """True if ``conv2d(x, weight, stride=stride, padding=padding)`` can run on the HIP implicit-GEMM
    kernels (fp32, channels_last x, 3x3/pad 1 or 1x1/pad 0, stride 1 or 2, channels multiples of 16)."""
    if not (x.is_cuda and x.dtype == torch.float32 and x.dim() == 4 and weight.dtype == torch.float32):
        return False
    n, cin, h, w = x.shape
    cout, cin2, kh, kw = weight.shape
    if cin2 != cin:
        return False
    return bool(_lib.load().dmc_conv_nhwc_supported(n, h, w, cin, cout, kh, kw, int(stride), int(padding)))


def _conv_geom(x, weight, stride, padding):
    n, cin, h, w = x.shape
    cout, _, kh, kw = weight.shape
    oh, ow = (h + 2 * padding - kh) // stride + 1, (w + 2 * padding - kw) // stride + 1
    return n, h, w, cin, cout, kh, kw, oh, ow


def _conv_fwd(x, weight, bias, keep, stride, padding, act, want_stats, presplit=None):
    lib = _lib.load()
    n, h, w, cin, cout, kh, kw, oh, ow = _conv_geom(x, weight, stride, padding)
    y = torch.empty((n, cout, oh, ow), dtype=torch.float32, device=x.device, memory_format=_CL)
    part, nblk = None, 0
    if want_stats:
        nblk = lib.dmc_conv_nhwc_stat_blocks(n, h, w, cin, cout, kh, stride, padding)
        part = torch.empty((nblk, cout, 2), dtype=torch.float64, device=x.device)
    wpack = presplit if presplit is not None else _floats(lib.dmc_conv_nhwc_wt_bytes(cin, cout, kh, kw), x.device)
    wptr = None if presplit is not None else _lib.ptr(weight)      # NULL: wpack already holds the slices
    _lib.check(lib.dmc_conv_nhwc_fwd(_lib.ptr(x), wptr, _lib.ptr(wpack), _lib.ptr(bias), _lib.ptr(keep), _lib.ptr(y),
                                     _lib.ptr(part), nblk, n, h, w, cin, cout, kh, kw, stride, padding, int(act),
                                     _stream()), "dmc_conv_nhwc_fwd")
    return y, part, nblk


def _conv_dgrad(dy, weight, x_shape, stride, padding, presplit=None, addend=None):
    lib = _lib.load()
    n, cin, h, w = x_shape
    cout, _, kh, kw = weight.shape
    dx = torch.empty((n, cin, h, w), dtype=torch.float32, device=dy.device, memory_format=_CL)
    wt = presplit if presplit is not None else _floats(lib.dmc_conv_nhwc_wt_bytes(cin, cout, kh, kw), dy.device)
    wptr = None if presplit is not None else _lib.ptr(weight)      # NULL: wt already holds the transposed slices
    if addend is not None:                      # dx = data gradient + addend, in the convolution's epilogue
        addend = _as_cl(addend)
        _lib.check(lib.dmc_conv_nhwc_dgrad_add(_lib.ptr(dy), wptr, _lib.ptr(wt), _lib.ptr(addend), _lib.ptr(dx), n, h, w,
                                               cin, cout, kh, kw, stride, padding, _stream()), "dmc_conv_nhwc_dgrad_add")
        return dx
    _lib.check(lib.dmc_conv_nhwc_dgrad(_lib.ptr(dy), wptr, _lib.ptr(wt), _lib.ptr(dx), n, h, w, cin,
                                       cout, kh, kw, stride, padding, _stream()), "dmc_conv_nhwc_dgrad")
    return dx


def _conv_wgrad(x, dy, weight, stride, padding):
    lib = _lib.load()
    n, cin, h, w = x.shape
    cout, _, kh, kw = weight.shape
    dw = torch.empty((cout, cin, kh, kw), dtype=torch.float32, device=x.device, memory_format=_CL)
    work = _floats(lib.dmc_conv_nhwc_wgrad_bytes(n, h, w, cin, cout, kh, kw, stride, padding), x.device)
    _lib.check(lib.dmc_conv_nhwc_wgrad(_lib.ptr(x), _lib.ptr(dy), _lib.ptr(dw), _lib.ptr(work), n, h, w, cin, cout,
                                       kh, kw, stride, padding, _stream()), "dmc_conv_nhwc_wgrad")
    return dw


def _as_cl(t):
    return t if _is_cl(t) else t.contiguous(memory_format=_CL)


def _grad_like(dw, weight):
    """dw (channels_last memory) in the strides of ``weight`` (no copy when weight is channels_last)."""
    return dw if _is_cl(weight) and weight.stride() == dw.stride() else dw.contiguous().view_as(weight).contiguous()


class _ConvNHWC(torch.autograd.Function):
    """nn.Conv2d(bias=False) on the fp32 matrix cores: the ResNet's 3x3 / 1x1 convolutions
    (torchvision BasicBlock behind code/dmcnet/model.py:305,352)."""

    @staticmethod
    def forward(ctx, x, weight, stride, padding):
        _need_cuda(x, weight)
        x, wcl = _as_cl(x), _as_cl(weight)
        with _span("conv_nhwc_fwd"):
            y, _, _ = _conv_fwd(x, wcl, None, None, stride, padding, 0, False)
        ctx.save_for_backward(x, weight)
        ctx.geom = (stride, padding)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, weight = ctx.saved_tensors
        stride, padding = ctx.geom
        dy, wcl = _as_cl(dy), _as_cl(weight)
        dx = dw = None
        if ctx.needs_input_grad[0]:
            with _span("conv_nhwc_dgrad"):
                dx = _conv_dgrad(dy, wcl, x.shape, stride, padding)
        if ctx.needs_input_grad[1]:
            with _span("conv_nhwc_wgrad"):
                dw = _grad_like(_conv_wgrad(x, dy, wcl, stride, padding), weight)
        return dx, dw, None, None


def conv_nhwc(x, weight, stride=1, padding=1):
    """conv2d(x, weight, None, stride, padding) for a channels_last ``x`` (see conv_nhwc_supported)."""
    return _ConvNHWC.apply(x, weight, int(stride), int(padding))



# ------------------------------------------------------------------ pre-split bf16x3 operands (conv_x3s.hip)
#: True (default): stride-1 3x3 convolutions of the fused conv -> bn op run on conv_x3s.hip -- both operands arrive as
#: bf16x3 slice tensors written by the PRODUCER of the activation (BatchNorm apply / stem pool / BatchNorm backward), the
#: convolution's main loop is LDS reads + MFMAs only.  DMC_X3S=0: the in-loop-split kernels of conv_nhwc.hip.
X3S = __import__("os").environ.get("DMC_X3S", "1") != "0"
#: DMC_BN_BWD_LINK=1: a pre-split data gradient also reduces the BatchNorm-backward sums of the unit it feeds (BnBwdLink).
#: Off by default: measured neutral (13.28 vs 13.27 ms per step, two A/B pairs on one box) -- the 0.33 ms of bn_partial
#: launches it removes come back as un-overlapped epilogue time of the data-gradient kernels.
BN_BWD_LINK = __import__("os").environ.get("DMC_BN_BWD_LINK", "0") == "1"


def x3s_of(t):
    """The slice tensor attached to activation ``t`` by its producer (or None)."""
    return getattr(t, "_dmc_x3s", None)


def f32_valid(t):
    """False when ``t``'s fp32 memory was not written (its producer emitted slices only)."""
    return getattr(t, "_dmc_f32", True)


def _attach_x3s(t, xs, has_f32=True):
    t._dmc_x3s = xs
    t._dmc_f32 = has_f32
    return t


def _x3s_buffer(m, c, device):
    return torch.empty(_lib.load().dmc_x3s_slices_bytes(m, c), dtype=torch.uint8, device=device)


def x3s_split(x):
    """Slice tensor of a channels_last fp32 activation (the stand-alone producer: tests, inputs nobody split)."""
    n, c, h, w = x.shape
    xs = _x3s_buffer(n * h * w, c, x.device)
    _lib.check(_lib.load().dmc_x3s_split(_lib.ptr(x), _lib.ptr(xs), n * h * w, c, _stream()), "dmc_x3s_split")
    return xs


def x3s_merge(xs, shape):
    """fp32 channels_last tensor of ``shape`` from its slice tensor (exact: the three slices sum to the value)."""
    n, c, h, w = shape
    x = torch.empty(shape, dtype=torch.float32, device=xs.device, memory_format=torch.channels_last)
    _lib.check(_lib.load().dmc_x3s_merge(_lib.ptr(xs), _lib.ptr(x), n * h * w, c, _stream()), "dmc_x3s_merge")
    return x


def x3s_pack_weights(weight, forward=True, transposed=True):
    """(wpack_f, wpack_t) of a channels_last [Cout, Cin, 3, 3] weight for dmc_x3s_conv_fwd / dmc_x3s_conv_dgrad."""
    lib = _lib.load()
    cout, cin = weight.shape[0], weight.shape[1]
    nb = lib.dmc_x3s_wpack_bytes(cin, cout)
    wf = torch.empty(nb, dtype=torch.uint8, device=weight.device) if forward else None
    wt = torch.empty(nb, dtype=torch.uint8, device=weight.device) if transposed else None
    _lib.check(lib.dmc_x3s_pack_weights(_lib.ptr(_as_cl(weight)), _lib.ptr(wf), _lib.ptr(wt), cin, cout, _stream()),
               "dmc_x3s_pack_weights")
    return wf, wt


def x3s_conv_fwd(xs, wpack_f, n, h, w, cin, cout, want_stats=False):
    """conv3x3 (stride 1, padding 1) of the activation whose slice tensor is ``xs`` -> (y fp32 channels_last, statistics
    partials [blocks, Cout, 2] float64 or None)."""
    lib = _lib.load()
    y = torch.empty((n, cout, h, w), dtype=torch.float32, device=xs.device, memory_format=torch.channels_last)
    part, nblk = None, 0
    if want_stats:
        nblk = lib.dmc_x3s_conv_stat_blocks(n, h, w, cout)
        part = torch.empty((nblk, cout, 2), dtype=torch.float64, device=xs.device)
    _lib.check(lib.dmc_x3s_conv_fwd(_lib.ptr(xs), _lib.ptr(wpack_f), _lib.ptr(y), _lib.ptr(part), nblk, n, h, w, cin, cout, _stream()),
               "dmc_x3s_conv_fwd")
    return y, part


def x3s_conv_dgrad(dys, wpack_t, n, h, w, cin, cout, addend=None):
    dx = torch.empty((n, cin, h, w), dtype=torch.float32, device=dys.device, memory_format=torch.channels_last)
    _lib.check(_lib.load().dmc_x3s_conv_dgrad(_lib.ptr(dys), _lib.ptr(wpack_t), _lib.ptr(addend), _lib.ptr(dx), n, h, w, cin, cout,
                                              _stream()), "dmc_x3s_conv_dgrad")
    return dx


def x3s_conv_wgrad(xs, dys, n, h, w, cin, cout):
    lib = _lib.load()
    dw = torch.empty((cout, cin, 3, 3), dtype=torch.float32, device=xs.device, memory_format=torch.channels_last)
    work = _floats(lib.dmc_x3s_conv_wgrad_bytes(n, h, w, cin, cout), xs.device)
    _lib.check(lib.dmc_x3s_conv_wgrad(_lib.ptr(xs), _lib.ptr(dys), _lib.ptr(dw), _lib.ptr(work), n, h, w, cin, cout, _stream()),
               "dmc_x3s_conv_wgrad")
    return dw


def x3s_usable(n, h, w, conv):
    """True if ``conv`` on an [n, Cin, h, w] activation takes the pre-split path (3x3, stride 1, padding 1, no bias)."""
    if not X3S or conv.kernel_size != (3, 3) or conv.stride != (1, 1) or conv.padding != (1, 1) or conv.bias is not None:
        return False
    if conv.dilation != (1, 1) or conv.groups != 1:
        return False
    lib = _lib.load()
    if lib.dmc_get_option(b"conv_arith") != 1 or lib.dmc_get_option(b"conv_path") != 1:
        return False
    cin, cout = conv.in_channels, conv.out_channels
    return bool(lib.dmc_x3s_conv_supported(n, h, w, cin, cout)) and bool(lib.dmc_x3s_conv_wgrad_supported(n, h, w, cin, cout))


# ------------------------------------------------------------------ stride-2 block pair on s2d slice tensors (conv_x3q.hip)
def x3q_split(x):
    """Space-to-depth slice tensor of a channels_last fp32 activation with even H, W (stand-alone producer: tests)."""
    n, c, h, w = x.shape
    xq = _x3s_buffer(n * h * w, c, x.device)
    _lib.check(_lib.load().dmc_x3q_split(_lib.ptr(x), _lib.ptr(xq), n, h, w, c, _stream()), "dmc_x3q_split")
    return xq


def x3q_merge(xq, shape):
    n, c, h, w = shape
    x = torch.empty(shape, dtype=torch.float32, device=xq.device, memory_format=torch.channels_last)
    _lib.check(_lib.load().dmc_x3q_merge(_lib.ptr(xq), _lib.ptr(x), n, h, w, c, _stream()), "dmc_x3q_merge")
    return x


def x3q_pack_weights(w3, w1, forward=True, transposed=True):
    """(wpack_f, wpack_t) of the channels_last [Cout, Cin, 3, 3] / [Cout, Cin, 1, 1] weight pair of a stride-2 block."""
    lib = _lib.load()
    cout, cin = w3.shape[0], w3.shape[1]
    nb = lib.dmc_x3q_wpack_bytes(cin, cout)
    wf = torch.empty(nb, dtype=torch.uint8, device=w3.device) if forward else None
    wt = torch.empty(nb, dtype=torch.uint8, device=w3.device) if transposed else None
    _lib.check(lib.dmc_x3q_pack_weights(_lib.ptr(_as_cl(w3)), _lib.ptr(_as_cl(w1)), _lib.ptr(wf), _lib.ptr(wt), cin, cout, _stream()),
               "dmc_x3q_pack_weights")
    return wf, wt


def x3q_conv_fwd(xq, wpack_f, n, oh, ow, cin, cout, want_stats=False):
    """(y3, y1, partials3, partials1): the 3x3 / stride-2 convolution and the 1x1 / stride-2 shortcut of the activation whose
    s2d slice tensor is ``xq``, both [n, cout, oh, ow] channels_last fp32, from ONE launch."""
    lib = _lib.load()
    y3 = torch.empty((n, cout, oh, ow), dtype=torch.float32, device=xq.device, memory_format=torch.channels_last)
    y1 = torch.empty_like(y3)
    p3 = p1 = None
    nblk = 0
    if want_stats:
        nblk = lib.dmc_x3q_stat_blocks(n, oh, ow, cout)
        p3 = torch.empty((nblk, cout, 2), dtype=torch.float64, device=xq.device)
        p1 = torch.empty_like(p3)
    _lib.check(lib.dmc_x3q_conv_fwd(_lib.ptr(xq), _lib.ptr(wpack_f), _lib.ptr(y3), _lib.ptr(y1), _lib.ptr(p3), _lib.ptr(p1), nblk,
                                    n, oh, ow, cin, cout, _stream()), "dmc_x3q_conv_fwd")
    return y3, y1, p3, p1


def x3q_conv_dgrad(dys3, dys1, wpack_t, n, oh, ow, cin, cout):
    """dx [n, cin, 2 oh, 2 ow] of the pair from the slice tensors of the two output gradients."""
    dx = torch.empty((n, cin, 2 * oh, 2 * ow), dtype=torch.float32, device=dys3.device, memory_format=torch.channels_last)
    _lib.check(_lib.load().dmc_x3q_conv_dgrad(_lib.ptr(dys3), _lib.ptr(dys1), _lib.ptr(wpack_t), _lib.ptr(dx), n, oh, ow, cin, cout,
                                              _stream()), "dmc_x3q_conv_dgrad")
    return dx


def x3q_conv_wgrad(xq, dys3, dys1, n, oh, ow, cin, cout):
    """(dw3 [cout, cin, 3, 3], dw1 [cout, cin, 1, 1]), channels_last memory, of the stride-2 pair."""
    lib = _lib.load()
    dw3 = torch.empty((cout, cin, 3, 3), dtype=torch.float32, device=xq.device, memory_format=torch.channels_last)
    dw1 = torch.empty((cout, cin, 1, 1), dtype=torch.float32, device=xq.device, memory_format=torch.channels_last)
    work = _floats(lib.dmc_x3q_conv_wgrad_bytes(n, oh, ow, cin, cout), xq.device)
    _lib.check(lib.dmc_x3q_conv_wgrad(_lib.ptr(xq), _lib.ptr(dys3), _lib.ptr(dys1), _lib.ptr(dw3), _lib.ptr(dw1), _lib.ptr(work),
                                      n, oh, ow, cin, cout, _stream()), "dmc_x3q_conv_wgrad")
    return dw3, dw1


class ResidualGradLink:
    """Couples the two fused ops of an identity-shortcut residual block (torchvision BasicBlock: `out += identity`, behind
    code/dmcnet/model.py:305): the block input feeds the first convolution AND the residual add, so autograd would sum the
    two gradients in a separate elementwise pass over the block input (96 MB per tensor in layer1 at 120 frames).  With a link
    the block's LAST op (the one given ``residual``) parks its residual gradient here instead of returning it, and the
    block's FIRST op (which autograd always runs later: its output feeds the last op) adds it in the epilogue of its data-
    gradient launch.  The sum is the same two fp32 addends; only the pass is saved."""
    __slots__ = ("armed", "grad")

    def __init__(self):
        self.armed = False
        self.grad = None


#: True (default): the classifier's weight gradients run on a side HIP stream.  Nothing reads a weight gradient before the
#: optimizer / the gradient exchange, while everything else in the backward pass is one dependent chain; on its own stream
#: a (matrix-bound) weight-gradient launch overlaps the (memory-bound) BatchNorm passes of the layers below it: 12.43 ->
#: 12.25 ms per step.  The main stream re-joins when backward() returns (an autograd-engine callback), in the gradient
#: exchange before a bucket is read, and in join_wgrad_stream().  DMC_WGRAD_STREAM=0: one stream.
#: Used where a backward pass is wrapped in ``with ops.wgrad_side_stream():`` -- DmcnetTrainStep does (config 2: -0.32 ms);
#: the GAN step does not (measured 0.1 ms slower there: its D step is closer to launch-bound and gains nothing back).
WGRAD_STREAM = __import__("os").environ.get("DMC_WGRAD_STREAM", "1") != "0"
_WGRAD_STREAMS = {}
_WGRAD_PENDING = [False]
_WGRAD_SCOPE = [0]
_WGRAD_COUNT = [0]            # launches that went to the side stream (diagnostics / tests)
_WGRAD_SEEN = set()           # id() of EVERY weight whose gradient went to the side stream in this backward pass (cleared per pass, not per join)
_WGRAD_MAIN = set()           # id() of the weights forced to the main stream for the REST of this backward pass (seen twice)


class wgrad_side_stream(object):
    """Context manager around ``loss.backward()``: weight gradients of the classifier convolutions inside it may run on
    the side stream (see WGRAD_STREAM).  A plain global counter: backward functions run on the autograd engine's thread."""

    def __enter__(self):
        _WGRAD_SCOPE[0] += 1
        _WGRAD_SEEN.clear()
        _WGRAD_MAIN.clear()
        return self

    def __exit__(self, *exc):
        _WGRAD_SCOPE[0] -= 1
        join_wgrad_stream()
        _WGRAD_SEEN.clear()
        _WGRAD_MAIN.clear()
        return False


def _wgrad_stream(device):
    key = torch.device(device).index
    if key not in _WGRAD_STREAMS:
        _WGRAD_STREAMS[key] = torch.cuda.Stream(device=device)
    return _WGRAD_STREAMS[key]


def join_wgrad_stream():
    """The current stream waits for the weight gradients launched on the side stream (no-op when none are pending).
    _WGRAD_SEEN survives: a mid-pass join (a shared weight's second use, a gradient bucket being read) completes the gradients
    in flight but a weight B that produced one before it may still be used AGAIN later in the pass -- its second gradient
    must then be produced on the main stream, where the engine sums the two."""
    if _WGRAD_PENDING[0]:
        cur = torch.cuda.current_stream()
        for st in _WGRAD_STREAMS.values():
            cur.wait_stream(st)
        _WGRAD_PENDING[0] = False


def _wgrad_side_ok(weight):
    """True if ``weight``'s gradient may be produced on the side stream (see _on_wgrad_stream)."""
    if weight.grad is not None:                 # ``weight.grad += dw`` would run on the main stream at once
        return False
    # a weight used TWICE in one backward pass (a shared convolution, a module called twice): the engine sums the two
    # gradients on the main stream -- in its input buffer or in AccumulateGrad -- believing the main stream produced the
    # first one.  The second sighting therefore re-joins (the first gradient is complete on the main stream) and stays there.
    # _WGRAD_SEEN is per PASS (cleared by the scope, not by a join): with two shared weights A and B used alternately, A's
    # second use joins mid-pass; B's second use afterwards must still be recognised.  Any further use (a module called three
    # times, a discriminator applied to real, fake and an interpolate) stays on the main stream too -- its gradient is
    # summed into the same buffer.
    if id(weight) in _WGRAD_MAIN:
        return False
    if id(weight) in _WGRAD_SEEN:
        join_wgrad_stream()                     # no-op when an earlier join already completed the first gradient
        _WGRAD_MAIN.add(id(weight))
        return False
    # C++-level gradient hooks (torch's DistributedDataParallel reducer) read the gradient on the main stream the moment it
    # is accumulated and are not visible from Python: with a process group up, only parameters that carry THIS package's
    # deferring hook (ddp.GradBucketReducer) may use the side stream
    post = getattr(weight, "_post_accumulate_grad_hooks", None)
    if torch.distributed.is_available() and torch.distributed.is_initialized():
        if not post or not all(getattr(h, "_dmc_defers_read", False) for h in post.values()):
            return False
    # a hook that reads the gradient the moment it is accumulated would read it on the main stream, before the side stream
    # has written it: only hooks that declare they defer the read (the gradient exchange's, ddp.py) are compatible
    if getattr(weight, "_backward_hooks", None):
        return False
    if post and not all(getattr(h, "_dmc_defers_read", False) for h in post.values()):
        return False
    return True


def _on_wgrad_stream(weight, reads, launch):
    """``launch()`` (allocates, launches, returns the weight gradient -- a tuple of them when ``weight`` is a tuple of
    parameters served by one call) on the side stream when that is safe: inside an autograd backward pass (the join is
    queued as an engine callback: it runs on the caller's stream before backward() returns) and with no gradient to
    accumulate into."""
    weights = weight if isinstance(weight, tuple) else (weight,)
    if not WGRAD_STREAM or _WGRAD_SCOPE[0] <= 0 or not all(_wgrad_side_ok(w) for w in weights):
        return launch()
    if PROBE is not None and (PROBE.only is None or "conv_nhwc_wgrad" in PROBE.only or "stem_wgrad" in PROBE.only):
        return launch()                         # HIP-event spans around this call time the launch stream: stay on it
    if not _WGRAD_PENDING[0]:
        try:
            torch.autograd.Variable._execution_engine.queue_callback(join_wgrad_stream)
        except RuntimeError:                    # not inside a backward pass (a direct call): stay on this stream
            return launch()
    main, side = torch.cuda.current_stream(), _wgrad_stream(weights[0].device)
    side.wait_stream(main)                      # the operands were written on the main stream
    for t in reads:
        t.record_stream(side)                   # their memory is not reused before the side stream has read it
    _WGRAD_PENDING[0] = True
    _WGRAD_COUNT[0] += 1
    for w in weights:
        _WGRAD_SEEN.add(id(w))
    with torch.cuda.stream(side):
        dw = launch()
    for t in (dw if isinstance(dw, tuple) else (dw,)):
        t.record_stream(main)
    return dw


class BnBwdLink:
    """Couples a fused conv -> bn op U with the ONE pre-split convolution V that reads its result: V's data-gradient launch
    writes U's output gradient, so it also reduces U's BatchNorm-backward sums (dbeta, dgamma) from the tile it holds in LDS
    (dmc_x3s_conv_dgrad_bnb) and U's backward skips its reduction pass (bn_partial: a read of dout and y).  ``kind``:
    "inner" = U's result feeds V alone (conv1 -> conv2 of a block); "block" = U closes a block whose output feeds an
    identity-shortcut block -- V's launch is then U's complete output gradient only when it also adds the residual branch's
    gradient (ResidualGradLink), which V checks at backward time.  Unused links cost nothing: U falls back to its own pass."""
    __slots__ = ("kind", "y", "stats", "gamma", "beta", "mask", "relu", "dgamma", "dbeta", "ready")

    def __init__(self, kind):
        self.kind, self.ready = kind, False
        self.y = self.stats = self.gamma = self.beta = self.mask = self.dgamma = self.dbeta = None
        self.relu = False


class _ConvBnAct(torch.autograd.Function):
    """relu?(BatchNorm2d(conv2d(x, w)) [+ residual]) in training mode: the ResNet's conv -> bn [-> add] [-> relu]
    chains (torchvision BasicBlock / Bottleneck / downsample behind code/dmcnet/model.py:305,352) on the
    matrix-core NHWC kernels.  The convolution's epilogue reduces the batch statistics (no separate pass
    over its output), one streaming pass normalises / adds / rectifies; the backward runs the BatchNorm
    backward (two passes) and feeds the data- and weight-gradient kernels (deterministic).

    ``xs``: the slice tensor of ``x`` (or None); ``mode`` bit 0: write the fp32 result, bit 1: write its slice tensor
    (returned second, non-differentiable), bit 2: take the pre-split convolution path (conv_x3s.hip), bit 3: the slice
    tensor is written SPACE-TO-DEPTH (its consumer is a stride-2 block pair, conv_x3q.hip)."""

    @staticmethod
    def forward(ctx, x, weight, residual, gamma, beta, running_mean, running_var, stride, padding, relu, eps,
                momentum, link=None, xs=None, mode=1, bn_out=None, bn_in=None):
        lib = _lib.load()
        _need_cuda(x, weight, residual, gamma, beta)
        ctx.set_materialize_grads(False)
        ctx.bn_out, ctx.bn_in = bn_out, None    # else autograd zero-fills a gradient for the slice output every backward
        want_f32, want_xs, use_x3s = bool(mode & 1), bool(mode & 2), bool(mode & 4)
        wcl = _as_cl(weight)
        cout, cin = weight.shape[0], weight.shape[1]
        n, _, h, w = x.shape
        ctx.wsplit_t = None
        ctx.wsplit_t2 = None
        ctx.link = None
        if use_x3s:
            if xs is None:
                xs = x3s_split(_as_cl(x))
            with _span("conv_nhwc_fwd"):
                nb = lib.dmc_x3s_wpack_bytes(cin, cout)
                wf = torch.empty(nb, dtype=torch.uint8, device=x.device)
                ctx.wsplit_t = torch.empty(nb, dtype=torch.uint8, device=x.device) if ctx.needs_input_grad[0] else None
                _lib.check(lib.dmc_x3s_pack_weights(_lib.ptr(wcl), _lib.ptr(wf), _lib.ptr(ctx.wsplit_t), cin, cout, _stream()),
                           "dmc_x3s_pack_weights")
                y = torch.empty((n, cout, h, w), dtype=torch.float32, device=x.device, memory_format=_CL)
                nblk = lib.dmc_x3s_conv_stat_blocks(n, h, w, cout)
                part = torch.empty((nblk, cout, 2), dtype=torch.float64, device=x.device)
                _lib.check(lib.dmc_x3s_conv_fwd(_lib.ptr(xs), _lib.ptr(wf), _lib.ptr(y), _lib.ptr(part), nblk, n, h, w, cin, cout,
                                                _stream()), "dmc_x3s_conv_fwd")
            wf_ok = True
            if bn_in is not None and stride == 1 and ctx.needs_input_grad[0]:
                ctx.bn_in = bn_in                           # this op's data gradient is the producer's output gradient
        else:
            if not f32_valid(x):
                raise RuntimeError("conv_bn_act: the input's fp32 memory was not written by its producer (slices only)")
            x = _as_cl(x)
            with _span("conv_nhwc_fwd"):
                wf = None
                if ctx.needs_input_grad[0] and lib.dmc_conv_nhwc_presplit_supported(cin, cout):
                    # bf16x3 kernels: the forward's and the data gradient's weight slices from ONE launch
                    nb = lib.dmc_conv_nhwc_wt_bytes(cin, cout, weight.shape[2], weight.shape[3])
                    wf, ctx.wsplit_t = _floats(nb, x.device), _floats(nb, x.device)
                    _lib.check(lib.dmc_conv_nhwc_split(_lib.ptr(wcl), _lib.ptr(wf), _lib.ptr(ctx.wsplit_t), cin, cout,
                                                       weight.shape[2], weight.shape[3], _stream()), "dmc_conv_nhwc_split")
                y, part, nblk = _conv_fwd(x, wcl, None, None, stride, padding, 0, True, presplit=wf)
                # 3x3 / stride 2 (layerN.0.conv1): the data gradient in ONE pre-split launch instead of four parity-class launches
                ctx.wsplit_t2 = None
                if (X3S and ctx.needs_input_grad[0] and stride == 2 and padding == 1 and tuple(weight.shape[2:]) == (3, 3)
                        and h == 2 * y.shape[2] and w == 2 * y.shape[3] and lib.dmc_get_option(b"conv_arith") == 1
                        and lib.dmc_x3s_conv_dgrad_s2_supported(n, y.shape[2], y.shape[3], cin, cout)):
                    ctx.wsplit_t2 = torch.empty(lib.dmc_x3s_wpack_bytes(cin, cout), dtype=torch.uint8, device=x.device)
                    _lib.check(lib.dmc_x3s_pack_weights_s2(_lib.ptr(wcl), _lib.ptr(ctx.wsplit_t2), cin, cout, _stream()),
                               "dmc_x3s_pack_weights_s2")
            wf_ok = wf is not None
        if link is not None:
            if residual is None:
                if wf_ok and stride == 1:                   # first op of the block: will add the parked gradient
                    link.armed, ctx.link = True, link
            elif link.armed and ctx.needs_input_grad[2]:    # last op of the block: will park its residual gradient
                ctx.link = link
        n, _, oh, ow = y.shape
        m = n * oh * ow
        stats = _floats(lib.dmc_bn_act_stats_bytes(cout), x.device)
        out = torch.empty_like(y)                           # not written when the consumer reads slices only
        out_xs = _x3s_buffer(m, cout, x.device) if want_xs else None
        mask = None
        if residual is not None:
            if not f32_valid(residual):
                raise RuntimeError("conv_bn_act: the residual's fp32 memory was not written by its producer")
            residual = _as_cl(residual)
            if relu:
                mask = torch.empty(m * (cout // 4), dtype=torch.uint8, device=x.device)
        with _span("bn_apply_fwd"):
            _lib.check(lib.dmc_conv_nhwc_stats_final(_lib.ptr(part), nblk, cout, m, _lib.ptr(stats),
                                                     _lib.ptr(running_mean), _lib.ptr(running_var), float(eps),
                                                     float(momentum), _stream()), "dmc_conv_nhwc_stats_final")
            if want_xs and (mode & 8):
                _lib.check(lib.dmc_bn_apply_act_x3q(_lib.ptr(y), _lib.ptr(residual), _lib.ptr(gamma), _lib.ptr(beta),
                                                    _lib.ptr(stats), _lib.ptr(out) if want_f32 else None, _lib.ptr(out_xs),
                                                    _lib.ptr(mask), n, oh, ow, cout, int(relu), _stream()), "dmc_bn_apply_act_x3q")
            elif want_xs or not want_f32:
                _lib.check(lib.dmc_bn_apply_act_x3s(_lib.ptr(y), _lib.ptr(residual), _lib.ptr(gamma), _lib.ptr(beta),
                                                    _lib.ptr(stats), _lib.ptr(out) if want_f32 else None, _lib.ptr(out_xs),
                                                    _lib.ptr(mask), m, cout, int(relu), _stream()), "dmc_bn_apply_act_x3s")
            else:
                _lib.check(lib.dmc_bn_apply_act_nhwc(_lib.ptr(y), _lib.ptr(residual), _lib.ptr(gamma), _lib.ptr(beta),
                                                     _lib.ptr(stats), _lib.ptr(out), _lib.ptr(mask), m, cout, int(relu),
                                                     _stream()), "dmc_bn_apply_act_nhwc")
        if bn_out is not None:                              # what the consumer's data gradient needs for this op's BatchNorm sums
            bn_out.y, bn_out.stats, bn_out.gamma, bn_out.beta, bn_out.mask, bn_out.relu = y, stats, gamma, beta, mask, bool(relu)
        # the pre-split path keeps the input's slices for its weight gradient, not the fp32 input
        ctx.save_for_backward(xs if use_x3s else x, weight, y, gamma, beta, stats, mask)
        ctx.cfg = (int(stride), int(padding), bool(relu), residual is not None, use_x3s, tuple(x.shape))
        if out_xs is None:
            out_xs = torch.empty(0, dtype=torch.uint8, device=x.device)
        ctx.mark_non_differentiable(out_xs)
        return out, out_xs

    @staticmethod
    def backward(ctx, dout, _dxs):
        lib = _lib.load()
        x, weight, y, gamma, beta, stats, mask = ctx.saved_tensors
        if dout is None:                    # the result did not reach the loss
            return (None,) * 17
        stride, padding, relu, has_res, use_x3s, x_shape = ctx.cfg
        n, cout, oh, ow = y.shape
        m = n * oh * ow
        cin = weight.shape[1]
        dout = _as_cl(dout)
        want_dres = has_res and ctx.needs_input_grad[2]
        dres = torch.empty_like(y) if (want_dres and relu) else None
        dgamma, dbeta = torch.empty_like(gamma), torch.empty_like(gamma)
        scratch = _floats(lib.dmc_bn_act_scratch_bytes(cout), y.device)
        dy = dys = None
        pre = ctx.bn_out is not None and ctx.bn_out.ready   # the consumer's data gradient already reduced dgamma / dbeta
        with _span("bn_act_bwd"):
            if pre:
                dgamma, dbeta = ctx.bn_out.dgamma, ctx.bn_out.dbeta
                s2 = ctx.wsplit_t2 is not None and ctx.needs_input_grad[0]
                if use_x3s or s2:
                    dys = _x3s_buffer(m, cout, y.device)
                if not use_x3s:
                    dy = torch.empty_like(y)
                _lib.check(lib.dmc_bn_act_bwd_x3s_apply(_lib.ptr(y), None, _lib.ptr(gamma), _lib.ptr(beta), _lib.ptr(stats),
                                                        _lib.ptr(dout), _lib.ptr(dy), _lib.ptr(dys), _lib.ptr(dres),
                                                        _lib.ptr(dgamma), _lib.ptr(dbeta), _lib.ptr(mask), m, cout,
                                                        int(relu), _stream()), "dmc_bn_act_bwd_x3s_apply")
            elif use_x3s:                                   # the convolution's output gradient: slices only
                dys = _x3s_buffer(m, cout, y.device)
                _lib.check(lib.dmc_bn_act_bwd_x3s(_lib.ptr(y), None, _lib.ptr(gamma), _lib.ptr(beta), _lib.ptr(stats),
                                                  _lib.ptr(scratch), _lib.ptr(dout), None, _lib.ptr(dys), _lib.ptr(dres),
                                                  _lib.ptr(dgamma), _lib.ptr(dbeta), _lib.ptr(mask), m, cout,
                                                  int(relu), _stream()), "dmc_bn_act_bwd_x3s")
            elif ctx.wsplit_t2 is not None and ctx.needs_input_grad[0]:   # fp32 for the weight gradient, slices for the data gradient
                dy = torch.empty_like(y)
                dys = _x3s_buffer(m, cout, y.device)
                _lib.check(lib.dmc_bn_act_bwd_x3s(_lib.ptr(y), None, _lib.ptr(gamma), _lib.ptr(beta), _lib.ptr(stats),
                                                  _lib.ptr(scratch), _lib.ptr(dout), _lib.ptr(dy), _lib.ptr(dys), _lib.ptr(dres),
                                                  _lib.ptr(dgamma), _lib.ptr(dbeta), _lib.ptr(mask), m, cout,
                                                  int(relu), _stream()), "dmc_bn_act_bwd_x3s")
            else:
                dy = torch.empty_like(y)
                _lib.check(lib.dmc_bn_act_bwd(_lib.ptr(y), None, _lib.ptr(gamma), _lib.ptr(beta), _lib.ptr(stats),
                                              _lib.ptr(scratch), _lib.ptr(dout), _lib.ptr(dy), _lib.ptr(dres),
                                              _lib.ptr(dgamma), _lib.ptr(dbeta), _lib.ptr(mask), m, cout,
                                              int(relu), _stream()), "dmc_bn_act_bwd")
        if want_dres and not relu:
            dres = dout
        addend = None
        if ctx.link is not None:
            if has_res:
                ctx.link.grad, dres = dres, None            # parked for the block's first op (ResidualGradLink)
            else:
                addend, ctx.link.grad = ctx.link.grad, None
        wcl = _as_cl(weight)
        dx = dw = None
        if use_x3s:
            nn_, _, h, w = x_shape
            if ctx.needs_input_grad[0]:
                with _span("conv_nhwc_dgrad"):
                    dx = torch.empty(x_shape, dtype=torch.float32, device=y.device, memory_format=_CL)
                    if addend is not None:
                        addend = _as_cl(addend)
                    bl = ctx.bn_in
                    if bl is not None and bl.y is not None and (bl.kind == "inner" or addend is not None):
                        # dx is the producer's COMPLETE output gradient: reduce its BatchNorm sums in this launch's epilogue
                        nblk = lib.dmc_x3s_conv_stat_blocks(nn_, h, w, cin)
                        part = torch.empty((nblk, cin, 2), dtype=torch.float64, device=y.device)
                        bl.dgamma, bl.dbeta = torch.empty_like(bl.gamma), torch.empty_like(bl.gamma)
                        _lib.check(lib.dmc_x3s_conv_dgrad_bnb(_lib.ptr(dys), _lib.ptr(ctx.wsplit_t), _lib.ptr(addend), _lib.ptr(dx),
                                                              _lib.ptr(bl.y), _lib.ptr(bl.stats), _lib.ptr(bl.gamma), _lib.ptr(bl.beta),
                                                              _lib.ptr(bl.mask), int(bl.relu), _lib.ptr(part), nblk, _lib.ptr(bl.dgamma),
                                                              _lib.ptr(bl.dbeta), nn_, h, w, cin, cout, _stream()),
                                   "dmc_x3s_conv_dgrad_bnb")
                        bl.ready = True
                    else:
                        _lib.check(lib.dmc_x3s_conv_dgrad(_lib.ptr(dys), _lib.ptr(ctx.wsplit_t), _lib.ptr(addend), _lib.ptr(dx),
                                                          nn_, h, w, cin, cout, _stream()), "dmc_x3s_conv_dgrad")
            if ctx.needs_input_grad[1]:
                with _span("conv_nhwc_wgrad"):
                    def launch():
                        dwc = torch.empty((cout, cin, 3, 3), dtype=torch.float32, device=y.device, memory_format=_CL)
                        work = _floats(lib.dmc_x3s_conv_wgrad_bytes(nn_, h, w, cin, cout), y.device)
                        _lib.check(lib.dmc_x3s_conv_wgrad(_lib.ptr(x), _lib.ptr(dys), _lib.ptr(dwc), _lib.ptr(work), nn_, h, w, cin,
                                                          cout, _stream()), "dmc_x3s_conv_wgrad")
                        return _grad_like(dwc, weight)
                    dw = _on_wgrad_stream(weight, (x, dys), launch)
        else:
            if ctx.needs_input_grad[0]:
                with _span("conv_nhwc_dgrad"):
                    if dys is not None:
                        dx = torch.empty(x_shape, dtype=torch.float32, device=y.device, memory_format=_CL)
                        _lib.check(lib.dmc_x3s_conv_dgrad_s2(_lib.ptr(dys), _lib.ptr(ctx.wsplit_t2), _lib.ptr(dx), n, oh, ow, cin,
                                                             cout, _stream()), "dmc_x3s_conv_dgrad_s2")
                    else:
                        dx = _conv_dgrad(dy, wcl, x.shape, stride, padding, presplit=ctx.wsplit_t, addend=addend)
            if ctx.needs_input_grad[1]:
                with _span("conv_nhwc_wgrad"):
                    dw = _on_wgrad_stream(weight, (x, dy), lambda: _grad_like(_conv_wgrad(x, dy, wcl, stride, padding), weight))
        return dx, dw, dres, dgamma, dbeta, None, None, None, None, None, None, None, None, None, None, None, None


def conv_bn_act_supported(x, conv, bn):
    """True if conv -> bn [-> add] [-> relu] can run as the fused NHWC training op."""
    if not (torch.is_grad_enabled() and bn.training and bn.track_running_stats and bn.affine):
        return False
    if bn.momentum is None:                       # cumulative moving average: the stock module handles it
        return False
    if conv.bias is not None or conv.dilation != (1, 1) or conv.groups != 1 or conv.padding_mode != "zeros":
        return False
    if conv.stride[0] != conv.stride[1] or conv.padding[0] != conv.padding[1]:
        return False
    if not _is_cl(x) or not conv_nhwc_supported(x, conv.weight, conv.stride[0], conv.padding[0]):
        return False
    n, _, h, w = x.shape
    k, s, p = conv.kernel_size[0], conv.stride[0], conv.padding[0]
    oh, ow = (h + 2 * p - k) // s + 1, (w + 2 * p - k) // s + 1
    return bool(_lib.load().dmc_bn_act_supported(n * oh * ow, conv.out_channels))


def conv_bn_eval_supported(x, conv, bn):
    """True if conv -> bn(running statistics) [-> add] [-> relu] can run forward-only on this package's kernels
    (evaluation / validation: code/dmcnet/test.py:139-198, validate() of code/dmcnet/train.py)."""
    if torch.is_grad_enabled() or bn.training or not bn.track_running_stats or not bn.affine:
        return False
    if conv.bias is not None or conv.dilation != (1, 1) or conv.groups != 1 or conv.padding_mode != "zeros":
        return False
    if conv.stride[0] != conv.stride[1] or conv.padding[0] != conv.padding[1]:
        return False
    if not _is_cl(x) or not conv_nhwc_supported(x, conv.weight, conv.stride[0], conv.padding[0]):
        return False
    n, _, h, w = x.shape
    k, s, p = conv.kernel_size[0], conv.stride[0], conv.padding[0]
    oh, ow = (h + 2 * p - k) // s + 1, (w + 2 * p - k) // s + 1
    return bool(_lib.load().dmc_bn_act_supported(n * oh * ow, conv.out_channels)) and conv.out_channels % 16 == 0


def _bn_eval_stats(bn):
    """[mean[C], 1 / sqrt(var + eps)[C]] of a BatchNorm's running statistics.  Built on EVERY call: the training kernels update the
    buffers through raw pointers, which a tensor version counter does not see, so nothing derived from them may be cached."""
    return torch.cat([bn.running_mean, torch.rsqrt(bn.running_var + bn.eps)]).contiguous()


def conv_bn_act_eval(x, conv, bn, residual=None, relu=True, want_f32=True, want_slices=False, s2d=False, fused=True):
    """Forward-only relu?(bn(conv(x)) [+ residual]) with the BatchNorm's RUNNING statistics (eval mode, no autograd).

    A convolution on the pre-split path (x3s_usable) is ONE launch, dmc_x3s_conv_bn_eval: the normalisation, the shortcut and
    the ReLU run in the convolution's epilogue and no fp32 convolution result reaches memory.  ``fused=False`` -- and every
    other convolution -- takes two passes: the convolution kernel of the training op without its statistics epilogue, then
    the normalisation as one streaming pass; the results are bit-identical.  ``want_slices``: the result's slice tensor is
    written too (x3s_of); ``s2d``: that tensor is space-to-depth (x3q_of) for a stride-2 pair that is the result's only
    reader; ``want_f32=False``: slices only, the returned tensor's fp32 memory stays unwritten (f32_valid)."""
    lib = _lib.load()
    _need_cuda(x, conv.weight, residual)
    n, cin, h, w = x.shape
    cout = conv.out_channels
    wcl = _as_cl(conv.weight.detach())
    stride, padding = conv.stride[0], conv.padding[0]
    if not want_f32 and not want_slices:
        want_f32 = True
    s2d = bool(s2d and want_slices)
    if residual is not None:
        if not f32_valid(residual):
            raise RuntimeError("conv_bn_act_eval: the residual's fp32 memory was not written by its producer")
        residual = _as_cl(residual)
    use_x3s = x3s_usable(n, h, w, conv)
    if use_x3s:
        xs = x3s_of(x)
        if xs is None:
            if not f32_valid(x):
                raise RuntimeError("conv_bn_act_eval: the input carries neither slices nor valid fp32 memory")
            xs = x3s_split(_as_cl(x))
        wf, _ = x3s_pack_weights(wcl, forward=True, transposed=False)
    stats = _bn_eval_stats(bn)
    if use_x3s and fused:
        out = torch.empty((n, cout, h, w), dtype=torch.float32, device=x.device, memory_format=_CL)
        out_xs = _x3s_buffer(n * h * w, cout, x.device) if want_slices else None
        _lib.check(lib.dmc_x3s_conv_bn_eval(_lib.ptr(xs), _lib.ptr(wf), _lib.ptr(stats), _lib.ptr(bn.weight), _lib.ptr(bn.bias),
                                            _lib.ptr(residual), _lib.ptr(out) if want_f32 else None, _lib.ptr(out_xs), int(s2d),
                                            int(relu), n, h, w, cin, cout, _stream()), "dmc_x3s_conv_bn_eval")
    else:
        if use_x3s:
            y, _ = x3s_conv_fwd(xs, wf, n, h, w, cin, cout)
        else:
            if not f32_valid(x):
                raise RuntimeError("conv_bn_act_eval: the input's fp32 memory was not written by its producer (slices only)")
            y, _, _ = _conv_fwd(_as_cl(x), wcl, None, None, stride, padding, 0, False)
        m = y.shape[0] * y.shape[2] * y.shape[3]
        out = torch.empty_like(y)
        out_xs = _x3s_buffer(m, cout, x.device) if want_slices else None
        if s2d:
            _lib.check(lib.dmc_bn_apply_act_x3q(_lib.ptr(y), _lib.ptr(residual), _lib.ptr(bn.weight), _lib.ptr(bn.bias), _lib.ptr(stats),
                                                _lib.ptr(out) if want_f32 else None, _lib.ptr(out_xs), None, y.shape[0], y.shape[2],
                                                y.shape[3], cout, int(relu), _stream()), "dmc_bn_apply_act_x3q")
        else:
            _lib.check(lib.dmc_bn_apply_act_x3s(_lib.ptr(y), _lib.ptr(residual), _lib.ptr(bn.weight), _lib.ptr(bn.bias), _lib.ptr(stats),
                                                _lib.ptr(out) if want_f32 else None, _lib.ptr(out_xs), None, m, cout, int(relu),
                                                _stream()), "dmc_bn_apply_act_x3s")
    if s2d:
        out._dmc_x3q, out._dmc_f32 = out_xs, want_f32
    elif want_slices:
        _attach_x3s(out, out_xs, want_f32)
    return out


def conv_bn_act(x, conv, bn, residual=None, relu=True, link=None, want_f32=True, want_slices=False, bn_link=None, s2d=False):
    """relu?(bn(conv(x)) [+ residual]) for a channels_last ``x`` (see conv_bn_act_supported); ``link``: the
    ResidualGradLink shared by the first and the last op of an identity-shortcut block.  ``want_slices``: also write
    the result's bf16x3 slice tensor (attached to the returned tensor, see x3s_of) for a pre-split consumer;
    ``want_f32=False``: ONLY the slices -- the returned tensor's fp32 memory is then not written (f32_valid).
    ``bn_link``: "inner" / "block" -- the result has ONE pre-split consumer (see BnBwdLink); the link travels on the
    returned tensor and that consumer picks it up from its input."""
    if bn.num_batches_tracked is not None:
        if _PENDING_COUNTERS is not None:
            _PENDING_COUNTERS.append(bn.num_batches_tracked)
        else:
            bn.num_batches_tracked.add_(1)
    if not want_f32 and not want_slices:
        want_f32 = True
    n, _, h, w = x.shape
    use_x3s = x3s_usable(n, h, w, conv)
    mode = int(want_f32) | (int(want_slices) << 1) | (int(use_x3s) << 2) | (int(bool(s2d and want_slices)) << 3)
    bn_out = BnBwdLink(bn_link) if (bn_link and BN_BWD_LINK and want_slices and not s2d) else None
    bn_in = getattr(x, "_dmc_bnlink", None) if use_x3s else None
    out, out_xs = _ConvBnAct.apply(x, conv.weight, residual, bn.weight, bn.bias, bn.running_mean, bn.running_var,
                                   conv.stride[0], conv.padding[0], relu, bn.eps,
                                   bn.momentum if bn.momentum is not None else 0.1, link,
                                   x3s_of(x) if use_x3s else None, mode, bn_out, bn_in)
    if want_slices and s2d:
        out._dmc_x3q, out._dmc_f32 = out_xs, want_f32
    elif want_slices:
        _attach_x3s(out, out_xs, want_f32)
    if bn_out is not None:
        out._dmc_bnlink = bn_out
    return out


# ------------------------------------------------------------------ the stride-2 block pair (conv_x3q.hip)
#: True (default): a BasicBlock with a stride-2 conv1 and a 1x1 / stride-2 downsample runs both convolutions -- which read
#: the same block input -- as ONE launch per direction on the input's space-to-depth slice tensor.  DMC_X3Q=0: the separate
#: in-loop-split launches of conv_nhwc.hip (+ the stride-2 data gradient of conv_x3s.hip).
X3Q = __import__("os").environ.get("DMC_X3Q", "1") != "0"


def x3q_of(t):
    """The space-to-depth slice tensor attached to activation ``t`` by its producer (or None)."""
    return getattr(t, "_dmc_x3q", None)


def _bn_trains(bn):
    return bn.training and bn.track_running_stats and bn.affine and bn.momentum is not None


def s2_pair_usable(x_shape, unit):
    """True if ``unit`` (a resnet.ResidualUnit of kind "basic" with a downsample branch) on an input of ``x_shape`` takes the
    fused stride-2 pair path: conv1 3x3 / stride 2 / padding 1 and downsample = (1x1 / stride 2, BatchNorm2d), both bias-free,
    BatchNorms in training mode, autograd on, shapes the kernels cover.  The producer of the block input asks the same
    question to decide the layout (and the absence of an fp32 copy) of what it writes."""
    if not (X3Q and X3S and torch.is_grad_enabled()):
        return False
    ds = getattr(unit, "downsample", None)
    if getattr(unit, "kind", None) != "basic" or ds is None or len(ds) != 2:
        return False
    c3, c1 = unit.conv1, ds[0]
    for c, k, p in ((c3, (3, 3), (1, 1)), (c1, (1, 1), (0, 0))):
        if not isinstance(c, torch.nn.Conv2d) or c.kernel_size != k or c.stride != (2, 2) or c.padding != p or c.bias is not None:
            return False
        if c.dilation != (1, 1) or c.groups != 1 or c.padding_mode != "zeros" or c.weight.dtype != torch.float32:
            return False
    if not isinstance(ds[1], torch.nn.BatchNorm2d) or not _bn_trains(unit.bn1) or not _bn_trains(ds[1]):
        return False
    n, cin, h, w = x_shape
    cout = c3.out_channels
    if c3.in_channels != cin or c1.in_channels != cin or c1.out_channels != cout or (h & 1) or (w & 1):
        return False
    lib = _lib.load()
    if lib.dmc_get_option(b"conv_arith") != 1 or lib.dmc_get_option(b"conv_path") != 1:
        return False
    return bool(lib.dmc_x3q_supported(n, h // 2, w // 2, cin, cout)) and bool(lib.dmc_x3q_conv_wgrad_supported(n, h // 2, w // 2, cin, cout)) \
        and bool(lib.dmc_bn_act_supported(n * (h // 2) * (w // 2), cout))


class _ConvBnS2Pair(torch.autograd.Function):
    """(relu(bn1(conv1(x))), bn_d(downsample_conv(x))) of a stride-2 BasicBlock (torchvision, behind code/dmcnet/model.py:305,352)
    in training mode: ONE convolution launch for both branches (conv_x3q.hip: the shortcut reads the centre tap's operand), both
    BatchNorms' statistics from its epilogue; the backward runs the two BatchNorm backwards (slice outputs), ONE data-gradient
    launch for the sum of both branches and the two weight gradients from one call.  ``xq``: the space-to-depth slice tensor
    of ``x``; ``x`` itself only carries the autograd edge (its fp32 memory may be unwritten).  ``want_xs``: the main branch's
    result is written as a slice tensor ONLY (its consumer, conv2, takes the pre-split path)."""

    @staticmethod
    def forward(ctx, x, xq, w3, w1, g3, b3, rm3, rv3, eps3, mom3, g1, b1, rm1, rv1, eps1, mom1, want_xs):
        lib = _lib.load()
        _need_cuda(x, w3, w1, g3, b3, g1, b1)
        ctx.set_materialize_grads(False)
        n, cin, h, w = x.shape
        cout, oh, ow = w3.shape[0], h // 2, w // 2
        m = n * oh * ow
        dev = x.device
        with _span("conv_nhwc_fwd"):
            nb = lib.dmc_x3q_wpack_bytes(cin, cout)
            wf = torch.empty(nb, dtype=torch.uint8, device=dev)
            ctx.wt = torch.empty(nb, dtype=torch.uint8, device=dev) if ctx.needs_input_grad[0] else None
            _lib.check(lib.dmc_x3q_pack_weights(_lib.ptr(_as_cl(w3)), _lib.ptr(_as_cl(w1)), _lib.ptr(wf), _lib.ptr(ctx.wt), cin, cout,
                                                _stream()), "dmc_x3q_pack_weights")
            y3 = torch.empty((n, cout, oh, ow), dtype=torch.float32, device=dev, memory_format=_CL)
            y1 = torch.empty_like(y3)
            nblk = lib.dmc_x3q_stat_blocks(n, oh, ow, cout)
            part = torch.empty((2, nblk, cout, 2), dtype=torch.float64, device=dev)
            _lib.check(lib.dmc_x3q_conv_fwd(_lib.ptr(xq), _lib.ptr(wf), _lib.ptr(y3), _lib.ptr(y1), _lib.ptr(part[0]), _lib.ptr(part[1]),
                                            nblk, n, oh, ow, cin, cout, _stream()), "dmc_x3q_conv_fwd")
        stats3 = _floats(lib.dmc_bn_act_stats_bytes(cout), dev)
        stats1 = _floats(lib.dmc_bn_act_stats_bytes(cout), dev)
        out3 = torch.empty_like(y3)                         # not written when conv2 reads slices only
        out3_xs = _x3s_buffer(m, cout, dev) if want_xs else None
        out1 = torch.empty_like(y1)
        with _span("bn_apply_fwd"):
            _lib.check(lib.dmc_conv_nhwc_stats_final(_lib.ptr(part[0]), nblk, cout, m, _lib.ptr(stats3), _lib.ptr(rm3), _lib.ptr(rv3),
                                                     float(eps3), float(mom3), _stream()), "dmc_conv_nhwc_stats_final")
            _lib.check(lib.dmc_conv_nhwc_stats_final(_lib.ptr(part[1]), nblk, cout, m, _lib.ptr(stats1), _lib.ptr(rm1), _lib.ptr(rv1),
                                                     float(eps1), float(mom1), _stream()), "dmc_conv_nhwc_stats_final")
            _lib.check(lib.dmc_bn_apply_act_x3s(_lib.ptr(y3), None, _lib.ptr(g3), _lib.ptr(b3), _lib.ptr(stats3),
                                                None if want_xs else _lib.ptr(out3), _lib.ptr(out3_xs), None, m, cout, 1, _stream()),
                       "dmc_bn_apply_act_x3s")
            _lib.check(lib.dmc_bn_apply_act_nhwc(_lib.ptr(y1), None, _lib.ptr(g1), _lib.ptr(b1), _lib.ptr(stats1), _lib.ptr(out1), None,
                                                 m, cout, 0, _stream()), "dmc_bn_apply_act_nhwc")
        ctx.save_for_backward(xq, w3, w1, y3, y1, g3, b3, stats3, g1, b1, stats1)
        ctx.shape = (n, cin, h, w, cout)
        if out3_xs is None:
            out3_xs = torch.empty(0, dtype=torch.uint8, device=dev)
        ctx.mark_non_differentiable(out3_xs)
        return out3, out3_xs, out1

    @staticmethod
    def backward(ctx, dout3, _dxs, dout1):
        lib = _lib.load()
        xq, w3, w1, y3, y1, g3, b3, stats3, g1, b1, stats1 = ctx.saved_tensors
        n, cin, h, w, cout = ctx.shape
        oh, ow = h // 2, w // 2
        m = n * oh * ow
        if dout3 is None and dout1 is None:
            return (None,) * 17
        dout3 = torch.zeros_like(y3) if dout3 is None else _as_cl(dout3)
        dout1 = torch.zeros_like(y1) if dout1 is None else _as_cl(dout1)
        dg3, db3, dg1, db1 = torch.empty_like(g3), torch.empty_like(g3), torch.empty_like(g1), torch.empty_like(g1)
        dys3, dys1 = _x3s_buffer(m, cout, y3.device), _x3s_buffer(m, cout, y3.device)
        with _span("bn_act_bwd"):
            for y, g, b, st, dout, dys, dg, db, relu in ((y3, g3, b3, stats3, dout3, dys3, dg3, db3, 1),
                                                          (y1, g1, b1, stats1, dout1, dys1, dg1, db1, 0)):
                scratch = _floats(lib.dmc_bn_act_scratch_bytes(cout), y.device)
                _lib.check(lib.dmc_bn_act_bwd_x3s(_lib.ptr(y), None, _lib.ptr(g), _lib.ptr(b), _lib.ptr(st), _lib.ptr(scratch),
                                                  _lib.ptr(dout), None, _lib.ptr(dys), None, _lib.ptr(dg), _lib.ptr(db), None,
                                                  m, cout, relu, _stream()), "dmc_bn_act_bwd_x3s")
        dx = dw3 = dw1 = None
        if ctx.needs_input_grad[0]:
            with _span("conv_nhwc_dgrad"):
                dx = torch.empty((n, cin, h, w), dtype=torch.float32, device=y3.device, memory_format=_CL)
                _lib.check(lib.dmc_x3q_conv_dgrad(_lib.ptr(dys3), _lib.ptr(dys1), _lib.ptr(ctx.wt), _lib.ptr(dx), n, oh, ow, cin, cout,
                                                  _stream()), "dmc_x3q_conv_dgrad")
        if ctx.needs_input_grad[2] or ctx.needs_input_grad[3]:
            with _span("conv_nhwc_wgrad"):
                def launch():
                    d3 = torch.empty((cout, cin, 3, 3), dtype=torch.float32, device=y3.device, memory_format=_CL)
                    d1 = torch.empty((cout, cin, 1, 1), dtype=torch.float32, device=y3.device, memory_format=_CL)
                    work = _floats(lib.dmc_x3q_conv_wgrad_bytes(n, oh, ow, cin, cout), y3.device)
                    _lib.check(lib.dmc_x3q_conv_wgrad(_lib.ptr(xq), _lib.ptr(dys3), _lib.ptr(dys1), _lib.ptr(d3), _lib.ptr(d1),
                                                      _lib.ptr(work), n, oh, ow, cin, cout, _stream()), "dmc_x3q_conv_wgrad")
                    return _grad_like(d3, w3), _grad_like(d1, w1)
                dw3, dw1 = _on_wgrad_stream((w3, w1), (xq, dys3, dys1), launch)
        return dx, None, dw3, dw1, dg3, db3, None, None, None, None, dg1, db1, None, None, None, None, None


def conv_bn_s2_pair(x, unit, want_slices):
    """(relu(bn1(conv1(x))), downsample(x)) of a stride-2 BasicBlock ``unit`` (see s2_pair_usable); ``want_slices``: conv2 of
    the unit takes the pre-split path, the first result is returned as slices only (x3s_of)."""
    bn3, bn1 = unit.bn1, unit.downsample[1]
    for bn in (bn3, bn1):
        if bn.num_batches_tracked is not None:
            if _PENDING_COUNTERS is not None:
                _PENDING_COUNTERS.append(bn.num_batches_tracked)
            else:
                bn.num_batches_tracked.add_(1)
    xq = x3q_of(x)
    if xq is None:
        if not f32_valid(x):
            raise RuntimeError("conv_bn_s2_pair: the input carries neither s2d slices nor valid fp32 memory")
        xq = x3q_split(_as_cl(x))
    out3, out3_xs, out1 = _ConvBnS2Pair.apply(x, xq, unit.conv1.weight, unit.downsample[0].weight, bn3.weight, bn3.bias,
                                              bn3.running_mean, bn3.running_var, bn3.eps, bn3.momentum, bn1.weight, bn1.bias,
                                              bn1.running_mean, bn1.running_var, bn1.eps, bn1.momentum, bool(want_slices))
    if want_slices:
        _attach_x3s(out3, out3_xs, False)
    return out3, out1


def _bn_evals(bn):
    return (not bn.training) and bn.track_running_stats and bn.affine


def _s2_pair_eval_unit_ok(unit):
    """The part of s2_pair_eval_usable that looks at modes and structure only (no device, no shape): autograd off, a "basic" unit
    whose conv1 is 3x3 / stride 2 / padding 1 and whose downsample is (1x1 / stride 2, BatchNorm2d), both bias-free fp32, both
    BatchNorms in eval mode with running statistics."""
    if not (X3Q and X3S) or torch.is_grad_enabled():
        return False
    ds = getattr(unit, "downsample", None)
    if getattr(unit, "kind", None) != "basic" or ds is None or len(ds) != 2:
        return False
    for c, k, p in ((unit.conv1, (3, 3), (1, 1)), (ds[0], (1, 1), (0, 0))):
        if not isinstance(c, torch.nn.Conv2d) or c.kernel_size != k or c.stride != (2, 2) or c.padding != p or c.bias is not None:
            return False
        if c.dilation != (1, 1) or c.groups != 1 or c.padding_mode != "zeros" or c.weight.dtype != torch.float32:
            return False
    return isinstance(ds[1], torch.nn.BatchNorm2d) and _bn_evals(unit.bn1) and _bn_evals(ds[1])


def s2_pair_eval_usable(x_shape, unit):
    """The no-grad, eval-BatchNorm counterpart of s2_pair_usable: True if ``unit`` (a "basic" resnet.ResidualUnit with a
    downsample branch, on the GPU) on an input of ``x_shape`` takes conv_bn_s2_pair_eval -- conv1 3x3 / stride 2 / padding 1 and
    downsample = (1x1 / stride 2, BatchNorm2d), both bias-free, both BatchNorms in eval mode with running statistics, autograd
    off, a shape the forward kernel covers (no weight gradient is needed).  The producer of the block input asks the same
    question before it writes space-to-depth slices and leaves the fp32 form unwritten."""
    if not _s2_pair_eval_unit_ok(unit):
        return False
    c3, c1 = unit.conv1, unit.downsample[0]
    if not (c3.weight.is_cuda and c1.weight.is_cuda):
        return False
    n, cin, h, w = x_shape
    cout = c3.out_channels
    if c3.in_channels != cin or c1.in_channels != cin or c1.out_channels != cout or (h & 1) or (w & 1):
        return False
    lib = _lib.load()
    if lib.dmc_get_option(b"conv_arith") != 1 or lib.dmc_get_option(b"conv_path") != 1:
        return False
    return bool(lib.dmc_x3q_supported(n, h // 2, w // 2, cin, cout))


def conv_bn_s2_pair_eval(x, unit, want_slices):
    """(relu(bn1(conv1(x))), downsample(x)) of a stride-2 BasicBlock ``unit`` in eval mode (see s2_pair_eval_usable): ONE launch,
    dmc_x3q_conv_bn_eval, for both convolutions and both running-statistics BatchNorms.  ``x`` carries its space-to-depth
    slice tensor (x3q_of) or valid fp32 memory, which is split on the fly; ``want_slices``: conv2 of the unit takes the
    pre-split path, the first result is returned as slices only (x3s_of)."""
    lib = _lib.load()
    bn3, bn1 = unit.bn1, unit.downsample[1]
    w3, w1 = unit.conv1.weight.detach(), unit.downsample[0].weight.detach()
    _need_cuda(x, w3, w1)
    xq = x3q_of(x)
    if xq is None:
        if not f32_valid(x):
            raise RuntimeError("conv_bn_s2_pair_eval: the input carries neither s2d slices nor valid fp32 memory")
        xq = x3q_split(_as_cl(x))
    n, cin, h, w = x.shape
    cout, oh, ow = w3.shape[0], h // 2, w // 2
    wf, _ = x3q_pack_weights(w3, w1, forward=True, transposed=False)
    stats3, stats1 = _bn_eval_stats(bn3), _bn_eval_stats(bn1)
    out3 = torch.empty((n, cout, oh, ow), dtype=torch.float32, device=x.device, memory_format=_CL)   # not written when conv2 reads slices only
    out3_xs = _x3s_buffer(n * oh * ow, cout, x.device) if want_slices else None
    out1 = torch.empty_like(out3)
    _lib.check(lib.dmc_x3q_conv_bn_eval(_lib.ptr(xq), _lib.ptr(wf), _lib.ptr(stats3), _lib.ptr(bn3.weight), _lib.ptr(bn3.bias),
                                        _lib.ptr(stats1), _lib.ptr(bn1.weight), _lib.ptr(bn1.bias),
                                        None if want_slices else _lib.ptr(out3), _lib.ptr(out3_xs), _lib.ptr(out1), n, oh, ow, cin, cout,
                                        _stream()), "dmc_x3q_conv_bn_eval")
    if want_slices:
        _attach_x3s(out3, out3_xs, False)
    return out3, out1


class _DiscBlock(torch.autograd.Function):
    """One discriminator block, Conv2d(3x3, stride s, padding 1, bias) -> LeakyReLU(0.2) ->
    Dropout2d keep mask -> [BatchNorm2d(eps 0.8)], code/dmcnet_GAN/model.py:254-279, on NHWC tensors:
    the convolution epilogue applies bias / LeakyReLU / mask and reduces the BatchNorm statistics, one
    streaming pass normalises; the backward folds the BatchNorm backward, the mask and the LeakyReLU
    derivative into one pass and feeds the matrix-core data / weight gradients.
    ``first`` = 1 / True: the 2-channel NCHW input block (direct kernels, disc_first.hip); 2: Discriminator4's 8 -> 16 block on
    NHWC (direct kernels, disc_c8.hip: the same epilogue and statistic partials as the matrix-core route); 0: conv_nhwc.hip."""

    @staticmethod
    def forward(ctx, x, weight, bias, keep, gamma, beta, running_mean, running_var, stride, training, eps,
                momentum, first):
        lib = _lib.load()
        _need_cuda(x, weight, bias, keep, gamma, beta)
        use_bn = gamma is not None
        cout = weight.shape[0]
        if first == 1:
            x = x.contiguous()
            m, _, h, w = x.shape
            oh, ow = (h - 1) // 2 + 1, (w - 1) // 2 + 1
            wq = weight.contiguous()
            z = torch.empty((m, cout, oh, ow), dtype=torch.float32, device=x.device, memory_format=_CL)
            with _span("disc_first_fwd"):
                _lib.check(lib.dmc_disc_first_fwd(_lib.ptr(x), _lib.ptr(wq), _lib.ptr(bias), _lib.ptr(keep), _lib.ptr(z),
                                                  m, h, w, cout, 1, _stream()), "dmc_disc_first_fwd")
            part, nblk = None, 0
            if use_bn:
                raise NotImplementedError("the 2-channel first block has no BatchNorm in any discriminator")
        elif first == 2:
            x, wq = _as_cl(x), _as_cl(weight)
            m, _, h, w = x.shape
            z = torch.empty((m, cout, (h - 1) // 2 + 1, (w - 1) // 2 + 1), dtype=torch.float32, device=x.device, memory_format=_CL)
            part, nblk = None, 0
            if use_bn and training:
                nblk = lib.dmc_disc_c8_stat_blocks(m, h, w)
                part = torch.empty((nblk, cout, 2), dtype=torch.float64, device=x.device)
            with _span("disc_c8_fwd"):
                _lib.check(lib.dmc_disc_c8_fwd(_lib.ptr(x), _lib.ptr(wq), _lib.ptr(bias), _lib.ptr(keep), _lib.ptr(z), _lib.ptr(part),
                                               nblk, m, h, w, 1, _stream()), "dmc_disc_c8_fwd")
        else:
            x, wq = _as_cl(x), _as_cl(weight)
            with _span("disc_conv_fwd"):
                z, part, nblk = _conv_fwd(x, wq, bias, keep, stride, 1, 1, use_bn and training)
        if DEBUG_DISC_Z is not None:
            DEBUG_DISC_Z.append(z)
        y, stats = z, None
        if use_bn:
            m_rows = z.shape[0] * z.shape[2] * z.shape[3]
            stats = _floats(lib.dmc_bn_act_stats_bytes(cout), x.device)
            y = torch.empty_like(z)
            with _span("disc_bn_fwd"):
                if training:
                    _lib.check(lib.dmc_conv_nhwc_stats_final(_lib.ptr(part), nblk, cout, m_rows, _lib.ptr(stats),
                                                             _lib.ptr(running_mean), _lib.ptr(running_var),
                                                             float(eps), float(momentum), _stream()),
                               "dmc_conv_nhwc_stats_final")
                    _lib.check(lib.dmc_bn_apply_nhwc(_lib.ptr(z), _lib.ptr(gamma), _lib.ptr(beta), _lib.ptr(stats),
                                                     _lib.ptr(y), m_rows, cout, _stream()), "dmc_bn_apply_nhwc")
                else:
                    _lib.check(lib.dmc_bn_act_fwd(_lib.ptr(z), None, _lib.ptr(gamma), _lib.ptr(beta),
                                                  _lib.ptr(running_mean), _lib.ptr(running_var), _lib.ptr(y),
                                                  _lib.ptr(stats), None, None, m_rows, cout, 0, 0, float(eps),
                                                  float(momentum), _stream()), "dmc_bn_act_fwd")
        ctx.save_for_backward(x, weight, z, keep, gamma, beta, stats)
        ctx.cfg = (int(stride), bool(training), int(first), use_bn, bias is not None)
        return y

    @staticmethod
    def backward(ctx, dy):
        lib = _lib.load()
        x, weight, z, keep, gamma, beta, stats = ctx.saved_tensors
        stride, training, first, use_bn, has_bias = ctx.cfg
        if use_bn and not training:
            raise NotImplementedError("backward through eval-mode BatchNorm is not implemented")
        dy = _as_cl(dy)
        m, cout, oh, ow = z.shape
        rows = m * oh * ow
        g = torch.empty_like(z)
        dgamma = dbeta = None
        scratch = _floats(lib.dmc_bn_act_scratch_bytes(cout), z.device)
        if use_bn:
            dgamma, dbeta = torch.empty_like(gamma), torch.empty_like(gamma)
        with _span("disc_bn_bwd"):
            _lib.check(lib.dmc_bn_bwd_act_nhwc(_lib.ptr(z), _lib.ptr(gamma), _lib.ptr(beta), _lib.ptr(stats),
                                               _lib.ptr(scratch), _lib.ptr(dy), _lib.ptr(g), _lib.ptr(dgamma),
                                               _lib.ptr(dbeta), _lib.ptr(keep), oh * ow, 0.2, rows, cout, _stream()),
                       "dmc_bn_bwd_act_nhwc")
        dx = dw = db = None
        want_w = ctx.needs_input_grad[1]
        if first == 2:
            wq = _as_cl(weight)
            mm, _, h, w = x.shape
            if ctx.needs_input_grad[0]:
                dx = torch.empty_like(x)
                with _span("disc_c8_dgrad"):
                    _lib.check(lib.dmc_disc_c8_dgrad(_lib.ptr(g), _lib.ptr(wq), _lib.ptr(dx), mm, h, w, _stream()), "dmc_disc_c8_dgrad")
            if want_w:
                dw = torch.empty(weight.shape, dtype=torch.float32, device=x.device, memory_format=_CL)
                db = torch.empty(cout, dtype=torch.float32, device=x.device) if has_bias else None
                work = _floats(lib.dmc_disc_c8_wgrad_bytes(mm, h, w), x.device)
                with _span("disc_c8_wgrad"):
                    _lib.check(lib.dmc_disc_c8_wgrad(_lib.ptr(x), _lib.ptr(g), _lib.ptr(dw), _lib.ptr(db), _lib.ptr(work), mm, h, w,
                                                     _stream()), "dmc_disc_c8_wgrad")
                dw = _grad_like(dw, weight)
        elif first:
            wq = weight.contiguous()
            mm, _, h, w = x.shape
            if ctx.needs_input_grad[0]:
                dx = torch.empty_like(x)
                with _span("disc_first_dgrad"):
                    _lib.check(lib.dmc_disc_first_dgrad(_lib.ptr(g), _lib.ptr(wq), _lib.ptr(dx), mm, h, w, cout,
                                                        _stream()), "dmc_disc_first_dgrad")
            if want_w:
                dw = torch.empty_like(wq)
                db = torch.empty(cout, dtype=torch.float32, device=x.device) if has_bias else None
                work = _floats(lib.dmc_disc_first_wgrad_bytes(cout), x.device)
                with _span("disc_first_wgrad"):
                    _lib.check(lib.dmc_disc_first_wgrad(_lib.ptr(x), _lib.ptr(g), _lib.ptr(dw), _lib.ptr(db),
                                                        _lib.ptr(work), mm, h, w, cout, _stream()),
                               "dmc_disc_first_wgrad")
                dw = dw.view_as(weight)
        else:
            wq = _as_cl(weight)
            if ctx.needs_input_grad[0]:
                with _span("disc_conv_dgrad"):
                    dx = _conv_dgrad(g, wq, x.shape, stride, 1)
            if want_w:
                with _span("disc_conv_wgrad"):
                    dw = _grad_like(_conv_wgrad(x, g, wq, stride, 1), weight)
                if has_bias:
                    db = torch.empty(cout, dtype=torch.float32, device=x.device)
                    _lib.check(lib.dmc_channel_sum_nhwc(_lib.ptr(g), _lib.ptr(scratch), _lib.ptr(db), rows, cout,
                                                        _stream()), "dmc_channel_sum_nhwc")
        if not want_w:
            db = None
        return dx, dw, db, None, dgamma, dbeta, None, None, None, None, None, None, None


def _disc_c8_supported(x, conv):
    """The 8 -> 16, stride-2 block of Discriminator4 on csrc/disc_c8.hip: fp32 weights and bias on the device, a shape that
    dmc_disc_c8_supported accepts (even H and W)."""
    if conv.in_channels != 8 or conv.out_channels != 16 or conv.stride != (2, 2) or conv.padding_mode != "zeros":
        return False
    if not (conv.weight.is_cuda and conv.weight.dtype == torch.float32):
        return False
    n, cin, h, w = x.shape
    lib = _lib.load()
    return cin == 8 and bool(lib.dmc_disc_c8_supported(n, h, w)) and bool(lib.dmc_bn_act_supported(1, 16))


def disc_block_supported(x, conv, first, c8=False):
    """True if the HIP discriminator-block path handles this convolution (else the stock ops run).  ``c8``: also count the
    8 -> 16 route of csrc/disc_c8.hip (the caller's switch, model.DISC_C8)."""
    if not (x.is_cuda and x.dtype == torch.float32 and x.dim() == 4):
        return False
    if conv.kernel_size != (3, 3) or conv.padding != (1, 1) or conv.dilation != (1, 1) or conv.groups != 1:
        return False
    if first:
        return conv.in_channels == 2 and conv.stride == (2, 2) and \
            bool(_lib.load().dmc_disc_first_supported(conv.out_channels))
    if conv.stride not in ((1, 1), (2, 2)):
        return False
    if c8 and _disc_c8_supported(x, conv):
        return True
    return conv_nhwc_supported(x, conv.weight, conv.stride[0], 1) and \
        bool(_lib.load().dmc_bn_act_supported(1, conv.out_channels))


def disc_block(x, conv, keep, bn, training, first=False, c8=False):
    """x -> BN(keep * LeakyReLU_0.2(conv(x))) (BN optional) through the fused NHWC path.  ``x`` is the
    NCHW 2-channel cue for ``first`` blocks, a channels_last activation otherwise.  ``c8``: the 8 -> 16 block takes
    csrc/disc_c8.hip (as disc_block_supported was asked)."""
    if bn is not None and training and bn.num_batches_tracked is not None:
        bn.num_batches_tracked.add_(1)
    if keep is not None:
        keep = keep.contiguous()
    first = 1 if first else (2 if c8 and _disc_c8_supported(x, conv) else 0)
    if bn is None:
        return _DiscBlock.apply(x, conv.weight, conv.bias, keep, None, None, None, None, conv.stride[0], training,
                                0.0, 0.0, first)
    return _DiscBlock.apply(x, conv.weight, conv.bias, keep, bn.weight, bn.bias, bn.running_mean, bn.running_var,
                            conv.stride[0], training, bn.eps, bn.momentum if bn.momentum is not None else 0.1, first)


class _DiscHead(torch.autograd.Function):
    """adv_layer = Linear(C * H * W -> 2) of a discriminator (code/dmcnet_GAN/model.py:290,297-298) on the channels_last activation
    the blocks leave, csrc/disc_head.hip: the weight stays in the reference's (c, h, w) column order, nothing is permuted or copied.
    The backward produces only what is asked for: with the discriminator's parameters as constants (the G step) it is one
    streaming write of dx."""

    @staticmethod
    def forward(ctx, x, weight, bias):
        lib = _lib.load()
        _need_cuda(x, weight, bias)
        x, weight, bias = _as_cl(x), weight.contiguous(), bias.contiguous()
        m, c, h, w = x.shape
        out = torch.empty((m, 2), dtype=torch.float32, device=x.device)
        with _span("disc_head_fwd"):
            _lib.check(lib.dmc_disc_head_fwd(_lib.ptr(x), _lib.ptr(weight), _lib.ptr(bias), _lib.ptr(out), m, c, h, w, _stream()),
                       "dmc_disc_head_fwd")
        ctx.save_for_backward(x, weight)
        return out

    @staticmethod
    def backward(ctx, dv):
        lib = _lib.load()
        x, weight = ctx.saved_tensors
        m, c, h, w = x.shape
        dv = dv.contiguous()
        want_x, want_w, want_b = ctx.needs_input_grad
        if not (want_x or want_w or want_b):
            return None, None, None
        dx = torch.empty_like(x) if want_x else None
        dw = torch.empty_like(weight) if want_w else None
        db = torch.empty(2, dtype=torch.float32, device=x.device) if want_b else None
        work = _floats(lib.dmc_disc_head_bwd_bytes(m, c, h, w), x.device) if want_w else None
        with _span("disc_head_bwd"):
            _lib.check(lib.dmc_disc_head_bwd(_lib.ptr(x) if want_w else None, _lib.ptr(weight) if want_x else None, _lib.ptr(dv),
                                             _lib.ptr(dx), _lib.ptr(dw), _lib.ptr(db), _lib.ptr(work), m, c, h, w, _stream()),
                       "dmc_disc_head_bwd")
        return dx, dw, db


def disc_head_supported(x, linear):
    """True if ``ops.disc_head`` serves ``linear`` (an nn.Linear(C * H * W, 2) with a bias) on the 4-D activation ``x``: fp32 on the
    GPU, channels_last memory, a shape that dmc_disc_head_supported accepts (C a multiple of 16, fewer than 2^31 elements)."""
    if not (x.is_cuda and x.dtype == torch.float32 and x.dim() == 4 and _is_cl(x)):
        return False
    wt, b = linear.weight, linear.bias
    if b is None or not (wt.is_cuda and wt.dtype == torch.float32 and b.dtype == torch.float32):
        return False
    m, c, h, w = x.shape
    if tuple(wt.shape) != (2, c * h * w) or m == 0:
        return False
    return bool(_lib.load().dmc_disc_head_supported(m, c, h, w))


def disc_head(x, weight, bias):
    """validity [M, 2] = flatten_(c,h,w)(x) @ weight.T + bias for the channels_last activation ``x`` [M, C, H, W]."""
    return _DiscHead.apply(x, weight, bias)


_STD = (0.229, 0.224, 0.225)


def u8_frames_buffer(shape, device):
    """A contiguous uint8 tensor of ``shape`` whose storage has 16 spare bytes behind it (what
    ``prepare_inputs`` wants for its aligned 4-pixel reads): the H2D copy target of a loader."""
    n = 1
    for d in shape:
        n *= int(d)
    return torch.empty(n + 16, dtype=torch.uint8, device=device)[:n].view(tuple(shape))


def check_geometry_plans(boxes, h0, w0, oh, ow):
    """Raise ValueError unless every plan (y0, x0, h, w, rh, rw, cy, cx) crops inside the H0 x W0 frame, resizes to a
    positive size and takes its OH x OW output window inside the resized box."""
    b = boxes.to(torch.int64)
    y0, x0, h, w, rh, rw, cy, cx = (b[:, i] for i in range(8))
    ok = (y0 >= 0) & (x0 >= 0) & (h > 0) & (w > 0) & (y0 + h <= h0) & (x0 + w <= w0) & (rh > 0) & (rw > 0) & \
         (cy >= 0) & (cx >= 0) & (cy + oh <= rh) & (cx + ow <= rw)
    if not bool(ok.all()):
        bad = int((~ok).nonzero()[0])
        raise ValueError("geometry plan %d = %s leaves the %d x %d frame or its resized box (output %d x %d)"
                         % (bad, [int(v) for v in boxes[bad]], h0, w0, oh, ow))


def prepare_inputs(frames_u8, flip=None, flow_ds_factor=0, boxes=None, out_size=None, *, upsample_interp=False, src_index=None):
    """uint8 [N,H0,W0,7] HWC frames (+ optional [N] flip flags, [N,8] int32 geometry plans
    (y0,x0,h,w,rh,rw,cy,cx -- see transforms.geometry_plan) and an output size) on the GPU ->
    (input_flow [N,2,H,W], input_mv [N,2,H,W], input_residual
    [N,3,H,W]) exactly as the reference's loader produces them: crop + bilinear resize
    (code/dmcnet/transforms.py:36-139), flip (:47-58), blockify / normalise
    (code/dmcnet/dataset.py:215-263).  Without ``boxes`` / ``out_size`` the frames are taken whole.

    ``upsample_interp``: with ``flow_ds_factor`` > 0, bring the block means back by the reference's linear interpolation
    (code/dmcnet/dataset.py:236-246) instead of by repetition -- ``CoviarDataSet(..., upsample_interp=True)``'s flow, bit for
    bit; needs at least two blocks on each axis (scipy refuses one, so does this).  ``src_index`` [N_out] int32: output ``n`` is
    computed from frame ``src_index[n]``; ``flip`` and ``boxes`` then have N_out entries (the ten crops of
    ``transforms.GroupOverSample`` are ten plans over one uploaded frame).  Host-side ``src_index`` / ``boxes`` are range-checked;
    device-resident ones are the caller's responsibility.  With both at their defaults this is ``dmc_prepare_inputs_crop``."""
    import ctypes
    lib = _lib.load()
    if not frames_u8.is_cuda or frames_u8.dtype != torch.uint8 or frames_u8.dim() != 4 \
            or frames_u8.shape[-1] != 7:
        raise _lib.DmcHipError("prepare_inputs expects a CUDA uint8 tensor [N,H,W,7]")
    n_src, h0, w0, _ = frames_u8.shape
    dev = frames_u8.device
    oh, ow = (h0, w0) if out_size is None else (int(out_size[0]), int(out_size[1]))
    views = bool(upsample_interp) or src_index is not None
    n = n_src
    if src_index is not None:
        if src_index.dim() != 1 or src_index.numel() == 0:
            raise ValueError("src_index must be a non-empty [N_out] tensor")
        n = int(src_index.numel())
        if not src_index.is_cuda and not bool(((src_index >= 0) & (src_index < n_src)).all()):
            raise ValueError("src_index names a frame outside 0 .. %d" % (n_src - 1))
        src_index = src_index.to(dev, torch.int32).contiguous()
    if upsample_interp:
        f = int(flow_ds_factor)
        if f <= 0:
            raise ValueError("upsample_interp needs flow_ds_factor > 0")
        if -(-oh // f) < 2 or -(-ow // f) < 2:
            raise ValueError("upsample_interp needs at least two %d x %d blocks on each axis of the %d x %d output" % (f, f, oh, ow))
    if flip is not None and views and flip.numel() != n:
        raise ValueError("flip must have one entry per output (%d)" % n)
    # the 4-pixel path reads whole aligned dwords: it needs 16 spare bytes behind the last frame.
    # ``u8_frames_buffer`` allocates such tensors; anything else is copied once into one.
    spare = frames_u8.untyped_storage().nbytes() - frames_u8.storage_offset() - frames_u8.numel()
    if frames_u8.is_contiguous() and spare >= 16:
        padded = frames_u8
    else:
        padded = u8_frames_buffer(frames_u8.shape, dev)
        padded.copy_(frames_u8)
    if flip is not None:
        flip = flip.to(dev, torch.uint8).contiguous()
    if boxes is not None:
        if tuple(boxes.shape) != (n, 8):
            raise ValueError("boxes must be [N,8] (y0, x0, h, w, rh, rw, cy, cx)")
        if not boxes.is_cuda:
            # the kernel indexes the frames with these numbers and cannot truncate the way numpy slicing does: a plan that
            # leaves the frame or the resized box is refused while it is still a host tensor (plans already on the device
            # are the caller's responsibility: checking them would cost a synchronisation per batch)
            check_geometry_plans(boxes, h0, w0, oh, ow)
        boxes = boxes.to(dev, torch.int32).contiguous()
    elif (oh, ow) != (h0, w0):
        boxes = torch.tensor([[0, 0, h0, w0, oh, ow, 0, 0]] * n, dtype=torch.int32, device=dev)
    flow = torch.empty((n, 2, oh, ow), dtype=torch.float32, device=dev)
    mv = torch.empty((n, 2, oh, ow), dtype=torch.float32, device=dev)
    res = torch.empty((n, 3, oh, ow), dtype=torch.float32, device=dev)
    std = torch.tensor(_STD, dtype=torch.float64).float()
    std4 = (ctypes.c_float * 4)(float(torch.mean(std)), float(std[0]), float(std[1]), float(std[2]))
    if views:
        work = _floats(lib.dmc_prepare_views_workspace_bytes(n, oh, ow, int(flow_ds_factor), int(bool(upsample_interp))), dev)
        with _span("prepare_inputs"):
            _lib.check(lib.dmc_prepare_inputs_views(_lib.ptr(padded), _lib.ptr(src_index), _lib.ptr(boxes), _lib.ptr(flip),
                                                    _lib.ptr(flow), _lib.ptr(mv), _lib.ptr(res), _lib.ptr(work), n_src, n, h0, w0,
                                                    oh, ow, int(flow_ds_factor), int(bool(upsample_interp)),
                                                    ctypes.cast(std4, ctypes.c_void_p), _stream()), "dmc_prepare_inputs_views")
        return flow, mv, res
    work = _floats(lib.dmc_prepare_crop_workspace_bytes(n, oh, ow, int(flow_ds_factor)), dev)
    with _span("prepare_inputs"):
        _lib.check(lib.dmc_prepare_inputs_crop(_lib.ptr(padded), _lib.ptr(boxes), _lib.ptr(flip), _lib.ptr(flow),
                                               _lib.ptr(mv), _lib.ptr(res), _lib.ptr(work), n, h0, w0, oh, ow,
                                               int(flow_ds_factor), ctypes.cast(std4, ctypes.c_void_p),
                                               _stream()), "dmc_prepare_inputs_crop")
    return flow, mv, res


_CLIP_MEAN = (0.485, 0.456, 0.406)


def check_clip_plans(plans, h0, w0, oh, ow):
    """Raise ValueError unless every clip plan (y1, x1, flip) takes its OH x OW window inside the H0 x W0 clip."""
    p = plans.to(torch.int64)
    ok = (p[:, 0] >= 0) & (p[:, 1] >= 0) & (p[:, 0] + oh <= h0) & (p[:, 1] + ow <= w0)
    if not bool(ok.all()):
        bad = int((~ok).nonzero()[0])
        raise ValueError("clip plan %d = %s leaves the %d x %d clip (output %d x %d)"
                         % (bad, [int(v) for v in plans[bad]], h0, w0, oh, ow))


def prepare_clip(clips_u8, plans, out_size, flow_ds_factor=0, mean=_CLIP_MEAN, std=_STD, out=None):
    """uint8 clips [B,H0,W0,T*7] as decoded (frame t = channels 7t .. 7t+6 = flow_x flow_y mv_x mv_y res0 res1 res2) and
    [B,3] int32 plans (y1, x1, flip) -> the fp32 batch [B,7,T,OH,OW] of the reference's I3D loader for modality 'flow+mp4',
    bit for bit: crop, flip (flow_x / mv_x -> 256 - v as uint8), ToTensor with the truncated f x f flow block means, / 255,
    and Normalize over the first ``len(mean)`` channels only (code/dmcnet_I3D/data/image_transforms.py:47-59,138-200,
    video_transforms.py:23-70) -- ``dmc_prepare_clip``; see ``i3d_data.ClipTransform`` for the same chain on the CPU.

    ``flow_ds_factor`` 0 or 1: no blockify.  ``plans`` on the host are range-checked (``check_clip_plans``); plans already on
    the device are the caller's responsibility.  ``out``: a contiguous fp32 [B,7,T,OH,OW] CUDA tensor to write into (it is
    returned), e.g. the hipGraph input buffer ``I3DTrainer.static_batch()[0]``."""
    import ctypes
    lib = _lib.load()
    if not clips_u8.is_cuda or clips_u8.dtype != torch.uint8 or clips_u8.dim() != 4 or clips_u8.shape[-1] % 7 \
            or clips_u8.shape[-1] == 0:
        raise _lib.DmcHipError("prepare_clip expects a CUDA uint8 tensor [B,H0,W0,T*7]")
    b, h0, w0, t7 = (int(v) for v in clips_u8.shape)
    t = t7 // 7
    dev = clips_u8.device
    oh, ow = int(out_size[0]), int(out_size[1])
    if oh <= 0 or ow <= 0 or oh > h0 or ow > w0:
        raise ValueError("prepare_clip: output %d x %d does not fit the %d x %d clip" % (oh, ow, h0, w0))
    if int(flow_ds_factor) < 0:
        raise ValueError("prepare_clip: negative flow_ds_factor")
    mean, std = [float(v) for v in mean], [float(v) for v in std]
    if len(mean) != len(std) or len(mean) > 7:
        raise ValueError("prepare_clip: mean and std need the same number of entries, at most 7")
    if tuple(plans.shape) != (b, 3):
        raise ValueError("plans must be [B,3] (y1, x1, flip)")
    if not plans.is_cuda:
        check_clip_plans(plans, h0, w0, oh, ow)
    plans = plans.to(dev, torch.int32).contiguous()
    spare = clips_u8.untyped_storage().nbytes() - clips_u8.storage_offset() - clips_u8.numel()
    if clips_u8.is_contiguous() and spare >= 16 and clips_u8.data_ptr() % 4 == 0:
        padded = clips_u8
    else:
        padded = u8_frames_buffer(clips_u8.shape, dev)
        padded.copy_(clips_u8)
    if out is None:
        out = torch.empty((b, 7, t, oh, ow), dtype=torch.float32, device=dev)
    elif not out.is_cuda or out.dtype != torch.float32 or tuple(out.shape) != (b, 7, t, oh, ow) or not out.is_contiguous() \
            or out.device != dev:
        raise ValueError("prepare_clip: out must be a contiguous fp32 CUDA tensor %s on %s" % ((b, 7, t, oh, ow), dev))
    n = len(mean)
    mean_c, std_c = (ctypes.c_float * max(n, 1))(*mean), (ctypes.c_float * max(n, 1))(*std)
    nbytes = lib.dmc_prepare_clip_workspace_bytes(b, t, oh, ow, int(flow_ds_factor))
    work = _floats(nbytes, dev) if nbytes else None
    with _span("prepare_clip"):
        _lib.check(lib.dmc_prepare_clip(_lib.ptr(padded), _lib.ptr(plans), _lib.ptr(out), _lib.ptr(work), b, t, h0, w0, oh, ow,
                                        int(flow_ds_factor), n, ctypes.cast(mean_c, ctypes.c_void_p),
                                        ctypes.cast(std_c, ctypes.c_void_p), _stream()), "dmc_prepare_clip")
    return out


# ------------------------------------------------------------------ I3D trunk: bf16 Conv3d (conv3d_bf16.hip)
_CL3 = torch.channels_last_3d


def _as_cl3(t, dtype=torch.bfloat16):
    if t.dtype != dtype:
        t = t.to(dtype)
    return t if t.is_contiguous(memory_format=_CL3) else t.contiguous(memory_format=_CL3)


def conv3d_bf16_supported(x, weight, stride=(1, 1, 1), padding=None):
    """True if ``conv3d(x, weight)`` (bf16 ``x`` [N,Cin,D,H,W], fp32 ``weight``, stride 1, padding k // 2, kernel
    extents 1 or 3, channels multiples of 8) can run on the HIP implicit-GEMM kernels; the weight gradient
    additionally needs a 1x1x1 or 3x3x3 kernel."""
    if not (x.is_cuda and x.dim() == 5 and x.dtype == torch.bfloat16 and weight.dtype == torch.float32):
        return False
    if tuple(stride) != (1, 1, 1) or x.shape[1] != weight.shape[1]:
        return False
    kd, kh, kw = weight.shape[2:]
    if padding is not None and tuple(padding) != (kd // 2, kh // 2, kw // 2):
        return False
    if not ((kd, kh, kw) == (1, 1, 1) or (kd, kh, kw) == (3, 3, 3)):
        return False
    n, cin, d, h, w = x.shape
    return bool(_lib.load().dmc_conv3d_bf16_supported(n, d, h, w, cin, weight.shape[0], kd, kh, kw))


class _Conv3dBf16(torch.autograd.Function):
    """nn.Conv3d(bias=False, stride 1, TF-"SAME") of the I3D trunk's Unit3Dpy
    (code/dmcnet_I3D/network/i3d.py:372-393) on the bf16 matrix cores: bf16 NDHWC activations, fp32 master
    weights rounded to bf16 per call, fp32 accumulation; deterministic weight gradient in fp32."""

    @staticmethod
    def forward(ctx, x, weight):
        lib = _lib.load()
        if not (x.is_cuda and weight.is_cuda):
            raise _lib.DmcHipError("conv3d_bf16 runs on the HIP extension only (no CPU fallback)")
        ctx.x_was_cl3 = x.is_contiguous(memory_format=_CL3)
        x = _as_cl3(x)
        wc = weight.detach().contiguous()
        n, cin, d, h, w = x.shape
        cout, _, kd, kh, kw = wc.shape
        t = kd * kh * kw
        y = torch.empty((n, cout, d, h, w), dtype=torch.bfloat16, device=x.device, memory_format=_CL3)
        wpack = _floats(lib.dmc_conv3d_bf16_wpack_bytes(cin, cout, kd, kh, kw), x.device)
        with _span("conv3d_bf16_fwd"):
            _lib.check(lib.dmc_conv3d_bf16_fwd(_lib.ptr(x), _lib.ptr(wc), cin * t, t, 1, _lib.ptr(wpack), _lib.ptr(y),
                                               None, n, d, h, w, cin, cout, kd, kh, kw, _stream()),
                       "dmc_conv3d_bf16_fwd")
        ctx.save_for_backward(x, weight)
        return y

    @staticmethod
    def backward(ctx, dy, _dstat=None):
        lib = _lib.load()
        x, weight = ctx.saved_tensors
        dy = _as_cl3(dy)
        wc = weight.detach().contiguous()
        n, cin, d, h, w = x.shape
        cout, _, kd, kh, kw = wc.shape
        t = kd * kh * kw
        dx = dw = None
        if ctx.needs_input_grad[0]:
            dx = torch.empty_like(x)
            wpack = _floats(lib.dmc_conv3d_bf16_wpack_bytes(cin, cout, kd, kh, kw), x.device)
            with _span("conv3d_bf16_dgrad"):
                _lib.check(lib.dmc_conv3d_bf16_dgrad(_lib.ptr(dy), _lib.ptr(wc), cin * t, t, 1, _lib.ptr(wpack),
                                                     _lib.ptr(dx), n, d, h, w, cin, cout, kd, kh, kw, _stream()),
                           "dmc_conv3d_bf16_dgrad")
            if not ctx.x_was_cl3:          # hand the gradient back in the producer's layout (a stock op's backward --
                dx = dx.contiguous()       # e.g. MIOpen's stem convolution -- then sees the problem it saw in the forward)
        if ctx.needs_input_grad[1]:
            dw = torch.empty_like(wc)
            work = _floats(lib.dmc_conv3d_bf16_wgrad_bytes(n, d, h, w, cin, cout, kd, kh, kw), x.device)
            with _span("conv3d_bf16_wgrad"):
                _lib.check(lib.dmc_conv3d_bf16_wgrad(_lib.ptr(x), _lib.ptr(dy), _lib.ptr(dw), _lib.ptr(work), n, d, h, w,
                                                     cin, cout, kd, kh, kw, _stream()), "dmc_conv3d_bf16_wgrad")
            dw = dw.view_as(weight)
        return dx, dw


def conv3d_bf16(x, weight):
    """conv3d(x, weight, None, 1, k // 2) for a bf16 ``x`` (see conv3d_bf16_supported); returns a bf16
    channels_last_3d tensor."""
    return _Conv3dBf16.apply(x, weight)


def maxpool3d_tf_supported(x, kernel, stride):
    """True if MaxPool3dTFPadding(kernel, stride)(x) can run on the HIP kernels (bf16 CUDA [N,C,D,H,W], C % 8 == 0)."""
    if not (x.is_cuda and x.dim() == 5 and x.dtype == torch.bfloat16):
        return False
    n, c, d, h, w = x.shape
    return bool(_lib.load().dmc_maxpool3d_tf_out_shape(d, h, w, c, *[int(k) for k in kernel], *[int(s) for s in stride],
                                                       None, None, None))


class _MaxPool3dTF(torch.autograd.Function):
    """MaxPool3dTFPadding (code/dmcnet_I3D/network/i3d.py:406-418) on bf16 NDHWC tensors: zero padding to the
    TF-"SAME" extent and MaxPool3d(ceil_mode=True) in one pass; the backward gathers from the stored winning taps."""

    @staticmethod
    def forward(ctx, x, kernel, stride):
        import ctypes
        lib = _lib.load()
        if not (x.is_cuda and x.dtype == torch.bfloat16):
            raise _lib.DmcHipError("maxpool3d_tf runs on the HIP extension only: bf16 CUDA tensors (no CPU fallback)")
        ctx.x_was_cl3 = x.is_contiguous(memory_format=_CL3)
        x = _as_cl3(x)
        n, c, d, h, w = x.shape
        od, oh, ow = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
        if not lib.dmc_maxpool3d_tf_out_shape(d, h, w, c, *kernel, *stride, ctypes.byref(od), ctypes.byref(oh), ctypes.byref(ow)):
            raise _lib.DmcHipError("maxpool3d_tf: unsupported shape %s kernel %s stride %s" % (tuple(x.shape), kernel, stride))
        y = torch.empty((n, c, od.value, oh.value, ow.value), dtype=torch.bfloat16, device=x.device, memory_format=_CL3)
        code = torch.empty(y.numel(), dtype=torch.uint8, device=x.device)
        with _span("maxpool3d_fwd"):
            _lib.check(lib.dmc_maxpool3d_tf_bf16_fwd(_lib.ptr(x), _lib.ptr(y), _lib.ptr(code), n, d, h, w, c, *kernel, *stride,
                                                     _stream()), "dmc_maxpool3d_tf_bf16_fwd")
        ctx.save_for_backward(code)
        ctx.geom = (tuple(x.shape), kernel, stride)
        return y

    @staticmethod
    def backward(ctx, dy):
        lib = _lib.load()
        (code,) = ctx.saved_tensors
        (n, c, d, h, w), kernel, stride = ctx.geom
        dy = _as_cl3(dy)
        dx = torch.empty((n, c, d, h, w), dtype=torch.bfloat16, device=dy.device, memory_format=_CL3)
        with _span("maxpool3d_bwd"):
            _lib.check(lib.dmc_maxpool3d_tf_bf16_bwd(_lib.ptr(dy), _lib.ptr(code), _lib.ptr(dx), n, d, h, w, c, *kernel, *stride,
                                                     _stream()), "dmc_maxpool3d_tf_bf16_bwd")
        if not ctx.x_was_cl3:
            dx = dx.contiguous()
        return dx, None, None


def maxpool3d_tf(x, kernel, stride):
    """MaxPool3dTFPadding(kernel, stride)(x) for a bf16 ``x`` (see maxpool3d_tf_supported); channels_last_3d result."""
    return _MaxPool3dTF.apply(x, tuple(int(k) for k in kernel), tuple(int(s) for s in stride))


#: weight gradients of the I3D trunk's serial units on the side stream (DMC_UNIT3D_WGRAD_SIDE=0: inside the unit's one call)
UNIT3D_WGRAD_SIDE = __import__("os").environ.get("DMC_UNIT3D_WGRAD_SIDE", "1") != "0"
UNIT3D_WGRAD_SIDE_MINW = int(__import__("os").environ.get("DMC_UNIT3D_WGRAD_SIDE_MINW", "56"))


class _ConvBnRelu3d(torch.autograd.Function):
    """relu?(BatchNorm3d(conv3d(x, w))) of a Unit3Dpy in training mode (code/dmcnet_I3D/network/i3d.py:390-398) on the
    bf16 kernels: the convolution's epilogue reduces the batch statistics, one streaming pass normalises and rectifies;
    the backward runs the ReLU + BatchNorm backward in two passes and feeds the data / weight gradient kernels."""

    @staticmethod
    def forward(ctx, x, weight, gamma, beta, running_mean, running_var, eps, momentum, relu, into=None):
        lib = _lib.load()
        if not (x.is_cuda and weight.is_cuda):
            raise _lib.DmcHipError("conv_bn_relu3d runs on the HIP extension only (no CPU fallback)")
        ctx.x_was_cl3 = x.is_contiguous(memory_format=_CL3)
        x = _as_cl3(x)
        wc = weight.detach()
        if not wc.is_contiguous():
            wc = wc.contiguous()
        n, cin, d, h, w = x.shape
        cout, _, kd, kh, kw = wc.shape
        geom = (n, d, h, w, cin, cout, kd, kh, kw)
        # ONE foreign call (pack + convolution with the statistics in its epilogue + BatchNorm / ReLU pass) and one
        # workspace: the trunk is bound by the host that issues its ~940 launches per micro-step (csrc/unit3d.hip)
        y = torch.empty((n, cout, d, h, w), dtype=torch.bfloat16, device=x.device, memory_format=_CL3)
        # `into`: a channel slice of a wider NDHWC tensor (an Inception block's output) that receives the result in place --
        # the block then needs no torch.cat; autograd sees a view of it as this op's output (the buffer itself has no history)
        if into is not None:
            ld = into.stride(4)
            if not (into.dtype == torch.bfloat16 and tuple(into.shape) == (n, cout, d, h, w) and ld >= cout and ld % 8 == 0
                    and into.storage_offset() % 8 == 0 and into.stride() == (d * h * w * ld, 1, h * w * ld, w * ld, ld)):
                raise ValueError("conv_bn_relu3d: `into` must be a channel slice of a channels_last_3d bf16 tensor of this op's shape")
            out = into
        else:
            out, ld = torch.empty_like(y), cout
        ws = torch.empty(lib.dmc_unit3d_bf16_fwd_workspace_bytes(*geom), dtype=torch.uint8, device=x.device)
        with _span("conv3d_bf16_fwd"):
            _lib.check(lib.dmc_unit3d_bf16_fwd_into(_lib.ptr(x), _lib.ptr(wc), _lib.ptr(gamma), _lib.ptr(beta), _lib.ptr(running_mean),
                                                    _lib.ptr(running_var), _lib.ptr(ws), _lib.ptr(y), _lib.ptr(out), ld, *geom, int(relu),
                                                    float(eps), float(momentum), _stream()), "dmc_unit3d_bf16_fwd_into")
        ctx.save_for_backward(x, weight, y, gamma, beta, ws)
        ctx.relu, ctx.geom = bool(relu), geom
        return out

    @staticmethod
    def backward(ctx, dout):
        lib = _lib.load()
        x, weight, y, gamma, beta, ws = ctx.saved_tensors
        geom = ctx.geom
        n, d, h, w, cin, cout, kd, kh, kw = geom
        # a channel slice of a concatenated (Inception) gradient is read in place: NDHWC memory with a wider pixel stride
        ld = dout.stride(4) if dout.dim() == 5 else 0
        if not (dout.dtype == torch.bfloat16 and ld >= cout and ld % 8 == 0 and dout.storage_offset() % 8 == 0
                and dout.stride() == (d * h * w * ld, 1, h * w * ld, w * ld, ld)):
            dout, ld = _as_cl3(dout), cout
        dy = torch.empty_like(y)
        dgamma, dbeta = torch.empty_like(gamma), torch.empty_like(gamma)
        dx = torch.empty_like(x) if ctx.needs_input_grad[0] else None
        # the weight gradient on the side stream (see _on_wgrad_stream) for the units of the trunk's SERIAL part (the stem's
        # successors, 56-wide maps): their input gradient heads a dependent chain, nothing reads dw.  Inside the Inception
        # blocks the branches already overlap on their own streams.
        side = ctx.needs_input_grad[1] and UNIT3D_WGRAD_SIDE and w >= UNIT3D_WGRAD_SIDE_MINW and WGRAD_STREAM and _WGRAD_SCOPE[0] > 0
        dw = torch.empty(weight.shape, dtype=torch.float32, device=x.device) if ctx.needs_input_grad[1] and not side else None
        bws = torch.empty(lib.dmc_unit3d_bf16_bwd_workspace_bytes(*geom), dtype=torch.uint8, device=x.device)
        with _span("conv3d_bf16_bwd"):
            _lib.check(lib.dmc_unit3d_bf16_bwd(_lib.ptr(dout), ld, _lib.ptr(x), _lib.ptr(y), _lib.ptr(ws), _lib.ptr(gamma),
                                               _lib.ptr(beta), _lib.ptr(bws), _lib.ptr(dy), _lib.ptr(dx), _lib.ptr(dw),
                                               _lib.ptr(dgamma), _lib.ptr(dbeta), *geom, int(ctx.relu), _stream()),
                       "dmc_unit3d_bf16_bwd")
        if side:
            def launch():
                dw_ = torch.empty(weight.shape, dtype=torch.float32, device=x.device)
                work_ = torch.empty(lib.dmc_conv3d_bf16_wgrad_bytes(*geom), dtype=torch.uint8, device=x.device)
                _lib.check(lib.dmc_conv3d_bf16_wgrad(_lib.ptr(x), _lib.ptr(dy), _lib.ptr(dw_), _lib.ptr(work_), *geom, _stream()),
                           "dmc_conv3d_bf16_wgrad")
                return dw_
            with _span("conv3d_bf16_wgrad"):
                dw = _on_wgrad_stream(weight, (x, dy), launch)
        if dx is not None and not ctx.x_was_cl3:
            dx = dx.contiguous()
        return dx, dw, dgamma, dbeta, None, None, None, None, None, None


def conv_bn_relu3d_supported(x, conv, bn):
    """True if conv -> BatchNorm3d (training) [-> ReLU] of a Unit3Dpy can run as the fused bf16 op."""
    if not (torch.is_grad_enabled() and bn.training and bn.track_running_stats and bn.affine and bn.momentum is not None):
        return False
    if bn.weight.dtype != torch.float32 or not conv3d_bf16_supported(x, conv.weight, conv.stride, conv.padding):
        return False
    n, _, d, h, w = x.shape
    return bool(_lib.load().dmc_bn3d_bf16_supported(n * d * h * w, conv.out_channels))


def conv_bn_relu3d(x, conv, bn, relu=True, into=None):
    """relu?(bn(conv(x))) for a bf16 ``x`` (see conv_bn_relu3d_supported); updates the running statistics and
    ``num_batches_tracked`` as nn.BatchNorm3d does.  ``into``: see _ConvBnRelu3d.forward."""
    if bn.num_batches_tracked is not None:
        if _PENDING_COUNTERS is not None:
            _PENDING_COUNTERS.append(bn.num_batches_tracked)
        else:
            bn.num_batches_tracked.add_(1)
    return _ConvBnRelu3d.apply(x, conv.weight, bn.weight, bn.bias, bn.running_mean, bn.running_var, bn.eps, bn.momentum,
                               bool(relu), into)


class _JoinSlices(torch.autograd.Function):
    """The concatenation that already happened: ``parts`` are channel slices of ``buf`` that their producers wrote in place
    (conv_bn_relu3d(..., into=...)).  Forward hands out ``buf``; backward hands each producer its slice of the gradient -- what
    torch.cat's backward does, without the forward copies."""

    @staticmethod
    def forward(ctx, buf, *parts):
        ctx.widths = [p.shape[1] for p in parts]
        return buf.view(buf.shape)

    @staticmethod
    def backward(ctx, g):
        outs, c = [], 0
        for wd in ctx.widths:
            outs.append(g[:, c:c + wd])
            c += wd
        return (None,) + tuple(outs)


def join_slices(buf, parts):
    return _JoinSlices.apply(buf, *parts)


class _Fanout4(torch.autograd.Function):
    """x handed to four consumers; backward adds their four gradients in ONE pass (dmc_add4_bf16) instead of the engine's three
    additions -- in the engine's order (the consumer created last delivers first) and with its bf16 rounding after every sum, so
    the result is bit for bit the engine's."""

    @staticmethod
    def forward(ctx, x):
        return tuple(x.view(x.shape) for _ in range(4))

    @staticmethod
    def backward(ctx, g0, g1, g2, g3):
        gs = [g for g in (g3, g2, g1, g0) if g is not None]
        if (len(gs) == 4 and all(g.is_cuda and g.dtype == torch.bfloat16 and g.shape == gs[0].shape and g.stride() == gs[0].stride()
                                 and g.storage_offset() % 8 == 0 for g in gs)
                and gs[0].numel() % 8 == 0 and (gs[0].is_contiguous() or gs[0].is_contiguous(memory_format=_CL3))):
            out = torch.empty_like(gs[0])
            _lib.check(_lib.load().dmc_add4_bf16(_lib.ptr(gs[0]), _lib.ptr(gs[1]), _lib.ptr(gs[2]), _lib.ptr(gs[3]), _lib.ptr(out),
                                                 out.numel(), _stream()), "dmc_add4_bf16")
            return out
        r = None
        for g in gs:
            r = g if r is None else r + g
        return r


def fanout4(x):
    return _Fanout4.apply(x)


class _Stem3dBnRelu(torch.autograd.Function):
    """relu(BatchNorm3d(conv3d_1a_7x7(x))) of the I3D stem in a bf16 trunk (code/dmcnet_I3D/network/i3d.py:480-481,
    :390-398): forward on dmc_stem3d_bf16_fwd (statistics in its epilogue) + the fused BatchNorm3d / ReLU pass; the
    BatchNorm / ReLU backward on bn3d_bf16.hip, the weight gradient on dmc_stem3d_bf16_wgrad, the 2-channel data gradient on
    dmc_stem3d_bf16_dgrad (PyTorch-ROCm / MIOpen only for frames wider than 256)."""

    @staticmethod
    def forward(ctx, x, weight, gamma, beta, running_mean, running_var, eps, momentum, relu):
        lib = _lib.load()
        if not (x.is_cuda and weight.is_cuda):
            raise _lib.DmcHipError("stem3d runs on the HIP extension only (no CPU fallback)")
        xc = x.detach().float().contiguous()
        wc = weight.detach().float().contiguous()
        n, _, t, h, w = xc.shape
        od, oh, ow = (t - 2) // 2 + 1, (h - 2) // 2 + 1, (w - 2) // 2 + 1
        y = torch.empty((n, 64, od, oh, ow), dtype=torch.bfloat16, device=x.device, memory_format=_CL3)
        work = _floats(lib.dmc_stem3d_bf16_workspace_bytes(n, t, h, w), x.device)
        nblk = lib.dmc_stem3d_bf16_stat_blocks(n, t, h, w)
        part = torch.empty((nblk, 64, 2), dtype=torch.float32, device=x.device)
        with _span("stem3d_fwd"):
            _lib.check(lib.dmc_stem3d_bf16_fwd(_lib.ptr(xc), _lib.ptr(wc), _lib.ptr(work), _lib.ptr(y), _lib.ptr(part), n, t, h, w,
                                               _stream()), "dmc_stem3d_bf16_fwd")
        stats = torch.empty(128, dtype=torch.float32, device=x.device)
        out = torch.empty_like(y)
        m = n * od * oh * ow
        with _span("bn3d_fwd"):
            _lib.check(lib.dmc_bn3d_bf16_fwd(_lib.ptr(y), _lib.ptr(part), nblk, _lib.ptr(gamma), _lib.ptr(beta), _lib.ptr(stats),
                                             _lib.ptr(running_mean), _lib.ptr(running_var), _lib.ptr(out), m, 64, int(relu),
                                             float(eps), float(momentum), _stream()), "dmc_bn3d_bf16_fwd")
        ctx.save_for_backward(xc, weight, y, gamma, beta, stats)
        ctx.relu = bool(relu)
        return out

    @staticmethod
    def backward(ctx, dout):
        lib = _lib.load()
        xc, weight, y, gamma, beta, stats = ctx.saved_tensors
        n, _, od, oh, ow = y.shape
        m = n * od * oh * ow
        dout = _as_cl3(dout)
        dy = torch.empty_like(y)
        dgamma, dbeta = torch.empty_like(gamma), torch.empty_like(gamma)
        scratch = _floats(lib.dmc_bn3d_bf16_scratch_bytes(64), y.device)
        with _span("bn3d_bwd"):
            _lib.check(lib.dmc_bn3d_bf16_bwd(_lib.ptr(dout), 64, _lib.ptr(y), _lib.ptr(stats), _lib.ptr(gamma), _lib.ptr(beta),
                                             _lib.ptr(scratch), _lib.ptr(dy), _lib.ptr(dgamma), _lib.ptr(dbeta), m, 64,
                                             int(ctx.relu), _stream()), "dmc_bn3d_bf16_bwd")
        t, h, w = xc.shape[2:]
        dx = dw = None
        if ctx.needs_input_grad[1]:
            def launch():       # nothing below reads dw: on the side stream it runs next to the data gradient and the generator's backward
                dw_ = torch.empty((64, 2, 7, 7, 7), dtype=torch.float32, device=y.device)
                work_ = _floats(lib.dmc_stem3d_bf16_wgrad_workspace_bytes(n, t, h, w), y.device)
                _lib.check(lib.dmc_stem3d_bf16_wgrad(_lib.ptr(xc), _lib.ptr(dy), _lib.ptr(dw_), _lib.ptr(work_), n, t, h, w, _stream()),
                           "dmc_stem3d_bf16_wgrad")
                return dw_.to(weight.dtype)
            with _span("stem3d_wgrad"):
                dw = _on_wgrad_stream(weight, (xc, dy), launch)
        if ctx.needs_input_grad[0] and w <= 256:           # data gradient (2 channels): row GEMM + fold on the matrix cores
            dx = torch.empty((n, 2, t, h, w), dtype=torch.float32, device=y.device)
            work = _floats(lib.dmc_stem3d_bf16_dgrad_workspace_bytes(), y.device)
            with _span("stem3d_dgrad"):
                _lib.check(lib.dmc_stem3d_bf16_dgrad(_lib.ptr(dy), _lib.ptr(weight.detach().float().contiguous()), _lib.ptr(dx),
                                                     _lib.ptr(work), n, t, h, w, _stream()), "dmc_stem3d_bf16_dgrad")
        elif ctx.needs_input_grad[0]:                      # wider than the kernel's row tile: MIOpen, on the stock path's tensors
            xpad = torch.nn.functional.pad(xc.bfloat16(), (2, 3, 2, 3, 2, 3))
            with _span("stem3d_dgrad"):
                dxp, _, _ = torch.ops.aten.convolution_backward(
                    dy.contiguous(), xpad, weight.detach().bfloat16(), None, (2, 2, 2), (0, 0, 0), (1, 1, 1), False, (0, 0, 0), 1,
                    (True, False, False))
            dx = dxp[:, :, 2:2 + t, 2:2 + h, 2:2 + w].float()
        return dx, dw, dgamma, dbeta, None, None, None, None, None


def stem3d_supported(x, conv, bn):
    """True if the I3D stem unit (2 -> 64 channels, 7x7x7, stride 2, TF-"SAME") can take the bf16 HIP forward: a CUDA
    fp32 / bf16 cue inside a bf16 autocast region, BatchNorm3d in training mode."""
    if not (x.is_cuda and x.dim() == 5 and x.shape[1] == 2 and torch.is_autocast_enabled()
            and torch.get_autocast_dtype("cuda") == torch.bfloat16):
        return False
    if tuple(conv.weight.shape) != (64, 2, 7, 7, 7) or tuple(conv.stride) != (2, 2, 2) or conv.bias is not None:
        return False
    if not (torch.is_grad_enabled() and bn.training and bn.track_running_stats and bn.affine and bn.momentum is not None):
        return False
    return all(int(s) >= 2 and int(s) % 2 == 0 for s in x.shape[2:])


def stem3d_bn_relu(x, conv, bn, relu=True):
    if bn.num_batches_tracked is not None:
        if _PENDING_COUNTERS is not None:
            _PENDING_COUNTERS.append(bn.num_batches_tracked)
        else:
            bn.num_batches_tracked.add_(1)
    return _Stem3dBnRelu.apply(x, conv.weight, bn.weight, bn.bias, bn.running_mean, bn.running_var, bn.eps, bn.momentum,
                               bool(relu))


# ---- eval mode of the I3D trunk: BatchNorm3d with RUNNING statistics in the convolution epilogue (forward only) ----

def _bn_eval_ok(bn):
    """BatchNorm3d in eval mode with running statistics and affine fp32 parameters, no autograd (the eval entries are forward-only)."""
    return (not torch.is_grad_enabled() and not bn.training and bn.track_running_stats and bn.affine and bn.running_mean is not None
            and bn.weight.dtype == torch.float32 and bn.running_mean.dtype == torch.float32 and bn.running_var.dtype == torch.float32)


def conv_bn_relu3d_eval_supported(x, conv, bn):
    """True if conv -> BatchNorm3d (eval: running statistics) [-> ReLU] of a Unit3Dpy can run forward-only as ONE convolution
    launch with the normalisation in its epilogue (code/dmcnet_I3D/network/i3d.py:390-398 under net.eval() + no_grad)."""
    if not _bn_eval_ok(bn) or conv.bias is not None:
        return False
    return conv3d_bf16_supported(x, conv.weight, conv.stride, conv.padding)


def conv_bn_relu3d_eval(x, conv, bn, relu=True, into=None):
    """Forward-only relu?(bn(conv(x))) with the BatchNorm's running statistics (see conv_bn_relu3d_eval_supported): the training
    op's convolution kernels on the same bf16-rounded weights, the BatchNorm as a per-channel affine map in their epilogue
    (dmc_unit3d_bf16_fwd_eval) -- one read of x, one write of the result, one bf16 rounding; the running buffers are read, not
    updated.  ``into``: a channel slice of a wider channels_last_3d bf16 tensor (an Inception block's output) that receives the
    result in place; returns it (or a new channels_last_3d bf16 tensor)."""
    lib = _lib.load()
    if not (x.is_cuda and conv.weight.is_cuda and bn.running_mean.is_cuda):
        raise _lib.DmcHipError("conv_bn_relu3d_eval runs on the HIP extension only (no CPU fallback)")
    x = _as_cl3(x)
    wc = conv.weight.detach()
    if not wc.is_contiguous():
        wc = wc.contiguous()
    n, cin, d, h, w = x.shape
    cout, _, kd, kh, kw = wc.shape
    geom = (n, d, h, w, cin, cout, kd, kh, kw)
    if into is not None:
        ld = into.stride(4)
        if not (into.dtype == torch.bfloat16 and tuple(into.shape) == (n, cout, d, h, w) and ld >= cout and ld % 8 == 0
                and into.storage_offset() % 8 == 0 and into.stride() == (d * h * w * ld, 1, h * w * ld, w * ld, ld)):
            raise ValueError("conv_bn_relu3d_eval: `into` must be a channel slice of a channels_last_3d bf16 tensor of this op's shape")
        out = into
    else:
        out, ld = torch.empty((n, cout, d, h, w), dtype=torch.bfloat16, device=x.device, memory_format=_CL3), cout
    ws = torch.empty(lib.dmc_unit3d_bf16_eval_workspace_bytes(*geom), dtype=torch.uint8, device=x.device)
    with _span("conv3d_bf16_eval"):
        _lib.check(lib.dmc_unit3d_bf16_fwd_eval(_lib.ptr(x), _lib.ptr(wc), _lib.ptr(bn.weight), _lib.ptr(bn.bias), _lib.ptr(bn.running_mean),
                                                _lib.ptr(bn.running_var), float(bn.eps), _lib.ptr(ws), _lib.ptr(out), ld, *geom, int(relu),
                                                _stream()), "dmc_unit3d_bf16_fwd_eval")
    return out


def stem3d_eval_supported(x, conv, bn):
    """True if the I3D stem unit (2 -> 64 channels, 7x7x7, stride 2, TF-"SAME") can run forward-only with its BatchNorm3d in eval
    mode in the convolution's epilogue: a CUDA cue inside a bf16 autocast region, no autograd."""
    if not (x.is_cuda and x.dim() == 5 and x.shape[1] == 2 and torch.is_autocast_enabled()
            and torch.get_autocast_dtype("cuda") == torch.bfloat16):
        return False
    if tuple(conv.weight.shape) != (64, 2, 7, 7, 7) or tuple(conv.stride) != (2, 2, 2) or conv.bias is not None:
        return False
    if not _bn_eval_ok(bn):
        return False
    return all(int(s) >= 2 and int(s) % 2 == 0 for s in x.shape[2:])


def stem3d_bn_relu_eval(x, conv, bn, relu=True):
    """Forward-only relu?(bn(conv3d_1a_7x7(x))) with the BatchNorm's running statistics (dmc_stem3d_bf16_fwd_eval): the stem
    kernel with the affine map in its epilogue; a dense channels_last_3d bf16 result."""
    lib = _lib.load()
    if not (x.is_cuda and conv.weight.is_cuda and bn.running_mean.is_cuda):
        raise _lib.DmcHipError("stem3d_bn_relu_eval runs on the HIP extension only (no CPU fallback)")
    xc = x.detach().float().contiguous()
    wc = conv.weight.detach().float().contiguous()
    n, _, t, h, w = xc.shape
    od, oh, ow = (t - 2) // 2 + 1, (h - 2) // 2 + 1, (w - 2) // 2 + 1
    out = torch.empty((n, 64, od, oh, ow), dtype=torch.bfloat16, device=x.device, memory_format=_CL3)
    work = _floats(lib.dmc_stem3d_bf16_eval_workspace_bytes(n, t, h, w), x.device)
    with _span("stem3d_eval"):
        _lib.check(lib.dmc_stem3d_bf16_fwd_eval(_lib.ptr(xc), _lib.ptr(wc), _lib.ptr(bn.weight), _lib.ptr(bn.bias), _lib.ptr(bn.running_mean),
                                                _lib.ptr(bn.running_var), float(bn.eps), _lib.ptr(work), _lib.ptr(out), n, t, h, w,
                                                int(relu), _stream()), "dmc_stem3d_bf16_fwd_eval")
    return out


# ---- ContextNetwork / ContextNetworkAtt in eval mode: one launch per dilated conv + BatchNorm + LeakyReLU unit (csrc/ctx_eval.hip) ----

_CTX_MAX_INDEX = 1 << 31       # one launch indexes frames * H * W * 128 (the widest activation) below this
_CTX_SLOPE = 0.1


def context_eval_chunks(n, h, w):
    """Frame ranges [(a, b), ...] of the launches that evaluate ``n`` frames of ``h`` x ``w``: they tile [0, n) in order and each
    keeps frames * h * w * 128 below 2^31 (what dmc_ctx_unit_supported accepts).  A pure function of its arguments."""
    n, h, w = int(n), int(h), int(w)
    if n <= 0 or h <= 0 or w <= 0:
        raise ValueError("context_eval_chunks: sizes must be positive")
    per = (_CTX_MAX_INDEX - 1) // (h * w * 128)
    if per <= 0:
        raise ValueError("context_eval_chunks: one %d x %d frame is more than a launch can index" % (h, w))
    return [(a, min(a + per, n)) for a in range(0, n, per)]


def _ctx_unit_parts(unit, dilation=None):
    """(conv, bn) of a Sequential(Conv2d 3x3 dilated no-bias, BatchNorm2d eval, LeakyReLU(0.1)), or None."""
    if not isinstance(unit, torch.nn.Sequential) or len(unit) != 3:
        return None
    conv, bn, act = unit[0], unit[1], unit[2]
    if not (isinstance(conv, torch.nn.Conv2d) and isinstance(bn, torch.nn.BatchNorm2d) and isinstance(act, torch.nn.LeakyReLU)):
        return None
    if abs(act.negative_slope - _CTX_SLOPE) > 1e-12:
        return None
    if conv.bias is not None or conv.groups != 1 or conv.padding_mode != "zeros" or tuple(conv.kernel_size) != (3, 3) or tuple(conv.stride) != (1, 1):
        return None
    if conv.dilation[0] != conv.dilation[1] or tuple(conv.padding) != tuple(conv.dilation):
        return None
    if dilation is not None and conv.dilation[0] != dilation:
        return None
    if bn.training or not bn.track_running_stats or not bn.affine or bn.running_mean is None:
        return None
    if not (conv.weight.is_cuda and bn.weight.is_cuda and bn.running_mean.is_cuda):
        return None
    if conv.weight.dtype != torch.float32 or bn.weight.dtype != torch.float32 or bn.running_mean.dtype != torch.float32:
        return None
    return conv, bn


def _ctx_plan(net):
    """(trunk [(conv, bn), ...], flow (conv, bn), att (conv, bn) | None) of a ContextNetwork / ContextNetworkAtt whose every unit
    the eval kernels serve, or None."""
    trunk = getattr(net, "conv_context", None)
    if not isinstance(trunk, torch.nn.Sequential):
        return None
    units = list(trunk)
    att = None
    if hasattr(net, "predict_att"):
        pa = net.predict_att
        if not (isinstance(pa, torch.nn.Sequential) and len(pa) == 2 and isinstance(pa[1], torch.nn.ReLU)):
            return None
        flow, att = _ctx_unit_parts(net.predict_flow, 1), _ctx_unit_parts(pa[0], 1)
        if flow is None or att is None:
            return None
    else:
        if len(units) < 2:
            return None
        flow = _ctx_unit_parts(units.pop(), 1)
        if flow is None:
            return None
    parts = [_ctx_unit_parts(u) for u in units]
    if not parts or any(p is None for p in parts):
        return None
    c = 5
    for conv, _ in parts:
        if conv.in_channels != c:
            return None
        c = conv.out_channels
    heads = [flow] + ([att] if att is not None else [])
    if parts[0][0].dilation[0] != 1 or any(h[0].in_channels != c or h[0].out_channels != 2 for h in heads) or c != 32:
        return None
    return parts, flow, att


def context_eval_supported(net, x):
    """True if ``net`` (model.ContextNetwork / ContextNetworkAtt, batch_norm=True, every BatchNorm in eval mode) can be evaluated
    on ``x`` by this package's kernels: no autograd, a CUDA fp32 [N, 5, H, W] input, every unit of the expected form and accepted
    by dmc_ctx_unit_supported (code/dmcnet/model.py:45-104 under model.eval() + no_grad)."""
    if torch.is_grad_enabled():
        return False
    if not (torch.is_tensor(x) and x.is_cuda and x.dtype == torch.float32 and x.dim() == 4 and x.shape[1] == 5 and x.numel() > 0):
        return False
    plan = _ctx_plan(net)
    if plan is None:
        return False
    n, _, h, w = x.shape
    try:
        a, b = context_eval_chunks(n, h, w)[0]
    except ValueError:
        return False
    lib = _lib.load()
    parts, flow, _ = plan
    return all(lib.dmc_ctx_unit_supported(b - a, h, w, conv.in_channels, conv.out_channels, conv.dilation[0]) for conv, _ in parts + [flow])


def context_eval(net, x):
    """``net(x)`` of a ContextNetwork (-> gen_flow [N, 2, H, W]) or ContextNetworkAtt (-> (gen_flow, att_flow)) in eval mode on
    the kernels of csrc/ctx_eval.hip: seven launches per frame range (context_eval_chunks), NHWC fp32 between the units, the
    weights of the middle units split into bf16 slices once per call.  Requires context_eval_supported(net, x)."""
    lib = _lib.load()
    if not context_eval_supported(net, x):
        raise _lib.DmcHipError("context_eval: the network or the input is not served by the eval kernels (context_eval_supported)")
    parts, flow, att = _ctx_plan(net)
    x = x.contiguous()
    n, _, h, w = x.shape
    dev = x.device
    s = _stream()
    with _span("context_eval"):
        bns = [(_bn_eval_stats(bn), bn.weight.detach().contiguous(), bn.bias.detach().contiguous()) for _, bn in parts]
        w_first = parts[0][0].weight.detach().contiguous()
        packs = []
        for conv, _ in parts[1:]:
            cin, cout = conv.in_channels, conv.out_channels
            wp = torch.empty(lib.dmc_ctx_wpack_bytes(cin, cout), dtype=torch.uint8, device=dev)
            _lib.check(lib.dmc_ctx_pack_weights(_lib.ptr(conv.weight.detach().permute(0, 2, 3, 1).contiguous()), _lib.ptr(wp), cin, cout, s),
                       "dmc_ctx_pack_weights")
            packs.append(wp)
        heads = []
        for conv, bn in [flow] + ([att] if att is not None else []):
            heads.append((conv.weight.detach().permute(0, 2, 3, 1).contiguous(), _bn_eval_stats(bn), bn.weight.detach().contiguous(),
                          bn.bias.detach().contiguous()))
        out_flow = torch.empty((n, 2, h, w), dtype=torch.float32, device=dev)
        out_att = torch.empty((n, 2, h, w), dtype=torch.float32, device=dev) if att is not None else None
        for a, b in context_eval_chunks(n, h, w):
            f = b - a
            cur = torch.empty((f, h, w, 32), dtype=torch.float32, device=dev)
            st, g, be = bns[0]
            _lib.check(lib.dmc_ctx_first_eval(_lib.ptr(x[a:b]), _lib.ptr(w_first), _lib.ptr(st), _lib.ptr(g), _lib.ptr(be), _lib.ptr(cur),
                                              f, h, w, s), "dmc_ctx_first_eval")
            for (conv, _), wp, (st, g, be) in zip(parts[1:], packs, bns[1:]):
                nxt = torch.empty((f, h, w, conv.out_channels), dtype=torch.float32, device=dev)
                _lib.check(lib.dmc_ctx_unit_eval(_lib.ptr(cur), _lib.ptr(wp), _lib.ptr(st), _lib.ptr(g), _lib.ptr(be), _lib.ptr(nxt), f, h, w,
                                                 conv.in_channels, conv.out_channels, conv.dilation[0], s), "dmc_ctx_unit_eval")
                cur = nxt
            hf = heads[0]
            ha = heads[1] if att is not None else (None, None, None, None)
            _lib.check(lib.dmc_ctx_heads_eval(_lib.ptr(cur), _lib.ptr(hf[0]), _lib.ptr(hf[1]), _lib.ptr(hf[2]), _lib.ptr(hf[3]),
                                              _lib.ptr(ha[0]), _lib.ptr(ha[1]), _lib.ptr(ha[2]), _lib.ptr(ha[3]), _lib.ptr(out_flow[a:b]),
                                              _lib.ptr(out_att[a:b]) if att is not None else None, f, h, w, s), "dmc_ctx_heads_eval")
    if att is not None:
        return out_flow, out_att
    return out_flow


# ---- EstimatorDenseNet / EstimatorDenseNetSmall in eval mode: one feature buffer instead of the concatenations (csrc/dense_eval.hip) ----

#: bytes one feature buffer may take (dense_eval_chunks' default): the evaluator's 25-frame batch of 224 x 224 is one frame range for
#: both networks (2.33 GB at 464 channels)
DENSE_EVAL_BUDGET = 4 << 30
_DENSE_MAX_INDEX = 1 << 31     # one launch indexes frames * H * W * CT below this
_DENSE_SLOPE = 0.1
_DENSE_SLOT0 = 16              # the input's slot: ch_in live channels, zeros up to 16


def dense_eval_layout(widths, ch_in=5):
    """The feature buffer of a dense stack with layer widths ``widths`` over ``ch_in`` input channels, as a dict:
      "offsets"  first buffer channel of slot 0 (the input, 16 wide) and of slot k + 1 (the output of conv_k, round_up(width, 32) wide);
      "ct"       channels per pixel of the buffer;
      "layers"   per conv_k: (K, R, index) -- it reads buffer channels [0, K) and writes [K, K + R); ``index`` (int64 [K]) maps a
                 buffer channel to the input channel of the reference's conv_k, whose input is cat(y_{k-1}, ..., y_0, x), or -1 for a pad;
      "head"     (K, 2, index) of predict_flow the same way, K = ct.
    A pure function of its arguments."""
    widths = [int(v) for v in widths]
    ch_in = int(ch_in)
    if not widths or min(widths) <= 0 or not 0 < ch_in <= _DENSE_SLOT0:
        raise ValueError("dense_eval_layout: widths must be positive and 0 < ch_in <= %d" % _DENSE_SLOT0)
    offsets = [0, _DENSE_SLOT0]
    for v in widths:
        offsets.append(offsets[-1] + (v + 31) // 32 * 32)
    live = [ch_in] + widths                                        # live channels per slot

    def index(k):                                                  # the input of conv_k (k == len(widths): predict_flow)
        idx = torch.full((offsets[k + 1],), -1, dtype=torch.int64)
        ref = sum(widths[:k])                                      # x comes last in the reference's order ...
        idx[0:ch_in] = torch.arange(ref, ref + ch_in)
        for j in range(k):                                         # ... behind y_0, which is behind y_1, ...
            ref -= widths[j]
            idx[offsets[j + 1]:offsets[j + 1] + live[j + 1]] = torch.arange(ref, ref + widths[j])
        return idx

    layers = [(offsets[k + 1], offsets[k + 2] - offsets[k + 1], index(k)) for k in range(len(widths))]
    return {"offsets": offsets[:-1], "ct": offsets[-1], "layers": layers, "head": (offsets[-1], 2, index(len(widths)))}


def dense_eval_chunks(n, h, w, ct, budget_bytes=None):
    """Frame ranges [(a, b), ...] of the feature buffers that evaluate ``n`` frames of ``h`` x ``w`` with ``ct`` buffer channels: they
    tile [0, n) in order, each keeps frames * h * w * ct below 2^31 (what dmc_dense_supported accepts) and its fp32 buffer within
    ``budget_bytes`` (default DENSE_EVAL_BUDGET).  ValueError when a single frame does not fit.  A pure function of its arguments."""
    n, h, w, ct = int(n), int(h), int(w), int(ct)
    budget = DENSE_EVAL_BUDGET if budget_bytes is None else int(budget_bytes)
    if n <= 0 or h <= 0 or w <= 0 or ct <= 0:
        raise ValueError("dense_eval_chunks: sizes must be positive")
    per = min((_DENSE_MAX_INDEX - 1) // (h * w * ct), budget // (h * w * ct * 4))
    if per <= 0:
        raise ValueError("dense_eval_chunks: one %d x %d frame of %d channels is more than a launch can index or the budget holds" % (h, w, ct))
    return [(a, min(a + per, n)) for a in range(0, n, per)]


def _dense_conv_ok(conv, cin, cout=None, on_device=True):
    if not isinstance(conv, torch.nn.Conv2d) or conv.bias is None or conv.groups != 1 or conv.padding_mode != "zeros":
        return False
    if tuple(conv.kernel_size) != (3, 3) or tuple(conv.stride) != (1, 1) or tuple(conv.padding) != (1, 1) or tuple(conv.dilation) != (1, 1):
        return False
    if conv.in_channels != cin or (cout is not None and conv.out_channels != cout):
        return False
    return all((p.is_cuda or not on_device) and p.dtype == torch.float32 for p in (conv.weight, conv.bias))


def _dense_plan(net, on_device=True):
    """([conv_0, ...], predict_flow) of a dense estimator (model.DenseEstimatorBase) whose every unit the eval kernels serve, or None.
    ``on_device=False`` leaves out the one test that needs a GPU, that the parameters are CUDA tensors (the structural part alone)."""
    depth = getattr(net, "depth", None)
    if not isinstance(depth, int) or depth <= 0:
        return None
    convs, c = [], 5
    for i in range(depth):
        unit = getattr(net, "conv_%d" % i, None)
        if not isinstance(unit, torch.nn.Sequential) or len(unit) != 2 or not isinstance(unit[1], torch.nn.LeakyReLU):
            return None
        if abs(unit[1].negative_slope - _DENSE_SLOPE) > 1e-12 or not _dense_conv_ok(unit[0], c, None, on_device) or unit[0].out_channels > 128:
            return None
        convs.append(unit[0])
        c += unit[0].out_channels
    head = getattr(net, "predict_flow", None)
    if not _dense_conv_ok(head, c, 2, on_device):
        return None
    return convs, head


def dense_eval_supported(net, x):
    """True if ``net`` (model.EstimatorDenseNet / EstimatorDenseNetSmall: a DenseEstimatorBase with the stock forward) can be evaluated
    on ``x`` by the kernels of csrc/dense_eval.hip: no autograd, a non-empty CUDA fp32 [N, 5, H, W] input, every unit a
    Sequential(Conv2d 3x3 / stride 1 / padding 1 with bias, LeakyReLU(0.1)) of at most 128 channels whose inputs chain as the
    concatenations do, predict_flow a Conv2d of the same geometry with 2 channels, CUDA fp32 parameters, a frame range that
    fits (dense_eval_chunks) and every layer accepted by dmc_dense_supported."""
    if torch.is_grad_enabled():
        return False
    if not (torch.is_tensor(x) and x.is_cuda and x.dtype == torch.float32 and x.dim() == 4 and x.shape[1] == 5 and x.numel() > 0):
        return False
    plan = _dense_plan(net)
    if plan is None:
        return False
    lay = dense_eval_layout([c.out_channels for c in plan[0]])
    n, _, h, w = x.shape
    try:
        a, b = dense_eval_chunks(n, h, w, lay["ct"])[0]
    except ValueError:
        return False
    lib = _lib.load()
    return all(lib.dmc_dense_supported(b - a, h, w, lay["ct"], k, r) for k, r, _ in lay["layers"] + [lay["head"]])


def _dense_weight(conv, k, r, index):
    """(weight OHWI [r][3][3][k], bias [r]) of ``conv`` in buffer order: input channel ``index[b]`` of the module at buffer channel b,
    zeros in the pad columns, the pad rows and the pad bias entries."""
    w = conv.weight.detach().permute(0, 2, 3, 1)
    index = index.to(w.device)
    live = (index >= 0).nonzero().reshape(-1)
    wp = torch.zeros((r, 3, 3, k), dtype=torch.float32, device=w.device)
    wp[:conv.out_channels].index_copy_(3, live, w.index_select(3, index[live]))
    bp = torch.zeros((r,), dtype=torch.float32, device=w.device)
    bp[:conv.out_channels] = conv.bias.detach()
    return wp, bp


def dense_eval(net, x):
    """``net(x)`` of an EstimatorDenseNet / EstimatorDenseNetSmall (-> gen_flow [N, 2, H, W]) in eval mode on the kernels of
    csrc/dense_eval.hip: per frame range (dense_eval_chunks) one NHWC fp32 feature buffer, the ingest, one launch per layer that
    reads a prefix of the buffer and appends its slot, and the head -- no concatenation.  The weights are permuted into buffer order,
    padded and split into bf16 slices once per call.  Requires dense_eval_supported(net, x)."""
    lib = _lib.load()
    if not dense_eval_supported(net, x):
        raise _lib.DmcHipError("dense_eval: the network or the input is not served by the eval kernels (dense_eval_supported)")
    convs, head = _dense_plan(net)
    lay = dense_eval_layout([c.out_channels for c in convs])
    ct = lay["ct"]
    x = x.contiguous()
    n, _, h, w = x.shape
    dev = x.device
    s = _stream()
    with _span("dense_eval"):
        layers = []
        for conv, (k, r, index) in zip(convs, lay["layers"]):
            wp, bp = _dense_weight(conv, k, r, index)
            pack = torch.empty(lib.dmc_dense_wpack_bytes(k, r), dtype=torch.uint8, device=dev)
            _lib.check(lib.dmc_dense_pack_weights(_lib.ptr(wp), _lib.ptr(pack), k, r, s), "dmc_dense_pack_weights")
            layers.append((pack, bp, k, r))
        hk, _, hindex = lay["head"]
        hw_, hb = _dense_weight(head, hk, 2, hindex)
        out = torch.empty((n, 2, h, w), dtype=torch.float32, device=dev)
        for a, b in dense_eval_chunks(n, h, w, ct):
            f = b - a
            feat = torch.empty((f, h, w, ct), dtype=torch.float32, device=dev)
            _lib.check(lib.dmc_dense_ingest(_lib.ptr(x[a:b]), _lib.ptr(feat), f, h, w, ct, s), "dmc_dense_ingest")
            for pack, bp, k, r in layers:
                _lib.check(lib.dmc_dense_layer_eval(_lib.ptr(feat), _lib.ptr(pack), _lib.ptr(bp), f, h, w, ct, k, r, s), "dmc_dense_layer_eval")
            _lib.check(lib.dmc_dense_head_eval(_lib.ptr(feat), _lib.ptr(hw_), _lib.ptr(hb), _lib.ptr(out[a:b]), f, h, w, ct, hk, s),
                       "dmc_dense_head_eval")
            del feat
    return out


# ---- EstimatorDenseNet / EstimatorDenseNetSmall in training: forward on the feature buffer, backward in place (csrc/dense_train.hip) ----

#: bytes one feature buffer (and one gradient buffer) of the training route may take: dense_eval_chunks' budget on that route
DENSE_TRAIN_BUDGET = 4 << 30


def _dense_train_chunks(n, h, w, ct):
    return dense_eval_chunks(n, h, w, ct, budget_bytes=DENSE_TRAIN_BUDGET)


def dense_train_supported(net, x):
    """True if ``net(x)`` of an EstimatorDenseNet / EstimatorDenseNetSmall can run WITH autograd on the kernels of csrc/dense_eval.hip
    (forward) and csrc/dense_train.hip (backward): autograd enabled, a non-empty CUDA fp32 [N, 5, H, W] input, a
    model.DenseEstimatorBase with the stock forward (not EstimatorDenseNetTiny), the structure
    dense_eval_supported asks for (_dense_plan), frame ranges that fit (dense_eval_chunks under DENSE_TRAIN_BUDGET) and every range
    and layer accepted by dmc_densetrain_supported."""
    if not torch.is_grad_enabled():
        return False
    if not (torch.is_tensor(x) and x.is_cuda and x.dtype == torch.float32 and x.dim() == 4 and x.shape[1] == 5 and x.numel() > 0):
        return False
    base = next((c for c in type(net).__mro__ if c.__name__ == "DenseEstimatorBase"), None)
    if base is None or type(net).forward is not base.forward:     # EstimatorDenseNetTiny has a forward (and kernels) of its own
        return False
    plan = _dense_plan(net)
    if plan is None:
        return False
    lay = dense_eval_layout([c.out_channels for c in plan[0]])
    n, _, h, w = x.shape
    try:
        chunks = _dense_train_chunks(n, h, w, lay["ct"])
    except ValueError:
        return False
    lib = _lib.load()
    sizes = sorted({b - a for a, b in chunks})
    return all(lib.dmc_densetrain_supported(f, h, w, lay["ct"], k, r) for f in sizes for k, r, _ in lay["layers"] + [lay["head"]])


def _dense_weight_grad(dwb, cout, index):
    """The inverse of _dense_weight for a gradient: ``dwb`` OHWI [r][3][3][k] in buffer order -> [cout, cin, 3, 3] in the module's
    order (input channel ``index[b]`` from buffer channel b); the pad rows and the pad columns are dropped."""
    index = index.to(dwb.device)
    live = (index >= 0).nonzero().reshape(-1)
    out = torch.empty((cout, 3, 3, int(live.numel())), dtype=dwb.dtype, device=dwb.device)
    out.index_copy_(3, index[live], dwb[:cout].index_select(3, live))
    return out.permute(0, 3, 1, 2).contiguous()


def _dense_dgrad_blocks(k):
    """[(c0, cb), ...]: the data gradient's output channels [0, k) in blocks of at most 128, the last padded to a multiple of 32."""
    return [(c0, min(128, (k - c0 + 31) // 32 * 32)) for c0 in range(0, k, 128)]


def _dense_dgrad_packs(wp, k, r):
    """The transposed, tap-mirrored bf16x3 packs of ``wp`` (OHWI [r][3][3][k], buffer order), one per block of _dense_dgrad_blocks."""
    lib = _lib.load()
    packs = []
    for c0, cb in _dense_dgrad_blocks(k):
        blk = torch.zeros((r, 3, 3, cb), dtype=torch.float32, device=wp.device)
        live = min(cb, k - c0)
        blk[..., :live] = wp[..., c0:c0 + live]
        pack = torch.empty(lib.dmc_dconv_wpack_bytes(cb, r), dtype=torch.uint8, device=wp.device)
        _lib.check(lib.dmc_dconv_pack_weights(_lib.ptr(blk), _lib.ptr(pack), cb, r, 1, _stream()), "dmc_dconv_pack_weights")
        packs.append((c0, cb, pack))
    return packs


class _DenseTrain(torch.autograd.Function):
    """The dense stack of an EstimatorDenseNet / EstimatorDenseNetSmall over ``x`` and its twelve parameters (w_0, b_0, ..., w_4, b_4,
    w_head, b_head).  Forward: the launches of dense_eval per frame range; every range's feature buffer is kept.  Backward: per
    range one gradient buffer of the same layout (csrc/dense_train.hip); the ranges' parameter gradients are added in range order."""

    @staticmethod
    def forward(ctx, x, meta, *params):
        lib = _lib.load()
        lay, widths = meta
        ct = lay["ct"]
        x = x.contiguous()
        n, _, h, w = x.shape
        dev = x.device
        s = _stream()
        with _span("dense_train_fwd"):
            layers = []
            for i, (k, r, index) in enumerate(lay["layers"]):
                wp, bp = _dense_weight(_ConvView(params[2 * i], params[2 * i + 1]), k, r, index)
                pack = torch.empty(lib.dmc_dense_wpack_bytes(k, r), dtype=torch.uint8, device=dev)
                _lib.check(lib.dmc_dense_pack_weights(_lib.ptr(wp), _lib.ptr(pack), k, r, s), "dmc_dense_pack_weights")
                layers.append((wp, bp, pack, k, r))
            hk, _, hindex = lay["head"]
            hw_, hb = _dense_weight(_ConvView(params[-2], params[-1]), hk, 2, hindex)
            out = torch.empty((n, 2, h, w), dtype=torch.float32, device=dev)
            feats = []
            for a, b in _dense_train_chunks(n, h, w, ct):
                f = b - a
                feat = torch.empty((f, h, w, ct), dtype=torch.float32, device=dev)
                _lib.check(lib.dmc_dense_ingest(_lib.ptr(x[a:b]), _lib.ptr(feat), f, h, w, ct, s), "dmc_dense_ingest")
                for _, bp, pack, k, r in layers:
                    _lib.check(lib.dmc_dense_layer_eval(_lib.ptr(feat), _lib.ptr(pack), _lib.ptr(bp), f, h, w, ct, k, r, s), "dmc_dense_layer_eval")
                _lib.check(lib.dmc_dense_head_eval(_lib.ptr(feat), _lib.ptr(hw_), _lib.ptr(hb), _lib.ptr(out[a:b]), f, h, w, ct, hk, s),
                           "dmc_dense_head_eval")
                feats.append((a, b, feat))
        ctx.dense = (lay, widths, feats, [(wp, k, r) for wp, _, _, k, r in layers], hw_, (n, h, w))
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dout):
        lib = _lib.load()
        lay, widths, feats, layers, hw_, (n, h, w) = ctx.dense
        ct = lay["ct"]
        dout = dout.contiguous()
        dev = dout.device
        s = _stream()
        need_dx = ctx.needs_input_grad[0]
        depth = len(layers)
        with _span("dense_train_bwd"):
            packs = [_dense_dgrad_packs(wp, k, r) if (i > 0 or need_dx) else None for i, (wp, k, r) in enumerate(layers)]
            dx = torch.empty((n, 5, h, w), dtype=torch.float32, device=dev) if need_dx else None
            total = None
            for a, b, feat in feats:
                f = b - a
                G = torch.empty((f, h, w, ct), dtype=torch.float32, device=dev)
                dws = [torch.empty((r, 3, 3, k), dtype=torch.float32, device=dev) for _, k, r in layers]
                dbs = [torch.empty((r,), dtype=torch.float32, device=dev) for _, _, r in layers]
                dwh = torch.empty((2, 3, 3, ct), dtype=torch.float32, device=dev)
                dbh = torch.empty((2,), dtype=torch.float32, device=dev)
                dpart = dout[a:b]
                _lib.check(lib.dmc_densetrain_head_dgrad(_lib.ptr(dpart), _lib.ptr(hw_), _lib.ptr(G), f, h, w, ct, s), "dmc_densetrain_head_dgrad")
                work = torch.empty(lib.dmc_densetrain_head_workspace_bytes(f, h, w, ct), dtype=torch.uint8, device=dev)
                _lib.check(lib.dmc_densetrain_head_wgrad(_lib.ptr(dpart), _lib.ptr(feat), _lib.ptr(dwh), _lib.ptr(dbh), _lib.ptr(work), f, h, w, ct, s),
                           "dmc_densetrain_head_wgrad")
                for i in range(depth - 1, -1, -1):
                    _, k, r = layers[i]
                    work = torch.empty(lib.dmc_densetrain_mask_workspace_bytes(f, h, w, r), dtype=torch.uint8, device=dev)
                    _lib.check(lib.dmc_densetrain_mask(_lib.ptr(feat), _lib.ptr(G), _lib.ptr(dbs[i]), _lib.ptr(work), f, h, w, ct, k, r, s),
                               "dmc_densetrain_mask")
                    work = torch.empty(lib.dmc_densetrain_wgrad_workspace_bytes(f, h, w, k, r), dtype=torch.uint8, device=dev)
                    _lib.check(lib.dmc_densetrain_layer_wgrad(_lib.ptr(feat), _lib.ptr(G), _lib.ptr(dws[i]), _lib.ptr(work), f, h, w, ct, k, r, s),
                               "dmc_densetrain_layer_wgrad")
                    del work
                    if packs[i] is not None:
                        for c0, cb, pack in packs[i]:
                            _lib.check(lib.dmc_densetrain_layer_dgrad(_lib.ptr(G), _lib.ptr(pack), f, h, w, ct, k, r, c0, cb, s),
                                       "dmc_densetrain_layer_dgrad")
                if need_dx:
                    _lib.check(lib.dmc_densetrain_export(_lib.ptr(G), _lib.ptr(dx[a:b]), f, h, w, ct, s), "dmc_densetrain_export")
                del G
                part = dws + dbs + [dwh, dbh]
                if total is None:
                    total = part
                else:                                              # the ranges in order
                    for t, p in zip(total, part):
                        t.add_(p)
            ctx.dense = None
            dws, dbs, dwh, dbh = total[:depth], total[depth:2 * depth], total[-2], total[-1]
            grads = []
            for i, (_, _, index) in enumerate(lay["layers"]):
                grads.append(_dense_weight_grad(dws[i], widths[i], index))
                grads.append(dbs[i][:widths[i]].clone())
            grads.append(_dense_weight_grad(dwh, 2, lay["head"][2]))
            grads.append(dbh)
        return (dx, None) + tuple(g if ctx.needs_input_grad[2 + j] else None for j, g in enumerate(grads))


class _ConvView(object):
    """What _dense_weight reads of a convolution, for a (weight, bias) pair that is not a module's."""

    def __init__(self, weight, bias):
        self.weight, self.bias, self.out_channels = weight, bias, int(weight.shape[0])


def dense_train(net, x):
    """``net(x)`` of an EstimatorDenseNet / EstimatorDenseNetSmall (-> gen_flow [N, 2, H, W]) with autograd, as ONE
    torch.autograd.Function over ``x`` and the twelve parameters: the forward is dense_eval's launches per frame range with every
    range's feature buffer kept; the backward (csrc/dense_train.hip) runs in a second buffer of the same layout -- head, then per
    layer the LeakyReLU mask with the bias gradient, the weight gradient and the in-place data gradient -- without a concatenation,
    a saved pre-activation or an atomic.  Raises DmcHipError unless dense_train_supported(net, x): never a silent fall-back."""
    if not dense_train_supported(net, x):
        raise _lib.DmcHipError("dense_train: the network or the input is not served by the training kernels (dense_train_supported)")
    convs, head = _dense_plan(net)
    widths = [c.out_channels for c in convs]
    lay = dense_eval_layout(widths)
    params = []
    for c in convs + [head]:
        params += [c.weight, c.bias]
    return _DenseTrain.apply(x, (lay, widths), *params)


# ---- EstimatorDenseNetTinyEarlyFusionSum / Stack: eval and training on one feature buffer (csrc/early_fusion.hip) ----

_EF_WIDTHS = (8, 6, 4, 2)      # conv_1 .. conv_4
_EF_SLOPE = 0.1


def early_fusion_layout(stack):
    """The feature buffer of an early-fusion estimator (``stack``: cat(m, r), else m + r), as a dict:
      "offsets"  slot name -> (first buffer channel, live channels), in production order: "m" and "r" (Stack) or "s" (Sum), then
                 "y1" .. "y4"; every slot is padded to a multiple of 4 channels;
      "ct"       channels per pixel of the buffer (Stack 40, Sum 32);
      "layers"   per conv_k, k = 1 .. 4: (K, R, index) -- it reads buffer channels [0, K) and writes [K, K + round_up4(R)); ``index``
                 (int64 [K]) maps a buffer channel to the input channel of the reference's conv_k, whose input is
                 cat(y_{k-1}, ..., y_1, base) with base = cat(m, r) or s, or -1 for a pad;
      "head"     (K, 2, index) of predict_flow the same way, K = ct.
    A pure function of its argument."""
    stack = bool(stack)
    base = 16 if stack else 8
    offsets = {"m": (0, 8), "r": (8, 8)} if stack else {"s": (0, 8)}
    first = [base]
    for v in _EF_WIDTHS:
        first.append(first[-1] + (v + 3) // 4 * 4)
    for j, v in enumerate(_EF_WIDTHS):
        offsets["y%d" % (j + 1)] = (first[j], v)

    def index(k):                                                  # the input of conv_k (k == 5: predict_flow): y_1 .. y_{k-1} exist
        idx = torch.full((first[k - 1],), -1, dtype=torch.int64)
        ref = sum(_EF_WIDTHS[:k - 1])                              # the base comes last in the reference's order ...
        idx[0:base] = torch.arange(ref, ref + base)
        for j in range(k - 1):                                     # ... behind y_1, which is behind y_2, ...
            ref -= _EF_WIDTHS[j]
            idx[first[j]:first[j] + _EF_WIDTHS[j]] = torch.arange(ref, ref + _EF_WIDTHS[j])
        return idx

    layers = [(first[k - 1], _EF_WIDTHS[k - 1], index(k)) for k in (1, 2, 3, 4)]
    return {"offsets": offsets, "ct": first[-1], "layers": layers, "head": (first[-1], 2, index(5))}


def _ef_plan(net, on_device=True):
    """(stack, conv_0_mv, conv_0_r, [conv_1 .. conv_4], predict_flow) of a model._EarlyFusion with the stock forward whose every unit
    the kernels serve, or None.  ``on_device=False`` leaves out the test that the parameters are CUDA tensors."""
    base = next((c for c in type(net).__mro__ if c.__name__ == "_EarlyFusion"), None)
    if base is None or type(net).forward is not base.forward or not isinstance(getattr(net, "stack", None), bool):
        return None

    def unit(name, cin, cout):
        u = getattr(net, name, None)
        if not isinstance(u, torch.nn.Sequential) or len(u) != 2 or not isinstance(u[1], torch.nn.LeakyReLU):
            return None
        if abs(u[1].negative_slope - _EF_SLOPE) > 1e-12 or not _dense_conv_ok(u[0], cin, cout, on_device):
            return None
        return u[0]

    mv, res = unit("conv_0_mv", 2, 8), unit("conv_0_r", 3, 8)
    if mv is None or res is None:
        return None
    convs, c = [], 16 if net.stack else 8
    for i, v in enumerate(_EF_WIDTHS):
        conv = unit("conv_%d" % (i + 1), c, v)
        if conv is None:
            return None
        convs.append(conv)
        c += v
    head = getattr(net, "predict_flow", None)
    if not _dense_conv_ok(head, c, 2, on_device):
        return None
    return net.stack, mv, res, convs, head


def _ef_input_ok(x):
    return torch.is_tensor(x) and x.is_cuda and x.dtype == torch.float32 and x.dim() == 4 and x.shape[1] == 5 and x.numel() > 0


def _ef_ranges_ok(lay, chunks, h, w):
    lib = _lib.load()
    sizes = sorted({b - a for a, b in chunks})
    return all(lib.dmc_ef_supported(f, h, w, lay["ct"], k, r) for f in sizes for k, r, _ in lay["layers"] + [lay["head"]])


def early_fusion_supported(net, x):
    """True if ``net`` (model.EstimatorDenseNetTinyEarlyFusionSum / Stack: a model._EarlyFusion with the stock forward) can be
    evaluated on ``x`` by the kernels of csrc/early_fusion.hip: no autograd, a non-empty CUDA fp32 [N, 5, H, W] input, every unit a
    Sequential(Conv2d 3x3 / stride 1 / padding 1 with bias, LeakyReLU(0.1)) of _EarlyFusion's channel counts, predict_flow a Conv2d
    of the same geometry with 2 channels, CUDA fp32 parameters, a frame range that fits (dense_eval_chunks) and every layer
    accepted by dmc_ef_supported."""
    if torch.is_grad_enabled() or not _ef_input_ok(x):
        return False
    plan = _ef_plan(net)
    if plan is None:
        return False
    lay = early_fusion_layout(plan[0])
    n, _, h, w = x.shape
    try:
        chunks = dense_eval_chunks(n, h, w, lay["ct"])
    except ValueError:
        return False
    return _ef_ranges_ok(lay, chunks, h, w)


def _ef_weights(lay, convs, head):
    """[(w [R][9][K] in buffer order, bias [R], K, R), ...] of conv_1 .. conv_4 and of predict_flow; ``convs`` / ``head`` are modules or
    _ConvView pairs."""
    out = []
    for conv, (k, r, index) in zip(list(convs) + [head], lay["layers"] + [lay["head"]]):
        wp, bp = _dense_weight(conv, k, r, index)
        out.append((wp, bp, k, r))
    return out


def _ef_forward(lib, stack, lay, x, first, weights, chunks, keep):
    """The forward launches per frame range: dmc_ef_first, four dmc_ef_layer, dmc_ef_head.  ``first`` = (w_mv, b_mv, w_r, b_r).  With
    ``keep`` every range's (a, b, feat, signs) is returned as well (signs: the sign plane, Sum only)."""
    ct = lay["ct"]
    n, _, h, w = x.shape
    dev = x.device
    s = _stream()
    out = torch.empty((n, 2, h, w), dtype=torch.float32, device=dev)
    kept = []
    for a, b in chunks:
        f = b - a
        feat = torch.empty((f, h, w, ct), dtype=torch.float32, device=dev)
        signs = torch.empty((f, h, w), dtype=torch.int16, device=dev) if keep and not stack else None
        _lib.check(lib.dmc_ef_first(_lib.ptr(x[a:b]), _lib.ptr(first[0]), _lib.ptr(first[1]), _lib.ptr(first[2]), _lib.ptr(first[3]),
                                    _lib.ptr(feat), _lib.ptr(signs), f, h, w, ct, int(stack), s), "dmc_ef_first")
        for wp, bp, k, r in weights[:-1]:
            _lib.check(lib.dmc_ef_layer(_lib.ptr(feat), _lib.ptr(wp), _lib.ptr(bp), f, h, w, ct, k, r, s), "dmc_ef_layer")
        hw_, hb, hk, _ = weights[-1]
        _lib.check(lib.dmc_ef_head(_lib.ptr(feat), _lib.ptr(hw_), _lib.ptr(hb), _lib.ptr(out[a:b]), f, h, w, ct, hk, s), "dmc_ef_head")
        if keep:
            kept.append((a, b, feat, signs))
        del feat
    return out, kept


def early_fusion_eval(net, x):
    """``net(x)`` of an EstimatorDenseNetTinyEarlyFusionSum / Stack (-> gen_flow [N, 2, H, W]) with autograd off on the kernels of
    csrc/early_fusion.hip: per frame range (dense_eval_chunks) one NHWC fp32 feature buffer, dmc_ef_first, one dmc_ef_layer per
    conv_1 .. conv_4 that reads a prefix of the buffer and appends its slot, and dmc_ef_head -- no concatenation.  The weights are
    permuted into buffer order once per call.  Requires early_fusion_supported(net, x)."""
    lib = _lib.load()
    if not early_fusion_supported(net, x):
        raise _lib.DmcHipError("early_fusion_eval: the network or the input is not served by the kernels (early_fusion_supported)")
    stack, mv, res, convs, head = _ef_plan(net)
    lay = early_fusion_layout(stack)
    x = x.contiguous()
    n, _, h, w = x.shape
    with _span("early_fusion_eval"):
        first = [t.detach().contiguous() for t in (mv.weight, mv.bias, res.weight, res.bias)]
        out, _ = _ef_forward(lib, stack, lay, x, first, _ef_weights(lay, convs, head), dense_eval_chunks(n, h, w, lay["ct"]), False)
    return out


def early_fusion_train_supported(net, x):
    """True if ``net(x)`` of an early-fusion estimator can run WITH autograd on the kernels of csrc/early_fusion.hip, forward and
    backward: autograd enabled, a non-empty CUDA fp32 [N, 5, H, W] input that does NOT require a gradient (no input gradient is
    built: such a call takes the stock modules), the structure early_fusion_supported asks for, frame ranges that fit
    (dense_eval_chunks under DENSE_TRAIN_BUDGET) and every range and layer accepted by dmc_ef_supported."""
    if not torch.is_grad_enabled() or not _ef_input_ok(x) or x.requires_grad:
        return False
    plan = _ef_plan(net)
    if plan is None:
        return False
    lay = early_fusion_layout(plan[0])
    n, _, h, w = x.shape
    try:
        chunks = _dense_train_chunks(n, h, w, lay["ct"])
    except ValueError:
        return False
    return _ef_ranges_ok(lay, chunks, h, w)


class _EarlyFusionTrain(torch.autograd.Function):
    """An early-fusion estimator over ``x`` and its fourteen parameters (w_mv, b_mv, w_r, b_r, w_1, b_1, ..., w_4, b_4, w_head,
    b_head).  Forward: the launches of early_fusion_eval per frame range; every range's feature buffer and, for Sum, sign plane is
    kept.  Backward: per range one gradient buffer of the same layout, from the head down; the ranges' parameter gradients are
    added in range order.  No gradient with respect to ``x``."""

    @staticmethod
    def forward(ctx, x, meta, *params):
        lib = _lib.load()
        stack, lay = meta
        x = x.contiguous()
        n, _, h, w = x.shape
        with _span("early_fusion_train_fwd"):
            first = [p.detach().contiguous() for p in params[:4]]
            views = [_ConvView(params[4 + 2 * i], params[5 + 2 * i]) for i in range(5)]
            weights = _ef_weights(lay, views[:4], views[4])
            out, kept = _ef_forward(lib, stack, lay, x, first, weights, _dense_train_chunks(n, h, w, lay["ct"]), True)
        ctx.save_for_backward(x)
        ctx.ef = (stack, lay, kept, weights)
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dout):
        lib = _lib.load()
        stack, lay, kept, weights = ctx.ef
        x, = ctx.saved_tensors
        ct = lay["ct"]
        n, _, h, w = x.shape
        dout = dout.contiguous()
        dev = dout.device
        s = _stream()

        def work(nbytes):
            return torch.empty(max(int(nbytes), 1), dtype=torch.uint8, device=dev)

        with _span("early_fusion_train_bwd"):
            total = None
            hw_, _, hk, _ = weights[-1]
            for a, b, feat, signs in kept:
                f = b - a
                G = torch.empty((f, h, w, ct), dtype=torch.float32, device=dev)
                dws = [torch.empty((r, 3, 3, k), dtype=torch.float32, device=dev) for _, _, k, r in weights]
                dbs = [torch.empty((r,), dtype=torch.float32, device=dev) for _, _, _, r in weights]
                firsts = [torch.empty(shape, dtype=torch.float32, device=dev) for shape in ((8, 2, 3, 3), (8,), (8, 3, 3, 3), (8,))]
                dpart = dout[a:b]
                _lib.check(lib.dmc_ef_head_dgrad(_lib.ptr(dpart), _lib.ptr(hw_), _lib.ptr(G), f, h, w, ct, hk, s), "dmc_ef_head_dgrad")
                ws = work(lib.dmc_ef_head_wgrad_workspace_bytes(f, h, w, hk))
                _lib.check(lib.dmc_ef_head_wgrad(_lib.ptr(dpart), _lib.ptr(feat), _lib.ptr(dws[4]), _lib.ptr(dbs[4]), _lib.ptr(ws), f, h, w, ct, hk, s),
                           "dmc_ef_head_wgrad")
                for i in (3, 2, 1, 0):
                    wp, _, k, r = weights[i]
                    ws = work(lib.dmc_ef_layer_mask_workspace_bytes(f, h, w, r))
                    _lib.check(lib.dmc_ef_layer_mask(_lib.ptr(feat), _lib.ptr(G), _lib.ptr(dbs[i]), _lib.ptr(ws), f, h, w, ct, k, r, s),
                               "dmc_ef_layer_mask")
                    ws = work(lib.dmc_ef_layer_wgrad_workspace_bytes(f, h, w, k, r))
                    _lib.check(lib.dmc_ef_layer_wgrad(_lib.ptr(feat), _lib.ptr(G), _lib.ptr(dws[i]), _lib.ptr(ws), f, h, w, ct, k, r, s),
                               "dmc_ef_layer_wgrad")
                    _lib.check(lib.dmc_ef_layer_dgrad(_lib.ptr(G), _lib.ptr(wp), f, h, w, ct, k, r, s), "dmc_ef_layer_dgrad")
                ws = work(lib.dmc_ef_first_bwd_workspace_bytes(f, h, w))
                _lib.check(lib.dmc_ef_first_bwd(_lib.ptr(G), _lib.ptr(x[a:b]), _lib.ptr(signs), _lib.ptr(feat), _lib.ptr(firsts[0]),
                                                _lib.ptr(firsts[1]), _lib.ptr(firsts[2]), _lib.ptr(firsts[3]), _lib.ptr(ws), f, h, w, ct,
                                                int(stack), s), "dmc_ef_first_bwd")
                del G, ws
                part = firsts + dws + dbs
                if total is None:
                    total = part
                else:                                              # the ranges in order
                    for t, p in zip(total, part):
                        t.add_(p)
            ctx.ef = None
            grads = list(total[:4])
            dws, dbs = total[4:9], total[9:14]
            for i, (_, r, index) in enumerate(lay["layers"] + [lay["head"]]):
                grads.append(_dense_weight_grad(dws[i], r, index))
                grads.append(dbs[i])
        return (None, None) + tuple(g if ctx.needs_input_grad[2 + j] else None for j, g in enumerate(grads))


def early_fusion_train(net, x):
    """``net(x)`` of an EstimatorDenseNetTinyEarlyFusionSum / Stack (-> gen_flow [N, 2, H, W]) with autograd, as ONE
    torch.autograd.Function over ``x`` and the fourteen parameters: the forward is early_fusion_eval's launches per frame range with
    every range's feature buffer (and, for Sum, the sign plane of the two first convolutions) kept; the backward runs in a second
    buffer of the same layout -- head, then per layer the LeakyReLU mask with the bias gradient, the weight gradient and the in-place
    data gradient, then the two first convolutions' gradients -- without a concatenation or an atomic.  The weight gradients come back
    in the parameters' own layout; ``x`` gets no gradient.  Raises DmcHipError unless early_fusion_train_supported(net, x)."""
    if not early_fusion_train_supported(net, x):
        raise _lib.DmcHipError("early_fusion_train: the network or the input is not served by the kernels (early_fusion_train_supported)")
    stack, mv, res, convs, head = _ef_plan(net)
    params = [mv.weight, mv.bias, res.weight, res.bias]
    for c in convs + [head]:
        params += [c.weight, c.bias]
    return _EarlyFusionTrain.apply(x, (stack, early_fusion_layout(stack)), *params)


# ---- ContextNetwork / ContextNetworkAtt in training: the dilated convolutions of the middle units (csrc/dconv.hip) ----

def _dconv_geom_ok(x, cin, cout, dilation):
    if not (torch.is_tensor(x) and x.is_cuda and x.dtype == torch.float32 and x.dim() == 4 and x.shape[1] == cin and x.numel() > 0):
        return False
    n, _, h, w = x.shape
    return bool(_lib.load().dmc_dconv_supported(n, h, w, cin, cout, int(dilation)))


def _dconv_module_ok(conv):
    if not isinstance(conv, torch.nn.Conv2d):
        return False
    if conv.bias is not None or conv.groups != 1 or conv.padding_mode != "zeros" or tuple(conv.kernel_size) != (3, 3) or tuple(conv.stride) != (1, 1):
        return False
    if conv.dilation[0] != conv.dilation[1] or tuple(conv.padding) != tuple(conv.dilation):
        return False
    return conv.weight.is_cuda and conv.weight.dtype == torch.float32


def dilated_conv_supported(x, conv):
    """True if ``conv(x)`` can run as ``dilated_conv(x, conv.weight, conv.dilation[0])``: a Conv2d 3x3, stride 1, padding = dilation,
    no bias, fp32 CUDA weights (code/dmcnet/model.py:45-104, the middle units), a CUDA fp32 [N, Cin, H, W] input and a shape that
    dmc_dconv_supported accepts (Cin, Cout in {32, 64, 96, 128}, dilation in {1, 2, 4, 8, 16}, N H W 128 < 2^31).  False on the CPU."""
    return _dconv_module_ok(conv) and _dconv_geom_ok(x, conv.in_channels, conv.out_channels, conv.dilation[0])


def _dconv_pack(wcl, cin, cout, transposed):
    lib = _lib.load()
    wp = torch.empty(lib.dmc_dconv_wpack_bytes(cin, cout), dtype=torch.uint8, device=wcl.device)
    _lib.check(lib.dmc_dconv_pack_weights(_lib.ptr(wcl), _lib.ptr(wp), cin, cout, int(transposed), _stream()), "dmc_dconv_pack_weights")
    return wp


class _DilatedConv(torch.autograd.Function):
    """Conv2d(Cin, Cout, 3, 1, d, d, bias=False) of a ContextNetwork middle unit (code/dmcnet/model.py:45-104) over channels_last
    tensors: forward, data gradient (the same kernel on the transposed weight pack) and weight gradient on csrc/dconv.hip."""

    @staticmethod
    def forward(ctx, x, weight, dilation):
        _need_cuda(x, weight)
        cout, cin = int(weight.shape[0]), int(weight.shape[1])
        if not (weight.dim() == 4 and tuple(weight.shape[2:]) == (3, 3) and _dconv_geom_ok(x, cin, cout, dilation)):
            raise _lib.DmcHipError("dilated_conv: x %s, weight %s, dilation %s is not served by the kernels (dilated_conv_supported)"
                                   % (tuple(x.shape), tuple(weight.shape), dilation))
        lib = _lib.load()
        x, wcl = _as_cl(x), _as_cl(weight.detach())
        n, _, h, w = x.shape
        with _span("dconv_fwd"):
            y = torch.empty((n, cout, h, w), dtype=torch.float32, device=x.device, memory_format=_CL)
            _lib.check(lib.dmc_dconv_fwd(_lib.ptr(x), _lib.ptr(_dconv_pack(wcl, cin, cout, False)), _lib.ptr(y), n, h, w, cin, cout, dilation,
                                         _stream()), "dmc_dconv_fwd")
        ctx.save_for_backward(x, weight)
        ctx.dilation = dilation
        return y

    @staticmethod
    def backward(ctx, dy):
        x, weight = ctx.saved_tensors
        lib = _lib.load()
        d = ctx.dilation
        n, cin, h, w = x.shape
        cout = int(weight.shape[0])
        dy = _as_cl(dy)
        dx = dw = None
        if ctx.needs_input_grad[0]:
            with _span("dconv_dgrad"):
                wt = _dconv_pack(_as_cl(weight.detach()), cin, cout, True)
                dx = torch.empty((n, cin, h, w), dtype=torch.float32, device=x.device, memory_format=_CL)
                _lib.check(lib.dmc_dconv_fwd(_lib.ptr(dy), _lib.ptr(wt), _lib.ptr(dx), n, h, w, cout, cin, d, _stream()), "dmc_dconv_fwd")
        if ctx.needs_input_grad[1]:
            with _span("dconv_wgrad"):
                dwcl = torch.empty((cout, cin, 3, 3), dtype=torch.float32, device=x.device, memory_format=_CL)
                work = torch.empty(lib.dmc_dconv_wgrad_workspace_bytes(n, h, w, cin, cout), dtype=torch.uint8, device=x.device)
                _lib.check(lib.dmc_dconv_wgrad(_lib.ptr(x), _lib.ptr(dy), _lib.ptr(dwcl), _lib.ptr(work), n, h, w, cin, cout, d, _stream()),
                           "dmc_dconv_wgrad")
                dw = _grad_like(dwcl, weight)
        return dx, dw, None


def dilated_conv(x, weight, dilation):
    """``F.conv2d(x, weight, None, 1, dilation, dilation)`` for a 3x3 ``weight`` [Cout, Cin, 3, 3] on the kernels of csrc/dconv.hip,
    with autograd.  ``x`` is a CUDA fp32 [N, Cin, H, W] tensor (made channels_last if it is not); the result is an ordinary
    [N, Cout, H, W] tensor in channels_last memory.  Gradients honour ``requires_grad``: a frozen weight launches no weight
    gradient, an input that needs none no data gradient.  Shapes: see dilated_conv_supported.  No CPU fallback."""
    return _DilatedConv.apply(x, weight, int(dilation))


# ---- ... and their BatchNorm2d + LeakyReLU in one op (csrc/ctx_bn.hip) ----

def bn_leaky_supported(x, bn, act):
    """True if ``act(bn(x))`` can run as ``bn_leaky(x, bn, act.negative_slope)``: a CUDA fp32 [N, C, H, W] ``x`` (any strides: it is
    made channels_last), an nn.BatchNorm2d in train() with affine parameters, running statistics and a momentum, all fp32 on the
    GPU, an nn.LeakyReLU with a slope in (0, 1), and a shape dmc_bnlrelu_supported accepts (C in {32, 64, 96, 128}, N H W >= 2,
    N H W C < 2^31).  False on the CPU."""
    if not (torch.is_tensor(x) and x.is_cuda and x.dtype == torch.float32 and x.dim() == 4 and x.numel() > 0):
        return False
    if not (isinstance(bn, torch.nn.BatchNorm2d) and bn.training and bn.affine and bn.track_running_stats and bn.momentum is not None
            and bn.num_features == x.shape[1]):
        return False
    if not all(t is not None and t.is_cuda and t.dtype == torch.float32 for t in (bn.weight, bn.bias, bn.running_mean, bn.running_var)):
        return False
    if not (isinstance(act, torch.nn.LeakyReLU) and 0.0 < act.negative_slope < 1.0):
        return False
    n, c, h, w = x.shape
    return bool(_lib.load().dmc_bnlrelu_supported(n * h * w, c))


class _BnLeaky(torch.autograd.Function):
    """LeakyReLU(BatchNorm2d(x)) with batch statistics of a ContextNetwork unit (code/dmcnet/model.py:45-104) over channels_last
    tensors.  Kept for the backward: x and the 2 C floats (mean, invstd); the slope of every element is recomputed from them."""

    @staticmethod
    def forward(ctx, x, gamma, beta, running_mean, running_var, slope, eps, momentum):
        _need_cuda(x, gamma, beta, running_mean, running_var)
        lib = _lib.load()
        if not (x.dim() == 4 and x.numel() > 0 and lib.dmc_bnlrelu_supported(x.shape[0] * x.shape[2] * x.shape[3], x.shape[1])
                and gamma.numel() == x.shape[1] and beta.numel() == x.shape[1]):
            raise _lib.DmcHipError("bn_leaky: x %s with %d BatchNorm channels is not served by the kernels (bn_leaky_supported)"
                                   % (tuple(x.shape), gamma.numel()))
        x, gamma, beta = _as_cl(x), gamma.detach().contiguous(), beta.detach().contiguous()
        n, c, h, w = x.shape
        m = n * h * w
        y = torch.empty((n, c, h, w), dtype=torch.float32, device=x.device, memory_format=_CL)
        stats = torch.empty(2 * c, dtype=torch.float32, device=x.device)
        scratch = torch.empty(lib.dmc_bnlrelu_scratch_bytes(m, c), dtype=torch.uint8, device=x.device)
        with _span("bn_leaky_fwd"):
            _lib.check(lib.dmc_bnlrelu_fwd(_lib.ptr(x), _lib.ptr(gamma), _lib.ptr(beta), _lib.ptr(running_mean), _lib.ptr(running_var),
                                           _lib.ptr(y), _lib.ptr(stats), _lib.ptr(scratch), m, c, float(slope), float(eps), float(momentum),
                                           _stream()), "dmc_bnlrelu_fwd")
        ctx.save_for_backward(x, gamma, beta, stats)
        ctx.slope = float(slope)
        return y

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dy):
        x, gamma, beta, stats = ctx.saved_tensors
        lib = _lib.load()
        n, c, h, w = x.shape
        m = n * h * w
        dy = _as_cl(dy)
        dz = torch.empty((n, c, h, w), dtype=torch.float32, device=x.device, memory_format=_CL)
        dgamma, dbeta = torch.empty_like(gamma), torch.empty_like(beta)
        scratch = torch.empty(lib.dmc_bnlrelu_scratch_bytes(m, c), dtype=torch.uint8, device=x.device)
        with _span("bn_leaky_bwd"):
            _lib.check(lib.dmc_bnlrelu_bwd(_lib.ptr(x), _lib.ptr(dy), _lib.ptr(gamma), _lib.ptr(beta), _lib.ptr(stats), _lib.ptr(scratch),
                                           _lib.ptr(dz), _lib.ptr(dgamma), _lib.ptr(dbeta), m, c, ctx.slope, _stream()), "dmc_bnlrelu_bwd")
        need = ctx.needs_input_grad
        return (dz if need[0] else None, dgamma if need[1] else None, dbeta if need[2] else None, None, None, None, None, None)


def bn_leaky(x, bn, slope):
    """``F.leaky_relu(bn(x), slope)`` for an nn.BatchNorm2d ``bn`` in train() on the kernels of csrc/ctx_bn.hip, with autograd
    (once differentiable).  ``x`` is a CUDA fp32 [N, C, H, W] tensor (made channels_last if it is not, and so is the gradient that
    arrives); the result is an ordinary tensor in channels_last memory.  Updates ``bn.running_mean``, ``bn.running_var`` and
    ``bn.num_batches_tracked`` as the module does.  A frozen weight or bias and an input that needs no gradient get None.  Shapes
    and modules: see bn_leaky_supported.  No CPU fallback."""
    _need_cuda(x)
    if not (isinstance(bn, torch.nn.BatchNorm2d) and bn.training and bn.affine and bn.track_running_stats and bn.momentum is not None):
        raise _lib.DmcHipError("bn_leaky: the BatchNorm2d must be in train() with affine parameters, running statistics and a momentum "
                               "(bn_leaky_supported)")
    y = _BnLeaky.apply(x, bn.weight, bn.bias, bn.running_mean, bn.running_var, float(slope), bn.eps, bn.momentum)
    bn.num_batches_tracked.add_(1)
    return y


# ---- ... and the two ends: the first unit's 5 -> 32 convolution, the heads' 32 -> 2 convolutions and their BatchNorm (csrc/ctx_ends.hip) ----

def _ends_geom_ok(x, c):
    if not (torch.is_tensor(x) and x.is_cuda and x.dtype == torch.float32 and x.dim() == 4 and x.shape[1] == c and x.numel() > 0):
        return False
    n, _, h, w = x.shape
    return bool(_lib.load().dmc_ctxends_supported(n, h, w))


def _ends_conv_ok(conv, cin, cout):
    return (_dconv_module_ok(conv) and conv.dilation[0] == 1 and conv.in_channels == cin and conv.out_channels == cout)


def ctx_first_conv_supported(x, conv):
    """True if ``conv(x)`` can run as ``ctx_first_conv(x, conv.weight)``: a Conv2d(5, 32, 3, 1, 1, 1, bias=False) with fp32 CUDA
    weights (the first unit of code/dmcnet/model.py:45-104), a CUDA fp32 [N, 5, H, W] input and N H W 128 < 2^31
    (dmc_ctxends_supported).  False on the CPU."""
    return _ends_conv_ok(conv, 5, 32) and _ends_geom_ok(x, 5)


def _like_weight(dw, weight):
    """dw in the strides of ``weight``."""
    return dw if dw.stride() == weight.stride() else torch.empty_like(weight).copy_(dw)


class _CtxFirstConv(torch.autograd.Function):
    """Conv2d(5, 32, 3, 1, 1, 1, bias=False) of the first ContextNetwork unit (code/dmcnet/model.py:45-104): NCHW planes in,
    channels_last out; forward, data gradient and weight gradient on csrc/ctx_ends.hip."""

    @staticmethod
    def forward(ctx, x, weight):
        _need_cuda(x, weight)
        if not (weight.dim() == 4 and tuple(weight.shape) == (32, 5, 3, 3) and _ends_geom_ok(x, 5)):
            raise _lib.DmcHipError("ctx_first_conv: x %s, weight %s is not served by the kernels (ctx_first_conv_supported)"
                                   % (tuple(x.shape), tuple(weight.shape)))
        lib = _lib.load()
        x = x.contiguous()
        n, _, h, w = x.shape
        with _span("ctx_first_fwd"):
            y = torch.empty((n, 32, h, w), dtype=torch.float32, device=x.device, memory_format=_CL)
            _lib.check(lib.dmc_ctxends_first_fwd(_lib.ptr(x), _lib.ptr(weight.detach().contiguous()), _lib.ptr(y), n, h, w, _stream()),
                       "dmc_ctxends_first_fwd")
        ctx.save_for_backward(x, weight)
        return y

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dy):
        x, weight = ctx.saved_tensors
        lib = _lib.load()
        n, _, h, w = x.shape
        dy = _as_cl(dy)
        dx = dw = None
        if ctx.needs_input_grad[0]:
            with _span("ctx_first_dgrad"):
                dx = torch.empty((n, 5, h, w), dtype=torch.float32, device=x.device)
                _lib.check(lib.dmc_ctxends_first_dgrad(_lib.ptr(dy), _lib.ptr(weight.detach().contiguous()), _lib.ptr(dx), n, h, w, _stream()),
                           "dmc_ctxends_first_dgrad")
        if ctx.needs_input_grad[1]:
            with _span("ctx_first_wgrad"):
                dwc = torch.empty((32, 5, 3, 3), dtype=torch.float32, device=x.device)
                work = torch.empty(lib.dmc_ctxends_wgrad_workspace_bytes(n, h, w, 5), dtype=torch.uint8, device=x.device)
                _lib.check(lib.dmc_ctxends_first_wgrad(_lib.ptr(x), _lib.ptr(dy), _lib.ptr(dwc), _lib.ptr(work), n, h, w, _stream()),
                           "dmc_ctxends_first_wgrad")
                dw = _like_weight(dwc, weight)
        return dx, dw


def ctx_first_conv(x, weight):
    """``F.conv2d(x, weight, None, 1, 1, 1)`` for the first ContextNetwork unit's ``weight`` [32, 5, 3, 3] on the kernels of
    csrc/ctx_ends.hip, with autograd (once differentiable).  ``x`` is a CUDA fp32 [N, 5, H, W] tensor (made contiguous if it is not);
    the result is an ordinary [N, 32, H, W] tensor in channels_last memory.  A frozen weight launches no weight gradient, an input
    that needs no gradient no data gradient; the weight gradient has the weight's strides.  No CPU fallback."""
    return _CtxFirstConv.apply(x, weight)


def ctx_head_convs_supported(t, convs):
    """True if ``[conv(t) for conv in convs]`` can run as ``ctx_head_convs(t, [conv.weight for conv in convs])``: one or two
    Conv2d(32, 2, 3, 1, 1, 1, bias=False) with fp32 CUDA weights (predict_flow / predict_att of code/dmcnet/model.py:45-104), a CUDA
    fp32 [N, 32, H, W] input and N H W 128 < 2^31.  False on the CPU."""
    convs = list(convs)
    return 1 <= len(convs) <= 2 and all(_ends_conv_ok(c, 32, 2) for c in convs) and _ends_geom_ok(t, 32)


class _CtxHeadConvs(torch.autograd.Function):
    """The Conv2d(32, 2, 3, 1, 1, 1, bias=False) of one or two ContextNetwork heads over the same trunk activation
    (code/dmcnet/model.py:45-104): channels_last in, NCHW planes out, each pass one launch that reads the trunk tensor once; the
    data gradient is the sum over the heads."""

    @staticmethod
    def forward(ctx, t, *weights):
        _need_cuda(t, *weights)
        if not (1 <= len(weights) <= 2 and all(w.dim() == 4 and tuple(w.shape) == (2, 32, 3, 3) for w in weights) and _ends_geom_ok(t, 32)):
            raise _lib.DmcHipError("ctx_head_convs: t %s with weights %s is not served by the kernels (ctx_head_convs_supported)"
                                   % (tuple(t.shape), [tuple(w.shape) for w in weights]))
        ctx.set_materialize_grads(False)
        lib = _lib.load()
        t = _as_cl(t)
        n, _, h, w = t.shape
        ws = [_as_cl(wt.detach()) for wt in weights] + [None]
        with _span("ctx_heads_fwd"):
            outs = [torch.empty((n, 2, h, w), dtype=torch.float32, device=t.device) for _ in weights] + [None]
            _lib.check(lib.dmc_ctxends_heads_fwd(_lib.ptr(t), _lib.ptr(ws[0]), _lib.ptr(ws[1]), _lib.ptr(outs[0]), _lib.ptr(outs[1]), n, h, w,
                                                 _stream()), "dmc_ctxends_heads_fwd")
        ctx.save_for_backward(t, *weights)
        return tuple(outs[:len(weights)])

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, *dzs):
        t, weights = ctx.saved_tensors[0], ctx.saved_tensors[1:]
        lib = _lib.load()
        n, _, h, w = t.shape
        k = len(weights)
        dzs = [d.contiguous() if d is not None else None for d in dzs]
        dt, dws = None, [None] * k
        if all(d is None for d in dzs):
            return (None,) * (1 + k)
        if ctx.needs_input_grad[0]:
            with _span("ctx_heads_dgrad"):
                ws = [_as_cl(wt.detach()) for wt in weights]
                if k == 1:
                    dzs2, ws2 = [dzs[0], None], [ws[0], None]
                elif dzs[0] is None:        # the flow slot is the head that has a gradient
                    dzs2, ws2 = [dzs[1], None], [ws[1], None]
                else:
                    dzs2, ws2 = dzs, ws
                dt = torch.empty((n, 32, h, w), dtype=torch.float32, device=t.device, memory_format=_CL)
                _lib.check(lib.dmc_ctxends_heads_dgrad(_lib.ptr(dzs2[0]), _lib.ptr(dzs2[1]), _lib.ptr(ws2[0]), _lib.ptr(ws2[1]), _lib.ptr(dt),
                                                       n, h, w, _stream()), "dmc_ctxends_heads_dgrad")
        live = [i for i in range(k) if ctx.needs_input_grad[1 + i] and dzs[i] is not None]
        if live:
            with _span("ctx_heads_wgrad"):
                dwcl = [torch.empty((2, 32, 3, 3), dtype=torch.float32, device=t.device, memory_format=_CL) for _ in live]
                work = torch.empty(lib.dmc_ctxends_wgrad_workspace_bytes(n, h, w, 2 * len(live)), dtype=torch.uint8, device=t.device)
                dz2 = [dzs[i] for i in live] + [None]
                dw2 = dwcl + [None]
                _lib.check(lib.dmc_ctxends_heads_wgrad(_lib.ptr(t), _lib.ptr(dz2[0]), _lib.ptr(dz2[1]), _lib.ptr(dw2[0]), _lib.ptr(dw2[1]),
                                                       _lib.ptr(work), n, h, w, _stream()), "dmc_ctxends_heads_wgrad")
                for i, d in zip(live, dwcl):
                    dws[i] = _like_weight(d, weights[i])
        return (dt,) + tuple(dws)


def ctx_head_convs(t, weights):
    """``tuple(F.conv2d(t, w, None, 1, 1, 1) for w in weights)`` for one or two head weights [2, 32, 3, 3] on the kernels of
    csrc/ctx_ends.hip, with autograd (once differentiable).  ``t`` is a CUDA fp32 [N, 32, H, W] tensor (made channels_last if it is
    not); the results are contiguous [N, 2, H, W] tensors.  Every pass is one launch over both heads; the data gradient is the
    sum of the heads' (a head whose output got no gradient is left out).  A frozen weight launches no weight gradient for it, an
    input that needs no gradient no data gradient; weight gradients have the weights' strides.  No CPU fallback."""
    return _CtxHeadConvs.apply(t, *weights)


def bn_leaky_planes_supported(z, bn, act, relu=None):
    """True if ``act(bn(z))`` (followed by ``relu``, an nn.ReLU, when given) can run as ``bn_leaky_planes(z, bn, act.negative_slope,
    relu is not None)``: a CUDA fp32 [N, 2, H, W] ``z``, an nn.BatchNorm2d(2) in train() with affine parameters, running statistics
    and a momentum, all fp32 on the GPU, an nn.LeakyReLU with a slope in (0, 1), N H W >= 2 and N H W 128 < 2^31.  False on the CPU."""
    if not (torch.is_tensor(z) and z.is_cuda and z.dtype == torch.float32 and z.dim() == 4 and z.shape[1] == 2 and z.numel() > 0):
        return False
    if not (isinstance(bn, torch.nn.BatchNorm2d) and bn.training and bn.affine and bn.track_running_stats and bn.momentum is not None
            and bn.num_features == 2):
        return False
    if not all(t is not None and t.is_cuda and t.dtype == torch.float32 for t in (bn.weight, bn.bias, bn.running_mean, bn.running_var)):
        return False
    if not (isinstance(act, torch.nn.LeakyReLU) and 0.0 < act.negative_slope < 1.0):
        return False
    if relu is not None and not isinstance(relu, torch.nn.ReLU):
        return False
    n, _, h, w = z.shape
    return _lib.load().dmc_ctxends_bn_scratch_bytes(n, h, w) > 0


class _BnLeakyPlanes(torch.autograd.Function):
    """[ReLU(]LeakyReLU(BatchNorm2d(z))[)] with batch statistics of a ContextNetwork head (code/dmcnet/model.py:45-104) over
    contiguous [N, 2, H, W] planes.  Kept for the backward: z and the 4 floats (mean, invstd)."""

    @staticmethod
    def forward(ctx, z, gamma, beta, running_mean, running_var, slope, eps, momentum, relu):
        _need_cuda(z, gamma, beta, running_mean, running_var)
        lib = _lib.load()
        if not (z.dim() == 4 and z.shape[1] == 2 and z.numel() > 0 and gamma.numel() == 2 and beta.numel() == 2
                and lib.dmc_ctxends_bn_scratch_bytes(z.shape[0], z.shape[2], z.shape[3]) > 0):
            raise _lib.DmcHipError("bn_leaky_planes: z %s with %d BatchNorm channels is not served by the kernels (bn_leaky_planes_supported)"
                                   % (tuple(z.shape), gamma.numel()))
        z, gamma, beta = z.contiguous(), gamma.detach().contiguous(), beta.detach().contiguous()
        n, _, h, w = z.shape
        y = torch.empty_like(z)
        stats = torch.empty(4, dtype=torch.float32, device=z.device)
        scratch = torch.empty(lib.dmc_ctxends_bn_scratch_bytes(n, h, w), dtype=torch.uint8, device=z.device)
        with _span("bn_leaky_planes_fwd"):
            _lib.check(lib.dmc_ctxends_bn_fwd(_lib.ptr(z), _lib.ptr(gamma), _lib.ptr(beta), _lib.ptr(running_mean), _lib.ptr(running_var),
                                              _lib.ptr(y), _lib.ptr(stats), _lib.ptr(scratch), n, h, w, float(slope), float(eps),
                                              float(momentum), int(bool(relu)), _stream()), "dmc_ctxends_bn_fwd")
        ctx.save_for_backward(z, gamma, beta, stats)
        ctx.slope, ctx.relu = float(slope), int(bool(relu))
        return y

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dy):
        z, gamma, beta, stats = ctx.saved_tensors
        lib = _lib.load()
        n, _, h, w = z.shape
        dy = dy.contiguous()
        dz = torch.empty_like(z)
        dgamma, dbeta = torch.empty_like(gamma), torch.empty_like(beta)
        scratch = torch.empty(lib.dmc_ctxends_bn_scratch_bytes(n, h, w), dtype=torch.uint8, device=z.device)
        with _span("bn_leaky_planes_bwd"):
            _lib.check(lib.dmc_ctxends_bn_bwd(_lib.ptr(z), _lib.ptr(dy), _lib.ptr(gamma), _lib.ptr(beta), _lib.ptr(stats), _lib.ptr(scratch),
                                              _lib.ptr(dz), _lib.ptr(dgamma), _lib.ptr(dbeta), n, h, w, ctx.slope, ctx.relu, _stream()),
                       "dmc_ctxends_bn_bwd")
        need = ctx.needs_input_grad
        return (dz if need[0] else None, dgamma if need[1] else None, dbeta if need[2] else None, None, None, None, None, None, None)


def bn_leaky_planes(z, bn, slope, relu=False):
    """``F.leaky_relu(bn(z), slope)`` -- and ``F.relu`` of that with ``relu=True`` -- for an nn.BatchNorm2d(2) ``bn`` in train() on the
    kernels of csrc/ctx_ends.hip, with autograd (once differentiable).  ``z`` is a CUDA fp32 [N, 2, H, W] tensor (made contiguous
    if it is not, and so is the gradient that arrives); the result is contiguous.  Updates ``bn.running_mean``, ``bn.running_var``
    and ``bn.num_batches_tracked`` as the module does.  A frozen weight or bias and an input that needs no gradient get None.
    Shapes and modules: see bn_leaky_planes_supported.  No CPU fallback."""
    _need_cuda(z)
    if not (isinstance(bn, torch.nn.BatchNorm2d) and bn.training and bn.affine and bn.track_running_stats and bn.momentum is not None):
        raise _lib.DmcHipError("bn_leaky_planes: the BatchNorm2d must be in train() with affine parameters, running statistics and a "
                               "momentum (bn_leaky_planes_supported)")
    y = _BnLeakyPlanes.apply(z, bn.weight, bn.bias, bn.running_mean, bn.running_var, float(slope), bn.eps, bn.momentum, bool(relu))
    bn.num_batches_tracked.add_(1)
    return y


def _ctx_train_plan(net):
    """(first unit, [(conv, bn, act), ...] middle units, [head modules]) of a ContextNetwork / ContextNetworkAtt with BatchNorm
    whose middle units are of the form dilated_conv serves, or None."""
    trunk = getattr(net, "conv_context", None)
    if not isinstance(trunk, torch.nn.Sequential):
        return None
    units = list(trunk)
    if hasattr(net, "predict_att"):
        heads = [net.predict_flow, net.predict_att]
    else:
        if len(units) < 3:
            return None
        heads = [units.pop()]
    if len(units) < 2:
        return None
    middle = []
    for u in units[1:]:
        if not (isinstance(u, torch.nn.Sequential) and len(u) == 3 and isinstance(u[0], torch.nn.Conv2d)
                and isinstance(u[1], torch.nn.BatchNorm2d) and isinstance(u[2], torch.nn.LeakyReLU)):
            return None
        middle.append((u[0], u[1], u[2]))
    return units[0], middle, heads


def context_train_supported(net, x):
    """True if ``net`` (model.ContextNetwork / ContextNetworkAtt, batch_norm=True) can run its middle units' convolutions on
    ops.dilated_conv for the input ``x``: autograd enabled, a CUDA fp32 [N, 5, H, W] input, every middle unit accepted by
    dilated_conv_supported (a batch past the index bound therefore takes the stock route as a whole)."""
    if not torch.is_grad_enabled():
        return False
    if not (torch.is_tensor(x) and x.is_cuda and x.dtype == torch.float32 and x.dim() == 4 and x.shape[1] == 5 and x.numel() > 0):
        return False
    plan = _ctx_train_plan(net)
    if plan is None:
        return False
    first, middle, _ = plan
    if not (isinstance(first, torch.nn.Sequential) and isinstance(first[0], torch.nn.Conv2d) and first[0].out_channels == middle[0][0].in_channels
            and tuple(first[0].stride) == (1, 1) and tuple(first[0].kernel_size) == (3, 3) and tuple(first[0].padding) == tuple(first[0].dilation)):
        return False
    n, _, h, w = x.shape
    lib = _lib.load()
    c = first[0].out_channels
    for conv, _, _ in middle:
        if conv.in_channels != c or not _dconv_module_ok(conv):
            return False
        if not lib.dmc_dconv_supported(n, h, w, conv.in_channels, conv.out_channels, conv.dilation[0]):
            return False
        c = conv.out_channels
    return True


def _ctx_head_parts(head):
    """(unit, relu | None) of a head: the unit itself, or Sequential(unit, nn.ReLU) (predict_att)."""
    if (isinstance(head, torch.nn.Sequential) and len(head) == 2 and isinstance(head[0], torch.nn.Sequential)
            and isinstance(head[1], torch.nn.ReLU)):
        return head[0], head[1]
    return head, None


def _ctx_heads_own(heads, t, fused_bn):
    """The heads on ops.ctx_head_convs (one call over every head whose convolution it serves) and, with ``fused_bn``, their
    BatchNorm + LeakyReLU (+ ReLU) on ops.bn_leaky_planes; whatever is of another form keeps its stock modules."""
    parts = [_ctx_head_parts(h) for h in heads]
    own = [i for i, (u, _) in enumerate(parts) if isinstance(u, torch.nn.Sequential) and len(u) >= 1 and _ends_conv_ok(u[0], 32, 2)]
    if not own or len(own) > 2 or not _ends_geom_ok(t, 32):
        return [h(t) for h in heads]
    zs = dict(zip(own, ctx_head_convs(t, [parts[i][0][0].weight for i in own])))
    outs = []
    for i, h in enumerate(heads):
        if i not in zs:
            outs.append(h(t))
            continue
        unit, relu = parts[i]
        z = zs[i]
        if fused_bn and len(unit) == 3 and bn_leaky_planes_supported(z, unit[1], unit[2], relu):
            outs.append(bn_leaky_planes(z, unit[1], unit[2].negative_slope, relu is not None))
            continue
        for m in list(unit)[1:]:
            z = m(z)
        outs.append(relu(z) if relu is not None else z)
    return outs


def context_train(net, x, checked=False, fused_bn=False, own_ends=False):
    """``net(x)`` of a ContextNetwork (-> gen_flow) or ContextNetworkAtt (-> (gen_flow, att_flow)) with autograd, unit by unit: the
    first unit and the head(s) as their stock modules on a channels_last input, every middle unit as ops.dilated_conv followed by
    the module's OWN BatchNorm2d and LeakyReLU (running statistics, momentum, num_batches_tracked and the in-place activation as
    before).  Requires context_train_supported(net, x); ``checked=True``: the caller has just asked it (the modules' forward).

    ``fused_bn=True`` (model.CTX_TRAIN_BN): the BatchNorm2d + LeakyReLU of the first unit (behind its own stock Conv2d) and of
    every middle unit run as ops.bn_leaky wherever bn_leaky_supported accepts them; a unit it refuses (a BatchNorm in eval()
    inside a training network) keeps its stock modules, the others are unaffected.  The heads stay stock.

    ``own_ends=True`` (model.CTX_TRAIN_ENDS): the first unit's Conv2d(5, 32, 3, 1, 1, 1, bias=False) runs as ops.ctx_first_conv and
    the heads' Conv2d(32, 2, 3, 1, 1, 1, bias=False) as one ops.ctx_head_convs call (csrc/ctx_ends.hip); together with
    ``fused_bn`` each head's BatchNorm2d + LeakyReLU (+ the attention head's ReLU) runs as ops.bn_leaky_planes where
    bn_leaky_planes_supported accepts it (a head it refuses keeps its stock modules behind our convolution).  A first unit or a
    head of another form keeps its stock module.  ``own_ends=False``: exactly the route described above."""
    if not checked and not context_train_supported(net, x):
        raise _lib.DmcHipError("context_train: the network or the input is not served by the kernels (context_train_supported)")
    first, middle, heads = _ctx_train_plan(net)
    with _span("context_train"):
        def tail(t, bn, act):
            return bn_leaky(t, bn, act.negative_slope) if fused_bn and bn_leaky_supported(t, bn, act) else act(bn(t))
        if own_ends and ctx_first_conv_supported(x, first[0]):
            t = ctx_first_conv(x, first[0].weight)
            if len(first) == 3 and isinstance(first[1], torch.nn.BatchNorm2d) and isinstance(first[2], torch.nn.LeakyReLU):
                t = tail(t, first[1], first[2])
            else:
                for m in list(first)[1:]:
                    t = m(t)
        elif fused_bn and len(first) == 3 and isinstance(first[1], torch.nn.BatchNorm2d) and isinstance(first[2], torch.nn.LeakyReLU):
            t = tail(first[0](_as_cl(x)), first[1], first[2])
        else:
            t = first(_as_cl(x))
        for conv, bn, act in middle:
            t = tail(dilated_conv(t, conv.weight, conv.dilation[0]), bn, act)
        outs = _ctx_heads_own(heads, t, fused_bn) if own_ends else [h(t) for h in heads]
    return outs[0] if len(outs) == 1 else tuple(outs)
