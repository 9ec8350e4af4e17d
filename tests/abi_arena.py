"""Guarded arenas for memory-contract tests of the C ABI (include/dmcnet_hip.h: the caller owns every buffer, workspace sizes
come from the size queries, nothing outside those buffers is touched, outputs are overwritten).

An ``Arena`` is ONE ``torch.uint8`` allocation, every byte set to a fill value.  A case carves its buffers out of it: each
has exactly the promised byte size, starts at a 256-byte-aligned address and keeps at least ``MARGIN`` bytes of fill on both
sides.  ``run_case`` runs a case twice, over an arena filled with 0xFF (NaN as bf16 / fp32 / fp64, -1 as int32) and one filled
with 0x00, and checks, in this order:

  ``rc``     the entry point returned what the case expects (DMC_OK unless it says otherwise);
  ``guard``  every byte outside the carved buffers still equals the fill;
  ``in``     every IN buffer still holds the bytes that were copied in;
  ``ab``     every OUT / INOUT buffer has the same bytes in both runs -- an element that was never written (0xFF against
             0x00), a result that depends on stale workspace, a read outside an input that should have produced zeros;
  ``nan``    no floating-point OUT / INOUT buffer of the 0xFF run holds a NaN, unless the case declared it as specified.

A failure raises ``ArenaViolation`` (an AssertionError) whose ``check`` attribute is the name above.

Not covered: a read outside a buffer whose value is discarded and cannot change any result leaves no trace in memory, so
these checks cannot see it.  Nothing here provokes a fault: a guard-band overrun is a write into memory this process owns.

The module works on any device (tests/test_abi_arena_cpu.py drives it with CPU tensors and Python stand-ins)."""
import ctypes

import torch

MARGIN = 1 << 20          # bytes of fill on each side of every buffer (as tests/test_x3s_wgrad_addr_gpu.py)
ALIGN = 256
IN, OUT, INOUT, WORK = "IN", "OUT", "INOUT", "WORK"
FILLS = (0xFF, 0x00)
DMC_OK = 0
_FLOAT = (torch.float32, torch.float64, torch.bfloat16, torch.float16)


class ArenaViolation(AssertionError):
    def __init__(self, check, message):
        AssertionError.__init__(self, "[%s] %s" % (check, message))
        self.check = check


class Buf(object):
    """One carved buffer: ``u8`` is the exact byte range, ``t`` the same memory as ``dtype`` elements (of ``shape``)."""

    def __init__(self, name, role, offset, u8, dtype, shape, init, nan_ok):
        self.name, self.role, self.offset, self.u8, self.dtype, self.init, self.nan_ok = name, role, offset, u8, dtype, init, nan_ok
        self.nbytes = u8.numel()
        item = torch.empty(0, dtype=dtype).element_size()
        self.t = u8[:self.nbytes // item * item].view(dtype)
        if shape is not None:
            self.t = self.t[:int(torch.Size(shape).numel())].view(shape)

    @property
    def ptr(self):
        return ctypes.c_void_p(self.u8.data_ptr())

    def at(self, byte_offset):
        """A pointer into the buffer (a channel slice of a wider tensor)."""
        assert 0 <= byte_offset < self.nbytes
        return ctypes.c_void_p(self.u8.data_ptr() + byte_offset)


class Arena(object):
    def __init__(self, fill, device, capacity, dry=False):
        self.fill, self.device, self.dry = fill, torch.device(device), dry     # dry: calls are checked against the signatures, not made
        raw = torch.empty(capacity + ALIGN, dtype=torch.uint8, device=self.device)
        skew = (-raw.data_ptr()) % ALIGN
        self.mem = raw[skew:skew + capacity]
        self.mem.fill_(fill)
        self.bufs, self.rcs = [], []
        self._next = MARGIN

    # ---- carving
    def carve(self, name, role, nbytes=None, like=None, dtype=torch.float32, shape=None, nan_ok=False, slack=0):
        """``like``: a tensor whose bytes size (and, for IN / INOUT, initialise) the buffer; otherwise ``nbytes`` (what a size
        query returned) or ``shape`` x ``dtype``.  ``slack``: documented spare bytes behind the data, part of the buffer."""
        init = None
        if like is not None:
            like = like.contiguous()
            dtype, shape = like.dtype, tuple(like.shape)
            nbytes = like.numel() * like.element_size()
            if role in (IN, INOUT):
                init = like.reshape(-1).view(torch.uint8).to(self.device).clone()
        elif nbytes is None:
            nbytes = int(torch.Size(shape).numel()) * torch.empty(0, dtype=dtype).element_size()
        elif role in (IN, INOUT):
            raise ValueError("%s: an %s buffer needs its initial contents" % (name, role))
        nbytes = int(nbytes) + slack
        if nbytes <= 0:
            raise ValueError("%s: empty buffer" % name)
        off = self._next
        if off + nbytes + MARGIN > self.mem.numel():
            raise ValueError("arena of %d bytes is too small for %s (%d bytes at %d)" % (self.mem.numel(), name, nbytes, off))
        self._next = (off + nbytes + MARGIN + ALIGN - 1) // ALIGN * ALIGN
        u8 = self.mem[off:off + nbytes]
        assert u8.data_ptr() % ALIGN == 0
        if init is not None:
            u8[:init.numel()].copy_(init)
            if slack:       # spare bytes are the caller's: their contents are part of what was "copied in"
                init = u8.clone()
        b = Buf(name, role, off, u8, dtype, shape, init, nan_ok)
        self.bufs.append(b)
        return b

    def inp(self, name, tensor, **kw):
        return self.carve(name, IN, like=tensor, **kw)

    def inout(self, name, tensor, **kw):
        return self.carve(name, INOUT, like=tensor, **kw)

    def out(self, name, shape=None, dtype=torch.float32, nbytes=None, **kw):
        return self.carve(name, OUT, nbytes=nbytes, dtype=dtype, shape=shape, **kw)

    def work(self, name, nbytes, **kw):
        return self.carve(name, WORK, nbytes=nbytes, dtype=torch.uint8, **kw)

    # ---- calling
    def call(self, name, *args):
        """Calls entry point ``name`` of the library as a foreign caller would: buffers as raw pointers, None as NULL, a
        list of buffers as a host array of device pointers, a CPU tensor as a host pointer; the current raw stream is
        appended.  The return code is recorded (and returned)."""
        from dmcnet_amd import _lib, ops
        conv, keep = [], []
        for a in args:
            if a is None:
                conv.append(ctypes.c_void_p(0))
            elif isinstance(a, Buf):
                conv.append(a.ptr)
            elif isinstance(a, (list, tuple)):
                arr = (ctypes.c_void_p * len(a))(*[b.u8.data_ptr() for b in a])
                keep.append(arr)
                conv.append(ctypes.cast(arr, ctypes.c_void_p))
            elif isinstance(a, torch.Tensor):
                assert not a.is_cuda
                keep.append(a)
                conv.append(ctypes.c_void_p(a.data_ptr()))
            else:
                conv.append(a)
        if self.dry:
            res, types = _lib.SIGNATURES[name]
            assert len(types) == len(conv) + 1 and types[-1] is ctypes.c_void_p, "%s takes %d arguments + the stream, got %d" % (name, len(types) - 1, len(conv))
            for i, (t, v) in enumerate(zip(types, conv)):
                if t is ctypes.c_void_p:
                    assert isinstance(v, ctypes.c_void_p), "%s: argument %d must be a pointer, got %r" % (name, i, v)
                elif t is ctypes.c_float:
                    assert isinstance(v, float), "%s: argument %d must be a float, got %r" % (name, i, v)
                else:
                    assert isinstance(v, int) and not isinstance(v, bool), "%s: argument %d must be an integer, got %r" % (name, i, v)
            rc = DMC_OK
        else:
            rc = getattr(_lib.load(), name)(*(conv + [ops._stream()]))
        self.rcs.append((name, int(rc)))
        return rc

    def returned(self, name, rc):
        """For stand-ins that are not library calls."""
        self.rcs.append((name, int(rc)))

    # ---- checks
    def damaged(self):
        """None, or a description of the first byte outside the carved buffers that lost its fill."""
        bad = self.mem != self.fill
        for b in self.bufs:
            bad[b.offset:b.offset + b.nbytes] = False
        if not bool(bad.any()):
            return None
        first = int(bad.nonzero()[0])
        best = None
        for b in self.bufs:
            d = b.offset - first if first < b.offset else first - (b.offset + b.nbytes) + 1
            where = "in front of" if first < b.offset else "behind"
            if best is None or d < best[0]:
                best = (d, where, b)
        return "%d guard bytes damaged (fill 0x%02X); the first is %d bytes %s %s buffer '%s' (%d bytes), value 0x%02X" % (
            int(bad.sum()), self.fill, best[0], best[1], best[2].role, best[2].name, best[2].nbytes, int(self.mem[first]))


def _sync(device):
    if torch.device(device).type == "cuda":
        torch.cuda.synchronize()


def _first_diff(a, b):
    d = (a != b).nonzero()
    return int(d[0]), int(d.numel())


def run_case(case, device="cuda:0", capacity=64 << 20, expect_rc=DMC_OK):
    """Runs ``case(arena)`` over a 0xFF-filled and a 0x00-filled arena and makes the five checks of the module docstring.
    ``expect_rc`` != DMC_OK: the (last) call must return that code and must have written nothing at all.
    Returns {buffer name: Buf} of the 0xFF run."""
    arenas = []
    for fill in FILLS:
        a = Arena(fill, device, capacity)
        case(a)
        _sync(device)
        arenas.append(a)
    for a in arenas:
        if not a.rcs:
            raise ArenaViolation("rc", "the case made no call")
        for name, rc in a.rcs[:-1]:
            if rc != DMC_OK:
                raise ArenaViolation("rc", "%s returned %d (fill 0x%02X)" % (name, rc, a.fill))
        name, rc = a.rcs[-1]
        if rc != expect_rc:
            text = ""
            if torch.device(device).type == "cuda":
                from dmcnet_amd import _lib
                text = ": " + _lib.load().dmc_last_error().decode()
            raise ArenaViolation("rc", "%s returned %d, expected %d (fill 0x%02X)%s" % (name, rc, expect_rc, a.fill, text))
    for a in arenas:
        msg = a.damaged()
        if msg is not None:
            raise ArenaViolation("guard", msg)
    for a in arenas:
        for b in a.bufs:
            if b.role == IN and not torch.equal(b.u8, b.init):
                i, n = _first_diff(b.u8, b.init)
                raise ArenaViolation("in", "IN buffer '%s' was altered: %d bytes, the first at byte %d (fill 0x%02X)" % (b.name, n, i, a.fill))
    A, B = arenas
    assert [(b.name, b.role, b.nbytes) for b in A.bufs] == [(b.name, b.role, b.nbytes) for b in B.bufs], "the case is not deterministic"
    if expect_rc != DMC_OK:        # a refused call: every buffer it could have written still holds the fill
        for a in arenas:
            for b in a.bufs:
                if b.role in (OUT, WORK) and not bool((b.u8 == a.fill).all()):
                    raise ArenaViolation("ab", "%s buffer '%s' was written by a refused call" % (b.role, b.name))
                if b.role == INOUT and not torch.equal(b.u8, b.init):
                    raise ArenaViolation("ab", "INOUT buffer '%s' was written by a refused call" % b.name)
        return {b.name: b for b in A.bufs}
    for ba, bb in zip(A.bufs, B.bufs):
        if ba.role in (OUT, INOUT) and not torch.equal(ba.u8, bb.u8):
            i, n = _first_diff(ba.u8, bb.u8)
            raise ArenaViolation("ab", "%s buffer '%s' differs between the 0xFF and the 0x00 run: %d of %d bytes, the first at byte %d "
                                 "(0x%02X against 0x%02X) -- an unwritten element, stale workspace, or a read outside an input"
                                 % (ba.role, ba.name, n, ba.nbytes, i, int(ba.u8[i]), int(bb.u8[i])))
    for b in A.bufs:
        if b.role in (OUT, INOUT) and b.dtype in _FLOAT and not b.nan_ok and bool(torch.isnan(b.t).any()):
            raise ArenaViolation("nan", "%s buffer '%s' holds %d NaN" % (b.role, b.name, int(torch.isnan(b.t).sum())))
    return {b.name: b for b in A.bufs}
