"""Reference arithmetic of the bf16x3 convolutions, in plain numpy on the CPU.

An fp32 value is the exact sum of three bf16 slices: s0 = its upper 16 bits, s1 = the upper 16 bits of the exact remainder
v - s0, s2 = the second remainder (8 significant bits each, truncation, never rounding).  A product of two such sums is
formed from SIX of the nine slice products; per 16 k-values each kept product is one matrix instruction that adds a
16-term dot product of bf16 values (exact: 16-bit products) into an fp32 accumulator.  ``six_product`` is that GEMM with
the set of kept products, their order and a k-range in which another set is kept as parameters, so that a defect -- one
product lost in one tap, in one 16-channel chunk, a mis-paired slice plane -- can be seeded and measured.

The convolutions and their two gradients are expressed as that GEMM by the im2col helpers; K is ordered [tap][channel]
(forward, data gradient), so "one tap" is a k-range.  Nothing here reads a kernel's result except the two metrics, which
are functions of fp64 quantities and of ``got`` only.

The im2col helpers take a ``dilation`` (the dilated 3 x 3 convolutions of the ContextNetwork, tests/test_ctx_products_gpu.py);
``loop_family`` is the value family for kernels that split both operands in the loop, ``ctx_pack`` those kernels' weight panels.

Pairs (i, j) name (slice of the first GEMM operand, slice of the second); the set SIX is symmetric, so which operand is the
activation does not matter for what is kept, only for the order of issue."""
import numpy as np

SIX = ((0, 0), (0, 1), (1, 0), (0, 2), (2, 0), (1, 1))
NINE = tuple((i, j) for i in range(3) for j in range(3))
#: order of issue inside one 16-chunk.  Weight-gradient and small-channel kernels: smallest products first.
ORDER_SMALL_FIRST = ((0, 2), (2, 0), (1, 1), (0, 1), (1, 0), (0, 0))
#: forward / data-gradient loops (first operand = activation): the weight slice is the outer index.
ORDER_WEIGHT_OUTER = ((2, 0), (1, 0), (0, 0), (1, 1), (0, 1), (0, 2))
MIN_GROUP = 1000


def _np32(v):
    if hasattr(v, "detach"):
        v = v.detach().cpu().numpy()
    return np.ascontiguousarray(v, dtype=np.float32)


def _trunc16(v):
    return (v.view(np.uint32) & np.uint32(0xFFFF0000)).view(np.float32)


def split(v):
    """(s0, s1, s2) of an fp32 array, each an fp32 array holding a bf16 value.  Asserts s0 + s1 + s2 == v bit for bit; the one
    bit pattern a sum cannot return is -0.0 (s0 keeps its sign bit, the remainders are +0, the sum is +0), which is asserted
    to compare equal instead."""
    v = _np32(v)
    assert np.isfinite(v).all()
    s0 = _trunc16(v)
    r1 = v - s0                       # exact: the low 16 bits of v's significand
    s1 = _trunc16(r1)
    s2 = r1 - s1                      # exact, <= 8 significant bits
    assert np.array_equal(_trunc16(s2), s2), "the second remainder is not a bf16 value"
    back = (s0 + s1) + s2             # <= 16, then 24 significant bits: no rounding
    assert np.array_equal(back, v)
    nz = v != 0
    assert np.array_equal(back.view(np.uint32)[nz], v.view(np.uint32)[nz])
    assert np.array_equal(s0.view(np.uint32)[~nz], v.view(np.uint32)[~nz])
    exact = s0.astype(np.float64) + s1.astype(np.float64) + s2.astype(np.float64)
    assert np.array_equal(exact, v.astype(np.float64))
    return s0, s1, s2


def split_rounded_s1(v):
    """A SEEDED DEFECT: s1 rounded to nearest bf16 instead of truncated, s2 left as the truncating split made it."""
    v = _np32(v)
    s0, s1, s2 = split(v)
    r1 = v - s0
    bits = r1.view(np.uint32).astype(np.uint64)
    rounded = ((bits + 0x7FFF + ((bits >> 16) & 1)) & 0xFFFF0000).astype(np.uint32).view(np.float32)
    return s0, rounded, s2


def six_product(a_slices, b_slices, keep=SIX, chunk=16, order=None, defect=None, reverse=False, peak=False):
    """[M, K] x [K, N] in bf16x3 arithmetic: per ``chunk`` k-values, each kept slice product (i, j) adds the exact dot product
    of a_slices[i] and b_slices[j] into an fp32 accumulator (one rounding per product and chunk).

    keep     the products formed (SIX in a correct kernel).
    order    sequence of pairs: the order of issue inside a chunk (default SIX as listed); a kept pair it does not name
             is issued last.
    defect   (k_lo, k_hi, keep_there): chunks inside [k_lo, k_hi) form ``keep_there`` instead (multiples of ``chunk``).
    reverse  walk the chunks from the last to the first.
    peak     also return the largest |accumulator| reached at any point (for the 2^24 exactness condition).
    Returns the fp32 accumulator as float64 [M, N]."""
    A = [np.ascontiguousarray(s, dtype=np.float64) for s in a_slices]
    B = [np.ascontiguousarray(s, dtype=np.float64) for s in b_slices]
    M, K = A[0].shape
    N = B[0].shape[1]
    assert B[0].shape[0] == K and K % chunk == 0
    order = tuple(order) if order is not None else SIX

    def sequence(kept):
        kept = tuple(kept)
        assert all(p in NINE for p in kept)
        return [p for p in order if p in kept] + [p for p in kept if p not in order]

    seq_ok = sequence(keep)
    k_lo = k_hi = 0
    seq_bad = seq_ok
    if defect is not None:
        k_lo, k_hi, kept_there = defect
        assert k_lo % chunk == 0 and k_hi % chunk == 0 and 0 <= k_lo <= k_hi <= K
        seq_bad = sequence(kept_there)
    nchunk = K // chunk
    A3 = [a.reshape(M, nchunk, chunk).transpose(1, 0, 2) for a in A]     # [chunk index, M, chunk]
    B3 = [b.reshape(nchunk, chunk, N) for b in B]
    acc = np.zeros((M, N), np.float32)
    top = 0.0
    step = max(1, (1 << 22) // max(1, M * N))                            # chunks per batched matmul
    starts = list(range(0, nchunk, step))
    for c0 in (reversed(starts) if reverse else starts):
        c1 = min(nchunk, c0 + step)
        need = set(seq_ok) | set(seq_bad)
        P = {p: np.matmul(A3[p[0]][c0:c1], B3[p[1]][c0:c1]) for p in need}
        cs = range(c1 - 1, c0 - 1, -1) if reverse else range(c0, c1)
        for c in cs:
            inside = k_lo <= c * chunk and (c + 1) * chunk <= k_hi
            for p in (seq_bad if inside else seq_ok):
                acc = (acc.astype(np.float64) + P[p][c - c0]).astype(np.float32)
                if peak:
                    top = max(top, float(np.abs(acc).max()))
    out = acc.astype(np.float64)
    return (out, top) if peak else out


# ---------------------------------------------------------------- convolutions as that GEMM (NCHW arrays in, K = [tap][channel])
def out_size(h, k, stride, pad):
    return (h + 2 * pad - k) // stride + 1


def im2col(x, k, stride, pad, dilation=1):
    """x [N, C, H, W] -> [N OH OW, k k C]: column tap * C + c of row (n, oy, ox) is x[n, c, oy stride - pad + ky d, ox stride - pad + kx d]
    (zero outside the image), tap = ky k + kx, d = ``dilation`` (the dilated 3 x 3 taps of the ContextNetwork read
    (y + (ky - 1) d, x + (kx - 1) d) with pad = d)."""
    x = np.asarray(x)
    n, c, h, w = x.shape
    d = dilation
    oh, ow = out_size(h, d * (k - 1) + 1, stride, pad), out_size(w, d * (k - 1) + 1, stride, pad)
    xp = np.zeros((n, c, h + 2 * pad + stride, w + 2 * pad + stride), x.dtype)
    xp[:, :, pad:pad + h, pad:pad + w] = x
    cols = []
    for ky in range(k):
        for kx in range(k):
            t = xp[:, :, ky * d:ky * d + stride * oh:stride, kx * d:kx * d + stride * ow:stride]
            cols.append(t.transpose(0, 2, 3, 1).reshape(n * oh * ow, c))
    return np.concatenate(cols, axis=1)


def weight_matrix(w):
    """w [Cout, Cin, k, k] -> [k k Cin, Cout] matching im2col's K order."""
    w = np.asarray(w)
    cout, cin, k, _ = w.shape
    return w.transpose(2, 3, 1, 0).reshape(k * k * cin, cout)


def col2nchw(y, n, oh, ow):
    """GEMM result [n oh ow, C] -> [n, C, oh, ow]."""
    return y.reshape(n, oh, ow, -1).transpose(0, 3, 1, 2)


def im2col_dgrad(dy, k, stride, pad, h, w, dilation=1):
    """dy [N, Cout, OH, OW] -> [N H W, k k Cout]: column tap * Cout + co of row (n, y, x) is dy[n, co, (y + pad - ky d) / stride,
    (x + pad - kx d) / stride] where both divide and land inside dy, zero elsewhere (d = ``dilation``)."""
    dy = np.asarray(dy)
    n, cout, oh, ow = dy.shape
    g = dy.transpose(0, 2, 3, 1)
    cols = []
    for ky in range(k):
        for kx in range(k):
            z = np.zeros((n, h, w, cout), dy.dtype)
            oy, ox = np.arange(oh), np.arange(ow)
            ys, xs = oy * stride - pad + ky * dilation, ox * stride - pad + kx * dilation
            vy, vx = (ys >= 0) & (ys < h), (xs >= 0) & (xs < w)
            z[:, ys[vy][:, None], xs[vx][None, :], :] = g[:, oy[vy][:, None], ox[vx][None, :], :]
            cols.append(z.reshape(n * h * w, cout))
    return np.concatenate(cols, axis=1)


def weight_matrix_dgrad(w):
    """w [Cout, Cin, k, k] -> [k k Cout, Cin] matching im2col_dgrad's K order."""
    w = np.asarray(w)
    cout, cin, k, _ = w.shape
    return w.transpose(2, 3, 0, 1).reshape(k * k * cout, cin)


def wgrad_operands(x, dy, k, stride, pad, dilation=1):
    """Weight gradient as a GEMM over the pixels: (dy as [Cout, P], im2col(x) as [P, k k Cin]); the product is dw as
    [Cout, tap * Cin + ci], so here one tap is a range of OUTPUT columns and K runs over (n, oy, ox)."""
    dy = np.asarray(dy)
    cout = dy.shape[1]
    return np.ascontiguousarray(dy.transpose(1, 0, 2, 3).reshape(cout, -1)), im2col(x, k, stride, pad, dilation)


def dw_from_matrix(m, cin, k):
    """[Cout, k k Cin] -> [Cout, Cin, k, k]."""
    return m.reshape(m.shape[0], k, k, cin).transpose(0, 3, 1, 2)


def pad_k(a, b, chunk=16):
    """Zero-pad the contraction length of (a [M, K], b [K, N]) to a multiple of ``chunk`` (zeros add nothing)."""
    k = a.shape[1]
    r = (-k) % chunk
    if r:
        a = np.concatenate([a, np.zeros((a.shape[0], r), a.dtype)], axis=1)
        b = np.concatenate([b, np.zeros((r, b.shape[1]), b.dtype)], axis=0)
    return a, b


def emulate(a, b, **kw):
    """six_product of two fp32 matrices (split here); K padded to the chunk."""
    a, b = pad_k(_np32(a), _np32(b), kw.get("chunk", 16))
    return six_product(split(a), split(b), **kw)


def fp64_and_bound(a, b):
    """(ref, B) of a GEMM: the fp64 product and the fp64 product of the absolute values, B = sum |a| |b| per output."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return a @ b, np.abs(a) @ np.abs(b)


# ---------------------------------------------------------------- metrics (fp64 quantities and ``got`` only)
def _f64(t):
    if hasattr(t, "detach"):
        t = t.detach().double().cpu().numpy()
    return np.asarray(t, np.float64)


def rms_metric(got, ref, bound):
    """rms(got - ref) / rms(B) over one group of outputs."""
    got, ref, bound = _f64(got), _f64(ref), _f64(bound)
    den = np.sqrt(np.mean(bound * bound))
    assert den > 0
    return float(np.sqrt(np.mean((got - ref) ** 2)) / den)


def max_metric(got, ref, bound):
    """max(|got - ref| / B) over one group of outputs; an output with B = 0 has no nonzero term and must be zero."""
    got, ref, bound = _f64(got), _f64(ref), _f64(bound)
    live = bound > 0
    assert np.all(got[~live] == 0), "an output without a single nonzero term is not zero"
    return float((np.abs(got - ref)[live] / bound[live]).max()) if live.any() else 0.0


def old_metric(got, ref):
    """max|got - ref| / max|ref|: the suite's 1e-5 bar, printed alongside."""
    got, ref = _f64(got), _f64(ref)
    return float(np.abs(got - ref).max() / max(np.abs(ref).max(), 1e-300))


def channel_groups(nchan, per_channel, width=64, min_count=MIN_GROUP):
    """[(c0, c1)] ranges of output channels: ``width``-wide blocks, neighbours merged until each holds >= ``min_count`` outputs
    (``per_channel`` outputs per channel); asserts the count."""
    edges = list(range(0, nchan, width)) + [nchan]
    groups, c0 = [], 0
    for e in edges[1:]:
        if (e - c0) * per_channel >= min_count:
            groups.append((c0, e))
            c0 = e
    if c0 < nchan:
        assert groups, "fewer than %d outputs in the whole tensor" % min_count
        groups[-1] = (groups[-1][0], nchan)
    assert all((b - a) * per_channel >= min_count for a, b in groups)
    return groups


# ---------------------------------------------------------------- crafted operands of the exact cases
def small_ints(rs, shape, amax=3, p_zero=0.5):
    """Integers in [-amax, amax], both signs, ``p_zero`` of them zero: exact bf16 values (slices 1 and 2 are zero)."""
    v = rs.randint(1, amax + 1, size=shape) * rs.choice([-1, 1], size=shape)
    return (v * (rs.uniform(size=shape) >= p_zero)).astype(np.float32)


def one_hot_channels(rs, shape, values=(1.0, 2.0)):
    """[N, C, H, W]: one nonzero channel per pixel, value +-1 / +-2."""
    n, c, h, w = shape
    out = np.zeros((n, h, w, c), np.float32)
    idx = rs.randint(0, c, size=(n, h, w))
    val = rs.choice(values, size=(n, h, w)) * rs.choice([-1.0, 1.0], size=(n, h, w))
    np.put_along_axis(out, idx[..., None], val[..., None].astype(np.float32), axis=3)
    return np.ascontiguousarray(out.transpose(0, 3, 1, 2))


def weight_family(rs, shape, family):
    """fp32 weights whose split is known by construction.  family 1: +-(256 p + q), split (+-256 p, +-q, 0); family 2:
    +-(65536 p + 256 q + r), split (+-65536 p, +-256 q, +-r); p, q, r in [128, 255] (the leading bit of every part is set, so
    truncation cuts exactly between the parts).  Returns (w, (s0, s1, s2)) and asserts the split."""
    p, q, r = (rs.randint(128, 256, size=shape).astype(np.float64) for _ in range(3))
    sign = rs.choice([-1.0, 1.0], size=shape)
    parts = (sign * 256 * p, sign * q, np.zeros(shape)) if family == 1 else (sign * 65536 * p, sign * 256 * q, sign * r)
    w = (parts[0] + parts[1] + parts[2]).astype(np.float32)
    for got, want in zip(split(w), parts):
        assert np.array_equal(got.astype(np.float64), want)
    return w, parts


def weight_seen_by_slice(parts, i):
    """What an operand that lives in slice ``i`` alone multiplies: the partner slices j with (i, j) among the six."""
    return sum(parts[j] for j in range(3) if (i, j) in SIX)


#: the in-loop family's significand c = 1 + 3 2^-9 + 3 2^-17 and the six-product sum of c c
LOOP_C = 1.0 + 3.0 * 2.0 ** -9 + 3.0 * 2.0 ** -17
LOOP_CC = 1.0 + 3.0 * 2.0 ** -8 + 3.0 * 2.0 ** -16 + 9.0 * 2.0 ** -18


def loop_family(rs, shape, lo=-3, hi=3):
    """Values for kernels that split BOTH operands in the loop (no slice tensor can be handed to them): v = +-2^e c with
    c = 1 + 3 2^-9 + 3 2^-17, e in [lo, hi].  The split is +-2^e (1, 3 2^-9, 3 2^-17) (asserted).  For ONE term a b of two
    such values the six slice products are 1, 3 2^-9 twice, 3 2^-17 twice and 9 2^-18, times +-2^(e+f): every partial sum is a
    multiple of 2^-18 below 2, so the sum +-2^(e+f) LOOP_CC is exact in fp32 in any order of issue, and it is NOT the fp32
    rounding of a b.  Dropping any of the six changes the bits; so does adding (1,2) or (2,1) (9 2^-26 = 1.125 ulp).  Adding
    (2,2) does NOT: 9 2^-34 lies below fp32 resolution at this magnitude (ulp 2^-23), so this family cannot see a spurious
    (2,2) product -- nothing with a single term can.  Returns (v, unit) with unit = +-2^e as float64: the expected value of
    a one-term output is unit_a unit_b LOOP_CC."""
    unit = np.exp2(rs.randint(lo, hi + 1, size=shape).astype(np.float64)) * rs.choice([-1.0, 1.0], size=shape)
    v = (unit * LOOP_C).astype(np.float32)
    assert np.array_equal(v.astype(np.float64), unit * LOOP_C)
    for got, want in zip(split(v), (1.0, 3.0 * 2.0 ** -9, 3.0 * 2.0 ** -17)):
        assert np.array_equal(got.astype(np.float64), unit * want)
    return v, unit


def only_tap(w, tap, block=None, width=64, axis=1):
    """Copy of w [Cout, Cin, k, k] that is zero outside tap ``tap`` (= ky k + kx) and, if ``block`` is given, outside the
    ``width``-wide block ``block`` of channel axis ``axis``."""
    k = w.shape[2]
    out = np.zeros_like(w)
    ky, kx = divmod(tap, k)
    out[:, :, ky, kx] = w[:, :, ky, kx]
    if block is not None:
        keep = np.zeros(w.shape[axis], bool)
        keep[block * width:(block + 1) * width] = True
        out = out * keep.reshape([-1 if a == axis else 1 for a in range(4)]).astype(out.dtype)
    return out


def one_hot_weights(rs, cout, cin, k, values=(1.0, 2.0)):
    """[Cout, Cin, k, k] with ONE nonzero entry per output channel (one tap, one input channel), +-1 / +-2."""
    w = np.zeros((cout, cin, k, k), np.float32)
    for co in range(cout):
        w[co, rs.randint(cin), rs.randint(k), rs.randint(k)] = rs.choice(values) * rs.choice([-1.0, 1.0])
    return w


def wide_range(rs, shape, channel_axis=1, lo=-6, hi=6, bf16_share=0.1):
    """Gaussian values with per-channel scales 2^lo .. 2^hi, a tenth of them cut to exact bf16 values."""
    v = rs.standard_normal(shape).astype(np.float32)
    sc = np.exp2(rs.randint(lo, hi + 1, size=shape[channel_axis])).astype(np.float32)
    v = v * sc.reshape([-1 if a == channel_axis else 1 for a in range(len(shape))])
    cut = rs.uniform(size=shape) < bf16_share
    return np.where(cut, _trunc16(np.ascontiguousarray(v)), v).astype(np.float32)


# ---------------------------------------------------------------- slice tensors of the kernels
def rotate_slices(xs, i):
    """``xs``: a slice tensor from ops.x3s_split / ops.x3q_split of exact-bf16 values, so that only slice 0 is populated.
    Returns a slice tensor with that plane in slice ``i`` and zeros elsewhere (both layouts lead with the slice index)."""
    v = xs.view(3, -1)
    assert not bool(v[1:].any()), "the values were not exact bf16"
    out = v.new_zeros(v.shape)
    out[i] = v[0]
    return out.view(-1)


def bf16_bits(s):
    """uint16 bit patterns of an fp32 array that holds bf16 values (asserted)."""
    s = _np32(s)
    assert np.array_equal(_trunc16(s), s), "not a bf16 value"
    return (s.view(np.uint32) >> np.uint32(16)).astype(np.uint16)


def ctx_pack(slices, transposed=False):
    """The weight panels of the dilated gather convolutions (csrc/ctx_common.h), built by the documented layout
    [9][K / 16][3][R][16] bf16 from three slice arrays [Cout, Cin, 3, 3] (fp32 holding bf16 values).
      forward:    K = Cin,  R = Cout, element (t, ci, co) = s[co][ci][t];
      transposed: K = Cout, R = Cin,  element (t', co, ci) = s[co][ci][8 - t'] (the data gradient's mirrored taps).
    Returns uint16 [9, K / 16, 3, R, 16]."""
    planes = []
    for s in slices:
        b = bf16_bits(s)
        cout, cin = b.shape[:2]
        b = b.reshape(cout, cin, 9)
        m = b[:, :, ::-1].transpose(2, 0, 1) if transposed else b.transpose(2, 1, 0)      # [9, K, R]
        k, r = m.shape[1:]
        planes.append(m.reshape(9, k // 16, 16, r).transpose(0, 1, 3, 2))                  # [9, K / 16, R, 16]
    return np.ascontiguousarray(np.stack(planes, axis=2))
