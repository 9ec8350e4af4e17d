"""GPU: dmc_prepare_clip / ops.prepare_clip / i3d_data.DeviceClipPrep against i3d_data.ClipTransform -- which
tests/test_i3d_clip_cpu.py ties to the reference's own chains (golden G13) -- under torch.equal, and the entry point's memory
contract in guarded arenas (tests/abi_arena.py).

Shapes are the smallest at which the kernel can go wrong: records of 7, 21, 28 and 112 bytes (T = 1, 3, 4, 16: unaligned, odd,
a dword multiple, the bank-stride case), outputs with whole and ragged f x f blocks, OW % 4 = 2 (the scalar-store tail), a
clip of exactly the output size, a 100-wide output (four chunks of 32 pixels, the last 4 wide), the last window of the last
clip (where the spare bytes behind the clips are read), both flip outcomes in one batch.

The arena cases are built here and appended to the registry of tests/abi_cases.py when this module is imported, so that the
registry's coverage check (tests/test_abi_arena_cpu.py, which runs after the whole suite has been collected) sees the entry
point; they are RUN here (tests/test_abi_arena_gpu.py is parametrised before this module is imported)."""
import numpy as np
import pytest
import torch

from dmcnet_amd import _lib, evaluate, i3d_data as D, ops
from tests import abi_cases
from tests.abi_arena import run_case
from tests.golden import tiny_i3d

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

#: (H0, W0, OH, OW, flow_ds_factor)
SHAPES = [(40, 52, 32, 48, 0), (40, 52, 32, 48, 16), (47, 61, 40, 36, 16), (30, 33, 24, 24, 5), (25, 37, 18, 30, 0),
          (25, 37, 18, 30, 1), (32, 48, 32, 48, 16), (20, 110, 17, 100, 16)]
FRAMES = [1, 3, 4, 16]
NORMS = {0: ((), ()), 3: (D.MEAN, D.STD), 7: ((0.485, 0.456, 0.406, 0.5, 0.45, 0.4, 0.35), (0.229, 0.224, 0.225, 0.25, 0.2, 0.3, 0.21))}


def clip_of(seed, h0, w0, t):
    clip = np.random.RandomState(seed).randint(0, 256, (h0, w0, t * 7)).astype(np.uint8)
    clip.reshape(h0 * w0, t, 7)[::3, :, 0] = 0                       # zeros in flow_x: 256 - 0 wraps to 0
    return clip


def plans_of(h0, w0, oh, ow, flip_first):
    """Two clips: an odd x1 inside, and the LAST window (y1 = H0 - OH, x1 = W0 - OW) in the last clip; opposite flips."""
    x1 = 1 if w0 - ow >= 1 else 0
    y1 = (h0 - oh) // 2
    return [(y1, x1, flip_first), (h0 - oh, w0 - ow, 1 - flip_first)]


def reference(clips, plans, size, f, mean, std):
    return torch.stack([D.apply_plan(c, p, size, max(int(f), 1), mean, std) for c, p in zip(clips, plans)])


def device(clips, plans, size, f, mean, std, **kw):
    buf = ops.u8_frames_buffer((len(clips),) + clips[0].shape, DEV)
    buf.copy_(torch.from_numpy(np.stack(clips)))
    return ops.prepare_clip(buf, torch.tensor(plans, dtype=torch.int32), size, f, mean, std, **kw)


@pytest.mark.parametrize("t", FRAMES)
@pytest.mark.parametrize("shape", SHAPES, ids=["%dx%d-%dx%d-f%d" % s for s in SHAPES])
def test_device_equals_clip_transform(shape, t):
    h0, w0, oh, ow, f = shape
    clips = [clip_of(100 + t, h0, w0, t), clip_of(200 + t, h0, w0, t)]
    for flip_first in (0, 1):
        plans = plans_of(h0, w0, oh, ow, flip_first)
        for n_norm in ((3, 0, 7) if t == 3 else (3,)):
            mean, std = NORMS[n_norm]
            got = device(clips, plans, (oh, ow), f, mean, std)
            want = reference(clips, plans, (oh, ow), f, mean, std)
            assert got.dtype == torch.float32 and tuple(got.shape) == (2, 7, t, oh, ow)
            assert torch.equal(got.cpu(), want), (shape, t, flip_first, n_norm)


@pytest.mark.parametrize("f", [0, 16])
def test_every_byte_value_in_every_channel(f):
    h0, w0, oh, ow, t = 40, 52, 32, 48, 3
    idx = np.arange(h0 * w0).reshape(h0, w0, 1, 1)
    clip = ((idx + 37 * np.arange(7).reshape(1, 1, 1, 7) + 11 * np.arange(t).reshape(1, 1, t, 1)) % 256).astype(np.uint8).reshape(h0, w0, t * 7)
    plans = [(3, 1, 0), (8, 4, 1)]
    for y1, x1, _ in plans:
        win = clip[y1:y1 + oh, x1:x1 + ow].reshape(-1, t, 7)
        assert all(len(np.unique(win[:, k, c])) == 256 for k in range(t) for c in range(7))
    got = device([clip, clip], plans, (oh, ow), f, D.MEAN, D.STD)
    assert torch.equal(got.cpu(), reference([clip, clip], plans, (oh, ow), f, D.MEAN, D.STD))


def test_recipe_shaped_clip():
    """B = 1, T = 8, 256 x 340 -> 224 x 224, f = 16, a random plan, flipped (the training recipe at an eighth of its frames)."""
    clip = clip_of(7, 256, 340, 8)
    rs = np.random.RandomState(8)
    plan = (int(rs.randint(0, 32)), int(rs.randint(0, 116)), 1)
    got = device([clip], [plan], (224, 224), 16, D.MEAN, D.STD)
    assert torch.equal(got.cpu(), reference([clip], [plan], (224, 224), 16, D.MEAN, D.STD))


def test_out_is_written_in_place_and_leaves_nothing_stale():
    h0, w0, oh, ow, t, f = 47, 61, 40, 36, 3, 16
    clips = [clip_of(31, h0, w0, t), clip_of(32, h0, w0, t)]
    out = torch.full((2, 7, t, oh, ow), float("nan"), device=DEV)
    for plans in ([(0, 0, 0), (7, 25, 1)], [(5, 3, 1), (1, 9, 0)]):
        ret = device(clips, plans, (oh, ow), f, D.MEAN, D.STD, out=out)
        assert ret is out
        assert torch.equal(out.cpu(), reference(clips, plans, (oh, ow), f, D.MEAN, D.STD))
    with pytest.raises(ValueError):
        device(clips, plans, (oh, ow), f, D.MEAN, D.STD, out=torch.empty((2, 7, t, oh, ow + 1), device=DEV))
    with pytest.raises(ValueError):                                   # a host plan that leaves the clip is refused
        device(clips, [(0, 0, 0), (8, 25, 1)], (oh, ow), f, D.MEAN, D.STD)


@pytest.mark.parametrize("train", [True, False])
def test_device_clip_prep_equals_the_transform(train):
    h0, w0, t = 40, 52, 3
    clips = [clip_of(40 + i, h0, w0, t) for i in range(3)]
    mk = lambda: D.ClipTransform((32, 48), train, 16 if train else 1, aug_seed=4)
    tf, tf2, tf3 = mk(), mk(), mk()
    prep = D.DeviceClipPrep.for_transform(tf, DEV)
    got = prep(D.collate_raw_clips([tf2.raw_item(c) for c in clips]))
    assert torch.equal(got.cpu(), torch.stack([tf3(c) for c in clips]))
    out = torch.empty_like(got)
    assert prep(D.collate_raw_clips([mk().raw_item(c) for c in clips[:1]] * 3), out=out) is out


def test_evaluate_i3d_with_device_prep():
    """evaluate_i3d over raw uint8 batches + DeviceClipPrep returns what it returns over the CPU-prepared loader."""
    h0, w0, t = 40, 52, 2
    net = tiny_i3d.build(5).to(DEV)
    names = ["a", "b", "b", "c"]
    tgt = torch.tensor([1, 3, 3, 0])
    clips = [clip_of(60 + i, h0, w0, t) for i in range(4)]
    mk = lambda: D.ClipTransform((32, 48), False, 1)
    tf_cpu, tf_raw = mk(), mk()
    cpu_loader = [(torch.stack([tf_cpu(c) for c in clips[2 * i:2 * i + 2]]), tgt[2 * i:2 * i + 2], names[2 * i:2 * i + 2]) for i in range(2)]
    raw_loader = [(D.collate_raw_clips([tf_raw.raw_item(c) for c in clips[2 * i:2 * i + 2]]), tgt[2 * i:2 * i + 2], names[2 * i:2 * i + 2])
                  for i in range(2)]
    a = evaluate.evaluate_i3d(net, cpu_loader, DEV)
    b = evaluate.evaluate_i3d(net, raw_loader, DEV, prep=D.DeviceClipPrep.for_transform(mk(), DEV))
    assert sorted(a) == sorted(b) and a["metrics"] == b["metrics"] and a["videos"] == b["videos"]
    for k in a:
        if isinstance(a[k], np.ndarray):
            assert np.array_equal(a[k], b[k]), k


# ---------------------------------------------------------------------------------------------------------------------
# memory contract: dmc_prepare_clip in guarded arenas (buffers of exactly the promised sizes, the clips with their 16 spare bytes)
# ---------------------------------------------------------------------------------------------------------------------
def clip_case(t, shape, flip_first):
    h0, w0, oh, ow, f = shape
    clips = torch.from_numpy(np.stack([clip_of(300 + t, h0, w0, t), clip_of(400 + t, h0, w0, t)]))
    plans = torch.tensor(plans_of(h0, w0, oh, ow, flip_first), dtype=torch.int32)
    mean, std = torch.tensor(D.MEAN, dtype=torch.float32), torch.tensor(D.STD, dtype=torch.float32)

    def fn(a):
        lib = _lib.load()
        a.call("dmc_prepare_clip", a.inp("clips", clips, slack=16), a.inp("plans", plans), a.out("out", (2, 7, t, oh, ow)),
               abi_cases.opt_work(a, "workspace", lib.dmc_prepare_clip_workspace_bytes(2, t, oh, ow, f)),
               2, t, h0, w0, oh, ow, f, 3, mean, std)

    def check(bufs):                                                  # bit for bit what the wrapper computes
        buf = ops.u8_frames_buffer(tuple(clips.shape), DEV)
        buf.copy_(clips)
        assert abi_cases.same(bufs["out"], ops.prepare_clip(buf, plans, (oh, ow), f))
    return fn, check


def refused_case(a):
    clips = torch.from_numpy(clip_of(1, 40, 52, 2)[None])
    a.call("dmc_prepare_clip", a.inp("clips", clips, slack=16), a.inp("plans", torch.zeros((1, 3), dtype=torch.int32)),
           a.out("out", (1, 7, 2, 32, 48)), None, 1, 2, 40, 52, 32, 53, 16, 3, torch.tensor(D.MEAN), torch.tensor(D.STD))


ARENA_CASES = []
for _t, _shape in ((3, SHAPES[0]), (3, SHAPES[1]), (16, SHAPES[2]), (4, SHAPES[4])):
    for _flip in (0, 1):
        _fn, _ck = clip_case(_t, _shape, _flip)
        ARENA_CASES.append(abi_cases.Case(abi_cases.tag("dmc_prepare_clip", "T%d" % _t, "%dx%d" % _shape[2:4], "f%d" % _shape[4], "flip%d" % _flip),
                                          ["dmc_prepare_clip"], _fn, check=_ck, capacity=16 << 20))
ARENA_CASES.append(abi_cases.Case("dmc_prepare_clip-refused-OW", ["dmc_prepare_clip"], refused_case, expect_rc=abi_cases.DMC_E_INVALID,
                                  capacity=16 << 20))
_known = {c.id for c in abi_cases.CASES}
abi_cases.CASES.extend(c for c in ARENA_CASES if c.id not in _known)


@pytest.mark.parametrize("case", ARENA_CASES, ids=[c.id for c in ARENA_CASES])
def test_prepare_clip_memory_contract(case):
    try:
        bufs = run_case(case.fn, device=DEV, capacity=case.capacity, expect_rc=case.expect_rc)
        if case.check is not None:
            case.check(bufs)
    except RuntimeError as e:
        if "HIP error" in str(e) or "illegal memory access" in str(e):
            # a faulted device serves nothing more: end the session here instead of launching the remaining cases on it
            pytest.exit("GPU fault in %s: %s" % (case.id, str(e).splitlines()[0]), returncode=3)
        raise
