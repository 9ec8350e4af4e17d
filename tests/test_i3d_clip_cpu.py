"""CPU checks of the I3D clip preparation (dmcnet_amd.i3d_data, dmc_prepare_clip): ``ClipTransform`` against golden G13 --
outputs of the REFERENCE's own Compose chains (tests/golden/make_golden_i3d_clip.py) -- under torch.equal, the plan / apply
split, the library's refusals (host code: no GPU needed), the collate function and the no-CPU-fallback rule."""
import ctypes
import os

import numpy as np
import pytest
import torch

from dmcnet_amd import _lib, i3d_data as D, ops
from tests.golden import make_golden_i3d_clip as G


@pytest.fixture(scope="module")
def g13(golden):
    return golden("g13_i3d_clip")


def transform_of(case):
    tag, train, aug_seed, _, _, size, f, _ = case
    return D.ClipTransform(size, bool(train), f, aug_seed)


@pytest.mark.parametrize("case", G.CASES, ids=[c[0] for c in G.CASES])
def test_clip_transform_equals_the_reference_chain(g13, case):
    tag, train, aug_seed, (h0, w0), t, size, f, seeds = case
    tf = transform_of(case)
    for i, seed in enumerate(seeds):                                 # the second call continues the transform's two streams
        got = tf(G.make_clip(seed, h0, w0, t))
        want = torch.from_numpy(g13["%s_out%d" % (tag, i)])
        assert got.dtype == torch.float32 and got.shape == want.shape
        assert torch.equal(got, want), (tag, i)


def test_golden_covers_both_flip_outcomes_and_the_zero_wrap(g13):
    flips = {}
    for case in G.CASES:
        if case[1]:
            flips[case[0]] = transform_of(case).plan(case[3])[2]
    assert [flips["train_s%d" % s] for s in (1, 2, 3, 4)] == [1, 0, 0, 1]
    clip = G.make_clip(11, 40, 52, 3)
    assert (clip[:, :, 0::7] == 0).any() and (clip[:, :, 2::7] == 0).any()
    # a flipped zero stays zero: normalised flow_x of the unblocked mv_x channel holds (0 / 255 - mean) / std
    out = torch.from_numpy(g13["train_s1_out0"])
    zero = (torch.tensor(0.0) / 255.0 - D.MEAN[2]) / D.STD[2]
    assert (out[2] == zero).any()


def test_table_in_the_fixture_is_the_case_table(g13):
    assert [str(t) for t in g13["tags"]] == [c[0] for c in G.CASES]
    for row, c in zip(g13["table"], G.CASES):
        assert list(row) == [c[1], c[2], c[3][0], c[3][1], c[4], c[5][0], c[5][1], c[6], len(c[7])]


@pytest.mark.parametrize("case", G.CASES, ids=[c[0] for c in G.CASES])
def test_plan_then_apply_equals_call(case):
    tag, train, aug_seed, (h0, w0), t, size, f, seeds = case
    a, b, c = transform_of(case), transform_of(case), transform_of(case)
    for seed in seeds:
        clip = G.make_clip(seed, h0, w0, t)
        plan = a.plan(clip.shape)
        manual = D.apply_plan(clip, plan, a.out_size, a.flow_ds_factor, a.mean, a.std)
        assert torch.equal(manual, b(clip))
        raw_clip, raw_plan = c.raw_item(clip)
        assert raw_clip is clip and raw_plan.dtype == np.int32 and tuple(raw_plan) == plan
    if not train:
        assert plan[2] == 0 and plan[:2] == (int(round((h0 - size[0]) / 2.)), int(round((w0 - size[1]) / 2.)))


def test_clip_transform_refusals():
    with pytest.raises(ValueError):
        D.ClipTransform(modality="rgb")
    with pytest.raises(ValueError):
        D.ClipTransform(modality="flow")
    with pytest.raises(ValueError):
        D.ClipTransform(flow_ds_factor=0)
    tf = D.ClipTransform((32, 48), True, 16, 0)
    with pytest.raises(ValueError):                                   # range(W0 - OW) is empty: the reference raises too
        tf(G.make_clip(1, 40, 48, 2))
    with pytest.raises(ValueError):
        tf(G.make_clip(1, 40, 52, 2).astype(np.float32))
    with pytest.raises(ValueError):
        D.apply_plan(G.make_clip(1, 40, 52, 2), (9, 0, 0), (32, 48))


def test_collate_raw_clips():
    tf = D.ClipTransform((32, 48), True, 16, 3)
    items = [tf.raw_item(G.make_clip(s, 40, 52, 2)) for s in (1, 2, 3)]
    clips, plans = D.collate_raw_clips(items)
    assert clips.dtype == torch.uint8 and tuple(clips.shape) == (3, 40, 52, 14)
    assert plans.dtype == torch.int32 and tuple(plans.shape) == (3, 3)
    assert torch.equal(clips[1], torch.from_numpy(items[1][0])) and plans[2].tolist() == list(items[2][1])
    for other in (G.make_clip(4, 41, 52, 2), G.make_clip(4, 40, 53, 2), G.make_clip(4, 40, 52, 3)):
        with pytest.raises(ValueError):
            D.collate_raw_clips(items + [(other, np.zeros(3, np.int32))])


def test_library_refuses_bad_arguments_before_any_launch():
    lib = _lib.load()
    assert lib.dmc_prepare_clip_workspace_bytes(3, 64, 224, 224, 16) == 0
    dummy = torch.zeros(64)
    p = _lib.ptr(dummy)
    ms = (ctypes.c_float * 7)(*([0.5] * 7))
    m = ctypes.cast(ms, ctypes.c_void_p)
    good = dict(clips=p, plans=p, out=p, work=None, B=1, T=2, H0=40, W0=52, OH=32, OW=48, f=16, n=3, mean=m, std=m)

    def call(**kw):
        a = dict(good, **kw)
        return lib.dmc_prepare_clip(a["clips"], a["plans"], a["out"], a["work"], a["B"], a["T"], a["H0"], a["W0"], a["OH"], a["OW"],
                                    a["f"], a["n"], a["mean"], a["std"], None)

    bad = [dict(clips=None), dict(plans=None), dict(out=None), dict(mean=None), dict(std=None),
           dict(B=0), dict(T=0), dict(H0=0), dict(W0=-1), dict(OH=0), dict(OW=0), dict(B=-3),
           dict(OH=41), dict(OW=53), dict(n=-1), dict(n=8), dict(f=-1)]
    for kw in bad:
        assert call(**kw) == -1, kw
        assert b"dmc_prepare_clip" in lib.dmc_last_error(), kw
    # pointers that the aligned dword reads cannot use
    assert call(clips=ctypes.c_void_p(dummy.data_ptr() + 1)) == -1


def test_prepare_clip_raises_on_cpu_tensors():
    clips = torch.zeros((1, 40, 52, 14), dtype=torch.uint8)
    plans = torch.zeros((1, 3), dtype=torch.int32)
    with pytest.raises(_lib.DmcHipError):
        ops.prepare_clip(clips, plans, (32, 48), 16)
    with pytest.raises(ValueError):
        ops.check_clip_plans(torch.tensor([[9, 0, 0]], dtype=torch.int32), 40, 52, 32, 48)
    with pytest.raises(ValueError):
        ops.check_clip_plans(torch.tensor([[0, -1, 0]], dtype=torch.int32), 40, 52, 32, 48)
    ops.check_clip_plans(torch.tensor([[8, 4, 1]], dtype=torch.int32), 40, 52, 32, 48)


@pytest.mark.skipif(not os.path.isdir(G.REF_DATA), reason="the reference tree is not on this machine")
def test_golden_regenerates_bit_identically(g13):
    import subprocess
    import sys
    import tempfile
    # in a child process: the generator installs stub modules (cv2, torchvision, skimage) into sys.modules
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "g13.npz")
        code = ("import sys, numpy as np; sys.path.insert(0, %r); from tests.golden import make_golden_i3d_clip as G; "
                "np.savez(%r, **G.generate())" % (G.ROOT, path))
        subprocess.check_call([sys.executable, "-c", code])
        new = dict(np.load(path))
    assert sorted(new) == sorted(g13)
    for k in new:
        assert new[k].dtype == g13[k].dtype and np.array_equal(new[k], g13[k]), k
