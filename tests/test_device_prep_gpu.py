"""Device input preparation: interpolated flow upsampling (``upsample_interp``) and the 10-crop views, on the GPU, against
the reference-held goldens (tests/golden/g9_dataset_item_extra.npz: the reference's own ``__getitem__``) and against the
plain-numpy restatement tests/interp_ref.py, which tests/test_device_prep_cpu.py ties to the dataset's scipy path.  Every
comparison is bit for bit.  No scipy here (``dataset.blockify(..., True)`` is never called)."""
import ctypes
import random
import sys

import numpy as np
import pytest
import torch

import dmcnet_amd
from dmcnet_amd import _lib, dataset, evaluate, ops, transforms
from tests import interp_ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _fixture_dataset(tmp_path, monkeypatch):
    from tests.golden import coviar_fixture as CF
    monkeypatch.setitem(sys.modules, "coviar", CF.coviar_module())
    return CF, CF.write_dataset(str(tmp_path))


def _chw(frames_hwc):
    return np.transpose(np.array(frames_hwc), (0, 3, 1, 2))


def test_device_prep_upsample_interp_matches_reference_getitem(golden, tmp_path, monkeypatch):
    """CoviarDataSet(..., flow_ds_factor=16, upsample_interp=True) through raw_item + DevicePrep.for_dataset == the flow the
    REFERENCE's __getitem__ returned (golden ``*_interp_c48`` whole blocks, ``*_interp_c40`` ragged), one test item and one
    seeded train item; mv / residual == __getitem__ of the same dataset without interpolation (they do not depend on it)."""
    CF, (data_root, flow_root, lst) = _fixture_dataset(tmp_path, monkeypatch)
    g = golden("g9_dataset_item_extra")
    for tag, is_train, minmax, seed, index, _ in (CF.CASES[0], CF.CASES[2]):
        for crop in CF.DS16_CROPS:
            mk = lambda interp: dataset.CoviarDataSet(data_root, flow_root, "hmdb51", lst, "mv", 1, 16, interp,
                                                      transforms.Compose([transforms.GroupCenterCrop(crop)]), 3, is_train,
                                                      True, 12, mv_minmaxnorm=minmax)
            ds = mk(True)
            prep = dataset.DevicePrep.for_dataset(ds, DEV)
            assert prep.upsample_interp and prep.flow_ds_factor == 16
            random.seed(seed)
            flow, mv, res, label = prep(dataset.collate_raw([ds.raw_item(index)]))
            key = "%s_interp_c%d" % (tag, crop)
            assert int(label[0]) == int(g[key + "_label"])
            assert torch.equal(flow[0].cpu(), torch.from_numpy(g[key + "_flow"])), key
            random.seed(seed)
            _, mv0, res0, _ = mk(False)[index]
            assert torch.equal(mv[0].cpu(), mv0) and torch.equal(res[0].cpu(), res0), key


def _nine_planned_frames():
    """The nine 256 x 340 frames / plans of test_prepare_inputs_crop_resize_flip_bit_exact: crop + resize + flip, scale +
    centre crop, centre crop + flip."""
    rs = np.random.RandomState(31)
    pipes = [transforms.Compose([transforms.GroupMultiScaleCrop(224, [1, .875, .75]), transforms.GroupRandomHorizontalFlip()]),
             transforms.Compose([transforms.GroupScale(256), transforms.GroupCenterCrop(224)]),
             transforms.Compose([transforms.GroupCenterCrop(224), transforms.GroupRandomHorizontalFlip()])]
    frames, plans, flips, want = [], [], [], []
    for k in range(9):
        f = rs.randint(0, 256, (256, 340, 7)).astype(np.uint8)
        random.seed(100 + k)
        plan, out, flip = transforms.geometry_plan(pipes[k % 3], f.shape)
        assert out == (224, 224)
        frames.append(f); plans.append(plan); flips.append(int(flip))
        want.append(np.transpose(np.asarray(transforms.apply_plan(f, plan, out, flip)), (2, 0, 1)))
    assert 0 < sum(flips) < len(flips) and any(p[2] != 224 for p in plans)
    return np.stack(frames), plans, flips, np.stack(want)


@pytest.mark.parametrize("factor", [16, 8, 32])
def test_prepare_inputs_upsample_interp_crop_resize_flip_bit_exact(factor):
    """ops.prepare_inputs(..., upsample_interp=True) through the three pipelines (both flip outcomes) == the numpy
    restatement of the interpolation on apply_plan's output; mv / residual == to_tensors."""
    frames, plans, flips, want = _nine_planned_frames()
    got = ops.prepare_inputs(torch.from_numpy(frames).to(DEV), torch.tensor(flips, dtype=torch.uint8), factor,
                             boxes=torch.tensor(plans, dtype=torch.int32), out_size=(224, 224), upsample_interp=True)
    ref = dataset.to_tensors(want, 0)
    assert torch.equal(got[0].cpu(), interp_ref.flow_tensor(want, factor))
    assert torch.equal(got[1].cpu(), ref[1]) and torch.equal(got[2].cpu(), ref[2])


@pytest.mark.parametrize("h,w,factor", [(100, 60, 16), (40, 56, 16), (50, 37, 8)])
def test_prepare_inputs_upsample_interp_whole_frame_ragged(h, w, factor):
    """The whole-frame route (no boxes) on non-square outputs, ragged on both axes, with a flipped frame."""
    rs = np.random.RandomState(h + w)
    hwc = rs.randint(0, 256, (4, h, w, 7)).astype(np.uint8)
    flip = [0, 1, 0, 1]
    want = np.stack([np.transpose(np.asarray(transforms.flip_with_x_negation(f) if fl else f), (2, 0, 1))
                     for f, fl in zip(hwc, flip)])
    got = ops.prepare_inputs(torch.from_numpy(hwc).to(DEV), torch.tensor(flip, dtype=torch.uint8), factor,
                             upsample_interp=True)
    ref = dataset.to_tensors(want, 0)
    assert torch.equal(got[0].cpu(), interp_ref.flow_tensor(want, factor))
    assert torch.equal(got[1].cpu(), ref[1]) and torch.equal(got[2].cpu(), ref[2])


@pytest.mark.parametrize("factor", [0, 16])
def test_views_entry_without_interp_equals_crop_entry(factor):
    """dmc_prepare_inputs_views with an identity src_index (and with NULL) and upsample_interp = 0 == dmc_prepare_inputs_crop,
    bit for bit; through ops.prepare_inputs(src_index=...) too."""
    frames, plans, flips, _ = _nine_planned_frames()
    lib = _lib.load()
    n = len(plans)
    fr = ops.u8_frames_buffer(frames.shape, DEV)
    fr.copy_(torch.from_numpy(frames))
    bx = torch.tensor(plans, dtype=torch.int32, device=DEV)
    fl = torch.tensor(flips, dtype=torch.uint8, device=DEV)
    ident = torch.arange(n, dtype=torch.int32, device=DEV)
    std = torch.tensor(ops._STD, dtype=torch.float64).float()
    std4 = (ctypes.c_float * 4)(float(torch.mean(std)), float(std[0]), float(std[1]), float(std[2]))
    stdp = ctypes.cast(std4, ctypes.c_void_p)
    stream = ops._stream()

    def outs():
        return [torch.full((n, c, 224, 224), float("nan"), device=DEV) for c in (2, 2, 3)]

    base = outs()
    work = torch.empty(lib.dmc_prepare_crop_workspace_bytes(n, 224, 224, factor) // 4 + 1, device=DEV)
    _lib.check(lib.dmc_prepare_inputs_crop(_lib.ptr(fr), _lib.ptr(bx), _lib.ptr(fl), *[_lib.ptr(t) for t in base],
                                           _lib.ptr(work), n, 256, 340, 224, 224, factor, stdp, stream), "crop")
    assert not any(bool(torch.isnan(t).any()) for t in base)
    for src in (ident, None):
        got = outs()
        work = torch.empty(lib.dmc_prepare_views_workspace_bytes(n, 224, 224, factor, 0) // 4 + 1, device=DEV)
        _lib.check(lib.dmc_prepare_inputs_views(_lib.ptr(fr), _lib.ptr(src), _lib.ptr(bx), _lib.ptr(fl),
                                                *[_lib.ptr(t) for t in got], _lib.ptr(work), n, n, 256, 340, 224, 224,
                                                factor, 0, stdp, stream), "views")
        for a, b in zip(got, base):
            assert torch.equal(a, b)
    got = ops.prepare_inputs(fr, fl, factor, boxes=bx, out_size=(224, 224), src_index=torch.arange(n, dtype=torch.int32))
    for a, b in zip(got, base):
        assert torch.equal(a, b)


def test_device_prep_ten_crop_matches_reference_getitem(golden, tmp_path, monkeypatch):
    """The 10-crop transform through raw_item + DevicePrep (ten views of each uploaded frame) == what the REFERENCE's
    __getitem__ returned with its own GroupOverSample (golden ``*_over_*``)."""
    CF, (data_root, flow_root, lst) = _fixture_dataset(tmp_path, monkeypatch)
    g = golden("g9_dataset_item_extra")
    for tag, is_train, minmax, seed, index, _ in (CF.CASES[0], CF.CASES[2]):
        ds = dataset.CoviarDataSet(data_root, flow_root, "hmdb51", lst, "mv", 1, 0, False,
                                   transforms.Compose([transforms.GroupOverSample(CF.CROP, None)]), 3, is_train, True, 12,
                                   mv_minmaxnorm=minmax)
        prep = dataset.DevicePrep.for_dataset(ds, DEV)
        random.seed(seed)
        flow, mv, res, label = prep(dataset.collate_raw([ds.raw_item(index)]))
        key = tag + "_over"
        assert tuple(flow.shape) == (1, 30, 2, CF.CROP, CF.CROP) and int(label[0]) == int(g[key + "_label"])
        for got, k in ((flow, "_flow"), (mv, "_mv"), (res, "_res")):
            assert torch.equal(got[0].cpu(), torch.from_numpy(g[key + k])), (key, k)


def _ten_crop_batch(seed=7, videos=2, segments=3):
    """Raw 10-crop batch of 256 x 340 synthetic frames (GroupOverSample(224, 256)) and the CPU transform's output
    [B, 30, 7, 224, 224]."""
    rs = np.random.RandomState(seed)
    over = transforms.GroupOverSample(224, 256)
    items, cpu = [], []
    for v in range(videos):
        frames = [rs.randint(0, 256, (256, 340, 7)).astype(np.uint8) for _ in range(segments)]
        plans, out, flips = transforms.oversample_plans(over, frames[0].shape)
        items.append((np.stack(frames), np.asarray(plans, np.int32), out, np.asarray(flips, bool), 3 + 5 * v))
        cpu.append(_chw(over(frames)))
    return dataset.collate_raw(items), np.stack(cpu)


def test_device_prep_ten_crop_scaled_batch_all_flow_modes():
    """GroupOverSample(224, 256) on 256 x 340 frames, batch 2 x 3 segments: DevicePrep == to_tensors of the CPU transform's
    output for flow_ds_factor 0 and 16, and == the numpy restatement for factor 16 with interpolation."""
    raw, cpu = _ten_crop_batch()
    for factor, interp in ((0, False), (16, False), (16, True)):
        flow, mv, res, label = dataset.DevicePrep(DEV, factor, interp)(raw)
        assert tuple(flow.shape) == (2, 30, 2, 224, 224) and tuple(res.shape) == (2, 30, 3, 224, 224)
        assert label.tolist() == [3, 8]
        for b in range(2):
            ref = dataset.to_tensors(cpu[b], factor)
            want_flow = interp_ref.flow_tensor(cpu[b], factor) if interp else ref[0]
            assert torch.equal(flow[b].cpu(), want_flow), (factor, interp, b)
            assert torch.equal(mv[b].cpu(), ref[1]) and torch.equal(res[b].cpu(), ref[2]), (factor, interp, b)


def test_evaluate_with_device_prep_equals_cpu_prepared_inputs():
    """evaluate.evaluate(..., test_crops=10, prep=DevicePrep) on raw batches returns the score arrays and the accuracy of the
    same model fed the CPU-prepared tensors: the inputs are bit-identical and the eval forward is deterministic."""
    torch.manual_seed(5)
    model = dmcnet_amd.Model(51, 3, "mv", base_model="resnet18", use_databn=0, gen_flow_or_delta=1,
                             arch_estimator="DenseNetTiny").to(DEV).eval()
    raw, cpu = _ten_crop_batch(seed=9)
    tensors = [dataset.to_tensors(cpu[b], 0) for b in range(2)]
    batch = tuple(torch.stack([t[i] for t in tensors]) for i in range(3)) + (raw[4],)
    want, acc_want = evaluate.evaluate(model, [batch], 3, test_crops=10, device=DEV)
    got, acc_got = evaluate.evaluate(model, [raw], 3, test_crops=10, device=DEV, prep=dataset.DevicePrep(DEV, 0))
    assert len(got) == len(want) == 2 and acc_got == acc_want
    for (a, la), (b, lb) in zip(got, want):
        assert la == lb and a.shape == (1, 51) and np.array_equal(a, b)


def test_refusals_before_any_launch():
    """One block on an axis with interpolation, interpolation without a factor, a host src_index out of range, a flip vector
    of the wrong length: ValueError from Python, DMC_E_INVALID from the C entry; the outputs stay untouched."""
    lib = _lib.load()
    fr = ops.u8_frames_buffer((2, 48, 16, 7), DEV)
    fr.zero_()
    with pytest.raises(ValueError):
        ops.prepare_inputs(fr, None, 16, upsample_interp=True)                       # 3 x 1 blocks
    with pytest.raises(ValueError):
        ops.prepare_inputs(fr, None, 0, upsample_interp=True)
    with pytest.raises(ValueError):
        ops.prepare_inputs(fr, None, 0, src_index=torch.tensor([0, 2], dtype=torch.int32))
    with pytest.raises(ValueError):
        ops.prepare_inputs(fr, None, 0, src_index=torch.tensor([-1], dtype=torch.int32))
    with pytest.raises(ValueError):
        ops.prepare_inputs(fr, torch.zeros(2, dtype=torch.uint8), 0, src_index=torch.tensor([0, 1, 1], dtype=torch.int32))
    outs = [torch.full((2, c, 48, 16), 7.0, device=DEV) for c in (2, 2, 3)]
    work = torch.empty(1024, device=DEV)
    std4 = (ctypes.c_float * 4)(0.226, 0.229, 0.224, 0.225)
    stdp = ctypes.cast(std4, ctypes.c_void_p)
    call = lambda n_src, n_out, factor, interp, src=None: lib.dmc_prepare_inputs_views(
        _lib.ptr(fr), _lib.ptr(src), None, None, *[_lib.ptr(t) for t in outs], _lib.ptr(work), n_src, n_out, 48, 16, 48, 16,
        factor, interp, stdp, ops._stream())
    assert call(2, 2, 16, 1) == -1 and b"two blocks" in lib.dmc_last_error()
    assert call(2, 2, 0, 1) == -1 and b"flow_ds_factor" in lib.dmc_last_error()
    assert call(2, 3, 0, 0) == -1 and b"src_index" in lib.dmc_last_error()
    assert call(2, 0, 0, 0) == -1
    torch.cuda.synchronize()
    assert all(bool((t == 7.0).all()) for t in outs)
    with pytest.raises(_lib.DmcHipError):
        _lib.check(call(2, 2, 16, 1), "dmc_prepare_inputs_views")
