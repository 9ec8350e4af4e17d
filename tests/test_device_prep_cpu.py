"""Host side of the device input preparation's interpolated flow upsampling and 10-crop views (no GPU): the numpy
restatement the GPU tests compare against is tied to the dataset's scipy path, the C ABI's tap export to the restatement,
the ten plans to ``transforms.GroupOverSample``, the raw item to the reference-held golden."""
import ctypes
import random
import sys

import numpy as np
import pytest
import torch

from dmcnet_amd import _lib, dataset, transforms
from tests import interp_ref

SHAPES = [(224, 224, 16), (48, 48, 16), (40, 40, 16), (40, 56, 16), (224, 224, 8), (100, 60, 16), (224, 224, 32)]


@pytest.mark.parametrize("h,w,factor", SHAPES)
def test_numpy_restatement_equals_scipy_blockify(h, w, factor):
    """tests/interp_ref.py == dataset.blockify(x, factor, upsample_interp=True) (scipy's interp1d, the reference's lines
    code/dmcnet/dataset.py:236-246), bit for bit, on integer input in [0, 256] (256: a flipped x component)."""
    x = np.random.RandomState(h * 1000 + w + factor).randint(0, 257, (3, 2, h, w))
    assert np.array_equal(interp_ref.blockify_interp(x, factor), dataset.blockify(x, factor, True))


def test_numpy_restatement_flipped_input_and_single_block():
    """A mirrored frame with the x component negated around 128 (transforms.flip_with_x_negation: values reach 256), through
    to the fp32 flow tensor; one block on an axis raises, as scipy does."""
    rs = np.random.RandomState(3)
    img = rs.randint(0, 256, (3, 56, 40, 7)).astype(np.uint8)
    flipped = np.stack([np.transpose(transforms.flip_with_x_negation(f), (2, 0, 1)) for f in img])      # [S,7,H,W] int32
    assert flipped[:, 0].max() <= 256 and flipped.dtype == np.int32
    assert np.array_equal(interp_ref.blockify_interp(flipped[:, 0:2], 16), dataset.blockify(flipped[:, 0:2], 16, True))
    assert torch.equal(interp_ref.flow_tensor(flipped, 16), dataset.to_tensors(flipped, 16, True)[0])
    one = rs.randint(0, 256, (1, 2, 16, 48))
    with pytest.raises(ValueError):
        interp_ref.blockify_interp(one, 16)
    with pytest.raises(ValueError):
        dataset.blockify(one, 16, True)


@pytest.mark.parametrize("factor", [8, 16, 32])
@pytest.mark.parametrize("n", [2, 3, 7, 14, 16])
def test_interp_taps_export_equals_numpy_tables(n, factor):
    """dmc_prepare_interp_taps (host only; the function the kernel calls) == numpy's linspace / searchsorted tables: lo
    exactly, dx and t as raw bits."""
    lib = _lib.load()
    lo, dx, t = np.full(n * factor, -1, np.int32), np.zeros(n * factor), np.zeros(n * factor)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    assert lib.dmc_prepare_interp_taps(n, factor, p(lo), p(dx), p(t)) == 0
    rlo, rdx, rt = interp_ref.taps(n, factor)
    assert np.array_equal(lo, rlo)
    assert np.array_equal(dx.view(np.uint64), rdx.view(np.uint64)) and np.array_equal(t.view(np.uint64), rt.view(np.uint64))
    assert set(lo.tolist()) == set(range(n - 1))                       # every interval is used (the kernel's dx table relies on it)


def test_interp_taps_export_refuses_bad_arguments():
    lib = _lib.load()
    buf = np.zeros(64)
    p = buf.ctypes.data_as(ctypes.c_void_p)
    for n in (1, 0, -3):
        assert lib.dmc_prepare_interp_taps(n, 16, p, p, p) == -1 and b"dmc_prepare_interp_taps" in lib.dmc_last_error()
    assert lib.dmc_prepare_interp_taps(4, 0, p, p, p) == -1
    assert lib.dmc_prepare_interp_taps(4, 16, None, p, p) == -1


@pytest.mark.parametrize("crop,scale", [(224, None), (224, 256), (48, 56)])
def test_oversample_plans_reproduce_group_oversample(crop, scale):
    """oversample_plans + apply_plan == GroupOverSample (code/dmcnet/transforms.py:77-114), bit for bit and in its order
    ((offset, frame, crop | mirror) -> index (o*S + s)*2 + f); the plans are the same alone or inside a Compose; no
    random number is drawn."""
    rs = np.random.RandomState(crop + (scale or 0))
    frames = [rs.randint(0, 256, (256, 340, 7)).astype(np.uint8) for _ in range(3)]
    over = transforms.GroupOverSample(crop, scale)
    want = over(frames)
    random.seed(17)
    state = random.getstate()
    plans, out, flips = transforms.oversample_plans(over, frames[0].shape)
    assert random.getstate() == state
    assert (plans, out, flips) == transforms.oversample_plans(transforms.Compose([over]), frames[0].shape)
    assert len(plans) == 10 and len(flips) == 10 and out == (crop, crop) and flips == [False, True] * 5
    a = scale if scale is not None else None
    for p in plans:
        assert p[:4] == (0, 0, 256, 340) and p[4:6] == ((a, a) if a else (256, 340))
    assert len(want) == 30
    for o in range(5):
        for s, f in enumerate(frames):
            for k in range(2):
                got = transforms.apply_plan(f, plans[2 * o + k], out, flips[2 * o + k])
                ref = want[(o * 3 + s) * 2 + k]
                assert got.shape == ref.shape and np.array_equal(got, ref), (o, s, k)
    with pytest.raises(ValueError):
        transforms.oversample_plans(transforms.GroupCenterCrop(crop), frames[0].shape)
    with pytest.raises(ValueError):                                   # geometry_plan itself is unchanged
        transforms.geometry_plan(over, frames[0].shape)


def test_raw_item_ten_crop_vs_reference_getitem(golden, tmp_path, monkeypatch):
    """raw_item with the 10-crop transform -> apply_plan per view -> to_tensors == what the REFERENCE's __getitem__ returned
    for the same files (golden g9_dataset_item_extra, ``*_over_*``), in the golden's order; collate_raw keeps both kinds of
    item and refuses to mix them."""
    from tests.golden import coviar_fixture as CF
    g = golden("g9_dataset_item_extra")
    monkeypatch.setitem(sys.modules, "coviar", CF.coviar_module())
    data_root, flow_root, lst = CF.write_dataset(str(tmp_path))
    for tag, is_train, minmax, seed, index, _ in (CF.CASES[0], CF.CASES[2]):
        ds = dataset.CoviarDataSet(data_root, flow_root, "hmdb51", lst, "mv", 1, 0, False,
                                   transforms.Compose([transforms.GroupOverSample(CF.CROP, None)]), 3, is_train, True, 12,
                                   mv_minmaxnorm=minmax)
        random.seed(seed)
        frames, plans, out, flips, label = ds.raw_item(index)
        assert frames.shape == (3, CF.H0, CF.W0, 7) and frames.dtype == np.uint8
        assert plans.shape == (10, 8) and plans.dtype == np.int32 and flips.shape == (10,) and out == (CF.CROP, CF.CROP)
        views = [transforms.apply_plan(frames[s], plans[2 * o + f], out, bool(flips[2 * o + f]))
                 for o in range(5) for s in range(3) for f in range(2)]
        flow, mv, res = dataset.to_tensors(np.transpose(np.array(views), (0, 3, 1, 2)), 0)
        key = tag + "_over"
        assert label == int(g[key + "_label"])
        assert torch.equal(flow, torch.from_numpy(g[key + "_flow"])) and torch.equal(mv, torch.from_numpy(g[key + "_mv"]))
        assert torch.equal(res, torch.from_numpy(g[key + "_res"]))
        random.seed(seed)
        batch = dataset.collate_raw([ds.raw_item(index), ds.raw_item(index)] if not is_train else [ds.raw_item(index)])
        assert tuple(batch[1].shape)[1:] == (10, 8) and tuple(batch[3].shape)[1:] == (10,) and batch[3].dtype == torch.uint8
        assert batch[2] == (CF.CROP, CF.CROP)
    single = dataset.CoviarDataSet(data_root, flow_root, "hmdb51", lst, "mv", 1, 0, False,
                                   transforms.Compose([transforms.GroupCenterCrop(CF.CROP)]), 3, False, True, 12)
    one = dataset.collate_raw([single.raw_item(0)])
    assert tuple(one[1].shape) == (1, 8) and tuple(one[3].shape) == (1,)
    with pytest.raises(ValueError):
        dataset.collate_raw([single.raw_item(0), (frames, plans, out, flips, label)])


def test_views_size_query_and_argument_refusal_without_gpu():
    """dmc_prepare_views_workspace_bytes is non-zero and monotone in N; the repeat path's size is the crop entry's;
    dmc_prepare_inputs_views refuses null pointers before any launch and names itself in dmc_last_error()."""
    lib = _lib.load()
    for interp in (0, 1):
        sizes = [lib.dmc_prepare_views_workspace_bytes(n, 224, 224, 16, interp) for n in (1, 2, 30, 120, 1200)]
        assert sizes[0] > 0 and all(a < b for a, b in zip(sizes, sizes[1:])), sizes
    assert lib.dmc_prepare_views_workspace_bytes(120, 224, 224, 16, 1) >= 120 * 2 * 14 * 14 * 4
    assert lib.dmc_prepare_views_workspace_bytes(120, 40, 56, 16, 1) >= 120 * 2 * 3 * 4 * 4
    for f in (0, 16):
        assert lib.dmc_prepare_views_workspace_bytes(7, 100, 60, f, 0) == lib.dmc_prepare_crop_workspace_bytes(7, 100, 60, f)
    assert lib.dmc_prepare_views_workspace_bytes(7, 100, 60, 0, 0) > 0
    rc = lib.dmc_prepare_inputs_views(None, None, None, None, None, None, None, None, 1, 1, 8, 8, 8, 8, 0, 0, None, None)
    assert rc == -1 and b"dmc_prepare_inputs_views" in lib.dmc_last_error()


def test_device_prep_constructor_reads_the_dataset_options():
    """DevicePrep.for_dataset takes flow_ds_factor and upsample_interp from the dataset; DevicePrep(device, factor) is the
    repeat path as before."""
    class _DS(object):
        _flow_ds_factor, _upsample_interp = 16, True
    p = dataset.DevicePrep.for_dataset(_DS(), "cpu")
    assert (p.flow_ds_factor, p.upsample_interp) == (16, True)
    p = dataset.DevicePrep("cpu", 16)
    assert (p.flow_ds_factor, p.upsample_interp) == (16, False)
    p = dataset.DevicePrep.for_dataset(dataset.SyntheticCoviarDataSet(4, 51, flow_ds_factor=16), "cpu")
    assert (p.flow_ds_factor, p.upsample_interp) == (16, False)
