"""The tensor side of the I3D variant's loader for modality ``flow+mp4``: a decoded uint8 clip -> the fp32
``[7, T, OH, OW]`` tensor ``I3DTrainer.step`` / ``evaluate.evaluate_i3d`` take, on the CPU (:class:`ClipTransform`, the
reference's chain restated in numpy / torch) and on the device (:class:`DeviceClipPrep`, ``dmc_prepare_clip``), bit for bit
the same.

Reference: code/dmcnet_I3D/data/iterator_factory.py:49-56,72-77 builds

    train:  Compose([RandomCrop((OH, OW)), RandomHorizontalFlip('flow+mp4'), ToTensor('flow+mp4', ds_factor),
                     Normalize(mean, std)], aug_seed=s)
    val:    Compose([CenterCrop((OH, OW)), ToTensor('flow+mp4'), Normalize(mean, std)])

from data/image_transforms.py:14-35,47-59,138-200 and data/video_transforms.py:23-70; a clip is packed as
``[H0, W0, T*7]`` uint8, frame ``t`` in channels ``7t .. 7t+6`` = flow_x, flow_y, mv_x, mv_y, res0, res1, res2
(data/video_iterator.py:150-178,428-433).  What the chain does, quirks included:

  * ``Compose`` gives transform ``i`` its own ``RandomState(aug_seed + i)``: the crop draws from ``aug_seed``, the flip
    from ``aug_seed + 1``;
  * random crop: ``x1 = rng.choice(range(W0 - OW))`` THEN ``y1 = rng.choice(range(H0 - OH))`` -- the last column / row
    offset is never drawn and a clip of exactly the output size raises; centre crop: Python 3's ``round`` (half to even);
  * flip (a draw per clip, ``rand() < 0.5``): mirror along W; flow_x and mv_x of every frame become ``256 - v`` cast to
    uint8, so 0 stays 0;
  * ToTensor: ``if self._flow_ds_factor is not 0 or 1`` is always true -- the two flow channels of every frame are replaced
    by their f x f block means (ragged blocks zero-padded and divided by f^2), repeated back and ASSIGNED INTO THE UINT8
    ARRAY, i.e. truncated: floor(sum / f^2).  f = 1 (the validation default) is the identity; then ``float() / 255``;
  * Normalize zips over the first dimension and stops at ``len(mean)`` = 3: flow_x, flow_y and mv_x are normalised, mv_y
    and the residual stay in [0, 1].

Out of scope: frame sampling, decoding, and every modality but ``flow+mp4``.
"""
import numpy as np
import torch

MEAN = (0.485, 0.456, 0.406)
STD = (0.229, 0.224, 0.225)


def apply_plan(clip_u8, plan, out_size, flow_ds_factor=1, mean=MEAN, std=STD):
    """The chain after its random draws: crop at ``(y1, x1)``, flip if ``plan[2]``, ToTensor, Normalize -> float32 [7,T,OH,OW]."""
    y1, x1, flip = (int(v) for v in plan)
    oh, ow = out_size
    data = clip_u8[y1:y1 + oh, x1:x1 + ow, :]
    if data.shape[:2] != (oh, ow):
        raise ValueError("plan %s leaves the %s clip (output %d x %d)" % ((y1, x1, flip), clip_u8.shape[:2], oh, ow))
    if flip:
        data = np.ascontiguousarray(data[:, ::-1]).astype(np.int32)
        for c in (0, 2):
            data[:, :, c::7] = 256 - data[:, :, c::7]
    data = data.astype(np.uint8)
    clips = np.ascontiguousarray(data.reshape(oh, ow, -1, 7).transpose(3, 2, 0, 1))      # [7, T, OH, OW]
    f = int(flow_ds_factor)
    if f >= 2:
        ph, pw = (-oh) % f, (-ow) % f
        flow = np.pad(clips[0:2].astype(np.int64), ((0, 0), (0, 0), (0, ph), (0, pw)))
        sums = flow.reshape(2, -1, (oh + ph) // f, f, (ow + pw) // f, f).sum(axis=(3, 5))
        means = sums // (f * f)
        clips[0:2] = means.repeat(f, axis=2).repeat(f, axis=3)[:, :, :oh, :ow].astype(np.uint8)
    t = torch.from_numpy(clips).float() / 255.0
    for ch, m, s in zip(t, mean, std):
        ch.sub_(m).div_(s)
    return t


class ClipTransform(object):
    """The reference's ``flow+mp4`` chain on the CPU.  ``train=True``: random crop, random flip, ToTensor with
    ``flow_ds_factor``, Normalize; its two random streams (``RandomState(aug_seed)`` for the crop, ``RandomState(aug_seed + 1)``
    for the flip) are owned by this object and advance by one clip per ``__call__`` / ``plan`` / ``raw_item``.  ``train=False``:
    centre crop, no flip, no draw (the recipe's validation ``flow_ds_factor`` is 1)."""

    def __init__(self, out_size=(224, 224), train=True, flow_ds_factor=16, aug_seed=0, mean=MEAN, std=STD, modality="flow+mp4"):
        if modality != "flow+mp4":
            raise ValueError("ClipTransform covers modality 'flow+mp4' only (got %r)" % (modality,))
        if int(flow_ds_factor) < 1:
            raise ValueError("flow_ds_factor must be >= 1 (the reference cannot run 0)")
        if len(mean) != len(std) or len(mean) > 7:
            raise ValueError("mean and std need the same number of entries, at most 7")
        self.out_size = (int(out_size[0]), int(out_size[1])) if not isinstance(out_size, int) else (out_size, out_size)
        self.train, self.flow_ds_factor, self.aug_seed = bool(train), int(flow_ds_factor), aug_seed
        self.mean, self.std = tuple(float(v) for v in mean), tuple(float(v) for v in std)
        self.rng_crop = np.random.RandomState(aug_seed)
        self.rng_flip = np.random.RandomState(aug_seed + 1)

    def plan(self, shape):
        """(y1, x1, flip) for a clip of ``shape`` = (H0, W0, ...); consumes the draws ``__call__`` would."""
        h, w = int(shape[0]), int(shape[1])
        oh, ow = self.out_size
        if not self.train:
            if oh > h or ow > w:
                raise ValueError("centre crop %d x %d of a %d x %d clip" % (oh, ow, h, w))
            return int(round((h - oh) / 2.)), int(round((w - ow) / 2.)), 0
        if w - ow < 1 or h - oh < 1:
            raise ValueError("random crop %d x %d needs a clip larger than that on both axes (got %d x %d), as the reference's "
                             "rng.choice(range(0)) does" % (oh, ow, h, w))
        x1 = int(self.rng_crop.choice(range(w - ow)))
        y1 = int(self.rng_crop.choice(range(h - oh)))
        flip = 1 if self.rng_flip.rand() < 0.5 else 0
        return y1, x1, flip

    def _check(self, clip_u8):
        if not isinstance(clip_u8, np.ndarray) or clip_u8.dtype != np.uint8 or clip_u8.ndim != 3 or clip_u8.shape[2] % 7 \
                or clip_u8.shape[2] == 0:
            raise ValueError("expected a uint8 numpy clip [H0, W0, T*7]")

    def __call__(self, clip_u8):
        self._check(clip_u8)
        return apply_plan(clip_u8, self.plan(clip_u8.shape), self.out_size, self.flow_ds_factor, self.mean, self.std)

    def raw_item(self, clip_u8):
        """(clip_u8, plan int32 [3]): what a ``DataLoader`` hands to :func:`collate_raw_clips` / :class:`DeviceClipPrep`."""
        self._check(clip_u8)
        return clip_u8, np.asarray(self.plan(clip_u8.shape), np.int32)


def collate_raw_clips(items):
    """[(clip_u8 [H0,W0,T*7], plan [3]), ...] -> (clips uint8 [B,H0,W0,T*7], plans int32 [B,3]); one batch holds one shape."""
    shapes = {tuple(np.shape(it[0])) for it in items}
    if len(shapes) != 1:
        raise ValueError("collate_raw_clips: mixed clip shapes %s in one batch" % sorted(shapes))
    clips = torch.from_numpy(np.stack([np.ascontiguousarray(it[0]) for it in items]))
    plans = torch.from_numpy(np.stack([np.asarray(it[1], np.int32).reshape(3) for it in items]))
    return clips, plans


class DeviceClipPrep(object):
    """Raw batch (:func:`collate_raw_clips`) -> ``data [B,7,T,OH,OW]`` on the GPU by ``dmc_prepare_clip``: the uint8 clips
    travel as decoded (a quarter of the fp32 batch's bytes) and crop, flip, blockify, / 255 and Normalize run in one kernel.
    ``out=trainer.static_batch()[0]`` lets the batch land in the hipGraph input buffer of ``I3DTrainer``, which then skips
    its copy."""

    def __init__(self, device, out_size=(224, 224), flow_ds_factor=16, mean=MEAN, std=STD):
        self.device = torch.device(device)
        self.out_size = (int(out_size[0]), int(out_size[1]))
        self.flow_ds_factor = int(flow_ds_factor)
        self.mean, self.std = tuple(float(v) for v in mean), tuple(float(v) for v in std)

    @classmethod
    def for_transform(cls, tf, device):
        """The preparation that matches ``tf.__call__`` (a :class:`ClipTransform`): every option is read from it."""
        return cls(device, tf.out_size, tf.flow_ds_factor, tf.mean, tf.std)

    def __call__(self, raw, out=None):
        from . import ops
        clips, plans = raw
        if not plans.is_cuda:
            ops.check_clip_plans(plans, int(clips.shape[1]), int(clips.shape[2]), self.out_size[0], self.out_size[1])
        buf = ops.u8_frames_buffer(tuple(clips.shape), self.device)
        buf.copy_(clips, non_blocking=True)
        return ops.prepare_clip(buf, plans.to(self.device, torch.int32, non_blocking=True), self.out_size, self.flow_ds_factor,
                                self.mean, self.std, out=out)
