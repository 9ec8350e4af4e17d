#!/usr/bin/env python3
"""G13: the tensor contract of the I3D variant's loader for modality 'flow+mp4', produced by the REFERENCE's own transform
chains (code/dmcnet_I3D/data/iterator_factory.py:49-56,72-77) run in this container:

    python tests/golden/make_golden_i3d_clip.py

The reference's data/image_transforms.py and data/video_transforms.py are imported as they are, as submodules of an empty
stand-in package (the real ``data/__init__.py`` pulls the video reader in), with the stub ``cv2`` of make_golden.py and --
``skimage`` is absent from this image -- the documented ``block_reduce`` stand-in of make_golden_dataset.py (imported, not
copied).  The reference's own ``Compose`` chains then run on clips regenerated from ``numpy.random.RandomState(seed)``
(:func:`make_clip`); only the outputs and the case table are stored (tests/golden/g13_i3d_clip.npz).

Cases (:data:`CASES`): the training chain with aug_seed 1 .. 4 (1 and 4 flip, 2 and 3 do not), crop 32 x 48 of 40 x 52,
f = 16, the first of them called twice on one Compose (the streams advance); a ragged crop 40 x 36 of 47 x 61 (f = 16); an
f = 5 case; the centre-crop chain 47 x 61 -> 40 x 36 and -> 42 x 56 (``round`` of 3.5, 12.5, 2.5, 2.5).  Every clip holds
zeros in flow_x and mv_x (the ``256 - 0`` wrap of the flip).
"""
import importlib.util
import os
import sys
import types
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF_DATA = "/root/reference/code/dmcnet_I3D/data"
OUT = os.path.join(HERE, "g13_i3d_clip.npz")
MEAN = [0.485, 0.456, 0.406]
STD = [0.229, 0.224, 0.225]

#: (tag, train, aug_seed, (H0, W0), T, (OH, OW), flow_ds_factor, clip seeds: one call per seed on ONE Compose)
CASES = [
    ("train_s1", 1, 1, (40, 52), 3, (32, 48), 16, (11, 12)),
    ("train_s2", 1, 2, (40, 52), 2, (32, 48), 16, (13,)),
    ("train_s3", 1, 3, (40, 52), 2, (32, 48), 16, (14,)),
    ("train_s4", 1, 4, (40, 52), 2, (32, 48), 16, (15,)),
    ("ragged", 1, 1, (47, 61), 2, (40, 36), 16, (16,)),
    ("f5", 1, 4, (30, 33), 3, (24, 24), 5, (17,)),
    ("centre_a", 0, 0, (47, 61), 2, (40, 36), 1, (18,)),
    ("centre_b", 0, 0, (47, 61), 3, (42, 56), 1, (19,)),
]


def make_clip(seed, h0, w0, t):
    """A decoded clip [H0, W0, T*7] uint8; every third pixel of flow_x and every fifth of mv_x is 0."""
    clip = np.random.RandomState(seed).randint(0, 256, (h0, w0, t * 7)).astype(np.uint8)
    flat = clip.reshape(h0 * w0, t, 7)
    flat[::3, :, 0] = 0
    flat[::5, :, 2] = 0
    return clip


def import_reference():
    """The reference's two transform modules as (image_transforms, video_transforms)."""
    sys.path.insert(0, ROOT)
    from tests.golden.make_golden import install_stubs
    from tests.golden.make_golden_dataset import block_reduce_standin
    install_stubs()
    sys.modules["skimage.measure"].block_reduce = block_reduce_standin
    pkg = types.ModuleType("ref_i3d_data")
    pkg.__path__ = [REF_DATA]
    sys.modules["ref_i3d_data"] = pkg
    mods = []
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", SyntaxWarning)               # video_transforms.py:46 `is not 0 or 1`
        for name in ("image_transforms", "video_transforms"):
            spec = importlib.util.spec_from_file_location("ref_i3d_data." + name, os.path.join(REF_DATA, name + ".py"))
            mod = importlib.util.module_from_spec(spec)
            sys.modules[spec.name] = mod
            spec.loader.exec_module(mod)
            mods.append(mod)
    return mods


def generate():
    """{array name: value} of the fixture, from the reference's chains."""
    _it, vt = import_reference()
    out = {"tags": np.array([c[0] for c in CASES]),
           "table": np.array([[c[1], c[2], c[3][0], c[3][1], c[4], c[5][0], c[5][1], c[6], len(c[7])] for c in CASES], np.int64),
           "clip_seeds": np.array([list(c[7]) + [-1] * (2 - len(c[7])) for c in CASES], np.int64)}
    for tag, train, aug_seed, (h0, w0), t, size, f, seeds in CASES:
        if train:
            chain = vt.Compose([vt.RandomCrop(size), vt.RandomHorizontalFlip("flow+mp4"), vt.ToTensor("flow+mp4", f),
                                vt.Normalize(MEAN, STD)], aug_seed=aug_seed)
        else:
            chain = vt.Compose([vt.CenterCrop(size), vt.ToTensor("flow+mp4"), vt.Normalize(MEAN, STD)])
        for i, seed in enumerate(seeds):
            res = chain(make_clip(seed, h0, w0, t))
            assert tuple(res.shape) == (7, t) + tuple(size) and str(res.dtype) == "torch.float32"
            out["%s_out%d" % (tag, i)] = res.numpy().copy()
    return out


def main():
    out = generate()
    np.savez_compressed(OUT, **out)
    for k in sorted(out):
        print(k, out[k].shape, out[k].dtype)
    print(OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
