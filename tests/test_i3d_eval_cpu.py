"""The I3D eval path without a GPU: the video-level evaluator (evaluate.evaluate_i3d) against the reference's own evaluation loop
(golden G12: code/dmcnet_I3D/test/evaluate_video_hmdb_i3d.py executed around train/metric.py), driven by a fake net; and the
eval-mode trunk ops on CPU tensors (predicates False, the ops refuse: no CPU fallback)."""
import numpy as np
import pytest
import torch

from dmcnet_amd import _lib, evaluate, i3d, ops


class _FakeNet(torch.nn.Module):
    """Returns the golden's logits of the clips whose indices the loader put into data[:, 0, 0, 0, 0]."""

    def __init__(self, logits):
        super().__init__()
        self.logits = torch.from_numpy(logits)
        self.calls = []

    def forward(self, x):
        self.calls.append((tuple(x.shape), self.training, torch.is_grad_enabled()))
        return self.logits[x[:, 0, 0, 0, 0].long()]


def _loader(g):
    n, b = len(g["names"]), int(g["batch"])
    for s in range(0, n, b):
        data = torch.zeros(b, 7, 1, 1, 1)
        data[:, 0, 0, 0, 0] = torch.arange(s, s + b, dtype=torch.float32)
        yield data, torch.from_numpy(g["targets"][s:s + b]), [str(v) for v in g["names"][s:s + b]]


def test_evaluate_i3d_reproduces_the_reference_loop(golden, tmp_path):
    g = golden("g12_i3d_eval")
    net = _FakeNet(g["logits"]).train()
    path = str(tmp_path / "scores.npz")
    res = evaluate.evaluate_i3d(net, _loader(g), "cpu", score_path=path)
    # the score file: per-clip softmax scores and labels, bit for bit
    with np.load(path) as f:
        assert f["scores"].dtype == g["scores"].dtype and f["labels"].dtype == g["labels"].dtype
        assert np.array_equal(f["scores"], g["scores"]) and np.array_equal(f["labels"], g["labels"])
    assert np.array_equal(res["scores"], g["scores"]) and np.array_equal(res["labels"], g["labels"])
    for k, gk in (("loss-ce", "loss_ce"), ("top1", "top1"), ("top5", "top5")):
        assert abs(res["metrics"][k] - float(g[gk])) <= 1e-12, (k, res["metrics"][k], float(g[gk]))
    # the forward saw 5 channels, in eval mode, without autograd
    assert net.calls and all(s[1] == 5 and not tr and not ge for s, tr, ge in net.calls)
    # per video: first-seen order, summed (not averaged) softmax, clip counts 1 and 3
    names = [str(v) for v in g["names"]]
    order = list(dict.fromkeys(names))
    assert res["videos"] == order
    assert res["video_counts"].tolist() == [names.count(v) for v in order]
    assert sorted(set(res["video_counts"].tolist())) == [1, 3]
    for j, v in enumerate(order):
        idx = [i for i, n in enumerate(names) if n == v]
        acc = torch.from_numpy(g["scores"][idx[0]:idx[0] + 1]).clone()
        for i in idx[1:]:
            acc += torch.from_numpy(g["scores"][i:i + 1])
        assert np.array_equal(res["video_scores"][j:j + 1], acc.numpy())


def test_eval_ops_on_cpu_tensors_refuse():
    unit = i3d.Unit3Dpy(16, 32, (3, 3, 3)).eval()
    stem = i3d.Unit3Dpy(2, 64, (7, 7, 7), (2, 2, 2)).eval()
    x = torch.randn(1, 16, 2, 4, 4).bfloat16().contiguous(memory_format=torch.channels_last_3d)
    cue = torch.randn(1, 2, 4, 8, 8)
    with torch.no_grad():
        assert not ops.conv_bn_relu3d_eval_supported(x, unit.conv3d, unit.batch3d)
        assert not ops.stem3d_eval_supported(cue, stem.conv3d, stem.batch3d)
        with pytest.raises(_lib.DmcHipError):
            ops.conv_bn_relu3d_eval(x, unit.conv3d, unit.batch3d)
        with pytest.raises(_lib.DmcHipError):
            ops.stem3d_bn_relu_eval(cue, stem.conv3d, stem.batch3d)
        # the stock modules still serve CPU tensors (the fp32 trunk, any device)
        assert unit(x.float()).shape == (1, 32, 2, 4, 4)
    assert i3d.EVAL_FUSED in (True, False)
