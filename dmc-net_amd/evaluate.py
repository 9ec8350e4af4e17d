"""Evaluation path: per-video scores with TSN consensus, score dump and late fusion.

Mirrors the reference's ``test.py`` (code/dmcnet/test.py:139-198: forward over
``test_segments x test_crops`` frames, mean over them, ``np.savez(scores, labels, names)`` with
the videos re-ordered by sorted name) and ``combine.py`` (code/dmcnet/combine.py:35-57: weighted
sum of the I-frame / MV / residual / DMC score files, arg-max accuracy).  The forward pass is the
training path's HIP generator + classifier in eval mode; nothing here needs a gradient.

The I3D variant's video-level evaluator (``evaluate_i3d``) restates ``code/dmcnet_I3D/test/evaluate_video_{hmdb,ucf101}_i3d.py``
and the metrics of ``code/dmcnet_I3D/train/metric.py``.
"""
import numpy as np
import torch
import torch.nn.functional as F


@torch.no_grad()
def forward_video(model, input_mv, input_residual, test_segments, test_crops=1):
    """[B, segments*crops, C, H, W] inputs -> [B, num_class] numpy scores (mean over the frames)."""
    out = model(input_mv, input_residual)
    scores = out[0]
    scores = scores.view((-1, test_segments * test_crops) + tuple(scores.shape[1:])).mean(dim=1)
    return scores.cpu().numpy().copy()


@torch.no_grad()
def evaluate(model, loader, test_segments, test_crops=1, device="cuda:0", prep=None):
    """Returns (output, accuracy %) with ``output`` = [(video_scores [1,C], label), ...] in loader
    order, exactly what the reference accumulates before saving.  ``prep`` (a ``dataset.DevicePrep``)
    turns the loader's raw uint8 batches (``dataset.RawView`` + ``dataset.collate_raw``) into the float
    batch on the GPU, as in ``driver.validate``; with the 10-crop transform every frame is uploaded once."""
    model.eval()
    output = []
    for batch in loader:
        _flow, input_mv, input_residual, label = prep(batch) if prep is not None else batch
        s = forward_video(model, input_mv.to(device, non_blocking=True),
                          input_residual.to(device, non_blocking=True), test_segments, test_crops)
        for b in range(s.shape[0]):
            output.append((s[b:b + 1], int(label[b])))
    pred = np.array([int(np.argmax(x[0])) for x in output])
    labels = np.array([x[1] for x in output])
    return output, float((pred == labels).mean() * 100.0) if len(output) else 0.0


@torch.no_grad()
def evaluate_i3d(net, loader, device, score_path=None, prep=None):
    """Video-level evaluation of the I3D variant: the loop of the reference's evaluator
    (code/dmcnet_I3D/test/evaluate_video_hmdb_i3d.py:171-253; evaluate_video_ucf101_i3d.py is the same loop) with the metrics of
    code/dmcnet_I3D/train/metric.py -- ``MetricList(Loss("loss-ce"), Accuracy(topk=1, "top1"), Accuracy(topk=5, "top5"))``.

    ``loader``: any iterable of (data [b,7|5,T,H,W], target [b], video_subpath [b]).  Per batch, with ``net`` in eval mode and no
    autograd: logits = net(data[:, :5]) and loss = the cross entropy over the batch (its mean) -- what ``static_model.forward``
    computes with node='logit' (code/dmcnet_I3D/train/model.py:160-188) --, then a softmax per clip.  ``net`` is the only part
    that needs a device; everything after it runs on the host (fp32 torch tensors, the reference's operations in its order).

    ``prep`` (an ``i3d_data.DeviceClipPrep``): the loader yields (raw, target, video_subpath) with ``raw`` the uint8 batch of
    ``i3d_data.collate_raw_clips``, and ``data = prep(raw)`` is computed on the device (``dmc_prepare_clip``).

    The reference's quirks, kept as written:
      * a video's score is the SUM of its clips' softmax vectors, not their mean;
      * the loss recorded for a video is the batch-mean loss of the batch in which its FIRST clip appears;
      * loss-ce, top-1 and top-5 are computed over VIDEOS (one entry per distinct subpath, in first-seen order);
      * the saved ``.npz`` (``score_path``) holds PER-CLIP softmax scores ``scores`` [n_clips, C] float32 and ``labels``
        [n_clips, 1] int64, in loader order.

    Returns a dict: ``metrics`` {"loss-ce", "top1", "top5"} (fractions, as the reference logs them); per video, in first-seen
    order, ``videos``, ``video_scores`` [n, C] (softmax sums), ``video_counts``, ``video_labels``, ``video_losses``; per clip,
    ``scores`` and ``labels`` (the arrays of the score file)."""
    net.eval()
    per_video = {}                                          # subpath -> [label [1], loss (0-d), softmax sum [1, C], clip count]
    scores, labels = [], []
    for data, target, subpaths in loader:
        if prep is not None:
            data = prep(data)
        logits = net(data[:, :5].to(device=device, dtype=torch.float32, non_blocking=True))
        loss = F.cross_entropy(logits, target.to(device))
        prob = torch.softmax(logits, 1).cpu()
        target = target.cpu()
        scores.append(prob)
        labels.append(target.reshape(-1, 1))
        loss = loss.cpu()
        for i in range(prob.shape[0]):
            v = subpaths[i]
            if v in per_video:
                per_video[v][2] += prob[i:i + 1]
                per_video[v][3] += 1
            else:
                per_video[v] = [target[i:i + 1].clone(), loss.clone(), prob[i:i + 1].clone(), 1]
    # metric.Loss / metric.Accuracy over the videos: python-float sums divided by the number of videos
    n = len(per_video)
    loss_sum, hits = 0.0, {1: 0.0, 5: 0.0}
    for label, loss, pred, _ in per_video.values():
        loss_sum += float(loss.numpy().sum())
        for k in hits:
            top = pred.topk(k, 1, True, True)[1].t()
            hits[k] += float(top.eq(label.view(1, -1).expand_as(top)).view(-1).float().sum())
    metrics = {"loss-ce": loss_sum / n if n else float("nan"), "top1": hits[1] / n if n else float("nan"),
               "top5": hits[5] / n if n else float("nan")}
    clip_scores = np.concatenate([s.numpy() for s in scores], 0) if scores else np.zeros((0, 0), np.float32)
    clip_labels = np.concatenate([t.numpy() for t in labels], 0) if labels else np.zeros((0, 1), np.int64)
    if score_path is not None:
        np.savez(score_path, scores=clip_scores, labels=clip_labels)
    vals = list(per_video.values())
    return {"metrics": metrics, "videos": list(per_video.keys()),
            "video_scores": np.concatenate([v[2].numpy() for v in vals], 0) if vals else np.zeros((0, 0), np.float32),
            "video_counts": np.array([v[3] for v in vals], dtype=np.int64),
            "video_labels": np.array([int(v[0][0]) for v in vals], dtype=np.int64),
            "video_losses": np.array([float(v[1]) for v in vals], dtype=np.float32),
            "scores": clip_scores, "labels": clip_labels}


def save_scores(path, output, name_list):
    """Reference layout: entries re-ordered by sorted video name (code/dmcnet/test.py:183-198)."""
    order = {e: i for i, e in enumerate(sorted(name_list))}
    n = len(output)
    scores, labels, names = [None] * n, [None] * n, [None] * n
    for i in range(n):
        idx = order[name_list[i]]
        scores[idx], labels[idx], names[idx] = output[i], output[i][1], name_list[i]
    obj = np.empty(n, dtype=object)
    for i, (s, l) in enumerate(scores):
        obj[i] = (s, l)
    np.savez(path, scores=obj, labels=np.array(labels), names=np.array(names))


def load_scores(path):
    """Reads a score file written by the reference (pickled object array of (scores, label)) or
    by :func:`save_scores` -> (scores [n, C] float, labels [n] int, names [n])."""
    with np.load(path, allow_pickle=True) as d:
        scores = np.array([np.asarray(s[0]).reshape(-1, np.asarray(s[0]).shape[-1])[0]
                           for s in d["scores"]])
        labels = np.array([int(s[1]) for s in d["scores"]], dtype=np.int64)
        names = np.array([str(x) for x in d["names"]])
    return scores, labels, names


def combine(iframe, mv, res, flow=None, wi=2.0, wm=1.0, wr=1.0, wf=1.0):
    """Late fusion of (scores, labels) pairs -> (accuracy in [0,1], combined scores)."""
    (si, li), (sm, lm), (sr, lr) = iframe, mv, res
    if not (np.array_equal(li, lm) and np.array_equal(li, lr)):
        raise ValueError("score files disagree on the labels")
    combined = si * wi + sm * wm + sr * wr
    if flow is not None:
        combined = combined + wf * flow[0]
    return float(np.sum(np.argmax(combined, axis=1) == li)) / len(li), combined
