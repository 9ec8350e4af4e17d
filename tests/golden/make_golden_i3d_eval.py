#!/usr/bin/env python3
"""G12: the video-level evaluation loop of the reference's I3D evaluator, EXECUTED as written.

The lines of code/dmcnet_I3D/test/evaluate_video_hmdb_i3d.py from ``metrics = metric.MetricList(`` to its last
``metrics.update`` are read from the reference tree and run with ``exec`` around the reference's own train/metric.py, with
  * ``eval_iter``: batches of 2 clips whose video names repeat across batches (three videos with 1 clip, three with 3);
  * ``net.forward(data, target, node='logit')``: seeded logits looked up by the clip index carried in data[:, 0, 0, 0, 0], and
    the loss CrossEntropyLoss()(logits, target) -- what static_model.forward returns in eval mode (train/model.py:160-188).
Stored: the inputs (logits, targets, names), the final metric values and the per-clip scores / labels of the saved .npz.
Run in the build container: ``python tests/golden/make_golden_i3d_eval.py``."""
import importlib.util
import logging
import os
import tempfile
import textwrap
import time
import json
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference/code/dmcnet_I3D"
EVALUATOR = os.path.join(REF, "test", "evaluate_video_hmdb_i3d.py")

spec = importlib.util.spec_from_file_location("ref_metric", os.path.join(REF, "train", "metric.py"))
metric = importlib.util.module_from_spec(spec)
spec.loader.exec_module(metric)

lines = open(EVALUATOR).read().split("\n")
start = next(i for i, l in enumerate(lines) if l.strip().startswith("metrics = metric.MetricList("))
end = max(i for i, l in enumerate(lines) if "metrics.update(" in l)
loop = textwrap.dedent("\n".join(lines[start:end + 1]))

C = 51
names = np.array(["v_a", "v_b", "v_b", "v_c", "v_d", "v_b", "v_c", "v_e", "v_f", "v_c", "v_f", "v_f"])
rng = np.random.RandomState(121)
video_label = {v: int(rng.randint(C)) for v in sorted(set(names.tolist()))}
targets = np.array([video_label[v] for v in names], dtype=np.int64)
logits = (rng.standard_normal((len(names), C)) * 2.0).astype(np.float32)
for i, v in enumerate(names):             # some videos lean towards their label: top-1 / top-5 hits and misses
    logits[i, targets[i]] += {"v_a": 3.0, "v_b": 2.0, "v_f": 1.5, "v_c": 0.7}.get(str(v), 0.0)
BATCH = 2


class _Net:
    net = torch.nn.Module()

    def forward(self, data, target, node="logit"):
        out = torch.from_numpy(logits)[data[:, 0, 0, 0, 0].long()]
        return [out], [torch.nn.CrossEntropyLoss()(out, target)]


eval_iter = []
for b in range(0, len(names), BATCH):
    data = torch.zeros(BATCH, 7, 1, 1, 1)
    data[:, 0, 0, 0, 0] = torch.arange(b, b + BATCH, dtype=torch.float32)
    eval_iter.append((data, torch.from_numpy(targets[b:b + BATCH]), [str(v) for v in names[b:b + BATCH]]))

args = types.SimpleNamespace(dataset="hmdb51", split=1, task_name="g12", clip_length=250, batch_size=BATCH)
cwd = os.getcwd()
with tempfile.TemporaryDirectory() as tmp:
    os.chdir(tmp)
    try:
        os.makedirs("hmdb51_1")
        ns = dict(metric=metric, torch=torch, np=np, os=os, time=time, logging=logging, json=json, args=args, net=_Net(),
                  eval_iter=eval_iter)
        exec(compile(loop, EVALUATOR, "exec"), ns)
        with np.load(os.path.join("hmdb51_1", "g12_250.npz")) as f:
            saved_scores, saved_labels = f["scores"], f["labels"]
    finally:
        os.chdir(cwd)

vals = dict(nv[0] for nv in ns["metrics"].get_name_value())
out = {"logits": logits, "targets": targets, "names": names, "batch": np.int64(BATCH),
       "loss_ce": np.float64(vals["loss-ce"]), "top1": np.float64(vals["top1"]), "top5": np.float64(vals["top5"]),
       "scores": saved_scores, "labels": saved_labels}
np.savez(os.path.join(HERE, "g12_i3d_eval.npz"), **out)
print("G12 done", vals, saved_scores.shape, saved_labels.shape, saved_scores.dtype, saved_labels.dtype)
