"""GPU parity at BASELINE.json's sizes: whole training steps at B=40 clips (120 frames), the
C=101 per-rank workload of config 4, the 120-frame generator with generic weights, and the
data-parallel step with two ranks sharing the one GPU of the test box.

Reference lines reproduced: code/dmcnet/train.py:221-266 (dmcnet step),
code/dmcnet_GAN/train.py:261-371 (D step / G step).  Bars (BASELINE.json north_star): losses and
consensus logits within 1e-4 relative (2e-4 for the GAN pair, whose discriminator runs a chain of
BatchNorm(eps=0.8)); post-step weights are compared ABSOLUTELY, at a small fraction of the Adam step
``lr * lr_mult`` of their optimizer (Adam normalises the update: a relative bar on weights says
nothing about the gradient)."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import dmcnet_amd
from dmcnet_amd import train as T
from oracle import dmc_oracle as O
from tests.golden.make_golden import HP, WATCH, WATCH_D

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KW = dict(base_model="resnet18", use_databn=0, gen_flow_or_delta=1, arch_estimator="DenseNetTiny")
OPT = dict(lr=HP["lr"], weight_decay=HP["weight_decay"], lr_cls_mult=HP["lr_cls_mult"],
           lr_mse_mult=HP["lr_mse_mult"])


def rel_err(a, b):
    a, b = a.detach().double().cpu(), torch.as_tensor(b).double().cpu()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))


def _pair(num_class, gan, seed):
    o = O.OracleModel(num_class, 3, "mv", arch_d="Discriminator3" if gan else None, **KW)
    O.seeded_state_fill(o, seed)
    m = dmcnet_amd.Model(num_class, 3, "mv", arch_d="Discriminator3" if gan else None, **KW)
    m.load_state_dict(o.state_dict())
    return o.train(), m.to(DEV).train()


def _adam_step(key):
    """lr * lr_mult of the optimizer that owns ``key`` (HP of the shipped recipes)."""
    mult = HP["lr_cls_mult"] if key.startswith("base_model") else \
        HP["lr_mse_mult"] if key.startswith("gen_flow_model") else HP["lr_d_mult"]
    return HP["lr"] * mult


def _check_post_step(model, oracle, keys, frac):
    so, sm = oracle.state_dict(), model.state_dict()
    for k in keys:
        a, b = sm[k].float().cpu(), so[k].float()
        if "running_" in k:                       # BatchNorm statistics: plain relative bar
            assert rel_err(a, b) < 1e-4, k
        else:
            assert float((a - b).abs().max()) <= frac * _adam_step(k), (k, float((a - b).abs().max()))


@pytest.mark.parametrize("num_class", [51, 101])
def test_dmcnet_step_full_batch_vs_oracle(num_class):
    """One config-2 step at B=40 (C=51) and config 4's per-rank workload (C=101): BatchNorm
    statistics over 120 frames, the 1e-4 bar on the consensus logits at the real batch, post-step
    weights of all three parameter families."""
    o, m = _pair(num_class, False, 141)
    batch = O.synthetic_batch(seed=142, batch=40, num_segments=3, num_class=num_class, flow_ds_factor=16)
    oc, og = O.make_optimizers(o, **OPT)
    for opt in (oc, og):          # what the reference's main() does before every epoch (train.py:398-408)
        O.adjust_learning_rate(opt, 0, [20, 35, 45], 0.1, HP["lr"], HP["weight_decay"])
    ref = O.dmcnet_train_step(o, oc, og, batch, 3, HP["lr_cls"], HP["lr_mse"])
    step = T.DmcnetTrainStep(m, 3, HP["lr_cls"], HP["lr_mse"], **OPT)
    got = step.step(tuple(t.to(DEV) for t in batch))
    for k in ("loss", "loss_cls", "loss_mse", "output"):
        assert rel_err(got[k], ref[k]) < 1e-4, (k, rel_err(got[k], ref[k]))
    assert got["output"].shape == (40, num_class)
    assert rel_err(got["gen_flow"], ref["gen_flow"]) < 1e-5
    # gradients that survive the step (p.grad is not cleared until the next zero_grad).  The generator's
    # come from the short MSE graph: plain relative bar.  The classifier's pass 17 BatchNorm layers
    # backwards (dy - mean(dy) - xhat mean(dy xhat) cancels) and are only ~1e-3 accurate in ANY fp32
    # implementation: the bar is accuracy against an fp64 evaluation of the same graph -- the HIP path
    # may be at most 4x further from it than the fp32 CPU oracle is.
    po, pm = dict(o.named_parameters()), dict(m.named_parameters())
    for k in ("gen_flow_model.predict_flow.weight", "gen_flow_model.conv_0.0.weight"):
        assert rel_err(pm[k].grad, po[k].grad) < 2e-4, (k, rel_err(pm[k].grad, po[k].grad))
    if num_class == 51:
        o64, _ = _pair(num_class, False, 141)                 # same seeded weights as before the step
        o64 = o64.double()
        cue = ref["gen_flow"].double()                        # the classifier sees the detached cue
        logits = O.consensus(o64.base_model(cue), 3)
        torch.nn.functional.cross_entropy(logits, batch[3]).backward()
        p64 = dict(o64.named_parameters())
        worst = 0.0
        for k in ("base_model.fc.weight", "base_model.layer4.1.conv2.weight", "base_model.layer2.0.conv1.weight",
                  "base_model.layer1.0.conv1.weight", "base_model.conv1.weight", "base_model.bn1.weight"):
            e_hip, e_ref = rel_err(pm[k].grad, p64[k].grad), rel_err(po[k].grad, p64[k].grad)
            worst = max(worst, e_hip)
            assert e_hip <= max(4 * e_ref, 1e-4), (k, e_hip, e_ref)
        print("classifier gradients at B=40: worst HIP-vs-fp64 error %.1e" % worst)
    # generator: 5 % of its Adam step.  Classifier: 25 % -- a SMOKE bound only (it catches a missing or doubled
    # update, not a gradient error): the classifier's gradients carry the ~1e-3 fp32 error of the BatchNorm chain,
    # which Adam(eps=1e-3) maps to up to ~lr/4eps times that in the update.  The real check of the classifier's
    # gradients is the fp64-anchored criterion above.
    _check_post_step(m, o, [k for k in WATCH if k.startswith("gen_flow_model")], 0.05)
    _check_post_step(m, o, [k for k in WATCH if not k.startswith("gen_flow_model")] +
                     ["base_model.conv1.weight", "base_model.layer4.1.conv2.weight"], 0.25)


@pytest.mark.parametrize("num_class", [51, 101])
def test_gan_step_pair_full_batch_vs_oracle(num_class):
    """Config 3 at B=40 (C=51) and config 4's per-rank workload (dmcnet_GAN on UCF-101, C=101,
    code/dmcnet_GAN/train.py:43-44,261-371): a D step (240 frames through Discriminator3, classifier +
    discriminator step) followed by a G step (generator steps), Dropout2d masks forced to the oracle's."""
    o, m = _pair(num_class, True, 143)
    b0 = O.synthetic_batch(seed=144, batch=40, num_segments=3, num_class=num_class)
    b1 = O.synthetic_batch(seed=145, batch=40, num_segments=3, num_class=num_class)
    md = O.seeded_dropout_masks(146, o.discriminator, 240)
    mg = O.seeded_dropout_masks(147, o.discriminator, 120)
    oopts = O.make_optimizers(o, lr_d_mult=HP["lr_d_mult"], **OPT)
    for opt in oopts:
        O.adjust_learning_rate(opt, 0, [20, 35, 45], 0.1, HP["lr"], HP["weight_decay"])
    step = T.GanTrainStep(m, 3, HP["lr_cls"], HP["lr_adv_g"], HP["lr_adv_d"], HP["lr_mse"],
                          lr_d_mult=HP["lr_d_mult"], **OPT)
    for i, (b, masks) in enumerate(((b0, md), (b1, mg))):
        o.discriminator.forced_masks = masks
        m.discriminator.forced_masks = masks
        ref = O.gan_train_step(o, oopts[0], oopts[1], oopts[2], b, i, 3, HP["lr_cls"], HP["lr_adv_g"],
                               HP["lr_adv_d"], HP["lr_mse"])
        got = step.step(tuple(t.to(DEV) for t in b), i)
        for k in ("loss", "loss_cls", "loss_adv", "output", "validity") + (("loss_mse",) if i else ()):
            assert rel_err(got[k], ref[k]) < 2e-4, (i, k, rel_err(got[k], ref[k]))
        assert got["validity"].shape == ((240, 2) if i == 0 else (120, 2))
        # weights that stepped in this phase: D step -> classifier + discriminator, G step -> generator
        keys = [k for k in WATCH + WATCH_D if ("gen_flow_model" in k) == (i == 1)]
        _check_post_step(m, o, keys, 0.25)
        if i == 0:
            # The G step is checked from IDENTICAL weights: after the D step the two classifiers differ by Adam-normalised
            # rounding noise (<= 0.16 of a step), which the G step's Adam (lr * dg / eps for |g| <~ eps) turns into 0.2-0.6 of
            # a step on the generator weights whatever the convolution path (measured with tools/gan_full_batch_diag.py:
            # MIOpen 0.23, fp32 MFMA 0.30, bf16x3 0.28) -- a property of the comparison, not of the kernels.  The
            # generator's optimizer has not stepped yet, so no optimizer state is lost.
            m.load_state_dict(o.state_dict())


@pytest.mark.parametrize("gan", [False, True])
def test_full_batch_step_is_bitwise_deterministic(gan):
    """Two B=40 steps from the same state on the same batch (a D step + a G step for the GAN variant): every kernel of
    the default path has a fixed reduction order (no atomics; the convolutions, BatchNorm sums, weight gradients and
    the generator reduce partials in a fixed order), so losses, logits, the generated flow and EVERY parameter and
    BatchNorm buffer after the optimizer steps are bit-identical."""
    from dmcnet_amd import resnet
    if not resnet.OWN_CONV:
        pytest.skip("MIOpen's split-K weight gradients use atomics")
    runs = []
    for _ in range(2):
        _, m = _pair(51, gan, 151)
        batches = [O.synthetic_batch(seed=152 + i, batch=40, num_segments=3, num_class=51, flow_ds_factor=0 if gan else 16)
                   for i in range(2 if gan else 1)]
        outs = []
        if gan:
            step = T.GanTrainStep(m, 3, HP["lr_cls"], HP["lr_adv_g"], HP["lr_adv_d"], HP["lr_mse"],
                                  lr_d_mult=HP["lr_d_mult"], **OPT)
            for i, b in enumerate(batches):
                m.discriminator.forced_masks = O.seeded_dropout_masks(160 + i, m.discriminator, 240 if i == 0 else 120)
                outs.append(step.step(tuple(t.to(DEV) for t in b), i))
        else:
            step = T.DmcnetTrainStep(m, 3, HP["lr_cls"], HP["lr_mse"], **OPT)
            outs.append(step.step(tuple(t.to(DEV) for t in batches[0])))
        runs.append((outs, {k: v.detach().clone() for k, v in m.state_dict().items()}))
    (oa, sa), (ob, sb) = runs
    for ra, rb in zip(oa, ob):
        for k in ra:
            if torch.is_tensor(ra[k]):
                assert torch.equal(ra[k], rb[k]), k
    for k in sa:
        assert torch.equal(sa[k], sb[k]), k


def _generic_case(seed, frames):
    import copy
    o = O.seeded_state_fill(O.build_estimator("DenseNetTiny"), 15)
    m = dmcnet_amd.model.EstimatorDenseNetTiny(5)
    m.load_state_dict(o.state_dict())
    m.to(DEV)
    rs = np.random.RandomState(seed)
    x = torch.from_numpy(rs.standard_normal((frames, 5, 224, 224)).astype(np.float32))
    r = torch.from_numpy(rs.standard_normal((frames, 2, 224, 224)).astype(np.float32))
    return o, copy.deepcopy(o).double(), m, x, r


# (seed, frames, backward selection): the five data seeds of tools/gen_flip_lottery.py at 16 frames each for the default backward and
# for every data-gradient group on the Winograd kernel (mask 0x1F00); the full
# 120-frame batch once.  (16 frames = 0.8 M pixels per seed: the CPU side -- one fp32 and three fp64 passes -- sets the run time.)
GENERIC_CASES = ([(s, 16, m) for s in (23, 24, 25, 26, 27) for m in (0x300, 0x1F00)] + [(23, 120, 0x300)])


@pytest.mark.parametrize("seed,frames,backward_mask", GENERIC_CASES)
def test_generator_full_batch_generic_weights(seed, frames, backward_mask):
    """224 x 224 frames with GENERIC weights (mixed-sign pre-activations in every tile), conditioned on the run's own LeakyReLU
    branches (tests/gen_conditioned.py): every parameter gradient of the device run is compared with the fp64 backward whose
    slopes are FORCED to the signs the device run took (its saved features), the fp32 CPU oracle's with the fp64 backward
    forced to ITS signs; what is left is arithmetic, and the bar is <= 2x the oracle's distance.  The branch decisions
    themselves are counted: the device forward may disagree with the fp64 forward in at most 4x as many places as the oracle does.
    (The unconditioned ratio this replaces read 1x .. 200x over these seeds for EVERY kernel selection, the exact-fp32 ones
    included: profiles/r4_gen_wino.txt.)  Runs for the default kernel selection and with every data-gradient group on the
    Winograd kernel; the forward is the fused one-launch kernel (csrc/gen_fused.hip)."""
    from tests.gen_conditioned import conditioned_report
    o, o64, m, x, r = _generic_case(seed, frames)
    lib = dmcnet_amd._lib.load()
    before = lib.dmc_get_option(b"gen_wino")
    dmcnet_amd._lib.check(lib.dmc_set_option(b"gen_wino", backward_mask), "dmc_set_option")
    try:
        y = m.forward_mv_res(x[:, :2].contiguous().to(DEV), x[:, 2:].contiguous().to(DEV), add_mv=True)
        saved = y.grad_fn.saved_tensors[2].view(frames, 28, 224, 224)
        (y * r.to(DEV)).sum().backward()
    finally:
        dmcnet_amd._lib.check(lib.dmc_set_option(b"gen_wino", before), "dmc_set_option")
    rep = conditioned_report(o, o64, x, r, y.detach(), [p.grad for p in m.parameters()], saved)
    print("seed %d, %d frames: sign disagreements with fp64: device %d, oracle %d; output error %.2e (oracle %.2e)"
          % (seed, frames, rep["flips_hip"], rep["flips_ref"], rep["e_out_hip"], rep["e_out_ref"]))
    assert rep["flips_hip"] <= 4 * rep["flips_ref"] + 16, rep
    assert rep["e_out_hip"] <= max(2 * rep["e_out_ref"], 1e-6), rep
    for k, (e_hip, e_ref) in rep["params"].items():
        assert e_hip <= max(2 * e_ref, 2e-6), (k, e_hip, e_ref)


def _run_two_ranks(tmp_path, phase):
    port = 29600 + (os.getpid() % 300)
    procs = []
    for rank in range(2):
        env = dict(os.environ, RANK=str(rank), WORLD_SIZE="2", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port),
                   HSA_ENABLE_IPC_MODE_LEGACY="0")
        procs.append(subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "two_rank_worker.py"),
                                       phase, str(tmp_path)], env=env, cwd=ROOT,
                                      stdout=subprocess.PIPE, stderr=subprocess.STDOUT))
    outs = [p.communicate(timeout=600)[0].decode() for p in procs]
    for p, out in zip(procs, outs):
        assert p.returncode == 0, out[-3000:]
    return [torch.load(os.path.join(str(tmp_path), "%s_r%d.pt" % (phase, r))) for r in range(2)]


@pytest.mark.parametrize("phase", ["dmcnet", "gan"])
def test_two_ranks_on_one_gpu_match_single_process_shards(tmp_path, phase):
    """world_size 2 on ONE GPU (gloo transport, CUDA tensors): the real Model + HIP autograd +
    GradBucketReducer (per-optimizer bucket sets) + fused Adam on bucket views.  Each rank takes 2 of 4
    clips.  Expected gradients: the two shards evaluated one after the other in THIS process (per-rank
    BatchNorm statistics, as under DataParallel) and averaged."""
    r0, r1 = _run_two_ranks(tmp_path, phase)
    gan = phase == "gan"
    from tests.two_rank_worker import build, shard_batches, run_phases
    from dmcnet_amd import resnet
    expected = {}
    for rank in range(2):
        m = build(gan).to(DEV).train()
        res = run_phases(m, shard_batches(rank), gan, reducer=None, do_step=False, shard=rank,
                         state_after_first=r0["state_after_first"] if gan else None)
        for tag, grads in res["grads"].items():
            for k, g in grads.items():
                acc = expected.setdefault(tag, {})
                acc[k] = g.double() / 2 if k not in acc else acc[k] + g.double() / 2
    for tag in expected:
        for k, ge in expected[tag].items():
            g0, g1 = r0["grads"][tag][k], r1["grads"][tag][k]
            assert torch.equal(g0, g1), (tag, k)                       # identical on both ranks after the exchange
            # (1) the exchange itself: exactly the mean of the two ranks' own gradients (captured by hooks
            #     that run before the reducer's)
            mean_local = (r0["local"][tag][k].double() + r1["local"][tag][k].double()) / 2
            scale = float(mean_local.abs().max()) + 1e-30
            assert float((g0.double() - mean_local).abs().max()) <= 1e-6 * scale, (tag, k)
            # (2) against the two shards evaluated one after the other in THIS process.  Every kernel on the
            #     default path (own convolutions, DMC_OWN_CONV=1) has a fixed reduction order, so another
            #     process computes the same per-shard gradients; what is left is the fp32 rounding of the
            #     exchange's mean against the float64 mean taken here (<= 1 ulp of the largest entry) -> 1e-5,
            #     2e-6 for the generator's short MSE graph.  Only the stock path (DMC_OWN_CONV=0) goes through
            #     MIOpen, which may choose another algorithm in another process; there the BatchNorm backward
            #     chain (batch statistics over 6 frames, 294 values per channel in layer4) amplifies the
            #     reordering to percents of the largest entry and the bar is a sanity bound only.
            err = float((g0.double() - ge).abs().max()) / (float(ge.abs().max()) + 1e-30)
            if tag == "step" and k.startswith("gen_flow_model"):
                bar = 2e-6
            else:
                bar = 1e-5 if resnet.OWN_CONV else 0.25
            assert err < bar, (tag, k, err)
        assert set(r0["grads"][tag]) == set(expected[tag]), tag       # same set of parameters received a gradient
    # which buckets travelled
    sets = {tag: set(b) for tag, b in r0["bytes"].items()}
    if gan:
        assert sets["D"] == {"base_model", "discriminator"} and sets["G"] == {"gen_flow_model"}
        assert sum(r0["bytes"]["G"].values()) == 4584 * 4
    else:
        assert sets["step"] == {"base_model", "gen_flow_model"}
    assert all(w == "hook" for tag in r0["where"] for w in r0["where"][tag])
    # parameters identical across ranks after the optimizer steps
    for k in r0["params"]:
        assert torch.equal(r0["params"][k], r1["params"][k]), k
