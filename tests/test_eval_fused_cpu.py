"""CPU: the predicates behind the one-launch eval dispatch (ops.conv_bn_eval_supported, ops.s2_pair_eval_usable) are False for
CPU tensors, with autograd on and with a BatchNorm in training mode -- the units then run on the stock modules -- and the
DMC_EVAL_FUSED switch of resnet.py is read from the environment."""
import os
import subprocess
import sys

import torch

from dmcnet_amd import ops, resnet

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _unit():
    return resnet.ResidualUnit("basic", 64, 128, 2).eval()


def test_predicates_are_false_on_the_cpu():
    u = _unit()
    x = torch.zeros(2, 64, 28, 28).contiguous(memory_format=torch.channels_last)
    with torch.no_grad():
        assert not ops.s2_pair_eval_usable(tuple(x.shape), u)
        assert not ops.conv_bn_eval_supported(x, u.conv2, u.bn2)
        assert not ops.conv_bn_eval_supported(torch.zeros(2, 128, 14, 14).contiguous(memory_format=torch.channels_last), u.conv2, u.bn2)
        assert u(x).shape == (2, 128, 14, 14)                      # the stock modules serve the unit


def test_predicates_need_no_grad_and_eval_batchnorms():
    """The mode / structure half of the pair predicate (ops._s2_pair_eval_unit_ok: everything but the device and the shape) on a
    CPU unit, and ops.conv_bn_eval_supported's mode checks."""
    u = _unit()
    with torch.no_grad():
        assert ops._s2_pair_eval_unit_ok(u)
        assert not ops.s2_pair_eval_usable((2, 64, 28, 28), u)     # ... but the weights are not on the GPU
    assert not ops._s2_pair_eval_unit_ok(u)                        # autograd on
    assert not ops.s2_pair_usable((2, 64, 28, 28), u)              # ... and the training predicate wants training BatchNorms
    with torch.no_grad():
        u.bn1.train()
        assert not ops._s2_pair_eval_unit_ok(u)
        u.bn1.eval(); u.downsample[1].train()
        assert not ops._s2_pair_eval_unit_ok(u)
        u.downsample[1].eval()
        assert ops._s2_pair_eval_unit_ok(u)
        assert not ops._s2_pair_eval_unit_ok(resnet.ResidualUnit("basic", 64, 64, 1).eval())        # no downsample branch
        assert not ops._s2_pair_eval_unit_ok(resnet.ResidualUnit("bottleneck", 64, 64, 2).eval())
    x = torch.zeros(2, 128, 14, 14).contiguous(memory_format=torch.channels_last)
    v = _unit()
    assert not ops.conv_bn_eval_supported(x, v.conv2, v.bn2)       # autograd on
    with torch.no_grad():
        v.bn2.train()
        assert not ops.conv_bn_eval_supported(x, v.conv2, v.bn2)


def test_env_switch_is_honoured():
    code = "import sys; sys.path.insert(0, %r); from dmcnet_amd import resnet; print(int(resnet.EVAL_FUSED))" % ROOT
    for value, want in ((None, "1"), ("0", "0"), ("1", "1")):
        env = dict(os.environ)
        env.pop("DMC_EVAL_FUSED", None)
        if value is not None:
            env["DMC_EVAL_FUSED"] = value
        out = subprocess.run([sys.executable, "-c", code], env=env, stdout=subprocess.PIPE, check=True, universal_newlines=True).stdout
        assert out.strip().splitlines()[-1] == want, (value, out)
