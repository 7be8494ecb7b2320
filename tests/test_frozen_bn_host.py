"""Host-side pieces of train.py --freeze-bn (no GPU): the flag, the warning line, the freeze loop, and that the launch tape's
eligibility does not depend on it."""
import os
import sys
import types

import torch.nn as nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import train  # noqa: E402


def _args(*extra):
    return train.build_parser().parse_args(["DIR"] + list(extra))


def test_parser_accepts_freeze_bn():
    assert _args().freeze_bn is False
    a = _args("--freeze-bn", "--sgd", "--no-tape", "--pretrained-disp", "ckpt.pth.tar")
    assert a.freeze_bn is True and a.sgd is True and a.tape is False and a.pretrained_disp == "ckpt.pth.tar"


def test_warning_only_without_a_pretrained_network():
    assert train.freeze_bn_warning(_args()) is None
    assert train.freeze_bn_warning(_args("--pretrained-disp", "ckpt.pth.tar")) is None
    assert train.freeze_bn_warning(_args("--freeze-bn", "--pretrained-disp", "ckpt.pth.tar")) is None
    line = train.freeze_bn_warning(_args("--freeze-bn"))
    assert isinstance(line, str) and "\n" not in line and "--freeze-bn" in line and "--pretrained-disp" in line


def test_freeze_loop_puts_exactly_the_batchnorms_in_eval_mode():
    net = nn.Sequential(nn.Conv2d(3, 4, 3), nn.BatchNorm2d(4), nn.ReLU(), nn.Sequential(nn.Conv2d(4, 4, 3), nn.BatchNorm2d(4)), nn.Dropout2d())
    net.train()
    assert train.freeze_batchnorm(net) == 2
    assert net.training and net[0].training and net[4].training and net[3].training
    assert not net[1].training and not net[3][1].training
    net.train()                                     # the next epoch's net.train() thaws them: train() freezes again every epoch
    assert net[1].training
    assert train.freeze_batchnorm(net) == 2 and not net[1].training


def test_tape_refusal_does_not_depend_on_freeze_bn():
    fused, plain = types.SimpleNamespace(arena=object()), types.SimpleNamespace()
    for extra in ((), ("--sgd",), ("--loss", "DORN"), ("--unsupervised",), ("-s", "0.1")):
        a, b = _args(*extra), _args("--freeze-bn", *extra)
        for opt in (fused, plain):
            assert train.tape_refusal(a, opt) == train.tape_refusal(b, opt)
    assert train.tape_refusal(_args("--freeze-bn"), fused) is None
