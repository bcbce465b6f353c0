"""What the custom ResNet-torso path promises without a GPU: when it is
eligible, that the conv weights are laid out for it, that the state_dict
still round-trips, and that its kernels are part of the build."""

import torch

from distributed_reinforcement_learning_amd import ops
from distributed_reinforcement_learning_amd.models.impala_resnet import (
    ImpalaResNetActorCritic, ImpalaResNetTorso,
)
from distributed_reinforcement_learning_amd.ops import build as ops_build
from distributed_reinforcement_learning_amd.ops import resnet_op


class _Frames:
    """Stands in for a GPU frame batch: resnet_torso_ok reads only these."""

    def __init__(self, shape, is_cuda=True):
        self.shape = torch.Size(shape)
        self.is_cuda = is_cuda


def test_resnet_torso_ok_conditions(monkeypatch):
    monkeypatch.delenv("DRLA_RESNET_CONV", raising=False)
    monkeypatch.setattr(ops, "available", lambda: True)
    bf16 = ImpalaResNetTorso(4).to(torch.bfloat16)
    good = _Frames((8, 84, 84, 4))
    # the positive control: everything below flips exactly one condition
    assert resnet_op.resnet_torso_ok(bf16, good)
    assert not resnet_op.resnet_torso_ok(bf16, _Frames((8, 84, 84, 4), False))
    assert not resnet_op.resnet_torso_ok(
        bf16, torch.zeros(2, 84, 84, 4, dtype=torch.bfloat16))
    assert not resnet_op.resnet_torso_ok(ImpalaResNetTorso(4), good)
    for shape in ((8, 64, 64, 4), (8, 84, 84, 1), (8, 84, 84), (8, 42, 84, 4)):
        assert not resnet_op.resnet_torso_ok(bf16, _Frames(shape))
    assert not resnet_op.resnet_torso_ok(
        ImpalaResNetTorso(4, channels=(16, 32, 64)).to(torch.bfloat16), good)
    assert not resnet_op.resnet_torso_ok(
        ImpalaResNetTorso(1).to(torch.bfloat16), _Frames((8, 84, 84, 1)))
    # the switch is read at call time
    monkeypatch.setenv("DRLA_RESNET_CONV", "0")
    assert not resnet_op.resnet_torso_ok(bf16, good)
    monkeypatch.setenv("DRLA_RESNET_CONV", "1")
    assert resnet_op.resnet_torso_ok(bf16, good)
    monkeypatch.delenv("DRLA_RESNET_CONV")
    monkeypatch.setattr(ops, "available", lambda: False)
    assert not resnet_op.resnet_torso_ok(bf16, good)


def test_conv_weights_are_channels_last_and_flat_view_is_free():
    for dtype in (torch.float32, torch.bfloat16):
        torso = ImpalaResNetTorso(4).to(dtype)
        convs = [m for m in torso.modules()
                 if isinstance(m, torch.nn.Conv2d)]
        assert len(convs) == 15
        for c in convs:
            w = c.weight
            assert w.is_contiguous(memory_format=torch.channels_last)
            flat = resnet_op._flat(c)
            assert flat.shape == (w.shape[0], 9 * w.shape[1])
            assert flat.data_ptr() == w.data_ptr() and flat.is_contiguous()


def test_state_dict_round_trip_gives_identical_cpu_outputs():
    torch.manual_seed(0)
    a = ImpalaResNetActorCritic((84, 84, 4), 6, lstm_hidden_size=32)
    torch.manual_seed(1)
    b = ImpalaResNetActorCritic((84, 84, 4), 6, lstm_hidden_size=32)
    sd = a.state_dict()
    assert sd["conv.sections.0.conv.weight"].shape == (16, 4, 3, 3)
    assert sd["conv.sections.2.r2.c2.bias"].shape == (32,)
    b.load_state_dict(sd)
    x = torch.rand(2, 84, 84, 4)
    pa = torch.tensor([1, 3])
    h = torch.zeros(2, 32)
    with torch.no_grad():
        out_a = a.single_step(x, pa, h, h)
        out_b = b.single_step(x, pa, h, h)
    for ta, tb in zip(out_a, out_b):
        assert torch.equal(ta, tb)


def test_new_kernels_are_in_the_build():
    assert "conv3x3.hip" in ops_build.SOURCES
    assert resnet_op.SECTION_LAYERS == ((4, 5), (6, 7), (7, 8))
