"""Whole plans with fuse_inference(squeezes=True) on the GPU: a two-block squeeze-excite network per spelling (EfficientNet's Linear /
swish / sigmoid, MobileNetV3's 1x1 convolutions / ReLU / hard sigmoid; widths 32 / 8 and 96 / 24), batch 3 at 32^2, under FSPTQ and QBase
W8A8.  The logits are torch.equal to the same plan with every SqueezeLayer running its restatement (K.squeeze_gate_torch: the kernels
that were there before).  Against the flag-off plan only finiteness and the shape are asserted, the differing logits printed: the pool's
summation order and the integer layers move values across quantiser ties (DESIGN.md 5.23 found the same for LayerNorm)."""
import functools

import pytest
import torch
from torch import nn

import workloads as W
from test_gpu_gate import DEV, PLAN_CASES, _net, tagged

pytestmark = pytest.mark.gpu
SPELLINGS = {"linear_swish_sigmoid": dict(gate="sigmoid", squeeze="linear"), "conv_relu_hardsigmoid": dict(gate="hardsigmoid", squeeze="conv")}


class TwoBlocks(nn.Module):
    def __init__(self, **se):
        super().__init__()
        self.stem = nn.Sequential(nn.Conv2d(3, 32, 3, padding=1, bias=False), nn.BatchNorm2d(32), nn.ReLU())
        self.se1 = W.SqueezeExcite(32, 8, **se)
        self.mid = nn.Sequential(nn.Conv2d(32, 96, 1, bias=False), nn.BatchNorm2d(96), nn.ReLU())
        self.se2 = W.SqueezeExcite(96, 24, **se)
        self.last = nn.Sequential(nn.Conv2d(96, 64, 1, bias=False), nn.BatchNorm2d(64), nn.ReLU())
        self.pool, self.fc = nn.AdaptiveAvgPool2d(1), nn.Linear(64, 10)

    def forward(self, x):
        x = self.last(self.se2(self.mid(self.se1(self.stem(x)))))
        return self.fc(torch.flatten(self.pool(x), 1))


@functools.lru_cache(maxsize=None)
def plans(spelling, tag):
    from dlmc.utils.fuse import fuse_inference
    cfg, qtype, _ = PLAN_CASES[tag]
    net, x = _net(functools.partial(TwoBlocks, **SPELLINGS[spelling]), 3, cfg, qtype, 71, False)
    return fuse_inference(net, gates=True), fuse_inference(net, gates=True, squeezes=True), x[:3].contiguous()


@pytest.mark.parametrize("tag", ["fsptq", "qbase"])
@pytest.mark.parametrize("spelling", sorted(SPELLINGS))
def test_plan_equals_the_plan_of_restated_nodes(spelling, tag):
    from dlmc.utils.fuse import SqueezeLayer
    off, on, x = plans(spelling, tag)
    rep = on.fusion_report
    print(rep)
    nodes = [m for m in on.modules() if isinstance(m, SqueezeLayer)]
    assert rep.squeezes == 2 == len(nodes) and rep.gates == 2 == off.fusion_report.gates and rep.squeeze_left == [] and rep.skipped == []
    assert sorted((m.c, m.r) for m in nodes) == [(32, 8), (96, 24)]
    with torch.no_grad():
        a, tags = tagged(lambda: on(x))
        assert tags.count("squeeze") == 2 and torch.equal(a, on(x))
        for m in nodes:
            m.forward = m.restated
        try:
            b, tags_b = tagged(lambda: on(x))
        finally:
            for m in nodes:
                del m.forward
        base = off(x)
    assert "squeeze" not in tags_b and torch.equal(a, b), f"{int((a != b).sum())} of {a.numel()} logits differ from the restated plan"
    d = (a - base).abs()
    print(f"{spelling} {tag}: against the flag-off plan {int((d != 0).sum())} of {a.numel()} logits differ, by at most {float(d.max()):.3g} "
          f"(largest logit {float(base.abs().max()):.3g})")
    assert a.shape == base.shape and bool(torch.isfinite(a).all()) and bool(torch.isfinite(base).all())


@pytest.mark.parametrize("spelling", sorted(SPELLINGS))
def test_inputs_the_kernel_path_does_not_take_run_the_restatement(spelling):
    from dlmc.utils.fuse import SqueezeLayer
    _, on, _ = plans(spelling, "fsptq")
    node = next(m for m in on.modules() if isinstance(m, SqueezeLayer) and m.c == 32)
    torch.manual_seed(3)
    x = torch.relu(torch.randn(3, 32, 8, 8, device=DEV)).contiguous(memory_format=torch.channels_last)
    with torch.no_grad():
        want, tags = tagged(lambda: node(x))
        assert "squeeze" in tags and want.shape == (3, 32, 1, 1)
        for other in (x.contiguous(), x.double()):      # NCHW-dense; not fp32
            got, tags = tagged(lambda: node(other))
            assert "squeeze" not in tags and got.dtype == torch.float32 and torch.equal(got, want)
        with pytest.raises(ValueError, match="map"):
            node(torch.zeros(3, 16, 8, 8, device=DEV))
