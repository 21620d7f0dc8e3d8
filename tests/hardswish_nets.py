"""Small networks with a hard swish in each spelling fuse_inference(hardswish=True) meets (tests/test_hardswish_host.py,
tests/test_hardswish_gpu.py).  Each is the same two blocks on a 2 x 8 x 9 x 9 input, widths 8, 24 and 8: a MobileNetV3 unit - 1x1
expansion -> hard swish -> depthwise 3x3 -> hard swish -> squeeze-excite (convolution squeeze, hard sigmoid) -> 1x1 projection with an
identity shortcut - then a 1x1 convolution whose hard swish nobody takes as codes (a global mean reads it).  `NETS`: spelling -> (the
network's class, the order of the kernel's two multiplies that computes the spelling: DESIGN.md 5.30's table)."""
import torch
import torch.nn.functional as F
from torch import nn

import workloads as W


class FunctionalHardswish(nn.Module):
    def forward(self, x):
        return F.hardswish(x)


class MulDiv(nn.Module):
    """(x * r) / 6"""

    def forward(self, x):
        return x * F.relu6(x + 3) / 6


class MulSixth(nn.Module):
    """(r * x) * (1 / 6), the ReLU6 a module, the sum spelled 3 + x"""

    def __init__(self):
        super().__init__()
        self.relu6 = nn.ReLU6(inplace=True)

    def forward(self, x):
        return (self.relu6(3.0 + x) * x) * (1.0 / 6.0)


class GateDiv(nn.Module):
    """x * (r / 6), the ReLU6 spelled F.hardtanh(., 0, 6)"""

    def forward(self, x):
        return x * (F.hardtanh(x + 3.0, 0.0, 6.0) / 6.0)


class GateDivGateFirst(nn.Module):
    """(r / 6) * x"""

    def forward(self, x):
        return torch.div(F.relu6(torch.add(x, 3)), 6) * x


class TimesHardsigmoid(nn.Module):
    def forward(self, x):
        return x * F.hardsigmoid(x)


class HardsigmoidModuleTimes(nn.Module):
    """nn.Hardsigmoid()(x) * x: the gate first"""

    def __init__(self):
        super().__init__()
        self.gate = nn.Hardsigmoid()

    def forward(self, x):
        return torch.mul(self.gate(x), x)


class HardswishNet(nn.Module):
    """The two blocks, with `act()` as every hard swish.  `reader`: a convolution that reads an activated map as codes; `hardswishes`: how
    many hard swishes on maps it has; `codes`: how many of them hand codes on (the expansion's to the depthwise layer; the depthwise
    layer's is read by the squeeze-excite pool and gate, the last one's by the mean)."""
    reader, hardswishes, codes = "dw", 3, 1

    def __init__(self, act):
        super().__init__()
        self.expand = nn.Conv2d(8, 24, 1)
        self.act1 = act()
        self.dw = nn.Conv2d(24, 24, 3, padding=1, groups=24)
        self.act2 = act()
        self.se = W.SqueezeExcite(24, 8, gate="hardsigmoid", squeeze="conv")
        self.proj = nn.Conv2d(24, 8, 1)
        self.last = nn.Conv2d(8, 24, 1)
        self.act3 = act()
        self.fc = nn.Linear(24, 10)

    def forward(self, inp):
        t = inp + self.proj(self.se(self.act2(self.dw(self.act1(self.expand(inp))))))
        return self.fc(self.act3(self.last(t)).mean((2, 3)))


def _net(act):
    return type("Net" + act.__name__, (HardswishNet,), dict(__init__=lambda self: HardswishNet.__init__(self, act)))


NETS = {"nn.Hardswish": (_net(nn.Hardswish), "mul_first"), "F.hardswish": (_net(FunctionalHardswish), "mul_first"),
        "x * relu6(x + 3) / 6": (_net(MulDiv), "mul_first"), "(relu6(3 + x) * x) * (1 / 6)": (_net(MulSixth), "mul_first"),
        "x * (relu6(x + 3) / 6)": (_net(GateDiv), "gate_first"), "(relu6(x + 3) / 6) * x": (_net(GateDivGateFirst), "gate_first"),
        "x * F.hardsigmoid(x)": (_net(TimesHardsigmoid), "gate_first"), "nn.Hardsigmoid()(x) * x": (_net(HardsigmoidModuleTimes), "gate_first")}
