"""Three small networks with a swish in the three spellings fuse_inference(swish=True) meets (tests/test_swish_host.py,
tests/test_swish_gpu.py), each convolution -> swish -> plan convolution.  Each carries `reader`: the name of a convolution that reads
an activated map as codes, and `swishes`: how many swishes on maps it has."""
import torch
import torch.nn.functional as F
from torch import nn


class Swish(nn.Module):
    """A user module whose body is the multiply (EfficientNet's `swish` class): traced into it."""

    def forward(self, x):
        return torch.sigmoid(x) * x


class MulSwish(nn.Module):
    """`sigmoid(x) * x` in a user module behind a 3x3 convolution, read by a 1x1 plan convolution as codes AND by the shortcut add behind
    the next one as fp32 (the second reader); then `x * x.sigmoid()` read by one plan convolution alone.  64 channels: unpadded code rows,
    shifted where the quantiser is unsigned."""
    reader, swishes = "b", 2

    def __init__(self):
        super().__init__()
        self.a = nn.Conv2d(16, 64, 3, padding=1)
        self.act = Swish()
        self.b = nn.Conv2d(64, 64, 1)
        self.b2 = nn.Conv2d(64, 64, 1)
        self.c = nn.Conv2d(64, 32, 3, padding=1)

    def forward(self, inp):
        s = self.act(self.a(inp))
        t = self.b2(torch.relu(self.b(s))) + s
        return self.c(t * t.sigmoid())


class ModuleSiLU(nn.Module):
    """nn.SiLU behind a channel-padded producer (48 of 64 channels: the map is a channel slice, read in place), read by a depthwise plan
    convolution; a second nn.SiLU read by the 1x1 projection (code rows padded to 64); an identity shortcut."""
    reader, swishes = "proj", 2

    def __init__(self):
        super().__init__()
        self.expand = nn.Conv2d(16, 48, 1)
        self.act1 = nn.SiLU()
        self.dw = nn.Conv2d(48, 48, 3, padding=1, groups=48)
        self.act2 = nn.SiLU()
        self.proj = nn.Conv2d(48, 16, 1)
        self.head = nn.Conv2d(16, 64, 1)

    def forward(self, inp):
        return self.head(inp + self.proj(self.act2(self.dw(self.act1(self.expand(inp))))))


class FunctionalSiLU(nn.Module):
    """F.silu behind a 3x3 convolution, read by a 3x3 plan convolution; torch.mul(x, torch.sigmoid(x)) read by a 1x1 one."""
    reader, swishes = "b", 2

    def __init__(self):
        super().__init__()
        self.a = nn.Conv2d(16, 32, 3, padding=1)
        self.b = nn.Conv2d(32, 64, 3, padding=1)
        self.c = nn.Conv2d(64, 32, 1)

    def forward(self, inp):
        x = self.b(F.silu(self.a(inp)))
        return self.c(torch.mul(x, torch.sigmoid(x)))
