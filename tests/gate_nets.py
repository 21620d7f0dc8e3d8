"""Three small networks with a squeeze-excite gate in the three spellings fuse_inference(gates=True) meets (tests/test_gate_host.py,
tests/test_gpu_gate.py).  Each carries `reader`: the name of the convolution that reads the gated map."""
import torch
import torch.nn.functional as F
from torch import nn


class MBConvSE(nn.Module):
    """An MBConv-style block: 1x1 expansion + ReLU6, depthwise 3x3 + ReLU6, SE with Linear layers on the flattened pool, a swish between
    them and `x * torch.sigmoid(...)`, linear 1x1 projection, identity shortcut.  48 gated channels: the code rows are padded to 64 and
    the map is the channel slice of the depthwise layer's padded output."""
    reader = "proj"

    def __init__(self):
        super().__init__()
        self.expand = nn.Conv2d(16, 48, 1)
        self.dw = nn.Conv2d(48, 48, 3, padding=1, groups=48)
        self.pool = nn.AdaptiveAvgPool2d(1)
        self.fc1, self.fc2 = nn.Linear(48, 12), nn.Linear(12, 48)
        self.proj = nn.Conv2d(48, 16, 1)
        self.head = nn.Conv2d(16, 64, 1)

    def forward(self, inp):
        x = F.relu6(self.dw(F.relu6(self.expand(inp))))
        out = self.pool(x)
        out = out.view(x.size(0), -1)
        out = self.fc1(out)
        out = self.fc2(out * torch.sigmoid(out))
        out = out.view(x.size(0), x.size(1), 1, 1)
        return self.head(inp + self.proj(x * torch.sigmoid(out)))


class GhostSE(nn.Module):
    """3x3 convolution + ReLU, SE with 1x1 convolutions on the (N, C, 1, 1) pool, a ReLU between them and the hard sigmoid
    `F.relu6(v + 3.) / 6.`, then a 1x1 convolution.  64 gated channels: unpadded code rows, shifted where the quantiser is unsigned."""
    reader = "b"

    def __init__(self):
        super().__init__()
        self.a = nn.Conv2d(16, 64, 3, padding=1)
        self.pool = nn.AdaptiveAvgPool2d(1)
        self.reduce, self.expand = nn.Conv2d(64, 16, 1), nn.Conv2d(16, 64, 1)
        self.b = nn.Conv2d(64, 32, 1)

    def forward(self, inp):
        x = torch.relu(self.a(inp))
        v = self.expand(torch.relu(self.reduce(self.pool(x))))
        x = x * (F.relu6(v + 3.) / 6.)
        return torch.relu(self.b(x))


class RepVGGSE(nn.Module):
    """A RepVGG-SE style block: 3x3 convolution, SE (1x1 convolutions, ReLU, sigmoid, view(-1, C, 1, 1)), the multiply, THEN the ReLU,
    then the next block's 3x3 convolution.  The gated map goes negative; the ReLU behind the multiply belongs to the gate node."""
    reader = "b"

    def __init__(self):
        super().__init__()
        self.c = 32
        self.a = nn.Conv2d(16, 32, 3, padding=1)
        self.pool = nn.AdaptiveAvgPool2d(1)
        self.down, self.up = nn.Conv2d(32, 8, 1), nn.Conv2d(8, 32, 1)
        self.b = nn.Conv2d(32, 32, 3, padding=1)

    def forward(self, inp):
        x = self.a(inp)
        g = torch.sigmoid(self.up(F.relu(self.down(self.pool(x))))).view(-1, self.c, 1, 1)
        return self.b(torch.relu(x * g))
