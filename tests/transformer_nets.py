"""Small networks for the LayerNorm / GELU passes of the int8 plan (a helper, not a test): the smallest transformer that has every
pattern, and toys that spell one pattern each.  Inputs of the toys: rows [N, 16, 64]."""
import torch
import torch.nn.functional as F
from torch import nn

import workloads as W


def small_vit():
    """32^2 images in 8^2 patches (17 tokens, an odd row count), dim 64, 2 heads of 32, MLP 128, depth 2, 10 classes."""
    return W.ViT(image_size=32, patch_size=8, num_classes=10, dim=64, depth=2, heads=2, mlp_dim=128, dim_head=32)


class FunctionalGelu(nn.Module):
    """A user module whose body is F.gelu: traced into."""

    def forward(self, x):
        return F.gelu(x)


class Rows(nn.Module):
    """norm -> fc1 -> act -> fc2 on rows, the pieces and the wiring given by the test: `body(self, x)`."""

    def __init__(self, body, width=64, norm=None, hidden=128):
        super().__init__()
        self.norm = nn.LayerNorm(width) if norm is None else norm
        self.fc1, self.fc2, self.fc3 = nn.Linear(width, hidden), nn.Linear(hidden, 64), nn.Linear(hidden, 64)
        self.act, self.tanh_act, self.user_act = nn.GELU(), nn.GELU(approximate="tanh"), FunctionalGelu()
        self.body = body

    def forward(self, x):
        return self.body(self, x)


def plain(self, x):                      # LayerNorm -> Linear -> GELU -> Linear
    return self.fc2(self.act(self.fc1(self.norm(x))))


def shared(self, x):                     # the normalised rows and the activated rows have a second, fp32 reader each
    n = self.norm(x)
    a = self.act(self.fc1(n))
    return self.fc2(a) + n + a.sum(-1, keepdim=True)


def functional_spellings(self, x):
    h = self.user_act(self.fc1(self.norm(x)))
    return self.fc2(h) + self.fc3(F.gelu(self.fc1(x), approximate="none"))


def tanh_gelu(self, x):
    return self.fc2(F.gelu(self.fc1(x), approximate="tanh"))


def tanh_gelu_module(self, x):
    return self.fc2(self.tanh_act(self.fc1(x)))


def functional_layer_norm(self, x):
    return self.fc1(F.layer_norm(x, (64,)))


def nobody_takes_codes(self, x):
    return torch.tanh(self.norm(x)) + torch.tanh(self.act(x))


def two_quantisers(self, x):             # (the test gives fc2 and fc3 different input scales)
    a = self.act(self.fc1(x))
    return self.fc2(a) + self.fc3(a)


def conv_reader():
    """GELU on a 4-D map read by a plan convolution of 24 input channels: channel-padded code rows, as behind a swish."""
    class Net(nn.Module):
        def __init__(self):
            super().__init__()
            self.a, self.b, self.act = nn.Conv2d(64, 24, 1), nn.Conv2d(24, 64, 3, padding=1), nn.GELU()

        def forward(self, x):
            return self.b(self.act(self.a(x)))
    return Net()
