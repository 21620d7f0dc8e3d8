"""Toys for the attention pass of the int8 plan (a helper, not a test): one network per spelling of the attention core that the plan
takes, and one per spelling it leaves alone.  Inputs: tokens [N, 16, 64]; 2 heads of 32 unless said otherwise."""
import torch
import torch.nn.functional as F
from torch import nn


class Attn(nn.Module):
    """to_qkv -> `core(self, q, k, v)` on [B, H, T, D] views -> `tail(self, o, b, t)` -> to_out.  `split`: "vit" (reshape + permute of
    the packed projection, workloads.ViT's spelling) or "chunk" (chunk(3, -1), then one reshape + permute each: the reference's)."""

    def __init__(self, core, tail=None, split="vit", heads=2, dim_head=32, dim=64):
        super().__init__()
        self.heads, self.dim_head, self.scale = heads, dim_head, dim_head ** -0.5
        self.to_qkv = nn.Linear(dim, 3 * heads * dim_head, bias=False)
        self.to_out = nn.Linear(heads * dim_head, dim)
        self.attend, self.attend_rows = nn.Softmax(dim=-1), nn.Softmax(dim=-2)
        self.core, self.tail, self.split = core, tail or merge_reshape, split

    def forward(self, x):
        qkv = self.to_qkv(x)
        b, t = qkv.shape[0], qkv.shape[1]
        if self.split == "vit":
            qkv = qkv.reshape(b, t, 3, self.heads, self.dim_head).permute(2, 0, 3, 1, 4)
            q, k, v = qkv[0], qkv[1], qkv[2]
        else:
            c = qkv.chunk(3, dim=-1)
            q, k, v = (c[i].reshape(b, t, self.heads, self.dim_head).permute(0, 2, 1, 3) for i in range(3))
        return self.tail(self, self.core(self, q, k, v), b, t)


# ---- tails
def merge_reshape(self, o, b, t):
    return self.to_out(o.permute(0, 2, 1, 3).reshape(b, t, self.heads * self.dim_head))


def merge_transpose_flatten(self, o, b, t):
    return self.to_out(o.transpose(1, 2).flatten(2))


def no_merge(self, o, b, t):             # the heads are averaged, not merged: the node stands at the second product, fp32 only
    return self.to_out(torch.cat((o.mean(1), o.amax(1)), dim=-1))


# ---- cores the plan takes
def vit_spelling(self, q, k, v):
    return torch.matmul(torch.softmax(torch.matmul(q, k.transpose(-1, -2)) * self.scale, dim=-1), v)


def module_softmax(self, q, k, v):       # the reference's: nn.Softmax(dim=-1) as `attend`
    dots = torch.matmul(q, k.transpose(-1, -2)) * self.scale
    return torch.matmul(self.attend(dots), v)


def sdpa(self, q, k, v):
    return F.scaled_dot_product_attention(q, k, v)


def sdpa_scale(self, q, k, v):
    return F.scaled_dot_product_attention(q, k, v, dropout_p=0.0, is_causal=False, scale=0.25)


def scale_on_the_left(self, q, k, v):
    return (self.scale * (q @ k.transpose(-2, -1))).softmax(3) @ v


def functional_softmax(self, q, k, v):
    return torch.matmul(F.softmax(torch.matmul(q, k.transpose(2, 3)) * self.scale, -1), v)


TAKEN = {"vit_spelling": lambda: Attn(vit_spelling), "chunk_module_softmax": lambda: Attn(module_softmax, split="chunk"),
         "sdpa": lambda: Attn(sdpa), "sdpa_scale": lambda: Attn(sdpa_scale), "scale_on_the_left": lambda: Attn(scale_on_the_left),
         "functional_softmax_flatten": lambda: Attn(functional_softmax, merge_transpose_flatten)}


# ---- cores the plan leaves alone
def masked(self, q, k, v):
    s = torch.matmul(q, k.transpose(-1, -2)) * self.scale
    return torch.matmul(torch.softmax(s + torch.ones(16, 16).tril().log(), dim=-1), v)


def causal(self, q, k, v):
    return F.scaled_dot_product_attention(q, k, v, is_causal=True)


def softmax_over_queries(self, q, k, v):
    return torch.matmul(self.attend_rows(torch.matmul(q, k.transpose(-1, -2)) * self.scale), v)


def scores_read_twice(self, q, k, v):
    s = torch.matmul(q, k.transpose(-1, -2)) * self.scale
    return torch.matmul(torch.softmax(s, dim=-1), v) + s.mean(-1, keepdim=True)


LEFT_ALONE = {"masked": lambda: Attn(masked), "causal": lambda: Attn(causal), "softmax_over_queries": lambda: Attn(softmax_over_queries),
              "scores_read_twice": lambda: Attn(scores_read_twice), "dim_head_48": lambda: Attn(vit_spelling, heads=4, dim_head=48)}
