"""Inputs and expected values for the exact and tight tests of the attention kernel (csrc/attention.hip; its header pins the arithmetic
step by step), built on the CPU only: ONE table for tests/test_attention_cases_host.py (every construction's preconditions, proven
without a GPU) and tests/test_gpu_attention_exact.py (the same tensors launched and compared).  TEST INFRASTRUCTURE ONLY.

1. ties      (`tie_case`)  Keys as in test_gpu_attention.py (a): key j is the +-1 code of j's 9 bits at dimensions (7 bit + 3) % D.
             q_i = 512 code(pi(i)) with the dimensions of the bits in Z_i zeroed: the keys j < Tk that agree with pi(i) outside Z_i all
             have the score fl32(512 (9 - |Z_i|) scale) - the products are integers, the chain is exact - and every other key lies
             512 scale 2 = 128 (D = 64) or 181 (D = 32) lower: p = expf(0) = 1 for the ties, 0 for the rest, l = their count, o = the
             integer sum of their v rows, out = fl32(sum / count) - one IEEE division of two fp32 integers, which is what `want` is.
             Z_i rotates with i + h + b over ZSETS: bit 0 (neighbours in one lane half), bit 2 (the two lane halves), bits 5 and 6 (other
             key blocks: al = expf(0) = 1), {2, 5}, {0, 2, 6}.  pi is test (a)'s affine map, so the ties fall on every key block and lane
             half; every second round of the two large sets goes to a `pi` whose ties lie partly past Tk (`edge_pis`) where Tk has one:
             counts 5 (Tk = 65), 6 and 7 (77, 197) and, at the one shape added for it (Tk = 37), 3.
             What separates a true division from a multiply by fl32(1 / c): only c = 3, 5, 6, 7 can (1, 2, 4, 8 are exact either way),
             and of ZSETS only the two large sets reach those, only at Tk in {37, 65, 77, 197}: at most 19 % of the family's elements could
             separate whatever pi and v are, so "a quarter of the checked elements" is read over the elements whose count is no power
             of two (20 - 54 % of integer sums separate at such c); `separating` gives the mask, the host test the
             figures.
2. uniform   (`uniform_case`)  q = 0 (or scale = 0 with random q): every score is +-0, p = 1, l = Tk, o_c the integer column sum S_c,
             every row fl32(S_c / Tk).  B = 1, H = 5: head h rotates the waves by h & 3, so the partial last tile meets all four
             rotations and the wrap.
3. probe     (`probe_case`)  scores 0 and x on the grid x = -k / 8, k = 1 .. 512 (two heads of 256 rows), scale a power of two so
             that fl32(q scale) = x exactly.  "block0": keys 0 (score 0, v = 0) and 1 (score x, v = 1): out = e / (1 + e).  "blocks":
             key 0 (score x, v = 1) in block 0, the maximum 0 at keys 32 and 36 (the two lane halves, v = 0), the other keys 4096 x
             (512 or more below the running maximum: p = 0; their v = 3 would show): x goes through al, out = e / (2 + e).
             `probe_model` is the kernel's fp32 order with expf replaced by a function of choice.
4. -inf      (`inf_prefix_case`)  k[..., 0:40, 0] = -inf (block 0 and a part of block 1) or every key; rows with q[..., 0] > 0 score
             -inf there, rows with q[..., 0] <= 0 are NaN (+inf, or 0 inf).  One q[..., 0] is set to 0.
5. stores    (`store_case`, `padded`)  n01 inputs and the geometry of an output view inside a larger parent."""
import functools

import numpy as np
import torch

from test_gpu_attention import SHAPES, U, f32

DIMS = (32, 64)
NBITS = 9
ZSETS = ((0,), (2,), (5,), (6,), (2, 5), (0, 2, 6))
BASE_TIE_SHAPES = [s[:4] for s in SHAPES] + [(1, 5, 129, 257), (1, 4, 97, 40)]      # (B, H, Tq, Tk)
TIE_SHAPES = BASE_TIE_SHAPES + [(1, 2, 40, 37)]      # no Z of ZSETS leaves 3 ties at Tk in {17, 40, 65, 77, 197, 257}; at Tk = 37 two do
GAP = 104.0                                                                      # expf(x) = 0 in fp32 for x < -104
UNIFORM_TQ = (1, 31, 32, 33, 95, 96, 97, 127, 128, 129, 160, 161, 256, 257)
UNIFORM_TK = (1, 2, 31, 32, 33, 64, 65)
UNIFORM_BH = (1, 5)
PROBE_VARIANTS = ("block0", "blocks")
PROBE_TOL = 4 * U
INF_SHAPES = [SHAPES[0][:4], SHAPES[3][:4]]                                      # Tk = 197 and Tq != Tk = 77: both beyond key 40
INF_PREFIX = 40
STORE_TQ = (33, 129)
STORE_BHTK = (2, 3, 50)


def code(d):
    """[512, d]: row j is the +-1 code of j's 9 bits (test (a)'s keys)."""
    j = torch.arange(1 << NBITS)
    c = torch.zeros(1 << NBITS, d)
    for bit in range(NBITS):
        c[:, (7 * bit + 3) % d] = ((j >> bit) & 1).float() * 2 - 1
    return c


def zmask(z):
    return sum(1 << bit for bit in z)


def tied(pi, zm, tk):
    """[..., Tk] bool: key j < Tk agrees with pi outside the bits of zm."""
    j = torch.arange(tk)
    return ((j ^ pi[..., None]) & ~zm[..., None] & ((1 << NBITS) - 1)) == 0


def edge_pis(tk, z):
    """The pi < Tk whose ties under Z = z are cut by Tk to a count that is no power of two."""
    p = torch.arange(tk)
    n = tied(p, torch.full_like(p, zmask(z)), tk).sum(-1)
    return [int(x) for x in p[(n & (n - 1)) != 0]]


@functools.lru_cache(maxsize=None)
def tie_case(shape, d):
    """dict(q, k, v, scale, want [B, H, Tq, D], count [B, H, Tq], zi [B, H, Tq] (index into ZSETS), pi, mask [B, H, Tq, Tk])."""
    b, h, tq, tk = shape
    scale = f32(d ** -0.5)
    i, hh, bb = torch.arange(tq)[None, None, :], torch.arange(h)[None, :, None], torch.arange(b)[:, None, None]
    pi = ((7 * i + 3 + 5 * hh + 11 * bb) % tk).expand(b, h, tq).clone()
    zi = ((i + hh + bb) % len(ZSETS)).expand(b, h, tq)
    for n, z in enumerate(ZSETS):
        edge = edge_pis(tk, z)
        if len(z) > 1 and edge:
            e = torch.tensor(edge)[((i // 12 + hh + bb) % len(edge)).expand(b, h, tq)]
            pi = torch.where((zi == n) & ((i // len(ZSETS)) % 2 == 0), e, pi)
    zm = torch.tensor([zmask(z) for z in ZSETS])[zi]
    cd = code(d)
    keep = torch.ones(len(ZSETS), d)
    for n, z in enumerate(ZSETS):
        for bit in z:
            keep[n, (7 * bit + 3) % d] = 0.0
    q = 512.0 * cd[pi] * keep[zi]
    k = cd[:tk].expand(b, h, tk, d).contiguous()
    g = torch.Generator().manual_seed(1000 * d + sum(shape))
    v = (torch.randperm((1 << 21) - 1, generator=g)[:b * h * tk * d] + 1).float().reshape(b, h, tk, d)      # 8 of them: below 2^24
    mask = tied(pi, zm, tk)
    count = mask.sum(-1)
    total = (mask.double() @ v.double()).float()
    return dict(q=q, k=k, v=v, scale=scale, want=total / count[..., None].float(), total=total, count=count, zi=zi, pi=pi, mask=mask)


def separating(total, count):
    """Where a multiply by fl32(1 / count) gives another fp32 number than the division (both IEEE, on the CPU)."""
    c = count[..., None].float().expand_as(total)
    return total * (1.0 / c) != total / c


@functools.lru_cache(maxsize=None)
def uniform_case(tq, tk, d, zero_scale):
    """dict(q, k, v, scale, want [H, D]): q = 0 and scale = D^-0.5, or random nonzero q and scale = 0."""
    b, h = UNIFORM_BH
    g = torch.Generator().manual_seed(100000 * d + 300 * tq + tk)
    k = torch.randn(b, h, tk, d, generator=g)
    q = torch.randn(b, h, tq, d, generator=g) if zero_scale else torch.zeros(b, h, tq, d)
    v = (torch.randperm((1 << 17) - 1, generator=g)[:b * h * tk * d] + 1).float().reshape(b, h, tk, d)       # 65 of them: below 2^24
    s = v.double().sum(2).float()
    return dict(q=q, k=k, v=v, scale=0.0 if zero_scale else f32(d ** -0.5), total=s, want=(s / float(tk))[0])


def probe_grid():
    return -(torch.arange(512, dtype=torch.float64) + 1) / 8


@functools.lru_cache(maxsize=None)
def probe_case(d, variant):
    """dict(q, k, v, scale, x [1, 2, 256] float64, ref [1, 2, 256] float64): every channel of row i is e / (1 + e) or e / (2 + e)."""
    scale = {64: 0.125, 32: 0.25}[d]
    x = probe_grid().reshape(1, 2, 256)
    q = torch.zeros(1, 2, 256, d)
    q[..., 0] = (x / scale).float()
    tk = {"block0": 2, "blocks": 37}[variant]
    k, v = torch.zeros(1, 2, tk, d), torch.zeros(1, 2, tk, d)
    e = torch.exp(x)
    if variant == "block0":
        k[:, :, 1, 0], v[:, :, 1] = 1.0, 1.0
        ref = e / (1 + e)
    else:
        k[:, :, :, 0], v[:, :, :] = 4096.0, 3.0
        k[:, :, 0, 0], v[:, :, 0] = 1.0, 1.0
        for key in (32, 36):
            k[:, :, key, 0], v[:, :, key] = 0.0, 0.0
        ref = e / (2 + e)
    return dict(q=q, k=k, v=v, scale=scale, x=x, ref=ref)


def probe_model(x, variant, exp32):
    """The kernel's order for the probe in numpy float32, `exp32` (float32 array -> float32 array) standing for expf: float32 [512]."""
    one = np.float32(1)
    e = exp32(np.asarray(x, dtype=np.float32))
    assert e.dtype == np.float32
    if variant == "block0":      # m = 0; half 0: t = 1 + e; half 1: 0;  o = e
        return e / ((one + e) + np.float32(0))
    # block 0: m = x, p = 1, l_0 = 1, o = 1;  block 1: al = e, l_0 = fl(fl(1 e) + 1), l_1 = fl(0 e + 1), o = fl(1 e) + 0
    return (one * e) / (((one * e) + one) + one)


def exp_rounded(x):
    """The correctly rounded float32 exponential (float64's, rounded once more: off the grid's values by far less than a float64 ulp
    from a float32 midpoint, which test_probe_model asserts)."""
    return np.exp(x.astype(np.float64)).astype(np.float32)


def exp2_prescaled(x):
    """v_exp_f32 on a pre-scaled argument: 2^fl32(x fl32(log2 e)), the power of two itself exact."""
    t = x * np.float32(1.4426950408889634)
    return np.exp2(t.astype(np.float64)).astype(np.float32)


def n01(b, h, tq, tk, d, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(b, h, tq, d, generator=g), torch.randn(b, h, tk, d, generator=g), torch.randn(b, h, tk, d, generator=g)


@functools.lru_cache(maxsize=None)
def inf_prefix_case(shape, d, every_key):
    """dict(q, k, v, scale, nan [B, H, Tq] bool (rows that are NaN), first (the first key that is not -inf, or Tk))."""
    b, h, tq, tk = shape
    q, k, v = n01(b, h, tq, tk, d, 7 * d + sum(shape) + every_key)
    q[0, 0, 1, 0] = 0.0
    first = tk if every_key else INF_PREFIX
    k[:, :, :first, 0] = float("-inf")
    return dict(q=q, k=k, v=v, scale=f32(d ** -0.5), nan=torch.ones(b, h, tq, dtype=torch.bool) if every_key else q[..., 0] <= 0, first=first)


@functools.lru_cache(maxsize=None)
def negative_scale_case(shape, d):
    b, h, tq, tk = shape
    q, k, v = n01(b, h, tq, tk, d, 11 * d + sum(shape))
    return dict(q=q, k=k, v=v, scale=-f32(d ** -0.5))


@functools.lru_cache(maxsize=None)
def store_case(tq, d):
    b, h, tk = STORE_BHTK
    q, k, v = n01(b, h, tq, tk, d, 13 * d + tq)
    return dict(q=q, k=k, v=v, scale=f32(d ** -0.5))


def padded(b, h, tq, d):
    """The merged output [B, Tq, H D] as a view of a parent [B, Tq + 2, H D + 8] from row 1 and column 4 on: (parent shape, element offset
    of the view, (batch, head, token) strides in elements)."""
    row = h * d + 8
    return (b, tq + 2, row), row + 4, ((tq + 2) * row, d, row)
