"""Inputs and expected values for the exact and tight tests of the two window attention kernels (csrc/window_attention.hip and
csrc/window_attention_f16.hip; their headers pin the arithmetic step by step), built on the CPU only: ONE table for
tests/test_window_attention_cases_host.py (every construction's preconditions, proven without a GPU) and
tests/test_gpu_window_attention_exact.py (the same tensors launched on both kernels and compared).  TEST INFRASTRUCTURE ONLY.

Every q, k and v of a bitwise family is exactly representable in f16 (small integers, +-512, 4096, 8192; v: `f16_integers`), so both
kernels see the same operands; every sum that enters a result is a sum of integers below 2^24, exact in every order.  Key layout of both
kernels: accumulator register r of a lane half = key (r & 3) + 8 (r >> 2) + 4 half of a 32-key block - key bits 0, 1: the register
within its quad, bit 2: the lane half, bits 3, 4: the quad, bit 5: the block.

1. ties      (`tie_case`)  1 .. 8 keys share the exact maximal score, every other key lies 128 or more below (p = 0, P = 0): out =
             fl32(integer sum of the tied v rows / count), one IEEE division.  The tied keys of row i are those that agree with pi(i)
             outside the key bits of Z_i; Z rotates over ZSETS, pi is affine in i and in the index the way depends on, and every second
             round of the sets of two or three bits goes to a pi whose group is cut by T to 3, 5, 6 or 7 keys (`edge_pis`).  Four ways:
             "qk" (+-1 codes of the key index, q = 512 code(pi) with the dimensions of Z zeroed), "bias" (q = 0, per head), "mask"
             (q = 0, nW = 3, B = 6), "split" (bias = R + c, mask = -R + the tie table: R differs per key, so neither term alone ties).
2. order     (`order_case`)  two live keys per row: key A's score goes through the construction, key B's is the pinned result placed
             in the term with k_B = 0; the rest lies 200 below.  `order_models` evaluates the pinned and the alternative orders.
             The FMA construction first proposed (q.k = 2^24 + 2 m, scale 1 - 2^-24, bias -2^24) separates by 1 - 2 m 2^-24, just
             UNDER 1; it is replaced by q.k = 2^25 + 4 m (4096 * 8192 + m * 4, m <= 2048: exact products of f16 operands), scale
             1 - 2^-24, term -2^25: a scale = 2^25 + 4 m - 2 - 4 m 2^-24 lies just below the midpoint of an ulp of 4 and is rounded
             to 2^25 + 4 m - 4, pinned 4 m - 4; the fused multiply-add gives 4 m - 2 - 4 m 2^-24: apart by 2 - 4 m 2^-24 >= 1.9995.
3. uniform / placement at every T in 1 .. 64 (`uniform_case`, `placement_case`), terms in TERMS.
4. probe     (`probe_case`)  scores 0 and x = -k / 8, k = 1 .. 512, v = 0 and 1: out = e / (1 + e); `probe_tol_f16` is derived below.
5. non-finite (`plant_case`)  one NaN / +inf / 1e5 planted, and the expected mask.
6. stores, 7. independence, 8. bound additions: n01 inputs (`n01_case`) and the views (`term_parent`, `term_view`)."""
import functools

import numpy as np
import torch

from attention_exact_cases import edge_pis, exp2_prescaled, exp_rounded, padded, probe_grid, probe_model, separating, tied, zmask  # noqa: F401
from test_gpu_attention import U, f32

DIMS = (32, 64)
OPERANDS = ("f32", "f16")
TERMS = ("none", "bias", "mask", "bias+mask")
GAP = 104.0                                                                      # expf(x) = 0 in fp32 for x < -104
E16 = 2.0 ** -11

ZSETS = ((0,), (2,), (3,), (4,), (5,), (2, 5), (0, 2, 5), (1, 3, 4))
TIE_T = (1, 8, 33, 37, 49, 63, 64)
TIE_WAYS = ("qk", "bias", "mask", "split")
TIE_BHW = {"qk": (2, 3, 1), "bias": (2, 5, 1), "mask": (6, 2, 3), "split": (4, 3, 2)}      # (B, H, nW)

ORDER_T = (37, 64)
ORDER_KINDS = ("bias_before_mask", "no_presummed_terms", "no_fma_bias", "no_fma_mask")
ORDER_TARGET = {"bias_before_mask": "mask_first", "no_presummed_terms": "terms_first", "no_fma_bias": "fma", "no_fma_mask": "fma"}
ORDER_PAIRS = ((1, 0), (3, 7), (10, 18), (5, 36), (35, 32), (33, 2), (20, 34), (30, 26))      # (key A, key B) per head / window, all 16 distinct
ORDER_C0, ORDER_C1 = 3, 20

ALL_T = tuple(range(1, 65))
UNIFORM_BH = (1, 5)
PLACE_BHW = (4, 2, 2)

PROBE_BHT = (2, 4, 64)
PROBE_VARIANTS = ("terms", "qk")
PROBE_PLACES = {"half": 4, "block": 32}      # the second key: the other lane half of block 0 / block 1 (the first is key 0)
PROBE_TOL = 4 * U

PLANT_SHAPE = (2, 3, 49, 2)                  # (B, H, T, nW)
PLANT_KINDS = ("nan_q", "nan_k", "nan_v", "inf_bias")
PLANT_KINDS_F16 = ("big_k", "big_v")
STORE_T = (1, 33, 49)
STORE_BH = (1, 5)
INDEP_BHT = (3, 3, 49)
BOUND_SHAPES = ((2, 3, 33, 2), (2, 3, 49, 2))      # (B, H, T, nW)


def roundup4(t):
    return (t + 3) // 4 * 4


@functools.lru_cache(maxsize=None)
def f16_integers():
    """The 5120 integers of 1 .. 16384 that f16 holds exactly (all to 2048, the even ones to 4096, ...)."""
    x = torch.arange(1, 16385).float()
    return x[x.half().float() == x]


def perm_v(b, h, t, d, g):
    """[B, H, T, D]: per (b, h) its own seeded permutation of f16_integers - distinct within a head, 64 of them below 2^24."""
    ints = f16_integers()
    return torch.stack([ints[torch.randperm(len(ints), generator=g)[:t * d]].reshape(t, d) for _ in range(b * h)]).reshape(b, h, t, d)


def small_ints(shape, g):
    """Integers in -3 .. 3: a k that q = 0 (or a q that is 0 on its channels) makes irrelevant, exact in f16."""
    return torch.randint(-3, 4, shape, generator=g).float()


def code6(d):
    """[64, d]: row j is the +-1 code of j's 6 bits at the dimensions (7 bit + 3) % d (distinct for d = 32 and 64)."""
    j = torch.arange(64)
    c = torch.zeros(64, d)
    for bit in range(6):
        c[:, (7 * bit + 3) % d] = ((j >> bit) & 1).float() * 2 - 1
    return c


def score_steps(q, k, scale, bias, mask):
    """The headers' score steps in numpy float32, each rounded by itself: fl32(fl32(fl32(a scale) + bias) + mask), a = q . k as float64
    (the callers assert that it is an fp32 integer: the chain is exact).  bias [H or 1, T, T], mask [nW, T, T] or None.  Returns
    (float32 [B, H, T, T], a float64)."""
    a = (q.double() @ k.double().transpose(-1, -2)).numpy()
    s = a.astype(np.float32) * np.float32(scale)
    if bias is not None:
        s = s + bias.numpy()[None]
    if mask is not None:
        s = s + mask.repeat(q.shape[0] // mask.shape[0], 1, 1).numpy()[:, None]
    assert s.dtype == np.float32
    return s, a


def scores64(q, k, scale, bias, mask):
    s = scale * (q.double() @ k.double().transpose(-1, -2))
    if bias is not None:
        s = s + bias.double()[None]
    if mask is not None:
        s = s + mask.double().repeat(q.shape[0] // mask.shape[0], 1, 1)[:, None]
    return s


# ------------------------------------------------------------------------------------------- 1. ties
def tie_layout(rows, t):
    """(pi [R, T], zi [R, T] (index into ZSETS), tied [R, T, T] bool) for R independent tables (heads, windows or (b, h) pairs)."""
    i, r = torch.arange(t)[None, :], torch.arange(rows)[:, None]
    pi = ((7 * i + 3 + 5 * r) % t).expand(rows, t).clone()
    zi = ((i + r) % len(ZSETS)).expand(rows, t)
    for n, z in enumerate(ZSETS):
        edge = edge_pis(t, z)
        if len(z) > 1 and edge:
            e = torch.tensor(edge)[((i // len(ZSETS)) * 3 + i + r) % len(edge)].expand(rows, t)
            pi = torch.where((zi == n) & ((i // len(ZSETS)) % 2 == 0), e, pi)
    zm = torch.tensor([zmask(z) for z in ZSETS])[zi]
    return pi, zi, tied(pi, zm, t)


def _noise(r, t, a, b):
    i, j, rr = torch.arange(t)[None, :, None], torch.arange(t)[None, None, :], torch.arange(r)[:, None, None]
    return ((a * i + b * j + rr) % 50).float()


@functools.lru_cache(maxsize=None)
def tie_case(way, t, d):
    """dict(q, k, v, scale, bias, mask, want, total [B, H, T, D], count, zi [B, H, T], tied [B, H, T, T])."""
    b, h, nw = TIE_BHW[way]
    g = torch.Generator().manual_seed(1000 * d + 10 * t + TIE_WAYS.index(way))
    scale = f32(d ** -0.5)
    v = perm_v(b, h, t, d, g)
    bias = mask = None
    if way == "qk":
        pi, zi, tm = (x.reshape(b, h, *x.shape[1:]) for x in tie_layout(b * h, t))
        cd, keep = code6(d), torch.ones(len(ZSETS), d)
        for n, z in enumerate(ZSETS):
            for bit in z:
                keep[n, (7 * bit + 3) % d] = 0.0
        q, k = 512.0 * cd[pi] * keep[zi], cd[:t].expand(b, h, t, d).contiguous()
    else:
        q, k = torch.zeros(b, h, t, d), small_ints((b, h, t, d), g)
        rows = h if way == "bias" else nw
        pi, zi, tm = tie_layout(rows, t)
        top = (((torch.arange(t)[None, :] + 2 * torch.arange(rows)[:, None]) % 9 - 4) * 0.5)[..., None]      # the tied score of a row
        table = torch.where(tm, top, top - 128.0 - _noise(rows, t, 3, 5))
        if way == "bias":
            bias = table
            zi, tm = zi[None].expand(b, h, t), tm[None].expand(b, h, t, t)
        else:
            if way == "mask":
                mask = table
            else:
                r_ij = ((5 * torch.arange(t)[None, :] + 3 * torch.arange(t)[:, None]) % 64).float() * 0.25      # distinct over a row's keys
                c_hi = ((torch.arange(t)[None, :] + 2 * torch.arange(h)[:, None]) % 9 - 4).float() * 0.5
                bias = r_ij[None] + c_hi[..., None]
                mask = torch.where(tm, torch.zeros(()), -128.0 - _noise(rows, t, 3, 5)) - r_ij[None]
            zi, tm = zi.repeat(b // nw, 1)[:, None].expand(b, h, t), tm.repeat(b // nw, 1, 1)[:, None].expand(b, h, t, t)
    count = tm.sum(-1)
    total = (tm.double() @ v.double()).float()
    return dict(q=q, k=k, v=v, scale=scale, bias=bias, mask=mask, want=total / count[..., None].float(), total=total, count=count, zi=zi, tied=tm)


# ------------------------------------------------------------------------------------------- 2. order of the score steps
def order_models(a, scale, bias, mask):
    """The score of one key under the pinned order and the alternatives, numpy float32 arrays in, dict of float32 arrays out.  `bias`
    or `mask` None: the term is absent.  "fma": the multiply by the scale fused with the FIRST term's add (one rounding: float64 holds
    the product of an integer below 2^26 and a 24-bit scale, and its sum with the term, exactly)."""
    a, sc = np.asarray(a, np.float32), np.float32(scale)
    s = a * sc
    first = bias if bias is not None else mask
    fused = (a.astype(np.float64) * np.float64(sc) + first.astype(np.float64))
    assert np.all(np.abs(a) < 2 ** 26) and np.all(fused == (a.astype(np.longdouble) * np.longdouble(sc) + first.astype(np.longdouble)))
    fused = fused.astype(np.float32)
    if bias is None or mask is None:
        return dict(pinned=s + first, fma=fused)
    return dict(pinned=(s + bias) + mask, mask_first=(s + mask) + bias, terms_first=s + (bias + mask), fma=fused + mask)


@functools.lru_cache(maxsize=None)
def order_case(kind, t, d):
    """dict(q, k, v, scale, bias, mask, want [B, H, T, D], a_key, b_key [B, H] (the live keys), parts = (a, biasA, maskA) float32
    [B, H, T] of key A for order_models, pinned [B, H, T])."""
    n = len(ORDER_PAIRS)
    by_mask = kind == "no_fma_mask"
    b, h = (n, 1) if by_mask else (1, n)
    g = torch.Generator().manual_seed(77 * d + t + ORDER_KINDS.index(kind))
    i = torch.arange(t)
    rr = torch.arange(n)
    m = (1 + (37 * i[None, :] + 211 * rr[:, None]) % 2048).float()                      # [n, T] in 1 .. 2048
    if kind == "bias_before_mask":
        scale, q0, k0, q1, k1 = 0.125, 2.0, 4.0, 0.0, 0.0
        bias_a, mask_a, pinned = torch.full((n, t), 2.0 ** 24), torch.ones(n, t), torch.full((n, t), 2.0 ** 24)
    elif kind == "no_presummed_terms":
        scale, q0, k0, q1, k1 = 0.125, 2.0, 12.0, 0.0, 0.0
        bias_a, mask_a, pinned = torch.full((n, t), 2.0 ** 25), torch.full((n, t), -2.0 ** 25), torch.full((n, t), 4.0)
    else:
        scale, q0, k0, q1, k1 = f32(1 - 2.0 ** -24), 4096.0, 8192.0, None, 4.0
        bias_a, mask_a, pinned = torch.full((n, t), -2.0 ** 25), torch.zeros(n, t), 4 * m - 4
        if by_mask:
            bias_a, mask_a = None, bias_a
    keys = torch.tensor(ORDER_PAIRS)
    ka, kb = keys[:, 0], keys[:, 1]
    q = torch.zeros(n, t, d)
    q[..., ORDER_C0] = q0
    q[..., ORDER_C1] = m if q1 is None else q1
    k = small_ints((n, t, d), g)
    k[..., ORDER_C0] = k[..., ORDER_C1] = 0.0
    k[rr, kb] = 0.0
    k[rr, ka] = 0.0
    k[rr, ka, ORDER_C0], k[rr, ka, ORDER_C1] = k0, k1
    low = pinned[..., None] - 201.0 - _noise(n, t, 3, 5)                                # [n, T, T]
    term = low.clone()                                                                   # the term that carries the placed values
    term[rr, :, kb] = pinned
    term[rr, :, ka] = mask_a if by_mask else bias_a
    if by_mask:
        bias, mask = None, term
    else:
        bias, mask = term, torch.zeros(1, t, t)
        mask[0, :, ka] = mask_a[0][:, None]                                              # (one value per kind: every head's key A, in every row)
    parts = (bias_a, mask_a)
    v = perm_v(b, h, t, d, g)
    shape = lambda x: x.reshape(b, h, *x.shape[1:])  # noqa: E731
    q, k = shape(q), shape(k)
    va = torch.gather(v, 2, shape(ka)[..., None, None].expand(b, h, 1, d))
    vb = torch.gather(v, 2, shape(kb)[..., None, None].expand(b, h, 1, d))
    a_val = torch.full((n, t), q0 * k0) + (m * k1 if q1 is None else 0.0)
    return dict(q=q, k=k, v=v, scale=scale, bias=bias, mask=mask, want=((va + vb) / 2).expand(b, h, t, d).contiguous(),
                a_key=shape(ka), b_key=shape(kb), parts=(shape(a_val), *(None if p is None else shape(p) for p in parts)), pinned=shape(pinned))


# ------------------------------------------------------------------------------------------- 3. uniform rows, placement
def _terms(terms, bias, mask):
    return (bias if "bias" in terms else None), (mask if "mask" in terms else None)


@functools.lru_cache(maxsize=None)
def uniform_case(t, d, terms):
    """dict(q, k, v, scale, bias [H, T, T] = 1.5, mask [1, T, T] = -2.25 (or None), want [H, D] = fl32(column sum / T))."""
    b, h = UNIFORM_BH
    g = torch.Generator().manual_seed(100000 * d + 300 * t + TERMS.index(terms))
    v = perm_v(b, h, t, d, g)
    total = v.double().sum(2).float()
    bias, mask = _terms(terms, torch.full((h, t, t), 1.5), torch.full((1, t, t), -2.25))
    return dict(q=torch.zeros(b, h, t, d), k=small_ints((b, h, t, d), g), v=v, scale=f32(d ** -0.5), bias=bias, mask=mask, total=total,
                want=(total / float(t))[0])


def _pick(rows, t):
    return (7 * torch.arange(t)[None, :] + 3 + 5 * torch.arange(rows)[:, None]) % t      # [rows, T]


@functools.lru_cache(maxsize=None)
def placement_case(t, d, terms):
    """dict(q, k, v, scale, bias, mask, sel [B, H, T] (the key that leads its row by 150 or more), want = the selected v row).  bias / mask:
    the table of test_gpu_window_attention.py (asymmetric in (i, j), another per head / window); bias+mask: the leader (300) sits in the
    bias on even rows and in the mask on odd rows, over the noise of both; none: +-1 key codes, q = 512 code(pick)."""
    b, h, nw = PLACE_BHW
    g = torch.Generator().manual_seed(200000 * d + 300 * t + TERMS.index(terms))
    v = perm_v(b, h, t, d, g)
    i, j = torch.arange(t)[None, :, None], torch.arange(t)[None, None, :]
    by_head, by_win = _pick(h, t), _pick(nw, t)
    sel_h, sel_w = by_head[None].expand(b, h, t), by_win.repeat(b // nw, 1)[:, None].expand(b, h, t)
    bias = mask = None
    scale = f32(d ** -0.5)
    q, k = torch.zeros(b, h, t, d), small_ints((b, h, t, d), g)
    if terms == "none":
        sel = _pick(b * h, t).reshape(b, h, t)
        cd, scale = code6(d), 0.25
        q, k = 512.0 * cd[sel], cd[:t].expand(b, h, t, d).contiguous()
    elif terms == "bias":
        bias, sel = torch.where(j == by_head[..., None], 200.0, _noise(h, t, 3, 5)), sel_h
    elif terms == "mask":
        mask, sel = torch.where(j == by_win[..., None], 200.0, _noise(nw, t, 3, 5)), sel_w
    else:
        even = (torch.arange(t) % 2 == 0)
        bias = _noise(h, t, 3, 5) + 300.0 * ((j == by_head[..., None]) & even[None, :, None])
        mask = _noise(nw, t, 5, 3) + 300.0 * ((j == by_win[..., None]) & ~even[None, :, None])
        sel = torch.where(even[None, None, :], sel_h, sel_w)
    return dict(q=q, k=k, v=v, scale=scale, bias=bias, mask=mask, sel=sel, want=torch.gather(v, 2, sel[..., None].expand(b, h, t, d)))


def term_parent(x, fill):
    """[R, T, T] -> the parent [R, T + 2, roundup4(T) + 8] filled with `fill` that holds x at [:, 1:T + 1, 4:4 + T]."""
    r, t, _ = x.shape
    parent = torch.full((r, t + 2, roundup4(t) + 8), fill, dtype=torch.float32)
    parent[:, 1:t + 1, 4:4 + t] = x
    return parent


def term_view(parent, t):
    return parent[:, 1:t + 1, 4:4 + t]


def row_parent(x, fill=float("nan")):
    """[B, H, T, D] -> the NaN-filled parent [B, H, T + 2, D] that holds x at [:, :, 1:T + 1]."""
    b, h, t, d = x.shape
    parent = torch.full((b, h, t + 2, d), fill, dtype=torch.float32)
    parent[:, :, 1:t + 1] = x
    return parent


# ------------------------------------------------------------------------------------------- 4. the probe
@functools.lru_cache(maxsize=None)
def probe_case(d, variant, place):
    """dict(q, k, v, scale, bias, mask, x, ref [B, H, T] float64).  Key 0: score 0, v = 0; key PROBE_PLACES[place]: score x, v = 1; every
    other key 1000 or more below.  x = -(1 + i + 64 h + 256 b) / 8.  "terms": q = 0, the bias [H, T, T] holds -(1 + i + 64 h) / 8 and the
    mask [2, T, T] the batch element's -32 (a bias cannot differ between batch elements; both are dyadic, their sum is exact).  "qk":
    q_i[0] = x / scale against k[0] = 1 of the second key, q_i[1] = -1000 / scale against k[1] = 1 of the dead keys; scale 2^-3 (D = 64) /
    2^-2 (D = 32): every product and the multiply are exact, and every operand is exact in f16."""
    b, h, t = PROBE_BHT
    second = PROBE_PLACES[place]
    x = probe_grid().reshape(b, h, t)
    dead = torch.ones(t, dtype=torch.bool)
    dead[[0, second]] = False
    v = torch.zeros(b, h, t, d)
    v[:, :, second] = 1.0
    v[:, :, dead] = 3.0                                                                   # (a dead key that were not dead would show)
    q, k, bias, mask = torch.zeros(b, h, t, d), torch.zeros(b, h, t, d), None, None
    if variant == "terms":
        scale = f32(d ** -0.5)
        k = small_ints((b, h, t, d), torch.Generator().manual_seed(d))
        bias = (-1000.0 - torch.arange(t).float())[None, None, :].repeat(h, t, 1)
        bias[:, :, 0] = 0.0
        bias[:, :, second] = x[0].float()
        mask = torch.zeros(b, t, t)
        mask[1, :, second] = -32.0
    else:
        scale = {64: 0.125, 32: 0.25}[d]
        q[..., 0], q[..., 1] = (x / scale).float(), -1000.0 / scale
        k[:, :, second, 0] = 1.0
        k[:, :, dead, 1] = 1.0
    e = torch.exp(x)
    return dict(q=q, k=k, v=v, scale=scale, bias=bias, mask=mask, x=x, ref=e / (1 + e), second=second)


# The f16 kernel's probe tolerance, from its header's per-step terms (u = 2^-24, E16 = 2^-11), e = exp(x) exact, x <= 0:
#   the scores are exact here (0 and x are fp32 numbers, m~ = 0, x - 0 is exact): the subtraction adds nothing;
#   t = fl32(x L), L = fl32(log2 e) within relative u of log2 e, the product rounded once: 2 u |x| on the natural-unit exponent;
#   p^ = v_exp_f32(t): 1 ulp, 2 u relative.                  Together |p^ - e| <= e r1,  r1 = expm1((2 |x| + 2) u);
#   P = h(p^): half an f16 ulp, at most E16 p^ for a normal result, 2^-25 in the subnormal range and where P = 0:
#                                                             dP = e r1 + max(E16 e (1 + r1), 2^-25) >= |P - e|;
#   numerator o = P * 1 exactly, l = fl32(1 + P) - the maximal key's weight is exactly 1, every dead key's exactly 0 - and one
#   division: out = P / (1 + P) (1 + th), |th| <= 2 u / (1 - u).  With f(y) = y / (1 + y): |f(P) - f(e)| = |P - e| / ((1 + P)(1 + e)),
#   and 1 + P >= 1 + max(e - dP, 0).  Hence
#       |out - f(e)| <= dP / ((1 + e)(1 + max(e - dP, 0))) + (f(e) + that) 2 u / (1 - u).
# Both weights of l are the ROUNDED ones: a kernel that summed the unrounded p^ would be off by dP / (1 + e) instead - up to (1 + e)
# times this tolerance (the host test shows grid points where that model exceeds it).
def probe_tol_f16(x):
    x = x.double()
    e = torch.exp(x)
    r1 = torch.expm1((2 * x.abs() + 2) * U)
    dp = e * r1 + torch.maximum(E16 * e * (1 + r1), torch.tensor(2.0 ** -25, dtype=torch.float64))
    first = dp / ((1 + e) * (1 + (e - dp).clamp_min(0)))
    return first + (e / (1 + e) + first) * 2 * U / (1 - U)


def probe_model_f16(x, exp2_32, rounded_l=True):
    """The f16 kernel's order for the probe in numpy: p^ = exp2_32(fl32(x L)), P = h(p^), out = fl32(P / fl32(1 + P)) - or, with
    rounded_l=False, the l of a kernel that sums the unrounded weights: fl32(P / fl32(1 + p^)).  float32 [512]."""
    t = np.asarray(x, np.float32) * np.float32(1.44269502162933349609375)
    p = exp2_32(t)
    assert p.dtype == np.float32
    ph = p.astype(np.float16).astype(np.float32)
    return ph / (np.float32(1) + (ph if rounded_l else p))


def exp2_rounded(t):
    return np.exp2(t.astype(np.float64)).astype(np.float32)


# ------------------------------------------------------------------------------------------- 5 .. 8. n01 inputs
@functools.lru_cache(maxsize=None)
def n01_case(b, h, t, d, nw, seed=0):
    """dict(q, k, v [B, H, T, D], bias [H, T, T] N(0, 1), mask [nW, T, T] of 0 / -100 with a 0 diagonal, scale)."""
    g = torch.Generator().manual_seed(13 * d + 1000 * t + 7 * b + h + 100003 * seed)
    q, k, v = (torch.randn(b, h, t, d, generator=g) for _ in range(3))
    mask = torch.where((torch.rand(nw, t, t, generator=g) < 0.4) & ~torch.eye(t, dtype=torch.bool), -100.0, 0.0)
    return dict(q=q, k=k, v=v, bias=torch.randn(h, t, t, generator=g), mask=mask, scale=f32(d ** -0.5))


def plant_positions(d):
    """(b, h, index, channel): both lane halves (index bit 2), both key blocks (index >= 32), a channel in each 32-channel block."""
    return ((0, 1, 5, 3), (1, 2, 38, d - 1), (1, 0, 32, 17), (0, 2, 12, d // 2 + 9))


@functools.lru_cache(maxsize=None)
def plant_case(kind, d, which):
    """dict(q, k, v, bias, mask, scale, hit [B, H, T, D] bool: the elements the headers promise to be NaN (nan_*, inf_bias) / not finite
    (big_*), and no other).  big_k: h(1e5) = +inf as an operand: s_ij = +inf where q_ic scale > 0 - that row is NaN - and -inf where it
    is negative: key j drops out of that row, which stays finite (torch's unfused graph on the rounded operands says the same)."""
    b, h, t, nw = PLANT_SHAPE
    c = {n: (x.clone() if torch.is_tensor(x) else x) for n, x in n01_case(b, h, t, d, nw).items()}
    bi, hi, at, ch = plant_positions(d)[which]
    hit = torch.zeros(b, h, t, d, dtype=torch.bool)
    if kind == "nan_q":
        c["q"][bi, hi, at, ch] = float("nan")
        hit[bi, hi, at] = True
    elif kind == "nan_k":
        c["k"][bi, hi, at, ch] = float("nan")
        hit[bi, hi] = True
    elif kind == "nan_v":
        c["v"][bi, hi, at, ch] = float("nan")
        hit[bi, hi, :, ch] = True
    elif kind == "inf_bias":
        c["bias"][hi, at, (at * 7 + 3) % t] = float("inf")
        hit[:, hi, at] = True
    elif kind == "big_k":
        c["k"][bi, hi, at, ch] = 1e5
        hit[bi, hi] = (c["q"][bi, hi, :, ch] * c["scale"] > 0)[:, None]
    elif kind == "big_v":
        c["v"][bi, hi, at, ch] = 1e5
        hit[bi, hi, :, ch] = True
    else:
        raise ValueError(kind)
    return dict(c, hit=hit, at=(bi, hi, at, ch))


def torch_graph(q, k, v, scale, bias, mask):
    """The unfused graph in float64 on the CPU."""
    return torch.softmax(scores64(q, k, scale, bias, mask), dim=-1) @ v.double()


@functools.lru_cache(maxsize=None)
def indep_tile(d):
    """One (q, k, v [T, D], bias tile, mask tile [T, T]) at T = 49, and other k, v for the eight neighbours of the second arm."""
    b, h, t = INDEP_BHT
    c = n01_case(1, 1, t, d, 1, seed=1)
    o = n01_case(b, h, t, d, 1, seed=2)
    return dict(q=c["q"][0, 0], k=c["k"][0, 0], v=c["v"][0, 0], bias=c["bias"], mask=c["mask"], scale=c["scale"], other_k=o["k"], other_v=o["v"])


@functools.lru_cache(maxsize=None)
def inf_tail_case(shape, d):
    """n01 with bias and mask; the mask's parent (term_parent, fill -inf) is -inf from the first key of the 16-byte piece that holds key
    T - 1 to the end of every row's stride: the whole last piece and the pieces after it.  dict(..., mask = the dense [nW, T, T])."""
    b, h, t, nw = shape
    c = dict(n01_case(b, h, t, d, nw, seed=3))
    mask = c["mask"].clone()
    mask[:, :, 4 * ((t - 1) // 4):] = float("-inf")
    return dict(c, mask=mask, first_inf=4 * ((t - 1) // 4))
