"""The calls of the pooled head kernel - csrc/conv_gap_i8.hip: conv_gap_i8_kernel<1> (64-wide slices) and <2> (128-wide) - that its image loop,
its slice-width rule, its pixel rows and its quantisers need, with their float64 reference: ONE table for tests/test_gap_head_host.py (the
launch record, the exactness conditions and what keeps a case from proving nothing, on the CPU) and tests/test_gpu_gap_head_exact.py (the
same calls launched and compared byte for byte).  TEST INFRASTRUCTURE ONLY.

A launch is described by its record (dlmc._native.gap_launch_record: slice width, nslice, ngroups, dynamic LDS bytes - the launcher's own
function, for the CU count it uses): a workgroup owns one slice of output channels and the images group, group + ngroups, ...  Every case
names the facts it exists for (`width`, `loops`), and both files assert them from the record (`launch_facts`), never from a copy of the rule.
  image loop   `loops`: N = 2 ngroups + ngroups // 2 from the record of this device, so every workgroup owns two or three images - the
               accumulator reset, the staging buffer's reuse behind the trailing barrier, the n += ngroups addressing of the codes, the
               shortcut and both outputs, the weights' staying valid.  Both slice widths (K = 2048: 16 slices of 128; K = 64 * 31: an odd
               number of 64-wide slices).  Every image has bytes of its own; in loop128 image 1 + ngroups holds only the zero-point code: its
               convolution is 0 and its output the bias itself, so a stale accumulator or staging row shows byte for byte.
  slice width  (C, K) = (320, 256) is the last C that runs 128-wide, (384, 256) the first that does not, (64, 192) runs 64-wide because of K,
               (2048, 64) is the LDS maximum (the hipFuncSetAttribute path); LDS_ORDER is the small, large, small sequence of one process.
  pixel rows   H W in {1, 31, 32, 33, 49, 63, 64} (wave rb = 1 owns rows 32 .. 63: idle, one row, all but one, all), as 1 x 1, 31 x 1, 4 x 8,
               1 x 33, 7 x 7, 7 x 9, 64 x 1 and 8 x 8.
  operands     tests/exact_layers.py's full-range layers: codes over all 256 byte values, weight codes in +-127, per-channel dyadic weight
               scales that differ, a dyadic input scale != 1, biases that are multiples of the channel's unit (one call without a bias);
               uint8 codes with a zero point above and below 128 and int8 codes with a zero point != 0; with and without the fp32 shortcut;
               no activation, ReLU, ReLU6.  NZ = 8 zero-weight channels carry edge values (NaN, +-inf, +-1e30, -0, 254.5, 255.5) in the bias.
  quantisers   QUANT_KINDS: the plain unsigned byte quantiser and its DLMCQ_EMIT_SHIFT128 form, an unsigned one with a zero point, a signed
               one, QBase with g > 0 and a float offset.  The scale (a power of two) and the zero point are computed from the reference's own
               pooled values (`pick_quant`) so that the 10 % tails leave the code range; `quant_facts` then asserts that both clamp ends and
               more than 100 distinct codes occur.
  special      through the shortcut: the map of image 0 is -0 everywhere, one pixel of image 1 is NaN, one of image 2 +inf: exactly those
               two (n, k) outputs are not finite (`SPECIAL`).

The reference, in three steps (`reference`):
  1. the pre-pool fp32 map: float64 convolution of the dequantised operands + bias + shortcut, then the activation.  It IS the kernel's fp32
     value, bit for bit, under tests/exact_stages.py's conditions, asserted on the actual operands (pair_stages, assert_final_units,
     exact_f32): the integer sums, the (shift - zp) SUM qw term and their sum below 2^24; fma(sum, s_in s_w[k], bias[k]) a multiple of the
     unit below 2^24 units; the shortcut sum an fp32 number.
  2. the pool: the three lines of csrc/gap.hip's header in numpy float32 (tests/test_gpu_gap.py: `restate`) - a sequential sum in pixel order,
     then a true division by float(H W).  THIS STEP ROUNDS: it is a restatement of the definition, not an exact-value argument.
  3. the codes: the oracle's quantiser of the pooled reference, as bytes (exact_layers.quantise, or test_gpu_epilogue_exact.expect_codes)."""
import functools
import math
from dataclasses import dataclass
from typing import Optional

import numpy as np
import torch

import exact_layers as X
import exact_stages as S
from test_gpu_gap import restate

NZ = 8                      # zero-weight channels [0, NZ): the first eight of exact_layers.EDGE_VALUES in the bias (0 where a shortcut is added)
G1 = dict(stride=1, pad=0, dil=1)
SPECIAL = {"negzero_image": 0, "nan": (1, NZ + 3, 2), "inf": (2, NZ + 40, 5)}      # (image, channel, pixel) of the NaN and of the +inf


@dataclass(frozen=True)
class Case:
    cid: str
    c: int
    k: int
    h: int
    w: int
    n: Optional[int]          # None: from the launch record (loops)
    width: int                # the slice width the record must answer
    uns: bool                 # uint8 codes
    zp: int                   # the input zero point
    act: int                  # DLMCQ_ACT_*
    res: bool                 # an fp32 shortcut
    quant: str                # QUANT_KINDS
    bias: bool = True
    loops: bool = False       # every workgroup owns >= 2 images, and not all the same number
    zero_image: bool = False  # image 1 + ngroups holds only the zero-point code
    special: bool = False     # SPECIAL in the shortcut

    def n_for(self, record):
        """The batch: as written, or 2 ngroups + ngroups // 2 for the ngroups the launcher uses on this device (`record`: N.gap_launch_record)."""
        if self.n is not None:
            return self.n
        ngroups = record(1 << 30, self.c, self.k)[2]
        assert ngroups >= 2, (self.cid, ngroups)
        return 2 * ngroups + ngroups // 2


QUANT_KINDS = ("plain", "shift", "uzp", "signed", "qbase_g")

CASES = [
    # ---- the image loop
    Case("loop128", 64, 2048, 3, 3, None, 128, True, 77, 0, False, "uzp", loops=True, zero_image=True),
    Case("loop64", 64, 64 * 31, 7, 7, None, 64, False, -37, 1, True, "plain", loops=True),
    # ---- the slice-width rule and the LDS sizes
    Case("edge320", 320, 256, 7, 7, 3, 128, True, 200, 2, False, "shift"),
    Case("edge384", 384, 256, 7, 7, 3, 64, False, 5, 1, True, "signed"),
    Case("k192", 64, 192, 8, 8, 4, 64, True, 131, 0, False, "qbase_g", bias=False),
    Case("lds64", 64, 64, 7, 7, 10, 64, True, 77, 1, False, "plain"),
    Case("lds2048", 2048, 64, 7, 7, 10, 64, True, 200, 1, True, "uzp"),
    # ---- pixel rows
    Case("hw1", 64, 128, 1, 1, 48, 128, True, 77, 1, False, "plain"),       # (48 images: 3072 code bytes, so that every byte value occurs)
    Case("hw31", 64, 64, 31, 1, 10, 64, False, -37, 0, True, "shift"),
    Case("hw32", 128, 128, 4, 8, 6, 128, True, 200, 2, True, "shift"),
    Case("hw33", 64, 64, 1, 33, 10, 64, True, 131, 0, False, "signed"),
    Case("hw63", 64, 128, 7, 9, 6, 128, False, 5, 2, False, "qbase_g"),
    Case("hw64", 64, 64, 64, 1, 10, 64, True, 77, 1, True, "uzp"),
    # ---- special values through the shortcut
    Case("special", 64, 128, 3, 3, 6, 128, True, 200, 1, True, "plain", special=True),
]
BY_ID = {c.cid: c for c in CASES}
LDS_ORDER = ("lds64", "lds2048", "lds64")          # one process: the dynamic-LDS attribute small, raised, small again
assert len(BY_ID) == len(CASES) and {c.quant for c in CASES} == set(QUANT_KINDS)
assert {c.h * c.w for c in CASES} >= {1, 31, 32, 33, 49, 63, 64} and {(c.h, c.w) for c in CASES} >= {(1, 33), (64, 1), (7, 9), (8, 8)}
assert {(c.uns, c.zp > 128) for c in CASES if c.uns} == {(True, True), (True, False)} and any(not c.uns and c.zp for c in CASES)
assert {(c.act, c.res) for c in CASES} == {(a, r) for a in (0, 1, 2) for r in (False, True)} and sum(not c.bias for c in CASES) == 1


# ---- the launcher's rule, restated (csrc/conv_gap_i8.hip: gap_lds_bytes, gap_launch_record) - the host file compares the record with it
def lds_bytes(c, bn):
    return bn * (c + 16) + 3 * bn * 4 + 64 * (bn + 4) * 4


def launch_restated(n, c, k, cus):
    nt = 2 if k % 128 == 0 and lds_bytes(c, 128) <= 78 * 1024 else 1
    nslice = k // (64 * nt)
    return 64 * nt, nslice, max(1, min(-(-2 * cus // nslice), n)), lds_bytes(c, 64 * nt)


def launch_facts(case, n, record):
    """The facts a case exists for, asserted from the launcher's own record `record(n, c, k)`; returns the record."""
    rec = record(n, case.c, case.k)
    width, nslice, ngroups, lds = rec
    assert width == case.width and nslice * width == case.k and 1 <= ngroups <= n, (case.cid, rec)
    if case.loops:
        owned = [len(range(g, n, ngroups)) for g in range(ngroups)]
        assert min(owned) >= 2 and min(owned) != max(owned), (case.cid, rec, n, "images per workgroup", min(owned), max(owned))
    return rec


# ---- operands
def make_layer(case, n, gen):
    """exact_layers.make_full_range_layer for a 1 x 1 layer, with NZ edge channels instead of its default (which would leave a quarter of a
    64-channel layer live): the channels revived carry weights and biases drawn the same way."""
    lay = X.make_full_range_layer(gen, n, case.c, case.h, case.w, case.k, 1, signed_in=not case.uns, zp=case.zp, edge_bias=not case.res)
    lay.wq[NZ:lay.nz] = torch.randint(-127, 128, tuple(lay.wq[NZ:lay.nz].shape), generator=gen).to(torch.int8)
    lay.nz = NZ
    lay.bias = X.full_range_bias(case.k, NZ, case.k, lay.unit, gen, edge=not case.res) if case.bias else torch.zeros(case.k)
    return lay


def make_shortcut(case, shape, gen):
    """fp32 shortcut (N, K, H, W): multiples of 1/4; `special`: SPECIAL's three."""
    res = torch.randint(-12, 13, shape, generator=gen).float() * 0.25
    if case.special:
        res[SPECIAL["negzero_image"]] = -0.0
        for name, v in (("nan", float("nan")), ("inf", float("inf"))):
            i, ch, p = SPECIAL[name]
            res[i, ch].view(-1)[p] = v
    return res


def pick_quant(kind, pooled):
    """The consumer's quantiser for the reference's pooled values (fp32 (N, K)): a power-of-two scale and, where the kind has one, a zero
    point that put the 10 % tails of the live channels' finite values outside the code range - from the reference alone."""
    v = pooled[:, NZ:]
    v = v[v.isfinite()].double()
    q10, q90 = (float(torch.quantile(v, q)) for q in (0.1, 0.9))
    mid = 0.5 * (q10 + q90)                       # the code range (256 codes, narrower than q10 .. q90) is centred here: both tenths clamp
    if kind in ("plain", "shift"):                # codes 0 .. 255 from 0 up: the top tenth clamps (the bottom: whatever is <= 0)
        assert q90 > 0
        return X.Quant(2.0 ** math.floor(math.log2(q90 / 255.0)), shift128=kind == "shift")
    scale = 2.0 ** math.floor(math.log2((q90 - q10) / 256.0))
    if kind == "uzp":
        return X.Quant(scale, float(round(127.5 - mid / scale)), 0, 255, X.FORM_ZEROPOINT)
    if kind == "signed":
        return X.Quant(scale, float(round(-0.5 - mid / scale)), -128, 127, X.FORM_ZEROPOINT)
    assert kind == "qbase_g"                      # a float offset: the value of code 0
    return X.Quant(scale, float(np.float32(mid - 127.5 * scale)), 0, 255, X.FORM_QBASE, g=0.01)


def quant_facts(pooled, q):
    """(the lower clamp end occurs, the upper one, distinct codes) among the reference's codes of the values that are no NaN."""
    c = X.oracle_codes(pooled, q)
    c = c[~c.isnan()]
    return bool((c == q.lo).any()), bool((c == q.hi).any()), int(c.unique().numel())


def assert_quant_facts(case, pooled, q):
    lo, hi, distinct = quant_facts(pooled, q)
    assert lo and hi and distinct > 100, (case.cid, q.tag(), "lower end", lo, "upper end", hi, "distinct codes", distinct)


@functools.lru_cache(maxsize=None)
def reference(cid, n, zero_at=None):
    """dict(lay, res, shift, pre (fp32 (N, K, H, W): the map before the pool), pooled (fp32 (N, K)), quant) of a case at batch n, every
    exactness condition and the quantiser's facts asserted; `zero_at`: the image that holds only the zero-point code.  Cached and shared:
    nobody writes to it."""
    case = BY_ID[cid]
    gen = torch.Generator().manual_seed(77000 + 13 * CASES.index(case))
    lay = make_layer(case, n, gen)
    shift = 128 if case.uns else 0
    if zero_at is not None:
        lay.codes[zero_at] = case.zp
    true, bias, _ = S.pair_stages(lay, G1, shift)
    res = None
    if case.res:
        res = make_shortcut(case, tuple(true.shape), gen)
        true = X.exact_f32(true + res.double(), "+ shortcut").double()
    S.assert_final_units(true, lay)
    pre = X.exact_f32(X.activation(true, case.act), "activation")
    rows = pre.permute(0, 2, 3, 1).reshape(n, case.h * case.w, case.k).numpy()
    with np.errstate(invalid="ignore", over="ignore"):
        pooled = torch.from_numpy(restate(rows))
    quant = pick_quant(case.quant, pooled)
    assert_quant_facts(case, pooled, quant)
    return dict(lay=lay, bias=bias, res=res, shift=shift, pre=pre, pooled=pooled, quant=quant, zero_at=zero_at)


def prepare(case, record):
    """(N, the launch record with the case's facts asserted, the reference) of a case on the device `record` answers for."""
    n = case.n_for(record)
    rec = launch_facts(case, n, record)
    return n, rec, reference(case.cid, n, 1 + rec[2] if case.zero_image else None)


# ---- the pool kernel (csrc/gap.hip: gap_nhwc_kernel, one thread per (image, 4 channels), `#pragma unroll 8` over the pixels)
POOL_HW = (2, 8, 9, 16, 17)                # every remainder of the unrolled loop that matters: 1, 7, 8 = 0, 15 = 7 + 8, 16 = 0 twice
POOL_SHAPES = [(300, 4, hw) for hw in POOL_HW] + [(300, 12, 9)]      # N > 256 with C = 4: one thread per image, two workgroups; C = 12: the
#                                                                     image index changes inside a wave


def pool_reference(n, c, hw):
    """(rows fp32 [N, HW, C], pooled fp32 (N, C) by the restatement, quantiser)."""
    gen = torch.Generator().manual_seed(5000 + 31 * hw + c)
    rows = (torch.randn(n, hw, c, generator=gen) * 3.0).float()
    pooled = torch.from_numpy(restate(rows.numpy()))
    return rows, pooled, X.Quant(2.0 ** -6, 128.0, 0, 255, X.FORM_ZEROPOINT)
