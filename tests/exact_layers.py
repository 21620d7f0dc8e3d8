"""Int8 layers whose fp32 result is exact, and their exact reference.  TEST INFRASTRUCTURE ONLY.

Input codes are small integers (uint8 in [0, 4] or int8 in [-2, 2]) with an integral zero point and input scale 1; weight codes
are in {-1, 0, 1} with weight scale 1 and an integral weight offset where the kernel has an asymmetric form.  Every sum is then an
integer of a few thousand at most, and fma(sum, 1, bias) (+ residual) is exact for biases and residuals with a few fractional bits:
the float64 convolution below IS the kernel's fp32 result, so the codes of the consumer's quantiser can be compared byte for byte
with no tolerance and no off-by-one allowance.

What the layers carry (the epilogue's hard cases, csrc/conv_epilogue.h):
  * exact rounding ties on even and odd integers - per-channel bias fractions of 0.5 / 1.5 / 2.5 / -0.5 / 0.25 on channels whose
    integer sum changes from pixel to pixel;
  * edge values on channels whose weights are all zero (their output is the bias exactly): NaN, +-inf, +-1e30, -0, values one ulp
    either side of a tie, ties at the clamp bounds (254.5, 255.5, -127.5, -128.5), and v = s (k + 1/2) for the consumer scales
    awkward consumer scales s (AWKWARD_SCALES), where the correctly rounded division v / s hits the tie exactly and v * fl(1 / s)
    may not;
  * the same edge values per pixel through an fp32 residual, for kernels that add one.
The codes come from the oracle's quantisers (oracle/fakequant_oracle.py) and are mapped to bytes as the kernels' code_of does."""
import math
from dataclasses import dataclass
from typing import Optional

import torch
import torch.nn.functional as F

from oracle import fakequant_oracle as O

FORM_EMULATE, FORM_QBASE, FORM_ZEROPOINT, FORM_SYMMETRIC = range(4)      # DLMCQ_FORM_* (include/dlmcq.h)


def _next(v, toward):
    return float(torch.nextafter(torch.tensor(v, dtype=torch.float32), torch.tensor(toward, dtype=torch.float32)))


# the consumer scales with awkward ties: v = s (k + 1/2) is exact and v / s is the tie itself, but fl(1 / s) is not 1 / s.  For 3 and 6
# fl(v * fl(1 / s)) still lands ON the tie for every k (fl(1 / 3) is off by 2^-25 relative, less than half an ulp of any product), so
# those values test that an exact tie is flagged; for 7 and 15 the product lands an ulp or two off the tie for the k below, and a fast
# path that trusted it would round the wrong way - the division must decide.
AWKWARD_SCALES = (3.0, 6.0, 7.0, 15.0)
_AWKWARD_K = {3.0: (0, 1, 2, 5, 40), 6.0: (0, 1, 2, 5, 40), 7.0: (6, 12, 14, 22, 24), 15.0: (2, 6, 10, 12, 14)}
_EDGE_FIXED = [float("nan"), float("inf"), -float("inf"), 1e30, -1e30, -0.0, 254.5, 255.5, 256.0, -127.5, -128.5, 127.5, -1.5, 126.5]
_NEAR_TIES = [_next(k + 0.5, d) for k in (0, 1, 2, 3, 126, 253) for d in (math.inf, -math.inf)]
_AWKWARD = [s * (_AWKWARD_K[s][i] + 0.5) for i in range(5) for s in AWKWARD_SCALES] + [s * -1.5 for s in AWKWARD_SCALES] + [-0.5 * 3.0]
EDGE_VALUES = [float(torch.tensor(v, dtype=torch.float32)) for v in _EDGE_FIXED + _AWKWARD + _NEAR_TIES]
TIE_FRACTIONS = (0.5, -0.5, 1.5, 2.5, 0.25, 0.0)


@dataclass(frozen=True)
class Quant:
    """A consumer quantiser as the int8 entry points take it (kernels.EmitCodes)."""
    scale: float
    zp: Optional[float] = None
    lo: int = 0
    hi: int = 255
    form: int = FORM_ZEROPOINT
    g: float = 0.0
    shift128: bool = False

    @property
    def plain(self):
        """The quantiser of every post-ReLU tensor (epi_plain): unsigned byte range, no zero point tensor."""
        return self.zp is None and self.lo == 0 and self.hi == 255

    def tag(self):
        z = "plain" if self.zp is None else f"zp{self.zp:g}"
        return f"f{self.form}_s{self.scale:g}_{z}_{self.lo}_{self.hi}" + ("_x80" if self.shift128 else "")


def plain_quants():
    """The plain quantiser at every scale the epilogue treats differently: exact ties (1, 0.5), awkward ties (3, 6, 7, 15), an
    ordinary scale (0.1), saturating tame scales (1e-30, 2^-100: the `tame` bound) and a denormal one (1e-41: rdv is NaN, all exact)."""
    scales = (1.0, 0.5, 3.0, 6.0, 7.0, 15.0, 0.1, 1e-30, 2.0 ** -100)
    # (the denormal scale in QBASE form, which clamps before it rounds: v / s = inf gives 255 there, where the STE round of the other
    #  forms turns it into NaN -> code 0 - the same byte a NaN reciprocal would give)
    return [Quant(s, form=FORM_SYMMETRIC if i % 2 else FORM_ZEROPOINT) for i, s in enumerate(scales)] + [Quant(1e-41, form=FORM_QBASE)]


def nonplain_quants():
    """Quantisers with a zero point / offset or a signed range, at exact and awkward scales (g = 0: the divisor is the scale)."""
    return [Quant(1.0, 3.0), Quant(3.0, 3.0), Quant(7.0, 3.0), Quant(15.0, 3.0, form=FORM_QBASE), Quant(6.0, 3.0, form=FORM_QBASE),
            Quant(1.0, -5.0, -127, 127), Quant(7.0, None, -128, 127), Quant(6.0, 2.0, 0, 255, FORM_EMULATE), Quant(1e-41, 3.0),
            Quant(0.5, 0.0)]


def f32(v):
    return torch.tensor(v, dtype=torch.float32)


def oracle_codes(v, q):
    """Float codes (NaN possible) of an fp32 tensor under quantiser q - the oracle's forms."""
    s, z = f32(q.scale), f32(0.0 if q.zp is None else q.zp)
    if q.form == FORM_EMULATE:
        return O.fq_emulate(v, s, z, q.lo, q.hi)[0]
    if q.form == FORM_QBASE:
        return O.fq_qbase(v, s, z, q.lo, q.hi, q.g)[0]
    if q.form == FORM_ZEROPOINT:
        return O.fq_zeropoint(v, s, z, q.lo, q.hi)[0]
    return O.fq_symmetric(v, s, q.lo, q.hi)[0]


def code_bytes(codes, q):
    """Float codes -> the bytes the kernels store (code_of): NaN -> 0, negatives two's complement, ^ 0x80 under SHIFT128; the dtype of
    kernels.EmitCodes.dtype."""
    c = torch.nan_to_num(codes, nan=0.0).to(torch.int32)
    if q.shift128:
        return ((c & 0xff) ^ 0x80).to(torch.uint8).view(torch.int8)
    return c.to(torch.uint8) if q.lo >= 0 else c.to(torch.int8)


def quantise(v, q):
    assert v.dtype == torch.float32
    return code_bytes(oracle_codes(v, q), q)


def code_ints(v, q):
    """The oracle's codes of an fp32 tensor as int64 (NaN -> 0, as code_of): the integers themselves, whatever byte the range stores
    them in - `quantise(v, q).long()` wherever the range is a uint8 or an int8 one."""
    assert v.dtype == torch.float32
    return torch.nan_to_num(oracle_codes(v, q), nan=0.0).long()


def dequant_scale(q):
    """The fp32 scale a form dequantises with, float64: QBASE (s - s g) + s g in fp32 (the oracle's ste_scale), else the scale."""
    s = f32(q.scale)
    return float(O.ste_scale(s, q.g) if q.form == FORM_QBASE else s)


def exact_fma(a64, m64, b64, what="fma"):
    """fl32(a * m + b) as ONE rounding of the exact value - the device's fused multiply-add - from float64 tensors that hold fp32
    numbers.  Asserted for every element, none left out: the three operands are fp32 numbers (so a * m, 24 x 24 bits, is exact in
    float64) and the float64 sum p + b has no rounding error (Knuth's TwoSum: the error term is 0), so the single cast to fp32 is the
    only rounding.  A sum that is not finite (a NaN or an infinity in b) needs no argument."""
    a64, m64, b64 = torch.broadcast_tensors(a64, m64, b64)
    for t in (a64, m64, b64):
        back = t.float().double()
        assert bool(((back == t) | (back.isnan() & t.isnan())).all()), f"{what}: an operand is no fp32 number"
    p = a64 * m64
    assert bool(((p != 0) | (a64 == 0) | (m64 == 0) | p.isnan()).all()), f"{what}: the product underflows float64"
    s = p + b64
    bb = s - p
    err = (p - (s - bb)) + (b64 - bb)
    ok = (err == 0) | ~s.isfinite()
    assert bool(ok.all()), f"{what}: {int((~ok).sum())} float64 sums are not exact, e.g. {s[~ok].flatten()[:4].tolist()}"
    return s.float()


def exact_f32(v64, what="reference"):
    """float64 -> float32, asserting the cast is exact (NaN stays NaN)."""
    v32 = v64.float()
    back = v32.double()
    ok = (back == v64) | (back.isnan() & v64.isnan())
    assert bool(ok.all()), f"{what}: {int((~ok).sum())} values not exact in fp32, e.g. {v64[~ok].flatten()[:4].tolist()}"
    return v32


def activation(v64, act):
    """torch semantics on float64: 0 none, 1 ReLU, 2 ReLU6 (NaN kept)."""
    if act == 1:
        return torch.relu(v64)
    if act == 2:
        return F.relu6(v64)
    return v64


@dataclass
class Layer:
    """The integer operands of an int8 convolution (CPU tensors).  codes: (N, C, H, W) uint8 / int8; wq: int8 (K, C / groups, R, S);
    zero-weight channels [0, nz); bias fp32 [K]; w_off fp32 [K] or None; zp: the input zero point."""
    codes: torch.Tensor
    zp: float
    wq: torch.Tensor
    bias: torch.Tensor
    w_off: Optional[torch.Tensor]
    nz: int
    groups: int = 1

    def x64(self):
        return self.codes.double() - self.zp

    def w64(self):
        w = self.wq.double()
        if self.w_off is not None:
            w = w + self.w_off.double().reshape(-1, 1, 1, 1)
        return w


def edge_bias(k, nz, gen, values=None):
    """Bias [k]: the edge values on channels [0, nz) (cycled), tie fractions plus small integers on the others."""
    values = EDGE_VALUES if values is None else values
    b = torch.empty(k, dtype=torch.float32)
    for i in range(nz):
        b[i] = values[i % len(values)]
    live = k - nz
    if live:
        frac = torch.tensor(TIE_FRACTIONS, dtype=torch.float32)[torch.arange(live) % len(TIE_FRACTIONS)]
        b[nz:] = frac + torch.randint(-3, 4, (live,), generator=gen).float()
    return b


def make_layer(gen, n, c, h, w, k, r, s=None, *, nz=None, signed_in=False, zp=0.0, asym=False, depthwise=False, density=0.5):
    """Random exact operands.  nz zero-weight channels first (default: as many as there are edge values, leaving a quarter of the
    channels - at least 8 - live)."""
    s = r if s is None else s
    nz = min(len(EDGE_VALUES), k - max(8, k // 4)) if nz is None else nz
    if signed_in:
        codes = torch.randint(-2, 3, (n, c, h, w), generator=gen).to(torch.int8)
    else:
        codes = torch.randint(0, 5, (n, c, h, w), generator=gen).to(torch.uint8)
    cin = 1 if depthwise else c
    wq = torch.randint(-1, 2, (k, cin, r, s), generator=gen).to(torch.int8)
    wq[torch.rand(wq.shape, generator=gen) > density] = 0
    wq[:nz] = 0
    w_off = None
    if asym:
        w_off = torch.randint(-1, 2, (k,), generator=gen).float()
        w_off[:nz] = 0.0
    return Layer(codes, float(zp), wq, edge_bias(k, nz, gen), w_off, nz, c if depthwise else 1)


def edge_residual(shape, nz, gen):
    """fp32 residual (N, K, P, Q): the edge values per pixel on channels [0, nz) (the layer's bias there must be 0), multiples of 0.25
    with an occasional +-inf / NaN on the others."""
    n, k, p, q = shape
    res = (torch.randint(-12, 13, shape, generator=gen).float() * 0.25)
    ev = torch.tensor(EDGE_VALUES, dtype=torch.float32)
    idx = (torch.arange(n * p * q).reshape(n, 1, p, q) + torch.arange(nz).reshape(1, nz, 1, 1) * 7) % len(EDGE_VALUES)
    res[:, :nz] = ev[idx]
    live = res[:, nz:]
    spots = torch.rand(live.shape, generator=gen)
    live[spots < 0.002] = float("inf")
    live[(spots >= 0.002) & (spots < 0.004)] = -float("inf")
    live[(spots >= 0.004) & (spots < 0.006)] = float("nan")
    return res


def conv_ref(layer, stride=1, pad=0, residual=None, act=0, pool=False):
    """The layer's exact output, float64 -> fp32: convolution of the integer operands, + bias, + residual, activation (torch
    semantics), and for the pooling first layer ReLU -> max_pool2d(3, 2, 1)."""
    y = F.conv2d(layer.x64(), layer.w64(), stride=stride, padding=pad, groups=layer.groups)
    y = y + layer.bias.double().reshape(1, -1, 1, 1)
    if residual is not None:
        y = y + residual.double()
    y = activation(y, act)
    if pool:
        y = F.max_pool2d(y, 3, 2, 1)
    return exact_f32(y, "layer output")


def second_gemm_ref(codes1, q1, wq2, bias2, act2=1, w_off2=None):
    """The 1x1 layer that reads the first quantiser's codes (chain, dual chain, dwpw): its input is (code - zp) * s1, taken from the
    reference's own first-layer codes; weight scale 1.  codes1: the bytes of quantise(.., q1) (unshifted)."""
    c = codes1.to(torch.int32).double()
    x = (c - (0.0 if q1.zp is None else q1.zp)) * q1.scale
    w = wq2.double()
    if w_off2 is not None:
        w = w + w_off2.double().reshape(-1, 1, 1, 1)
    y = F.conv2d(x, w) + bias2.double().reshape(1, -1, 1, 1)
    return exact_f32(activation(y, act2), "second layer output")


def identity_pw(k, c, nz, gen, density=0.05):
    """Weights [k, c, 1, 1] of a 1x1 layer that shows the first layer's codes: output channel j < c reads input channel j with weight +1
    (and little else), channels [c, c + nz) are all zero (edge biases), the rest sparse {-1, 0, 1}; with its bias."""
    wq = torch.randint(-1, 2, (k, c, 1, 1), generator=gen).to(torch.int8)
    wq[torch.rand(wq.shape, generator=gen) > density] = 0
    m = min(k, c)
    wq[:m] = 0
    wq[torch.arange(m), torch.arange(m)] = 1
    nz = max(0, min(nz, k - m))
    wq[m:m + nz] = 0
    b = edge_bias(k, 0, gen)
    b[:m] += 4.0 - b[:m].floor() + torch.randint(0, 4, (m,), generator=gen).float()     # (positive: a first code that moves shows after ReLU)
    for i in range(nz):
        b[m + i] = EDGE_VALUES[i % len(EDGE_VALUES)]
    return wq, b


# ------------------------------------------------------------------------------------------------ full-range operands, dyadic scales
# The int32 accumulation of the int8 kernels is exact and their dequantisation is ONE fma.  With power-of-two scales the fp32 result is
# therefore the real-valued result for operands over the whole byte range, as long as every fp32 stage of the epilogue's chain stays
# representable (sums below 2^24 units): the layers below have codes uniform over all 256 byte values, weight codes uniform in +-127,
# per-channel weight scales 2^-(10 + k % 5) that differ from channel to channel, an input scale 2^e != 1 and biases that are multiples of
# each channel's s_in * s_w[k] - and are still compared with no tolerance (tests/test_gpu_tiled_variants.py).
FULL_TARGET_SIGMA = 12.0        # standard deviation of the outputs of the widest-scale channels: a good share of them lies in (0, 6)
TIE_SCALES = (0.25, 2.0 ** -5, 0.5)     # the consumer scales of tests/test_gpu_tiled_variants.py: the biases carry tie fractions against them


@dataclass
class FullLayer:
    """codes (N, C, H, W) uint8 / int8 over the full byte range; wq int8 (K, C, R, S) in +-127, zero on channels [0, nz) and [live, K);
    s_w fp32 [K] dyadic; w_int int [K] or None: the weight offset in units of s_w[k]; s_in a power of two; bias fp32 [K]."""
    codes: torch.Tensor
    zp: int
    wq: torch.Tensor
    s_w: torch.Tensor
    w_int: Optional[torch.Tensor]
    s_in: float
    bias: torch.Tensor
    nz: int
    live: int
    groups: int = 1                 # the depthwise form: groups = channels, wq (C, 1, R, S)

    @property
    def unit(self):                 # s_in * s_w[k], float64 (a power of two: exact)
        return self.s_in * self.s_w.double()

    @property
    def w_off(self):
        return None if self.w_int is None else exact_f32(self.w_int.double() * self.s_w.double(), "weight offset")

    def xint(self):
        return self.codes.double() - self.zp

    def w64(self):
        w = self.wq.double() if self.w_int is None else self.wq.double() + self.w_int.double().reshape(-1, 1, 1, 1)
        return w * self.s_w.double().reshape(-1, 1, 1, 1)


def full_range_bias(k, nz, live, unit, gen, edge=True):
    """Bias [k], every entry a multiple of its channel's unit: the edge values (or 0: `edge=False`, a residual carries them) on the
    zero-weight channels [0, nz), tie fractions against the consumer scales plus small integers on [nz, live), 0 on [live, k)."""
    b = torch.zeros(k, dtype=torch.float64)
    n = live - nz
    idx = torch.arange(n)
    s = torch.tensor(TIE_SCALES, dtype=torch.float64)[idx % len(TIE_SCALES)]
    frac = torch.tensor(TIE_FRACTIONS, dtype=torch.float64)[(idx // len(TIE_SCALES)) % len(TIE_FRACTIONS)]
    b[nz:live] = s * (frac + torch.randint(-3, 4, (n,), generator=gen).double())
    q = b[nz:live] / unit[nz:live]
    assert bool((q == q.round()).all()), "a bias is no multiple of its channel's s_in * s_w[k]"
    b = b.float()
    if edge:
        for i in range(nz):
            b[i] = EDGE_VALUES[i % len(EDGE_VALUES)]
    return b


def full_range_sigma(taps, signed_in, zp):
    """Standard deviation of the integer sum of `taps` products of a uniform byte about its zero point and a uniform weight code in
    +-127 - from the shape alone."""
    mean = (-0.5 if signed_in else 127.5) - zp
    return math.sqrt(taps) * math.sqrt((127 * 128) / 3.0) * math.sqrt((256 * 256 - 1) / 12.0 + mean * mean)


def make_full_range_layer(gen, n, c, h, w, k, r, s=None, *, signed_in=False, asym=False, zp=None, live=None, edge_bias=True, zp_side=None,
                          depthwise=False):
    """Random full-range operands (see above).  `depthwise`: k == c groups of one channel - wq is (C, 1, R, S), the input scale is sized
    from the R S taps of one channel, and the codes lie in memory as NHWC (a permuted view: the depthwise tensors are large).  zp: the input zero point - default: an integer in 1..254 other than 128 for uint8 codes,
    0 for int8 codes.  `live`: channels [live, k)
    are all zero (the padding of a narrow layer).  `zp_side`: "high" / "low" - a uint8 zero point above / below 128 (padded calls: the pad-table
    byte has its high bit set, or not; a wrong sign or shift of the padding shows in the first); default: either."""
    s = r if s is None else s
    live = k if live is None else live
    nz = min(len(EDGE_VALUES), live - max(8, live // 4))
    assert not depthwise or k == c
    shape = (n, h, w, c) if depthwise else (n, c, h, w)
    if signed_in:
        codes = torch.randint(-128, 128, shape, generator=gen).to(torch.int8)
        zp = 0 if zp is None else zp
    else:
        codes = torch.randint(0, 256, shape, generator=gen).to(torch.uint8)
        if zp is None:
            d = int(torch.randint(1, 127, (1,), generator=gen))
            up = bool(torch.randint(0, 2, (1,), generator=gen)) if zp_side is None else zp_side == "high"
            zp = 128 + d if up else 128 - d
    if depthwise:
        codes = codes.permute(0, 3, 1, 2)
    cin = 1 if depthwise else c
    wq = torch.randint(-127, 128, (k, cin, r, s), generator=gen).to(torch.int8)
    wq[:nz] = 0
    wq[live:] = 0
    s_w = (2.0 ** -(10 + torch.arange(k) % 5).double()).float()
    w_int = None
    if asym:
        w_int = torch.randint(-1, 2, (k,), generator=gen)
        w_int[:nz] = 0
        w_int[live:] = 0
    # the input scale: a power of two that puts the widest-scale channels' outputs at FULL_TARGET_SIGMA (from the shape alone: the
    # integer sum of r s c products of a uniform byte about its zero point and a uniform weight code)
    sigma_int = full_range_sigma(r * s * cin, signed_in, zp)
    s_in = 2.0 ** round(math.log2(FULL_TARGET_SIGMA / (sigma_int * 2.0 ** -10)))
    if depthwise and s_in == 1.0:
        s_in = 0.5                  # (a 1 x 1 filter: the target lands on 1, and a scale of 1 hides a dropped multiplication)
    lay = FullLayer(codes, int(zp), wq, s_w, w_int, s_in, torch.zeros(k), nz, live, c if depthwise else 1)
    lay.bias = full_range_bias(k, nz, live, lay.unit, gen, edge=edge_bias)
    return lay


def second_gemm_full_ref(codes1, q1, wq2, s_w2, bias2, act2=1, w_int2=None):
    """second_gemm_ref on full-range operands: the 1x1 layer that reads the reference's own first-stage codes as (code - zp) * q1.scale
    against weight codes in +-127 with dyadic per-channel scales s_w2 [K] and, in the asymmetric form, a weight offset of w_int2[k] units
    of s_w2[k].  codes1: (N, C, P, Q) bytes of quantise(.., q1), unshifted; asserts |SUM (code - zp) qw| < 2^24 (the kernel's fma takes
    the integer sum as an fp32 number) and that the result is one."""
    assert q1.lo == 0 and q1.hi == 255 and not q1.shift128
    ci = codes1.to(torch.int32).double() - (0.0 if q1.zp is None else q1.zp)
    isum = F.conv2d(ci, wq2.double())
    assert float(isum.abs().max()) < float(1 << 24), "the second layer's integer sum is no fp32 number"
    w = wq2.double() if w_int2 is None else wq2.double() + w_int2.double().reshape(-1, 1, 1, 1)
    y = F.conv2d(ci * q1.scale, w * s_w2.double().reshape(-1, 1, 1, 1))
    unit = q1.scale * s_w2.double().reshape(1, -1, 1, 1)
    first = exact_f32(isum * unit + bias2.double().reshape(1, -1, 1, 1), "second layer: fma(sum, s_in s_w, bias)").double()
    if w_int2 is not None:
        first = exact_f32(first + ci.sum(dim=1, keepdim=True) * (w_int2.double().reshape(1, -1, 1, 1) * unit), "second layer: + rowsum * s_in w_off").double()
    y = y + bias2.double().reshape(1, -1, 1, 1)
    ok = (first == y) | (first.isnan() & y.isnan())
    assert bool(ok.all()), "second layer: the staged chain and the convolution of the dequantised operands disagree"
    return exact_f32(activation(y, act2), "second layer output")


@dataclass
class SecondLayer:
    """The 1x1 layer behind a first quantiser (chain, dual chain, recomputing chain): wq int8 (K2, K, 1, 1) in +-127, zero on the edge
    channels [0, nz); s_w fp32 [K2] dyadic; bias fp32 [K2], multiples of q1.scale * s_w[k] on the live channels, the edge values on the others."""
    wq: torch.Tensor
    s_w: torch.Tensor
    bias: torch.Tensor
    nz: int


def make_full_range_second(gen, codes1, q1, k2):
    """Full-range operands of the layer that reads the REFERENCE's own first-stage codes `codes1` (N, K, P, Q; bytes of quantise(.., q1),
    unshifted) as (code - zp) * q1.scale: weight codes uniform in +-127, per-channel dyadic scales s_w[k] = 2^(e - k % 5) that differ from
    channel to channel, biases that are multiples of each channel's q1.scale * s_w[k] and carry the tie fractions of full_range_bias.  e is
    sized the way make_full_range_layer sizes its input scale - a power of two from the shape (K products per sum, a uniform weight code)
    and from the codes' own second moment about the zero point - so that the widest channels' outputs have FULL_TARGET_SIGMA."""
    k = codes1.shape[1]
    nz = min(len(EDGE_VALUES), k2 - max(8, k2 // 4))
    wq = torch.randint(-127, 128, (k2, k, 1, 1), generator=gen).to(torch.int8)
    wq[:nz] = 0
    ci = codes1.to(torch.int32).double() - (0.0 if q1.zp is None else q1.zp)
    sigma_int = math.sqrt(k * float((ci * ci).mean()) * (127 * 128) / 3.0)
    e = round(math.log2(FULL_TARGET_SIGMA / (q1.scale * sigma_int)))
    s_w = (2.0 ** (e - torch.arange(k2) % 5).double()).float()
    lay = SecondLayer(wq, s_w, torch.zeros(k2), nz)
    lay.bias = full_range_bias(k2, nz, k2, q1.scale * s_w.double(), gen)
    return lay
