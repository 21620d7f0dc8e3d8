"""The calls of the operand-preparation kernels - the small kernels that turn fp32 weights and images into the bytes the matrix-core kernels
read - with a plain reference for each: ONE table per kernel for tests/test_operand_cases_host.py (the facts every case exists for, proven on
the CPU, so that no case passes vacuously) and tests/test_gpu_operands_exact.py (the same calls launched and compared byte for byte, every
output in a sentinel-filled buffer with guard bytes behind it).  TEST INFRASTRUCTURE ONLY: nothing here imports the library.

  weights   dlmcq_quantize_weight_krsc_i8 (csrc/conv_i8.hip) and dlmcq_quantize_weight_stem_i8 (csrc/conv_stem_i8.hip):
            q = clamp(R(fl32(w / s_k)), lo, hi), NaN -> code 0, wsum[k] = SUM codes (include/dlmcq.h).  Two references: the oracle's
            fq_symmetric (the same IEEE fp32 operations) everywhere, and float64 arithmetic on the DYADIC rows w = fl32(m s_k), s_k a power
            of two and m a multiple of 1/2, where the quotient is m exactly.  `edge_weights`: per row a walk over the ladder lo - 2.5 ..
            hi + 2.5 in steps of 1/2 (every tie m +- 1/2 of the range, the four ties at the clamp ends, values beyond both ends; ordered
            from both ends inward so that short rows reach the clamp ends first) and SPECIALS (NaN, +-inf, -0, a denormal, +-1e30); per
            channel scales that differ, with (the [K] layout) a negative one, one so small that 1e30 / s overflows, and 0 (x / 0, 0 / 0).
            `wsum_weights`: rows whose codes are all hi, all lo, alternating.  `gauss_weights`: Gaussian rows, non-dyadic scales.
  image     dlmcq_quantize_pad_nhwc4: `edge_image` (ties and exact_layers.EDGE_VALUES at the four corner pixels of every channel and at
            random positions) in every layout of IMAGE_LAYOUTS; `image_route` restates the host's route condition; `image_expected` the
            padded NHWC4 bytes (channels >= C: 0 inside the image; border: the border code in all four bytes).
  pool      dlmcq_maxpool_codes_nhwc against F.max_pool2d of the codes as float64.
  pack      dlmcq_pack_int4 / dlmcq_unpack_int4 against two lines of integer torch.
  table     dlmcq_dwpw_pack_table against the record of its header comment restated in numpy.
  grid cap  GRID_CAP: one size per kernel that takes the second trip of its grid-stride loop."""
from dataclasses import dataclass

import numpy as np
import torch
import torch.nn.functional as F

import exact_layers as X
from oracle import fakequant_oracle as O

EINVAL, EALIGN = -1, -4                     # DLMCQ_EINVAL, DLMCQ_EALIGN (include/dlmcq.h)
SENTINELS = (0x5A, 0xA5)                    # every output is written into both fills: a byte that keeps BOTH was never written
GUARD = 256                                 # bytes behind every output that must keep the fill


# ------------------------------------------------------------------------------------------------ weights
RANGES = ((-127, 127), (-128, 127), (-8, 7), (-7, 7), (0, 15), (0, 0))
SCALE_LAYOUTS = ("tensor", "channel")       # one scale (numel == 1); a [K, 1, 1, 1] scale
SPECIALS = (float("nan"), float("inf"), -float("inf"), -0.0, 1e-41, 1e30, -1e30)
KRSC_SHAPES = {
    # cid: (shape, the facts the shape exists for)
    "one": ((1, 1, 1, 1), "a single element"),
    "sub_wave": ((3, 1, 3, 3), "9 elements: less than a wave"),
    "r1s3": ((5, 7, 1, 3), "R != S, odd C: the (c, r, s) -> (r, s, c) transposition"),
    "r3s1": ((5, 7, 3, 1), "R != S the other way"),
    "wave64": ((4, 64, 1, 1), "exactly one wave"),
    "wave65": ((4, 65, 1, 1), "one element in the second wave"),
    "block255": ((2, 255, 1, 1), "one short of the block"),
    "block256": ((2, 256, 1, 1), "exactly one trip of the block loop"),
    "block257": ((2, 257, 1, 1), "the second trip of the block loop"),
    "c64_3x3": ((3, 64, 3, 3), "a real 3 x 3 layer: 576 elements"),
    "c512_3x3": ((2, 512, 3, 3), "4608 elements: 18 trips; the wsum rows"),
    "linear": ((1000, 128), "a 2-D Linear weight: more workgroups than CUs"),
}
GAUSS_SHAPES = ("r1s3", "c64_3x3", "linear")
WSUM_SHAPE = "c512_3x3"
STEM_C, STEM_R, STEM_S, STEM_K = (1, 2, 3, 4), (1, 3, 7), (1, 3, 7, 8), (1, 8, 64, 96)


def ladder(lo, hi):
    """The multiples of 1/2 in [lo - 2.5, hi + 2.5], from both ends inward: hi + 2.5, lo - 2.5, hi + 2, lo - 2, ..."""
    a = np.arange(2 * lo - 5, 2 * hi + 6, dtype=np.float64) / 2
    out = np.empty_like(a)
    out[0::2] = a[::-1][:(len(a) + 1) // 2]
    out[1::2] = a[:len(a) // 2]
    return out


def channel_scales(k_out, layout):
    """([K] fp32 scales, [K] kinds): powers of two that differ from channel to channel; in the [K] layout channels 2, 3, 4 (mod 5) carry a
    negative scale, one so small that 1e30 / s overflows, and 0."""
    if layout == "tensor":
        return np.full(k_out, 2.0 ** -4, np.float32), ["normal"] * k_out
    kinds = [("normal", "normal", "negative", "tiny", "zero")[k % 5] for k in range(k_out)]
    val = {"negative": -2.0 ** -3, "tiny": 2.0 ** -120, "zero": 0.0}
    return np.array([val.get(kind, 2.0 ** -(2 + k % 4)) for k, kind in enumerate(kinds)], np.float32), kinds


@dataclass
class Weights:
    """One call's operands (CPU): w fp32 KCRS (or [K, C]); scale as the wrapper takes it; s_k [K] float32 numpy; m [K, n] float64: the
    exact quotient w / s_k on the dyadic positions, NaN elsewhere; kinds [K]."""
    w: torch.Tensor
    scale: torch.Tensor
    s_k: np.ndarray
    m: np.ndarray
    kinds: list

    @property
    def dyadic(self):
        return ~np.isnan(self.m)


def _finish(shape, m, special, s_k, kinds, layout):
    """special [K, n]: the index into SPECIALS a position holds, -1 for a multiple m of the row's scale."""
    k_out = shape[0]
    w64 = m * s_k.astype(np.float64)[:, None]
    zero = np.array([kind == "zero" for kind in kinds])
    w64[zero] = m[zero]                                 # scale 0: the values themselves (x / 0) and 0 (0 / 0)
    w = w64.astype(np.float32)
    assert (w.astype(np.float64) == w64).all(), "a dyadic weight is no fp32 number"
    w[special >= 0] = np.array(SPECIALS, np.float32)[special[special >= 0]]
    m = np.where((special >= 0) | zero[:, None], np.nan, m)
    scale = torch.from_numpy(s_k[:1].copy()) if layout == "tensor" else torch.from_numpy(s_k.copy()).reshape((k_out,) + (1,) * (len(shape) - 1))
    return Weights(torch.from_numpy(w).reshape(shape), scale, s_k, m, kinds)


def edge_weights(shape, lo, hi, layout):
    k_out, n = shape[0], int(np.prod(shape[1:]))
    lad = ladder(lo, hi)
    period = len(SPECIALS) + len(lad)
    j = (np.arange(k_out)[:, None] * n + np.arange(n)[None, :]) % period
    special = np.where(j < len(SPECIALS), j, -1)
    m = np.where(special >= 0, 0.0, lad[np.maximum(j - len(SPECIALS), 0)])
    s_k, kinds = channel_scales(k_out, layout)
    return _finish(shape, m, special, s_k, kinds, layout)


def wsum_weights(shape, lo, hi, layout, first):
    """Row k holds codes that are all hi ((k + first) % 3 == 0: m = hi, hi + 1, hi + 2, ...), all lo (1) or hi, lo alternating (2)."""
    k_out, n = shape[0], int(np.prod(shape[1:]))
    i = np.arange(n, dtype=np.float64)[None, :]
    role = ((np.arange(k_out) + first) % 3)[:, None]
    m = np.where(role == 0, hi + i % 3, np.where(role == 1, lo - i % 3, np.where(i % 2 == 0, float(hi), float(lo))))
    s_k, kinds = channel_scales(k_out, "tensor")
    if layout == "channel":
        s_k = (2.0 ** -(2 + np.arange(k_out) % 4)).astype(np.float32)
    return _finish(shape, m, np.full(m.shape, -1), s_k, kinds, layout), role[:, 0]


def gauss_weights(shape, lo, hi, layout, seed):
    """Gaussian rows with the scale the flow gives them: amax / max(|lo|, |hi|, 1) + 1e-6, per channel or per tensor - not dyadic."""
    gg = torch.Generator().manual_seed(7700 + seed)
    k_out = shape[0]
    w = torch.randn(shape, generator=gg) * 0.05
    amax = w.abs().amax() if layout == "tensor" else w.reshape(k_out, -1).abs().amax(dim=1)
    s = (amax / float(max(abs(lo), abs(hi), 1)) + 1e-6).reshape(-1)
    scale = s if layout == "tensor" else s.reshape((k_out,) + (1,) * (len(shape) - 1))
    s_k = s.expand(k_out).contiguous().numpy()
    return Weights(w, scale, s_k, np.full((k_out, w[0].numel()), np.nan), ["gauss"] * k_out)


def oracle_weight_codes(wt, lo, hi):
    """int8 codes in the input's own KCRS order: the oracle's fq_symmetric, NaN -> 0."""
    s = torch.from_numpy(wt.s_k.copy()).reshape((-1,) + (1,) * (wt.w.dim() - 1))
    q = O.fq_symmetric(wt.w, s, lo, hi)[0]
    return torch.nan_to_num(q, nan=0.0).to(torch.int32).to(torch.int8)


def float64_weight_codes(wt, lo, hi):
    """[K, n] float64: clamp(rint(m), lo, hi) on the dyadic positions (rint: half to even, as IEEE fp32's), NaN elsewhere."""
    return np.clip(np.rint(wt.m), lo, hi)


def krsc_index(k, c, r, s, C, R, S):
    """Where element [k][c][r][s] of the fp32 weight goes in the KRSC code tensor (flat)."""
    return ((k * R + r) * S + s) * C + c


def stem_index(k, c, r, s, R):
    """... and in the first layer's [K][R][8 taps][4 channels] tensor."""
    return ((k * R + r) * 8 + s) * 4 + c


def krsc_layout(codes):
    """codes int8 [K, C, R, S] (or [K, C]) -> [K, R, S, C]."""
    if codes.dim() == 2:
        codes = codes[:, :, None, None]
    return codes.permute(0, 2, 3, 1).contiguous()


def stem_layout(codes):
    """codes int8 [K, C, R, S] -> [K, R, 8, 4], taps >= S and channels >= C zero."""
    k_out, c, r, s = codes.shape
    out = torch.zeros((k_out, r, 8, 4), dtype=torch.int8)
    out[:, :, :s, :c] = codes.permute(0, 2, 3, 1)
    return out


def wsum_of(codes):
    return codes.reshape(codes.shape[0], -1).to(torch.int64).sum(dim=1)


def weight_facts(wt, codes, lo, hi):
    """The facts present in one call's operands and reference codes ([K, C, R, S] int8)."""
    k_out = codes.shape[0]
    c = codes.reshape(k_out, -1).numpy().astype(np.int64)
    w = wt.w.reshape(k_out, -1).numpy()
    m, dy = wt.m, wt.dyadic
    facts = set()
    with np.errstate(invalid="ignore"):
        tie = dy & (m * 2 % 2 == 1)
        if (dy & (m > hi + 0.5) & (c == hi)).any():
            facts.add("clamp_hi")
        if (dy & (m < lo - 0.5) & (c == lo)).any():
            facts.add("clamp_lo")
        if (tie & (m > 0)).any():
            facts.add("tie_pos")
        if (tie & (m < 0)).any():
            facts.add("tie_neg")
        present = set(m[tie].tolist())
        if {hi - 0.5, hi + 0.5, lo - 0.5, lo + 0.5} <= present:
            facts.add("ties_at_bounds")
        if {v + 0.5 for v in range(lo - 1, hi + 1)} <= present:
            facts.add("every_tie")
    if (np.isnan(w) & (c == 0)).any():
        facts.add("nan_code0")
    if (np.isinf(w) & (c == 0)).any():
        facts.add("inf_code0")
    if (np.signbit(w) & (w == 0)).any():
        facts.add("neg_zero")
    if ((w != 0) & (np.abs(w) < 2.0 ** -126)).any():
        facts.add("denormal")
    if (np.abs(w) == np.float32(1e30)).any():
        facts.add("huge")
    for k, kind in enumerate(wt.kinds):
        if kind == "negative" and (dy[k] & (c[k] != 0)).any():
            facts.add("negative_scale")
        if kind == "tiny" and (np.isfinite(w[k]) & (np.abs(w[k]) == np.float32(1e30)) & (c[k] == 0)).any():
            facts.add("overflow")                      # 1e30 / 2^-120 = inf -> R(inf) = NaN -> code 0 (a clamp alone would give hi)
        if kind == "zero" and (w[k] != 0).any() and (w[k] == 0).any() and (c[k] == 0).all():
            facts.add("zero_scale")
    return facts


# what a shape's edge rows must show, per scale layout (the host test asserts it for every range; (0, 0) has no tie inside its range)
SMALL = {"one", "sub_wave"}
EDGE_FACTS = {"clamp_hi", "clamp_lo", "tie_pos", "tie_neg", "ties_at_bounds", "nan_code0", "inf_code0", "neg_zero", "denormal", "huge"}
CHANNEL_FACTS = {"negative_scale", "overflow", "zero_scale"}          # the [K] layout: every one in the 1000-row shape, whose rows walk through everything


def stated_facts(cid, shape, lo, hi, layout):
    if cid in SMALL:
        return set()
    n = int(np.prod(shape[1:]))
    facts = set(EDGE_FACTS)
    if shape[0] * n >= len(SPECIALS) + 2 * (hi - lo) + 11:
        facts.add("every_tie")
    if layout == "channel" and shape[0] >= 3 and (lo, hi) != (0, 0):
        facts.add("negative_scale")                     # (a range of one code shows no sign)
    if layout == "channel" and cid == "linear":
        facts |= {"overflow", "zero_scale"}
    return facts


WEIGHT_REFUSALS = (
    # what, overrides of (K, C, R, S, lo, hi), which pointer is NULL, return code: krsc, stem
    ("lo > hi", dict(lo=3, hi=2), None, EINVAL, EINVAL),
    ("lo < -128", dict(lo=-129), None, EINVAL, EINVAL),
    ("hi > 127", dict(hi=128), None, EINVAL, EINVAL),
    ("w NULL", {}, 0, EINVAL, EINVAL),
    ("wq NULL", {}, 1, EINVAL, EINVAL),
    ("wsum NULL", {}, 2, EINVAL, EINVAL),
    ("scale NULL", {}, 3, EINVAL, EINVAL),
    ("K = 0", dict(K=0), None, 0, EINVAL),
    ("C = 5", dict(C=5), None, None, EINVAL),
    ("R = 8", dict(R=8), None, None, EINVAL),
    ("S = 9", dict(S=9), None, None, EINVAL),
)
REFUSAL_BASE = dict(K=4, C=3, R=3, S=3, lo=-127, hi=127)


# ------------------------------------------------------------------------------------------------ image
SHIFTED = [X.Quant(1.0, None, 0, 255, X.FORM_ZEROPOINT, shift128=True), X.Quant(3.0, 3.0, 0, 255, X.FORM_ZEROPOINT, shift128=True)]
IMAGE_QUANTS = X.plain_quants() + X.nonplain_quants() + SHIFTED        # ALL_Q + SHIFTED of tests/test_gpu_epilogue_exact.py
IMAGE_LAYOUTS = ("contig", "channels_last", "hslice", "wslice")
IMAGE_FILL = 77.25                          # what the storage around a sliced view holds: never an image value
IMAGE_SLACK = 32                            # bytes the consumer over-reads: allocated by the caller, never written


@dataclass(frozen=True)
class ImageCase:
    cid: str
    n: int
    c: int
    h: int
    w: int
    pad: int
    layout: str
    route: str                              # "x4": four pixels per thread; "pixel"
    twin: str = ""                          # the case with the same logical image on the other route


def _image_cases():
    out = []
    for c in (1, 2, 3, 4):
        cl = "x4" if c == 1 else "pixel"    # channels_last: unit pixel stride only for one channel
        out += [
            ImageCase(f"c{c}_w4_one_group", 1, c, 3, 4, 1, "contig", "x4", f"c{c}_w4_wslice"),
            ImageCase(f"c{c}_w4_wslice", 1, c, 3, 4, 1, "wslice", "pixel", f"c{c}_w4_one_group"),
            ImageCase(f"c{c}_w8_pad3", 3, c, 5, 8, 3, "contig", "x4", f"c{c}_w8_wslice"),
            ImageCase(f"c{c}_w8_wslice", 3, c, 5, 8, 3, "wslice", "pixel", f"c{c}_w8_pad3"),
            ImageCase(f"c{c}_w20_pad0", 1, c, 4, 20, 0, "contig", "x4"),
            ImageCase(f"c{c}_w5", 3, c, 3, 5, 1, "contig", "pixel"),
            ImageCase(f"c{c}_w18", 1, c, 2, 18, 3, "contig", "pixel"),
            ImageCase(f"c{c}_w8_cl", 3, c, 4, 8, 1, "channels_last", cl),
            ImageCase(f"c{c}_w5_cl_pad0", 1, c, 3, 5, 0, "channels_last", "pixel"),
            ImageCase(f"c{c}_w8_hslice", 1, c, 5, 8, 3, "hslice", "x4"),
            ImageCase(f"c{c}_w4_wslice_pad0", 3, c, 3, 4, 0, "wslice", "pixel"),
        ]
    return out


IMAGE_CASES = {c.cid: c for c in _image_cases()}
CORNER_TIES = (0.5, -0.5, 1.5, 2.5, -1.5, 3.5)


def corner_pixels(h, w):
    return ((0, 0), (0, w - 1), (h - 1, 0), (h - 1, w - 1))


def edge_image(seed, n, c, h, w):
    """fp32 image: multiples of 1/2 (exact ties at scales 1 and 0.5), exact_layers.EDGE_VALUES at random positions, and at the four corner
    pixels of every channel alternately a tie and an edge value."""
    gg = torch.Generator().manual_seed(8800 + seed)
    img = torch.randint(-8, 9, (n, c, h, w), generator=gg).float() * 0.5
    ev = torch.tensor(X.EDGE_VALUES, dtype=torch.float32)
    flat = img.view(-1)
    cnt = min(flat.numel() // 2, 4 * len(ev))
    pos = torch.randperm(flat.numel(), generator=gg)[:cnt]
    flat[pos] = ev[(torch.arange(cnt) + 5 * seed) % len(ev)]
    i = seed
    for b in range(n):
        for ch in range(c):
            for (y, x) in corner_pixels(h, w):
                img[b, ch, y, x] = CORNER_TIES[i % len(CORNER_TIES)] if i % 2 else float(ev[(i // 2) % len(ev)])
                i += 1
    img[0, 0, 0, 1] = float("nan")          # (every image holds a NaN, whatever its size; W >= 4: no corner)
    return img


def image_of(case):
    return edge_image(sorted(IMAGE_CASES).index(case.cid if case.route == "x4" or not case.twin else case.twin), case.n, case.c, case.h, case.w)


def embed(img, layout):
    """(storage, view): `view(storage)` is the (N, C, H, W) image in the layout's strides - applied to the CPU storage and to its device copy."""
    n, c, h, w = img.shape
    if layout == "contig":
        return img.clone(), lambda t: t
    if layout == "channels_last":
        return img.permute(0, 2, 3, 1).contiguous(), lambda t: t.permute(0, 3, 1, 2)
    if layout == "hslice":                  # rows 2 .. 2 + H of a taller tensor
        st = torch.full((n, c, h + 3, w), IMAGE_FILL)
        st[:, :, 2:2 + h] = img
        return st, lambda t: t[:, :, 2:2 + h]
    assert layout == "wslice"               # columns 1 .. 1 + W of a wider tensor: the base is 4 bytes past a 16-byte boundary
    st = torch.full((n, c, h, w + 4), IMAGE_FILL)
    st[..., 1:1 + w] = img
    return st, lambda t: t[..., 1:1 + w]


def image_route(c, w, strides, base_mod16):
    """The host's condition (dlmcq_quantize_pad_nhwc4), restated: four pixels per thread when W % 4 == 0, the pixel stride is 1, the row and
    image (and, for C > 1, channel) strides are multiples of 4 elements and the base is 16-byte aligned."""
    sn, sc, sh, sw = strides
    return "x4" if (w % 4 == 0 and sw == 1 and sh % 4 == 0 and sn % 4 == 0 and (c == 1 or sc % 4 == 0) and base_mod16 == 0) else "pixel"


def border_byte(q, code0):
    """include/dlmcq.h: the border holds the code of x' = 0; under DLMCQ_PAD_CODE0 code 0 - the byte 0x80 with DLMCQ_EMIT_SHIFT128."""
    if code0:
        return 0x80 if q.shift128 else 0
    return int(X.quantise(torch.zeros(1), q).view(torch.uint8))


def padded_nhwc(img, pad):
    return F.pad(img, (pad, pad, pad, pad), value=0.0).permute(0, 2, 3, 1).contiguous()


def image_expected(img, pad, q, code0, codes=None):
    """uint8 [N, Hp, Wp, 4].  `codes`: the quantiser's bytes of padded_nhwc(img, pad) (default: exact_layers.quantise)."""
    n, c, h, w = img.shape
    codes = X.quantise(padded_nhwc(img, pad), q) if codes is None else codes
    out = torch.zeros((n, h + 2 * pad, w + 2 * pad, 4), dtype=torch.uint8)
    out[..., :c] = codes.view(torch.uint8)
    border = torch.ones((h + 2 * pad, w + 2 * pad), dtype=torch.bool)
    border[pad:pad + h, pad:pad + w] = False
    out[:, border, :] = border_byte(q, code0)
    return out


# ------------------------------------------------------------------------------------------------ max-pool on codes
@dataclass(frozen=True)
class PoolCase:
    cid: str
    n: int
    c: int
    h: int
    w: int
    k: int
    s: int
    p: int
    offset: int = 0                         # byte offset of both views into their allocations: 4 takes the one-dword route
    why: str = ""

    @property
    def pq(self):
        return (self.h + 2 * self.p - self.k) // self.s + 1, (self.w + 2 * self.p - self.k) // self.s + 1

    @property
    def route(self):
        """The host's condition restated: 16 channels per thread when C % 16 == 0 and both pointers are 16-byte aligned."""
        return "vec" if self.c % 16 == 0 and self.offset % 16 == 0 else "dword"


POOL_CASES = {c.cid: c for c in (
    PoolCase("c4", 2, 4, 5, 6, 3, 3, 1, why="one dword per pixel"),
    PoolCase("p1q1", 1, 16, 7, 7, 7, 7, 0, why="P = Q = 1; the vector route with one vector per pixel"),
    PoolCase("pad_half", 2, 16, 6, 5, 2, 2, 1, why="2 pad == kernel"),
    PoolCase("c20", 2, 20, 9, 11, 3, 2, 1, why="C % 16 != 0"),
    PoolCase("k1", 1, 64, 8, 8, 1, 1, 0, why="the identity"),
    PoolCase("k5s1", 3, 32, 7, 9, 5, 1, 2, why="overlapping windows"),
    PoolCase("resnet", 2, 64, 14, 14, 3, 2, 1, why="the plan's pool"),
    PoolCase("p1q1_off4", 1, 16, 7, 7, 7, 7, 0, 4, why="C = 16 on 4-byte aligned views"),
    PoolCase("pad_half_off4", 2, 16, 6, 5, 2, 2, 1, 4, why="C = 16 on 4-byte aligned views"),
    PoolCase("k1_off4", 1, 64, 8, 8, 1, 1, 0, 4, why="C = 64 on 4-byte aligned views"),
    PoolCase("resnet_off4", 2, 64, 14, 14, 3, 2, 1, 4, why="C = 64 on 4-byte aligned views"),
)}
POOL_CONTENTS = ("bytes", "minimum", "corners")
POOL_REFUSALS = (
    # what, (N, H, W, C, kernel, stride, pad), byte offset of the views, return code
    ("C % 4 != 0", (1, 6, 6, 6, 3, 2, 1), 0, EINVAL),
    ("2 pad > kernel", (1, 6, 6, 8, 3, 2, 2), 0, EINVAL),
    ("pooled size < 1", (1, 2, 6, 8, 5, 1, 0), 0, EINVAL),
    ("2-byte aligned", (1, 6, 6, 8, 3, 2, 1), 2, EALIGN),
)


def pool_codes(case, content, unsigned):
    """NHWC bytes (uint8 or int8) [N, H, W, C]."""
    gg = torch.Generator().manual_seed(6600 + sorted(POOL_CASES).index(case.cid))
    dt = torch.uint8 if unsigned else torch.int8
    lowest = 0 if unsigned else -128
    shape = (case.n, case.h, case.w, case.c)
    numel = int(np.prod(shape))
    if content == "bytes":                  # every byte value, in random order
        v = (torch.arange(numel) % 256)[torch.randperm(numel, generator=gg)] + lowest
        return v.reshape(shape).to(dt)
    x = torch.full(shape, lowest, dtype=torch.int64)
    if content == "corners":                # the minimum everywhere but single maxima in the four corners of every channel
        for i, (y, xx) in enumerate(corner_pixels(case.h, case.w)):
            x[:, y, xx, :] = lowest + 1 + (torch.arange(case.n)[:, None] * 7 + torch.arange(case.c)[None, :] * 4 + i) % 255
    return x.to(dt)


def pool_expected(codes, case):
    """F.max_pool2d of the codes as float64 (integers: exact), NHWC bytes [N, P, Q, C] in the input's dtype."""
    y = F.max_pool2d(codes.permute(0, 3, 1, 2).double(), case.k, case.s, case.p)
    return y.permute(0, 2, 3, 1).contiguous().to(torch.int64).to(codes.dtype)


def windows_covering(size, k, s, p, at):
    """How many pooling windows along one axis cover coordinate `at`."""
    n_out = (size + 2 * p - k) // s + 1
    return sum(1 for o in range(n_out) if o * s - p <= at <= o * s - p + k - 1)


# ------------------------------------------------------------------------------------------------ pack / unpack
PACK_N = (1, 2, 15, 16, 17, 31, 32, 33, 4111)
CODE_OFFSETS, PACKED_OFFSETS = (0, 1, 4, 15), (0, 1, 4)


def nibble_codes(n, signed, seed=0):
    """int8 [n]: all 16 values of the range (-8 .. 7 or 0 .. 15), the first 16 in order, then shuffled."""
    gg = torch.Generator().manual_seed(5500 + seed)
    v = torch.arange(n) % 16
    if n > 16:
        v[16:] = v[16:][torch.randperm(n - 16, generator=gg)]
    return (v - 8 if signed else v).to(torch.int8)


def pack_expected(codes):
    c = torch.cat([codes.to(torch.int16) & 15, torch.zeros(codes.numel() % 2, dtype=torch.int16)])
    return (c[0::2] | (c[1::2] << 4)).to(torch.uint8)


def unpack_expected(packed, n, signed):
    v = torch.stack([packed & 15, packed >> 4], dim=1).reshape(-1)[:n].to(torch.int8)
    return (v ^ 8) - 8 if signed else v


# ------------------------------------------------------------------------------------------------ the dw+pw constant table
TABLE_C = (64, 128, 320)
TABLE_VARIANTS = (
    # bias, w_offset, x_unsigned, zero point
    (True, True, True, 131.0),
    (True, False, True, 77.0),
    (False, True, False, -37.0),
    (False, False, False, 5.0),
    (True, True, False, None),
)
TABLE_REFUSALS = (("C = 32", 32, 0, EINVAL), ("C = 96", 96, 0, EINVAL), ("table 8-byte aligned", 64, 8, EALIGN))
BIAS_BITS = (0x80000000, 0x7fc00000, 0xffc00000, 0x7f800000, 0xff800000)      # -0, NaN, -NaN, +inf, -inf


def table_slot(c):
    """The record of channel c: chunk c >> 6, slot (c & 15) * 4 + ((c >> 4) & 3)."""
    return c >> 6, (c & 15) * 4 + ((c >> 4) & 3)


def table_operands(c, seed):
    """w int8 [3, 3, C] over all of -128 .. 127, per-channel scales / offsets that are no powers of two, a bias with BIAS_BITS, s_in."""
    gg = torch.Generator().manual_seed(4400 + seed)
    w = torch.randint(-128, 128, (3, 3, c), generator=gg).to(torch.int8)
    w[:, :, 1], w[:, :, 2] = 127, -128                              # the code sums 9 * 127 and 9 * -128
    free = (torch.arange(9 * c) % c >= 3).nonzero().flatten()[:256]
    w.view(-1)[free] = (torch.arange(256) - 128).to(torch.int8)[torch.randperm(256, generator=gg)]
    s_w = (torch.rand(c, generator=gg) * 0.01 + 1e-3).float()
    o_w = torch.randn(c, generator=gg).float()
    bias = torch.randn(c, generator=gg).float()
    bias.view(torch.int32)[3:3 + len(BIAS_BITS)] = torch.tensor(BIAS_BITS, dtype=torch.int64).to(torch.int32)
    return w, s_w, o_w, bias, torch.tensor([0.0371], dtype=torch.float32)


def table_expected(w, bias, s_in, zp, s_w, o_w, unsigned):
    """int32 [C / 64, 64, 8]: {taps 0-3, taps 4-7, tap 8 as signed bytes, (shift - zp) SUM w, fl32(s_in s_w), fl32(s_in o_w) or 0, bias or 0, 0}
    - the record above dwpw_pack_table_kernel; shift = 128 for uint8 codes (they reach the matrix cores as code - 128), 0 for int8."""
    c = w.shape[2]
    wn = w.reshape(9, c).numpy()
    rec = np.zeros((c // 64, 64, 8), dtype=np.uint32)
    taps = np.zeros((12, c), dtype=np.uint32)
    taps[:9] = wn.astype(np.int32) & 0xff
    sin = s_in.numpy().astype(np.float32)[0]
    dz = (128 if unsigned else 0) - int(0.0 if zp is None else zp)
    for ch in range(c):
        chunk, slot = table_slot(ch)
        r = rec[chunk, slot]
        for d in range(3):
            r[d] = taps[4 * d, ch] | (taps[4 * d + 1, ch] << 8) | (taps[4 * d + 2, ch] << 16) | (taps[4 * d + 3, ch] << 24)
        r[3] = np.int64(dz * int(wn[:, ch].astype(np.int64).sum())) & 0xffffffff
        r[4] = (sin * s_w.numpy()[ch:ch + 1]).astype(np.float32).view(np.uint32)[0]
        r[5] = 0 if o_w is None else (sin * o_w.numpy()[ch:ch + 1]).astype(np.float32).view(np.uint32)[0]
        r[6] = 0 if bias is None else bias.numpy()[ch:ch + 1].view(np.uint32)[0]
    return torch.from_numpy(rec.view(np.int32))


# ------------------------------------------------------------------------------------------------ the grid caps
GRID_CAP = {
    # pack_grid: at most DLMCQ_CUS * 16 blocks of DLMCQ_BLOCK threads, 16 codes per thread and trip
    "pack": dict(n=(1 << 24) + 4096 + 5),
    # dlmcq_quantize_pad_nhwc4 (pixel route) and dlmcq_maxpool_codes_nhwc: at most 65536 blocks, one pixel / one dword per thread and trip
    "image": dict(n=1, c=1, h=4097, w=4099, pad=0),
    "pool": dict(n=1, c=4, h=4097, w=4099, k=1, s=1, p=0),
}


def big_image(h, w):
    """The grid-cap image: multiples of 1/2 in +-130 (ties and both clamp ends at scale 1), built without a permutation."""
    gg = torch.Generator().manual_seed(3300)
    return torch.randint(-260, 261, (1, 1, h, w), generator=gg, dtype=torch.int16).float() * 0.5
