"""The calls that reach every instantiation of the depthwise kernels - csrc/conv_dw_i8.hip (DW_TABLE, 26: conv_dw3p2_i8_kernel and
conv_dw3_i8_kernel in FAST 0 / 1 / 2 x R6 x XOFF, conv_dw_i8_kernel in R6), csrc/conv_dwm_i8.hip (DWM_TABLE, 8: HPW 4 / 5 x XS x R6) and
csrc/conv_dwpw_i8.hip (DWPW_TABLE, 6: K 128 / 192 / 512 x HPW 2 / 3): ONE table for tests/test_dw_variants_host.py (which record does the
dispatch pick: DLMCQ_ROUTE_ONLY | DLMCQ_ROUTE_DW_VARIANT on placeholder pointers, no GPU) and tests/test_gpu_dw_variants.py (the same calls
launched and compared with an exact float64 reference).  TEST INFRASTRUCTURE ONLY.

A record is ("dw", family, FAST, R6, XOFF), ("dwm", halo pieces per wave, XS, R6) or ("dwpw", K, halo pieces per wave), as
dlmc._native.decode_dw_variant answers the first two.  dlmcq_conv2d_dwpw_i8_nhwc takes no route query: its record is a function of K and W alone
(dwpw_launch: hp = ceil((64 + 2 (W + 1) + 2) / 16) halo pieces, 2 per wave up to W = 30, 3 up to W = 61), so those six are reached by shape and
the host test proves the formula for each case.

Every family has a list of geometries below, the smallest that exercise what its kernel can get wrong; a record's cases walk that list
(starting at a different place for every record) and vary, by case index i,
  * the input codes and zero point: uint8 with zero point 0 (i = 0: the FAST kernels' out-of-range buffer loads), uint8 with a zero point
    above 128 (1), int8 with a zero point that is not 0 (2), uint8 below 128 (3), int8 with zero point 0 (4); XS records of the matrix-core
    kernel take the int8 ones only, its other records the uint8 ones;
  * the quantiser (tests/test_gpu_halo_variants.py: QUANTS): FAST 1 / 2 and dwm records the plain ones, FAST 0 and generic records the ones with
    a zero point or a signed range, codes only, with the fp32 output, and the fp32 output alone; case 0 of every record at the consumer scale
    2^-5, where the upper clamp occurs;
  * the activation: ReLU6 in every case of an R6 record, else ReLU and none in turn; a null bias in case 1; symmetric and asymmetric weights
    in turn where FAST does not fix them.
The two grid-stride cases (more than 4096 x 256 work items: a thread runs a second, shorter pass) and the two matrix-core cases whose
workgroups own unequal numbers of tiles (sized from the device's CU count: `Case.geo_for`) ride on one record each."""
from dataclasses import dataclass, field
from typing import Optional

import test_dw_stem_refusals_host as D

from dlmc._native import FORCE_TILED, ROUTE_DW_VARIANT, ROUTE_ONLY, decode_dw_variant      # include/dlmcq.h

DWM_TP, DWPW_TP = 192, 64          # frame positions per tile (csrc/conv_dwm_i8.hip, csrc/conv_dwpw_i8.hip)

# THE 26 + 8 + 6 records, by hand: the launchers' tables must hold exactly these (an instantiation dropped or added is a diff here)
DW_RECORDS = [
    ("dw", "p2", 0, False, False), ("dw", "p2", 1, False, False), ("dw", "p2", 2, False, False),
    ("dw", "p2", 0, True, False), ("dw", "p2", 1, True, False), ("dw", "p2", 2, True, False),
    ("dw", "p2", 0, False, True), ("dw", "p2", 1, False, True), ("dw", "p2", 2, False, True),
    ("dw", "p2", 0, True, True), ("dw", "p2", 1, True, True), ("dw", "p2", 2, True, True),
    ("dw", "dw3", 0, False, False), ("dw", "dw3", 1, False, False), ("dw", "dw3", 2, False, False),
    ("dw", "dw3", 0, True, False), ("dw", "dw3", 1, True, False), ("dw", "dw3", 2, True, False),
    ("dw", "dw3", 0, False, True), ("dw", "dw3", 1, False, True), ("dw", "dw3", 2, False, True),
    ("dw", "dw3", 0, True, True), ("dw", "dw3", 1, True, True), ("dw", "dw3", 2, True, True),
    ("dw", "generic", 0, False, False), ("dw", "generic", 0, True, False),
]
DWM_RECORDS = [
    ("dwm", 4, False, False), ("dwm", 4, True, False), ("dwm", 4, False, True), ("dwm", 4, True, True),
    ("dwm", 5, False, False), ("dwm", 5, True, False), ("dwm", 5, False, True), ("dwm", 5, True, True),
]
DWPW_RECORDS = [("dwpw", 128, 2), ("dwpw", 128, 3), ("dwpw", 192, 2), ("dwpw", 192, 3), ("dwpw", 512, 2), ("dwpw", 512, 3)]
RECORDS = DW_RECORDS + DWM_RECORDS + DWPW_RECORDS
assert len(DW_RECORDS) == len(set(DW_RECORDS)) == 26 and len(DWM_RECORDS) == len(set(DWM_RECORDS)) == 8
assert len(DWPW_RECORDS) == len(set(DWPW_RECORDS)) == 6


def record_name(r):
    if r[0] == "dwm":
        return f"dwm_hpw{r[1]}" + ("_xs" if r[2] else "") + ("_r6" if r[3] else "")
    if r[0] == "dwpw":
        return f"dwpw_k{r[1]}_hpw{r[2]}"
    return f"{r[1]}_fast{r[2]}" + ("_r6" if r[3] else "") + ("_xoff" if r[4] else "")


def decode(rc):
    """A ROUTE_ONLY | ROUTE_DW_VARIANT answer -> the record, or the integer itself when it names no depthwise instantiation."""
    r = decode_dw_variant(rc)
    return rc if r is None else r


def dwm_pieces(w):
    """Halo pieces of 16 frame positions a tile needs (conv_dwm_launch): 4 per wave up to 16 pieces (W <= 30), 5 up to 20 (W <= 62)."""
    return (DWM_TP + 2 * (w + 1) + 2 + 15) // 16


def dwm_groups(cus, nchunks):
    """Workgroup groups conv_dwm_launch starts before it caps them at the tile count."""
    return max(((3 * cus) // nchunks) & ~7, 8)


def dwpw_pieces(w):
    return (DWPW_TP + 2 * (w + 1) + 2 + 15) // 16


@dataclass(frozen=True)
class Case:
    cid: str
    record: tuple
    geo: dict = field(hash=False, compare=False)      # N H W C R S stride pad (N: None = sized from the CU count - geo_for)
    uns: bool = True              # uint8 input codes, else int8
    zp: int = 0                   # the input zero point
    asym: bool = False            # per-channel weight offsets
    act: int = 1                  # DLMCQ_ACT_*
    quant: Optional[str] = "plain"      # tests/test_gpu_halo_variants.py: QUANTS; None: the fp32 output alone
    out: bool = False             # the fp32 output is wanted
    bias: bool = True             # False: a null bias - under a float offset, whose folded term rides in the bias, a bias of that term alone
    force: bool = False           # DLMCQ_FORCE_TILED: a layer the matrix-core kernel would take, on the vector kernels
    seed: int = 0
    # dwpw only: the pointwise layer and the quantiser between the two
    k: int = 0
    q1: str = ""                  # Q1 below
    asym2: bool = False
    dw_relu: int = 1

    @property
    def xoff(self):
        return self.record[0] == "dw" and self.record[4]

    @property
    def entry(self):
        return "dwpw_i8_nhwc" if self.record[0] == "dwpw" else "dw_i8_nhwc_xoff" if self.xoff else "dw_i8_nhwc"

    def geo_for(self, cus=256):
        g = dict(self.geo)
        if g["N"] is None:        # the matrix-core kernel: about one and a half tiles per workgroup group, never a whole number
            groups = dwm_groups(cus, g["C"] // 64)
            fs = (g["H"] + 1) * (g["W"] + 1)
            g["N"] = (3 * groups * DWM_TP // 2) // fs + 1
        return g

    def out_hw(self):
        g = self.geo
        return (g["H"] + 2 * g["pad"] - g["R"]) // g["stride"] + 1, (g["W"] + 2 * g["pad"] - g["S"]) // g["stride"] + 1

    def route_args(self, ptr=None, cus=256):
        """Overrides of D.BASE[self.entry] for the route query (`ptr` maps an argument name to a real address; placeholders otherwise)."""
        assert self.record[0] != "dwpw"
        p = (lambda name: D.P) if ptr is None else ptr
        a = dict(self.geo_for(cus))
        a.update(uns=int(self.uns), relu=self.act, x=p("x"), w=p("w"), s_in=p("s_in"), s_w=p("s_w"), zp_in=p("zp_in"),
                 out=p("out") if self.out else 0, bias=p("bias") if self.bias or self.xoff else 0, w_off=p("w_off") if self.asym else 0,
                 codes=p("codes") if self.quant else 0, q_scale=p("q_scale") if self.quant else 0, q_zp=0, q_lo=0, q_hi=255,
                 q_form=D.ZP | ROUTE_ONLY | ROUTE_DW_VARIANT | (FORCE_TILED if self.force else 0))
        if self.quant and self.quant.startswith("signed"):
            a.update(q_zp=p("q_zp"), q_lo=-128, q_hi=127)
        elif self.quant and self.quant.startswith("uzp"):
            a.update(q_zp=p("q_zp"))
        if self.xoff:
            a.update(x_off=p("x_off"), x_tap=p("x_tap"))
        return a


def _geo(n, h, w, c, r=3, s=None, stride=1, pad=1):
    return dict(N=n, H=h, W=w, C=c, R=r, S=r if s is None else s, stride=stride, pad=pad)


# conv_dw3p2_i8_kernel (3x3 / 1 / 1, C % 16 == 0, C <= 1024): odd Q (the unpaired last pixel) on three channel groups, even Q, W = 1, H = 1,
# C = 1024; N >= 2 (threads straddle image seams); all below 4096 pixels, so the matrix-core kernel declines the plain codes-only ones
P2_GEOS = [_geo(2, 5, 7, 48), _geo(3, 4, 6, 16), _geo(4, 9, 1, 16), _geo(4, 1, 15, 32), _geo(2, 3, 3, 1024)]
P2_GRID_STRIDE = _geo(9, 61, 60, 1024)        # 9 x 61 x 30 pairs x 64 groups = 1 054 080 > 4096 x 256 threads; DLMCQ_FORCE_TILED (dwm would take it)
# conv_dw3_i8_kernel: stride 2 / pad 1 on an odd height and an even width, C = 1040 at 1 / 1 (above P2's limit), C = 2048 on a 3x3 image
# (the widest taken: a 64 KB LDS table in the FAST 0 form) - and, without padding (no float offset term: not for the XOFF records),
# stride 1 / pad 0 and stride 2 / pad 0
DW3_PADDED = [_geo(2, 7, 8, 32, stride=2), _geo(2, 3, 4, 1040), _geo(2, 3, 3, 2048)]
DW3_UNPADDED = [_geo(2, 5, 6, 16, pad=0), _geo(2, 7, 9, 48, stride=2, pad=0)]
DW3_GRID_STRIDE = _geo(5, 59, 60, 1024, pad=0)      # 5 x 57 x 58 pixels x 64 groups = 1 057 920 > 4096 x 256
# conv_dw_i8_kernel: C % 16 != 0 (12 and 84), 5x5 / pad 2, 7x7 / 2 / 3, 1x1, a rectangular 3x5 filter, more padding than the filter needs
GENERIC_GEOS = [_geo(2, 6, 7, 12, 5, pad=2), _geo(2, 9, 10, 84, 7, stride=2, pad=3), _geo(3, 4, 5, 20, 1, pad=0), _geo(2, 5, 8, 12, 3, 5),
                _geo(2, 4, 4, 84, pad=3)]
# conv_dwm_i8_kernel (N H W >= 4096, C % 64 == 0, 14 <= W <= 62): W = 14 (just above 4096 pixels) and W = 30 (odd H, C = 192) take 4 halo
# pieces per wave, W = 31 and W = 62 five; every frame N (H + 1)(W + 1) ends in a partial tile of 192 positions
DWM_GEOS = {4: [_geo(21, 14, 14, 64), _geo(5, 29, 30, 192)], 5: [_geo(7, 19, 31, 64), _geo(3, 23, 62, 192)]}
DWM_UNEQUAL = {4: _geo(None, 14, 14, 64), 5: _geo(None, 19, 31, 64)}     # N from the CU count: workgroups own one or two tiles
# conv_dwpw_i8_kernel (C % 64 == 0, W <= 61): W = 30 / W = 31 either side of the piece boundary, W = 61 the widest; an image smaller than
# a 64-position tile (4 x 5 frame positions); C = 64 and 128; tiles cross images and the last one is partial
DWPW_GEOS = {2: [_geo(2, 5, 30, 64), _geo(5, 3, 4, 128)], 3: [_geo(3, 4, 31, 64), _geo(2, 3, 61, 128)]}
Q1 = ("q1_plain", "q1_zp", "q1_sym", "q1_zp128")      # tests/test_gpu_dw_variants.py: Q1S

_INPUT = ((True, 0), (True, 200), (False, -37), (True, 77), (False, 0))       # (uint8 codes, zero point) by case index
_INPUT_XS = {True: ((False, 0), (False, -37), (False, 64), (False, 0)), False: ((True, 0), (True, 200), (True, 77), (True, 131))}
_PLAIN = ("plain_hi", "plain", "plain_hi", "plain_hi", "plain")
# FAST 0 / generic: (quantiser, fp32 output wanted) - a plain quantiser reaches FAST 0 only next to an fp32 output
_OPEN = (("uzp_hi", False), ("signed", True), (None, True), ("plain_hi", True), ("signed_hi", False))


def _act(r6, i):
    return 2 if r6 else (1, 0)[i % 2]


def cases():
    out = []
    for ri, r in enumerate(DW_RECORDS):
        _, family, fast, r6, xoff = r
        geos = {"p2": P2_GEOS, "dw3": DW3_PADDED if xoff else DW3_PADDED + DW3_UNPADDED, "generic": GENERIC_GEOS}[family]
        count = len(geos) if family == "generic" else 3
        for i in range(count):
            uns, zp = _INPUT[i]
            quant, want_out = (_PLAIN[i], False) if fast else _OPEN[i]
            out.append(Case(f"{record_name(r)}/{i}", r, geos[(ri + i) % len(geos)], uns, zp, asym=(fast == 1) or (fast == 0 and i % 2 == 0),
                            act=_act(r6, i), quant=quant, out=want_out, bias=i != 1, seed=100 * ri + i))
    # the grid-stride cases: on the symmetric FAST records (the workload's own), plain quantiser, ReLU
    out.append(Case("p2_fast2/grid_stride", ("dw", "p2", 2, False, False), P2_GRID_STRIDE, True, 0, quant="plain", force=True, seed=7001))
    out.append(Case("dw3_fast2/grid_stride", ("dw", "dw3", 2, False, False), DW3_GRID_STRIDE, True, 200, quant="plain", seed=7002))
    for ri, r in enumerate(DWM_RECORDS):
        _, hpw, xs, r6 = r
        for i, geo in enumerate(DWM_GEOS[hpw]):
            uns, zp = _INPUT_XS[xs][i + 2 * ((ri // 2) % 2)]
            out.append(Case(f"{record_name(r)}/{i}", r, geo, uns, zp, asym=i % 2 == 0, act=_act(r6, i), quant=_PLAIN[i], bias=i != 1, seed=3000 + 100 * ri + i))
    for hpw in (4, 5):
        out.append(Case(f"dwm_hpw{hpw}/unequal_tiles", ("dwm", hpw, False, False), DWM_UNEQUAL[hpw], True, 131, asym=hpw == 5, quant="plain",
                        seed=7100 + hpw))
    for ri, r in enumerate(DWPW_RECORDS):
        _, k, hpw = r
        for i, geo in enumerate(DWPW_GEOS[hpw]):
            uns, zp = _INPUT[(ri + i) % len(_INPUT)]
            out.append(Case(f"{record_name(r)}/{i}", r, geo, uns, zp, asym=i == 1, act=(1, 0)[(ri // 2 + i) % 2], quant=("uzp_hi", "plain_hi", "signed_hi")[(ri + i) % 3],
                            bias=not (i == 1 and ri % 2), seed=5000 + 100 * ri + i, k=k, q1=Q1[(ri + 2 * i) % 4], asym2=i == 0, dw_relu=1 - i))
    return out


CASES = cases()
BY_RECORD = {r: [c for c in CASES if c.record == r] for r in RECORDS}
