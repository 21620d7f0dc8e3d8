"""The calls that reach every instantiation of the first-layer kernels - csrc/conv_stem_i8.hip (STEM_TABLE, 40: conv_stem_i8_kernel R 1 .. 7 x
ASYM x R6, the SWAP quad of R = 3, the XOFF quads of R = 3 and 7; STEM_POOL_TABLE, 7: conv_stem_pool_i8_kernel R 1 .. 7) and
csrc/conv_stem_pool7_i8.hip (2: XS) -, of the pointwise kernel - csrc/conv_pw_i8.hip (36: the nine DLMCQ_PW_PAIRS x ASYM x R6) - and of the
block-end kernel - csrc/conv_pwr_i8.hip (8: C 256 / 512 x {codes, fp32 + codes, fp32 alone}, the dual form with either pair first): ONE table
for tests/test_stem_pw_variants_host.py (which record does the dispatch pick: DLMCQ_ROUTE_ONLY | DLMCQ_ROUTE_PW_VARIANT on placeholder
pointers, no GPU) and tests/test_gpu_stem_pw_variants.py (the same calls launched and compared with an exact float64 reference).
TEST INFRASTRUCTURE ONLY.

A record is what dlmc._native.decode_stem_variant / decode_pw_variant answer: ("stem", R, ASYM, SWAP, R6, XOFF), ("pool", R), ("pool7", XS),
("pw", C, slice, ASYM, R6), ("pwr", C, OUTF, CODES, DUAL, SWP).  Every record has three calls, a ReLU6 twin its sibling's first two.

First layer (one wave = a tile of 32 output pixels x 64 channels, 4 tiles per workgroup, blockIdx.y = the slab of 64 channels): N = 3 images
whose P Q is no multiple of 32 (a partial last tile, image seams inside tiles); K = 64, K = 128 (a second slab: constants at n0 = 64), K = 72
(col < K inside the second slab; not for SWAP, which needs K % 64 == 0); S != R (S = 8 for R = 7, S = 1 for R >= 2, S = 3 for R = 1); strides
1 and 2; C = 1 .. 4 real channels on the asymmetric entry point (the padding channels of the NHWC4 buffer hold random bytes there: the
weights are zero on them and the code sum masks them); uint8 codes with a zero point either side of 128 and int8 codes; XOFF with pad 1 / 3
(pad 0 answers the plain record: FALLBACKS); SWAP needs 16-byte-aligned codes (4 bytes off answers the unswapped record: FALLBACKS).
Pooled first layer (a workgroup = 3 x 8 pooled pixels): odd and even P, Q, P = 1, K = 64 and below, fp32 + codes and codes alone; R = 7 /
stride 2 / K = 64 / codes only with an odd P stays on conv_stem_pool_i8_kernel.  conv_stem_pool7_i8_kernel (bands of 14 pooled rows, x tiles
of 31 pooled columns, 4 tasks per workgroup): PP = 15 and QP = 32 cross one band and one x tile, N = 3 gives 12 tasks, N = 1 with one band 2.
Pointwise (M >= 4096, blocks of 32 pixels, slices of 64 / 128 / 192 channels): M = 2 x 46 x 46 = 4232 = 132 blocks + 8 rows (the last block
is a quarter full); per pair one slice, two slices (the second reads its constants at n0 != 0) and K = 1024, the bound (K = 384 on the
512- and 1024-deep pairs, K = 64 / 192 alone where the slice is the layer); both input types, a null bias and DLMCQ_EMIT_SHIFT128 once per pair.
Block end (M >= 4096, M % 32 == 0, slices of 128): M = 4096 and 4608, K = 128 and 256, row-major and chunk-major fp32 tensors, K = 4096 once on
C = 256 (32 slices: 8 groups of workgroups, waves own unequal numbers of blocks); the dual form in both orders at strides 1 and 2.
Waves that loop (`Case.geo_for`: N sized from the device's CU count, one case per kernel template): some wave owns 3 blocks / tiles, another 2."""
from dataclasses import dataclass, field
from typing import Optional

import test_conv_dispatch_host as T
import test_dw_stem_refusals_host as D

from dlmc._native import (EMIT_SHIFT128, FP32_IN_CHUNK_MAJOR, FP32_OUT_CHUNK_MAJOR, ROUTE_ONLY, ROUTE_PW_VARIANT,      # include/dlmcq.h
                          decode_pw_variant, decode_stem_variant)

# THE 40 + 7 + 2 + 36 + 8 records, by hand: the launchers' tables must hold exactly these (an instantiation dropped or added is a diff here)
STEM_RECORDS = [
    ("stem", 1, False, False, False, False), ("stem", 1, True, False, False, False), ("stem", 1, False, False, True, False), ("stem", 1, True, False, True, False),
    ("stem", 2, False, False, False, False), ("stem", 2, True, False, False, False), ("stem", 2, False, False, True, False), ("stem", 2, True, False, True, False),
    ("stem", 3, False, False, False, False), ("stem", 3, True, False, False, False), ("stem", 3, False, False, True, False), ("stem", 3, True, False, True, False),
    ("stem", 4, False, False, False, False), ("stem", 4, True, False, False, False), ("stem", 4, False, False, True, False), ("stem", 4, True, False, True, False),
    ("stem", 5, False, False, False, False), ("stem", 5, True, False, False, False), ("stem", 5, False, False, True, False), ("stem", 5, True, False, True, False),
    ("stem", 6, False, False, False, False), ("stem", 6, True, False, False, False), ("stem", 6, False, False, True, False), ("stem", 6, True, False, True, False),
    ("stem", 7, False, False, False, False), ("stem", 7, True, False, False, False), ("stem", 7, False, False, True, False), ("stem", 7, True, False, True, False),
    ("stem", 3, False, True, False, False), ("stem", 3, True, True, False, False), ("stem", 3, False, True, True, False), ("stem", 3, True, True, True, False),
    ("stem", 3, False, False, False, True), ("stem", 3, True, False, False, True), ("stem", 3, False, False, True, True), ("stem", 3, True, False, True, True),
    ("stem", 7, False, False, False, True), ("stem", 7, True, False, False, True), ("stem", 7, False, False, True, True), ("stem", 7, True, False, True, True),
]
POOL_RECORDS = [("pool", 1), ("pool", 2), ("pool", 3), ("pool", 4), ("pool", 5), ("pool", 6), ("pool", 7)]
POOL7_RECORDS = [("pool7", False), ("pool7", True)]
PW_RECORDS = [
    ("pw", 64, 64, False, False), ("pw", 64, 64, True, False), ("pw", 64, 64, False, True), ("pw", 64, 64, True, True),
    ("pw", 64, 128, False, False), ("pw", 64, 128, True, False), ("pw", 64, 128, False, True), ("pw", 64, 128, True, True),
    ("pw", 64, 192, False, False), ("pw", 64, 192, True, False), ("pw", 64, 192, False, True), ("pw", 64, 192, True, True),
    ("pw", 128, 128, False, False), ("pw", 128, 128, True, False), ("pw", 128, 128, False, True), ("pw", 128, 128, True, True),
    ("pw", 128, 192, False, False), ("pw", 128, 192, True, False), ("pw", 128, 192, False, True), ("pw", 128, 192, True, True),
    ("pw", 192, 128, False, False), ("pw", 192, 128, True, False), ("pw", 192, 128, False, True), ("pw", 192, 128, True, True),
    ("pw", 192, 192, False, False), ("pw", 192, 192, True, False), ("pw", 192, 192, False, True), ("pw", 192, 192, True, True),
    ("pw", 512, 128, False, False), ("pw", 512, 128, True, False), ("pw", 512, 128, False, True), ("pw", 512, 128, True, True),
    ("pw", 1024, 128, False, False), ("pw", 1024, 128, True, False), ("pw", 1024, 128, False, True), ("pw", 1024, 128, True, True),
]
PWR_RECORDS = [
    ("pwr", 256, False, True, False, False), ("pwr", 256, True, True, False, False), ("pwr", 256, True, False, False, False),
    ("pwr", 512, False, True, False, False), ("pwr", 512, True, True, False, False), ("pwr", 512, True, False, False, False),
    ("pwr", 256, True, True, True, False), ("pwr", 256, True, True, True, True),
]
RECORDS = STEM_RECORDS + POOL_RECORDS + POOL7_RECORDS + PW_RECORDS + PWR_RECORDS
assert len(set(STEM_RECORDS)) == 40 and len(set(POOL_RECORDS)) == 7 and len(set(POOL7_RECORDS)) == 2 and len(set(PW_RECORDS)) == 36
assert len(set(PWR_RECORDS)) == 8 and len(RECORDS) == len(set(RECORDS)) == 93


def record_name(r):
    if r[0] == "stem":
        return f"stem_r{r[1]}" + "".join(t for f, t in zip(r[2:], ("_asym", "_swap", "_r6", "_xoff")) if f)
    if r[0] == "pool":
        return f"pool_r{r[1]}"
    if r[0] == "pool7":
        return "pool7" + ("_xs" if r[1] else "")
    if r[0] == "pw":
        return f"pw_{r[1]}_{r[2]}" + ("_asym" if r[3] else "") + ("_r6" if r[4] else "")
    return f"pwr_{r[1]}" + "".join(t for f, t in zip(r[2:], ("_out", "_codes", "_dual", "_swp")) if f)


def decode(rc):
    """A ROUTE_ONLY | ROUTE_PW_VARIANT answer -> the record, or the integer itself when it names none of these instantiations."""
    r = decode_stem_variant(rc) or decode_pw_variant(rc)
    return rc if r is None else r


# ---- the launchers' group formulas, restated (pw_go, pwr_go, stem_launch, the pooled entry point, stem_pool7_launch)
def pw_waves(c, bn):
    """(waves per workgroup, workgroups per CU) of pw_go<C, BN>."""
    wps = 1 if c >= 1024 else 3 if c >= 512 else 4
    lds1, stg = c * bn + 16 * bn, 4 * 32 * (bn + 16)
    big = c >= 1024 or (lds1 + stg) * wps > 158 * 1024
    return (6 if c >= 1024 else 4 * wps if big else 4), (1 if big else wps)


def pw_groups(cus, c, bn, k, nblk):
    nw, per_cu = pw_waves(c, bn)
    return min(max((cus * per_cu // (k // bn)) & ~7, 8), ((nblk + nw - 1) // nw + 7) & ~7), nw


def pwr_groups(cus, c, k, nblk, dual=False):
    nw = 6 if dual else 12 if c == 256 else 8
    return min(max((cus // (k // 128)) & ~7, 8), ((nblk + nw - 1) // nw + 7) & ~7), nw


def stem_workgroups(ntiles):
    return min((ntiles + 3) // 4, 2048)


POOL_WORKGROUPS = 1024      # conv_stem_pool_i8_kernel: persistent workgroups, one 3 x 8 pooled tile at a time


def _stem_geo(n, hp, wp, k, r, s, stride, c=4, pad=0):
    return dict(N=n, H=hp, W=wp, K=k, R=r, S=s, stride=stride, C=c, pad=pad)


def _pw_geo(n, h, w, c, k, **extra):
    return dict(N=n, H=h, W=w, C=c, K=k, R=1, S=1, stride=1, pad=0, dil=1, **extra)


@dataclass(frozen=True)
class Case:
    cid: str
    record: tuple
    entry: str                    # D.ENTRIES (first layer) or T.ENTRIES (pointwise, block end)
    geo: dict = field(hash=False, compare=False)      # N None: sized from the CU count (geo_for)
    uns: bool = True
    zp: Optional[int] = None      # the input zero point (None: make_full_range_layer's default for the type)
    act: int = 1                  # DLMCQ_ACT_*
    quant: Optional[str] = "plain"    # tests/test_gpu_stem_pw_variants.py: QUANTS; None: the fp32 output alone
    out: bool = False             # the fp32 output is wanted
    bias: bool = True
    res: bool = False             # an fp32 shortcut tensor
    cm: bool = False              # the call's fp32 tensors are chunk-major
    codes_off: int = 0            # bytes the codes pointer is moved off its 16-byte alignment (FALLBACKS)
    x_off: int = 0                # ... the operand pointer
    ref: Optional[str] = None     # the case whose operands and reference this one shares (a ReLU6 twin: its sibling's call)
    loops: Optional[str] = None   # the kernel template whose waves loop unequally in this case

    @property
    def family(self):
        return "stem" if self.record[0] in ("stem", "pool", "pool7") else self.record[0]

    @property
    def asym(self):
        return self.record[0] in ("stem", "pw") and bool(self.record[2] if self.record[0] == "stem" else self.record[3])

    @property
    def xoff(self):
        return self.entry == "i8_stem_xoff"

    def geo_for(self, cus=256):
        g = dict(self.geo)
        if g["N"] is None:
            if self.record[0] == "pw":          # 2.5 blocks per wave
                ngroups, nw = pw_groups(cus, g["C"], self.record[2], g["K"], 1 << 30)
                g["N"] = -(-(5 * ngroups * nw // 2) * 32 // (g["H"] * g["W"]))
            elif self.record[0] == "pwr":
                ngroups, nw = pwr_groups(cus, g["C"], g["K"], 1 << 30)
                g["N"] = (5 * ngroups * nw // 2) * 32 // (g["H"] * g["W"])
            elif self.record[0] == "pool":      # 2.5 pooled tiles per workgroup
                p, q = self.out_hw(g)
                tiles = -(-((p - 1) // 2 + 1) // 3) * -(-((q - 1) // 2 + 1) // 8)
                g["N"] = -(-(5 * POOL_WORKGROUPS // 2) // tiles)
            else:                               # conv_stem_i8_kernel: 2.5 tiles per wave of the capped grid
                p, q = self.out_hw(g)
                g["N"] = -(-(5 * stem_workgroups(1 << 30) * 4 // 2) * 32 // (p * q))
        return g

    @staticmethod
    def out_hw(g):
        return (g["H"] - g["R"]) // g["stride"] + 1, (g["W"] - g["S"]) // g["stride"] + 1

    def route_args(self, ptr=None, cus=256):
        """Overrides of the entry point's BASE for the route query (`ptr`: argument name -> real address; placeholders otherwise)."""
        real = ptr is not None
        p = (lambda name: T.P) if ptr is None else ptr
        g = self.geo_for(cus)
        codes = (p("codes") + self.codes_off) if self.quant else 0
        shift = EMIT_SHIFT128 if self.quant in ("shift", "shift6") else 0
        signed = self.quant in ("signed", "signed6")          # (first layer only: the other two families take the plain quantiser)
        if self.family == "stem":
            a = {k: v for k, v in g.items() if k in D.BASE[self.entry]}
            a.update(x=p("x") + self.x_off, w=p("w"), wsum=p("wsum"), s_in=p("s_in"), s_w=p("s_w"), zp_in=p("zp_in"), uns=int(self.uns), relu=self.act,
                     out=p("out") if self.out else 0, bias=p("bias") if self.bias or self.xoff else 0, codes=codes, q_scale=p("q_scale") if self.quant else 0,
                     q_zp=p("q_zp") if signed else 0, q_lo=-128 if signed else 0, q_hi=127 if signed else 255,
                     q_form=D.ZP | ROUTE_ONLY | ROUTE_PW_VARIANT)
            if "w_off" in D.BASE[self.entry]:
                a["w_off"] = p("w_off") if self.asym else 0
            if self.xoff:
                a.update(x_off=p("x_off"), x_tap=p("x_tap"))
            return a
        a = dict(g)
        a.update(uns=int(self.uns), out=p("out") if self.out else 0, codes=codes, res=p("res") if self.res else 0, relu=self.act, zp_in=p("zp_in"),
                 bias=p("bias") if self.bias else 0, form=T.FORM_ZEROPOINT | shift,
                 ctl=ROUTE_PW_VARIANT | ((FP32_IN_CHUNK_MAJOR if self.res else 0) | (FP32_OUT_CHUNK_MAJOR if self.out else 0) if self.cm else 0))
        if self.entry == "asym":
            a["w_off"] = p("w_off")
        if real:
            for name in ("x", "w", "wsum", "s_in", "s_w"):
                a[name] = p(name)
            a["q_scale"] = p("q_scale") if self.quant else 0
            if self.entry == "dual":
                a.update({n: p(n) for n in ("x2", "w2", "bias2", "wsum2", "s_in2", "zp_in2", "s_w2")})
        return a

    def ask(self, lib, args):
        """The route query for `args` (route_args)."""
        return decode(D.call(lib, self.entry, args) if self.family == "stem" else T.call(lib, self.entry, args))


# ---- the first layer: N = 3, P Q = 7 x 9 = 63 or 5 x 7 = 35 per image (no multiple of 32: 189 / 105 rows, image seams inside tiles)
def _stem_calls(r, swap, xoff):
    s = {1: 3, 7: 8}.get(r, 1)
    if xoff:            # the buffer carries the padding: the image is Hp - 2 pad
        pad = r // 2
        return [_stem_geo(3, 7 + 2 * pad, 9 + 2 * pad, 64, r, r, 1, 3, pad), _stem_geo(3, 13 + 2 * pad, 17 + 2 * pad, 128, r, r, 2, 4, pad),
                _stem_geo(3, 7 + 2 * pad, 9 + 2 * pad, 72, r, r, 1, 2, pad)]
    return [_stem_geo(3, 6 + r, 8 + s, 64, r, s, 1, 3), _stem_geo(3, 2 * 4 + r, 2 * 6 + r, 128, r, r, 2, 4),
            _stem_geo(3, 6 + r, 8 + r, 128 if swap else 72, r, r, 1, 1 if swap else 2)]


_STEM_INPUT = ((True, 200), (False, None), (True, 77))          # (uint8 codes, zero point) by call
_STEM_OUT = (("plain", True), ("signed", False), (None, True))    # (quantiser, fp32 output) by call, unswapped


def _cases():
    out = []
    for r in STEM_RECORDS:
        _, R, asym, swap, r6, xoff = r
        if r6:
            continue
        entry = "i8_stem_xoff" if xoff else "i8_stem_asym" if asym else "i8_stem_fused"
        for i, geo in enumerate(_stem_calls(R, swap, xoff)):
            uns, zp = (True, 0) if xoff and i != 1 else (False, 0) if xoff else _STEM_INPUT[i]
            quant, want_out = (("plain", "signed", "plain")[i], False) if swap else _STEM_OUT[i]      # (the first-layer entry points take no DLMCQ_EMIT_SHIFT128)
            quant = "plainx" if xoff and quant == "plain" else quant      # (a float offset's outputs are smaller: a finer plain quantiser)
            want_out = want_out or (R == 3 and not swap and not xoff and i == 1)      # (3 x 3, K % 64 == 0, codes alone: the swapped record's)
            geo = dict(geo, C=geo["C"] if asym else 4)
            c = Case(f"{record_name(r)}/{i}", r, entry, geo, uns, zp, act=(1, 0, 1)[i], quant=quant, out=want_out, bias=i != 1)
            out.append(c)
            if i < 2:
                twin = r[:4] + (True,) + r[5:]
                out.append(Case(f"{record_name(twin)}/{i}", twin, entry, geo, uns, zp, act=2, quant=("plain6", "signed6")[i],
                                out=want_out, bias=i != 1, ref=c.cid))
    out.append(Case("stem_r1/loops", ("stem", 1, False, False, False, False), "i8_stem_fused", _stem_geo(None, 64, 64, 8, 1, 1, 1), True, 131, quant="plain", loops="stem"))
    # the pooled first layer: (Hp, Wp) by call - P x Q = 7 x 10 (odd, even), 1 x 9 (P = 1), 6 x 7 (even, odd); K = 64, 24, 64
    for r in POOL_RECORDS:
        R = r[1]
        for i, (p, q, k, stride) in enumerate(((7, 10, 64, 1), (1, 9, 24, 2), (6, 7, 64, 2))):
            geo = _stem_geo(3, (p - 1) * stride + R, (q - 1) * stride + R, k, R, R, stride)
            if R == 7 and i == 2:
                geo = _stem_geo(3, 2 * 6 + 7, 2 * 7 + 8, 64, 7, 8, 2)      # 7 x 8: codes only, stride 2, K = 64, odd P - not the in-register kernel's
            uns, zp = _STEM_INPUT[i]
            out.append(Case(f"{record_name(r)}/{i}", r, "i8_stem_pool_fused", geo, uns, zp, act=(1, 0, 1)[i], quant=("plain", "signed", "plain")[i],
                            out=i == 0, bias=i != 1))
    out.append(Case("pool_r1/loops", ("pool", 1), "i8_stem_pool_fused", _stem_geo(None, 12, 32, 8, 1, 1, 1), True, 131, quant="plain", loops="pool"))
    # conv_stem_pool7_i8_kernel: P x Q = 30 x 64 -> 15 x 32 pooled (two bands, two x tiles: 12 tasks of N = 3), 4 x 6 -> 2 x 3 of N = 2 (2 tasks:
    # half a workgroup), 28 x 62 -> 14 x 31 (exactly one band and one x tile) of N = 5
    for r in POOL7_RECORDS:
        for i, (n, p, q, s) in enumerate(((3, 30, 64, 7), (2, 4, 6, 8), (5, 28, 62, 7))):
            out.append(Case(f"{record_name(r)}/{i}", r, "i8_stem_pool_fused", _stem_geo(n, 2 * (p - 1) + 7, 2 * (q - 1) + s, 64, 7, s, 2), r[1],
                            (200, None, 77)[i] if r[1] else (0, -37, 5)[i], act=(1, 0, 1)[i], quant=("plain", "signed", "plain")[i], bias=i != 1))
    # ---- pointwise: 2 x 46 x 46 = 4232 pixels
    for r in PW_RECORDS:
        _, C, bn, asym, r6 = r
        if r6:
            continue
        ks = (bn, bn, bn) if bn != 128 else (128, 256, 1024 if C <= 192 else 384)
        for i, k in enumerate(ks):
            uns, zp = _STEM_INPUT[i]
            c = Case(f"{record_name(r)}/{i}", r, "asym" if asym else "fused", _pw_geo(2, 46, 46, C, k), uns, zp, act=(1, 0, 1)[i], quant=("plain", "shift", "plain")[i],
                     bias=i != 1)
            out.append(c)
            if i < 2:
                twin = r[:4] + (True,)
                out.append(Case(f"{record_name(twin)}/{i}", twin, c.entry, c.geo, uns, zp, act=2, quant=("plain6", "shift6")[i], bias=i != 1, ref=c.cid))
    out.append(Case("pw_1024_128/loops", ("pw", 1024, 128, False, False), "fused", _pw_geo(None, 16, 16, 1024, 1024), False, None, quant="plain", loops="pw"))
    # ---- block end: 64 x 64 = 4096 pixels, 2 x 48 x 48 = 4608
    for r in PWR_RECORDS[:6]:
        _, C, outf, codes, _, _ = r
        geos = [_pw_geo(1, 64, 64, C, 128), _pw_geo(2, 48, 48, C, 256), _pw_geo(2, 48, 48, C, 128)]
        for i, geo in enumerate(geos):
            uns, zp = _STEM_INPUT[i]
            out.append(Case(f"{record_name(r)}/{i}", r, "fused", geo, uns, zp, quant=("plain", "shift", "plain")[i] if codes else None, out=outf, bias=i != 1,
                            res=True, cm=i == 1))
    out.append(Case("pwr_256_codes/k4096", ("pwr", 256, False, True, False, False), "fused", _pw_geo(1, 64, 64, 256, 4096), True, 77, quant="plain", res=True))
    out.append(Case("pwr_512_codes/loops", ("pwr", 512, False, True, False, False), "fused", _pw_geo(None, 16, 16, 512, 1024), False, None, quant="plain", res=True,
                    loops="pwr"))
    # the dual form: the 256-deep pair row by row on P x Q, the 512-deep one sampled at stride 1 / 2 / 2 from (P, Q) s-times as large
    for r in PWR_RECORDS[6:]:
        swp = r[5]
        for i, (n, p, q, s, k) in enumerate(((1, 64, 64, 1, 128), (2, 48, 48, 2, 256), (2, 48, 48, 2, 128))):
            dense, sampled = dict(H=p, W=q, C=256, stride=1), dict(H=s * p - (s - 1), W=s * q - (s - 1), C=512, stride=s)
            first, second = (sampled, dense) if swp else (dense, sampled)
            geo = dict(_pw_geo(n, first["H"], first["W"], first["C"], k), stride=first["stride"], H2=second["H"], W2=second["W"], C2=second["C"], R2=1, S2=1,
                       stride2=second["stride"], pad2=0, dil2=1, uns2=int(i != 1))
            out.append(Case(f"{record_name(r)}/{i}", r, "dual", geo, i != 0, None, quant=("plain", "shift", "plain")[i], out=True, bias=i != 1, cm=i == 1))
    return out


CASES = _cases()
BY_RECORD = {r: [c for c in CASES if c.record == r] for r in RECORDS}
BY_ID = {c.cid: c for c in CASES}

# ---- the fallbacks: (a case, what is changed, the record the changed call must answer)
FALLBACKS = [
    ("stem_r3_swap/0", dict(codes_off=4), ("stem", 3, False, False, False, False)),              # SWAP needs 16-byte-aligned codes
    ("stem_r3_asym_swap/0", dict(codes_off=4), ("stem", 3, True, False, False, False)),
    ("stem_r3_xoff/0", dict(pad0=True), ("stem", 3, False, False, False, False)),                # pad = 0: no border, the plain record
    ("stem_r7_asym_xoff/0", dict(pad0=True), ("stem", 7, True, False, False, False)),
    ("pool7/0", dict(codes_off=4), ("pool", 7)), ("pool7_xs/0", dict(x_off=4), ("pool", 7)),     # the in-register kernel needs both aligned
]
