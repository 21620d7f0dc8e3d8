"""The calls that reach every instantiation of conv_chain_i8_kernel (csrc/conv_chain_i8.hip: CHAIN_TABLE - the recomputing row in the first
epilogue's forms FL = 3 / 1, seven rows in FL = 3 / 1 / -1: 23 kernels) through its three entry points: ONE table for
tests/test_chain_variants_host.py (which instantiation, tile height and layouts does the launcher pick: DLMCQ_ROUTE_ONLY |
DLMCQ_ROUTE_CHAIN_VARIANT on placeholder pointers, no GPU; the reference's conditions) and tests/test_gpu_chain_variants.py (the same calls
launched and compared with an exact float64 reference).  TEST INFRASTRUCTURE ONLY.

A record is (table row, FL); a call's expected answer is ("chain", row, FL, rows per tile, icm, ocm) as dlmc._native.decode_chain_variant
gives it.  Every record has three calls.  Shapes are the smallest at which the kernel can go wrong: N = 2, 9 x 7 pixels (M = 126: two 64-row
tiles with the last one partial, three 56- or 49-row tiles; a tile spans the image seam), one call per table row with M = 35 (five images of
1 x 7: less than one tile), and block widths KD of 64 (one chunk: the prologue's request is the last), 192 (three: the double buffer wraps on
an odd count) and 256 (four) - each record sees all three.  Over a row's calls, by a running index so that no two dimensions move together:
  * the tile height `rows_per_tile` 0 (-> 64 at these sizes), 64, 56, 49; W3 as KRSC and DLMCQ_W2_CHUNK_MAJOR;
  * the fp32 layouts: row-major, both chunk-major, one of each in both directions (the 128 -> K -> 128 row keeps both in one: its mixed
    calls are in REFUSED_MIXED); the multi-operand forms have one fp32 tensor, whose layout is the output bit's;
  * the outputs: FL = 3 has the fp32 output, FL = 1 has none, both with and without the first codes; FL = -1 walks all four combinations,
    "neither" included (only the second codes are written);
  * the FL slot on purpose (chain_launch: ReLU and two quantisers with the unsigned byte range and no zero-point tensor -> 3 with an fp32
    output, 1 without; anything else -1): FL = 3 / 1 calls use the plain quantisers at scale 1/4 and 2^-5 (the upper clamp) and, for the
    second one, their DLMCQ_EMIT_SHIFT128 forms - which keep the compile-time form: the emission is an XOR behind the same pack; FL = -1 is
    reached by relu = 0 (first quantiser with zero point 100: negative values have codes), by a first quantiser with a zero-point tensor,
    and by a second quantiser with a signed range (or a zero-point tensor);
  * the inputs: uint8 codes with a zero point above / below 128 and int8 codes with zero point -37, on every operand in turn; a null
    bias on each operand and on the second layer in turn;
  * the sampled operand (dual, recomputing): stride 2 - from 18 x 13: the last row is skipped, the last column read - and stride 1; the
    recomputed block's own ReLU on and off;
  * one call per entry point places an input the kernel addresses through a buffer descriptor or reads by LDS-DMA, and the fp32 output
    where there is one, at addresses whose low 32 bits have bit 31 set (`high`).
`auto_rule_cases` holds the query-only calls of the 56-row rule, sized to trip it."""
from dataclasses import dataclass
from typing import Optional

import test_chain_refusals_host as R

from dlmc._native import (FP32_IN_CHUNK_MAJOR, FP32_OUT_CHUNK_MAJOR, ROUTE_CHAIN_VARIANT, ROUTE_ONLY, W2_CHUNK_MAJOR, decode_chain_variant)

# THE table, by hand: (C1, KB, C2, CA, CB, FL forms) in the launcher's order (dlmcq_x_chain_variant_table must list exactly this)
ROWS = [
    (64, 64, 0, 64, 64, (3, 1)),
    (64, 64, 0, 0, 0, (3, 1, -1)), (64, 128, 0, 0, 0, (3, 1, -1)), (128, 128, 0, 0, 0, (3, 1, -1)), (128, 256, 0, 0, 0, (3, 1, -1)),
    (256, 256, 0, 0, 0, (3, 1, -1)),
    (64, 64, 64, 0, 0, (3, 1, -1)), (128, 128, 256, 0, 0, (3, 1, -1)),
]
RECORDS = [(ri, fl) for ri, row in enumerate(ROWS) for fl in row[5]]
assert len(RECORDS) == len(set(RECORDS)) == 23
ONE_LAYOUT_ROWS = {3}              # the 128 -> K -> 128 row: no registers for two sets of fp32 offsets


def entry_of(ri):
    c1, kb, c2, ca, cb, _ = ROWS[ri]
    return "recompute_chain" if ca else "dual_chain" if c2 else "chain"


def chain_wgs(ri):
    """Workgroups per CU the row's kernels are compiled for (csrc/conv_chain_i8.hip: CHAIN_WGS): the 56-row rule's `slots` is 256 of these."""
    c1, kb, c2, ca, cb, _ = ROWS[ri]
    return 3 if c1 + c2 + ca + cb + kb <= 256 else 2


def record_name(r):
    c1, kb, c2, ca, cb, _ = ROWS[r[0]]
    mid = f"_a{ca}_b{cb}" if ca else f"_s{c2}" if c2 else ""
    return f"{entry_of(r[0])}_{c1}{mid}_{kb}_fl{'x' if r[1] < 0 else r[1]}"


def decode(rc):
    """A ROUTE_ONLY | ROUTE_CHAIN_VARIANT answer -> ("chain", row, FL, rows per tile, icm, ocm), or the integer itself when it is none."""
    r = decode_chain_variant(rc)
    return rc if r is None else r


# the first quantiser: always 0 .. 255 (GEMM 2 reads the codes as uint8); name -> (scale, zero point or None)
Q1 = {"p025": (0.25, None), "p2m5": (2.0 ** -5, None), "zp16": (0.25, 16.0), "zp100": (0.5, 100.0)}
INPUTS = ((True, "high"), (True, "low"), (False, None))        # (uint8 codes, side of 128 the zero point lies on); int8: zero point -37
SIGNED_ZP = -37
LAYOUTS = ((False, False), (True, True), (True, False), (False, True))      # (shortcut, output) chunk-major
OUTPUTS = ((True, True), (False, True), (True, False), (False, False))      # FL = -1: (fp32 output, first codes)


@dataclass(frozen=True)
class Case:
    cid: str
    record: tuple                 # (table row, FL)
    geo: tuple                    # (N, H, W)
    kd: int                       # the block width
    rpt: int                      # rows_per_tile as passed
    w3cm: bool
    in_cm: bool                   # DLMCQ_FP32_IN_CHUNK_MAJOR is passed (the plain form's shortcut)
    out_cm: bool                  # DLMCQ_FP32_OUT_CHUNK_MAJOR is passed
    out: bool
    codes: bool
    relu: int
    q1: str                       # Q1
    q2: str                       # tests/test_gpu_halo_variants.py: QUANTS
    relu2: int
    inputs: tuple                 # index into INPUTS for the own, sampled and unit operands
    null_bias: Optional[str]      # "own" / "sampled" / "unit" / "second": that bias is null
    stride: int = 1               # of the sampled operand
    relu_sc: int = 1
    high: tuple = ()              # tensors placed at addresses with bit 31 of the low half set
    seed: int = 0

    @property
    def row(self):
        return ROWS[self.record[0]]

    @property
    def entry(self):
        return entry_of(self.record[0])

    @property
    def m(self):
        return self.geo[0] * self.geo[1] * self.geo[2]

    def sampled_hw(self):
        n, h, w = self.geo
        return (h, w) if self.stride == 1 else (2 * h, 2 * w - 1)      # the last row skipped; the last column read

    def layouts(self):
        """(icm, ocm) as chain_launch resolves them: a call with one fp32 tensor has one layout."""
        icm = self.in_cm if self.entry == "chain" else self.out_cm
        return icm, (self.out_cm if self.out else icm)

    def expected(self):
        return ("chain", self.record[0], self.record[1], self.rpt or 64, *self.layouts())      # (the automatic rule: 64 at these sizes)

    def call_args(self, ptr=None):
        """Overrides of R.BASE for the launch (`ptr` maps an argument name to a real address; placeholders otherwise)."""
        p = (lambda name: R.P) if ptr is None else ptr
        c1, kb, c2, ca, cb, _ = self.row
        n, h, w = self.geo
        a = dict(N=n, H=h, W=w, C=c1, K=self.kd, K2=kb, rpt=self.rpt, relu=self.relu, relu2=self.relu2, relu_sc=self.relu_sc)
        for i, (sfx, on) in enumerate((("", True), ("b", self.entry != "chain"), ("a", self.entry == "recompute_chain"))):
            if on:
                a.update({"x" + sfx: p("x" + sfx), "w" + sfx: p("w" + sfx), "wsum" + sfx: p("wsum" + sfx), "s_in" + sfx: p("s_in" + sfx),
                          "zp_in" + sfx: p("zp_in" + sfx), "s_w" + sfx: p("s_w" + sfx), "uns" + sfx: int(INPUTS[self.inputs[i]][0]),
                          "bias" + sfx: 0 if self.null_bias == ("own", "sampled", "unit")[i] else p("bias" + sfx)})
        if self.entry == "chain":
            a["res"] = p("res")
        else:
            hb, wb = self.sampled_hw()
            a.update(Hb=hb, Wb=wb, Cb=c2 or cb, strideb=self.stride, Ca=ca or 64)
        zp1 = Q1[self.q1][1]
        a.update(out=p("out") if self.out else 0, codes=p("codes") if self.codes else 0, q_scale=p("q_scale"), q_zp=p("q_zp") if zp1 is not None else 0,
                 q_lo=0, q_hi=255, q_form=R.ZP)
        form2 = R.ZP | (W2_CHUNK_MAJOR if self.w3cm else 0) | (FP32_IN_CHUNK_MAJOR if self.in_cm else 0) | (FP32_OUT_CHUNK_MAJOR if self.out_cm else 0)
        a.update(w2=p("w2"), wsum2=p("wsum2"), s_w2=p("s_w2"), bias2=0 if self.null_bias == "second" else p("bias2"), codes2=p("codes2"),
                 q2_scale=p("q2_scale"), q2_zp=0, q2_lo=0, q2_hi=255, q2_form=form2)
        if self.q2.startswith("signed"):
            a.update(q2_zp=p("q2_zp"), q2_lo=-128, q2_hi=127)
        elif self.q2.startswith("uzp"):
            a.update(q2_zp=p("q2_zp"))
        elif self.q2.startswith("shift"):
            a["q2_form"] |= R.SHIFT128
        return a

    def route_args(self, ptr=None):
        """The query form of the very same arguments: nothing can launch."""
        a = self.call_args(ptr)
        a["q2_form"] |= ROUTE_ONLY | ROUTE_CHAIN_VARIANT
        return a


def cases():
    out = []
    g = 0                                     # the running index of the calls
    for ri, row in enumerate(ROWS):
        entry = entry_of(ri)
        multi = entry != "chain"
        nulls = {"chain": (None, "own", None, "second"), "dual_chain": (None, "own", "sampled", "second"),
                 "recompute_chain": (None, "own", "sampled", "unit", "second")}[entry]
        with_out = 0
        for fi, fl in enumerate(row[5]):
            for i in range(3):
                small = i == 2 and fi == ri % len(row[5])                 # one call per row with less than one tile
                if fl >= 0:
                    want_out, want_codes = fl == 3, bool((i + fi) % 2)
                    relu, q1 = 1, ("p2m5", "p025", "p2m5")[i]
                    q2 = (("plain_hi", "shift", "plain"), ("shift_hi", "plain", "plain_hi"))[(ri + fi) % 2][i]
                else:
                    want_out, want_codes = OUTPUTS[g % 4]
                    relu, q1 = ((0, "zp100"), (1, "zp16"), (1, "p2m5"))[i]
                    q2 = ("plain_hi", ("uzp_hi", "shift_hi")[ri % 2], ("signed_hi", "signed")[ri % 2])[i]
                in_cm, out_cm = LAYOUTS[(with_out if want_out else g) % 4]      # (a row's calls with two fp32 tensors walk all four)
                with_out += want_out
                if multi:
                    in_cm = False                                        # (no shortcut tensor: the input bit says nothing)
                if ri in ONE_LAYOUT_ROWS and want_out and in_cm != out_cm:
                    in_cm = out_cm = bool(g % 2)
                high = ()
                if i == 0 and fi == 0 and ri in (0, 1, 6):                # one call per entry point
                    high = (("res",) if entry == "chain" else ("xb",)) + ("out",)
                out.append(Case(f"{record_name((ri, fl))}/{i}", (ri, fl), (5, 1, 7) if small else (2, 9, 7), (64, 192, 256)[(i + ri) % 3],
                                (0, 64, 56, 49)[g % 4], bool(g % 2), in_cm, out_cm, want_out, want_codes, relu, q1, q2, 0 if g % 5 == 0 else 1,
                                (g % 3, (g + 1) % 3, (g + 2) % 3), nulls[g % len(nulls)], stride=(2, 1, 2)[i] if multi else 1, relu_sc=g % 2,
                                high=high, seed=9900 + g))
                g += 1
    return out


CASES = cases()
BY_RECORD = {r: [c for c in CASES if c.record == r] for r in RECORDS}

# the 128 -> K -> 128 row with its two fp32 tensors in different layouts: DLMCQ_EINVAL, query or launch
REFUSED_MIXED = [dict(C=128, K=192, K2=128, N=2, H=9, W=7, q2_form=R.ZP | bits | ROUTE_ONLY | ROUTE_CHAIN_VARIANT)
                 for bits in (FP32_IN_CHUNK_MAJOR, FP32_OUT_CHUNK_MAJOR)]


def auto_rule_cases():
    """[(id, entry, overrides of R.BASE, rows per tile the rule picks)]: chain_launch's automatic tile height - with t64 = ceil(M / 64) tiles,
    slots = 256 x CHAIN_WGS workgroup slots, full = t64 // slots rounds and left = t64 % slots tiles in the last one, 56 rows when
    2 <= full <= 4 and 0 < left and left * 8 < slots, else 64 - derived from that rule for one row of either CHAIN_WGS class: M values that
    select 56 and their neighbours that do not (full = 1 and 5, left = 0, left * 8 == slots).  KD = 64 keeps M * KD * 4 below the offset bound;
    the last tile is partial (M = 64 t64 - 13)."""
    out = []
    for ri in (1, 5, 0, 7):                   # 64 -> 64 (3 workgroups per CU), 256 -> 256 (2), the recomputing row (3), the wide dual row (2)
        c1, kb, c2, ca, cb, _ = ROWS[ri]
        slots = 256 * chain_wgs(ri)
        entry = entry_of(ri)
        for full, left, want in ((2, 1, 56), (4, slots // 8 - 1, 56), (3, slots // 16, 56), (1, 1, 64), (5, 1, 64), (2, 0, 64), (4, 0, 64),
                                 (2, slots // 8, 64), (4, slots // 8, 64), (3, slots - 1, 64)):
            m = 64 * (full * slots + left) - 13
            kw = dict(C=c1, K=64, K2=kb, N=m, H=1, W=1, Hb=1, Wb=1, Cb=c2 or cb or 64, Ca=ca or 64,
                      q2_form=R.ZP | ROUTE_ONLY | ROUTE_CHAIN_VARIANT)
            out.append((f"{record_name((ri, 3))}/full{full}_left{left}", entry, kw, want))
            for rpt in (56, 49, 1):           # an explicit height is passed through
                if (full, left) == (2, 1):
                    out.append((f"{record_name((ri, 3))}/full{full}_left{left}/rpt{rpt}", entry, dict(kw, rpt=rpt), rpt))
    return out
